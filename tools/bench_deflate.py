#!/usr/bin/env python3
"""ukm_deflate: the device's Huffman-only deflate beside zlib on the same bytes, and the driver's compressed output end to end.

    python tools/bench_deflate.py [--records 100000000] [--e2e-records 100000000] [--parent-bin PATH/unikmer]
                                  [--zlib-sample-mb 64] [--tmp DIR] [--out profiles/deflate.json]

Bodies: the three shapes of tools/bench_codec.py (sorted random 31-mers, dense sorted 15-mers, sorted random 31-mers with
4-byte taxids), encoded on the device.  Per body, on device tensors: ukm_deflate timed with the context's own event timer
(ukm_last_call_ms: all device work of the call, the two read-backs between the passes included), median of --steps calls
behind --warmup calls; GB/s of input; the share of a device-to-device copy of the same bytes timed in the same run; the
compressed size; the bytes the dynamic block header takes per chunk (parsed from the fragments of the first 64 chunks, each
deflated alone); and, on the first --zlib-sample-mb of the same body
(a whole number of chunks; the ratio of these bodies does not depend on the position), the host's zlib at level 6 and with
Z_HUFFMAN_ONLY: ratio and MB/s of one thread, and the device's ratio on exactly those bytes.  The device's output is inflated
by zlib and compared with the input on that sample.

End to end: `unikmer union a.unik b.unik -o out` (compressed output, uncompressed inputs) on two files of --e2e-records sorted
random 31-mers each, wall time of --e2e-runs (5) runs: this build with UNIKMER_DEVICE_GZIP=1, with UNIKMER_HOST_GZIP=1, and --parent-bin
(the parent commit's driver) when given; the three outputs must inflate to the same bytes.
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
CHUNK = 32768  # DFL_CHUNK of unikmer_amd/csrc/ukm_deflate.hip


def inflated_crc(path):
    """(CRC-32, length) of what a gzip file inflates to, streamed"""
    d, crc, n = zlib.decompressobj(31), 0, 0
    with open(path, "rb") as f:
        while True:
            b = f.read(1 << 24)
            if not b:
                break
            o = d.decompress(b)
            crc, n = zlib.crc32(o, crc), n + len(o)
    assert d.eof
    return crc, n


def header_bits(frag):
    """bits of the dynamic block header a fragment starts with (RFC 1951 3.2.7), None for a stored block"""
    pos = 0

    def take(n):
        nonlocal pos
        v = 0
        for i in range(n):
            v |= ((frag[(pos + i) >> 3] >> ((pos + i) & 7)) & 1) << i
        pos += n
        return v
    take(1)
    if take(2) != 2:
        return None
    hlit, hdist, hclen = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for i in range(hclen):
        cl[(16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)[i]] = take(3)
    code, table = 0, {}
    for bits in range(1, 8):
        for sym in range(19):
            if cl[sym] == bits:
                table[(bits, code)] = sym
                code += 1
        code <<= 1
    got = 0
    while got < hlit + hdist:
        c, bits = 0, 0
        while (bits, c) not in table:
            c, bits = (c << 1) | take(1), bits + 1
        sym = table[(bits, c)]
        got += 1 if sym < 16 else (take(2) + 3 if sym == 16 else (take(3) + 3 if sym == 17 else take(7) + 11))
    assert got == hlit + hdist
    return pos


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--e2e-records", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--zlib-sample-mb", type=int, default=64)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--e2e-only", default=None, help="comma-separated subset of device_gzip,host_gzip,parent")
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deflate.json"))
    a = ap.parse_args()
    assert a.steps >= 5

    import torch
    from unikmer_amd import lib, unikfile
    if not torch.cuda.is_available():
        raise SystemExit("bench_deflate.py needs the GPU")
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20241019)
    tmp = tempfile.mkdtemp(prefix="bench_deflate_", dir=a.tmp)
    S, T = lib.UNIK_SORTED, lib.UNIK_INCLUDE_TAXID

    def sorted_codes(n, bits):
        return torch.sort(torch.randint(0, 1 << bits, (n,), device=dev, generator=gen, dtype=torch.int64)).values

    def copy_ms(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        ts = []
        for i in range(a.warmup + a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    def host_zlib(raw, **kw):
        z = zlib.compressobj(6, zlib.DEFLATED, -15, 8, **kw)
        t0 = time.perf_counter()
        n = len(z.compress(raw)) + len(z.flush())
        dt = time.perf_counter() - t0
        return {"ratio": n / len(raw), "MBps": len(raw) / dt / 1e6}

    rows = []
    n = a.records
    for name, k, bits, tb in () if n <= 0 else (("sorted random 31-mers", 31, 62, 0), ("dense sorted 15-mers", 15, 30, 0), ("sorted random 31-mers, 4-byte taxids", 31, 62, 4)):
        keys = sorted_codes(n, bits)
        tax = torch.randint(1, 1 << 31, (n,), device=dev, generator=gen, dtype=torch.int32) if tb else None
        flags = S | (T if tb else 0)
        body = ctx.unik_encode(keys, k, flags, taxids=tax, taxid_bytes=tb).clone()
        del keys, tax
        torch.cuda.empty_cache()
        nb = body.numel()
        out = torch.empty(lib.deflate_bound(nb, final=True), dtype=torch.uint8, device=dev)
        call, scan = [], []
        for i in range(a.warmup + a.steps):
            frag, crc = ctx.deflate(body, final=True, out=out)
            if i >= a.warmup:
                call.append(ctx.last_call_ms())
                scan.append(ctx.last_kernel_ms())
        ms = statistics.median(call)
        cms = copy_ms(nb)
        nchunks = (nb + CHUNK - 1) // CHUNK
        sample = min(nb, (a.zlib_sample_mb << 20) // CHUNK * CHUNK)
        raw = body[:sample].cpu().numpy().tobytes()
        sfrag, scrc = ctx.deflate(body[:sample], final=True)
        sfrag = sfrag.cpu().numpy().tobytes()
        assert zlib.decompressobj(-15).decompress(sfrag) == raw and scrc == zlib.crc32(raw), "the device's fragment does not inflate to its input"
        hb = [header_bits(ctx.deflate(body[i * CHUNK: (i + 1) * CHUNK])[0].cpu().numpy().tobytes()) for i in range(min(64, nb // CHUNK))]
        hb = [h for h in hb if h is not None]
        row = {"shape": name, "n": n, "body_bytes": nb, "bytes_per_record": nb / n, "chunks": nchunks,
               "deflate_call_ms": ms, "deflate_call_ms_min": min(call), "deflate_call_ms_max": max(call), "between_passes_ms": statistics.median(scan),
               "deflate_GBps_in": nb / ms / 1e6, "copy_ms": cms, "copy_GBps": nb / cms / 1e6, "frac_of_copy": cms / ms,
               "out_bytes": int(frag.numel()), "ratio": frag.numel() / nb,
               "header_bytes_per_chunk": (statistics.mean(hb) / 8 if hb else None), "dynamic_chunks_of_64": len(hb),
               "sample_bytes": sample, "sample_ratio_device": len(sfrag) / sample,
               "host_zlib_level6": host_zlib(raw), "host_zlib_huffman_only": host_zlib(raw, strategy=zlib.Z_HUFFMAN_ONLY)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del body, out, frag
        torch.cuda.empty_cache()

    e2e = []
    m = a.e2e_records
    if m > 0:
        paths = []
        for i in range(2):
            keys = sorted_codes(m, 62)
            p = os.path.join(tmp, "in%d.unik" % i)
            unikfile.save(ctx, p, {"k": 31, "flag": S | 2}, keys, compress=False)
            paths.append(p)
            del keys
            torch.cuda.empty_cache()
        ctx.trim()
        sums = {}
        for label, exe, env in (("device_gzip", BIN, {"UNIKMER_DEVICE_GZIP": "1"}), ("host_gzip", BIN, {"UNIKMER_HOST_GZIP": "1"}),
                                ("parent", a.parent_bin, {})):
            if exe is None or (a.e2e_only and label not in a.e2e_only.split(",")):
                continue
            env_all = {k: v for k, v in os.environ.items() if k not in ("UNIKMER_DEVICE_GZIP", "UNIKMER_HOST_GZIP")}
            env_all.update(env)
            out = os.path.join(tmp, "out_" + label)
            ts = []
            for _ in range(a.e2e_runs):
                t0 = time.perf_counter()
                subprocess.check_call([exe, "union", paths[0], paths[1], "-o", out], env=env_all, stderr=subprocess.DEVNULL)
                ts.append(time.perf_counter() - t0)
                print("# %s: %.2f s" % (label, ts[-1]), flush=True)   # (a host-gzip run takes a minute: show that it is alive)
            sums[label] = inflated_crc(out + ".unik")
            e2e.append({"command": "union a.unik b.unik -o out", "records_per_file": m, "inputs": "uncompressed", "output": "gzip",
                        "binary": label, "out_file_bytes": os.path.getsize(out + ".unik"), "out_inflated_bytes": sums[label][1],
                        "wall_s_median": statistics.median(ts), "wall_s_min": min(ts), "wall_s_max": max(ts), "wall_s": ts})
            print(json.dumps(e2e[-1]), flush=True)
            os.remove(out + ".unik")
        assert len(set(sums.values())) == 1, "the outputs inflate to different bytes: %r" % sums

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    doc = {"tool": "tools/bench_deflate.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "chunk_bytes": CHUNK, "rows": rows, "end_to_end": e2e}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    shutil.rmtree(tmp, ignore_errors=True)
    ctx.close()


if __name__ == "__main__":
    main()
