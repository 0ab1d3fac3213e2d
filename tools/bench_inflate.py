#!/usr/bin/env python3
"""ukm_inflate: the device's inflate of ukm_deflate's fragments beside zlib on the same bytes, and the driver's gzip inputs
end to end.

    python tools/bench_inflate.py [--records 100000000] [--e2e-records 100000000] [--parent-bin PATH/unikmer]
                                  [--zlib-sample-mb 64] [--tmp DIR] [--out profiles/inflate.json]

Bodies: the three shapes of tools/bench_deflate.py (sorted random 31-mers, dense sorted 15-mers, sorted random 31-mers with
4-byte taxids), encoded and deflated on the device.  Per body, on device tensors: ukm_inflate of the whole fragment into a
buffer of the exact size, timed with the context's own event timer (ukm_last_call_ms), median of --steps calls behind --warmup
calls; GB/s of output; a device-to-device copy of the output bytes timed in the same run; the split of the call -- the size
side (candidates, the walk of every candidate, the chain: a size query's ukm_last_call_ms less its scan step), the scan step
(ukm_last_kernel_ms) and the write side (the rest), of which the second walk over the chain (statistic "inflate_cp_walk_us")
and the write pass behind it --; the candidates against the segments on the chain (statistics
"inflate_candidates" / "inflate_segments"); and the GPU host's zlib, one thread, raw inflate of the fragment of the first
--zlib-sample-mb of the same body.  The output is compared with the body, the CRC with ukm_deflate's.

End to end: `unikmer union a.unik b.unik -C -o out` on two device-gzipped files of --e2e-records sorted random 31-mers each,
wall time of --e2e-runs (5) runs: this build with UNIKMER_DEVICE_GUNZIP=1, with UNIKMER_HOST_GUNZIP=1, and --parent-bin (the
parent commit's driver) when given; the outputs must be the same bytes.
"""
import argparse
import hashlib
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
SWITCHES = ("UNIKMER_DEVICE_GZIP", "UNIKMER_HOST_GZIP", "UNIKMER_DEVICE_GUNZIP", "UNIKMER_HOST_GUNZIP", "UNIKMER_GUNZIP_REPORT")


def file_digest(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for b in iter(lambda: f.read(1 << 24), b""):
            h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--e2e-records", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--zlib-sample-mb", type=int, default=64)
    ap.add_argument("--e2e-runs", type=int, default=5)
    ap.add_argument("--e2e-only", default=None, help="comma-separated subset of device_gunzip,host_gunzip,parent")
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inflate.json"))
    a = ap.parse_args()
    assert a.steps >= 5

    import torch
    from unikmer_amd import lib, unikfile
    if not torch.cuda.is_available():
        raise SystemExit("bench_inflate.py needs the GPU")
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20241019)
    tmp = tempfile.mkdtemp(prefix="bench_inflate_", dir=a.tmp)
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

    def host_inflate(frag, expect):
        d = zlib.decompressobj(-15)
        t0 = time.perf_counter()
        n = len(d.decompress(frag))
        dt = time.perf_counter() - t0
        assert n == expect and d.eof
        return {"in_bytes": len(frag), "out_bytes": n, "ms": dt * 1e3, "MBps_out": n / dt / 1e6}

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
        frag, crc = ctx.deflate(body)
        frag = frag.clone()
        nf = frag.numel()
        out = torch.empty(nb, dtype=torch.uint8, device=dev)
        call, scan, query, walk2 = [], [], [], []
        for i in range(a.warmup + a.steps):
            got, consumed, c = ctx.inflate(frag, out=out)
            t_call, t_scan, t_walk2 = ctx.last_call_ms(), ctx.last_kernel_ms(), ctx.stat("inflate_cp_walk_us") / 1e3
            try:
                ctx.inflate(frag, out=out[:0])          # capacity 0: ends behind the scan
                raise AssertionError("a size query of a body must fail for capacity")
            except lib.CapacityError as e:
                assert e.needed == nb
            t_query = ctx.last_call_ms()
            if i >= a.warmup:
                call.append(t_call)
                scan.append(t_scan)
                query.append(t_query)
                walk2.append(t_walk2)
        assert consumed == nf and c == crc and got.numel() == nb and torch.equal(got, body), "the device's output is not the body"
        ms, sms, qms = statistics.median(call), statistics.median(scan), statistics.median(query)
        cms = copy_ms(nb)
        sample = min(nb, (a.zlib_sample_mb << 20) // CHUNK * CHUNK)
        sfrag, _ = ctx.deflate(body[:sample], final=True)
        row = {"shape": name, "n": n, "body_bytes": nb, "fragment_bytes": nf, "ratio": nf / nb,
               "inflate_call_ms": ms, "inflate_call_ms_min": min(call), "inflate_call_ms_max": max(call),
               "inflate_GBps_out": nb / ms / 1e6, "inflate_GBps_in": nf / ms / 1e6,
               "size_side_ms": qms - sms, "scan_step_ms": sms, "write_side_ms": ms - qms,
               "second_walk_ms": statistics.median(walk2), "write_pass_ms": ms - qms - statistics.median(walk2),
               "candidates": ctx.stat("inflate_candidates"), "chain_segments": ctx.stat("inflate_segments"),
               "copy_ms": cms, "copy_GBps": nb / cms / 1e6, "frac_of_copy": cms / ms,
               "host_zlib_inflate": host_inflate(sfrag.cpu().numpy().tobytes(), sample)}
        row["speedup_over_host_zlib"] = row["inflate_GBps_out"] * 1e3 / row["host_zlib_inflate"]["MBps_out"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del body, out, frag, got, sfrag
        torch.cuda.empty_cache()

    e2e = []
    m = a.e2e_records
    if m > 0:
        paths = []
        for i in range(2):
            keys = sorted_codes(m, 62)
            p = os.path.join(tmp, "in%d.unik" % i)
            unikfile.save(ctx, p, {"k": 31, "flag": S | 2}, keys, deflate="device")
            paths.append(p)
            del keys
            torch.cuda.empty_cache()
        ctx.trim()
        sums = {}
        for label, exe, env in (("device_gunzip", BIN, {"UNIKMER_DEVICE_GUNZIP": "1"}), ("host_gunzip", BIN, {"UNIKMER_HOST_GUNZIP": "1"}),
                                ("parent", a.parent_bin, {})):
            if exe is None or (a.e2e_only and label not in a.e2e_only.split(",")):
                continue
            env_all = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            env_all.update(env)
            out = os.path.join(tmp, "out_" + label)
            ts = []
            for _ in range(a.e2e_runs):
                t0 = time.perf_counter()
                subprocess.check_call([exe, "union", paths[0], paths[1], "-C", "-o", out], env=env_all, stderr=subprocess.DEVNULL)
                ts.append(time.perf_counter() - t0)
                print("# %s: %.2f s" % (label, ts[-1]), flush=True)
            sums[label] = file_digest(out + ".unik")
            e2e.append({"command": "union a.unik b.unik -C -o out", "records_per_file": m, "inputs": "device gzip", "output": "uncompressed",
                        "binary": label, "in_file_bytes": [os.path.getsize(p) for p in paths], "out_file_bytes": os.path.getsize(out + ".unik"),
                        "wall_s_median": statistics.median(ts), "wall_s_min": min(ts), "wall_s_max": max(ts), "wall_s": ts})
            print(json.dumps(e2e[-1]), flush=True)
            os.remove(out + ".unik")
        assert len(set(sums.values())) == 1, "the outputs differ: %r" % sums

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    doc = {"tool": "tools/bench_inflate.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "chunk_bytes": CHUNK, "rows": rows, "end_to_end": e2e}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    shutil.rmtree(tmp, ignore_errors=True)
    ctx.close()


if __name__ == "__main__":
    main()
