#!/usr/bin/env python3
"""ukm_unik_decode / ukm_unik_encode: the device codec, the host codec of unik.hpp beside it, and the driver end to end.

    python tools/bench_codec.py [--records 100000000] [--e2e-records 100000000] [--parent-bin PATH/unikmer]
                                [--tmp DIR] [--out profiles/unik_codec.json]

Shapes: sorted random 31-mers (5-6 byte deltas), dense sorted k = 15 codes (1-byte deltas, duplicates), the first with 4-byte
taxids.  Per shape, on device tensors: decode and encode timed with the context's own event timer (ukm_last_call_ms: all
device work of the call), median of --steps calls behind --warmup calls; the scan stage alone (ukm_last_kernel_ms); the
body's size; and the rate of body + arrays against a device-to-device copy that moves the same number of bytes, timed in
the same run with torch events.

Host codec: the same body as an uncompressed file in the page cache, read by unik::Reader::read_all and written by the
Writer's record loop (tools/codec_host_timer.cpp, built here with g++ -O2), median of 3.

End to end: `unikmer union a.unik b.unik -C -o out` on two files of --e2e-records sorted random 31-mers each, uncompressed
and gzip inputs, median wall time of 5 runs: this build with UNIKMER_DEVICE_CODEC=1, this build with UNIKMER_HOST_CODEC=1,
and --parent-bin (the parent commit's driver, built beside its own library) when given.
"""
import argparse
import gzip
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--e2e-records", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unik_codec.json"))
    a = ap.parse_args()
    assert a.steps >= 5

    import numpy as np
    import torch
    from unikmer_amd import lib, unikfile
    if not torch.cuda.is_available():
        raise SystemExit("bench_codec.py needs the GPU")
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20241019)
    tmp = tempfile.mkdtemp(prefix="bench_codec_", dir=a.tmp)
    S, T = lib.UNIK_SORTED, lib.UNIK_INCLUDE_TAXID

    def sorted_codes(n, bits):
        return torch.sort(torch.randint(0, 1 << bits, (n,), device=dev, generator=gen, dtype=torch.int64)).values

    def timed(fn):
        for _ in range(a.warmup):
            r = fn()
        call, scan = [], []
        for _ in range(a.steps):
            r = fn()
            call.append(ctx.last_call_ms())
            scan.append(ctx.last_kernel_ms())
        return {"call_ms": statistics.median(call), "call_ms_min": min(call), "scan_ms": statistics.median(scan)}, r

    def copy_ms(nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
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

    timer = os.path.join(tmp, "codec_host_timer")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "unikmer_amd", "host"),
                           os.path.join(ROOT, "tools", "codec_host_timer.cpp"), "-o", timer, "-lz"])

    def write_file(path, k, flags, tb, body, n, gz=False):
        h = unikfile.header_bytes({"k": k, "flag": flags | 2, "taxid_bytes": tb or 4, "number": n})
        with (gzip.open(path, "wb", compresslevel=1) if gz else open(path, "wb")) as f:
            f.write(h)
            f.write(body.cpu().numpy().tobytes())

    rows = []
    n = a.records
    for name, k, bits, tb in (("sorted random 31-mers", 31, 62, 0), ("dense sorted 15-mers", 15, 30, 0), ("sorted random 31-mers, 4-byte taxids", 31, 62, 4)):
        keys = sorted_codes(n, bits)
        tax = torch.randint(1, 1 << 31, (n,), device=dev, generator=gen, dtype=torch.int32) if tb else None
        flags = S | (T if tb else 0)
        out_b = torch.empty(lib.unik_encode_bound(n, k, flags, tb), dtype=torch.uint8, device=dev)
        te, body = timed(lambda: ctx.unik_encode(keys, k, flags, taxids=tax, taxid_bytes=tb, out=out_b))
        out_k = torch.empty(n, dtype=torch.int64, device=dev)
        out_t = torch.empty(n, dtype=torch.int32, device=dev) if tb else None
        td, (dk, dt) = timed(lambda: ctx.unik_decode(body, k, flags, tb, out=out_k, out_taxids=out_t))
        assert torch.equal(dk, keys) and (tax is None or torch.equal(dt, tax)), "decode(encode(x)) != x"
        nb = body.numel()
        moved = nb + n * (8 + (4 if tb else 0))
        cms = copy_ms(moved)
        path = os.path.join(tmp, "shape.unik")
        write_file(path, k, flags, tb, body, n)
        host = [json.loads(subprocess.check_output([timer, path, path + ".out"])) for _ in range(3)]
        assert host[0]["records"] == n and open(path, "rb").read() == open(path + ".out", "rb").read(), "host and device bodies differ"
        row = {"shape": name, "n": n, "k": k, "taxid_bytes": tb, "body_bytes": nb, "bytes_per_record": nb / n,
               "decode": td, "encode": te, "moved_bytes": moved, "copy_ms": cms,
               "decode_GBps": moved / td["call_ms"] / 1e6, "encode_GBps": moved / te["call_ms"] / 1e6, "copy_GBps": moved / cms / 1e6,
               "decode_frac_of_copy": cms / td["call_ms"], "encode_frac_of_copy": cms / te["call_ms"],
               "host_read_ms": statistics.median(h["read_ms"] for h in host), "host_write_ms": statistics.median(h["write_ms"] for h in host)}
        row["decode_speedup_over_host"] = row["host_read_ms"] / td["call_ms"]
        row["encode_speedup_over_host"] = row["host_write_ms"] / te["call_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        os.remove(path)
        os.remove(path + ".out")
        del keys, tax, out_b, out_k, out_t, body, dk, dt
        torch.cuda.empty_cache()

    # ---- the driver end to end --------------------------------------------------------------------------------------
    e2e = []
    m = a.e2e_records
    if m > 0:
        for gz in (False, True):
            paths = []
            for i in range(2):
                keys = sorted_codes(m, 62)
                body = ctx.unik_encode(keys, 31, S)
                p = os.path.join(tmp, "in%d%s.unik" % (i, "_gz" if gz else ""))
                write_file(p, 31, S, 0, body, m, gz=gz)
                paths.append(p)
                del keys, body
                torch.cuda.empty_cache()
            ctx.trim()
            outs = {}
            for label, exe, env in (("device_codec", BIN, {"UNIKMER_DEVICE_CODEC": "1"}), ("host_codec", BIN, {"UNIKMER_HOST_CODEC": "1"}),
                                    ("parent", a.parent_bin, {})):
                if exe is None:
                    continue
                env_all = {k: v for k, v in os.environ.items() if k not in ("UNIKMER_DEVICE_CODEC", "UNIKMER_HOST_CODEC")}
                env_all.update(env)
                out = os.path.join(tmp, "out_" + label)
                ts = []
                for _ in range(5):
                    t0 = time.perf_counter()
                    subprocess.check_call([exe, "union", paths[0], paths[1], "-C", "-o", out], env=env_all, stderr=subprocess.DEVNULL)
                    ts.append(time.perf_counter() - t0)
                outs[label] = out + ".unik"
                e2e.append({"command": "union a.unik b.unik -C -o out", "records_per_file": m, "inputs": "gzip" if gz else "uncompressed",
                            "binary": label, "wall_s_median": statistics.median(ts), "wall_s_min": min(ts), "wall_s_max": max(ts), "wall_s": ts})
                print(json.dumps(e2e[-1]), flush=True)
            ref = open(outs["host_codec"], "rb").read()
            for label, p in outs.items():
                assert open(p, "rb").read() == ref, "the output of %s differs" % label
            del ref
            for p in paths + list(outs.values()):
                os.remove(p)

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    doc = {"tool": "tools/bench_codec.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps, "warmup": a.warmup,
           "rows": rows, "end_to_end": e2e}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    shutil.rmtree(tmp, ignore_errors=True)
    ctx.close()


if __name__ == "__main__":
    main()
