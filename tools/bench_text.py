#!/usr/bin/env python3
"""ukm_view / ukm_dump: the device calls, and `unikmer view -t` / `unikmer dump -s` end to end against the host loops.

    python tools/bench_text.py [--records 100000000] [--e2e-records 100000000,2600000] [--e2e-runs 1,5]
                               [--parent-bin PATH/unikmer] [--tmp DIR] [--out profiles/text.json]

Calls, on device tensors of --records sorted random 31-mers with 4-byte taxids: ukm_view in the formats KMER, KMER_TAXID
and FASTA and ukm_dump of the KMER_TAXID text, timed with the context's own event timer (ukm_last_call_ms: all device work
of the call), median of --steps calls behind --warmup calls; GB/s of text written (read, for dump); and a device-to-device
copy of as many bytes as the call moves (records + text), timed in the same run with torch events -- the roofline a
streaming kernel can be held to.

End to end, per size in --e2e-records: `unikmer view -t f.unik -o text` and `unikmer dump -s text -o g -C` on an uncompressed
sorted file with per-record taxids, wall time, median of the runs given: this build with UNIKMER_DEVICE_TEXT=1, with
UNIKMER_HOST_TEXT=1, and --parent-bin (the parent commit's driver beside its own library) when given.
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--e2e-records", default="100000000,2600000")
    ap.add_argument("--e2e-runs", default="1,5")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "text.json"))
    a = ap.parse_args()

    import torch
    from unikmer_amd import lib, unikfile
    if not torch.cuda.is_available():
        raise SystemExit("bench_text.py needs the GPU")
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20241019)
    tmp = tempfile.mkdtemp(prefix="bench_text_", dir=a.tmp)
    k = 31

    def records(n):
        keys = torch.sort(torch.randint(0, 1 << 62, (n,), device=dev, generator=gen, dtype=torch.int64)).values
        return keys, torch.randint(1, 1 << 31, (n,), device=dev, generator=gen, dtype=torch.int32)

    def timed(fn):
        for _ in range(a.warmup):
            r = fn()
        call = []
        for _ in range(a.steps):
            r = fn()
            call.append(ctx.last_call_ms())
        return {"call_ms": statistics.median(call), "call_ms_min": min(call)}, r

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

    result = {"records": a.records, "k": k, "calls": [], "e2e": []}
    n = a.records
    keys, tax = records(n)
    text_kt = None
    for name, fmt in (("KMER", lib.VIEW_KMER), ("KMER_TAXID", lib.VIEW_KMER_TAXID), ("FASTA", lib.VIEW_FASTA)):
        out = torch.empty(lib.view_bound(n, k, False, fmt), dtype=torch.uint8, device=dev)
        t, text = timed(lambda: ctx.view(keys, tax, k=k, fmt=fmt, out=out))
        nb = text.numel()
        moved = nb + n * (8 + (4 if fmt == lib.VIEW_KMER_TAXID else 0))
        cms = copy_ms(moved)
        result["calls"].append({"call": "ukm_view " + name, "text_bytes": nb, "bytes_per_record": nb / n, **t, "text_GBps": nb / t["call_ms"] / 1e6,
                                "moved_bytes": moved, "moved_GBps": moved / t["call_ms"] / 1e6, "copy_ms": cms, "copy_GBps": moved / cms / 1e6,
                                "frac_of_copy": cms / t["call_ms"], "frac_of_8TBps": moved / t["call_ms"] / 1e6 / 8000})
        print(json.dumps(result["calls"][-1]), flush=True)
        if fmt == lib.VIEW_KMER_TAXID:
            text_kt = text.clone()
        del out, text
    ok, ot = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    t, (dk, dt) = timed(lambda: ctx.dump(text_kt, k=k, flags=lib.DUMP_TAXID, out=ok, out_taxids=ot))
    assert torch.equal(dk, keys) and torch.equal(dt, tax), "dump(view(x)) != x"
    nb = text_kt.numel()
    moved = 2 * nb + n * 12          # the text is read by both passes
    cms = copy_ms(moved)
    result["calls"].append({"call": "ukm_dump KMER_TAXID", "text_bytes": nb, **t, "text_GBps": nb / t["call_ms"] / 1e6, "moved_bytes": moved,
                            "moved_GBps": moved / t["call_ms"] / 1e6, "copy_ms": cms, "copy_GBps": moved / cms / 1e6, "frac_of_copy": cms / t["call_ms"],
                            "frac_of_8TBps": moved / t["call_ms"] / 1e6 / 8000})
    print(json.dumps(result["calls"][-1]), flush=True)
    del keys, tax, text_kt, ok, ot, dk, dt
    torch.cuda.empty_cache()

    S, T = lib.UNIK_SORTED, lib.UNIK_INCLUDE_TAXID
    bins = {"device": (BIN, {"UNIKMER_DEVICE_TEXT": "1"}), "host": (BIN, {"UNIKMER_HOST_TEXT": "1"})}
    if a.parent_bin:
        bins["parent"] = (a.parent_bin, {})

    def wall(exe, env, *args):
        e = {k_: v for k_, v in os.environ.items() if k_ not in ("UNIKMER_DEVICE_TEXT", "UNIKMER_HOST_TEXT")}
        e.update(env)
        t0 = time.perf_counter()
        subprocess.check_call([exe] + list(args), env=e)
        return time.perf_counter() - t0

    for m, runs in zip([int(x) for x in a.e2e_records.split(",") if x], [int(x) for x in a.e2e_runs.split(",") if x]):
        keys, tax = records(m)
        body = ctx.unik_encode(keys, k, S | T, taxids=tax, taxid_bytes=4)
        f = os.path.join(tmp, "in.unik")
        with open(f, "wb") as fh:
            fh.write(unikfile.header_bytes({"k": k, "flag": S | T | 2, "taxid_bytes": 4, "number": m}))
            fh.write(body.cpu().numpy().tobytes())
        del keys, tax, body
        row = {"records": m, "runs": runs}
        texts = {}
        for who, (exe, env) in bins.items():
            texts[who] = os.path.join(tmp, "text_" + who)
            row["view -t, " + who + " s"] = statistics.median(wall(exe, env, "view", "-t", f, "-o", texts[who]) for _ in range(runs))
        for who, (exe, env) in bins.items():
            row["dump -s, " + who + " s"] = statistics.median(wall(exe, env, "dump", "-s", "-C", texts["host"], "-o", os.path.join(tmp, "out_" + who))
                                                               for _ in range(runs))
        row["same text"] = all(subprocess.call(["cmp", "-s", texts["host"], p]) == 0 for p in texts.values())
        row["same files"] = all(subprocess.call(["cmp", "-s", os.path.join(tmp, "out_host.unik"), os.path.join(tmp, "out_" + w + ".unik")]) == 0 for w in bins)
        row["text_bytes"] = os.path.getsize(texts["host"])
        result["e2e"].append(row)
        print(json.dumps(row), flush=True)
        for p in list(texts.values()) + [os.path.join(tmp, "out_" + w + ".unik") for w in bins]:
            os.remove(p)
    shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
