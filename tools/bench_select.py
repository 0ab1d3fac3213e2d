#!/usr/bin/env python3
"""ukm_filter / ukm_grep against what a user would do today with torch on the same device.

    python tools/bench_select.py [--filter-sizes 100000000,1000000000] [--records 100000000]
                                 [--queries 100,2048,10000,1000000,10000000,100000000] [--out profiles/select.json]

Records: random 31-mer codes (seeded).  Timed with the context's own event timer (ukm_last_call_ms: all device work of the
call), median of --steps calls behind --warmup calls; torch compositions with torch events around them, the same way.

  ukm_filter at the defaults (-t 15 -w 7 -s 3 -d 1).  Algorithmic bytes = 8 B read per record + 8 B written per kept record;
  the fraction is bytes / call time / 8 TB/s.  Beside it: a plain device-to-device copy of the input (8 B + 8 B per record),
  which no selection can beat at the same share kept, and its rate.

  ukm_grep on --records records, half of them drawn from the queries, for every --queries size: each route forced where it
  applies (option "grep_lds" 1: the LDS table, only while the queries fit it; 0: sorted queries behind the prefix directory),
  then the library's choice.  The comparison is a composition that is NOT the code under test: torch.isin followed by
  boolean-mask indexing, and torch.sort of the queries + torch.searchsorted + gather-compare followed by boolean-mask
  indexing; `torch_ms` is the faster of the two.  Both include what ukm_grep includes: the queries arrive unsorted.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 31
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter-sizes", default="100000000,1000000000")
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--queries", default="100,2048,10000,1000000,10000000,100000000")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select.json"))
    a = ap.parse_args()
    assert a.steps >= 3

    import torch
    from unikmer_amd import lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_select.py needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20241017)

    def codes(n):
        return torch.randint(0, 1 << (2 * K), (n,), device=dev, generator=gen, dtype=torch.int64)

    def timed(fn):
        for _ in range(a.warmup):
            r = fn()
        call = []
        for _ in range(a.steps):
            r = fn()
            call.append(ctx.last_call_ms())
        return {"call_ms": statistics.median(call), "call_ms_min": min(call)}, r

    def torch_ms(fn):
        for _ in range(a.warmup):
            fn()
        ts = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
            del r
        return statistics.median(ts)

    rows = []
    for n in [int(x) for x in a.filter_sizes.split(",") if x]:
        rec = codes(n)
        out = torch.empty(n, dtype=torch.int64, device=dev)
        t, kept = timed(lambda: ctx.filter(rec, K, out=out))
        nk = kept.numel()
        copy_ms = torch_ms(lambda: out.copy_(rec))
        nbytes = 8 * n + 8 * nk
        rows.append({"call": "ukm_filter", "n": n, "k": K, "threshold": 15, "window": 7, "penalty_s": 3, "penalty_d": 1, "kept": nk,
                     "kept_share": nk / n, **t, "algorithmic_bytes": nbytes, "frac_of_8TBps": nbytes / (t["call_ms"] * 1e-3) / PEAK,
                     "copy_ms": copy_ms, "copy_bytes": 16 * n, "copy_frac_of_8TBps": 16 * n / (copy_ms * 1e-3) / PEAK,
                     "ratio_copy_over_filter": copy_ms / t["call_ms"]})
        print(json.dumps(rows[-1]), flush=True)
        del rec, out, kept
    torch.cuda.empty_cache()

    n = a.records
    pool = codes(n)
    pick = torch.randint(0, 1 << 62, (n,), device=dev, generator=gen, dtype=torch.int64)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    for nq in [int(x) for x in a.queries.split(",") if x]:
        q = codes(nq)
        rec = torch.where((pick & 1) == 0, q[(pick >> 1) % nq], pool)   # half of the records are queries; unsorted, with duplicates

        def isin():
            return rec[torch.isin(rec, q)]

        def searchsorted():
            qs = torch.sort(q).values
            idx = torch.searchsorted(qs, rec)
            idx.clamp_(max=nq - 1)
            return rec[qs[idx] == rec]
        want = isin()
        t_isin, t_ss = torch_ms(isin), torch_ms(searchsorted)
        res = {}
        for route in ("lds", "dir", "default"):
            if route == "lds" and nq > 2048:
                continue
            ctx.set_option("grep_lds", {"lds": 1, "dir": 0, "default": None}[route])
            try:
                t, r = timed(lambda: ctx.grep(rec, q, out=out))
                t["grep_route"] = ctx.stat("grep_route")
            finally:
                ctx.set_option("grep_lds", None)
            assert torch.equal(r, want), "ukm_grep and torch disagree"
            res["route_" + route] = t
        td = res["route_default"]
        nbytes = 8 * n + 8 * want.numel() + 8 * nq
        rows.append({"call": "ukm_grep", "n": n, "nq": nq, "kept": want.numel(), **res, "algorithmic_bytes": nbytes,
                     "frac_of_8TBps": nbytes / (td["call_ms"] * 1e-3) / PEAK, "torch_isin_ms": t_isin, "torch_searchsorted_ms": t_ss,
                     "torch_ms": min(t_isin, t_ss), "ratio_torch_over_ukm": min(t_isin, t_ss) / td["call_ms"]})
        print(json.dumps(rows[-1]), flush=True)
        del q, rec, want, r
        torch.cuda.empty_cache()

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    doc = {"tool": "tools/bench_select.py", "commit": commit, "device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK,
           "steps": a.steps, "warmup": a.warmup, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
