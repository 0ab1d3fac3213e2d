#!/usr/bin/env python
"""tools/setop_multi_bench.py -- ukm_setop2_multi against the separate ukm_setop2 calls.

`python tools/setop_multi_bench.py [--sizes 1e8,1e9] [--reps 20] [--out profiles/setop_multi.json]`

Device tensors, bench.py's generator (sets of --sizes sorted 62-bit codes each, its overlap), outputs resident before
anything is timed.  Four sequences per size, the median over --reps repetitions after --warmup:
  a  setop2(UNION) then setop2(INTER): bench.py's step, partition cache included
  b  the same plus setop2(DIFF)
  c  setop2_multi UNION | INTER
  d  setop2_multi UNION | INTER | DIFF
For each: kernel_ms (the sum of last_kernel_ms over the sequence's calls: hipEvents round the tile kernels), call_ms (the
sum of last_call_ms: the calls from their first launch to their last) and wall_ms (host clock round the sequence, device
synchronised), the algorithmic bytes (8 per input record per pass over the inputs, 8 per output record) and TB/s =
bytes / kernel time.  The results of c and d are compared with a's and b's, bit for bit, before anything is timed.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e8,1e9")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "setop_multi.json"))
    args = ap.parse_args()
    assert args.reps >= 1

    import torch
    import bench
    from unikmer_amd import lib
    U, I, D = lib.OP_UNION, lib.OP_INTER, lib.OP_DIFF
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    result = {"tool": "tools/setop_multi_bench.py", "reps": args.reps, "warmup": args.warmup, "statistic": "median",
              "device": torch.cuda.get_device_name(0), "sizes": []}
    for size in [int(float(s)) for s in args.sizes.split(",")]:
        A, B = bench.gen_sets_device((4 * size + 2) // 3, 32, 0, bench.SEED, dev)
        na, nb = A.numel(), B.numel()
        outs = {U: torch.zeros(na + nb, dtype=torch.int64, device=dev), I: torch.zeros(na, dtype=torch.int64, device=dev),
                D: torch.zeros(na, dtype=torch.int64, device=dev)}
        ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)

        def separate(ops):
            def run():
                k = c = 0.0
                n = {}
                for op in ops:
                    n[op] = ctx.setop2(op, A, B, out=outs[op]).numel()
                    k += ctx.last_kernel_ms()
                    c += ctx.last_call_ms()
                return n, k, c
            return run

        def fused(ops):
            def run():
                got = ctx.setop2_multi(A, B, ops=ops, out={op: outs[op] for op in ops})
                return {op: got[op].numel() for op in ops}, ctx.last_kernel_ms(), ctx.last_call_ms()
            return run
        seqs = {"a_setop2_union_inter": (separate((U, I)), (U, I), 2), "b_setop2_union_inter_diff": (separate((U, I, D)), (U, I, D), 3),
                "c_multi_union_inter": (fused((U, I)), (U, I), 1), "d_multi_union_inter_diff": (fused((U, I, D)), (U, I, D), 1)}
        # parity first: the fused outputs against the separate calls'
        n_sep, _, _ = seqs["b_setop2_union_inter_diff"][0]()
        keep = {op: outs[op][:n_sep[op]].clone() for op in (U, I, D)}
        for name in ("c_multi_union_inter", "d_multi_union_inter_diff"):
            for op in (U, I, D):
                outs[op].zero_()
            n_f, _, _ = seqs[name][0]()
            for op in seqs[name][1]:
                assert n_f[op] == n_sep[op] and torch.equal(outs[op][:n_f[op]], keep[op]), (name, op)
        del keep
        f0, s0 = ctx.stat("setop_multi_fused"), ctx.stat("setop_multi_split")
        entry = {"set_size": size, "na": na, "nb": nb, "n_union": n_sep[U], "n_inter": n_sep[I], "n_diff": n_sep[D], "sequences": {}}
        for name, (run, ops, passes) in seqs.items():
            for _ in range(args.warmup):
                run()
            ks, cs, ws = [], [], []
            for _ in range(args.reps):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                _, k, c = run()
                torch.cuda.synchronize(dev)
                ws.append((time.perf_counter() - t0) * 1e3)
                ks.append(k)
                cs.append(c)
            nbytes = 8.0 * (na + nb) * passes + 8.0 * sum(n_sep[op] for op in ops)
            k = statistics.median(ks)
            entry["sequences"][name] = {"kernel_ms": k, "call_ms": statistics.median(cs), "wall_ms": statistics.median(ws),
                                        "kernel_ms_min": min(ks), "kernel_ms_max": max(ks),
                                        "algorithmic_bytes": nbytes, "TBps": nbytes / (k * 1e-3) / 1e12}
        s = entry["sequences"]
        entry["ratio_c_over_a"] = {m: s["c_multi_union_inter"][m] / s["a_setop2_union_inter"][m] for m in ("kernel_ms", "call_ms", "wall_ms", "algorithmic_bytes")}
        entry["ratio_d_over_b"] = {m: s["d_multi_union_inter_diff"][m] / s["b_setop2_union_inter_diff"][m] for m in ("kernel_ms", "call_ms", "wall_ms", "algorithmic_bytes")}
        entry["routes"] = {"fused": ctx.stat("setop_multi_fused") - f0, "split": ctx.stat("setop_multi_split") - s0}
        result["sizes"].append(entry)
        print(json.dumps(entry), flush=True)
        ctx.close()
        del A, B, outs
        torch.cuda.empty_cache()
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
