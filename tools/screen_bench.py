#!/usr/bin/env python
"""tools/screen_bench.py -- ukm_screen against the only way the library offered before it.

`python tools/screen_bench.py [--shapes reads:1e6,reads:1e7,reads:1e8,long:1e7] [--reps 5] [--out profiles/screen.json]`

Shapes
  reads:S   1e6 records of 150 bases (k = 31, canonical), drawn at random positions from a random genome of 2 S bases, against a
            sorted set of S codes: every other distinct code of that genome, so about half of the windows hit
  long:S    ONE record of 1e8 bases (the genome of reads:S repeated) against the same set
Per shape the call is timed with and without per-code taxids (random nodes of a complete 8-ary tree of depth 7) and with
both routes forced (option "map_sorted" 0: lookups in genome order, fused with the reduction; 1: all (code, window) pairs
sorted first) and with the library's own choice.  Inputs and outputs are device tensors.  After --warmup calls, the median
(and min / max) over --reps calls of
  call_ms    ukm_last_call_ms: hipEvents around the whole call
  kernel_ms  ukm_last_kernel_ms: the lookup and reduction kernels
The baseline is what the library offered for the same answer before this call: Context.locate with the set as q_keys (every hit
materialised as 20 bytes), out_rec downloaded, np.bincount on the host.  Its figure is HOST WALL CLOCK and INCLUDES that
transfer and the host's counting -- that is the cost a user pays; it yields no LCA at all.  The hit counts of both ways are
compared before anything is timed.

Algorithmic bytes per window (what must move, not the cache lines that do), h = hit fraction, t = 1 with taxids:
  genome order  1 base + 8 window written + 8 read + 8 directory + 16 two probes of the set + 8 h t (taxid, pre-order number)
  sorted        1 + 8 + 8 + 4 index written + 24 P sort passes of a 12-byte pair (P = ceil(62 / 8) digit passes, an upper
                estimate: the sort's own plan may do fewer) + 12 pair + 8 directory + 8 set + 4 word written + 4 read + 8 h t
and the fraction of 8 TB/s these bytes amount to at the measured call time."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, READS, READ_LEN, LONG = 31, 1_000_000, 150, 100_000_000
HBM = 8e12


def alg_bytes(route_sorted, h, t):
    if not route_sorted:
        return 1 + 8 + 8 + 8 + 16 + 8 * h * t
    return 1 + 8 + 8 + 4 + 24 * math.ceil(2 * K / 8) + 12 + 8 + 8 + 4 + 4 + 8 * h * t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="reads:1e6,reads:1e7,reads:1e8,long:1e7")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--base-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "screen.json"))
    args = ap.parse_args()
    assert args.reps >= 5, "a median of at least 5 runs"

    import torch
    from unikmer_amd import lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    result = {"tool": "tools/screen_bench.py", "reps": args.reps, "warmup": args.warmup, "statistic": "median", "k": K,
              "device": torch.cuda.get_device_name(0), "hbm_bytes_per_s": HBM,
              "baseline": "Context.locate(set as q_keys) + download of out_rec + np.bincount; host wall clock, transfer and host time included",
              "shapes": []}
    ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    depth, arity = 7, 8
    nnodes = sum(arity ** d for d in range(depth + 1))
    child = np.arange(1, nnodes + 1, dtype=np.uint32)
    parent = ((child.astype(np.int64) - 2) // arity + 1).astype(np.uint32)
    parent[0] = 1
    ctx.taxonomy_load(child, parent)
    acgt = torch.tensor([65, 67, 71, 84], dtype=torch.uint8, device=dev)
    for shape in args.shapes.split(","):
        kind, size = shape.split(":")
        n_set = int(float(size))
        genome = acgt[torch.randint(0, 4, (2 * n_set,), device=dev, generator=g)]
        goff = torch.tensor([0, genome.numel()], dtype=torch.int64, device=dev)
        codes = ctx.count(genome, goff, K)                 # the genome's distinct canonical codes, sorted
        keys = codes[::2].contiguous()
        if keys.numel() > n_set:
            keys = keys[:n_set].contiguous()
        n_set = int(keys.numel())
        taxids = torch.randint(1, nnodes + 1, (n_set,), device=dev, generator=g, dtype=torch.int32)
        if kind == "reads":
            start = torch.randint(0, genome.numel() - READ_LEN, (READS,), device=dev, generator=g)
            bases = genome[(start[:, None] + torch.arange(READ_LEN, device=dev)[None, :]).reshape(-1)].contiguous()
            off = torch.arange(READS + 1, dtype=torch.int64, device=dev) * READ_LEN
        else:
            bases = genome.repeat((LONG + genome.numel() - 1) // genome.numel())[:LONG].contiguous()
            off = torch.tensor([0, LONG], dtype=torch.int64, device=dev)
        n_rec = int(off.numel()) - 1
        del genome, codes
        outs = tuple(torch.zeros(n_rec, dtype=torch.int32, device=dev) for _ in range(3))
        win, hit, lca = ctx.screen(bases, off, K, keys, taxids, outs=outs)     # untimed: grows the workspace
        n_win, n_hit = int(win.sum().item()), int(hit.sum().item())
        h = n_hit / n_win
        want_hit = hit.cpu().numpy().view(np.uint32).copy()

        # ---- baseline ----
        base = []
        for rep in range(args.base_reps + 1):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            q, rec, pos = ctx.locate(bases, off, K, keys, out_cap=n_win)
            cnt = np.bincount(rec.cpu().numpy().view(np.uint32), minlength=n_rec)
            base.append((time.perf_counter() - t0) * 1e3)
            if rep == 0:
                assert np.array_equal(cnt.astype(np.uint32), want_hit), "baseline and ukm_screen disagree"
            del q, rec, pos
        base_ms = statistics.median(base[1:])

        entry = {"shape": shape, "records": n_rec, "bases": int(bases.numel()), "windows": n_win, "set_codes": n_set, "hit_fraction": h,
                 "baseline_wall_ms": base_ms, "baseline_reps": args.base_reps, "runs": []}
        for with_tax in (False, True):
            for route in (0, 1, None):
                ctx.set_option("map_sorted", route)
                o = outs if with_tax else (outs[0], outs[1], None)
                call, kern, wall = [], [], []
                for i in range(args.warmup + args.reps):
                    torch.cuda.synchronize(dev)
                    t0 = time.perf_counter()
                    got = ctx.screen(bases, off, K, keys, taxids if with_tax else None, outs=o)
                    torch.cuda.synchronize(dev)
                    if i >= args.warmup:
                        wall.append((time.perf_counter() - t0) * 1e3)
                        call.append(ctx.last_call_ms())
                        kern.append(ctx.last_kernel_ms())
                assert np.array_equal(got[1].cpu().numpy().view(np.uint32), want_hit)
                is_sorted = route == 1 or (route is None and n_set >= (1 << 24))
                med = statistics.median(call)
                b = alg_bytes(is_sorted, h, 1 if with_tax else 0)
                run = {"taxids": with_tax, "map_sorted": route, "route": "sorted" if is_sorted else "genome order",
                       "call_ms": med, "call_ms_min": min(call), "call_ms_max": max(call), "kernel_ms": statistics.median(kern),
                       "kernel_ms_min": min(kern), "kernel_ms_max": max(kern), "wall_ms": statistics.median(wall),
                       "windows_per_s": n_win / (med * 1e-3), "alg_bytes_per_window": b, "hbm_fraction": b * n_win / (med * 1e-3) / HBM,
                       "baseline_over_call_wall": base_ms / statistics.median(wall)}
                entry["runs"].append(run)
                print(json.dumps({"shape": shape, **run}), flush=True)
        ctx.set_option("map_sorted", None)
        result["shapes"].append(entry)
        del bases, off, keys, taxids, outs
        ctx.trim()
        torch.cuda.empty_cache()
    ctx.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
