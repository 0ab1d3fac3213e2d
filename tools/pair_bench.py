#!/usr/bin/env python
"""tools/pair_bench.py -- ukm_pair_counts against one ukm_setop2 size query per pair.

`python tools/pair_bench.py [--shapes 1000x1e6,100x1e7,1000x1e4,1000x1e6x100] [--reps 5] [--out profiles/pair_counts.json]`

A shape is FILESxCODES[xSPREAD]: FILES sorted device tensors of about CODES codes each, drawn the way run_configs.py draws
its overlapping files from bench.py's generator: a universe of SPREAD x CODES codes (cumulated splitmix64 gaps; SPREAD
defaults to 2), of which every file keeps a 1 / SPREAD share chosen by a hash of its own.  SPREAD = 2 gives files that share
half their codes pairwise; a larger SPREAD gives more columns and less overlap at the same input size.

Per shape, the median over --reps calls after --warmup, inputs and outputs resident on the device:
  call_ms     ukm_last_call_ms: the whole call, first launch to last
  sort_ms     statistic pair_sort_us: tagging, sorting and ranking the records
  bits_ms     statistic pair_bits_us: zeroing the bit matrix and setting its bits, all blocks
  kernel_ms   ukm_last_kernel_ms: the launches of pair_popc_kernel, summed
  pair_words_per_s   the 32-bit pair-words the kernel's workgroups process (whole 64 x 64 tiles, whole K tiles) / kernel time
  valu_fraction      of the bound 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz / 2 instructions per pair-word = 3.93e13 pair-words/s
The baseline is the same matrix the only way the library offered before: Context.setop2(OP_INTER) as a size query per
pair, on the same tensors.  All N (N - 1) / 2 pairs where they are at most --pairs, else --pairs randomly chosen pairs scaled
up; the JSON says which ("extrapolated").  The counts of the timed pairs are compared with the matrix before anything is timed.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KT_COLS, TILE = 2048, 64
VALU_BOUND = 256 * 4 * 32 * 2.4e9 / 2


def pair_words(nfiles, ncols):
    """the pair-words pair_popc_kernel's workgroups process for the full matrix: ukm_pairs.h's default plan restated"""
    rows = (nfiles + TILE - 1) // TILE * TILE
    w = max(KT_COLS, min(1 << 31, (1 << 33) // rows // KT_COLS * KT_COLS))
    nt = rows // TILE
    ktiles = sum((min(w, ncols - c0) + KT_COLS - 1) // KT_COLS for c0 in range(0, ncols, w))
    return nt * (nt + 1) // 2 * TILE * TILE * ktiles * (KT_COLS // 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000x1e6,100x1e7,1000x1e4,1000x1e6x100")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=1000, help="pairs the baseline times")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_counts.json"))
    args = ap.parse_args()
    assert args.reps >= 5, "a median of at least 5 runs"

    import torch
    import bench
    from unikmer_amd import lib
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    result = {"tool": "tools/pair_bench.py", "reps": args.reps, "warmup": args.warmup, "statistic": "median",
              "device": torch.cuda.get_device_name(0), "valu_bound_pair_words_per_s": VALU_BOUND, "shapes": []}
    for shape in args.shapes.split(","):
        parts = shape.split("x")
        nfiles, per, spread = int(parts[0]), int(float(parts[1])), int(parts[2]) if len(parts) > 2 else 2
        nu = spread * per
        j = torch.arange(nu, dtype=torch.int64, device=dev)
        U = torch.cumsum(1 + (bench.splitmix64_torch(j ^ bench._i64(bench.SEED)) & ((1 << 32) - 1)), 0)
        files = []
        for f in range(nfiles):
            h = bench.splitmix64_torch(j ^ bench._i64(bench.SEED + 1000 * (f + 1)))
            files.append(U[((h >> 17) & 0xFFFFF) % spread == 0])
        del j, U, h
        total = sum(x.numel() for x in files)
        out = torch.zeros(nfiles * nfiles, dtype=torch.int64, device=dev)
        sizes = torch.zeros(nfiles, dtype=torch.int64, device=dev)
        ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
        ctx.pair_counts(files, out=out, sizes=sizes)      # untimed: grows the workspace
        ncols, nblocks = ctx.stat("pair_columns"), ctx.stat("pair_blocks")
        C = out.view(nfiles, nfiles).cpu()
        assert bool((C == C.T).all()) and bool((C.diagonal() == sizes.cpu()).all())
        assert sizes.cpu().tolist() == [x.numel() for x in files]

        # ---- baseline: one size query per pair ----
        all_pairs = nfiles * (nfiles - 1) // 2
        rnd = random.Random(bench.SEED)
        if all_pairs <= args.pairs:
            pairs = [(a, b) for a in range(nfiles) for b in range(a + 1, nfiles)]
        else:
            pairs = []
            while len(pairs) < args.pairs:
                a, b = rnd.randrange(nfiles), rnd.randrange(nfiles)
                if a != b:
                    pairs.append((a, b))
        scratch = torch.zeros(max(x.numel() for x in files) + 8, dtype=torch.int64, device=dev)
        for a, b in pairs[:50]:                            # parity (and warm-up of the baseline)
            assert ctx.setop2(lib.OP_INTER, files[a], files[b], out=scratch).numel() == int(C[a, b]), (a, b)
        base = []
        for _ in range(args.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for a, b in pairs:
                ctx.setop2(lib.OP_INTER, files[a], files[b], out=scratch)
            torch.cuda.synchronize(dev)
            base.append((time.perf_counter() - t0) * 1e3)
        base_ms = statistics.median(base) * all_pairs / len(pairs)

        # ---- the call ----
        for _ in range(args.warmup):
            ctx.pair_counts(files, out=out, sizes=sizes)
        rows = {k: [] for k in ("call_ms", "sort_ms", "bits_ms", "kernel_ms", "wall_ms")}
        for _ in range(args.reps):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            ctx.pair_counts(files, out=out, sizes=sizes)
            torch.cuda.synchronize(dev)
            rows["wall_ms"].append((time.perf_counter() - t0) * 1e3)
            rows["call_ms"].append(ctx.last_call_ms())
            rows["kernel_ms"].append(ctx.last_kernel_ms())
            rows["sort_ms"].append(ctx.stat("pair_sort_us") / 1e3)
            rows["bits_ms"].append(ctx.stat("pair_bits_us") / 1e3)
        assert bool((out.view(nfiles, nfiles).cpu() == C).all())
        med = {k: statistics.median(v) for k, v in rows.items()}
        pw = pair_words(nfiles, ncols)
        useful = nfiles * (nfiles + 1) // 2 * ((ncols + 31) // 32)
        entry = {"shape": shape, "files": nfiles, "codes_per_file": per, "spread": spread, "records": total, "columns": ncols, "blocks": nblocks,
                 **med, "kernel_ms_min": min(rows["kernel_ms"]), "kernel_ms_max": max(rows["kernel_ms"]),
                 "pair_words": pw, "pair_words_per_s": pw / (med["kernel_ms"] * 1e-3), "valu_fraction": pw / (med["kernel_ms"] * 1e-3) / VALU_BOUND,
                 "useful_pair_words": useful, "useful_pair_words_per_s": useful / (med["kernel_ms"] * 1e-3),
                 "baseline": {"what": "Context.setop2(OP_INTER) size query per pair, host wall clock, device synchronised", "pairs_timed": len(pairs),
                              "pairs_all": all_pairs, "extrapolated": len(pairs) < all_pairs, "ms_all_pairs": base_ms,
                              "ms_per_pair": statistics.median(base) / len(pairs)},
                 "ratio_baseline_over_call_wall": base_ms / med["wall_ms"]}
        result["shapes"].append(entry)
        print(json.dumps(entry), flush=True)
        ctx.close()
        del files, out, sizes, scratch
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
