#!/usr/bin/env python3
"""ukm_rfilter and ukm_tsplit beside the existing calls they are built on.

    python tools/bench_taxsel.py [--records 100000000] [--out profiles/rfilter_tsplit.json]

Timed with the context's own event timer (ukm_last_call_ms: all device work of the call), median of --steps calls behind
--warmup calls.  Records: random codes and taxids drawn uniformly from a complete 8-ary tree of depth 7 (2,396,745 nodes),
ranks by depth, a hashed tenth of the nodes `no rank`; all arrays on the device.

  ukm_rfilter (-N -n -L <the rank of depth 5>) next to ukm_grep by taxid over the SAME records with the taxids the filter
  keeps as queries: the same selection kernel, the same records kept -- the yardstick.  What differs is how the bitmap comes
  about (one pass over the taxonomy against one pass over the queries); the builder's time is reported on its own as the
  time of ukm_rank_pass over a single taxid (builder kernel + a one-thread lookup).

  ukm_tsplit next to ukm_sort_pairs of the same (taxid, record index) pairs at key_bits = 32: the sort it contains (this
  change does not touch ukm_sort.hip).  `extra_ms` = what pairing, gathering the codes and compacting the run heads add.
  Once with taxids from the whole tree (millions of groups) and once with 1000 distinct taxids.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RANKS = ["domain", "kingdom", "phylum", "class", "order", "family", "genus", "species"]   # depth 0 .. 7


def synth_tree(depth=7, arity=8):
    T = sum(arity ** d for d in range(depth + 1))
    child = np.arange(1, T + 1, dtype=np.uint32)
    parent = ((child.astype(np.int64) - 2) // arity + 1).astype(np.uint32)
    parent[0] = 1
    return child, parent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rfilter_tsplit.json"))
    a = ap.parse_args()
    assert a.steps >= 3

    import torch
    from unikmer_amd import lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_taxsel.py needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20241018)

    def timed(fn):
        for _ in range(a.warmup):
            r = fn()
        call = []
        for _ in range(a.steps):
            r = fn()
            call.append(ctx.last_call_ms())
        return {"call_ms": statistics.median(call), "call_ms_min": min(call)}, r

    # the taxonomy: ranks by depth, rank id = depth + 1, `no rank` (id 9) for a hashed tenth
    child, parent = synth_tree()
    T = len(child)
    depth = np.zeros(T + 1, dtype=np.int64)
    for d, first in enumerate(np.cumsum([0] + [8 ** x for x in range(8)])[:-1]):
        depth[first + 1:] = d
    rank_id = (depth[1:] + 1).astype(np.uint8)
    h = (child.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(40)
    rank_id[(h % np.uint64(10)) == 0] = 9
    rank_id[0] = 1
    ctx.taxonomy_load(child, parent)
    ctx.taxonomy_set_ranks(child, rank_id)
    order = {d + 1: len(RANKS) - d for d in range(len(RANKS))}
    f = lib.RankFilter.make(order=order, no_rank=[9], lower=order[6], discard_norank=True, save_norank=True)   # -N -n -L family

    n = a.records
    rows = []
    codes = torch.randint(0, 1 << 62, (n,), device=dev, generator=gen, dtype=torch.int64)
    tax = torch.randint(1, T + 1, (n,), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    out_t = torch.empty(n, dtype=torch.int32, device=dev)

    # ---- rfilter beside grep by taxid ----
    kept_ids = child[ctx.rank_pass(f, child) != 0]
    q = torch.from_numpy(kept_ids.view(np.int32)).to(dev)
    one = np.array([5], dtype=np.uint32)
    t_build, _ = timed(lambda: ctx.rank_pass(f, one))
    t_rf, r = timed(lambda: ctx.rfilter(codes, f, taxids=tax, out=out, out_taxids=out_t))
    kept = r[0].numel()
    first = r[0][:1000].clone()
    t_grep, g = timed(lambda: ctx.grep(codes, query_taxids=q, taxids=tax, out=out, out_taxids=out_t))
    assert g[0].numel() == kept and torch.equal(g[0][:1000], first), "ukm_rfilter and ukm_grep by taxid disagree"
    nbytes = 12 * n + 12 * kept
    rows.append({"call": "ukm_rfilter", "n": n, "taxonomy_nodes": T, "filter": "-N -n -L family", "kept": kept, "kept_share": kept / n,
                 "rfilter": t_rf, "grep_by_taxid": {**t_grep, "queries": int(len(kept_ids))}, "bitmap_build": t_build,
                 "ratio_grep_over_rfilter": t_grep["call_ms"] / t_rf["call_ms"], "algorithmic_bytes": nbytes,
                 "frac_of_8TBps": nbytes / (t_rf["call_ms"] * 1e-3) / 8e12})
    print(json.dumps(rows[-1]), flush=True)
    del q, g, r

    # ---- tsplit beside the pair sort it contains ----
    gt = torch.empty(n, dtype=torch.int32, device=dev)
    go = torch.empty(n + 1, dtype=torch.int64, device=dev)
    idx0 = torch.arange(n, device=dev, dtype=torch.int32)
    for label, taxids in (("whole tree", tax), ("1000 taxids", (tax.to(torch.int64) % 1000 + 1).to(torch.int32))):
        keys0 = taxids.to(torch.int64)
        sk, sv = torch.empty_like(keys0), torch.empty_like(idx0)

        def sort_pairs():
            sk.copy_(keys0)
            sv.copy_(idx0)
            torch.cuda.current_stream(dev).synchronize()
            return ctx.sort_pairs(sk, sv, 32)
        t_sort, _ = timed(sort_pairs)
        t_split, s = timed(lambda: ctx.tsplit(codes, taxids, out=out, group_taxids=gt, group_off=go))
        groups = s[1].numel()
        assert torch.equal(s[0][:1000], codes[sv[:1000].to(torch.int64)]), "ukm_tsplit and the pair sort disagree"
        rows.append({"call": "ukm_tsplit", "n": n, "taxids": label, "groups": groups, "tsplit": t_split,
                     "sort_pairs_key_bits_32": t_sort, "extra_ms": t_split["call_ms"] - t_sort["call_ms"],
                     "ratio_sort_over_tsplit": t_sort["call_ms"] / t_split["call_ms"]})
        print(json.dumps(rows[-1]), flush=True)
        del keys0, sk, sv, s

    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        except Exception:
            commit = "unknown"
    doc = {"tool": "tools/bench_taxsel.py", "commit": commit, "device": torch.cuda.get_device_name(0), "steps": a.steps,
           "warmup": a.warmup, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
