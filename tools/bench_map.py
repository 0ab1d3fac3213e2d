#!/usr/bin/env python3
"""ukm_map / ukm_locate on a synthetic genome against what a user would do today with torch on the same device.

    python tools/bench_map.py [--bases 100000000] [--sets 1000000,100000000] [--queries 10000000] [--out profiles/map_locate.json]

Genome: ONE record of uniformly random ACGT (seeded), k = 31.  A set of n codes is half windows of the genome (every
second one / a random sample) and half random codes, sorted and distinct, so about half of it can hit.  Timed with the
context's own event timers (ukm_last_call_ms: all device work of the call; ukm_last_kernel_ms: the join kernel), median of
--steps calls behind --warmup calls.  Both calls are timed on both routes -- option "map_sorted" 0 (lookups in genome order;
ukm_map sorts only the hits) and 1 (every (code, window) pair sorted, the sorted array looked up in sorted order) -- and as
the library chooses itself (`route_default`).

The torch side is MEMBERSHIP only -- torch.searchsorted of the precomputed windows in the sorted set plus a gather-compare,
torch events around it -- which is less than the call does (no windows, no multiple-mapped filter, no runs); `ratio_call` =
(ukm_encode_kmers call + torch membership) / ukm call on the default route, `ratio_join` = torch membership / join kernel.

Bytes are counted from the shapes (see `algorithmic_bytes`), the fraction is bytes / call time / 8 TB/s as in DESIGN.md.

    python tools/bench_map.py --gapped [--parent-lib path/to/libunikmer_hip.so] [--sets 1000000,10000000,100000000]

writes profiles/map_gapped.json instead: per set size ukm_map_gapped at x = 0, at x = 3 X = 2, and at x = 3 X = 2 with
circular = 1 (allow_multi 0, min_len 200, the last two also at min_len 33, where regions come out; each the median of three ukm_last_call_ms behind one warm-up call, all three kept), and
ukm_map from this tree beside ukm_map from --parent-lib (the library of the parent commit, built elsewhere; loaded with plain
ctypes next to this tree's, the two timed alternately on the same inputs in the same process).
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


def algorithmic_bytes(kind, n_bases, n_win, n_keys, n_hits, n_out, allow_multi):
    """what the chosen route has to move, from the shapes: bases read once; windows written and read once (8 B each way);
    per window one directory entry pair (8 B) and one code of the sorted array (8 B); ukm_map: a flag byte written and read
    per window, without allow_multi the hits compacted (12 B), sorted (8 one-byte digit passes over 62 bits, 12 B read +
    12 B written each) and read again (12 B); ukm_locate: the queries sorted (8 passes over 64 bits), the hits compacted,
    sorted by query index (ceil(log2(nq) / 8) passes) and expanded (12 B read, 20 B written); results 20 B each."""
    b = n_bases + 16 * n_win + 16 * n_win
    if kind == "map":
        b += 2 * n_win
        if not allow_multi:
            b += 12 * n_hits + 8 * 24 * n_hits + 12 * n_hits
        b += 20 * n_out
    else:
        qpasses = -(-max(1, int(n_keys).bit_length()) // 8)
        b += 8 * 24 * n_keys + 12 * n_hits + qpasses * 24 * n_hits + 12 * n_hits + 20 * n_out
    return int(b)


def raw_map_library(path, stream):
    """ukm_map of ANOTHER build of the library through plain ctypes (its binding may not know this tree's symbols)"""
    import ctypes as C
    L = C.CDLL(path)
    vp, u64, i32 = C.c_void_p, C.c_uint64, C.c_int
    L.ukm_ctx_create.argtypes = [i32, C.POINTER(vp)]
    L.ukm_ctx_set_stream.argtypes = [vp, vp]
    L.ukm_ctx_destroy.argtypes = [vp]
    L.ukm_last_call_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.ukm_map.argtypes = [vp, vp, vp, u64, vp, u64, i32, i32, vp, u64, i32, u64, vp, vp, vp, u64, C.POINTER(u64)]
    h = vp()
    assert L.ukm_ctx_create(0, C.byref(h)) == 0
    assert L.ukm_ctx_set_stream(h, vp(stream)) == 0

    def call(bases, off, goff, S, allow, min_len, outs):
        n = u64()
        rc = L.ukm_map(h, bases.data_ptr(), off.data_ptr(), off.numel() - 1, goff.data_ptr(), goff.numel() - 1, K, 0, S.data_ptr(), S.numel(),
                       allow, min_len, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[0].numel(), C.byref(n))
        assert rc == 0, rc
        ms = C.c_float()
        assert L.ukm_last_call_ms(h, C.byref(ms)) == 0
        return ms.value, n.value
    return call, lambda: L.ukm_ctx_destroy(h)


def gapped(a, torch, lib, ctx, dev, bases, off, goff, W, make_set):
    """the rows of profiles/map_gapped.json (module docstring)"""
    stream = torch.cuda.current_stream(dev).cuda_stream
    parent, parent_close = raw_map_library(a.parent_lib, stream) if a.parent_lib else (None, None)
    REPEATS = 3
    rows = []
    for n in [int(x) for x in a.sets.split(",") if x]:
        S = make_set(n)
        row = {"n_bases": a.bases, "k": K, "n_windows": W.numel(), "n_set": S.numel(), "allow_multi": 0, "min_len": 200}

        def three(fn):
            fn()
            ms = []
            for _ in range(REPEATS):
                r = fn()
                ms.append(ctx.last_call_ms())
            return {"call_ms": statistics.median(ms), "call_ms_all": ms}, r
        # (min_len 200 keeps no region on this input -- its runs are single windows; K + 2 keeps the groups of three runs)
        for name, kw in (("gapped_x0", dict(max_gap_size=0, max_gap_num=0)), ("gapped_x3_X2", dict(max_gap_size=3, max_gap_num=2)),
                         ("gapped_x3_X2_circular", dict(max_gap_size=3, max_gap_num=2, circular=True)),
                         ("gapped_x3_X2_min_len_33", dict(max_gap_size=3, max_gap_num=2, min_len=K + 2)),
                         ("gapped_x3_X2_circular_min_len_33", dict(max_gap_size=3, max_gap_num=2, circular=True, min_len=K + 2))):
            kw = dict(dict(min_len=200), **kw)
            first = ctx.map_gapped(bases, off, goff, K, S, **kw)
            cap = max(1, first[0].numel())
            row[name], r = three(lambda: ctx.map_gapped(bases, off, goff, K, S, out_cap=cap, **kw))
            row[name]["regions"] = r[0].numel()
        # ukm_map of this tree and of the parent, alternately: warm-up each, then head, parent, head, parent, head, parent
        first = ctx.map(bases, off, goff, K, S, min_len=200)
        cap = max(1, first[0].numel())
        outs = [torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int64, device=dev), torch.empty(cap, dtype=torch.int64, device=dev)]
        head_ms, parent_ms = [], []
        for i in range(REPEATS + 1):
            r = ctx.map(bases, off, goff, K, S, min_len=200, out_cap=cap)
            if i:
                head_ms.append(ctx.last_call_ms())
            if parent:
                ms, cnt = parent(bases, off, goff, S, 0, 200, outs)
                assert cnt == r[0].numel() and all(torch.equal(x, y[:cnt]) for x, y in zip(r, outs)), "ukm_map differs from the parent's"
                if i:
                    parent_ms.append(ms)
        assert all(torch.equal(x, y) for x, y in zip(r, ctx.map_gapped(bases, off, goff, K, S, min_len=200))), "x = 0 is not ukm_map"
        row["ukm_map"] = {"call_ms": statistics.median(head_ms), "call_ms_all": head_ms, "regions": r[0].numel()}
        if parent:
            row["ukm_map_parent"] = {"call_ms": statistics.median(parent_ms), "call_ms_all": parent_ms}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del S
    if parent:
        parent_close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=100_000_000)
    ap.add_argument("--sets", default="1000000,100000000")
    ap.add_argument("--queries", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--commit", default=None, help="what to record as the commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=None, help="default: profiles/map_locate.json, with --gapped profiles/map_gapped.json")
    ap.add_argument("--gapped", action="store_true", help="the ukm_map_gapped rows instead (module docstring)")
    ap.add_argument("--parent-lib", default=None, help="--gapped: a libunikmer_hip.so of the parent commit to time ukm_map of")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "map_gapped.json" if a.gapped else "map_locate.json")
    if a.gapped and a.sets == "1000000,100000000":
        a.sets = "1000000,10000000,100000000"

    import torch
    from unikmer_amd import lib
    if not torch.cuda.is_available():
        raise SystemExit("bench_map.py needs the GPU: there is no CPU path to time")
    dev = torch.device("cuda", 0)
    ctx = lib.Context(0, stream=torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(20240917)
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    bases = acgt[torch.randint(0, 4, (a.bases,), device=dev, generator=gen)]
    off = torch.tensor([0, a.bases], dtype=torch.int64, device=dev)
    goff = torch.tensor([0, 1], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def timed(fn):
        """median / min of ukm_last_call_ms and ukm_last_kernel_ms over the timed calls; the last result"""
        for _ in range(a.warmup):
            r = fn()
        call, kern = [], []
        for _ in range(a.steps):
            r = fn()
            call.append(ctx.last_call_ms())
            kern.append(ctx.last_kernel_ms())
        return {"call_ms": statistics.median(call), "call_ms_min": min(call), "kernel_ms": statistics.median(kern)}, r

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
        return statistics.median(ts), r

    enc, W = timed(lambda: ctx.encode_kmers(bases, off, K))
    n_win = W.numel()

    def membership(S):
        def f():
            idx = torch.searchsorted(S, W)
            idx.clamp_(max=S.numel() - 1)
            return (S[idx] == W).sum()
        return f

    def make_set(n):
        half = n // 2
        own = W[::2][:half] if half * 2 >= n_win // 2 else W[torch.randint(0, n_win, (half,), device=dev, generator=gen)]
        rnd = torch.randint(0, 1 << (2 * K), (n - own.numel(),), device=dev, generator=gen, dtype=torch.int64)
        return torch.unique(torch.cat([own, rnd]))      # sorted, distinct (codes < 2^62: signed order = unsigned order)

    def write(rows, formula):
        commit = a.commit
        if commit is None:
            try:
                commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
            except Exception:
                commit = "unknown"
        doc = {"tool": "tools/bench_map.py" + (" --gapped" if a.gapped else ""), "commit": commit, "device": torch.cuda.get_device_name(0),
               "peak_bytes_per_s": PEAK, "steps": 3 if a.gapped else a.steps, "warmup": 1 if a.gapped else a.warmup, "bytes_formula": formula,
               "rows": rows}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")
        ctx.close()

    if a.gapped:
        write(gapped(a, torch, lib, ctx, dev, bases, off, goff, W, make_set), None)
        return

    rows = []
    for n in [int(x) for x in a.sets.split(",") if x]:
        S = make_set(n)
        t_ms, hits = torch_ms(membership(S))
        hits = int(hits.item())
        for allow in (1, 0):
            res = {}
            for route in ("join", "sorted", "default"):
                ctx.set_option("map_sorted", {"join": 0, "sorted": 1, "default": None}[route])
                try:
                    first = ctx.map(bases, off, goff, K, S, allow_multi=allow, min_len=200)
                    cap = max(1, first[0].numel())
                    t, r = timed(lambda: ctx.map(bases, off, goff, K, S, allow_multi=allow, min_len=200, out_cap=cap))
                finally:
                    ctx.set_option("map_sorted", None)
                res[route] = (t, r)
            (tj, rj), (ts_, rs), (td, rd) = res["join"], res["sorted"], res["default"]
            assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(rj, rs, rd)), "the routes disagree"
            nbytes = algorithmic_bytes("map", a.bases, n_win, S.numel(), hits, rj[0].numel(), allow)
            rows.append({"call": "ukm_map", "n_bases": a.bases, "k": K, "n_windows": n_win, "n_set": S.numel(), "windows_in_set": hits,
                         "allow_multi": allow, "min_len": 200, "regions": rj[0].numel(),
                         "route_join": tj, "route_sorted": ts_, "route_default": td, "algorithmic_bytes": nbytes,
                         "frac_of_8TBps": nbytes / (td["call_ms"] * 1e-3) / PEAK,
                         "torch_membership_ms": t_ms, "ukm_encode_call_ms": enc["call_ms"],
                         "ratio_call": (enc["call_ms"] + t_ms) / td["call_ms"], "ratio_join": t_ms / tj["kernel_ms"]})
            print(json.dumps(rows[-1]), flush=True)
        del S

    # locate: queries half windows of the genome, half random, in random order
    nq = a.queries
    own = W[torch.randint(0, n_win, (nq // 2,), device=dev, generator=gen)]
    rnd = torch.randint(0, 1 << (2 * K), (nq - own.numel(),), device=dev, generator=gen, dtype=torch.int64)
    Q = torch.cat([own, rnd])[torch.randperm(nq, device=dev, generator=gen)]
    Qs = torch.sort(Q).values
    t_ms, hits = torch_ms(membership(Qs))
    hits = int(hits.item())
    first = ctx.locate(bases, off, K, Q)
    cap = max(1, first[0].numel())
    assert cap == hits, (cap, hits)
    res = {}
    for route in ("join", "sorted", "default"):
        ctx.set_option("map_sorted", {"join": 0, "sorted": 1, "default": None}[route])
        try:
            res[route] = timed(lambda: ctx.locate(bases, off, K, Q, out_cap=cap))
        finally:
            ctx.set_option("map_sorted", None)
    (tl, rl), (ts_, rs), (td, rd) = res["join"], res["sorted"], res["default"]
    assert all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(rl, rs, rd)), "the routes disagree"
    nbytes = algorithmic_bytes("locate", a.bases, n_win, nq, hits, hits, 1)
    rows.append({"call": "ukm_locate", "n_bases": a.bases, "k": K, "n_windows": n_win, "n_queries": nq, "entries": hits,
                 "route_join": tl, "route_sorted": ts_, "route_default": td, "algorithmic_bytes": nbytes,
                 "frac_of_8TBps": nbytes / (td["call_ms"] * 1e-3) / PEAK,
                 "torch_membership_ms": t_ms, "ukm_encode_call_ms": enc["call_ms"],
                 "ratio_call": (enc["call_ms"] + t_ms) / td["call_ms"], "ratio_join": t_ms / tl["kernel_ms"]})
    print(json.dumps(rows[-1]), flush=True)

    write(rows, algorithmic_bytes.__doc__)


if __name__ == "__main__":
    main()
