"""Kernel-only times of the window kernels on n bases in `nrec` records: every window (encode k=31, ntHash k=51: stripwin_kernel),
the Scaled-MinHash sketch at --scale 1000 (ntHash k=51: nthash_strip_kernel, and window_kernel<true, true> with the option
nthash_strip = 0) and the minimizer sketch (k=31, w=15: the ntHash pass + minimizer_kernel).  Every case asserts the
statistic "window_route", so that a time is never attributed to another kernel than the one named here.
Usage: python tools/win_bench.py [--n 1e8] [--nrec 100] [--json PATH]"""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench
from unikmer_amd import lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=float, default=1e8)
ap.add_argument("--nrec", type=int, default=100)
ap.add_argument("--k", type=int, default=31)
ap.add_argument("--kh", type=int, default=51)
ap.add_argument("--w", type=int, default=15)
ap.add_argument("--scale", type=int, default=1000)
ap.add_argument("--json", default=None, help="write the result to this file as well")
a = ap.parse_args()
n = int(a.n)
dev = torch.device("cuda:0")
ctx = L.Context(0)
i = torch.arange(n, dtype=torch.int64, device=dev)
w = bench.splitmix64_torch((i >> 5) ^ bench._i64(bench.SEED))
bases = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)[(w >> (2 * (i & 31))) & 3]
del i, w
off = torch.tensor([n * r // a.nrec for r in range(a.nrec + 1)], dtype=torch.int64, device=dev)
out = torch.empty(n, dtype=torch.int64, device=dev)
mh = ctx.max_hash(a.scale)
ROUTE_WINDOW, ROUTE_STRIPWIN, ROUTE_NTSTRIP = 1, 2, 3   # the values of the statistic "window_route"
# name, call, the route that must have answered, context options for the call
CASES = (("encode_k31", lambda: ctx.encode_kmers(bases, off, a.k, out=out), ROUTE_STRIPWIN, {}),
         ("nthash_k51", lambda: ctx.nthash(bases, off, a.kh, out=out), ROUTE_STRIPWIN, {}),
         ("nthash_k51_scaled_strip", lambda: ctx.nthash(bases, off, a.kh, max_hash=mh, out=out), ROUTE_NTSTRIP, {}),
         ("nthash_k51_scaled_window", lambda: ctx.nthash(bases, off, a.kh, max_hash=mh, out=out), ROUTE_WINDOW, {"nthash_strip": 0}),
         ("minimizer_k31_w15", lambda: ctx.minimizer(bases, off, a.k, a.w, out=out), ROUTE_STRIPWIN, {}))   # (the route of its ntHash pass)
res = {}
for name, fn, route, opts in CASES:
    for key, v in opts.items():
        ctx.set_option(key, v)
    ks, cs = [], []
    for rep in range(2 + 7):    # two calls to warm up (code objects, the workspace), seven timed
        n_out = len(fn())
        assert ctx.stat("window_route") == route, (name, ctx.stat("window_route"), route)
        if rep >= 2:
            ks.append(ctx.last_kernel_ms())
            cs.append(ctx.last_call_ms())
    for key in opts:
        ctx.set_option(key, None)
    res[name] = {"kernel_ms": min(ks), "kernel_ms_median": statistics.median(ks), "call_ms": min(cs), "n_out": n_out, "window_route": route}
    if n_out == n - a.nrec * ((a.kh if "nthash" in name else a.k) - 1):     # every window written: 1 byte read, 8 written per base
        res[name]["GBps"] = 9 * n / min(ks) / 1e6
print(json.dumps(res))
if a.json:
    with open(a.json, "w") as fh:
        json.dump(res, fh, indent=1)
