"""The record-staging step that every entry point over (bases, rec_off) starts with: rec_off[0] must be 0.

One record of 40 bases handed over as rec_off = [1, 40] is UKM_ERR_INVALID with the message "<C entry>: rec_off[0] must be 0",
from every entry point and for rec_off as a host array and as a device tensor (the library reads rec_off[n_rec] and
rec_off[0] back from the device there); no kernel has run by then.  The same context then answers the valid call,
rec_off = [0, 40], with the oracle's result.  Expected values of locate / map come from the model of test_gpu_map.py.
"""
import numpy as np
import pytest

from test_gpu_map import model_locate, model_map, windows

pytestmark = pytest.mark.gpu

K, W, NB = 5, 3, 40
U64 = np.uint64


@pytest.fixture(scope="module")
def env():
    from unikmer_amd import lib
    from oracle import oracle
    ctx = lib.Context(0)
    yield lib, ctx, oracle
    ctx.close()


@pytest.fixture(scope="module")
def rec(env):
    """the record, its windows from the oracle's iterator, the queries of locate and the sorted set of map"""
    O = env[2]
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(40).integers(0, 4, NB)].copy()
    off = np.array([0, NB], dtype=U64)
    wins = windows(O, seq, off, K)
    allw = np.array(wins[0], dtype=U64)
    return seq, off, wins, allw[::3].copy(), np.unique(allw[(np.arange(len(allw)) // 6) % 2 == 0])


def _place(x, form):
    if form == "host":
        return x
    import torch
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x.view(np.int64) if x.dtype == U64 else x).cuda()


def _host(t):
    return t.cpu().numpy().view({8: U64, 4: np.uint32}[t.element_size()]) if hasattr(t, "cpu") else t


def _cols(res):
    return [_host(c).astype(np.int64).tolist() for c in res]


def _rows(rows):
    return [[r[i] for r in rows] for i in range(3)]


# name of the C entry -> (the call, the oracle's answer for the valid record)
ENTRIES = {
    "ukm_encode_kmers": (lambda ctx, b, o, q, s: ctx.encode_kmers(b, o, K),
                         lambda O, seq, off, wins, q, s: O.count_windows(seq, off, K)),
    "ukm_nthash": (lambda ctx, b, o, q, s: ctx.nthash(b, o, K),
                   lambda O, seq, off, wins, q, s: O.count_windows(seq, off, K, hashed=True)),
    "ukm_minimizer": (lambda ctx, b, o, q, s: ctx.minimizer(b, o, K, W),
                      lambda O, seq, off, wins, q, s: O.minimizer(seq, K, W)[0]),
    "ukm_count": (lambda ctx, b, o, q, s: ctx.count(b, o, K),
                  lambda O, seq, off, wins, q, s: O.unique(O.sort_u64(O.count_windows(seq, off, K)))),
    "ukm_locate": (lambda ctx, b, o, q, s: ctx.locate(b, o, K, q),
                   lambda O, seq, off, wins, q, s: _rows(model_locate(wins, q.tolist()))),
    "ukm_map": (lambda ctx, b, o, q, s: ctx.map(b, o, None, K, s, allow_multi=True, min_len=K),
                lambda O, seq, off, wins, q, s: _rows(model_map(wins, [0], s.tolist(), K, True, K))),
    # (without gaps on linear records ukm_map_gapped is ukm_map: tests/test_gpu_map_gapped.py)
    "ukm_map_gapped": (lambda ctx, b, o, q, s: ctx.map_gapped(b, o, None, K, s, allow_multi=True, min_len=K),
                       lambda O, seq, off, wins, q, s: _rows(model_map(wins, [0], s.tolist(), K, True, K))),
}


@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_rec_off_must_start_at_zero(env, rec, entry, form):
    L, ctx, O = env
    seq, off, wins, q, s = rec
    call, expect = ENTRIES[entry]
    b, qd, sd = _place(seq, form), _place(q, form), _place(s, form)
    with pytest.raises(L.UkmError) as e:
        call(ctx, b, _place(np.array([1, NB], dtype=U64), form), qd, sd)
    assert e.value.code == L.ERR_INVALID, e.value
    assert "rec_off[0] must be 0" in str(e.value) and entry + ":" in str(e.value), e.value
    # the same context, straight after
    got = call(ctx, b, _place(off, form), qd, sd)
    want = expect(O, seq, off, wins, q, s)
    if isinstance(got, tuple):
        assert len(want[0]) > 0 and _cols(got) == want
    else:
        assert len(want) > 0 and np.array_equal(_host(got), want)
