"""The alignment contract of include/unikmer_hip.h, for every entry point: a device pointer needs only the natural
alignment of its element type, results never depend on the address, and a call reads nothing as data and writes nothing
outside the arrays it was given.

A host that sub-allocates many decoded .unik files from one slab hands the library streams that start on
any 8-byte slot, taxids on any 4-byte slot, and that lie back to back.  Here all inputs of one call are packed that way:
every uint64 input into ONE int64 device tensor, every uint32 input into one int32 tensor, bases into one uint8 tensor.
Inside a tensor the arrays are separated only by the guard words that give each array the start residue the schedule
below prescribes, with SLACK elements in front of the first and behind the last array, so that no access which stays
inside an allocation elsewhere in the suite can leave one here.  Guard words and slack are hostile:

  - in front of a sorted code stream its first code, behind it its last code + 1 (stream_backs: where that value could
    not change the result, another one) -- a vector load that runs past a stream's end and is taken for data adds a record;
  - round a taxid array taxid 1, the root: folding it in changes the LCA;
  - round bases legal bases; round unsorted arrays (records, queries) the neighbouring values.

After every call the complete input tensors, guards included, are compared with their host image (the in-place sorts are
exempt on the array they sort), and every output is the middle of a test_gpu_capacity.Guarded buffer whose front guard
is FRONT + shift elements long.

The CPU twins at the top run without a GPU: the schedule reaches every residue the contract names for every array of
every case, the guards are hostile by the oracle's own word, and both checkers report a planted word.
"""
import functools

import numpy as np
import pytest

import test_gpu_capacity as CAP
from test_gpu_capacity import CASES, NAMES, Guarded, attempt, FRONT, SIGNED, U64, U32

U8 = np.uint8
SLACK = 128                       # elements in front of the first and behind the last array of a packed tensor
LAYOUTS = (0, 1, 2, 3)
ROOT_TAXID = 1
# The layout schedule.  SCHEDULE[dtype][layout][i % period]: where array i of a call (file i of an n-way call; outputs are
# numbered on behind the inputs) starts, in elements behind a 16-byte boundary.  Layout 0: everything 16-byte aligned.
# Layouts 1-3, keys: (i + layout) mod 2, both parities of the 8-byte slot, neighbouring files differ.  Taxids:
# 1 + (i + layout) mod 3 -- with layout 0 all four 4-byte residues, neighbouring files differ, and the keys and the taxids
# of one stream share a residue in at most one layout.  (Not (i + layout) mod 4: next to an all-aligned layout 0, three
# layouts reach four residues only when none of them is 0.)  Bytes: 1, 6, 11 in the same rotation: every residue mod 4 for
# bases; 0, 1 and 3 among them for uint8 outputs.
SCHEDULE = {
    np.dtype(U64): ((0, 0), (1, 0), (0, 1), (1, 0)),
    np.dtype(U32): ((0, 0, 0), (2, 3, 1), (3, 1, 2), (1, 2, 3)),
    np.dtype(U8): ((0, 0, 0), (6, 11, 1), (11, 1, 6), (1, 6, 11)),
}
INTERSECTING = ("setop2-inter", "inter-", "common-", "merge-repeated", "merge-chunk", "merge-pcommon")


def residue(dtype, i, layout):
    row = SCHEDULE[np.dtype(dtype)][layout]
    return row[i % len(row)]


# ---- the packing helper -------------------------------------------------------------------------------------------------------
def is_sorted(a):
    return len(a) < 2 or bool(np.all(a[1:] >= a[:-1]))


def guards(a, back=None):
    """(front, back) guard values of an input array; back: the value stream_backs chose for a sorted code stream"""
    if a.dtype == U32:
        return U32(ROOT_TAXID), U32(ROOT_TAXID)
    if a.dtype == U8 or len(a) == 0:
        return 0, 0                                                # (bases: the legal-base pattern of Pack.image)
    if is_sorted(a):
        return a[0], (U64(back) if back is not None else a[-1] + U64(1))
    return a[0], a[-1]


class Slot:
    def __init__(self, a, start, name, front, back):
        self.a, self.start, self.end, self.name, self.front, self.back = a, start, start + len(a), name, front, back


class Pack:
    """the inputs of one call under one layout"""

    def __init__(self, layout):
        self.layout = layout
        self.slots = {np.dtype(dt): [] for dt in (U64, U32, U8)}
        self.buf = {}

    def add(self, a, i, name, back=None, res=None):
        dt = a.dtype
        per = 16 // dt.itemsize
        prev = self.slots[dt][-1].end if self.slots[dt] else SLACK
        r = residue(dt, i, self.layout) if res is None else res
        s = Slot(a, prev + (r - prev) % per, name, *guards(a, back))
        self.slots[dt].append(s)
        return s

    def image(self, dt):
        """the host image of one tensor: slack, arrays and the guard words between them"""
        slots = self.slots[np.dtype(dt)]
        n = slots[-1].end + SLACK
        n += -n % (16 // np.dtype(dt).itemsize)
        if np.dtype(dt) == U8:
            img = np.frombuffer(b"ACGT", dtype=U8)[np.arange(n) % 4].copy()
        else:
            img = np.empty(n, dtype=dt)
            img[:slots[0].start] = slots[0].front
            for s, nxt in zip(slots, slots[1:] + [None]):
                img[s.end:nxt.start if nxt else n] = s.back          # (a gap belongs to the array in front of it)
        for s in slots:
            img[s.start:s.end] = s.a
        return img

    def materialise(self, place="device"):
        self.img = {dt: self.image(dt) for dt, slots in self.slots.items() if slots}
        for dt, img in self.img.items():
            if place == "device":
                import torch
                self.buf[dt] = torch.from_numpy(img.view(SIGNED[dt])).cuda()
                assert self.buf[dt].data_ptr() % 16 == 0
            else:
                self.buf[dt] = img.copy()
        if place == "device":
            torch.cuda.synchronize()
        return self

    def view(self, s):
        return self.buf[s.a.dtype][s.start:s.end]

    def check(self, what, exempt=()):
        """no call writes to an input: arrays, guard words and slack are what they were (exempt: arrays sorted in place)"""
        for dt, img in self.img.items():
            b = self.buf[dt]
            h = b.cpu().numpy().view(dt) if hasattr(b, "cpu") else b
            bad = np.flatnonzero(h != img)
            for s in exempt:
                if s.a.dtype == dt:
                    bad = bad[(bad < s.start) | (bad >= s.end)]
            if len(bad):
                at = int(bad[0])
                near = min(self.slots[dt], key=lambda s: 0 if s.start <= at < s.end else min(abs(at - s.start), abs(at - s.end + 1)))
                raise AssertionError("%s, layout %d: %d words of the %s inputs written, the first at %d (%s is [%d, %d))"
                                     % (what, self.layout, len(bad), dt, at, near.name, near.start, near.end))


def _placed(x):
    return isinstance(x, np.ndarray) and x.dtype in (U64, U32, U8)


def host_only(case):
    """positions of case.data() that the oracle alone uses: `ex` of the n-way cases, `wins` of locate / map"""
    d = case.data()
    if case.name.startswith(("locate", "map")):
        return {3}
    return {2} if isinstance(d[0], list) else set()


def stream_backs(case):
    """The back guard of every code stream of a 2-way / n-way case where it is not simply the stream's last code + 1:
    {name of the array: value}.  The intersecting operations: the largest last code of the call + 1 behind every stream.
    The differences: a later stream whose last code is the first stream's would carry the first stream's guard and cancel
    it; it gets its last code + 2."""
    d = case.data()
    if not (case.name.startswith("setop2") or isinstance(d[0], list)):
        return {}
    named = [("data[0][%d]" % i, s) for i, s in enumerate(d[0])] if isinstance(d[0], list) else [("data[0]", d[0]), ("data[1]", d[1])]
    if case.name.startswith(INTERSECTING):
        top = max(int(s.max()) for _, s in named) + 1
        return {n: top for n, s in named if is_sorted(s)}
    if case.name.startswith(("setop2-diff", "diff-")):
        first = int(named[0][1][-1])
        return {n: first + 2 for n, s in named[1:] if is_sorted(s) and int(s[-1]) == first}
    return {}


def place_case(case, layout):
    """Every array the call reads, by one rule over case.data(): a top-level array is array number i of its type, member i
    of a list is file i.  Returns (pack, slots) with slots shaped like data(): a Slot where an array was placed."""
    pack, keep, backs = Pack(layout), host_only(case), stream_backs(case)
    count = {np.dtype(dt): 0 for dt in (U64, U32, U8)}
    slots = []
    for p, x in enumerate(case.data()):
        if p in keep:
            slots.append(x)
        elif _placed(x):
            slots.append(pack.add(x, count[x.dtype], "data[%d]" % p, backs.get("data[%d]" % p)))
            count[x.dtype] += 1
        elif isinstance(x, (list, tuple)) and any(_placed(e) for e in x):
            slots.append([pack.add(e, i, "data[%d][%d]" % (p, i), backs.get("data[%d][%d]" % (p, i))) if _placed(e) else e
                          for i, e in enumerate(x)])
        else:
            slots.append(x)
    return pack, slots


def out_index(slots):
    """outputs are numbered on behind the uint64 inputs"""
    flat = [s for x in slots for s in (x if isinstance(x, list) else [x]) if isinstance(s, Slot)]
    return sum(1 for s in flat if s.a.dtype == U64)


def out_shifts(case, slots, layout):
    n0 = out_index(slots)
    return [residue(dt, n0 + o, layout) for o, dt in enumerate(case.dtypes)]


def device_data(pack, slots):
    sub = lambda s: pack.view(s) if isinstance(s, Slot) else s
    return tuple([sub(e) for e in x] if isinstance(x, list) else sub(x) for x in slots)


def key_taxid_pairs(case, slots):
    """(keys slot, taxids slot) of every stream that has both"""
    if isinstance(slots[0], list):
        return [(k, t) for k, t in zip(slots[0], slots[1] or []) if isinstance(t, Slot)]
    at = [(0, 2), (1, 3)] if case.name.startswith("setop2") else [(p - 1, p) for p in range(1, len(slots))]
    return [(slots[k], slots[t]) for k, t in at
            if isinstance(slots[k], Slot) and isinstance(slots[t], Slot) and slots[k].a.dtype == U64 and slots[t].a.dtype == U32]


# ---- CPU twins ----------------------------------------------------------------------------------------------------------------
WANT = {np.dtype(U64): {0, 8}, np.dtype(U32): {0, 4, 8, 12}}


def test_schedule_coverage():
    """from fake 512-byte aligned bases: every array of every case at every residue its type has, layout 0 all aligned,
    nothing overlaps, SLACK elements at both ends, neighbouring files apart, keys and taxids of a stream apart twice"""
    base = {np.dtype(U64): 512 * 1000, np.dtype(U32): 512 * 2000, np.dtype(U8): 512 * 3000, "out": 512 * 4000}
    for row in SCHEDULE[np.dtype(U8)]:
        assert {r % 4 for r in row} <= {0, 1, 2, 3}
    assert {0, 1, 3} <= {r % 4 for lay in SCHEDULE[np.dtype(U8)] for r in lay[:1]}          # a uint8 output: array 0 of its type
    for name in NAMES:
        case = CASES[name]
        seen, pair_diff, order = {}, {}, []
        for layout in LAYOUTS:
            pack, slots = place_case(case, layout)
            for dt, ss in pack.slots.items():
                if not ss:
                    continue
                n = len(pack.image(dt))
                assert ss[0].start >= SLACK and n - ss[-1].end >= SLACK, (name, layout, dt)
                for s, nxt in zip(ss, ss[1:]):
                    assert s.end <= nxt.start < s.end + 16 // dt.itemsize, (name, layout, s.name)
                for s in ss:
                    addr = base[dt] + s.start * dt.itemsize
                    assert addr % dt.itemsize == 0
                    seen.setdefault(s.name, (dt, set()))[1].add(addr % 16)
                    assert layout or addr % 16 == 0, (name, s.name)
            for o, (dt, sh) in enumerate(zip(case.dtypes, out_shifts(case, slots, layout))):
                addr = base["out"] + (FRONT + sh) * np.dtype(dt).itemsize
                seen.setdefault("out[%d]" % o, (np.dtype(dt), set()))[1].add(addr % 16)
                assert layout or addr % 16 == 0, (name, o)
            if layout and isinstance(slots[0], list):
                for p in (0, 1):
                    ss = slots[p] if isinstance(slots[p], list) else []
                    for a, b in zip(ss, ss[1:]):
                        if isinstance(a, Slot) and isinstance(b, Slot):
                            assert (a.start * a.a.itemsize) % 16 != (b.start * b.a.itemsize) % 16, (name, layout, a.name)
            pairs = key_taxid_pairs(case, slots)
            n0 = out_index(slots)
            if len(case.dtypes) == 2 and case.dtypes[1] == U32:
                pairs = pairs + [("out", residue(U64, n0, layout) * 8, residue(U32, n0 + 1, layout) * 4)]
            for pr in pairs:
                key, rk, rt = (pr[0].name, pr[0].start * 8 % 16, pr[1].start * 4 % 16) if isinstance(pr[0], Slot) else pr
                pair_diff[key] = pair_diff.get(key, 0) + (rk != rt)
        assert seen, name
        for what, (dt, res) in seen.items():
            if dt == U8:
                assert {r % 4 for r in res} == {0, 1, 2, 3}, (name, what, res)
            else:
                assert res == WANT[dt], (name, what, res)
        for what, d in pair_diff.items():
            assert d >= 2, (name, what, d)


def is_set_operation(case):
    return case.name.startswith("setop2") or isinstance(case.data()[0], list)


def extended(case, how):
    """the case's data with every stream made one record longer.  "keys": the back guard behind it as a record (with the
    guard taxid, where the stream has taxids per record); "taxid": the last code once more with the guard taxid"""
    d = list(case.data())
    backs = stream_backs(case)
    nway = isinstance(d[0], list)
    ks, ts = (list(d[0]), list(d[1]) if d[1] is not None else None) if nway else (list(d[:2]), list(d[2:4]))
    for i, k in enumerate(ks):
        more = guards(k, backs.get("data[0][%d]" % i if nway else "data[%d]" % i))[1] if how == "keys" else k[-1]
        ks[i] = np.append(k, more).astype(U64)
        if ts is not None and isinstance(ts[i], np.ndarray):
            ts[i] = np.append(ts[i], U32(ROOT_TAXID)).astype(U32)
    if nway:
        return ks, ts, CAP._expand(ks, ts)
    return ks + ts


def differs(a, b):
    return len(a) != len(b) or not np.array_equal(a, b)


@functools.lru_cache(None)
def hostile(name):
    """(a record read from behind a stream's end changes the result, a taxid read from there changes the taxids)"""
    case = CASES[name]
    O, tax, _ = CAP._oracle()
    exp = case.expected()

    def run(how):
        e = case._expect(O, tax, *extended(case, how))
        e = list(e) if isinstance(e, (tuple, list)) else [e]
        return [np.ascontiguousarray(a, dtype=dt) for a, dt in zip(e, case.dtypes)]
    by_keys = any(differs(g, e) for g, e in zip(run("keys"), exp))
    d = case.data()
    per_record = any(isinstance(t, np.ndarray) for t in ((d[1] or []) if isinstance(d[0], list) else d[2:4]))
    by_taxid = per_record and differs(run("taxid")[1], exp[1])
    return by_keys, by_taxid, per_record


SETOPS = [n for n in NAMES if n.startswith("setop2") or n.split("-")[0] in ("union", "merge", "inter", "diff", "common")]


def test_guards_are_hostile():
    """the oracle alone: a kernel that took a guard word for a record would not give expected().  Every 2-way and n-way
    case must notice through its keys or through its taxids"""
    assert all(is_set_operation(CASES[n]) for n in SETOPS) and not any(is_set_operation(CASES[n]) for n in NAMES if n not in SETOPS)
    quiet = []
    for name in SETOPS:
        by_keys, by_taxid, per_record = hostile(name)
        if not (by_keys or by_taxid):
            quiet.append(name)
    assert not quiet, quiet


def test_the_checkers_check():
    """on plain numpy buffers: a word at mid[-1] of a shifted Guarded and a word in an input guard are both reported"""
    g = Guarded(U64, 10, 10, "host", shift=1)
    assert len(g.buf) == FRONT + 1 + 10 + 64 and g.mid.ctypes.data - g.buf.ctypes.data == 8 * (FRONT + 1)
    g.check("untouched")
    g.mid[:] = 7
    g.check("the middle is the call's")
    g.buf[FRONT] = 7                                             # mid[-1]: the slot a 16-byte head store would take along
    with pytest.raises(AssertionError, match="1 guard words written, at offsets \\[-1\\]"):
        g.check("mid[-1]")
    g = Guarded(U8, 5, 5, "host", shift=3)
    g.buf[FRONT + 3 + 5] = 0
    with pytest.raises(AssertionError, match="at offsets \\[5\\]"):
        g.check("behind")

    a, t = np.arange(10, 20, dtype=U64), np.arange(1, 8, dtype=U32)
    for layout in LAYOUTS:
        pack = Pack(layout)
        sa, sb_, st = pack.add(a, 0, "a"), pack.add(a + U64(100), 1, "b"), pack.add(t, 0, "t")
        pack.materialise("host")
        assert np.array_equal(pack.view(sa), a) and np.array_equal(pack.view(st), t)
        assert pack.buf[np.dtype(U64)][sa.start - 1] == a[0] and pack.buf[np.dtype(U64)][sb_.end] == a[-1] + U64(101)
        assert pack.buf[np.dtype(U32)][st.end] == ROOT_TAXID
        pack.check("untouched")
        pack.buf[np.dtype(U64)][sa.start - 1] += U64(1)          # the guard word in front of a
        with pytest.raises(AssertionError, match="1 words of the uint64 inputs written"):
            pack.check("front guard")
        pack.buf[np.dtype(U64)][sa.start - 1] -= U64(1)
        pack.buf[np.dtype(U32)][st.end] = 9                      # the guard word behind t
        with pytest.raises(AssertionError, match="uint32 inputs written"):
            pack.check("back guard")
        pack.buf[np.dtype(U32)][st.end] = ROOT_TAXID
        pack.buf[np.dtype(U64)][sb_.start + 2] = 0               # an input itself ...
        with pytest.raises(AssertionError):
            pack.check("input")
        pack.check("sorted in place", exempt=[sb_])              # ... unless the call sorts it in place


# ---- the case table on the device ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def env():
    from unikmer_amd import lib as L
    from conftest import synth_tree
    ctx = L.Context(0)
    ctx.taxonomy_load(*synth_tree(5, 8))
    yield ctx, L
    ctx.close()


def run_layout(ctx, L, case, layout, caps, opts):
    pack, slots = place_case(case, layout)
    pack.materialise()
    data = device_data(pack, slots)
    shifts = out_shifts(case, slots, layout)
    if isinstance(data[0], list) and len(data[0]) >= 64 and not case.name.startswith("merge"):
        assert ctx._nway_args(data[0], data[1])[6][-1] == "device"      # the binding's table path for many device tensors
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        for cap in caps:
            attempt(ctx, L, case, cap, "device", shifts=shifts, data=data)
            pack.check("%s, out_cap = %d" % (case.name, cap))
    finally:
        for k in opts:
            ctx.set_option(k, None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_alignment(env, name, monkeypatch):
    """one case under the four layouts at out_cap = need; the tiled cases before that at tile + 1 (the failing, guarded store
    path at an odd address) and once more at layout 3 with ticketed tiles; union-tree-* and inter-pfold-* also without
    UKM_F_DEVICE_STREAMS, so that the library classifies the interior pointers itself"""
    ctx, L = env
    case = CASES[name]
    need = len(case.expected()[0])
    caps = ([case.tile + 1] if case.tile else []) + [need]
    for layout in LAYOUTS:
        run_layout(ctx, L, case, layout, caps, case.opts)
    if case.tile:
        run_layout(ctx, L, case, 3, caps, dict(case.opts, force_ticket=1))
    if name.startswith(("union-tree-", "inter-pfold-")):
        monkeypatch.setenv("UKM_PY_NO_DEVICE_FLAG", "1")
        for layout in LAYOUTS:
            run_layout(ctx, L, case, layout, caps, case.opts)


# ---- entry points the table lacks ---------------------------------------------------------------------------------------------
def _host(t, dt):
    return t.cpu().numpy().view(dt)


@pytest.mark.gpu
@pytest.mark.parametrize("n,bits,opts", [(100_003, 42, {}), (1 << 23, 64, {"sort_counting": 1})], ids=["host-hist", "lds-buckets"])
def test_sort_u64(n, bits, opts):
    """in place on an interior view: the host-histogram route and, from SORT_LOCAL_MIN, the LDS bucket route"""
    from unikmer_amd import lib as L
    from test_gpu_workspace import SORT_LOCAL_MIN
    assert (n >= SORT_LOCAL_MIN) == bool(opts) and n <= SORT_LOCAL_MIN
    x = np.random.default_rng(n).integers(0, 1 << bits, n, dtype=U64)
    x[::7][:len(x[1::7])] = x[1::7]
    want = np.sort(x)
    ctx = L.Context(0)            # (a context of its own: the sort keeps state from one call to the next)
    try:
        for k, v in opts.items():
            ctx.set_option(k, v)
        for layout in LAYOUTS:
            pack = Pack(layout)
            s = pack.add(x, 0, "keys")
            pack.materialise()
            ctx.sort_u64(pack.view(s), bits)
            assert np.array_equal(_host(pack.view(s), U64), want), layout
            pack.check("ukm_sort_u64", exempt=[s])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_sort_pairs(env):
    ctx, L = env
    n, bits = 100_003, 42
    x = np.random.default_rng(3).integers(0, 1 << bits, n, dtype=U64)
    x[::7][:len(x[1::7])] = x[1::7]
    order = np.argsort(x, kind="stable")
    for layout in LAYOUTS:
        pack = Pack(layout)
        sk, sv = pack.add(x, 0, "keys"), pack.add(np.arange(n, dtype=U32), 2, "payload")
        assert layout == 0 or sk.start * 8 % 16 != sv.start * 4 % 16
        pack.materialise()
        ctx.sort_pairs(pack.view(sk), pack.view(sv), bits)
        assert np.array_equal(_host(pack.view(sk), U64), x[order]) and np.array_equal(_host(pack.view(sv), U32), order.astype(U32)), layout
        pack.check("ukm_sort_pairs", exempt=[sk, sv])


@pytest.mark.gpu
def test_lca(env):
    ctx, L = env
    O, tax, T = CAP._oracle()
    n = 5000
    rng = np.random.default_rng(9)
    a, b = rng.integers(0, T + 2, n).astype(U32), rng.integers(0, T + 2, n).astype(U32)
    want = np.array([tax.lca(x, y) for x, y in zip(a.tolist(), b.tolist())], dtype=U32)
    for layout in LAYOUTS:
        pack = Pack(layout)
        sa, sb_ = pack.add(a, 0, "a"), pack.add(b, 1, "b")
        pack.materialise()
        out = Guarded(U32, n, n, "device", shift=residue(U32, 2, layout))
        assert layout == 0 or len({sa.start % 4, sb_.start % 4, out.front % 4}) == 3
        ctx.lca(pack.view(sa), pack.view(sb_), out=out.mid)
        out.check("ukm_lca, layout %d" % layout)
        assert np.array_equal(out.head(n), want), layout
        pack.check("ukm_lca")


@pytest.fixture(scope="module")
def ranked():
    import test_gpu_taxsel as TS
    from unikmer_amd import lib as L
    ctx = L.Context(0)
    TS.load_tax(ctx)
    yield ctx, L, TS
    ctx.close()


@pytest.mark.gpu
def test_rank_pass_and_rfilter(ranked):
    ctx, L, TS = ranked
    from test_taxsel_cpu import FILTERS, to_rank_filter
    n = 3 * TS.TILE + 5
    codes, tax = TS.records(n, 3)
    for layout in LAYOUTS:
        pack = Pack(layout)
        sk, st = pack.add(codes, 0, "keys"), pack.add(tax, 0, "taxids")
        pack.materialise()
        for name in sorted(FILTERS):
            keep = TS.model_mask(name, tax)
            f = to_rank_filter(L, FILTERS[name])
            what = "filter %s, layout %d" % (name, layout)
            bits = Guarded(U8, n, n, "device", shift=residue(U8, 0, layout))
            ctx.rank_pass(f, pack.view(st), out=bits.mid)
            bits.check("ukm_rank_pass, " + what)
            assert np.array_equal(bits.head(n), keep.astype(U8)), what
            need = int(keep.sum())
            ok = Guarded(U64, need, n, "device", shift=residue(U64, 1, layout))
            ot = Guarded(U32, need, n, "device", shift=residue(U32, 1, layout))
            gk, gt = ctx.rfilter(pack.view(sk), f, taxids=pack.view(st), out=ok.mid, out_taxids=ot.mid)
            ok.check("ukm_rfilter keys, " + what)
            ot.check("ukm_rfilter taxids, " + what)
            assert len(gk) == need and np.array_equal(ok.head(need), codes[keep]) and np.array_equal(ot.head(need), tax[keep]), what
            pack.check("ukm_rank_pass / ukm_rfilter, " + what)
    assert {residue(U8, 0, layout) % 4 for layout in LAYOUTS} >= {0, 1, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["37", "boundaries"])
def test_tsplit(ranked, pattern):
    ctx, L, TS = ranked
    n = 3 * TS.TILE + 5
    codes, tax = TS.split_case(n, pattern)
    wk, wt, wo = TS.model_split(codes, tax)
    g = len(wt)
    for layout in LAYOUTS:
        pack = Pack(layout)
        sk, st = pack.add(codes, 0, "keys"), pack.add(tax, 0, "taxids")
        pack.materialise()
        ok = Guarded(U64, n, n, "device", shift=residue(U64, 1, layout))
        gt = Guarded(U32, g, g, "device", shift=residue(U32, 1, layout))
        go = Guarded(U64, g + 1, g + 1, "device", shift=residue(U64, 2, layout))
        ctx.tsplit(pack.view(sk), pack.view(st), out=ok.mid, group_taxids=gt.mid, group_off=go.mid)
        for b, what in ((ok, "out_keys"), (gt, "group_taxids"), (go, "group_off")):
            b.check("ukm_tsplit %s, layout %d" % (what, layout))
        assert np.array_equal(ok.head(n), wk) and np.array_equal(gt.head(g), wt) and np.array_equal(go.head(g + 1), wo), layout
        pack.check("ukm_tsplit")


@pytest.mark.gpu
def test_partition_points(env):
    ctx, L = env
    A = CAP._universe(100_000)
    sp = np.array([0, A[10], A[10] + U64(1), A[-1], 2 ** 63], dtype=U64)
    want = np.searchsorted(A, sp, side="left").astype(U64)
    for layout in LAYOUTS:
        pack = Pack(layout)
        sa, ss = pack.add(A, 0, "keys"), pack.add(sp, 1, "splitters")
        pack.materialise()
        assert layout % 2 == 0 or sa.start % 2 == 1                  # the keys on an odd slot
        cuts = Guarded(U64, len(sp), len(sp), "device", shift=residue(U64, 2, layout))
        ctx.partition_points(pack.view(sa), pack.view(ss), out=cuts.mid)
        cuts.check("ukm_partition_points, layout %d" % layout)
        assert np.array_equal(cuts.head(len(sp)), want), layout
        pack.check("ukm_partition_points")


@pytest.mark.gpu
def test_setop2_cached_tables_on_odd_slots(monkeypatch):
    """309 plain tiles, inputs and output on odd 8-byte slots: union searches and looks back, inter and diff run from the
    verified partition and the match-count table of the call before them"""
    import test_gpu_part_reuse as PR
    from unikmer_amd import lib as L
    monkeypatch.setenv("UKM_SETOP_OFFS_OPS", "7")
    A, B = PR._sets()
    pack = Pack(1)
    sa, sb_ = pack.add(A, 0, "A", res=1), pack.add(B, 1, "B", res=1)
    pack.materialise()
    a, b = pack.view(sa), pack.view(sb_)
    assert a.data_ptr() % 16 == 8 and b.data_ptr() % 16 == 8
    ctx = L.Context(0)
    try:
        for k, op in enumerate((PR.OP_UNION, PR.OP_INTER, PR.OP_DIFF)):
            want = PR._ref(op)
            out = Guarded(U64, len(want), len(A) + len(B), "device", shift=1)
            assert out.mid.data_ptr() % 16 == 8
            got = ctx.setop2(op, a, b, out=out.mid)
            out.check("ukm_setop2 op %d" % op)
            assert len(got) == len(want) and np.array_equal(out.head(len(want)), want), op
            assert (ctx.stat("setop_part_hits"), ctx.stat("setop_part_stale"), ctx.stat("setop_offs_hits"), ctx.stat("setop_offs_stale")) == (k, 0, k, 0)
            pack.check("ukm_setop2 op %d" % op)
    finally:
        ctx.close()
