"""`rfilter` / `tsplit`: what can be checked without a GPU -- the five entry points exist in header, binding and library,
ukm_rank_filter_plan (a pure host function) agrees with the model for every rank id, `--help` lists the commands, bad
invocations are refused with the reference's messages before a device context is created, and `rfilter --list-order`
prints the rank file back.

The model -- isPassed (rfilter.go:438-520) restated over plain dicts -- lives here; tests/test_gpu_taxsel.py uses the same
functions for the device results.  Expected values never come from the library.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "unikmer_amd", "bin", "unikmer")
NEW = ("ukm_taxonomy_set_ranks", "ukm_rank_filter_plan", "ukm_rank_pass", "ukm_rfilter", "ukm_tsplit")

# ---- the model -----------------------------------------------------------------------------------------------------------
# the ordered ranks of the tests, highest first (the rank file's order), and the ranks without order
RANKS = ["domain", "kingdom", "phylum", "class", "order", "family", "genus", "species", "subspecies", "varietas", "forma", "strain"]
NORANKS = ["no rank", "clade"]
ORDER = {r: len(RANKS) - i for i, r in enumerate(RANKS)}      # readRankOrderFromFile: the LAST line has order 1
# rank ids as a host would hand them out (any numbering will do): 1.., with id 255 in use
RANK_IDS = {r: i + 1 for i, r in enumerate(sorted(RANKS + NORANKS))}
RANK_IDS["species"] = 255


def make_filter(lower=None, higher=None, equal=(), black=(), discard_norank=False, save_norank=False, discard_root=False, root_taxid=1):
    return dict(order=ORDER, noranks=set(NORANKS), lower=lower, higher=higher, equal=list(equal), black=set(black),
                discard_norank=discard_norank or save_norank, save_norank=save_norank, discard_root=discard_root, root_taxid=root_taxid)


# "The filter list" of the issue; class / family / genus / phylum are ranks of both test trees
FILTERS = {
    "none": make_filter(),
    "L": make_filter(lower="family"),                     # unordered ranks not discarded: kept under -L
    "H": make_filter(higher="family"),                    # ... dropped under -H
    "E": make_filter(equal=["class", "genus"]),           # ... dropped under -E alone
    "E+L": make_filter(equal=["class"], lower="genus"),
    "E+H": make_filter(equal=["genus"], higher="class"),
    "N": make_filter(discard_norank=True),
    "N-n-L": make_filter(save_norank=True, lower="phylum"),
    "n-without-L": make_filter(save_norank=True),        # newRankFilter does not refuse it: falls through to the limits
    "n-H": make_filter(save_norank=True, higher="family"),
    "B": make_filter(black=["family", "clade"]),
    "R": make_filter(discard_root=True, root_taxid=1),
    "R-other": make_filter(discard_root=True, root_taxid=7),
}


def self_decision(flt, rank):
    """isPassed for a node whose own rank is `rank` ("" = no known rank), up to the walk: 'drop', 'keep' or 'walk'"""
    if rank == "":
        return "drop"
    if rank in flt["black"]:
        return "drop"
    if rank in flt["noranks"] and flt["discard_norank"]:
        if not flt["save_norank"]:
            return "drop"
        if flt["lower"]:
            return "walk"
    order = flt["order"].get(rank, 0)
    o_equals = [flt["order"][e] for e in flt["equal"]]
    if o_equals:
        if order in o_equals:
            return "keep"
        if flt["lower"]:
            return "keep" if order < flt["order"][flt["lower"]] else "drop"
        if flt["higher"]:
            return "keep" if order > flt["order"][flt["higher"]] else "drop"
        return "drop"
    if flt["lower"]:
        return "keep" if order < flt["order"][flt["lower"]] else "drop"
    if flt["higher"]:
        return "keep" if order > flt["order"][flt["higher"]] else "drop"
    return "keep"


def walk_decision(flt, rank):
    """what an ancestor of rank `rank` means to the walk: 'go' on, 'keep' or 'drop'"""
    order = flt["order"].get(rank, 0)
    lower = flt["order"][flt["lower"]] if flt["lower"] else 0                  # (0 = not given: no walk ever starts)
    if order > 0:
        return "keep" if order <= lower else "drop"                            # <=, not <
    return "go"


def is_passed(tax, flt, t, trace=None):
    """tax = (parent, rank, merged): dicts taxid -> parent taxid / rank string / new taxid.  trace: a list that receives why"""
    parent, rank, merged = tax
    why = trace if trace is not None else []
    if flt["discard_root"] and t == flt["root_taxid"]:
        why.append("root")
        return False
    x = t
    if x not in parent:
        x = merged.get(x, 0)       # a merged id is looked up as its target, and a walk starts from the target
        if x not in parent:
            why.append("absent")
            return False
    d = self_decision(flt, rank.get(x, ""))
    if d != "walk":
        why.append("self")
        return d == "keep"
    p = parent[x]
    while True:
        if p == 1:
            why.append("walk:parent1")
            return False
        if p not in parent:
            why.append("walk:absent")
            return False
        w = walk_decision(flt, rank.get(p, ""))
        if w != "go":
            why.append("walk:order")
            return w == "keep"
        if parent[p] == p:
            why.append("walk:root")
            return False
        p = parent[p]


def to_rank_filter(lib, flt, ids=RANK_IDS):
    o = flt["order"]
    return lib.RankFilter.make(order={ids[r]: o[r] for r in o if r in ids}, no_rank=[ids[r] for r in flt["noranks"] if r in ids],
                               black=[ids[r] for r in flt["black"] if r in ids], lower=o[flt["lower"]] if flt["lower"] else 0,
                               higher=o[flt["higher"]] if flt["higher"] else 0, equal=[o[e] for e in flt["equal"]],
                               discard_norank=flt["discard_norank"], save_norank=flt["save_norank"], discard_root=flt["discard_root"],
                               root_taxid=flt["root_taxid"])


# ---- library ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    from unikmer_amd import build
    build.build()
    assert os.path.exists(BIN)

    def run(*args, stdin=None):
        return subprocess.run([BIN] + [str(a) for a in args], input=stdin, capture_output=True)
    return run


def test_entry_points_declared_listed_exported(cli):
    from unikmer_amd import lib
    header = open(os.path.join(ROOT, "include", "unikmer_hip.h")).read()
    so = ctypes.CDLL(lib.SO_PATH)
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in lib.SYMBOLS
        assert hasattr(so, name)
        assert callable(getattr(lib.Context, name[4:]))
    assert "typedef struct ukm_rank_filter {" in header
    # the binding's structure has the header's layout: 256 orders, two 256-byte tables, the limits, 32 orders of -E, the flags
    assert ctypes.sizeof(lib.RankFilter) == 1024 + 256 + 256 + 8 + 128 + 4 + 4 + 4
    assert lib.RankFilter.root_taxid.offset == ctypes.sizeof(lib.RankFilter) - 4 and lib.RankFilter.n_equal.offset == 1024 + 512 + 8 + 128


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_rank_filter_plan_matches_model(cli, name):
    """every rank id 0 .. 255: the ids of RANK_IDS (255 among them) by their names, id 0 as "no known rank", and every other
    id as a rank that the rank file does not mention"""
    from unikmer_amd import lib
    flt = FILTERS[name]
    names = {i: r for r, i in RANK_IDS.items()}
    assert 255 in names and len(names) == len(RANK_IDS)
    sa, wa = lib.Context.rank_filter_plan(to_rank_filter(lib, flt))
    code_self, code_walk = {"drop": 0, "keep": 1, "walk": 2}, {"go": 0, "keep": 1, "drop": 2}
    seen = set()
    for r in range(256):
        rank = "" if r == 0 else names.get(r, "unmentioned rank %d" % r)
        want = self_decision(flt, rank)
        seen.add(want)
        assert sa[r] == code_self[want], (name, r, rank, want, int(sa[r]))
        assert wa[r] == code_walk[walk_decision(flt, rank)], (name, r, rank, int(wa[r]))
    assert "keep" in seen and "drop" in seen
    assert ("walk" in seen) == (name == "N-n-L")


def test_rank_filter_plan_refusals(cli):
    from unikmer_amd import lib
    f = to_rank_filter(lib, FILTERS["L"])
    f.higher = 3
    with pytest.raises(lib.UkmError) as e:
        lib.Context.rank_filter_plan(f)
    assert e.value.code == lib.ERR_INVALID
    for n_equal in (-1, 33, 1 << 20):
        f = to_rank_filter(lib, FILTERS["E"])
        f.n_equal = n_equal
        with pytest.raises(lib.UkmError) as e:
            lib.Context.rank_filter_plan(f)
        assert e.value.code == lib.ERR_INVALID, n_equal
    f = to_rank_filter(lib, FILTERS["E"])
    f.n_equal = 32                                                             # (the unused entries are order 0)
    lib.Context.rank_filter_plan(f)
    L = lib.load()
    sa = np.zeros(256, dtype=np.uint8)
    assert L.ukm_rank_filter_plan(None, sa.ctypes.data, sa.ctypes.data) == lib.ERR_INVALID


# ---- command line ----------------------------------------------------------------------------------------------------------
def test_help_lists_both_commands(cli):
    p = cli("--help")
    text = (p.stdout + p.stderr).decode()
    assert p.returncode == 0
    for cmd in ("rfilter", "tsplit"):
        assert re.search(r"\b%s\b" % cmd, text), cmd


def failed(p, message):
    return p.returncode != 0 and p.stderr.startswith(b"[ERRO] ") and message in p.stderr


RANK_FILE = "# test ranks\n\n" + "".join("!%s\n" % r for r in NORANKS) + "\n" + "".join(r + "\n" for r in RANKS)


@pytest.fixture(scope="module")
def files(cli, tmp_path_factory):
    d = tmp_path_factory.mktemp("taxselcli")
    kmers = b"AAAAAAAAAAA\nAACCGGTTAAC\nACGTACGTTGC\n"                # ascending codes
    taxed = b"AAAAAAAAAAA\t9606\nAACCGGTTAAC\t562\nACGTACGTTGC\t7\n"
    assert cli("dump", "-K", "-s", "-o", d / "plain", stdin=kmers).returncode == 0
    assert cli("dump", "-K", "-s", "-o", d / "taxed", stdin=taxed).returncode == 0
    assert cli("dump", "-K", "-o", d / "unsorted", stdin=taxed).returncode == 0
    (d / "ranks.txt").write_text(RANK_FILE)
    db = d / "db"
    db.mkdir()
    rows = [(1, 1, "no rank"), (2, 1, "Domain"), (3, 2, "weird rank"), (4, 2, "alien"), (5, 3, "species")]
    (db / "nodes.dmp").write_text("".join("%d\t|\t%d\t|\t%s\t|\t\t|\n" % r for r in rows))
    return dict(d=d, plain=str(d / "plain.unik"), taxed=str(d / "taxed.unik"), unsorted=str(d / "unsorted.unik"),
                ranks=str(d / "ranks.txt"), db=str(db))


def test_rfilter_refusals_come_before_the_device(cli, files):
    """on a machine without a GPU a device context cannot be created: each of these messages shows that the check came first"""
    taxed, plain = files["taxed"], files["plain"]
    p = cli("rfilter", "-L", "genus", "-H", "family", "-r", files["ranks"], taxed)
    assert failed(p, b"-H/--higher-than and -L/--lower-than can't be simultaneous given")
    p = cli("rfilter", "-n", "-r", files["ranks"], taxed)
    assert failed(p, b"flag -n/--save-predictable-norank only works along with -L/--lower-than")
    p = cli("rfilter", "-L", "genus", "-r", files["ranks"], "--data-dir", files["db"], taxed)
    assert failed(p, b"rank order not defined in rank file: alien, weird rank\n")       # sorted names
    # a taxonomy whose ranks are all defined, an input without taxids
    db2 = files["d"] / "db2"
    db2.mkdir(exist_ok=True)
    (db2 / "nodes.dmp").write_text("1\t|\t1\t|\tno rank\t|\n2\t|\t1\t|\tgenus\t|\n")
    p = cli("rfilter", "-L", "genus", "-r", files["ranks"], "--data-dir", db2, plain)
    assert failed(p, b"taxid information not found: %s" % plain.encode())
    p = cli("rfilter", "-L", "genus", "-r", files["ranks"], "--data-dir", db2, taxed, plain)
    assert failed(p, b"taxid information not found: %s" % plain.encode())
    p = cli("rfilter", "-L", "tribe", "-r", files["ranks"], "--data-dir", db2, taxed)
    assert failed(p, b"rank order not defined in rank file: tribe")
    p = cli("rfilter", "-L", "family", "-r", files["ranks"], "--data-dir", db2, taxed)
    assert failed(p, b"rank order not found in taxonomy database: family")


def test_rfilter_list_order(cli, files, tmp_path):
    p = cli("rfilter", "--list-order", "-r", files["ranks"])           # no device, no taxonomy
    assert p.returncode == 0, p.stderr
    assert p.stdout.decode().splitlines() == RANKS
    rf = tmp_path / "two.txt"
    rf.write_text("Family\n# comment\n  genus , Species,strain\n\n!No Rank\nforma\n")
    p = cli("rfilter", "--list-order", "-r", rf)
    lines = p.stdout.decode().splitlines()
    assert p.returncode == 0 and len(lines) == 3
    assert lines[0] == "family" and set(lines[1].split(",")) == {"genus", "species", "strain"} and lines[2] == "forma"
    empty = tmp_path / "empty.txt"
    empty.write_text("# nothing\n!no rank\n")
    assert failed(cli("rfilter", "--list-order", "-r", empty), b"no ranks found in file: %s" % str(empty).encode())


def test_rfilter_without_rank_file_names_the_flag(cli, files, tmp_path):
    """the reference's built-in rank list is not carried: without -r and without <data-dir>/ranks.txt the error says what to do"""
    p = cli("rfilter", "--list-order", "--data-dir", tmp_path)
    assert failed(p, b"-r") and b"ranks.txt" in p.stderr
    p = cli("rfilter", "-L", "genus", "--data-dir", tmp_path, files["taxed"])
    assert failed(p, b"-r/--rank-file")
    (tmp_path / "ranks.txt").write_text(RANK_FILE)                      # <data-dir>/ranks.txt is read when it is there
    p = cli("rfilter", "--list-order", "--data-dir", tmp_path)
    assert p.returncode == 0 and p.stdout.decode().splitlines() == RANKS


def test_tsplit_refusals_come_before_the_device(cli, files, tmp_path):
    taxed, plain, unsorted = files["taxed"], files["plain"], files["unsorted"]
    out = tmp_path / "out"
    for prefix in ("", ".hidden"):
        assert failed(cli("tsplit", "-o", prefix, "-O", out, taxed), b'-o/--out-prefix should not be empty or starting with "."')
    assert failed(cli("tsplit", "-O", out, unsorted), b"input should be sorted: %s" % unsorted.encode())
    p = cli("tsplit", "-O", out, plain, taxed)
    assert failed(p, b"taxid information not found in previous files, but found in this: %s" % taxed.encode())
    p = cli("tsplit", "-O", out, taxed, plain)
    assert failed(p, b"taxid information found in previous files, but missing in this: %s" % plain.encode())
    assert not out.exists()
