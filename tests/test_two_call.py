"""lib.py's size-query helper (_sized: view, dump, unik_decode and tsplit go through it) against a fake entry point.  No GPU:
the helper only looks at return codes and counts."""
import pytest


@pytest.fixture(scope="module")
def lib():
    from unikmer_amd import build, lib as L
    build.build()  # (an error's text is the library's ukm_last_error)
    return L


class Fake:
    """an entry point that leaves `need` records: call(outs) -> (rc, n_out), outs None is the size query"""

    def __init__(self, lib, need, codes=()):
        self.lib, self.need, self.codes, self.caps = lib, need, list(codes), []

    def __call__(self, outs):
        cap = 0 if outs is None else len(outs)
        self.caps.append(cap)
        if self.codes:
            return self.codes.pop(0), self.need
        return (self.lib.OK if cap >= self.need else self.lib.ERR_CAPACITY), self.need


def test_outputs_that_fit_take_one_call(lib):
    f, mine = Fake(lib, 3), [0] * 8
    outs, n = lib._sized(f, mine, lambda need: pytest.fail("nothing to allocate"))
    assert outs is mine and n == 3 and f.caps == [8]


def test_size_query_then_the_exact_size(lib):
    f = Fake(lib, 5)
    outs, n = lib._sized(f, None, lambda need: [0] * need)
    assert f.caps == [0, 5] and len(outs) == 5 and n == 5
    f = Fake(lib, 0)  # nothing to leave: the query answers OK, and the one call that counts still runs
    outs, n = lib._sized(f, None, lambda need: [0] * need)
    assert f.caps == [0, 0] and outs == [] and n == 0


def test_a_second_capacity_error_or_any_other_code_is_raised(lib):
    f = Fake(lib, 5, [lib.ERR_CAPACITY, lib.ERR_CAPACITY])
    with pytest.raises(lib.CapacityError) as e:
        lib._sized(f, None, lambda need: [0] * need)
    assert e.value.needed == 5 and f.caps == [0, 5]  # no third call
    f = Fake(lib, 5, [lib.ERR_FORMAT])
    with pytest.raises(lib.FormatError):
        lib._sized(f, None, lambda need: pytest.fail("the query failed: nothing to allocate"))
    assert f.caps == [0]
    f = Fake(lib, 5, [lib.ERR_CAPACITY, lib.ERR_UNSORTED])
    with pytest.raises(lib.UnsortedError):
        lib._sized(f, None, lambda need: [0] * need)
    assert f.caps == [0, 5]
    f, mine = Fake(lib, 9), [0] * 8  # the caller's own outputs are too small: one call, the size in the error
    with pytest.raises(lib.CapacityError) as e:
        lib._sized(f, mine, lambda need: pytest.fail("the caller's outputs are not replaced"))
    assert e.value.needed == 9 and f.caps == [8]
