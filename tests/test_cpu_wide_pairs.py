"""CPU: the sends of tests/wide_pairs.py do what the GPU tests rely on.

MAXLOC / MINLOC are idempotent and associative: an executor that drops a leaf,
or combines one twice, is invisible to them unless the dropped leaf was the
only one that could have produced the result.  On the oracle alone: the struct
layouts are the table's, and leaving out any single rank's leaf changes the
result of both ops, for every struct kind, at the largest communicator.
"""
import numpy as np
import pytest

import typemap_util as TM
from wide_pairs import PAIR_KINDS, PAIR_LAYOUT, pair_sends


@pytest.fixture(scope="module")
def types(mvx, oracle):
    t = {k: TM.both(mvx, oracle, "struct", 2, [1, 1], v[1], v[0]) for k, v in PAIR_KINDS.items()}
    yield t
    TM.free_all(mvx, oracle, t.values())


def test_layouts_are_the_table(mvx, types):
    for kind, (ext, size) in PAIR_LAYOUT.items():
        assert (mvx.MPI_Type_extent(types[kind])[1], mvx.MPI_Type_size(types[kind])[1]) == (ext, size), kind
        assert bool(mvx.plan(mvx.COLL_ALLREDUCE, 64, 0, 301, types[kind], 111).packed) == (size < ext), kind


@pytest.mark.parametrize("kind", list(PAIR_KINDS))
def test_every_rank_decides_some_element(oracle, types, kind):
    p, n = 64, 301
    h = types[kind]
    ext = PAIR_LAYOUT[kind][0]
    S = list(pair_sends(kind, p, n, 5))
    for op in (111, 110):
        full = [np.full(n * ext, 0x5C, np.uint8) for _ in range(p)]
        assert oracle.allreduce(S, full, n, h, op) == [0] * p
        for r in range(p):
            less = list(S)
            less[r] = S[(r + 1) % p]                    # rank r's leaf gone, its neighbour's twice
            out = [np.full(n * ext, 0x5C, np.uint8) for _ in range(p)]
            assert oracle.allreduce(less, out, n, h, op) == [0] * p
            assert not np.array_equal(out[0], full[0]), (kind, op, r)


@pytest.mark.parametrize("kind", ["float_int", "double_int"])
def test_one_value_in_twenty_is_nan_and_most_columns_are_clean(kind):
    p, n = 64, 301
    vdt = np.dtype(PAIR_KINDS[kind][2])
    b = pair_sends(kind, p, n, 5).reshape(p, n, PAIR_LAYOUT[kind][0])
    nan = np.isnan(np.ascontiguousarray(b[:, :, :vdt.itemsize]).view(vdt).reshape(p, n))
    assert 0.03 < nan.mean() < 0.07
    assert 0.55 < (~nan.any(0)).mean() < 0.85
