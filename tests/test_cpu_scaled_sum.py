"""CPU: the per-rank scaled sum (mvx_op_create_scaled_sum; device-layer op index
MVX_SCALED_SUM = 169): the handle, the (op, type) verdicts, the plans
(MPI_SUM's but for the handle), the launch plans (MPI_SUM's kernels
instantiated for op index 15) and the scratch slots of programs over more
than 8 leaves (MVX_SUM_ACC32's)."""
import ctypes

import pytest

import acc32_ref as A

SCALED, SUM, SUM_ACC32 = 169, 102, 164
MPI_INT, MPI_FLOAT, MPI_REAL, E4M3 = 6, 10, 26, 72
ERR_OP, ERR_ARG, NOT_DEFINED = 9, 12, 329
TYPES = (MPI_FLOAT, MPI_REAL) + A.TYPES
ESIZE = {MPI_FLOAT: 4, MPI_REAL: 4, **A.ESIZE}


def _colls(mvx):
    return {"ar": mvx.COLL_ALLREDUCE, "red": mvx.COLL_REDUCE, "rs": mvx.COLL_REDUCE_SCATTER, "scan": mvx.COLL_SCAN}


@pytest.fixture
def op(mvx):
    made = []

    def make(p):
        rc, h = mvx.op_create_scaled_sum([0.5 + r for r in range(p)], 2.0)
        assert rc == 0
        made.append(h)
        return h
    try:
        yield make
    finally:
        for h in made:
            mvx.MPI_Op_free(h)


def test_create_and_free(mvx):
    assert mvx.MVX_SCALED_SUM == SCALED and mvx.DEFINED_SCALED == {SCALED: [10, 26, 64, 65, 72, 73]}
    rc, h = mvx.op_create_scaled_sum([1.0, 2.0, 3.0])
    assert rc == 0 and h >= 200
    assert mvx.plan(mvx.COLL_ALLREDUCE, 3, 0, 10, E4M3, h).opkind == mvx.OPKIND_PREDEFINED
    assert mvx.MPI_Op_free(h) == (0, 0)
    assert mvx.MPI_Op_free(h)[0] == ERR_OP                                  # freed: the handle is invalid again
    assert mvx.op_create_scaled_sum([], nranks=0)[0] == ERR_ARG
    assert mvx.op_create_scaled_sum([1.0] * 65)[0] == ERR_ARG
    rc, h = mvx.op_create_scaled_sum([1.0] * 64)
    assert rc == 0 and mvx.MPI_Op_free(h) == (0, 0)
    assert mvx.MPI_Op_free(SCALED)[0] == ERR_OP                             # 169 is no MPI-level op


def test_defined_on_f32_and_the_narrow_floats_alone(mvx, op):
    hip, h2 = mvx.hip(), op(2)
    made = []
    try:
        for t in (E4M3, MPI_FLOAT):
            made += [mvx.MPI_Type_contiguous(2, t), mvx.MPI_Type_vector(3, 1, 2, t)]
        assert all(rc == 0 for rc, _ in made)
        for t in list(mvx.DEVICE_TYPES) + [d for _, d in made]:
            ok = t in TYPES
            assert hip.mvx_op_apply(SCALED, t, None, None, 0, None) == (0 if ok else NOT_DEFINED), t
            assert hip.mvx_op_supported(SCALED, t) == ok, t
            assert hip.mvx_op_element_size(SCALED, t) == (ESIZE[t] if ok else 0), t
            assert mvx.plan(mvx.COLL_ALLREDUCE, 2, 0, 100, t, h2).symmetric == ok, t
    finally:
        for _, d in made:
            mvx.MPI_Type_free(d)


def _image(P):
    Q = type(P)()
    ctypes.memmove(ctypes.byref(Q), ctypes.byref(P), ctypes.sizeof(P))
    Q.op = 0
    return bytes(Q)


@pytest.mark.parametrize("p", [2, 5, 8, 12, 33])
def test_planned_as_mpi_sum(mvx, op, p):
    h = op(p)
    for t in TYPES:
        for cname, coll in _colls(mvx).items():
            root = p // 2 if cname == "red" else 0
            for n in (1, 5, 300, (8 << 10) // ESIZE[t] + 1, 20001):
                rc = [n // p + (1 if r < n % p else 0) for r in range(p)] if cname == "rs" else None
                for r in range(p):
                    got = mvx.plan(coll, p, r, n, t, h, root, recvcnts=rc)
                    ref = mvx.plan(coll, p, r, n, t, SUM, root, recvcnts=rc)
                    assert got.op == h and got.opkind == mvx.OPKIND_PREDEFINED and got.symmetric == 1
                    assert _image(got) == _image(ref), (t, cname, n, r)


def _launch(mvx, o, t, k, n, tmask, cmask, offs):
    srcs = [(q + 1 << 32) + 256 + x for q, x in enumerate(offs[:k])]
    rc, pl = mvx.op_plan(o, t, srcs, (40 << 32) + 256 + offs[k], n, tmask, cmask)
    assert rc == 0
    return pl.symbol.decode(), pl.tag.decode(), pl.blocks, pl.dynamic_lds


@pytest.mark.parametrize("t", [MPI_FLOAT] + list(A.TYPES))
def test_launch_plan_is_sums_kernel_with_op_index_15(mvx, t):
    """The tree over 8 leaves, the chain over 4, the apply and a misaligned
    launch, small and past the non-temporal threshold (the body kernels)."""
    hip, e, bases = mvx.hip(), ESIZE[t], set()
    for n in (17, 4099, (64 << 20) // e):
        for k, tm, cm, offs in ((8, hip.mvx_tree_mask(8), 0, [0] * 9), (4, 0, hip.mvx_chain_mask(4), [0] * 5),
                                (2, 1, 0, [0] * 3), (2, 1, 0, [0, e, 0])):
            sym, tag, blocks, lds = _launch(mvx, SCALED, t, k, n, tm, cm, offs)
            rsym, rtag, rblocks, rlds = _launch(mvx, SUM, t, k, n, tm, cm, offs)
            base, rest = sym.split("<", 1)
            rbase, rrest = rsym.split("<", 1)
            assert base == rbase and rest.startswith("15, ") and rrest.startswith("2, "), (sym, rsym)
            assert rest[3:] == rrest[2:] and (blocks, lds) == (rblocks, rlds), (sym, rsym, blocks, rblocks, lds, rlds)
            assert tag.startswith("scaled_") and tag[6:] == rtag[3:], (tag, rtag)
            bases.add(base)
    assert bases == {"k_combine", "k_tree_body", "k_chain_body"}


@pytest.mark.parametrize("p", [9, 33, 64])
def test_wide_slots_are_sum_acc32s(mvx, op, p):
    h, wide_seen = op(p), False
    for cname, coll in _colls(mvx).items():
        for n in (1, 7, 300, 20001):
            rc = [n // p + 1] * p if cname == "rs" else None
            for r in range(p):
                P = mvx.plan(coll, p, r, n, E4M3, h, p - 1 if cname == "red" else 0, recvcnts=rc)
                Q = mvx.plan(coll, p, r, n, E4M3, SUM_ACC32, p - 1 if cname == "red" else 0, recvcnts=rc)
                assert P.wide_slots() == Q.wide_slots(), (cname, n, r)
                wide_seen |= P.k > 8 and P.wide_slots()[1] > 0
    assert wide_seen
