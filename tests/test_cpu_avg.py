"""CPU: the extension op MVX_AVG (168), the ranks' mean: the handle, the
(op, type) verdicts, the plans (MPI_SUM's but for the handle), the launch
plans (MPI_SUM's kernels instantiated for op index 14) and the scratch slots
of programs over more than 8 leaves."""
import ctypes
import os
import re

import pytest

import acc32_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AVG, SUM, SUM_ACC32 = 168, 102, 164
MPI_INT, MPI_FLOAT, MPI_DOUBLE, E4M3 = 6, 10, 11, 72
NOT_DEFINED, PERM_OP = 329, 844
TYPES = (10, 11, 26, 27) + A.TYPES              # the f32 / f64 kinds and the four narrow floats
ESIZE = {10: 4, 11: 8, 26: 4, 27: 8, **A.ESIZE}


def _colls(mvx):
    return {"ar": mvx.COLL_ALLREDUCE, "red": mvx.COLL_REDUCE, "rs": mvx.COLL_REDUCE_SCATTER, "scan": mvx.COLL_SCAN}


def _verdict(mvx, h):
    return mvx.hip().mvx_op_apply(AVG, h, None, None, 0, None)


def test_handle_is_168_in_both_headers_and_the_mirror(mvx):
    assert mvx.MVX_AVG == AVG and mvx.OP_NAMES[AVG] == "MVX_AVG"
    assert mvx.DEFINED_AVG == {AVG: [10, 11, 26, 27, 64, 65, 72, 73]}
    for table in (mvx.DEFINED, mvx.DEFINED_EXT, mvx.DEFINED_EXT8, mvx.DEFINED_ACC32):
        assert AVG not in table
    for header in ("mvx_mpi.h", "mvx_embed.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert re.search(r"#define\s+MVX_AVG\s+168\b", text), header


def test_defined_on_f32_f64_and_the_narrow_floats_alone(mvx):
    hip = mvx.hip()
    for h in mvx.DEVICE_TYPES:
        ok = h in TYPES
        assert _verdict(mvx, h) == (0 if ok else NOT_DEFINED), h
        assert hip.mvx_op_supported(AVG, h) == ok, h
        assert hip.mvx_op_element_size(AVG, h) == (mvx.NP_DTYPE[h].itemsize if ok else 0), h
    made = []
    try:
        for h in (E4M3, MPI_FLOAT):
            made.append(mvx.MPI_Type_contiguous(2, h))
            made.append(mvx.MPI_Type_struct(2, [1, 1], [0, 4], [h, MPI_INT]))
            made.append(mvx.MPI_Type_vector(3, 1, 2, h))
        for rc, d in made:
            assert rc == 0
            assert _verdict(mvx, d) == NOT_DEFINED and hip.mvx_op_supported(AVG, d) == 0, d
    finally:
        for _, d in made:
            mvx.MPI_Type_free(d)


def _image(P):
    Q = type(P)()
    ctypes.memmove(ctypes.byref(Q), ctypes.byref(P), ctypes.sizeof(P))
    Q.op = 0
    return bytes(Q)


@pytest.mark.parametrize("p", [2, 5, 8, 12, 33])
def test_permanent_symmetric_and_planned_as_mpi_sum(mvx, p):
    assert mvx.MPI_Op_free(AVG) == (PERM_OP, AVG)
    for h in TYPES:
        for cname, coll in _colls(mvx).items():
            root = p // 2 if cname == "red" else 0
            for n in (1, 5, 300, (8 << 10) // ESIZE[h] + 1, 20001):
                rc = [n // p + (1 if r < n % p else 0) for r in range(p)] if cname == "rs" else None
                for r in range(p):
                    got = mvx.plan(coll, p, r, n, h, AVG, root, recvcnts=rc)
                    ref = mvx.plan(coll, p, r, n, h, SUM, root, recvcnts=rc)
                    assert got.op == AVG and got.opkind == mvx.OPKIND_PREDEFINED and got.symmetric == 1
                    assert _image(got) == _image(ref), (h, cname, n, r)
    assert mvx.plan(mvx.COLL_ALLREDUCE, p, 0, 100, MPI_INT, AVG).symmetric == 0      # undefined: roles matter


def _launch(mvx, op, h, k, n, tmask, cmask, offs):
    srcs = [(q + 1 << 32) + 256 + o for q, o in enumerate(offs[:k])]
    rc, pl = mvx.op_plan(op, h, srcs, (40 << 32) + 256 + offs[k], n, tmask, cmask)
    assert rc == 0
    return pl.symbol.decode(), pl.tag.decode(), pl.blocks, pl.dynamic_lds


@pytest.mark.parametrize("h", [10, 11] + list(A.TYPES))
def test_launch_plan_is_sums_kernel_with_op_index_14(mvx, h):
    """mvx_op_plan: the kernel MPI_SUM gets for the same pointers and n with 14
    (OAVG) as its first template argument, the same grid and LDS reservation:
    the tree over 8 leaves, the chain over 4, the apply and a misaligned launch,
    small and past the non-temporal threshold (the body kernels)."""
    hip = mvx.hip()
    e = ESIZE[h]
    bases = set()
    for n in (17, 4099, (64 << 20) // e):
        for k, tm, cm, offs in ((8, hip.mvx_tree_mask(8), 0, [0] * 9), (4, 0, hip.mvx_chain_mask(4), [0] * 5),
                                (2, 1, 0, [0] * 3), (2, 1, 0, [0, e, 0])):
            sym, tag, blocks, lds = _launch(mvx, AVG, h, k, n, tm, cm, offs)
            rsym, rtag, rblocks, rlds = _launch(mvx, SUM, h, k, n, tm, cm, offs)
            base, rest = sym.split("<", 1)
            rbase, rrest = rsym.split("<", 1)
            assert base == rbase and rest.startswith("14, ") and rrest.startswith("2, "), (sym, rsym)
            assert rest[2:] == rrest[1:] and (blocks, lds) == (rblocks, rlds), (sym, rsym, blocks, rblocks, lds, rlds)
            assert tag.startswith("avg_") and tag[3:] == rtag[3:], (tag, rtag)
            bases.add(base)
    assert bases == {"k_combine", "k_tree_body", "k_chain_body"}


@pytest.mark.parametrize("p", [9, 33, 64])
def test_wide_slots_are_the_sums(mvx, p):
    """Programs over more than 8 leaves take MPI_SUM's scratch slots on
    MPI_FLOAT and MVX_SUM_ACC32's (f32 temporaries) on E4M3."""
    assert mvx.hip().mvx_op_supported(AVG, MPI_FLOAT) == 1 and mvx.hip().mvx_op_supported(AVG, E4M3) == 1
    wide_seen = False
    for cname, coll in _colls(mvx).items():
        for n in (1, 7, 300, 20001):
            rc = [n // p + 1] * p if cname == "rs" else None
            for r in range(p):
                for h, twin in ((MPI_FLOAT, SUM), (E4M3, SUM_ACC32)):
                    P = mvx.plan(coll, p, r, n, h, AVG, p - 1 if cname == "red" else 0, recvcnts=rc)
                    Q = mvx.plan(coll, p, r, n, h, twin, p - 1 if cname == "red" else 0, recvcnts=rc)
                    assert P.wide_slots() == Q.wide_slots(), (cname, n, r, h)
                    wide_seen |= P.k > 8 and P.wide_slots()[1] > 0
    assert wide_seen
