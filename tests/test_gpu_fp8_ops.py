"""GPU: the op kernels of the extension datatypes MVX_FLOAT8_E4M3 /
MVX_FLOAT8_E5M2.

Every (op, type) pair -- seven ops, two types -- against tests/fp8_ref.py,
which owes nothing to the product: all 65,536 (inout, in) byte pairs in either
role (every tie, subnormal, overflowing pair, NaN and signed-zero role there
is -- this is the test that pins what the hardware narrowing does on
overflow), and every kernel family at the ragged sizes of
tests/test_gpu_small_launch.py with sixteen elements per 16-byte chunk.  Bit
for bit, but for a NaN result of SUM / PROD, which need only be NaN on both
sides (for E4M3 that still pins 7 of the 8 bits); the share of such elements
is asserted on the reference's result.
"""
import numpy as np
import pytest

import fp8_ref as H
import mvxtest as T
import small_launch as SL
from small_launch import SHAPE_CHAIN, SHAPE_TREE

pytestmark = pytest.mark.gpu

PAIRS = [(op, dt) for dt in H.TYPES for op in H.OPS]
IDS = ["%d-%s" % (op, H.NAMES[dt]) for op, dt in PAIRS]
TNAME = {H.E4M3: "f8e4m3", H.E5M2: "f8e5m2"}
BODY_NVEC = (1, 255, 256, 257, 511, 512, 513, 1025, 3372)      # test_gpu_small_launch.py
NAN_CAP = 0.10
V = 16                                                         # elements per 16-byte chunk
# NaN results among all 65,536 pairs (tests/test_cpu_fp8_types.py derives them)
PAIR_NANS = {(102, H.E4M3): 1456, (103, H.E4M3): 11140, (102, H.E5M2): 3038, (103, H.E5M2): 3044}


@pytest.fixture
def launch(mvx):
    def set_(cap, nt_log2):
        mvx.set_launch(cap or SL.DEFAULT_CAP, nt_log2)
    try:
        yield set_
    finally:
        mvx.set_launch(SL.DEFAULT_CAP, SL.DEFAULT_NT_LOG2)


def _nan_capped(op, dtype, ref):
    # (a launch of a few elements has no meaningful share: one NaN in nine is 11 %)
    if op in (102, 103) and ref.size >= 1000:
        share = H.nan_share(dtype, ref)
        assert share < NAN_CAP, ("NaN-exempt share of the reference result", share)


def _check(op, dtype, buf, host, offset, ref, what):
    """The destination against the reference, and every byte around it."""
    got = T.from_dev(buf)
    lo, nb = SL.GUARD + offset, ref.nbytes
    H.assert_same(op, dtype, got[lo:lo + nb], ref, what)
    assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + nb:], host[lo + nb:]), \
        ("bytes outside the destination changed", what)


def _sym_ok(sym, dtype, pre, suf):
    assert sym.startswith(pre) and sym.endswith(suf) and TNAME[dtype] in sym, (sym, pre, suf)


# ------------------------------------------------------- all 65,536 pairs

@pytest.mark.parametrize("op,dtype", PAIRS, ids=IDS)
def test_every_pair_in_either_role(mvx, launch, op, dtype):
    """All 65,536 (inout, in) byte pairs in one launch: the slow index as the
    inout operand (the cached build), then swapped (the non-temporal build)."""
    import torch
    slow, fast = SL.byte_pairs()
    n = slow.size
    for role, (inv, io), nt in (("inout", (fast, slow), 0), ("in", (slow, fast), 1)):
        launch(None, 4 if nt else -1)
        ref = H.op(op, dtype, inv, io)
        if op in (102, 103):
            assert int(H.isnan(dtype, ref).sum()) == PAIR_NANS[op, dtype]      # the NaN-exempt elements, exactly
        host = np.random.default_rng(5).integers(0, 256, n + 2 * SL.GUARD, dtype=np.uint8)
        host[SL.GUARD:SL.GUARD + n] = io
        buf = torch.from_numpy(host.copy()).cuda()
        din = torch.from_numpy(inv.copy()).cuda()
        assert mvx.op_apply(op, dtype, din, buf[SL.GUARD:SL.GUARD + n], n) == 0
        torch.cuda.synchronize()
        sym = mvx.last_kernel_symbol()
        _sym_ok(sym, dtype, "k_combine<%d, " % (op - 100), ", 2, 4, %d, 0>" % nt)
        _check(op, dtype, buf, host, 0, ref, (role, sym))


# ------------------------------------------------------------ ragged launches

def _combine(mvx, op, dtype, k, shape, n, offset=0, folded=False, seed=0, misalign=False):
    """mvx_op_combine over k leaves of n elements, every operand `offset`
    bytes off the 16-byte grid (misalign: each at an offset of its own, odd
    ones included, so the kernel takes element loads).  Returns (kernel
    symbol, grid blocks)."""
    import torch
    S = [H.rand_bits(dtype, n, 100 * seed + q) for q in range(k)]
    F = [H.rand_bits(dtype, n, 100 * seed + 50 + q) if folded and q % 2 else None for q in range(k)]

    def off(i):
        return (offset + 3 * (i + 1)) % 16 if misalign else offset
    dS = [SL._place(x, off(q), q)[1] for q, x in enumerate(S)]
    dF = [SL._place(x, off(q + 3), 20 + q)[1] if x is not None else None for q, x in enumerate(F)]
    buf, dst, host = SL._place(np.zeros(n, np.uint8), offset, 40)
    rc = mvx.op_combine(op, dtype, dS, dst, n, shape=shape, folds=dF if folded else None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    sym, blocks = mvx.last_kernel_symbol(), mvx.last_launch()[0]
    ref = H.combine(op, dtype, S, F, shape, n)
    _nan_capped(op, dtype, ref)
    _check(op, dtype, buf, host, offset, ref, (sym, op, dtype, k, shape, n, offset, folded, misalign))
    return sym, blocks


def _apply(mvx, op, dtype, n, offset=0, seed=0, misalign=False):
    """mvx_op_apply in place (inout = in op inout)."""
    import torch
    a, b = H.rand_bits(dtype, n, 100 * seed), H.rand_bits(dtype, n, 100 * seed + 1)
    ref = H.op(op, dtype, a, b)
    _nan_capped(op, dtype, ref)
    da = SL._place(a, (offset + 3) % 16 if misalign else offset, 1)[1]
    buf, db, host = SL._place(b, offset, 2)
    rc = mvx.op_apply(op, dtype, da, db, n)
    torch.cuda.synchronize()
    assert rc == 0, rc
    sym, blocks = mvx.last_kernel_symbol(), mvx.last_launch()[0]
    _check(op, dtype, buf, host, offset, ref, (sym, op, dtype, n, offset, misalign))
    return sym, blocks


def _capped(blocks, cap):
    assert blocks >= 1 and (cap is None or blocks <= cap), (blocks, cap)


@pytest.mark.parametrize("cap", [None, 1, 3])
@pytest.mark.parametrize("op,dtype", PAIRS, ids=IDS)
def test_body_kernels_ragged_sizes_and_grid_stride(mvx, launch, op, dtype, cap):
    """k_tree_body (k = 4, 8) and k_chain_body (k = 4 .. 8) at chunk counts
    around one and two blocks' work, the grid capped at 1 and 3 blocks."""
    launch(cap, 4)
    for nvec in BODY_NVEC:
        n = nvec * V
        for shape, ks in ((SHAPE_TREE, (4, 8)), (SHAPE_CHAIN, (4, 5, 6, 7, 8))):
            for k in ks:
                sym, blocks = _combine(mvx, op, dtype, k, shape, n, seed=k)
                pre, suf = SL.body_symbol(op, k, shape)
                _sym_ok(sym, dtype, pre, suf)
                _capped(blocks, cap)
                if cap is None:
                    assert blocks == (nvec + 511) // 512


# (name, k, shape, folded, KMAX, U): the apply kernel, the masked programs
# over 3 leaves (the KMAX = 4 kernels) and over 5, 6 and 7 (KMAX = 8)
FAMILIES = [
    ("apply", 2, SHAPE_TREE, False, 2, 4),
    ("tree3", 3, SHAPE_TREE, False, 4, 2),
    ("tree3-folded", 3, SHAPE_TREE, True, 4, 2),
    ("chain5", 5, SHAPE_CHAIN, False, 8, 1),
    ("chain5-folded", 5, SHAPE_CHAIN, True, 8, 1),
    ("tree6", 6, SHAPE_TREE, False, 8, 1),
    ("tree6-folded", 6, SHAPE_TREE, True, 8, 1),
    ("tree7", 7, SHAPE_TREE, False, 8, 1),
    ("tree7-folded", 7, SHAPE_TREE, True, 8, 1),
]
HEADS = ((1, 15), (6, 10), (15, 1))        # (bytes off the 16-byte grid, head elements)


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("op,dtype", PAIRS, ids=IDS)
def test_combine_families_head_tail_and_stride(mvx, launch, op, dtype, nt):
    """k_combine, cached and non-temporal builds, folded and unfolded:
    operands 1, 6 and 15 bytes off the 16-byte grid (heads of 15, 10 and 1
    elements, a tail of 3), n = 0, 1, 15, 16, 17 and sizes of several blocks
    under a grid cap; then operands misaligned against each other."""
    for fi, (_, k, shape, folded, kmax, u) in enumerate(FAMILIES):
        nleaves = k + (k // 2 if folded else 0)
        for ci, cap in enumerate((None, 1, 2)):
            launch(cap, 4 if nt else -1)

            def want(n):
                big = nt and (nleaves + 1) * n >= 16              # the 16-byte non-temporal threshold
                return "k_combine<%d, " % (op - 100), ", %d, %d, %d, 0>" % (kmax, u, 1 if big else 0)
            offset, head = HEADS[(fi + ci) % 3]
            for n in (0, 1, 15, 16, 17):
                if n == 0:
                    assert mvx.op_combine(op, dtype, [None] * k, None, 0, shape=shape) == 0
                    continue
                sym, blocks = _combine(mvx, op, dtype, k, shape, n, offset=offset, folded=folded, seed=n)
                _sym_ok(sym, dtype, *want(n))
                _capped(blocks, cap)
            for nvec in (1, 257, 1025):
                n = head + V * nvec + 3
                sym, blocks = _combine(mvx, op, dtype, k, shape, n, offset=offset, folded=folded, seed=nvec % 7)
                _sym_ok(sym, dtype, *want(n))
                _capped(blocks, cap)
                if cap is None:
                    assert blocks == max(1, (nvec + 256 * u - 1) // (256 * u))
            for n in (1, 255, 1000):
                sym, blocks = _combine(mvx, op, dtype, k, shape, n, folded=folded, seed=n % 5, misalign=True)
                _sym_ok(sym, dtype, *want(n))
                _capped(blocks, cap)


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("op,dtype", PAIRS, ids=IDS)
def test_apply_in_place_head_tail_and_stride(mvx, launch, op, dtype, nt):
    """mvx_op_apply itself (the destination aliases the inout operand)."""
    for cap in (None, 1, 2):
        launch(cap, 4 if nt else -1)
        for offset, head in HEADS:
            for n in (1, 15, 16, 17, head + V * 1025 + 3):
                sym, blocks = _apply(mvx, op, dtype, n, offset=offset, seed=n % 11)
                big = nt and 3 * n >= 16
                _sym_ok(sym, dtype, "k_combine<%d, " % (op - 100), ", 2, 4, %d, 0>" % (1 if big else 0))
                _capped(blocks, cap)
        assert mvx.op_apply(op, dtype, None, None, 0) == 0
        for n in (1, 255, 1000):
            sym, blocks = _apply(mvx, op, dtype, n, seed=n % 5, misalign=True)
            _capped(blocks, cap)


def test_undefined_ops_leave_the_operand(mvx):
    """BAND, BOR, BXOR, MAXLOC and MINLOC answer 329 and launch nothing."""
    import torch
    for dtype in H.TYPES:
        a = H.rand_bits(dtype, 1000, 1)
        b = H.rand_bits(dtype, 1000, 2)
        da, db = T.to_dev(a), T.to_dev(b)
        for op in H.UNDEFINED_OPS:
            assert mvx.op_apply(op, dtype, da, db, 1000) == 329
            assert mvx.op_combine(op, dtype, [da, db, da], db, 1000) == 329
        torch.cuda.synchronize()
        assert np.array_equal(T.from_dev(db), b)
