"""GPU: the kernels of MVX_SUM_ACC32 / MVX_PROD_ACC32 on the four narrow
floating types against tests/acc32_ref.py (float32 arithmetic in numpy, one
rounding at the end), which owes nothing to the product.

Every kernel family at the ragged sizes of tests/test_gpu_fp8_ops.py (16 or 8
elements per 16-byte chunk): the body kernels, the masked programs with heads,
tails, folded leaves and mutually misaligned operands, cached and
non-temporal; the two one-side-f32 programs of mvx_op_program_f32 for 1 to 8
leaves; and the two-operand op against the device's own MPI_SUM / MPI_PROD.
Bit for bit, but for a NaN result, which need only be NaN on both sides; the
share of such elements is asserted on the reference's result, on the CPU,
before anything is launched.
"""
import numpy as np
import pytest

import acc32_ref as A
import fp8_ref
import half_ref
import mvxtest as T
import small_launch as SL
from small_launch import SHAPE_CHAIN, SHAPE_TREE

pytestmark = pytest.mark.gpu

TNAME = {64: "_Float16", 65: "bf16", 72: "f8e4m3", 73: "f8e5m2"}
BODY_NVEC = (1, 255, 256, 257, 511, 512, 513, 1025, 3372)      # test_gpu_small_launch.py
NAN_CAP = 0.10
F32_OUT, F32_IN = 1, 2


def _o(op):
    return op - 164 + 12          # the template's op argument: OSUMA = 12, OPRODA = 13 (mvx_ops_fn.h)


@pytest.fixture
def launch(mvx):
    def set_(cap, nt_log2):
        mvx.set_launch(cap or SL.DEFAULT_CAP, nt_log2)
    try:
        yield set_
    finally:
        mvx.set_launch(SL.DEFAULT_CAP, SL.DEFAULT_NT_LOG2)


# NaN-exempt elements of the reference results so far, per (op, type):
# [NaN results, results].  Every reference result is counted here, on the CPU,
# before its launch; the share is asserted as soon as it means something (one
# NaN in nine elements is 11 %) and again at the end of every test.
NAN_SEEN = {}


def _nan_capped(op, dtype, ref=None, nan=None):
    """Count a reference result (narrow bytes, or `nan`: a mask of its
    NaN elements) and assert the (op, type) pair's share."""
    c = NAN_SEEN.setdefault((op, dtype), [0, 0])
    if ref is not None:
        nan = A.isnan(dtype, ref)
    if nan is not None:
        c[0] += int(nan.sum())
        c[1] += int(nan.size)
    if c[1] >= 1000:
        assert c[0] < NAN_CAP * c[1], ("NaN-exempt share of the reference results", op, dtype, c)


def _check(op, dtype, buf, host, offset, ref, what):
    """The destination against the reference, and every byte around it."""
    got = T.from_dev(buf)
    lo, nb = SL.GUARD + offset, ref.nbytes
    A.assert_same(op, dtype, got[lo:lo + nb], ref, what)
    assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + nb:], host[lo + nb:]), \
        ("bytes outside the destination changed", what)


def _sym_ok(sym, dtype, pre, suf):
    assert sym.startswith(pre) and sym.endswith(suf) and TNAME[dtype] in sym, (sym, pre, suf)


def _combine(mvx, op, dtype, k, shape, n, offset=0, folded=False, seed=0, misalign=False):
    """mvx_op_combine over k leaves of n elements, every operand `offset`
    bytes off the 16-byte grid (misalign: each at an offset of its own, so the
    kernel takes element loads).  Returns (kernel symbol, grid blocks)."""
    import torch
    e = A.ESIZE[dtype]
    S = [A.rand_bits(dtype, n, 100 * seed + q) for q in range(k)]
    F = [A.rand_bits(dtype, n, 100 * seed + 50 + q) if folded and q % 2 else None for q in range(k)]
    ref = A.combine(op, dtype, S, F, shape, n)
    _nan_capped(op, dtype, ref)

    def off(i):
        return (offset + 3 * e * (i + 1)) % 16 if misalign else offset
    dS = [SL._place(x, off(q), q)[1] for q, x in enumerate(S)]
    dF = [SL._place(x, off(q + 3), 20 + q)[1] if x is not None else None for q, x in enumerate(F)]
    buf, dst, host = SL._place(np.zeros(n * e, np.uint8), offset, 40)
    rc = mvx.op_combine(op, dtype, dS, dst, n, shape=shape, folds=dF if folded else None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    sym, blocks = mvx.last_kernel_symbol(), mvx.last_launch()[0]
    _check(op, dtype, buf, host, offset, ref, (sym, op, dtype, k, shape, n, offset, folded, misalign))
    return sym, blocks


def _apply(mvx, op, dtype, n, offset=0, seed=0, misalign=False):
    """mvx_op_apply in place (inout = in op inout)."""
    import torch
    e = A.ESIZE[dtype]
    a, b = A.rand_bits(dtype, n, 100 * seed), A.rand_bits(dtype, n, 100 * seed + 1)
    ref = A.run_program(op, dtype, [b, a], None, 1, 0, n)
    _nan_capped(op, dtype, ref)
    da = SL._place(a, (offset + 3 * e) % 16 if misalign else offset, 1)[1]
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
@pytest.mark.parametrize("op,dtype", A.PAIRS, ids=A.IDS)
def test_body_kernels_ragged_sizes_and_grid_stride(mvx, launch, op, dtype, cap):
    """k_tree_body (k = 4, 8) and k_chain_body (k = 4 .. 8) at chunk counts
    around one and two blocks' work, the grid capped at 1 and 3 blocks."""
    launch(cap, 4)
    V = 16 // A.ESIZE[dtype]
    for nvec in BODY_NVEC:
        n = nvec * V
        for shape, ks in ((SHAPE_TREE, (4, 8)), (SHAPE_CHAIN, (4, 5, 6, 7, 8))):
            for k in ks:
                sym, blocks = _combine(mvx, op, dtype, k, shape, n, seed=k)
                if shape == SHAPE_TREE:
                    _sym_ok(sym, dtype, "k_tree_body<%d, " % _o(op), ", %d, 2>" % k)
                else:
                    _sym_ok(sym, dtype, "k_chain_body<%d, " % _o(op), ", %d, 2>" % (4 if k == 4 else 8))
                _capped(blocks, cap)
                if cap is None:
                    assert blocks == (nvec + 511) // 512
    assert NAN_SEEN[op, dtype][1] >= 1000
    _nan_capped(op, dtype)


# (name, k, shape, folded, KMAX, U of the cached build, U of the non-temporal
# build, PROG): the apply kernel, the masked programs over 3 leaves (the
# KMAX = 4 kernels) and over 5, 6 and 7 (KMAX = 8), folded full trees and
# chains, and the fixed trees and chains through k_combine (a head or a tail
# keeps them off the body kernels)
FAMILIES = [
    ("apply", 2, SHAPE_TREE, False, 2, 4, 4, 0),
    ("tree3", 3, SHAPE_TREE, False, 4, 2, 2, 0),
    ("tree3-folded", 3, SHAPE_TREE, True, 4, 2, 2, 0),
    ("chain4-folded", 4, SHAPE_CHAIN, True, 4, 2, 2, 0),
    ("chain5-folded", 5, SHAPE_CHAIN, True, 8, 1, 1, 0),
    ("tree6", 6, SHAPE_TREE, False, 8, 1, 1, 0),
    ("tree7-folded", 7, SHAPE_TREE, True, 8, 1, 1, 0),
    ("tree8-folded", 8, SHAPE_TREE, True, 8, 1, 1, 0),
    ("tree4", 4, SHAPE_TREE, False, 4, 1, 2, 1),
    ("tree8", 8, SHAPE_TREE, False, 8, 1, 2, 1),
    ("chain4", 4, SHAPE_CHAIN, False, 8, 1, 1, 0),
    ("chain6", 6, SHAPE_CHAIN, False, 8, 1, 1, 0),
    ("chain8", 8, SHAPE_CHAIN, False, 8, 1, 1, 0),
]
# (bytes off the 16-byte grid, head elements) for 1-byte and 2-byte elements
HEADS = {1: ((1, 15), (6, 10), (15, 1)), 2: ((2, 7), (6, 5), (14, 1))}


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("op,dtype", A.PAIRS, ids=A.IDS)
def test_combine_families_head_tail_and_stride(mvx, launch, op, dtype, nt):
    """k_combine, cached and non-temporal builds, folded and unfolded:
    operands off the 16-byte grid (a head, a tail of 3), n = 0, 1, 15, 16, 17
    and sizes of several blocks under a grid cap; then operands misaligned
    against each other."""
    e = A.ESIZE[dtype]
    V = 16 // e
    for fi, (_, k, shape, folded, kmax, u0, u1, prog) in enumerate(FAMILIES):
        nleaves = k + (k // 2 if folded else 0)
        for ci, cap in enumerate((None, 1, 2)):
            launch(cap, 4 if nt else -1)

            def want(n):
                big = nt and (nleaves + 1) * n * e >= 16              # the 16-byte non-temporal threshold
                return "k_combine<%d, " % _o(op), ", %d, %d, %d, %d>" % (kmax, u1 if big else u0, 1 if big else 0, prog)
            offset, head = HEADS[e][(fi + ci) % 3]
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
                    u = u1 if nt else u0
                    assert blocks == max(1, (nvec + 256 * u - 1) // (256 * u))
            for n in (1, 255, 1000):
                sym, blocks = _combine(mvx, op, dtype, k, shape, n, folded=folded, seed=n % 5, misalign=True)
                _sym_ok(sym, dtype, *want(n))
                _capped(blocks, cap)
    assert NAN_SEEN[op, dtype][1] >= 1000
    _nan_capped(op, dtype)


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("op,dtype", A.PAIRS, ids=A.IDS)
def test_apply_in_place_head_tail_and_stride(mvx, launch, op, dtype, nt):
    """mvx_op_apply itself (the destination aliases the inout operand)."""
    e = A.ESIZE[dtype]
    V = 16 // e
    for cap in (None, 1, 2):
        launch(cap, 4 if nt else -1)
        for offset, head in HEADS[e]:
            for n in (1, 15, 16, 17, head + V * 1025 + 3):
                sym, blocks = _apply(mvx, op, dtype, n, offset=offset, seed=n % 11)
                big = nt and 3 * n * e >= 16
                _sym_ok(sym, dtype, "k_combine<%d, " % _o(op), ", 2, 4, %d, 0>" % (1 if big else 0))
                _capped(blocks, cap)
        assert mvx.op_apply(op, dtype, None, None, 0) == 0
        for n in (1, 255, 1000):
            sym, blocks = _apply(mvx, op, dtype, n, seed=n % 5, misalign=True)
            _capped(blocks, cap)
    assert NAN_SEEN[op, dtype][1] >= 1000
    _nan_capped(op, dtype)


# ------------------------------------------------- the one-side-f32 programs

def _masks(k, shape):
    return (A.tree_mask(k), 0) if shape == SHAPE_TREE else (0, A.chain_mask(k))


@pytest.mark.parametrize("op,dtype", A.PAIRS, ids=A.IDS)
def test_narrow_leaves_to_an_f32_result(mvx, op, dtype):
    """mvx_op_program_f32, F32_OUT: the program's float32 value, not narrowed;
    k = 1 .. 8 (k = 1 widens a leaf, with its fold partner), tree and chain,
    aligned (the word path), a head and a tail, and a misaligned leaf (the
    element path); folds on the odd leaves every other time."""
    import torch
    e = A.ESIZE[dtype]
    for k in range(1, 9):
        for shape in (SHAPE_TREE, SHAPE_CHAIN):
            tm, cm = _masks(k, shape)
            for ni, n in enumerate((1, 17, 4099)):
                for case, (off, mis) in enumerate(((0, False), (2, False), (0, True))):
                    folded = (k + ni + case) % 2 == 1
                    S = [A.rand_bits(dtype, n, 7 * k + q + n) for q in range(k)]
                    F = [A.rand_bits(dtype, n, 900 + 7 * k + q + n) if folded and (q % 2 or k == 1) else None
                         for q in range(k)]
                    ref = A.program_f32(op, dtype, S, F, tm, cm)
                    _nan_capped(op, dtype, nan=np.isnan(ref))
                    dS = [SL._place(x, (off + (e if mis and q == k - 1 else 0)) % 16, q)[1] for q, x in enumerate(S)]
                    dF = [SL._place(x, off, 20 + q)[1] if x is not None else None for q, x in enumerate(F)]
                    # the f32 side: 2 narrow bytes of head are 8 / 4 bytes of floats
                    foff = 0 if off == 0 else (16 - 4 * (2 // e)) % 16
                    buf, dst, host = SL._place(np.zeros(4 * n, np.uint8), foff, 40)
                    rc = mvx.op_program_f32(op, dtype, dS, dst, n, tm, cm, F32_OUT, folds=dF if folded else None)
                    torch.cuda.synchronize()
                    assert rc == 0, rc
                    sym = mvx.last_kernel_symbol()
                    _sym_ok(sym, dtype, "k_combine_f32<%d, " % _o(op), ", 0>")
                    got = T.from_dev(buf)
                    lo = SL.GUARD + foff
                    A.assert_same_f32(got[lo:lo + 4 * n], ref, (sym, k, shape, n, off, mis, folded))
                    assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + 4 * n:], host[lo + 4 * n:])
    assert NAN_SEEN[op, dtype][1] >= 1000
    _nan_capped(op, dtype)


def _f32_specials(dtype):
    """float32 values around what the narrowing must decide: beyond the
    format's range, the ties at the overflow boundary with their float32
    neighbours, the smallest magnitudes and their ties, float32 subnormals,
    zeros, infinities, NaN."""
    top = {64: 65504.0, 65: float(np.float32(3.3895313892515355e38)), 72: 448.0, 73: 57344.0}[dtype]
    ulp = {64: 32.0, 65: 2.0 ** 120, 72: 32.0, 73: 8192.0}[dtype]
    tiny = {64: 2.0 ** -24, 65: 2.0 ** -133, 72: 2.0 ** -9, 73: 2.0 ** -16}[dtype]
    v = [top, top + ulp / 2, top + ulp, 1e30, 3e38, np.inf, np.nan, 0.0, 1e-40, 1.4e-45, 2.0 ** -126,
         tiny, tiny / 2, 1.5 * tiny, 2.5 * tiny, tiny / 4, 1.0, 1.0 + 2.0 ** -12]
    out = []
    with np.errstate(all="ignore"):
        for x in v:
            f = np.float32(x)
            out += [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    a = np.array(out, np.float32)
    return np.concatenate([a, -a])


@pytest.mark.parametrize("op,dtype", A.PAIRS, ids=A.IDS)
def test_f32_leaves_to_the_narrow_result(mvx, op, dtype):
    """mvx_op_program_f32, F32_IN: float32 leaves (k = 1 .. 8, tree and
    chain), the result narrowed once.  k = 1 is the narrowing alone, on
    values beyond each format's range, ties at the overflow boundary and
    float32 subnormals; wider programs mix those into random leaves."""
    import torch
    e = A.ESIZE[dtype]
    sp = _f32_specials(dtype)
    for k in range(1, 9):
        for shape in (SHAPE_TREE, SHAPE_CHAIN):
            tm, cm = _masks(k, shape)
            for n in (1, 17, 4099):
                for off, mis in ((0, False), (2, False), (0, True)):
                    rng = np.random.default_rng(31 * k + n)
                    Y = []
                    for q in range(k):
                        y = (rng.standard_normal(n) * 2.0 ** rng.integers(-3, 4, n)).astype(np.float32)
                        if k == 1:
                            y[:min(n, sp.size)] = sp[:min(n, sp.size)]
                        else:
                            m = rng.random(n) < 0.02
                            y[m] = sp[rng.integers(0, sp.size, int(m.sum()))]
                        Y.append(y)
                    ref = A.round_to(dtype, A.masked_f32(op, Y, tm, cm))
                    if k > 1:      # k = 1 is the narrowing alone, on hand-picked values
                        _nan_capped(op, dtype, ref)
                    foff = 0 if off == 0 else (16 - 4 * (2 // e)) % 16
                    dY = [SL._place(y, (foff + (4 if mis and q == k - 1 else 0)) % 16, q)[1] for q, y in enumerate(Y)]
                    buf, dst, host = SL._place(np.zeros(n * e, np.uint8), off, 40)
                    rc = mvx.op_program_f32(op, dtype, dY, dst, n, tm, cm, F32_IN)
                    torch.cuda.synchronize()
                    assert rc == 0, rc
                    sym = mvx.last_kernel_symbol()
                    _sym_ok(sym, dtype, "k_combine_f32<%d, " % _o(op), ", 1>")
                    _check(op, dtype, buf, host, off, ref, (sym, k, shape, n, off, mis))
    assert NAN_SEEN[op, dtype][1] >= 1000
    _nan_capped(op, dtype)


def test_f32_side_argument_checks(mvx):
    d = T.to_dev(np.zeros(64, np.uint8))
    p = d.data_ptr()
    assert mvx.op_program_f32(102, 72, [p], p, 4, 0, 0, F32_OUT) == 12          # only the two wide ops
    assert mvx.op_program_f32(164, 10, [p], p, 4, 0, 0, F32_OUT) == 329
    assert mvx.op_program_f32(164, 72, [p], p, 4, 0, 0, 3) == 12
    assert mvx.op_program_f32(164, 72, [p], p + 2, 4, 0, 0, F32_OUT) == 12      # f32 operands are 4-byte aligned
    assert mvx.op_program_f32(164, 72, [p + 1], p, 4, 0, 0, F32_IN) == 12
    assert mvx.op_program_f32(164, 72, [p], p + 32, 4, 0, 0, F32_IN, folds=[p]) == 12
    assert mvx.op_program_f32(164, 72, [p], p, 0, 0, 0, F32_OUT) == 0


# ------------------------------------------- two operands: MPI_SUM / MPI_PROD

@pytest.mark.parametrize("op,dtype", A.PAIRS, ids=A.IDS)
def test_two_operands_equal_the_devices_own_per_step_op(mvx, launch, op, dtype):
    """k = 2, no fold: bit-equal to the device's MPI_SUM / MPI_PROD wherever
    that is not NaN, NaN where it is -- all 65,536 byte pairs of an 8-bit
    type, all 65,536 patterns of a 16-bit type against partners(), either
    role; and both equal acc32_ref."""
    import torch
    if dtype in fp8_ref.TYPES:
        a, b = SL.byte_pairs()
    else:
        part = half_ref.partners(dtype)
        a = np.tile(np.arange(65536, dtype=np.uint32).astype(np.uint16), part.size)
        b = np.repeat(part, 65536)
    n = a.size
    for (inv, io), nt in (((a, b), 0), ((b, a), 1)):
        launch(None, 4 if nt else -1)
        ref = A.run_program(op, dtype, [io.view(np.uint8), inv.view(np.uint8)], None, 1, 0, n)
        din = torch.from_numpy(inv.view(np.uint8).copy()).cuda()
        wide = torch.from_numpy(io.view(np.uint8).copy()).cuda()
        step = wide.clone()
        assert mvx.op_apply(op, dtype, din, wide, n) == 0
        sym = mvx.last_kernel_symbol()
        assert mvx.op_apply(A.BASE[op], dtype, din, step, n) == 0
        torch.cuda.synchronize()
        _sym_ok(sym, dtype, "k_combine<%d, " % _o(op), ", 2, 4, %d, 0>" % nt)
        A.assert_same(op, dtype, T.from_dev(wide), T.from_dev(step), ("device MPI_SUM / MPI_PROD", nt))
        A.assert_same(op, dtype, T.from_dev(wide), ref, ("acc32_ref", nt))


def test_undefined_pairs_leave_the_operand(mvx):
    """The wide ops on MPI_FLOAT and MPI_INT answer 329 and launch nothing."""
    import torch
    a = np.arange(1000, dtype=np.float32)
    da, db = T.to_dev(a.view(np.uint8)), T.to_dev(a.view(np.uint8))
    for op in A.OPS:
        for dtype in (10, 6):
            assert mvx.op_apply(op, dtype, da, db, 1000) == 329
            assert mvx.op_combine(op, dtype, [da, db, da], db, 1000) == 329
    torch.cuda.synchronize()
    assert np.array_equal(T.from_dev(db), a.view(np.uint8))
