"""TEST HELPER: one op / combine launch on small device buffers, checked.

Shared by tests/test_gpu_small_launch.py and tests/knob_worker.py.  Every
operand sits in an allocation of its own at a chosen byte offset from the
16-byte grid; the destination sits inside a patterned buffer with GUARD bytes
on both sides.  `combine` and `apply` run the launch, compare the result with
the CPU oracle (plan_exec.combine_cpu / oracle.op; bit for bit, but for
mvxtest.assert_same's NaN-payload rule of f32 / f64 SUM and PROD), check that
every byte outside the destination kept its pattern, and return the launched
kernel symbol and grid size.

`byte_table` is the plain numpy table of the 1-byte ops over all 65,536
(a, b) pairs; it owes nothing to the oracle.
"""
import numpy as np

import mvxtest as T
from plan_exec import SHAPE_CHAIN, SHAPE_TREE, combine_cpu  # noqa: F401

GUARD = 256
DEFAULT_CAP, DEFAULT_NT_LOG2 = 1 << 20, 26      # mvx_ops.hip: g_block_cap, 64 MiB


def leaves(dtype, k, n, seed=0, ties=0.0, folded=False):
    """k random leaves of n elements (mvxtest.rand_vec) and their fold
    partners (odd leaves, or None).  ties: that fraction of each leaf's
    elements takes the previous leaf's first 10 bytes (the x87 value of
    MPI_LONG_DOUBLE_INT: equal values, the loc = min rule)."""
    S = [T.rand_vec(dtype, n, 100 * seed + q) for q in range(k)]
    if ties:
        rng = np.random.default_rng(seed + 77)
        for q in range(1, k):
            sel = rng.random(n) < ties
            cur, prev = S[q].view(np.uint8).reshape(n, -1), S[q - 1].view(np.uint8).reshape(n, -1)
            cur[sel, :10] = prev[sel, :10]          # significand + sign / exponent
    F = [T.rand_vec(dtype, n, 100 * seed + 50 + q) if folded and q % 2 else None for q in range(k)]
    return S, F


def _u8(x):
    return np.ascontiguousarray(x).view(np.uint8).reshape(-1)


def _place(x, offset, seed):
    """(device buffer, device view of x, host image of the buffer): x's bytes
    at GUARD + offset into a buffer of seeded random bytes."""
    import torch
    b = _u8(x)
    host = np.random.default_rng(9000 + seed).integers(0, 256, GUARD + offset + b.size + GUARD + 16, dtype=np.uint8)
    lo = GUARD + offset
    host[lo:lo + b.size] = b
    buf = torch.from_numpy(host.copy()).cuda()
    assert buf.data_ptr() % 16 == 0
    return buf, buf[lo:lo + b.size], host


def _check(op, dtype, buf, host, offset, ref, what):
    got = T.from_dev(buf)
    lo, nb = GUARD + offset, ref.nbytes
    T.assert_same(op, dtype, got[lo:lo + nb], ref)
    assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + nb:], host[lo + nb:]), \
        ("bytes outside the destination changed", what)


def combine(mvx, op, dtype, k, shape, n, offset=0, folded=False, seed=0, ties=0.0, misalign=False):
    """op_combine over k leaves of n elements, every operand `offset` bytes
    off the 16-byte grid (misalign: each at an offset of its own, so the
    kernel's vec_ok is 0).  Returns (kernel symbol, grid blocks)."""
    import torch
    E = mvx.dtype_info(dtype)[0]
    S, F = leaves(dtype, k, n, seed, ties, folded)
    npd = S[0].dtype
    step = E if E < 16 else 8

    def off(i):
        return (offset + step * (i + 1)) % 16 if misalign else offset
    dS = [_place(x, off(q), q)[1] for q, x in enumerate(S)]
    dF = [_place(x, off(q + 3), 20 + q)[1] if x is not None else None for q, x in enumerate(F)]
    buf, dst, host = _place(np.zeros(n, npd), offset, 40)
    rc = mvx.op_combine(op, dtype, dS, dst, n, shape=shape, folds=dF if folded else None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    sym, blocks = mvx.last_kernel_symbol(), mvx.last_launch()[0]
    ref = combine_cpu(op, dtype, E, [_u8(x) for x in S], [_u8(x) if x is not None else None for x in F], shape, n)
    _check(op, dtype, buf, host, offset, ref.view(npd), (sym, op, dtype, k, shape, n, offset, folded, misalign))
    return sym, blocks


def apply(mvx, oracle, op, dtype, n, offset=0, seed=0, ties=0.0, misalign=False):
    """The plain op in place (mvx_op_apply: inout = in op inout).  Returns
    (kernel symbol, grid blocks)."""
    import torch
    E = mvx.dtype_info(dtype)[0]
    (a, b), _ = leaves(dtype, 2, n, seed, 0.0)
    if ties:
        sel = np.random.default_rng(seed).random(n) < ties
        a.view(np.uint8).reshape(n, -1)[sel, :10] = b.view(np.uint8).reshape(n, -1)[sel, :10]
    ref = T.clone(b)
    assert oracle.op(op, dtype, _u8(a), _u8(ref), n) == 0
    da = _place(a, (offset + (E if E < 16 else 8)) % 16 if misalign else offset, 1)[1]
    buf, db, host = _place(b, offset, 2)
    rc = mvx.op_apply(op, dtype, da, db, n)
    torch.cuda.synchronize()
    assert rc == 0, rc
    sym, blocks = mvx.last_kernel_symbol(), mvx.last_launch()[0]
    _check(op, dtype, buf, host, offset, ref, (sym, op, dtype, n, offset, misalign))
    return sym, blocks


def body_symbol(op, k, shape):
    """(prefix, suffix) of the body kernel an aligned, unfolded, whole-chunk
    non-temporal tree / chain of k leaves runs (mvx_ops_kern.h kfam / kchain)."""
    if shape == SHAPE_TREE:
        return "k_tree_body<%d, " % (op - 100), ", %d, 2>" % k
    return "k_chain_body<%d, " % (op - 100), ", %d, 2>" % (4 if k == 4 else 8)


# ------------------------------------------------------------ the byte table

BYTE_OPS = {1: list(range(100, 110)), 2: list(range(100, 110)), 3: [105, 107, 109]}


def byte_pairs():
    """(a, b): all 65,536 byte pairs, a the slow index."""
    v = np.arange(256, dtype=np.uint8)
    return np.repeat(v, 256), np.tile(v, 256)


def byte_table(op, dtype):
    """op over byte_pairs() in plain numpy: int64 arithmetic wrapped to 8
    bits, a signed compare for MPI_CHAR MAX / MIN, 0 / 1 from the logical
    ops."""
    a8, b8 = byte_pairs()
    signed = dtype == 1
    a = (a8.view(np.int8) if signed else a8).astype(np.int64)
    b = (b8.view(np.int8) if signed else b8).astype(np.int64)
    r = {
        100: lambda: np.where(b > a, b, a),
        101: lambda: np.where(a > b, b, a),
        102: lambda: a + b,
        103: lambda: a * b,
        104: lambda: ((a != 0) & (b != 0)).astype(np.int64),
        105: lambda: a & b,
        106: lambda: ((a != 0) | (b != 0)).astype(np.int64),
        107: lambda: a | b,
        108: lambda: ((a != 0) ^ (b != 0)).astype(np.int64),
        109: lambda: a ^ b,
    }[op]()
    return (r & 0xff).astype(np.uint8)


def byte_filler(op):
    """What leaves 2 .. k-1 of a body run hold so that the result stays
    op(a, b): None = repeat b (the ops for which op(op(a, b), b) = op(a, b)),
    else the op's identity byte."""
    return {100: None, 101: None, 104: None, 105: None, 106: None, 107: None,
            102: 0, 103: 1, 108: 0, 109: 0}[op]
