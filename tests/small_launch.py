"""TEST HELPER: one op / combine launch on small device buffers, checked; the
same launch planned only; and the case lists both kinds of test share.

Shared by tests/test_gpu_small_launch.py, tests/test_cpu_launch_plan.py and
tests/knob_worker.py.  Every operand sits in an allocation of its own at a
chosen byte offset from the 16-byte grid; the destination sits inside a
patterned buffer with GUARD bytes on both sides.  `combine` and `apply` run
the launch, compare the result with the CPU oracle (plan_exec.combine_cpu /
oracle.op; bit for bit, but for mvxtest.assert_same's NaN-payload rule of f32
/ f64 SUM and PROD), check that every byte outside the destination kept its
pattern, check that mvx_op_plan's answer for the addresses used is what ran
(kernel symbol, grid, dynamic LDS), and return the launched kernel symbol
and grid size.

`plan_combine` and `plan_apply` take the same arguments and return the same
pair from mvx_op_plan alone, for made-up addresses with the residues mod 16
the real buffers would have: no device, no torch, no memory.

`byte_table` is the plain numpy table of the 1-byte ops over all 65,536
(a, b) pairs; it owes nothing to the oracle.
"""
import types

import numpy as np

import mvxtest as T
from plan_exec import SHAPE_CHAIN, SHAPE_TREE, combine_cpu  # noqa: F401

GUARD = 256
DEFAULT_CAP, DEFAULT_NT_LOG2 = 1 << 20, 26      # mvx_ops_tab.h: Config::block_cap, nt_min_bytes (64 MiB)

# the cases of tests/test_gpu_small_launch.py (launched) and
# tests/test_cpu_launch_plan.py (planned)
BODY_NVEC = (1, 255, 256, 257, 511, 512, 513, 1025, 3372)
BODY_PAIRS = [(102, 10), (111, 17), (105, 8), (110, 18), (103, 24), (100, 1), (103, 2), (108, 1)]
PXI_NVEC = (1, 127, 128, 129, 255, 257, 1000)
COMBINE_NVEC = (0, 1, 1023, 1024, 1025, 4099)
MISALIGNED_N = (1, 255, 1000)
# k_combine families on MPI_FLOAT SUM: (name, k, shape, folded, KMAX, U of the
# cached build, U of the non-temporal build, PROG)
COMBINE_FAMILIES = [
    ("apply", 2, SHAPE_TREE, False, 2, 4, 4, 0),
    ("masked-tree6", 6, SHAPE_TREE, False, 8, 1, 1, 0),
    ("masked-chain7", 7, SHAPE_CHAIN, False, 8, 1, 1, 0),
    ("masked-folded-tree8", 8, SHAPE_TREE, True, 8, 1, 1, 0),
    ("prog4-k3", 3, SHAPE_TREE, False, 4, 2, 2, 0),
    ("prog4-folded-k4", 4, SHAPE_CHAIN, True, 4, 2, 2, 0),
    ("tree4-fallback", 4, SHAPE_TREE, False, 4, 1, 2, 1),
    ("tree8-fallback", 8, SHAPE_TREE, False, 8, 1, 2, 1),
]


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


def _offsets(E, k, offset, folded, misalign):
    """Bytes off the 16-byte grid of the k sources, of their fold partners
    (None: the leaf is not folded) and of the destination: all `offset`, or
    under misalign each operand at an offset of its own."""
    step = E if E < 16 else 8

    def off(i):
        return (offset + step * (i + 1)) % 16 if misalign else offset
    return [off(q) for q in range(k)], [off(q + 3) if folded and q % 2 else None for q in range(k)], offset


def _plan(mvx, op, dtype, srcs, folds, dst, n, shape):
    """(kernel symbol, grid blocks, dynamic LDS bytes) of mvx_op_plan for the
    TREE / CHAIN program over the leaves at these addresses."""
    k = len(srcs)
    tree = mvx.hip().mvx_tree_mask(k) if shape == SHAPE_TREE else 0
    chain = mvx.hip().mvx_chain_mask(k) if shape == SHAPE_CHAIN else 0
    rc, p = mvx.op_plan(op, dtype, [mvx.addr(x) for x in srcs], mvx.addr(dst), n, tree, chain,
                        folds=[mvx.addr(x) for x in folds] if folds is not None else None)
    assert rc == 0, rc
    return p.symbol.decode(), p.blocks, p.dynamic_lds


def _ran_as_planned(mvx, planned, what):
    """After a launch: the plan for its addresses is what ran.  Returns
    (kernel symbol, grid blocks)."""
    blocks, lds, _ = mvx.last_launch()
    ran = (mvx.last_kernel_symbol(), blocks, lds)
    assert planned == ran, ("planned", planned, "ran", ran, what)
    return ran[:2]


def combine(mvx, op, dtype, k, shape, n, offset=0, folded=False, seed=0, ties=0.0, misalign=False, data=None):
    """op_combine over k leaves of n elements, every operand `offset` bytes
    off the 16-byte grid (misalign: each at an offset of its own, so the
    kernel's vec_ok is 0).  data: (leaves, fold partners) to use in place of
    leaves()'s -- k arrays of n elements, and k arrays or None, None wherever
    `folded` has no partner.  Returns (kernel symbol, grid blocks)."""
    import torch
    E = mvx.dtype_info(dtype)[0]
    S, F = leaves(dtype, k, n, seed, ties, folded) if data is None else data
    assert len(S) == len(F) == k and all(len(x) == n and x.dtype == S[0].dtype for x in S), (k, n)
    assert [x is not None for x in F] == [bool(folded and q % 2) for q in range(k)], "fold partners: the odd leaves"
    npd = S[0].dtype
    so, fo, do = _offsets(E, k, offset, folded, misalign)
    dS = [_place(x, so[q], q)[1] for q, x in enumerate(S)]
    dF = [_place(x, fo[q], 20 + q)[1] if x is not None else None for q, x in enumerate(F)]
    buf, dst, host = _place(np.zeros(n, npd), do, 40)
    rc = mvx.op_combine(op, dtype, dS, dst, n, shape=shape, folds=dF if folded else None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    what = (op, dtype, k, shape, n, offset, folded, misalign)
    sym, blocks = _ran_as_planned(mvx, _plan(mvx, op, dtype, dS, dF if folded else None, dst, n, shape), what)
    ref = combine_cpu(op, dtype, E, [_u8(x) for x in S], [_u8(x) if x is not None else None for x in F], shape, n)
    _check(op, dtype, buf, host, offset, ref.view(npd), (sym,) + what)
    return sym, blocks


def apply(mvx, oracle, op, dtype, n, offset=0, seed=0, ties=0.0, misalign=False, data=None):
    """The plain op in place (mvx_op_apply: inout = in op inout).  data: (in,
    inout) of n elements to use in place of leaves()'s.  Returns (kernel
    symbol, grid blocks)."""
    import torch
    E = mvx.dtype_info(dtype)[0]
    (a, b), _ = leaves(dtype, 2, n, seed, 0.0) if data is None else (data, None)
    assert len(a) == len(b) == n and a.dtype == b.dtype, (n, len(a), len(b))
    if ties:
        sel = np.random.default_rng(seed).random(n) < ties
        a.view(np.uint8).reshape(n, -1)[sel, :10] = b.view(np.uint8).reshape(n, -1)[sel, :10]
    ref = T.clone(b)
    assert oracle.op(op, dtype, _u8(a), _u8(ref), n) == 0
    da = _place(a, _offsets(E, 1, offset, False, misalign)[0][0], 1)[1]
    buf, db, host = _place(b, offset, 2)
    rc = mvx.op_apply(op, dtype, da, db, n)
    torch.cuda.synchronize()
    assert rc == 0, rc
    what = (op, dtype, n, offset, misalign)
    sym, blocks = _ran_as_planned(mvx, _plan(mvx, op, dtype, [db, da], None, db, n, SHAPE_TREE), what)
    _check(op, dtype, buf, host, offset, ref, (sym,) + what)
    return sym, blocks


def launched_lds(mvx):
    """Dynamic LDS bytes of the last launch."""
    return mvx.last_launch()[1]


# ------------------------------------------------------------- planned only

_BASE = 1 << 32          # made-up allocations, 16-byte aligned like torch's, 4 GiB apart
_planned_lds = 0


def _fake(slot, offset):
    return _BASE * (slot + 1) + GUARD + offset


def _planned(got):
    global _planned_lds
    _planned_lds = got[2]
    return got[:2]


def plan_combine(mvx, op, dtype, k, shape, n, offset=0, folded=False, seed=0, ties=0.0, misalign=False, data=None):
    """What `combine` with these arguments would launch: (kernel symbol, grid
    blocks) from mvx_op_plan; seed, ties and data (the data) play no part."""
    so, fo, do = _offsets(mvx.dtype_info(dtype)[0], k, offset, folded, misalign)
    srcs = [_fake(q, o) for q, o in enumerate(so)]
    folds = [_fake(20 + q, o) if o is not None else None for q, o in enumerate(fo)] if folded else None
    return _planned(_plan(mvx, op, dtype, srcs, folds, _fake(40, do), n, shape))


def plan_apply(mvx, oracle, op, dtype, n, offset=0, seed=0, ties=0.0, misalign=False, data=None):
    """What `apply` with these arguments would launch (oracle is not used)."""
    da = _fake(1, _offsets(mvx.dtype_info(dtype)[0], 1, offset, False, misalign)[0][0])
    db = _fake(2, offset)
    return _planned(_plan(mvx, op, dtype, [db, da], None, db, n, SHAPE_TREE))


# plan_combine / plan_apply under the names the launching functions have, for
# checks written once and run either way (tests/knob_worker.py)
PLAN = types.SimpleNamespace(combine=plan_combine, apply=plan_apply, launched_lds=lambda mvx: _planned_lds)


def body_symbol(op, k, shape):
    """(prefix, suffix) of the body kernel an aligned, unfolded, whole-chunk
    non-temporal tree / chain of k leaves runs (mvx_ops_tab.h kfam / kchain)."""
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
