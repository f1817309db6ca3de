"""TEST HELPER: the reference for the f32-accumulating ops MVX_SUM_ACC32 (164)
and MVX_PROD_ACC32 (165) on MVX_FLOAT16, MVX_BFLOAT16, MVX_FLOAT8_E4M3 and
MVX_FLOAT8_E5M2.  It owes nothing to the product or to the oracle.

A result element is its block's whole combine program in numpy float32
arithmetic: every leaf widened exactly (half_ref.widen / fp8_ref.widen), every
fold, tree step and chain step one float32 add or multiply (round to nearest
even, subnormals kept), and the final value rounded ONCE to the format by the
rounding half_ref / fp8_ref use for their own ops (numpy's float16 conversion,
half_ref.narrow_bf16, fp8_ref.encode: nearest even, overflow not saturated).
No narrow value exists in between.  Programs are evaluated straight from the
masks or from the plan -- pre-folds, every segment's tree, the chain over the
segment heads -- whatever their leaf count: nothing here knows that the device
executor takes 8 leaves a launch.

Elements travel as uint8 byte views everywhere (1 or 2 bytes an element), as
in fp8_ref / half_ref.
"""
import numpy as np

import fp8_ref
import half_ref

SUM, PROD = 164, 165
OPS = (SUM, PROD)
BASE = {SUM: 102, PROD: 103}                       # the per-step op with the same two-operand result
TYPES = half_ref.TYPES + fp8_ref.TYPES             # 64, 65, 72, 73
NAMES = {**half_ref.NAMES, **fp8_ref.NAMES}
ESIZE = {64: 2, 65: 2, 72: 1, 73: 1}
NPT = {64: np.uint16, 65: np.uint16, 72: np.uint8, 73: np.uint8}
PAIRS = [(op, dt) for dt in TYPES for op in OPS]
IDS = ["%d-%s" % (op, NAMES[dt]) for op, dt in PAIRS]


def _mod(dtype):
    return half_ref if dtype in half_ref.TYPES else fp8_ref


def bits(dtype, u8):
    """A byte view -> the elements' bit patterns (uint8 / uint16)."""
    return np.ascontiguousarray(u8).view(np.uint8).reshape(-1).view(NPT[dtype])


def widen(dtype, u8):
    """Byte view -> exact float32 values."""
    f = _mod(dtype).widen(dtype, bits(dtype, u8))
    g = f.astype(np.float32)
    assert np.array_equal(g.astype(f.dtype), f, equal_nan=True)      # the widening is exact
    return g


def round_to(dtype, f):
    """float32 -> the format, rounded once (nearest even, overflow not
    saturated), as a uint8 byte view."""
    f = np.ascontiguousarray(f, np.float32)
    with np.errstate(all="ignore"):
        if dtype == half_ref.F16:
            u = f.astype(np.float16).view(np.uint16)
        elif dtype == half_ref.BF16:
            u = half_ref.narrow_bf16(f).astype(np.uint16)
        else:
            u = fp8_ref.encode(dtype, f.astype(np.float64))
    return np.ascontiguousarray(u).view(np.uint8)


def step(opn, a, b):
    """One float32 step, a the inout operand."""
    assert a.dtype == np.float32 and b.dtype == np.float32
    with np.errstate(all="ignore"):
        r = a + b if opn == SUM else a * b
    assert r.dtype == np.float32
    return r


def isnan(dtype, u8):
    return _mod(dtype).isnan(dtype, bits(dtype, u8))


def nan_share(dtype, ref):
    return float(isnan(dtype, ref).mean())


def assert_same(opn, dtype, got, ref, what=""):
    """Bit for bit; a NaN result need only be NaN on both sides."""
    _mod(dtype).assert_same(BASE[opn], dtype, bits(dtype, got), bits(dtype, ref), what)


def assert_same_f32(got, ref, what=""):
    """float32 values bit for bit, NaN for NaN."""
    got = np.ascontiguousarray(got).view(np.uint8).reshape(-1).view(np.float32)
    ref = np.ascontiguousarray(ref, np.float32).reshape(-1)
    assert got.size == ref.size, (got.size, ref.size, what)
    ok = (got.view(np.uint32) == ref.view(np.uint32)) | (np.isnan(got) & np.isnan(ref))
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (what, "%d elements differ" % bad.size, [(int(i), got[i], ref[i]) for i in bad[:6]])


# ------------------------------------------------------------ programs and plans

tree_mask = fp8_ref.tree_mask
chain_mask = fp8_ref.chain_mask


def _leaves_f32(opn, dtype, leaves, folds):
    y = []
    for q, a in enumerate(leaves):
        v = widen(dtype, a)
        if folds is not None and folds[q] is not None:
            v = step(opn, v, widen(dtype, folds[q]))
        y.append(v)
    return y


def masked_f32(opn, y, tmask, cmask):
    """The combine program of include/mvx_hip.h over float32 leaves: tree
    steps level by level, then the chain; the left operand is inout.  Returns
    the float32 value."""
    y = list(y)
    k = len(y)
    for l in range(3):
        for q in range(8):
            if tmask >> (l * 8 + q) & 1:
                assert q + (1 << l) < k
                y[q] = step(opn, y[q], y[q + (1 << l)])
    for q in range(1, k):
        if cmask >> q & 1:
            y[0] = step(opn, y[0], y[q])
    return y[0]


def program_f32(opn, dtype, leaves, folds, tmask, cmask):
    """The program's float32 value over narrow leaves (byte views), not narrowed."""
    return masked_f32(opn, _leaves_f32(opn, dtype, leaves, folds), tmask, cmask)


def run_program(opn, dtype, leaves, folds, tmask, cmask, n):
    return round_to(dtype, program_f32(opn, dtype, leaves, folds, tmask, cmask))[:n * ESIZE[dtype]]


def combine(opn, dtype, leaves, folds, shape, n):
    k = len(leaves)
    return run_program(opn, dtype, leaves, folds, tree_mask(k) if shape == 0 else 0,
                       chain_mask(k) if shape == 1 else 0, n)


def plan_f32(P, leaves, folds):
    """A predefined-op plan's chain-of-trees program (include/mvx_coll.h) in
    float32, any number of leaves."""
    assert not P.tree_swap and not P.chain_swap
    y = _leaves_f32(P.op, P.dtype, leaves, folds)
    for s, e in P.segments():
        h = 1
        while h < e - s:
            for q in range(s, e - h, 2 * h):
                y[q] = step(P.op, y[q], y[q + h])
            h *= 2
    for s, _ in P.segments()[1:]:
        y[0] = step(P.op, y[0], y[s])
    return y[0]


def run_plan_program(P, leaves, folds, n):
    return round_to(P.dtype, plan_f32(P, leaves, folds))[:n * ESIZE[P.dtype]]


def run_plans(plans, sends, recvs):
    """Execute all ranks' plans.  sends / recvs: per-rank uint8 arrays."""
    p = len(plans)
    outs = [None] * p
    for r, P in enumerate(plans):
        if not P.has_combine or P.c_cnt == 0:
            continue
        E = P.esize
        assert E == ESIZE[P.dtype]
        lo, hi = P.c_src_off * E, (P.c_src_off + P.c_cnt) * E
        leaves = [sends[P.leaf[q]][lo:hi] for q in range(P.k)]
        folds = [sends[P.leaf_fold[q]][lo:hi] if P.leaf_fold[q] >= 0 else None for q in range(P.k)]
        out = run_plan_program(P, leaves, folds, P.c_cnt)
        outs[r] = out
        if not P.c_dst_tmp:
            d = P.c_dst_off * E
            recvs[r][d:d + out.size] = out
    for r, P in enumerate(plans):
        E = P.esize
        for d in range(p):
            if P.b_send[d].cnt:
                o = P.b_send[d].off * E
                recvs[d][o:o + P.b_send[d].cnt * E] = outs[r][:P.b_send[d].cnt * E]
    return recvs


# ------------------------------------------------------------------- operands

def rand_bits(dtype, n, seed, special=None):
    """The per-step helpers' operands (magnitudes in [0.5, 2), either sign, a
    small share of arbitrary patterns), as a byte view."""
    m = _mod(dtype)
    v = m.rand_bits(dtype, n, seed) if special is None else m.rand_bits(dtype, n, seed, special)
    return np.ascontiguousarray(v).view(np.uint8)


def coll_vec(dtype, n, seed, special=None):
    """A rank's contribution (values in [0.5, 2) with a small share of NaN,
    extremes, zeros and 1), as a byte view."""
    m = _mod(dtype)
    v = m.coll_vec(dtype, n, seed) if special is None else m.coll_vec(dtype, n, seed, special)
    return np.ascontiguousarray(v).view(np.uint8)
