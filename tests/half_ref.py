"""TEST HELPER: a reference for the 16-bit floating extension types that owes
nothing to the product or to the oracle.

MVX_FLOAT16 (64) is numpy's float16: numpy adds and multiplies halves in
float32 and rounds the result once more, which equals the directly rounded
result (24 >= 2 * 11 + 2).  MVX_BFLOAT16 (65) is worked on its uint16 bit
patterns: widened by `<< 16` to float32, combined in float32 and narrowed
round-to-nearest-even by `(u + 0x7fff + ((u >> 16) & 1)) >> 16`, NaN mapped
to a NaN (24 >= 2 * 8 + 2; products are exact in float32).  MAX / MIN are
the reference's selects (coll.h:14-19) and return the chosen operand's bits;
the logical ops compare with zero and give 1.0 or 0.0 in the format.
tests/test_cpu_half_types.py checks both against exact float64 arithmetic.

Elements travel as uint16 bit patterns everywhere.  `op` is out of place;
`op_u8` has the oracle's in-place byte interface, and the program and plan
evaluators below are those of tests/plan_exec.py with this op in the place
of the oracle's.
"""
import numpy as np

F16, BF16 = 64, 65
TYPES = (F16, BF16)
OPS = (100, 101, 102, 103, 104, 106, 108)          # what MPI_FLOAT has
UNDEFINED_OPS = (105, 107, 109, 110, 111)
ONE = {F16: 0x3C00, BF16: 0x3F80}
NAMES = {F16: "f16", BF16: "bf16"}


def widen(dtype, u):
    """uint16 bit patterns -> exact float32 values."""
    u = np.ascontiguousarray(u, np.uint16)
    if dtype == F16:
        return u.view(np.float16).astype(np.float32)
    return (u.astype(np.uint32) << np.uint32(16)).view(np.float32)


def narrow_bf16(f):
    """float32 -> bfloat16 bit patterns, round to nearest even."""
    u = np.ascontiguousarray(f, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isnan(f), np.uint16(0x7fc0), r)


def narrow(dtype, f):
    """float32 values that widen() can produce -> their bit patterns, exactly
    (NaN payloads included); anything else is refused."""
    f = np.ascontiguousarray(f, np.float32)
    if dtype == F16:
        with np.errstate(all="ignore"):
            u = f.astype(np.float16).view(np.uint16)
    else:
        u = (f.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
    assert np.array_equal(widen(dtype, u).view(np.uint32), f.view(np.uint32)), "not a value of the format"
    return u


def isnan(dtype, u):
    return np.isnan(widen(dtype, u))


def op(opn, dtype, inv, io):
    """The new inout bits of inout = in op inout, element by element."""
    inv = np.ascontiguousarray(inv, np.uint16)
    io = np.ascontiguousarray(io, np.uint16)
    with np.errstate(all="ignore"):
        if dtype == F16:
            a, b = io.view(np.float16), inv.view(np.float16)
        else:
            a, b = widen(BF16, io), widen(BF16, inv)
        if opn == 100:
            return np.where(b > a, inv, io)
        if opn == 101:
            return np.where(a > b, inv, io)
        if opn in (102, 103):
            r = a + b if opn == 102 else a * b
            return r.view(np.uint16) if dtype == F16 else narrow_bf16(r)
        za, zb = a != 0, b != 0
        t = {104: za & zb, 106: za | zb, 108: za ^ zb}[opn]
        return np.where(t, np.uint16(ONE[dtype]), np.uint16(0))


def assert_same(opn, dtype, got, ref, what=""):
    """Bit for bit; a SUM / PROD result that is NaN need only be NaN on both
    sides (mvxtest.assert_same's rule for f32 / f64)."""
    got = np.ascontiguousarray(got).view(np.uint16).reshape(-1)
    ref = np.ascontiguousarray(ref).view(np.uint16).reshape(-1)
    assert got.size == ref.size, (got.size, ref.size, what)
    ok = got == ref
    if opn in (102, 103):
        ok |= isnan(dtype, got) & isnan(dtype, ref)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (what, "%d elements differ" % bad.size,
                           [(int(i), hex(int(got[i])), hex(int(ref[i]))) for i in bad[:6]])


def nan_share(dtype, ref):
    return float(isnan(dtype, np.ascontiguousarray(ref).view(np.uint16)).mean())


def op_u8(opn, dtype, inv_u8, io_u8, n):
    """In place on byte views, as oracle.op: io = in op io over n elements."""
    io = io_u8[:2 * n].view(np.uint16)
    io[:] = op(opn, dtype, inv_u8[:2 * n].view(np.uint16), io)
    return 0


# ------------------------------------------------ programs and plans (plan_exec.py)

def tree_mask(k):
    m, l = 0, 0
    while (1 << l) < k and l < 3:
        for q in range(0, k, 2 << l):
            if q + (1 << l) < k:
                m |= 1 << (l * 8 + q)
        l += 1
    return m


def chain_mask(k):
    return ((1 << k) - 1) & ~1 if k >= 2 else 0


def _folded(opn, dtype, leaves, folds, n):
    y = []
    for q, a in enumerate(leaves):
        v = a.copy()
        if folds is not None and folds[q] is not None:
            op_u8(opn, dtype, folds[q], v, n)
        y.append(v)
    return y


def run_program(opn, dtype, leaves, folds, tmask, cmask, n):
    """The combine program of include/mvx_hip.h over uint8 leaves: tree steps
    level by level, then the chain; the left operand is inout."""
    y = _folded(opn, dtype, leaves, folds, n)
    k = len(y)
    for l in range(3):
        for q in range(8):
            if tmask >> (l * 8 + q) & 1:
                assert q + (1 << l) < k
                op_u8(opn, dtype, y[q + (1 << l)], y[q], n)
    for q in range(1, k):
        if cmask >> q & 1:
            op_u8(opn, dtype, y[q], y[0], n)
    return y[0]


def combine(opn, dtype, leaves, folds, shape, n):
    k = len(leaves)
    return run_program(opn, dtype, leaves, folds, tree_mask(k) if shape == 0 else 0,
                       chain_mask(k) if shape == 1 else 0, n)


def run_plan_program(P, leaves, folds, n):
    """A predefined-op plan's chain-of-trees program (include/mvx_coll.h)."""
    assert not P.tree_swap and not P.chain_swap
    y = _folded(P.op, P.dtype, leaves, folds, n)
    for s, e in P.segments():
        h = 1
        while h < e - s:
            for q in range(s, e - h, 2 * h):
                op_u8(P.op, P.dtype, y[q + h], y[q], n)
            h *= 2
    for s, _ in P.segments()[1:]:
        op_u8(P.op, P.dtype, y[s], y[0], n)
    return y[0]


def run_plans(plans, sends, recvs):
    """Execute all ranks' plans.  sends / recvs: per-rank uint8 arrays."""
    p = len(plans)
    outs = [None] * p
    for r, P in enumerate(plans):
        if not P.has_combine or P.c_cnt == 0:
            continue
        E = P.esize
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

def partners(dtype):
    """The operands every one of the 65,536 patterns meets: zeros, the edges
    of the subnormal and normal ranges, 1 and its neighbours, the tie makers
    2^-8 .. 2^-12 with their odd neighbours (halves of an ulp of values near
    1, where round-to-nearest-even decides), both signs, the largest finite
    value, the infinities, one quiet and one signalling NaN."""
    if dtype == F16:
        frac, bias, emax = 10, 15, 0x1f
    else:
        frac, bias, emax = 7, 127, 0xff
    one = bias << frac
    pos = [0, 1, (1 << frac) - 1, 1 << frac, one, one - 1, one + 1, ((emax << frac) - 1)]
    for e in range(8, 13):
        t = (bias - e) << frac
        pos += [t, t + 1, t - 1]
    out = pos + [v | 0x8000 for v in pos]
    inf = emax << frac
    out += [inf, inf | 0x8000, inf | (1 << (frac - 1)), inf | 1]      # +-inf, quiet NaN, signalling NaN
    return np.array(out, np.uint16)


def near_one(dtype, n, rng):
    """Random values in [0.5, 2): both binades around 1, every fraction bit."""
    frac = 10 if dtype == F16 else 7
    one = ONE[dtype]
    return (one - (1 << frac) + rng.integers(0, 2 << frac, n)).astype(np.uint16)


def rand_bits(dtype, n, seed, special=0.1):
    """Mostly values in [0.5, 2) (sums and products that round at every
    step), with a share `special` split between arbitrary bit patterns and
    partners()."""
    rng = np.random.default_rng(seed)
    v = near_one(dtype, n, rng)
    v = np.where(rng.integers(0, 2, n) == 1, v | np.uint16(0x8000), v)      # either sign
    u = rng.random(n)
    part = partners(dtype)
    v = np.where(u < special / 2, rng.integers(0, 65536, n).astype(np.uint16), v)
    v = np.where((u >= special / 2) & (u < special), part[rng.integers(0, part.size, n)], v)
    return np.ascontiguousarray(v, np.uint16)


def coll_vec(dtype, n, seed, special=0.02):
    """A rank's contribution: values in [0.5, 2] with a share `special` (2 %)
    from {NaN, +inf, -inf, +0, -0, 1}."""
    rng = np.random.default_rng(seed)
    v = near_one(dtype, n, rng)
    frac = 10 if dtype == F16 else 7
    inf = (0x1f if dtype == F16 else 0xff) << frac
    sp = np.array([inf | 1 << (frac - 1), inf, inf | 0x8000, 0, 0x8000, ONE[dtype]], np.uint16)
    m = rng.random(n) < special
    v[m] = sp[rng.integers(0, sp.size, int(m.sum()))]
    return v
