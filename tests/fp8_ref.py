"""TEST HELPER: a reference for the 8-bit OCP floating extension types that
owes nothing to the product or to the oracle.

MVX_FLOAT8_E4M3 (72) is OCP e4m3fn: 1 sign, 4 exponent (bias 7) and 3 fraction
bits, no infinities, NaN = 0x7F / 0xFF, largest finite 448 = 0x7E, smallest
subnormal 2^-9.  MVX_FLOAT8_E5M2 (73) is OCP e5m2: 5 exponent bits (bias 15),
2 fraction bits, IEEE-style: infinities 0x7C / 0xFC, NaN 0x7D..0x7F and the
negatives, largest finite 57344 = 0x7B, smallest subnormal 2^-16.

Decoding is a 256-entry table to float64 built from those definitions.  SUM
and PROD add or multiply the decoded float64 values -- exact: the widest case,
57344 + 2^-16, needs 32 bits -- and encode() rounds the exact result once to
the format, to nearest, ties to even, with the OCP non-saturating overflow
rule: E5M2 gives +-inf from a rounded magnitude of 61440 (the tie to the even
"65536"), E4M3 gives NaN for a rounded magnitude above 448 (the tie 464 rounds
to 448).  MAX / MIN are the reference's selects (coll.h:14-19) on the decoded
values and return the chosen operand's byte; the logical ops compare with zero
and give 1.0 (0x38 / 0x3C) or 0.

Elements travel as uint8 bit patterns everywhere.  `op` is out of place
(`op_direct` computes it from the definitions; `op` reads the table of
`op_direct` over all 65,536 pairs); `op_u8` has the oracle's in-place byte
interface, and the program and plan evaluators below are those of
tests/plan_exec.py with this op in the place of the oracle's (the interface
of tests/half_ref.py).
"""
import numpy as np

E4M3, E5M2 = 72, 73
TYPES = (E4M3, E5M2)
OPS = (100, 101, 102, 103, 104, 106, 108)          # what MPI_FLOAT has
UNDEFINED_OPS = (105, 107, 109, 110, 111)
ONE = {E4M3: 0x38, E5M2: 0x3C}
NAMES = {E4M3: "e4m3", E5M2: "e5m2"}
FRAC = {E4M3: 3, E5M2: 2}
BIAS = {E4M3: 7, E5M2: 15}
MAX_FINITE = {E4M3: 0x7E, E5M2: 0x7B}              # 448, 57344
NAN = {E4M3: 0x7F, E5M2: 0x7E}
INF = 0x7C                                          # E5M2 only


def _decode_table(dtype):
    frac, bias = FRAC[dtype], BIAS[dtype]
    t = np.zeros(256, np.float64)
    for u in range(256):
        e, m = (u & 0x7f) >> frac, u & ((1 << frac) - 1)
        if dtype == E4M3 and (u & 0x7f) == 0x7f:
            v = float("nan")
        elif dtype == E5M2 and e == 0x1f:
            v = float("inf") if m == 0 else float("nan")
        elif e == 0:
            v = m * 2.0 ** (1 - bias - frac)
        else:
            v = (1 + m * 2.0 ** -frac) * 2.0 ** (e - bias)
        t[u] = -v if u & 0x80 else v
    return t


DECODE = {t: _decode_table(t) for t in TYPES}
_FINITE = {t: DECODE[t][:MAX_FINITE[t] + 1].copy() for t in TYPES}      # codes 0 .. max finite, increasing


def widen(dtype, u):
    """uint8 bit patterns -> their float64 values."""
    return DECODE[dtype][np.ascontiguousarray(u, np.uint8)]


def encode(dtype, x):
    """float64 -> bit patterns: round to nearest even, overflow not
    saturated.  NaN -> the positive quiet NaN."""
    x = np.ascontiguousarray(x, np.float64)
    prec = FRAC[dtype] + 1
    min_ulp = 1 - BIAS[dtype] - FRAC[dtype]
    with np.errstate(all="ignore"):
        _, e = np.frexp(np.where(np.isfinite(x), x, 0.0))
        ulp = np.ldexp(1.0, np.maximum(e - prec, min_ulp))
        r = np.rint(x / ulp) * ulp
    mag = np.abs(r)
    top = _FINITE[dtype][-1]
    code = np.searchsorted(_FINITE[dtype], np.where(mag <= top, mag, 0.0))
    fits = np.isfinite(x) & (mag <= top)
    assert np.array_equal(_FINITE[dtype][code][fits], mag[fits]), "rounding left the format's grid"
    over = NAN[dtype] if dtype == E4M3 else INF
    out = np.where(fits, code, over).astype(np.uint8)
    out = np.where(np.signbit(x), out | 0x80, out).astype(np.uint8)
    return np.where(np.isnan(x), np.uint8(NAN[dtype]), out).astype(np.uint8)


def narrow(dtype, f):
    """Values of the format (as float32 or float64) -> their bit patterns,
    exactly; anything else is refused.  A NaN becomes the positive quiet NaN."""
    f = np.ascontiguousarray(f, np.float64)
    u = encode(dtype, f)
    back = widen(dtype, u)
    ok = (back == f) & (np.signbit(back) == np.signbit(f)) | np.isnan(f)
    assert ok.all(), "not a value of the format"
    return u


def isnan(dtype, u):
    return np.isnan(widen(dtype, u))


def op_direct(opn, dtype, inv, io):
    """The new inout bits of inout = in op inout, element by element, from
    the definitions."""
    inv = np.ascontiguousarray(inv, np.uint8)
    io = np.ascontiguousarray(io, np.uint8)
    a, b = widen(dtype, io), widen(dtype, inv)
    with np.errstate(all="ignore"):
        if opn == 100:
            return np.where(b > a, inv, io)
        if opn == 101:
            return np.where(a > b, inv, io)
        if opn in (102, 103):
            return encode(dtype, a + b if opn == 102 else a * b)
        za, zb = a != 0, b != 0
        t = {104: za & zb, 106: za | zb, 108: za ^ zb}[opn]
        return np.where(t, np.uint8(ONE[dtype]), np.uint8(0))


_TABLES = {}


def op(opn, dtype, inv, io):
    """op_direct through its table over all 65,536 (inout, in) pairs,
    computed once per (op, type): the evaluators below call it many times."""
    if (opn, dtype) not in _TABLES:
        v = np.arange(256, dtype=np.uint8)
        _TABLES[opn, dtype] = op_direct(opn, dtype, np.tile(v, 256), np.repeat(v, 256)).reshape(256, 256)
    return _TABLES[opn, dtype][np.ascontiguousarray(io, np.uint8), np.ascontiguousarray(inv, np.uint8)]


def op_via_f32(opn, dtype, inv, io):
    """SUM / PROD in float32 arithmetic, narrowed once: what a kernel that
    works in f32 per step computes."""
    a, b = widen(dtype, io).astype(np.float32), widen(dtype, inv).astype(np.float32)
    with np.errstate(all="ignore"):
        r = a + b if opn == 102 else a * b
    assert r.dtype == np.float32
    return encode(dtype, r.astype(np.float64))


def assert_same(opn, dtype, got, ref, what=""):
    """Bit for bit; a SUM / PROD result that is NaN need only be NaN on both
    sides (mvxtest.assert_same's rule for f32 / f64).  For E4M3 that leaves
    only the sign free."""
    got = np.ascontiguousarray(got).view(np.uint8).reshape(-1)
    ref = np.ascontiguousarray(ref).view(np.uint8).reshape(-1)
    assert got.size == ref.size, (got.size, ref.size, what)
    ok = got == ref
    if opn in (102, 103):
        ok |= isnan(dtype, got) & isnan(dtype, ref)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, (what, "%d elements differ" % bad.size,
                           [(int(i), hex(int(got[i])), hex(int(ref[i]))) for i in bad[:6]])


def nan_share(dtype, ref):
    return float(isnan(dtype, np.ascontiguousarray(ref).view(np.uint8)).mean())


def op_u8(opn, dtype, inv_u8, io_u8, n):
    """In place on byte views, as oracle.op: io = in op io over n elements."""
    io_u8[:n] = op(opn, dtype, inv_u8[:n], io_u8[:n])
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
        assert E == 1
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
    """Operands of note: zeros, the edges of the subnormal and normal ranges,
    1 and its neighbours, small tie makers, both signs, the largest finite
    value, the infinities (E5M2) and the NaNs."""
    frac, bias = FRAC[dtype], BIAS[dtype]
    one = bias << frac
    pos = [0, 1, (1 << frac) - 1, 1 << frac, one, one - 1, one + 1, MAX_FINITE[dtype]]
    for e in range(frac + 1, frac + 4):
        t = (bias - e) << frac
        pos += [t, t + 1, t - 1]
    out = pos + [v | 0x80 for v in pos]
    out += [0x7F, 0xFF] if dtype == E4M3 else [INF, INF | 0x80, 0x7E, 0x7D]
    return np.array(out, np.uint8)


def near_one(dtype, n, rng):
    """Random values in [0.5, 2): both binades around 1, every fraction bit."""
    frac = FRAC[dtype]
    return (ONE[dtype] - (1 << frac) + rng.integers(0, 2 << frac, n)).astype(np.uint8)


def rand_bits(dtype, n, seed, special=0.03):
    """Magnitudes in [0.5, 2) with either sign (sums and products that round
    at every step), with a share `special` (3 %) of arbitrary bytes.  Uniform
    bytes alone would make 17 % of single E4M3 products NaN."""
    rng = np.random.default_rng(seed)
    v = near_one(dtype, n, rng)
    v = np.where(rng.integers(0, 2, n) == 1, v | np.uint8(0x80), v)         # either sign
    u = rng.random(n)
    v = np.where(u < special, rng.integers(0, 256, n).astype(np.uint8), v)
    return np.ascontiguousarray(v, np.uint8)


def coll_vec(dtype, n, seed, special=0.01):
    """A rank's contribution: values in [0.5, 2) with a share `special` (1 %)
    from {NaN, the largest magnitudes of either sign (E5M2: the infinities),
    +0, -0, 1}.  (E4M3 has no infinity to absorb an overflow: at 1 % a
    12-rank PROD is NaN in 5 % of its elements, at 2 % in 9 %.)"""
    rng = np.random.default_rng(seed)
    v = near_one(dtype, n, rng)
    big = MAX_FINITE[dtype] if dtype == E4M3 else INF
    sp = np.array([NAN[dtype], big, big | 0x80, 0, 0x80, ONE[dtype]], np.uint8)
    m = rng.random(n) < special
    v[m] = sp[rng.integers(0, sp.size, int(m.sum()))]
    return v
