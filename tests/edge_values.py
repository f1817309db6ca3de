"""TEST HELPER: operand pairs at the edges of every datatype; no device use.

`operands(spec)` returns (a, b), the `in` and `inout` operands of one op: the
cross product of the type's edge list with itself, so every value meets every
value in both roles.  A spec names a datatype: ("h", handle) for a predefined
handle, ("c2", base) for MPI_Type_contiguous(2, base) (derived_util.PAIR_BASES).

* float / double: FLOAT_EDGES, 24 bit patterns.  Of the 576 pairs 94 have a
  NaN sum (92 hold a NaN, 2 are inf - inf) and 100 a NaN product (8 are
  inf * 0): 0.163 and 0.174, inside NAN_CAP.
* complex: the cross of two lanes at a time (NaN meets no NaN: at most one of
  a pair's four input lanes holds one), the other two lanes finite; then a
  block of finite values in all four lanes, whose sums and products round but
  never overflow.  inf * 0 and inf - inf are kept.
* integers: INT_EDGE_BITS per width, as bit patterns, so the unsigned handles
  get the values above the signed maximum.
* struct pairs: the value cross, each pair under loc less, equal and greater
  (INT_MIN, INT_MAX and negative locs among them); padding bytes random,
  nonzero and different in the two operands.
* contiguous count-2 pairs: the same with the loc drawn from the value list
  (a NaN loc is a relation of its own for the float bases).
* x87 (12, 22, contiguous(2, MPI_LONG_DOUBLE)): mvxtest.xf_operands /
  xfi_operands, which cover every operand class, cut to X87_N elements.

`edge_leaves` places the pair in two slots of a k-leaf program (leaves and fold
partners) and fills the others with finite, unexceptional values (`tame`);
`rand_leaves` is mvxtest.rand_vec with random padding.  `nan_share` is the
fraction of NaN lanes of an oracle result, `NAN_CAP` its bound for SUM and
PROD on float, double and complex: a NaN lane there need only be NaN on the
device (mvxtest.assert_same), so it must stay a minority.
"""
import numpy as np

import derived_util as D
import mvxtest as T

NAN_CAP = 0.25
MAX_BYTES = 64 << 10                   # no operand is larger
X87_N = {12: 2048, 22: 1024}           # elements of the x87 operands (32 KiB)
STRUCT_PAIRS = (17, 18, 19, 20, 21)    # {value, int loc} structs
FLOAT_OPS = (102, 103)                 # the ops with the NaN rule

# FLOAT_EDGES by class: (name, sign, exponent field, fraction), the last two
# as functions of the format's exponent bias B, largest exponent field X (all
# ones) and fraction width m
_F = [
    ("+qnan", 0, lambda B, X, m: X, lambda m: 1 << (m - 1)),
    ("-qnan-payload", 1, lambda B, X, m: X, lambda m: (1 << (m - 1)) | 0x1234),
    ("+inf", 0, lambda B, X, m: X, lambda m: 0), ("-inf", 1, lambda B, X, m: X, lambda m: 0),
    ("+0", 0, lambda B, X, m: 0, lambda m: 0), ("-0", 1, lambda B, X, m: 0, lambda m: 0),
    ("+minsub", 0, lambda B, X, m: 0, lambda m: 1), ("-minsub", 1, lambda B, X, m: 0, lambda m: 1),
    ("maxsub", 0, lambda B, X, m: 0, lambda m: (1 << m) - 1),
    ("+minnorm", 0, lambda B, X, m: 1, lambda m: 0), ("-minnorm", 1, lambda B, X, m: 1, lambda m: 0),
    ("2minnorm", 0, lambda B, X, m: 2, lambda m: 0),
    ("+max", 0, lambda B, X, m: X - 1, lambda m: (1 << m) - 1),
    ("-max", 1, lambda B, X, m: X - 1, lambda m: (1 << m) - 1),
    ("max/2", 0, lambda B, X, m: X - 2, lambda m: (1 << m) - 1),
    ("1+ulp", 0, lambda B, X, m: B, lambda m: 1), ("1-ulp", 0, lambda B, X, m: B - 1, lambda m: (1 << m) - 1),
    ("ulp/2", 0, lambda B, X, m: B - m - 1, lambda m: 0),
    ("1", 0, lambda B, X, m: B, lambda m: 0), ("-1", 1, lambda B, X, m: B, lambda m: 0),
    ("-2", 1, lambda B, X, m: B + 1, lambda m: 0), ("0.5", 0, lambda B, X, m: B - 1, lambda m: 0),
    ("1.5", 0, lambda B, X, m: B, lambda m: 1 << (m - 1)), ("3", 0, lambda B, X, m: B + 1, lambda m: 1 << (m - 1)),
]
FLOAT_EDGE_NAMES = [f[0] for f in _F]


def _fmt(ft):
    """(unsigned type, exponent bits, fraction bits) of float32 / float64."""
    return (np.uint32, 8, 23) if np.dtype(ft).itemsize == 4 else (np.uint64, 11, 52)


def float_edges(ft):
    """The 24 edge values of float32 / float64, built from their bits."""
    ut, eb, m = _fmt(ft)
    B, X = (1 << (eb - 1)) - 1, (1 << eb) - 1
    return np.array([(s << (eb + m)) | (e(B, X, m) << m) | frac(m) for _, s, e, frac in _F], ut).view(ft)


def edge(ft, name):
    return float_edges(ft)[FLOAT_EDGE_NAMES.index(name)]


def _finite_mild(ft):
    """The edges whose sums and products with each other stay finite."""
    keep = [i for i, n in enumerate(FLOAT_EDGE_NAMES) if "nan" not in n and "inf" not in n and n.strip("+-") not in ("max", "max/2")]
    return float_edges(ft)[keep]


def int_edge_bits(width):
    """Bit patterns of one integer width: 0, 1, 2, all ones (-1 / the unsigned
    maximum), the signed maximum and minimum (the top bit alone; the two values
    around half the unsigned range), the two around half the signed range, the
    alternating patterns, and the neighbours of the extremes."""
    top = 1 << (width - 1)
    ones = (1 << width) - 1
    alt = ones // 3                                   # 0x55..55
    return [0, 1, 2, ones, top - 1, top, (top >> 1) - 1, top >> 1, alt, alt << 1, top + 1, ones - 1, top - 2]


def int_edges(dt):
    dt = np.dtype(dt)
    ut = np.dtype("u%d" % dt.itemsize)
    return np.array(int_edge_bits(8 * dt.itemsize), ut).view(dt)


LOGICAL_WORDS = np.array([0, 1, 1, 0, 2, -1, 1, 0], np.int32)     # mvxtest.rand_vec's


def scalar_edges(dt):
    dt = np.dtype(dt)
    return float_edges(dt) if dt.kind == "f" else int_edges(dt)


def cross(v, w=None):
    """(a, b): every element of v against every element of w (v itself)."""
    w = v if w is None else w
    return np.repeat(v, len(w)), np.tile(w, len(v))


def _complex_operands(dt):
    ft = np.dtype(np.float32 if dt.itemsize == 8 else np.float64)
    e = float_edges(ft)
    x, y = cross(e)
    keep = ~(np.isnan(x) & np.isnan(y))               # a NaN meets every value but a NaN
    x, y = x[keep], y[keep]
    mild = _finite_mild(ft)
    blocks = []
    # lanes: 0 a.re, 1 a.im, 2 b.re, 3 b.im -- every a lane against every b lane;
    # the NaN of each lane meets every value once, in the re x re and im x im
    # blocks (a NaN operand lane makes both lanes of a product NaN: repeating
    # those rows in the mixed blocks would only add exempt results)
    for p, (la, lb) in enumerate(((0, 2), (0, 3), (1, 2), (1, 3))):
        sel = np.ones(x.size, bool) if la + 2 == lb else ~(np.isnan(x) | np.isnan(y))
        lanes = np.empty((4, int(sel.sum())), ft)
        for q in range(4):
            lanes[q] = mild[(np.arange(lanes.shape[1]) * (2 * q + 3) + p + q) % mild.size]
        lanes[la], lanes[lb] = x[sel], y[sel]
        blocks.append(lanes)
    # all four lanes finite: products of 1 +- ulp, subnormals, signed zeros
    nfin = MAX_BYTES // 16 - sum(b.shape[1] for b in blocks)
    i = np.arange(nfin)
    blocks.append(np.stack([mild[(i * s + o) % mild.size] for s, o in ((1, 0), (5, 3), (7, 1), (11, 2))]))
    lanes = np.concatenate(blocks, axis=1)
    a, b = np.empty(lanes.shape[1], dt), np.empty(lanes.shape[1], dt)
    a.view(ft)[0::2], a.view(ft)[1::2] = lanes[0], lanes[1]
    b.view(ft)[0::2], b.view(ft)[1::2] = lanes[2], lanes[3]
    return a, b


def pad_mask(dt):
    """Per byte of one element: True where no field lies (padding)."""
    dt = np.dtype(dt)
    m = np.ones(dt.itemsize, bool)
    if not dt.names:
        m[:] = False
        return m
    for name in dt.names:
        ft, off = dt.fields[name][:2]
        m[off:off + ft.itemsize] = False
    return m


def fill_padding(a, b, seed):
    """Random nonzero padding bytes, different in a and b (or None) at every byte."""
    pm = pad_mask(a.dtype)
    if not pm.any():
        return
    rng = np.random.default_rng(seed)
    pa = rng.integers(1, 256, (len(a), int(pm.sum())))
    a.view(np.uint8).reshape(-1, a.dtype.itemsize)[:, pm] = pa
    if b is not None:
        b.view(np.uint8).reshape(-1, a.dtype.itemsize)[:, pm] = (pa - 1 + rng.integers(1, 255, pa.shape)) % 255 + 1


_I = np.iinfo(np.int32)
# loc pairs (in, inout) of the struct pairs: less, equal, greater
INT_LOC_REL = [
    [(_I.min, -5), (-5, 3), (3, _I.max), (_I.min, _I.max)],
    [(_I.min, _I.min), (-1, -1), (_I.max, _I.max), (0, 0)],
    [(-5, _I.min), (3, -5), (_I.max, 3), (_I.max, _I.min)],
]


def _loc_relations(dt, struct):
    """Lists of (in, inout) loc pairs, one list per relation."""
    if struct:
        return [np.array(r, dt) for r in INT_LOC_REL]
    e = scalar_edges(dt)
    fin = e[~np.isnan(e)] if dt.kind == "f" else e
    s = np.unique(fin)                                # ascending (-0 and +0 are one value)
    lo, hi = s[:-1], s[1:]
    rel = [np.stack([lo, hi], 1), np.stack([s, s], 1), np.stack([hi, lo], 1)]
    if dt.kind == "f":
        nan, nan2, one, pz, nz = (edge(dt, x) for x in ("+qnan", "-qnan-payload", "1", "+0", "-0"))
        rel.append(np.array([(nan, one), (one, nan), (nan, nan2), (pz, nz), (nz, pz)], dt))      # unordered; +0 / -0
    return rel


def _pair_operands(dt, struct, seed):
    vt, lt = dt.fields["v"][0], dt.fields["l"][0]
    va, vb = cross(scalar_edges(vt))
    rel = _loc_relations(lt, struct)
    nv = va.size
    a, b = np.zeros(nv * len(rel), dt), np.zeros(nv * len(rel), dt)
    for r, pairs in enumerate(rel):
        sl = slice(r * nv, (r + 1) * nv)
        pick = pairs[(np.arange(nv) + np.arange(nv) // 24) % len(pairs)]
        a["v"][sl], b["v"][sl] = va, vb
        a["l"][sl], b["l"][sl] = pick[:, 0], pick[:, 1]
    fill_padding(a, b, seed)
    return a, b


def np_dtype(spec):
    kind, code = spec
    return D.pair_dtype(code) if kind == "c2" else T.np_dtype(code)


def is_x87(spec):
    return spec[1] == 12 or spec == ("h", 22)


def has_nan_rule(op, spec):
    """SUM / PROD on float, double and complex: a NaN lane need only be NaN."""
    return op in FLOAT_OPS and spec[0] == "h" and np_dtype(spec).kind in "fc" and not is_x87(spec)


def operands(spec, seed=0):
    """(in, inout) at the edges of the datatype `spec`."""
    kind, code = spec
    dt = np_dtype(spec)
    if spec == ("h", 12):
        a, b = T.xf_operands(X87_N[12], seed)
        a, b = a.view(np.longdouble), b.view(np.longdouble)
    elif spec == ("h", 22):
        a, b = T.xfi_operands(X87_N[22], seed)
        a, b = a.view(dt), b.view(dt)
    elif spec == ("c2", 12):                          # value and loc slots: an x87 pair each
        n = X87_N[22]
        a, b = np.zeros(n, dt), np.zeros(n, dt)
        for slot, s in ((0, seed), (1, seed + 31)):
            xa, xb = T.xf_operands(n, s)
            a.view(np.uint8).reshape(n, 32)[:, 16 * slot:16 * slot + 16] = xa.view(np.uint8).reshape(n, 16)
            b.view(np.uint8).reshape(n, 32)[:, 16 * slot:16 * slot + 16] = xb.view(np.uint8).reshape(n, 16)
    elif spec == ("h", 25):
        a, b = cross(LOGICAL_WORDS)
    elif dt.names:
        a, b = _pair_operands(dt, kind == "h" and code in STRUCT_PAIRS, seed)
    elif dt.kind == "c":
        a, b = _complex_operands(dt)
    else:
        a, b = cross(scalar_edges(dt))
    assert a.dtype == dt and b.dtype == dt and a.nbytes == b.nbytes <= MAX_BYTES, (spec, a.dtype, a.nbytes)
    return a, b


def resize(x, n):
    """n elements of x (bytes kept, padding included), taken at a stride prime
    to its length: a cut is a sample of the whole cross, not its first rows,
    and more than len(x) elements go round again."""
    x = np.ascontiguousarray(x)
    if n == len(x):
        return T.clone(x)
    assert np.gcd(37, len(x)) == 1, len(x)
    idx = (len(x) * 7 // 9 + np.arange(n) * 37) % len(x)        # (the float cross's first rows are all NaN)
    return x.view(np.uint8).reshape(len(x), -1)[idx].copy().reshape(-1).view(x.dtype)


def tame(op, spec, n, seed):
    """n finite, unexceptional elements: small integers and halves (nonzero
    for PROD, so that no inf * 0 arises), random padding; the x87 types take
    mvxtest.rand_vec's mostly-finite values."""
    dt = np_dtype(spec)
    rng = np.random.default_rng(1000 + seed)
    if spec == ("c2", 12):
        return D.rand_pairs(12, n, 1000 + seed)
    if is_x87(spec):
        return T.rand_vec(spec[1], n, 1000 + seed).view(dt)

    def scalars(t):
        t = np.dtype(t)
        if t.kind == "c":
            out = np.zeros(n, t)
            ft = np.float32 if t.itemsize == 8 else np.float64
            out.view(ft)[0::2] = scalars(ft)
            if op != 103:                             # PROD: real factors
                out.view(ft)[1::2] = scalars(ft)
            return out
        if t.kind == "f":
            pool = np.array([1, -1, 2, 0.5, 1.5, 3, -2, -0.5] + ([] if op == 103 else [0, -3, 0.25]), t)
            return pool[rng.integers(0, pool.size, n)]
        lo = -3 if t.kind == "i" else 0
        return rng.integers(lo, 4, n).astype(t)
    if spec == ("h", 25):
        return rng.choice(LOGICAL_WORDS, n)
    if not dt.names:
        return scalars(dt)
    out = np.zeros(n, dt)
    out["v"] = scalars(dt.fields["v"][0])
    out["l"] = scalars(dt.fields["l"][0]) if spec[0] == "c2" or spec[1] not in STRUCT_PAIRS else rng.integers(-5, 50, n)
    fill_padding(out, None, 2000 + seed)
    return out


def slots(k, folded):
    """The operand slots of a k-leaf program: ("s", q) leaves, ("f", q) the
    fold partners of the odd leaves."""
    return [("s", q) for q in range(k)] + [("f", q) for q in range(k) if folded and q % 2]


def edge_leaves(op, spec, k, folded, n, rot, seed=0):
    """(S, F) of a k-leaf program over n elements: the edge pair (resized to
    n) in two slots chosen by `rot`, which walks through every ordered pair of
    slots, tame values in the others."""
    a, b = operands(spec, seed)
    sl = slots(k, folded)
    m = len(sl)
    i = rot % m
    j = (i + 1 + (rot // m) % (m - 1)) % m
    S, F = [None] * k, [None] * k
    for p, (w, q) in enumerate(sl):
        x = resize(a, n) if p == i else resize(b, n) if p == j else tame(op, spec, n, 10 * seed + p)
        (S if w == "s" else F)[q] = x
    return S, F


def rand_leaves(op, spec, k, folded, n, seed):
    """mvxtest.rand_vec leaves (derived_util.rand_pairs for the contiguous
    pairs) with random nonzero padding.  Under the NaN rule rand_vec's NaN and
    inf draws (1.5 % of the lanes) stay in leaves 0 and 1 and become 1 in the
    others: ten operands of them would make a third of a product NaN."""
    def one(s, calm):
        x = D.rand_pairs(spec[1], n, s) if spec[0] == "c2" else T.rand_vec(spec[1], n, s)
        x = np.ascontiguousarray(x).view(np_dtype(spec))
        if calm and has_nan_rule(op, spec):
            lanes = x.view(np.float32 if x.dtype.itemsize in (4, 8) and x.dtype != np.float64 else np.float64)
            lanes[~np.isfinite(lanes)] = 1
        if not is_x87(spec):
            fill_padding(x, None, 3000 + s)
        return x
    few = n * np_dtype(spec).itemsize < 64           # a single chunk: one NaN lane alone would pass NAN_CAP
    S = [one(100 * seed + q, q >= 2 or few) for q in range(k)]
    F = [one(100 * seed + 50 + q, True) if folded and q % 2 else None for q in range(k)]
    return S, F


def float_lanes(x):
    """The float lanes of a float, complex or float-valued pair array, else None."""
    fp = T._float_parts(x)
    return None if fp is None else fp[1]


def nan_share(ref):
    """Fraction of the result's float lanes that are NaN."""
    nan = float_lanes(ref)
    return float(nan.mean()) if nan is not None and nan.size else 0.0
