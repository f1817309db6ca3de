"""TEST HELPER: struct {value; int loc} types of every first-member kind that
mvx_ops.hip's derived_kind() maps to a pair kernel, and sends for them in
which every rank's leaf decides some element of a MAXLOC / MINLOC result
(tests/test_gpu_wide_derived.py; the claim itself is checked on the oracle
alone by tests/test_cpu_wide_pairs.py)."""
import numpy as np

import mvxtest as T

I, F, S16, L, LL, D, XF = 6, 10, 4, 8, 13, 11, 12

# member types, member displacements, the value's numpy type, the loc's offset
PAIR_KINDS = {
    "int_int": ([I, I], [0, 4], np.int32, 4),
    "float_int": ([F, I], [0, 4], np.float32, 4),
    "short_int": ([S16, I], [0, 4], np.int16, 4),
    "long_int": ([L, I], [0, 8], np.int64, 8),
    "longlong_int": ([LL, I], [0, 8], np.int64, 8),
    "double_int": ([D, I], [0, 8], np.float64, 8),
    "longdouble_int": ([XF, I], [0, 16], np.longdouble, 16),
}
# (extent, size) as MPI_Type_struct lays them out (the tests assert it from the
# library): size < extent is a type with a hole, which moves packed
PAIR_LAYOUT = {"int_int": (8, 8), "float_int": (8, 8), "short_int": (8, 6), "long_int": (16, 12),
               "longlong_int": (16, 12), "double_int": (16, 12), "longdouble_int": (32, 20)}


def pair_sends(kind, p, n, seed):
    """p ranks' sends of n struct {value; int loc} elements at the extent, as
    one (p, n * extent) byte array.

    Values come from -3..3 and locs from -9..9, so ties are common.  Element i
    belongs to rank i % p, and by (i // p) % 4 that rank holds there
      0: +100, the only maximum       1: -100, the only minimum
      2: +50 tied with other ranks    3: -50 tied with other ranks
    with loc -20 in a tie, below every other loc: its leaf alone decides the
    MAXLOC result at classes 0 and 2 and the MINLOC result at 1 and 3.  Three
    columns in ten also carry the awkward values, one value in six of them (5 %
    of all values): NaN for float and double, the x87 operand classes of
    mvxtest.xfi_operands for long double (every second value there), whose
    order dependence makes operand roles visible; the other columns stay clean
    so that the owners' wins are certain.  Every byte of a hole, of the x87
    slot's padding and past the type map is random."""
    vdt = np.dtype(PAIR_KINDS[kind][2])
    x87 = vdt == np.dtype(np.longdouble)
    loc_off = PAIR_KINDS[kind][3]
    ext = PAIR_LAYOUT[kind][0]
    rng = np.random.default_rng(seed)
    b = rng.integers(0, 256, (p, n, ext), dtype=np.uint8)
    vals = rng.integers(-3, 4, (p, n)).astype(np.float64)
    locs = rng.integers(-9, 10, (p, n)).astype(np.int32)
    awkward = (rng.random(n) < 0.3)[None, :] & (rng.random((p, n)) < (0.5 if x87 else 1 / 6))
    if vdt.kind == "f" and not x87:
        vals[awkward] = np.nan
    i = np.arange(n)
    cls = ((i // p) % 4)[None, :]
    mine = np.arange(p)[:, None] == (i % p)[None, :]
    tied = mine | (rng.random((p, n)) < 0.3)
    vals = np.where(mine & (cls == 0), 100.0, vals)
    vals = np.where(mine & (cls == 1), -100.0, vals)
    vals = np.where(tied & (cls == 2), 50.0, vals)
    vals = np.where(tied & (cls == 3), -50.0, vals)
    locs = np.where(mine & (cls >= 2), -20, locs).astype(np.int32)
    if x87:
        v = np.ascontiguousarray(vals.astype(np.longdouble)).view(np.uint8).reshape(p, n, 16)
        b[:, :, 0:10] = v[:, :, 0:10]                       # the slot's 6 padding bytes stay random
        pat = T.xfi_operands(p * n, seed)[0].view(np.uint8).reshape(p, n, 32)[:, :, 0:16]
        keep = awkward & ~mine & ~(tied & (cls >= 2))
        b[keep, 0:16] = pat[keep]
    else:
        with np.errstate(invalid="ignore"):
            v = vals.astype(vdt)
        b[:, :, 0:vdt.itemsize] = np.ascontiguousarray(v).view(np.uint8).reshape(p, n, vdt.itemsize)
    b[:, :, loc_off:loc_off + 4] = np.ascontiguousarray(locs).view(np.uint8).reshape(p, n, 4)
    return b.reshape(p, n * ext)
