"""TEST HELPER: MVX_SR_SUM's stochastically rounded narrowing as include/mvx_hip.h
defines it, in numpy float64 and integer arithmetic; owes nothing to the product."""
import numpy as np

import acc32_ref as A

M32 = 0xffffffff
# type: (mantissa bits m, least normal exponent emin, random bits nb, largest finite value)
FMT = {64: (10, -14, 16, 65504.0), 65: (7, -126, 16, 2.0 ** 127 * (2 - 2.0 ** -7)), 72: (3, -6, 8, 448.0),
       73: (2, -14, 8, 57344.0)}


def fmix32(h):
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def H(g, seed):
    """g: group indices (uint64 array or int); seed: 64-bit int."""
    g = np.asarray(g, np.uint64)
    c = fmix32((g >> np.uint64(32)) ^ np.uint64((seed >> 32) ^ 0x85EBCA77))
    return fmix32(((((g & np.uint64(M32)) ^ np.uint64(seed & M32)) * np.uint64(0x9E3779B1)) + c) & np.uint64(M32))


def sr_round(dtype, v, first, seed):
    """float32 values v, element j at index first + j of the reduced vector -> bytes of the type."""
    m, emin, nb, top = FMT[dtype]
    v = np.ascontiguousarray(v, np.float32)
    i, per = np.uint64(first) + np.arange(v.size, dtype=np.uint64), np.uint64(32 // nb)
    r = ((H(i // per, seed) >> (np.uint64(nb) * (i % per))) & np.uint64((1 << nb) - 1)).astype(np.int64)
    a, out = np.abs(v.astype(np.float64)), v.astype(np.float64)      # +-0, inf, NaN: as they are
    ok = np.isfinite(a) & (a > 0)
    with np.errstate(all="ignore"):
        q = np.ldexp(1.0, np.maximum(np.frexp(a[ok])[1] - 1, emin) - m)   # frexp - 1: floor(log2 |v|)
        lo = np.floor(a[ok] / q)
        t = np.floor((a[ok] / q - lo) * (1 << nb)).astype(np.int64)
        mag = (lo + (t + r[ok] >= (1 << nb))) * q
        mag[mag > top] = np.inf                                       # the type's own overflow
        out[ok] = np.copysign(mag, v[ok])
        return A.round_to(dtype, out.astype(np.float32))
