"""CPU: the extension datatypes MVX_FLOAT16 (64) and MVX_BFLOAT16 (65) in the
type engine, the (op, type) support matrix and the Python constants; and the
test reference tests/half_ref.py against exact float64 arithmetic.
"""
import os
import re

import numpy as np
import pytest

import half_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPI_SHORT, MPI_INT = 4, 6
K_BASIC = 0
TYPE_NULL = 3 | (5 << 6)        # MVX_ERR_TYPE_NULL


@pytest.mark.parametrize("h", H.TYPES)
def test_extent_size_alignment_dense_basic(mvx, h):
    assert mvx.dtype_info(h) == (2, 2)
    assert mvx.hip().mvx_dtype_extent(h) == 2
    assert mvx.MPI_Type_extent(h) == (0, 2) and mvx.MPI_Type_size(h) == (0, 2)
    assert mvx.type_layout(h) == dict(kind=K_BASIC, dense=1, lb=0, ub=2, span_lo=0, span_hi=2)
    assert mvx.MPI_Type_commit(h) == 0
    assert mvx.MPI_Type_free(h)[0] == 3 | (9 << 6)          # permanent, as every basic handle
    # alignment 2: a struct {char, half} puts nothing on it but pads to 2
    rc, s = mvx.MPI_Type_struct(2, [1, 1], [0, 2], [1, h])
    assert rc == 0 and mvx.MPI_Type_extent(s) == (0, 4)
    rc, s3 = mvx.MPI_Type_struct(2, [1, 1], [0, 2], [h, 1])
    assert rc == 0 and mvx.MPI_Type_extent(s3) == (0, 4)    # 3 bytes padded to the alignment
    mvx.MPI_Type_free(s)
    mvx.MPI_Type_free(s3)


def test_constants_and_headers(mvx):
    assert (mvx.MVX_FLOAT16, mvx.MVX_BFLOAT16) == (64, 65) == H.TYPES
    assert mvx.NP_DTYPE[64] == np.dtype(np.float16) and mvx.NP_DTYPE[65] == np.dtype(np.uint16)
    assert mvx.TYPE_NAMES[64] == "MVX_FLOAT16" and mvx.TYPE_NAMES[65] == "MVX_BFLOAT16"
    assert sorted(mvx.DEFINED_EXT) == sorted(H.OPS)
    for op in range(100, 112):
        assert mvx.DEFINED_EXT.get(op, []) == ([64, 65] if op in H.OPS else [])
        assert 64 not in mvx.DEFINED[op] and 65 not in mvx.DEFINED[op]      # the reference's table
    for header in ("mvx_mpi.h", "mvx_embed.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert re.search(r"#define\s+MVX_FLOAT16\s+64\b", text), header
        assert re.search(r"#define\s+MVX_BFLOAT16\s+65\b", text), header


def _verdicts(mvx, h):
    return [mvx.hip().mvx_op_apply(op, h, None, None, 0, None) for op in range(100, 112)]


@pytest.mark.parametrize("h", H.TYPES)
def test_support_matrix(mvx, h):
    """The seven ops of MPI_FLOAT answer 0, the other five 329; derived forms
    over the new types have no op at all (no pair type is added)."""
    want = [0 if op in H.OPS else 329 for op in range(100, 112)]
    assert _verdicts(mvx, h) == want == _verdicts(mvx, 10)
    for op in range(100, 112):
        assert bool(mvx.hip().mvx_op_supported(op, h)) == (op in H.OPS)
        assert mvx.hip().mvx_op_element_size(op, h) == (2 if op in H.OPS else 0)
    assert mvx.hip().mvx_op_apply(99, h, None, None, 0, None) == mvx.MPI_ERR_OP
    assert mvx.hip().mvx_op_apply(112, h, None, None, 0, None) == mvx.MPI_ERR_OP
    derived = [mvx.MPI_Type_contiguous(2, h), mvx.MPI_Type_contiguous(1, h), mvx.MPI_Type_vector(3, 1, 2, h),
               mvx.MPI_Type_struct(2, [1, 1], [0, 4], [h, MPI_INT]),
               mvx.MPI_Type_struct(2, [1, 1], [0, 2], [h, h])]
    for rc, d in derived:
        assert rc == 0
        assert _verdicts(mvx, d) == [329] * 12, d
        mvx.MPI_Type_free(d)


def _bounds(mvx, t):
    return (mvx.MPI_Type_extent(t), mvx.MPI_Type_size(t), mvx.MPI_Type_lb(t), mvx.MPI_Type_ub(t),
            mvx.type_layout(t))


@pytest.mark.parametrize("h", H.TYPES)
def test_constructors_give_the_bounds_of_short(mvx, h):
    """Every constructor over a new type == the same constructor over
    MPI_SHORT (the reference's 2-byte, 2-aligned basic type)."""
    makers = [
        lambda t: mvx.MPI_Type_contiguous(3, t),
        lambda t: mvx.MPI_Type_contiguous(0, t),
        lambda t: mvx.MPI_Type_vector(3, 1, 2, t),
        lambda t: mvx.MPI_Type_vector(4, 2, -3, t),
        lambda t: mvx.MPI_Type_hvector(2, 3, 10, t),
        lambda t: mvx.MPI_Type_indexed(3, [2, 1, 3], [5, 0, 9], t),
        lambda t: mvx.MPI_Type_hindexed(2, [1, 2], [6, 0], t),
        lambda t: mvx.MPI_Type_struct(3, [1, 2, 1], [0, 4, 12], [MPI_INT, t, 1]),
        lambda t: mvx.MPI_Type_struct(3, [1, 1, 1], [-2, 0, 9], [15, t, 16]),      # MPI_LB, MPI_UB markers
    ]
    for i, mk in enumerate(makers):
        (rc_a, a), (rc_b, b) = mk(h), mk(MPI_SHORT)
        assert rc_a == rc_b == 0, i
        assert mvx.MPI_Type_commit(a) == mvx.MPI_Type_commit(b) == 0
        assert _bounds(mvx, a) == _bounds(mvx, b), i
        # one level up: the derived type as an old type
        (rc_a2, a2), (rc_b2, b2) = mvx.MPI_Type_vector(2, 1, 3, a), mvx.MPI_Type_vector(2, 1, 3, b)
        assert rc_a2 == rc_b2 == 0 and _bounds(mvx, a2) == _bounds(mvx, b2), i
        for t in (a2, b2, a, b):
            mvx.MPI_Type_free(t)


@pytest.mark.parametrize("h", [34, 36, 63, 66, 99])
def test_other_handles_stay_unknown(mvx, h):
    with pytest.raises(ValueError):
        mvx.dtype_info(h)
    assert mvx.hip().mvx_dtype_extent(h) == 0
    assert mvx.MPI_Type_contiguous(2, h)[0] == TYPE_NULL
    assert mvx.MPI_Type_extent(h)[0] != 0
    assert _verdicts(mvx, h) == [329] * 12
    assert not any(mvx.hip().mvx_op_supported(op, h) for op in range(100, 112))


# ------------------------------------------------ the reference helper itself

def _round_exact(x, prec, min_ulp_exp, emax):
    """float64 -> the nearest value of a binary format with `prec` significand
    bits, smallest spacing 2^min_ulp_exp and overflow at 2^emax (ties to
    even), returned as float64."""
    _, e = np.frexp(x)
    ulp = np.ldexp(1.0, np.maximum(e - prec, min_ulp_exp))
    r = np.rint(x / ulp) * ulp
    return np.where(np.abs(r) >= 2.0 ** emax, np.copysign(np.inf, r), r)


@pytest.mark.parametrize("dtype", H.TYPES)
def test_reference_sum_prod_equal_directly_rounded_exact_results(dtype):
    """All 65,536 patterns against every partner: half_ref's SUM and PROD
    (float32 arithmetic rounded again) == the float64 result rounded once to
    the format.  The float64 sum or product of two 16-bit floats is exact,
    but for bfloat16 sums whose operands lie more than 2^37 apart, which
    round to the larger operand either way."""
    prec, min_ulp, emax = (11, -24, 16) if dtype == H.F16 else (8, -133, 128)
    allp = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    part = H.partners(dtype)
    assert part.size >= 48 and int(H.isnan(dtype, part).sum()) == 2
    a = np.repeat(allp, part.size)
    b = np.tile(part, allp.size)
    with np.errstate(all="ignore"):
        x, y = H.widen(dtype, a).astype(np.float64), H.widen(dtype, b).astype(np.float64)
    for opn in (102, 103):
        with np.errstate(all="ignore"):
            exact = x + y if opn == 102 else x * y
            want = _round_exact(exact, prec, min_ulp, emax)
        for inv, io in ((a, b), (b, a)):
            got = H.op(opn, dtype, inv, io)
            gv = H.widen(dtype, got).astype(np.float64)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(gv), nan)
            assert np.array_equal(gv[~nan], want[~nan])
            assert np.array_equal(np.signbit(gv[~nan]), np.signbit(want[~nan]))
        assert H.nan_share(dtype, got) < 0.10


@pytest.mark.parametrize("dtype", H.TYPES)
def test_reference_selects_and_logicals(dtype):
    one, qnan, inf = H.ONE[dtype], (0x7e00 if dtype == H.F16 else 0x7fc0), (0x7c00 if dtype == H.F16 else 0x7f80)
    u = lambda *v: np.array(v, np.uint16)      # noqa: E731
    # MAX: (b > a) ? b : a with a = inout; NaN and +-0 go by role
    assert H.op(100, dtype, u(qnan, one, 0x8000, 0), u(one, qnan, 0, 0x8000)).tolist() == [one, qnan, 0, 0x8000]
    assert H.op(101, dtype, u(qnan, one, 0x8000, inf), u(one, qnan, 0, one)).tolist() == [one, qnan, 0, one]
    assert H.op(104, dtype, u(qnan, 0x8000, 1), u(one, one, one)).tolist() == [one, 0, one]
    assert H.op(106, dtype, u(0x8000, 0, qnan), u(0, 0x8000, 0)).tolist() == [0, 0, one]
    assert H.op(108, dtype, u(1, 0, qnan), u(inf, 0x8000, one)).tolist() == [0, 0, 0]
    assert H.widen(dtype, u(one))[0] == 1.0
    assert H.narrow(dtype, H.widen(dtype, np.arange(0x7c00, dtype=np.uint16))).tolist() == list(range(0x7c00))
