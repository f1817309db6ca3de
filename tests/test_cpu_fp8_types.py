"""CPU: the extension datatypes MVX_FLOAT8_E4M3 (72) and MVX_FLOAT8_E5M2 (73)
in the type engine, the (op, type) support matrix, the launch plans and the
Python constants; and the test reference tests/fp8_ref.py against fixed values
and against itself.
"""
import os
import re

import numpy as np
import pytest

import fp8_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPI_UNSIGNED_CHAR, MPI_INT = 2, 6
K_BASIC = 0
TYPE_NULL = 3 | (5 << 6)        # MVX_ERR_TYPE_NULL
TNAME = {H.E4M3: "f8e4m3", H.E5M2: "f8e5m2"}


@pytest.mark.parametrize("h", H.TYPES)
def test_extent_size_alignment_dense_basic(mvx, h):
    assert mvx.dtype_info(h) == (1, 1)
    assert mvx.hip().mvx_dtype_extent(h) == 1
    assert mvx.MPI_Type_extent(h) == (0, 1) and mvx.MPI_Type_size(h) == (0, 1)
    assert mvx.type_layout(h) == dict(kind=K_BASIC, dense=1, lb=0, ub=1, span_lo=0, span_hi=1)
    assert mvx.MPI_Type_commit(h) == 0
    assert mvx.MPI_Type_free(h)[0] == 3 | (9 << 6)          # permanent, as every basic handle
    # alignment 1: a struct {char, fp8, fp8} is three bytes, no padding
    rc, s = mvx.MPI_Type_struct(3, [1, 1, 1], [0, 1, 2], [1, h, h])
    assert rc == 0 and mvx.MPI_Type_extent(s) == (0, 3)
    rc, s3 = mvx.MPI_Type_struct(2, [1, 1], [0, 4], [h, MPI_INT])
    assert rc == 0 and mvx.MPI_Type_extent(s3) == (0, 8)
    mvx.MPI_Type_free(s)
    mvx.MPI_Type_free(s3)


def test_constants_and_headers(mvx):
    assert (mvx.MVX_FLOAT8_E4M3, mvx.MVX_FLOAT8_E5M2) == (72, 73) == H.TYPES
    assert mvx.NP_DTYPE[72] == np.dtype(np.uint8) and mvx.NP_DTYPE[73] == np.dtype(np.uint8)
    assert mvx.TYPE_NAMES[72] == "MVX_FLOAT8_E4M3" and mvx.TYPE_NAMES[73] == "MVX_FLOAT8_E5M2"
    assert sorted(mvx.DEFINED_EXT8) == sorted(H.OPS)
    for op in range(100, 112):
        assert mvx.DEFINED_EXT8.get(op, []) == ([72, 73] if op in H.OPS else [])
        assert mvx.DEFINED_EXT.get(op, []) == ([64, 65] if op in H.OPS else [])      # untouched
        assert 72 not in mvx.DEFINED[op] and 73 not in mvx.DEFINED[op]               # the reference's table
    for header in ("mvx_mpi.h", "mvx_embed.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert re.search(r"#define\s+MVX_FLOAT8_E4M3\s+72\b", text), header
        assert re.search(r"#define\s+MVX_FLOAT8_E5M2\s+73\b", text), header


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
        assert mvx.hip().mvx_op_element_size(op, h) == (1 if op in H.OPS else 0)
    assert mvx.hip().mvx_op_apply(99, h, None, None, 0, None) == mvx.MPI_ERR_OP
    assert mvx.hip().mvx_op_apply(112, h, None, None, 0, None) == mvx.MPI_ERR_OP
    derived = [mvx.MPI_Type_contiguous(2, h), mvx.MPI_Type_contiguous(1, h), mvx.MPI_Type_vector(3, 1, 2, h),
               mvx.MPI_Type_struct(2, [1, 1], [0, 4], [h, MPI_INT]),
               mvx.MPI_Type_struct(2, [1, 1], [0, 1], [h, h])]
    for rc, d in derived:
        assert rc == 0
        assert _verdicts(mvx, d) == [329] * 12, d
        mvx.MPI_Type_free(d)


def _bounds(mvx, t):
    return (mvx.MPI_Type_extent(t), mvx.MPI_Type_size(t), mvx.MPI_Type_lb(t), mvx.MPI_Type_ub(t),
            mvx.type_layout(t))


@pytest.mark.parametrize("h", H.TYPES)
def test_constructors_give_the_bounds_of_unsigned_char(mvx, h):
    """Every constructor over a new type == the same constructor over
    MPI_UNSIGNED_CHAR (the constructors of
    test_cpu_half_types.py::test_constructors_give_the_bounds_of_short)."""
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
        (rc_a, a), (rc_b, b) = mk(h), mk(MPI_UNSIGNED_CHAR)
        assert rc_a == rc_b == 0, i
        assert mvx.MPI_Type_commit(a) == mvx.MPI_Type_commit(b) == 0
        assert _bounds(mvx, a) == _bounds(mvx, b), i
        # one level up: the derived type as an old type
        (rc_a2, a2), (rc_b2, b2) = mvx.MPI_Type_vector(2, 1, 3, a), mvx.MPI_Type_vector(2, 1, 3, b)
        assert rc_a2 == rc_b2 == 0 and _bounds(mvx, a2) == _bounds(mvx, b2), i
        for t in (a2, b2, a, b):
            mvx.MPI_Type_free(t)


@pytest.mark.parametrize("h", [71, 74])
def test_neighbouring_handles_stay_unknown(mvx, h):
    with pytest.raises(ValueError):
        mvx.dtype_info(h)
    assert mvx.hip().mvx_dtype_extent(h) == 0
    assert mvx.MPI_Type_contiguous(2, h)[0] == TYPE_NULL
    assert mvx.MPI_Type_extent(h)[0] != 0
    assert _verdicts(mvx, h) == [329] * 12
    assert not any(mvx.hip().mvx_op_supported(op, h) for op in range(100, 112))


# ------------------------------------------------------------- launch plans

@pytest.mark.parametrize("h", H.TYPES)
def test_launch_plans_name_the_element_type_and_keep_the_byte_grids(mvx, h):
    """mvx_op_plan (no device): the apply, a 3-leaf tree and an 8-leaf tree
    carry the new element type's name and have MPI_UNSIGNED_CHAR's grid for
    the same n; n = 0 plans nothing."""
    base = 1 << 32
    tree = mvx.hip().mvx_tree_mask
    for op in H.OPS:
        for k, tmask, kern in ((2, 1, "k_combine<%d, " % (op - 100)), (3, tree(3), "k_combine<%d, " % (op - 100)),
                               (8, tree(8), None)):
            srcs = [base * (q + 1) for q in range(k)]
            dst = srcs[0] if k == 2 else base * 40
            for n in (1, 15, 16, 17, 4099, 16 * 3372, 1 << 26):
                rc, p = mvx.op_plan(op, h, srcs, dst, n, tmask, 0)
                rc8, p8 = mvx.op_plan(op, MPI_UNSIGNED_CHAR, srcs, dst, n, tmask, 0)
                assert rc == rc8 == 0
                sym, sym8 = p.symbol.decode(), p8.symbol.decode()
                assert TNAME[h] in sym and TNAME[h] not in sym8, (sym, sym8)
                if kern:
                    assert sym.startswith(kern), sym
                else:       # the 8-leaf tree: the body kernel for a large launch, else k_combine's fixed tree
                    assert sym.startswith(("k_tree_body<%d, " % (op - 100), "k_combine<%d, " % (op - 100))), sym
                    assert sym.startswith("k_tree_body") == (n == 1 << 26), (sym, n)
                # the same kernel template but for the element type
                assert sym.replace("mvx::" + TNAME[h], "T").split("<")[0] == sym8.split("<")[0]
                assert sym.split(", ")[2:] == sym8.split(", ")[2:], (sym, sym8)
                assert (p.blocks, p.dynamic_lds) == (p8.blocks, p8.dynamic_lds), (op, k, n)
            rc, p = mvx.op_plan(op, h, srcs, dst, 0, tmask, 0)
            assert rc == 0 and p.blocks == 0 and p.symbol.decode() == ""
    for op in H.UNDEFINED_OPS:
        assert mvx.op_plan(op, h, [base, 2 * base], base, 5, 1, 0)[0] == 329
    assert mvx.op_plan(99, h, [base, 2 * base], base, 5, 1, 0)[0] == mvx.MPI_ERR_OP


# ------------------------------------------------ the reference helper itself

def _all_pairs():
    v = np.arange(256, dtype=np.uint8)
    return np.repeat(v, 256), np.tile(v, 256)


@pytest.mark.parametrize("dtype,tname", [(H.E4M3, "float8_e4m3fn"), (H.E5M2, "float8_e5m2")])
def test_reference_decode_table_equals_torch(dtype, tname):
    torch = pytest.importorskip("torch")
    if not hasattr(torch, tname):
        pytest.skip("torch without " + tname)
    allb = np.arange(256, dtype=np.uint8)
    t = torch.from_numpy(allb.copy()).view(getattr(torch, tname)).to(torch.float64).numpy()
    d = H.DECODE[dtype]
    nan = np.isnan(d)
    assert np.array_equal(np.isnan(t), nan)
    assert np.array_equal(t[~nan], d[~nan]) and np.array_equal(np.signbit(t), np.signbit(d))


@pytest.mark.parametrize("dtype", H.TYPES)
def test_reference_format_edges(dtype):
    d = H.DECODE[dtype]
    if dtype == H.E4M3:
        assert d[0x7E] == 448 and d[0x01] == 2.0 ** -9 and d[0x38] == 1.0 and d[0x08] == 2.0 ** -6
        assert np.isnan(d[0x7F]) and np.isnan(d[0xFF]) and int(np.isnan(d).sum()) == 2 and not np.isinf(d).any()
    else:
        assert d[0x7B] == 57344 and d[0x01] == 2.0 ** -16 and d[0x3C] == 1.0 and d[0x04] == 2.0 ** -14
        assert d[0x7C] == np.inf and d[0xFC] == -np.inf
        assert np.isnan(d[[0x7D, 0x7E, 0x7F, 0xFD, 0xFE, 0xFF]]).all() and int(np.isnan(d).sum()) == 6
    assert np.signbit(d[0x80]) and d[0x80] == 0 and not np.signbit(d[0])
    fin = np.isfinite(d)
    assert np.array_equal(H.encode(dtype, d[fin]), np.arange(256, dtype=np.uint8)[fin])       # every value encodes to itself
    assert np.array_equal(np.diff(d[:H.MAX_FINITE[dtype] + 1]) > 0, np.ones(H.MAX_FINITE[dtype], bool))


# (NaN, inf, finite pairs that overflow) of all 65,536 results
NONFINITE = {(H.E4M3, 102): (1456, 0, 436), (H.E4M3, 103): (11140, 0, 10120),
             (H.E5M2, 102): (3038, 1114, 120), (H.E5M2, 103): (3044, 9180, 8192)}


@pytest.mark.parametrize("dtype", H.TYPES)
@pytest.mark.parametrize("opn", [102, 103])
def test_reference_sum_prod_equal_f32_arithmetic_narrowed_once(dtype, opn):
    """All 65,536 pairs: the exact float64 result rounded once == float32
    arithmetic narrowed by the helper (the double-rounding claim the kernels
    rest on), and the non-finite results are exactly the expected ones."""
    a, b = _all_pairs()
    for inv, io in ((a, b), (b, a)):
        r = H.op_direct(opn, dtype, inv, io)
        assert np.array_equal(r, H.op_via_f32(opn, dtype, inv, io))
        assert np.array_equal(r, H.op(opn, dtype, inv, io))        # and the helper's table of it
    w = H.widen(dtype, r)
    fin = np.isfinite(H.widen(dtype, a)) & np.isfinite(H.widen(dtype, b))
    assert (int(np.isnan(w).sum()), int(np.isinf(w).sum()), int((fin & ~np.isfinite(w)).sum())) == NONFINITE[dtype, opn]
    # exactness of the float64 route: operands and result survive a trip through longdouble
    x, y = H.widen(dtype, a), H.widen(dtype, b)
    with np.errstate(all="ignore"):
        e64 = x + y if opn == 102 else x * y
        eld = x.astype(np.longdouble) + y if opn == 102 else x.astype(np.longdouble) * y
    ok = np.isfinite(e64)
    assert np.array_equal(e64[ok].astype(np.longdouble), eld[ok])


def test_reference_spot_values():
    u = lambda *v: np.array(v, np.uint8)      # noqa: E731
    n4 = lambda x: int(H.narrow(H.E4M3, np.array([x]))[0])      # noqa: E731
    n5 = lambda x: int(H.narrow(H.E5M2, np.array([x]))[0])      # noqa: E731
    assert H.op(102, H.E4M3, u(n4(16.0)), u(0x7E)).tolist() == [0x7E]          # 448 + 16: the tie 464 -> 448
    assert H.isnan(H.E4M3, H.op(102, H.E4M3, u(n4(32.0)), u(0x7E))).all()      # 448 + 32 -> NaN
    assert H.op(102, H.E5M2, u(n5(4096.0)), u(0x7B)).tolist() == [0x7C]        # 57344 + 4096: the tie 61440 -> inf
    assert H.op(102, H.E5M2, u(n5(2048.0)), u(0x7B)).tolist() == [0x7B]
    for dt in H.TYPES:
        assert H.op(102, dt, u(0x80), u(0x80)).tolist() == [0x80]               # -0 + -0
        assert H.op(102, dt, u(0x80), u(0x00)).tolist() == [0x00]               # +0 + -0
        assert H.op(102, dt, u(0x00), u(0x80)).tolist() == [0x00]
        assert H.op(103, dt, u(0x80), u(H.ONE[dt])).tolist() == [0x80]
    e = lambda dt, x: int(H.encode(dt, np.array([x]))[0])      # noqa: E731
    assert [e(H.E4M3, x) for x in (464.0, 464.5, 480.0, -464.0)] == [0x7E, 0x7F, 0x7F, 0xFE]
    assert H.isnan(H.E4M3, u(e(H.E4M3, -465.0))).all()
    assert [e(H.E5M2, x) for x in (61439.0, 61440.0, -61440.0, 1e9)] == [0x7B, 0x7C, 0xFC, 0x7C]
    assert [e(H.E4M3, x) for x in (2.0 ** -10, 2.0 ** -10 * 1.01, 3 * 2.0 ** -10, 2.0 ** -9)] == [0, 1, 2, 1]   # subnormal ties


@pytest.mark.parametrize("dtype", H.TYPES)
def test_reference_selects_and_logicals(dtype):
    one, qnan, big = H.ONE[dtype], H.NAN[dtype], H.MAX_FINITE[dtype]
    u = lambda *v: np.array(v, np.uint8)      # noqa: E731
    # MAX: (b > a) ? b : a with a = inout; NaN and +-0 go by role
    assert H.op(100, dtype, u(qnan, one, 0x80, 0), u(one, qnan, 0, 0x80)).tolist() == [one, qnan, 0, 0x80]
    assert H.op(101, dtype, u(qnan, one, 0x80, big), u(one, qnan, 0, one)).tolist() == [one, qnan, 0, one]
    assert H.op(100, dtype, u(big, one | 0x80), u(one, big | 0x80)).tolist() == [big, one | 0x80]
    assert H.op(104, dtype, u(qnan, 0x80, 1), u(one, one, one)).tolist() == [one, 0, one]
    assert H.op(106, dtype, u(0x80, 0, qnan), u(0, 0x80, 0)).tolist() == [0, 0, one]
    assert H.op(108, dtype, u(1, 0, qnan), u(big, 0x80, one)).tolist() == [0, 0, 0]
    assert H.widen(dtype, u(one))[0] == 1.0


@pytest.mark.parametrize("dtype", H.TYPES)
def test_rand_bits_keeps_the_nan_share_small(dtype):
    """The input distribution of the GPU tests: an 8-leaf tree with every odd
    leaf folded stays under 3 % NaN (uniform bytes would not)."""
    n = 20000
    S = [H.rand_bits(dtype, n, q) for q in range(8)]
    F = [H.rand_bits(dtype, n, 50 + q) if q % 2 else None for q in range(8)]
    for opn in (102, 103):
        assert H.nan_share(dtype, H.combine(opn, dtype, S, F, 0, n)) < 0.035
