"""CPU: plans of the extension datatypes MVX_FLOAT8_E4M3 / MVX_FLOAT8_E5M2.

The algorithm choice is the reference's for a 1-byte predefined type
(count * 1 against its byte thresholds): it must equal the oracle's for
MPI_UNSIGNED_CHAR on both sides of every threshold, in both device flavours.
For the five role-free ops the whole plan equals MPI_UNSIGNED_CHAR's but for
the handle; MAX and MIN are role-sensitive (NaN, +-0), as on MPI_FLOAT.
"""
import ctypes

import numpy as np
import pytest

import fp8_ref as H

MPI_UNSIGNED_CHAR = 2
PS = [1, 2, 3, 4, 5, 6, 7, 8, 12, 33]
SYMMETRIC_OPS = (102, 103, 104, 106, 108)


def _counts():
    """Elements around every byte threshold of the reference at 1 byte each:
    the coll_table entries (2 KiB .. 64 KiB), the _SMP_ knobs' defaults (1 KiB
    Reduce, 32 KiB Allreduce), the Reduce_scatter 512 KiB switch; and a few
    small counts below the rank count."""
    out = {1, 3, 5, 40, 300}
    for nbytes in (1 << 10, 2 << 10, 4 << 10, 8 << 10, 16 << 10, 32 << 10, 64 << 10, 128 << 10, 256 << 10,
                   512 << 10, 1 << 20):
        out |= {nbytes - 1, nbytes, nbytes + 1}
    return sorted(out)


COUNTS = _counts()


def _cnts(n, p):
    return [n // p + (1 if r < n % p else 0) for r in range(p)]


def _plans(mvx, coll, p, n, dtype, op, root, tuning=None):
    rc = _cnts(n, p) if coll == mvx.COLL_REDUCE_SCATTER else None
    return [mvx.plan(coll, p, r, n, dtype, op, root, recvcnts=rc, tuning=tuning) for r in range(p)]


def _image(P, dtype=None):
    """The plan's bytes (mvx_plan_build zeroes the struct first), with the
    handle replaced."""
    Q = type(P)()
    ctypes.memmove(ctypes.byref(Q), ctypes.byref(P), ctypes.sizeof(P))
    if dtype is not None:
        Q.dtype = dtype
    return bytes(Q)


def test_counts_straddle_every_threshold():
    for n in (1023, 1024, 1025, 2047, 2048, 2049, 32767, 32768, 32769, 524287, 524288, 524289):
        assert n in COUNTS


@pytest.mark.parametrize("p", PS)
def test_algorithm_is_the_reference_choice_for_one_byte_elements(mvx, oracle, p):
    smp = mvx.smp_tuning()
    seen = set()
    for coll in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE, mvx.COLL_REDUCE_SCATTER, mvx.COLL_SCAN):
        for n in COUNTS:
            if coll == mvx.COLL_SCAN:
                want = mvx.ALG_SCAN_RECDBL           # the oracle names no algorithm for Scan: there is one
                assert mvx.algorithm(coll, p, n, MPI_UNSIGNED_CHAR) == want
            else:
                want = oracle.algorithm(coll, p, n, MPI_UNSIGNED_CHAR)
            want_smp = mvx.algorithm(coll, p, n, MPI_UNSIGNED_CHAR, tuning=smp)
            for h in H.TYPES:
                assert mvx.algorithm(coll, p, n, h) == want, (coll, p, n, h)
                assert mvx.algorithm(coll, p, n, h, tuning=smp) == want_smp, (coll, p, n, h)
            seen.add((coll, want))
            # the _SMP_ defaults in bytes: count * 1 < 1 KiB (Reduce), 32 KiB (Allreduce)
            if coll == mvx.COLL_ALLREDUCE:
                assert (want_smp == mvx.ALG_SMP_LEADER) == (n < (1 << 15))
            if coll == mvx.COLL_REDUCE:
                assert (want_smp == mvx.ALG_SMP_LEADER) == (n < (1 << 10))
    if p >= 4:      # both sides of the switches were really visited
        assert {(mvx.COLL_ALLREDUCE, mvx.ALG_RECDBL), (mvx.COLL_ALLREDUCE, mvx.ALG_RABENSEIFNER),
                (mvx.COLL_REDUCE, mvx.ALG_BINOMIAL), (mvx.COLL_REDUCE, mvx.ALG_RABENSEIFNER),
                (mvx.COLL_REDUCE_SCATTER, mvx.ALG_RS_HALVING), (mvx.COLL_REDUCE_SCATTER, mvx.ALG_RS_PAIRWISE)} <= seen


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("h", H.TYPES)
def test_symmetric_op_plans_equal_unsigned_chars_but_for_the_handle(mvx, p, h):
    smp = mvx.smp_tuning()
    for coll in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE, mvx.COLL_REDUCE_SCATTER, mvx.COLL_SCAN):
        root = p // 2 if coll == mvx.COLL_REDUCE else 0
        for n in COUNTS:
            for op in SYMMETRIC_OPS:
                ref = _plans(mvx, coll, p, n, MPI_UNSIGNED_CHAR, op, root)
                got = _plans(mvx, coll, p, n, h, op, root)
                for r in range(p):
                    assert got[r].dtype == h and got[r].symmetric == 1 and got[r].esize == 1
                    assert _image(got[r], dtype=MPI_UNSIGNED_CHAR) == _image(ref[r]), (coll, p, n, op, r)
        for n in (5, 1023, 1024, 32767, 32768):          # the other device flavour
            ref = _plans(mvx, coll, p, n, MPI_UNSIGNED_CHAR, 102, root, tuning=smp)
            got = _plans(mvx, coll, p, n, h, 102, root, tuning=smp)
            for r in range(p):
                assert _image(got[r], dtype=MPI_UNSIGNED_CHAR) == _image(ref[r]), ("smp", coll, p, n, r)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("h", H.TYPES)
def test_max_min_plans_are_role_sensitive(mvx, p, h):
    """symmetric == 0, as for MPI_FLOAT (MPI_UNSIGNED_CHAR's MAX / MIN are
    role-free); the algorithm is still the 1-byte choice."""
    for coll in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE, mvx.COLL_REDUCE_SCATTER, mvx.COLL_SCAN):
        root = p - 1 if coll == mvx.COLL_REDUCE else 0
        for n in COUNTS:
            for op in (100, 101):
                ref = _plans(mvx, coll, p, n, MPI_UNSIGNED_CHAR, op, root)
                got = _plans(mvx, coll, p, n, h, op, root)
                flt = _plans(mvx, coll, p, n, 10, op, root)
                for r in range(p):
                    assert got[r].symmetric == 0 and flt[r].symmetric == 0 and ref[r].symmetric == 1
                    assert (got[r].alg, got[r].esize, got[r].count) == (ref[r].alg, 1, ref[r].count)


@pytest.mark.parametrize("h", H.TYPES)
def test_undefined_ops_are_reported_by_the_ranks_that_call_the_op(mvx, h):
    """BAND on an 8-bit float: the plan marks the same ranks as BAND on
    MPI_FLOAT (every rank whose schedule calls the op answers 329)."""
    for coll in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE, mvx.COLL_REDUCE_SCATTER, mvx.COLL_SCAN):
        for p in (1, 3, 4, 7, 12):
            for op in H.UNDEFINED_OPS:
                got = [P.calls_uop for P in _plans(mvx, coll, p, 80, h, op, 0)]
                ref = [P.calls_uop for P in _plans(mvx, coll, p, 20, 10, 105, 0)]     # 80 bytes either way
                assert got == ref, (coll, p, op)


def _straight(coll, opn, dtype, S, n, cnts, root):
    """The collective evaluated straight in the helper: rank order, rank 0's
    contribution as the first inout.  Used only for the ops whose result does
    not depend on the association (below)."""
    p = len(S)
    pre = [S[0].copy()]
    for r in range(1, p):
        pre.append(H.op(opn, dtype, S[r], pre[-1]))
    if coll == "scan":
        return pre
    if coll == "rs":
        off = np.cumsum([0] + cnts)
        return [pre[-1][off[r]:off[r + 1]] for r in range(p)]
    return [pre[-1] if (coll == "ar" or r == root) else None for r in range(p)]


@pytest.mark.parametrize("p", [1, 2, 3, 5, 8, 12])
@pytest.mark.parametrize("h", H.TYPES)
def test_plans_run_by_the_helper_equal_the_straight_collective(mvx, p, h):
    """Every rank's plan run by fp8_ref.run_plans == a straight evaluation of
    the collective in the helper.  The logical ops are associative and
    commutative on any input; MAX / MIN and SUM are checked on inputs where
    every association gives the same bits (no NaN and no zero for the
    selects; one nonzero contributor per element for SUM)."""
    colls = {"ar": mvx.COLL_ALLREDUCE, "red": mvx.COLL_REDUCE, "rs": mvx.COLL_REDUCE_SCATTER, "scan": mvx.COLL_SCAN}
    ints = H.narrow(h, np.array([0.0, 1.0, 2.0, 3.0, 4.0, -1.0, -2.0, 0.5, -0.5]))
    for n in (1, 5, 300, 2049):
        cnts = _cnts(n, p)
        rng = np.random.default_rng(31 * p + n)
        any_bits = [H.coll_vec(h, n, 77 * p + 5 * r + n, special=0.33) for r in range(p)]
        ordered = [H.near_one(h, n, rng) | (rng.integers(0, 2, n) * 0x80).astype(np.uint8) for r in range(p)]
        small = [ints[rng.integers(0, ints.size, n)] for r in range(p)]
        for op, S in ((104, any_bits), (106, any_bits), (108, any_bits), (100, ordered), (101, ordered), (102, small)):
            if op == 102:
                # one contributor per element, +0 from every other rank: each partial sum is exact
                S = [np.where(np.arange(n) % p == r, s, np.uint8(0)) for r, s in enumerate(S)]
            for cname, cid in colls.items():
                root = p - 1 if cname == "red" else 0
                plans = [mvx.plan(cid, p, r, 0 if cname == "rs" else n, h, op, root,
                                  cnts if cname == "rs" else None) for r in range(p)]
                sizes = [max(c, 1) for c in cnts] if cname == "rs" else [n] * p
                got = H.run_plans(plans, [s.copy() for s in S], [np.full(s, 0x5C, np.uint8) for s in sizes])
                want = _straight(cname, op, h, S, n, cnts, root)
                for r in range(p):
                    if want[r] is not None and want[r].size:
                        assert np.array_equal(got[r][:want[r].size], want[r]), (cname, p, n, op, r)


@pytest.mark.parametrize("p", [1, 2, 3, 5, 8, 12])
@pytest.mark.parametrize("h", H.TYPES)
def test_plans_with_the_reference_op_equal_the_oracles_float_collective(mvx, oracle, p, h):
    """MAX, MIN and the logical ops never round: each rank's plan evaluated
    with fp8_ref's op == the oracle's MPI_FLOAT collective (the reference's
    schedule) on the exactly widened inputs, narrowed -- at counts where 1-
    and 4-byte elements take the same algorithm.  Ties fp8_ref's evaluators
    and the plans' operand roles (NaN, +-0) to the reference without a GPU."""
    for n in (1, 5, 300):
        S = [H.coll_vec(h, n, 77 * p + 5 * r + n, special=0.33) for r in range(p)]
        F = [H.widen(h, s).astype(np.float32) for s in S]
        for op in (100, 101, 104, 106, 108):
            assert mvx.algorithm(mvx.COLL_ALLREDUCE, p, n, h) == oracle.algorithm(mvx.COLL_ALLREDUCE, p, n, 10)
            R = [np.zeros(n, np.float32) for _ in range(p)]
            assert oracle.allreduce([f.view(np.uint8) for f in F], [r.view(np.uint8) for r in R], n, 10, op) == [0] * p
            plans = [mvx.plan(mvx.COLL_ALLREDUCE, p, r, n, h, op) for r in range(p)]
            got = H.run_plans(plans, S, [np.zeros(n, np.uint8) for _ in range(p)])
            for r in range(p):
                assert np.array_equal(got[r], H.narrow(h, R[r])), (p, n, op, r)
            R = [np.zeros(n, np.float32) for _ in range(p)]
            assert oracle.scan([f.view(np.uint8) for f in F], [r.view(np.uint8) for r in R], n, 10, op) == [0] * p
            plans = [mvx.plan(mvx.COLL_SCAN, p, r, n, h, op) for r in range(p)]
            got = H.run_plans(plans, S, [np.zeros(n, np.uint8) for _ in range(p)])
            for r in range(p):
                assert np.array_equal(got[r], H.narrow(h, R[r])), ("scan", p, n, op, r)
