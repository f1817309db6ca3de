"""CPU: plans of the extension datatypes MVX_FLOAT16 / MVX_BFLOAT16.

The algorithm choice is the reference's for a 2-byte predefined type
(count * 2 against its byte thresholds): it must equal the oracle's for
MPI_SHORT on both sides of every threshold.  For the five role-free ops the
whole plan equals MPI_SHORT's but for the handle; MAX and MIN are
role-sensitive (NaN, +-0), as on MPI_FLOAT.
"""
import ctypes

import pytest

import half_ref as H

MPI_SHORT = 4
PS = [1, 2, 3, 4, 5, 6, 7, 8, 12, 33]
SYMMETRIC_OPS = (102, 103, 104, 106, 108)


def _counts():
    """Elements around every byte threshold of the reference at 2 bytes each:
    the coll_table entries (2 KiB .. 64 KiB), the _SMP_ knobs' defaults (1 KiB
    Reduce, 32 KiB Allreduce), the Reduce_scatter 512 KiB switch; and a few
    small counts below the rank count."""
    out = {1, 3, 5, 40, 300}
    for nbytes in (1 << 10, 2 << 10, 4 << 10, 8 << 10, 16 << 10, 32 << 10, 64 << 10, 128 << 10, 256 << 10,
                   512 << 10, 1 << 20):
        out |= {nbytes // 2 - 1, nbytes // 2, nbytes // 2 + 1}
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
    for n in (1023, 1024, 1025, 262143, 262144, 511, 512, 513, 16383, 16384, 16385):
        assert n in COUNTS


@pytest.mark.parametrize("p", PS)
def test_algorithm_is_the_reference_choice_for_two_byte_elements(mvx, oracle, p):
    smp = mvx.smp_tuning()
    seen = set()
    for coll in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE, mvx.COLL_REDUCE_SCATTER, mvx.COLL_SCAN):
        for n in COUNTS:
            if coll == mvx.COLL_SCAN:
                want = mvx.ALG_SCAN_RECDBL           # the oracle names no algorithm for Scan: there is one
                assert mvx.algorithm(coll, p, n, MPI_SHORT) == want
            else:
                want = oracle.algorithm(coll, p, n, MPI_SHORT)
            want_smp = mvx.algorithm(coll, p, n, MPI_SHORT, tuning=smp)
            for h in H.TYPES:
                assert mvx.algorithm(coll, p, n, h) == want, (coll, p, n, h)
                assert mvx.algorithm(coll, p, n, h, tuning=smp) == want_smp, (coll, p, n, h)
            seen.add((coll, want))
            # the _SMP_ defaults in bytes: count * 2 < 1 KiB (Reduce), 32 KiB (Allreduce)
            if coll == mvx.COLL_ALLREDUCE:
                assert (want_smp == mvx.ALG_SMP_LEADER) == (2 * n < (1 << 15))
            if coll == mvx.COLL_REDUCE:
                assert (want_smp == mvx.ALG_SMP_LEADER) == (2 * n < (1 << 10))
    if p >= 4:      # both sides of the switches were really visited
        assert {(mvx.COLL_ALLREDUCE, mvx.ALG_RECDBL), (mvx.COLL_ALLREDUCE, mvx.ALG_RABENSEIFNER),
                (mvx.COLL_REDUCE, mvx.ALG_BINOMIAL), (mvx.COLL_REDUCE, mvx.ALG_RABENSEIFNER),
                (mvx.COLL_REDUCE_SCATTER, mvx.ALG_RS_HALVING), (mvx.COLL_REDUCE_SCATTER, mvx.ALG_RS_PAIRWISE)} <= seen


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("h", H.TYPES)
def test_symmetric_op_plans_equal_shorts_but_for_the_handle(mvx, p, h):
    for coll in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE, mvx.COLL_REDUCE_SCATTER, mvx.COLL_SCAN):
        root = p // 2 if coll == mvx.COLL_REDUCE else 0
        for n in COUNTS:
            for op in SYMMETRIC_OPS:
                ref = _plans(mvx, coll, p, n, MPI_SHORT, op, root)
                got = _plans(mvx, coll, p, n, h, op, root)
                for r in range(p):
                    assert got[r].dtype == h and got[r].symmetric == 1 and got[r].esize == 2
                    assert _image(got[r], dtype=MPI_SHORT) == _image(ref[r]), (coll, p, n, op, r)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("h", H.TYPES)
def test_max_min_plans_are_role_sensitive(mvx, p, h):
    """symmetric == 0, as for MPI_FLOAT (MPI_SHORT's MAX / MIN are role-free);
    the algorithm is still the 2-byte choice."""
    for coll in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE, mvx.COLL_REDUCE_SCATTER, mvx.COLL_SCAN):
        root = p - 1 if coll == mvx.COLL_REDUCE else 0
        for n in COUNTS:
            for op in (100, 101):
                ref = _plans(mvx, coll, p, n, MPI_SHORT, op, root)
                got = _plans(mvx, coll, p, n, h, op, root)
                flt = _plans(mvx, coll, p, n, 10, op, root)
                for r in range(p):
                    assert got[r].symmetric == 0 and flt[r].symmetric == 0 and ref[r].symmetric == 1
                    assert (got[r].alg, got[r].esize, got[r].count) == (ref[r].alg, 2, ref[r].count)


@pytest.mark.parametrize("h", H.TYPES)
def test_undefined_ops_are_reported_by_the_ranks_that_call_the_op(mvx, h):
    """BAND on a 16-bit float: the plan marks the same ranks as BAND on
    MPI_FLOAT (every rank whose schedule calls the op answers 329)."""
    for coll in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE, mvx.COLL_REDUCE_SCATTER, mvx.COLL_SCAN):
        for p in (1, 3, 4, 7, 12):
            for op in H.UNDEFINED_OPS:
                got = [P.calls_uop for P in _plans(mvx, coll, p, 40, h, op, 0)]
                ref = [P.calls_uop for P in _plans(mvx, coll, p, 20, 10, 105, 0)]     # 80 bytes either way
                assert got == ref, (coll, p, op)


@pytest.mark.parametrize("p", [1, 2, 3, 5, 8, 12])
@pytest.mark.parametrize("h", H.TYPES)
def test_plans_with_the_reference_op_equal_the_oracles_float_collective(mvx, oracle, p, h):
    """MAX, MIN and the logical ops never round: each rank's plan evaluated
    with half_ref's op == the oracle's MPI_FLOAT collective (the reference's
    schedule) on the exactly widened inputs, narrowed -- at counts where 2-
    and 4-byte elements take the same algorithm.  Ties half_ref's evaluators
    and the plans' operand roles to the reference without a GPU."""
    import numpy as np
    for n in (1, 5, 300):
        S = [H.coll_vec(h, n, 77 * p + 5 * r + n, special=0.33) for r in range(p)]
        F = [H.widen(h, s) for s in S]
        for op in (100, 101, 104, 106, 108):
            assert mvx.algorithm(mvx.COLL_ALLREDUCE, p, n, h) == oracle.algorithm(mvx.COLL_ALLREDUCE, p, n, 10)
            R = [np.zeros(n, np.float32) for _ in range(p)]
            assert oracle.allreduce([f.view(np.uint8) for f in F], [r.view(np.uint8) for r in R], n, 10, op) == [0] * p
            plans = [mvx.plan(mvx.COLL_ALLREDUCE, p, r, n, h, op) for r in range(p)]
            got = H.run_plans(plans, [s.view(np.uint8) for s in S], [np.zeros(2 * n, np.uint8) for _ in range(p)])
            for r in range(p):
                assert np.array_equal(got[r].view(np.uint16), H.narrow(h, R[r])), (p, n, op, r)
            R = [np.zeros(n, np.float32) for _ in range(p)]
            assert oracle.scan([f.view(np.uint8) for f in F], [r.view(np.uint8) for r in R], n, 10, op) == [0] * p
            plans = [mvx.plan(mvx.COLL_SCAN, p, r, n, h, op) for r in range(p)]
            got = H.run_plans(plans, [s.view(np.uint8) for s in S], [np.zeros(2 * n, np.uint8) for _ in range(p)])
            for r in range(p):
                assert np.array_equal(got[r].view(np.uint16), H.narrow(h, R[r])), ("scan", p, n, op, r)
