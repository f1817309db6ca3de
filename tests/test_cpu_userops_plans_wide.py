"""CPU: libmvx.so's plans for user-defined ops above 8 ranks.

tests/test_cpu_userops_plans.py's four tests at p = 9..64 (the chains of trees
of DESIGN.md section 2d: up to 64 leaves, tree_swap, a 64-bit chain_swap), for
the noncommutative `mix` under both commute flags and the associative,
noncommutative `affine`.  Each rank's plan runs on the CPU (tests/plan_exec.py)
with the C user function the oracle's replay calls; results are bit-identical.
"""
import numpy as np
import pytest

import uops
from plan_exec import run_plans

H = 240
KINDS = {1: 1, 0: 2}   # commute flag -> OPKIND
PS = [9, 12, 16, 17, 31, 32, 33, 47, 48, 63, 64]
CASES = [("mix", 0), ("mix", 1), ("affine", 0)]
COUNTS = (1, 65, 1000)


def _sends(name, p, n, seed):
    return [uops.rand_for(name, n, seed + 7 * r) for r in range(p)]


def _setup(oracle, name, commute):
    assert oracle.user_op_set(H, uops.host_fn(name), commute) == 0
    return uops.UOPS[name][0], KINDS[commute]


def _u8(arrays):
    return [a.view(np.uint8) for a in arrays]


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name,commute", CASES)
def test_user_allreduce_plans_wide(mvx, oracle, p, name, commute):
    dt, kind = _setup(oracle, name, commute)
    for n in COUNTS:
        S = _sends(name, p, n, 100 * p + n)
        R0 = [np.zeros_like(S[0]) for _ in range(p)]
        assert oracle.allreduce(_u8(S), _u8(R0), n, dt, H) == [0] * p
        plans = [mvx.plan(mvx.COLL_ALLREDUCE, p, r, n, dt, H, opkind=kind) for r in range(p)]
        assert plans[0].alg == mvx.ALG_RECDBL
        assert max(P.k for P in plans) == 1 << (p.bit_length() - 1)       # the power of two below p
        R1 = run_plans(plans, _u8(S), [np.zeros(S[0].nbytes, np.uint8) for _ in range(p)])
        for r in range(p):
            assert np.array_equal(R1[r].view(S[0].dtype), R0[r]), (n, r)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name,commute", CASES)
def test_user_reduce_plans_wide(mvx, oracle, p, name, commute):
    dt, kind = _setup(oracle, name, commute)
    for n in COUNTS:
        S = _sends(name, p, n, 50 * p + n)
        for root in sorted({0, p // 2, p - 1}):
            R0 = [np.zeros_like(S[0]) for _ in range(p)]
            oracle.reduce(_u8(S), _u8(R0), n, dt, H, root)
            plans = [mvx.plan(mvx.COLL_REDUCE, p, r, n, dt, H, root, opkind=kind) for r in range(p)]
            assert plans[0].alg == mvx.ALG_BINOMIAL and plans[root].k == p
            R1 = run_plans(plans, _u8(S), [np.zeros(S[0].nbytes, np.uint8) for _ in range(p)])
            assert np.array_equal(R1[root].view(S[0].dtype), R0[root]), (n, root)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name,commute", CASES)
def test_user_scan_plans_wide(mvx, oracle, p, name, commute):
    dt, kind = _setup(oracle, name, commute)
    for n in COUNTS:
        S = _sends(name, p, n, 30 * p + n)
        R0 = [np.zeros_like(S[0]) for _ in range(p)]
        oracle.scan(_u8(S), _u8(R0), n, dt, H)
        plans = [mvx.plan(mvx.COLL_SCAN, p, r, n, dt, H, opkind=kind) for r in range(p)]
        assert plans[p - 1].k == p
        R1 = run_plans(plans, _u8(S), [np.zeros(S[0].nbytes, np.uint8) for _ in range(p)])
        for r in range(p):
            assert np.array_equal(R1[r].view(S[0].dtype), R0[r]), (n, r)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("name,commute", CASES)
def test_user_reduce_scatter_plans_wide(mvx, oracle, p, name, commute):
    dt, kind = _setup(oracle, name, commute)
    E = np.dtype(uops.UOPS[name][2]).itemsize
    seen = set()
    high = False
    for base in (1, 5, 30, 3000):
        cnts = [max(0, base + (r % 3) - 1) for r in range(p)]
        total = sum(cnts)
        S = _sends(name, p, total, 9 * p + base)
        R0 = [np.zeros(max(c, 1), S[0].dtype) for c in cnts]
        oracle.reduce_scatter(_u8(S), _u8(R0), cnts, dt, H)
        plans = [mvx.plan(mvx.COLL_REDUCE_SCATTER, p, r, 0, dt, H, recvcnts=cnts, opkind=kind) for r in range(p)]
        assert plans[0].alg == oracle.algorithm(3, p, total, dt, H)
        seen.add(plans[0].alg)
        high |= any(P.chain_swap >> 32 for P in plans)
        R1 = run_plans(plans, _u8(S), [np.zeros(max(c, 1) * E, np.uint8) for c in cnts])
        for r in range(p):
            assert np.array_equal(R1[r][: cnts[r] * E].view(S[0].dtype), R0[r][: cnts[r]]), (base, r, cnts)
    if commute == 0:
        assert mvx.ALG_RS_PAIRWISE in seen, seen
        assert high == (p > 32)          # role swaps of leaves 32..: the mask's upper half
