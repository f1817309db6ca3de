"""CPU: the launch policy of the reduction kernels, asked through mvx_op_plan.

Which template runs, with how many blocks and which LDS reservation is host
arithmetic on addresses and sizes (choose_family, split and plan in
mvx_ops.hip): nothing is launched, no buffer exists, no device is needed.
Here are the symbol and grid assertions of tests/test_gpu_small_launch.py on
the same cases (small_launch.plan_combine / plan_apply in place of combine /
apply; the GPU tests check on every launch that the plan is what ran), the
default policy at the benchmark's sizes, the alignment rule for every element
size and residue, and the op-side environment knobs, each group in a fresh
process (tests/knob_worker.py GROUP --plan).
"""
import json
import os
import subprocess
import sys

import pytest

import knob_worker
import small_launch as SL
from small_launch import (BODY_NVEC, BODY_PAIRS, COMBINE_FAMILIES, COMBINE_NVEC, MISALIGNED_N, PXI_NVEC, SHAPE_CHAIN,
                          SHAPE_TREE)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "knob_worker.py")
SUM, MAXLOC, FLOAT = 102, 111, 10


@pytest.fixture
def launch(mvx):
    """set(cap, log2): mvx.set_launch with cap None = the default grid; the
    defaults come back whatever the test does."""
    def set_(cap, nt_log2):
        mvx.set_launch(cap or SL.DEFAULT_CAP, nt_log2)
    try:
        yield set_
    finally:
        mvx.set_launch(SL.DEFAULT_CAP, SL.DEFAULT_NT_LOG2)


def _capped(blocks, cap):
    assert blocks >= 1 and (cap is None or blocks <= cap), (blocks, cap)


# ----------------------------- the cases of tests/test_gpu_small_launch.py

@pytest.mark.parametrize("cap", [None, 1, 3])
@pytest.mark.parametrize("op,dtype", BODY_PAIRS)
def test_body_kernels_ragged_sizes_and_grid_stride(mvx, launch, op, dtype, cap):
    launch(cap, 4)
    E = mvx.dtype_info(dtype)[0]
    for nvec in BODY_NVEC:
        n = nvec * 16 // E
        for shape, ks in ((SHAPE_TREE, (4, 8)), (SHAPE_CHAIN, (4, 5, 6, 7, 8))):
            for k in ks:
                sym, blocks = SL.plan_combine(mvx, op, dtype, k, shape, n, seed=k)
                pre, suf = SL.body_symbol(op, k, shape)
                assert sym.startswith(pre) and sym.endswith(suf), (sym, nvec, k, shape)
                _capped(blocks, cap)
                if cap is None:
                    assert blocks == (nvec + 511) // 512


@pytest.mark.parametrize("cap", [None, 1, 3])
@pytest.mark.parametrize("op", [110, 111])
def test_long_double_int_pair_body_ragged(mvx, launch, op, cap):
    launch(cap, 4)
    for n in PXI_NVEC:
        for k in (4, 8):
            sym, blocks = SL.plan_combine(mvx, op, 22, k, SHAPE_TREE, n, seed=k, ties=0.3)
            assert sym == "k_pxi_loc_body<%d, %d, 1>" % (op - 100, k), sym
            _capped(blocks, cap)
        sym, blocks = SL.plan_apply(mvx, None, op, 22, n, seed=n, ties=0.3)
        assert sym == "k_pxi_loc_body<%d, 2, 1>" % (op - 100), sym
        _capped(blocks, cap)
        if cap is None:
            assert blocks == (2 * n + 255) // 256


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("cap", [None, 1, 2])
@pytest.mark.parametrize("fam", COMBINE_FAMILIES, ids=[f[0] for f in COMBINE_FAMILIES])
def test_combine_families_head_tail_and_stride(mvx, launch, fam, cap, nt):
    _, k, shape, folded, kmax, u0, u1, prog = fam
    launch(cap, 4 if nt else -1)
    want = "k_combine<2, float, %d, %d, %d, %d>" % (kmax, u1 if nt else u0, nt, prog)
    # (one float from each of two operands is 12 bytes of traffic, under the
    # 16-byte threshold: the one launch here that stays cached)
    small = "k_combine<2, float, %d, %d, 0, %d>" % (kmax, u0, prog)
    u = u1 if nt else u0
    for nvec in COMBINE_NVEC:
        n = 3 + 4 * nvec + 2
        sym, blocks = SL.plan_combine(mvx, 102, 10, k, shape, n, offset=4, folded=folded, seed=nvec % 7)
        assert sym == want, (sym, want, nvec)
        _capped(blocks, cap)
        if cap is None:
            assert blocks == max(1, (nvec + 256 * u - 1) // (256 * u))
    for n in MISALIGNED_N:
        sym, blocks = SL.plan_combine(mvx, 102, 10, k, shape, n, folded=folded, seed=n % 5, misalign=True)
        assert sym == (small if (k + 1) * n * 4 < 16 else want), (sym, want, n)
        _capped(blocks, cap)


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("cap", [None, 1, 2])
def test_apply_in_place_head_tail_and_stride(mvx, launch, cap, nt):
    launch(cap, 4 if nt else -1)
    want = "k_combine<2, float, 2, 4, %d, 0>" % nt
    for nvec in COMBINE_NVEC:
        sym, blocks = SL.plan_apply(mvx, None, 102, 10, 3 + 4 * nvec + 2, offset=4, seed=nvec % 7)
        assert sym == want, sym
        _capped(blocks, cap)
    for n in MISALIGNED_N:
        sym, blocks = SL.plan_apply(mvx, None, 102, 10, n, seed=n % 5, misalign=True)
        assert sym == (want if 3 * n * 4 >= 16 else "k_combine<2, float, 2, 4, 0, 0>"), sym    # 12 bytes: cached
        _capped(blocks, cap)


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("cap", [None, 1, 2])
@pytest.mark.parametrize("k", [4, 8])
def test_long_double_sum_trees_small(mvx, launch, k, cap, nt):
    launch(cap, 4 if nt else -1)
    for nvec in (1, 255, 256, 257, 1025, 4099):
        for off in (0, 8):
            if off and nvec > 257:
                continue
            sym, blocks = SL.plan_combine(mvx, 102, 12, k, SHAPE_TREE, nvec, offset=off, seed=k + nvec % 3)
            assert sym.startswith("k_combine<2, ") and sym.endswith(", %d, 1, %d, 1>" % (k, nt)), sym
            _capped(blocks, cap)
            if cap is None:
                assert blocks == (nvec + 255) // 256


# ------------------------- the default policy at the benchmark's sizes

def _find(doc, key):
    """Every value stored under `key` anywhere in a JSON document."""
    if isinstance(doc, dict):
        return [v for k, v in doc.items() if k == key] + [x for v in doc.values() for x in _find(v, key)]
    if isinstance(doc, list):
        return [x for v in doc for x in _find(v, key)]
    return []


def test_default_plan_of_the_benchmark_launch(mvx, launch):
    """C2: MPI_SUM on MPI_FLOAT, the plain op on 64 Mi elements -- the tag and
    the symbol are the ones BENCH_r06.json records."""
    launch(None, SL.DEFAULT_NT_LOG2)
    n = 64 << 20
    inout, in_ = SL._fake(2, 0), SL._fake(1, 0)
    rc, p = mvx.op_plan(SUM, FLOAT, [inout, in_], inout, n, 1, 0)
    assert rc == 0
    assert (p.tag.decode(), p.symbol.decode(), p.blocks, p.dynamic_lds) == \
        ("sum_f32_k2_nt", "k_combine<2, float, 2, 4, 1, 0>", 16384, 0)
    bench = json.load(open(os.path.join(ROOT, "BENCH_r06.json")))
    assert _find(bench, "kernel") == [p.tag.decode()]
    assert _find(bench, "kernel_symbol") == [p.symbol.decode()]


def test_default_plan_of_large_trees_and_chains(mvx, launch):
    """Body kernels for aligned, unfolded, whole-chunk trees and chains from
    64 MiB of traffic; k_combine for everything else (tests/test_gpu_body.py
    asserts the same on launches)."""
    launch(None, SL.DEFAULT_NT_LOG2)
    n = 8 << 20                                             # 32 MiB of f32 per leaf
    assert SL.plan_combine(mvx, SUM, FLOAT, 8, SHAPE_TREE, n) == ("k_tree_body<2, float, 8, 2>", n // 4 // 512)
    sym, blocks = SL.plan_combine(mvx, SUM, FLOAT, 4, SHAPE_CHAIN, n)
    assert (sym, blocks) == ("k_chain_body<2, float, 4, 2>", n // 4 // 512)
    for kw in (dict(n=n + 1), dict(n=n, offset=4), dict(n=n, folded=True), dict(n=4096)):
        sym, _ = SL.plan_combine(mvx, SUM, FLOAT, 8, SHAPE_TREE, **kw)
        assert sym.startswith("k_combine<2, float, 8, "), (sym, kw)


def test_plan_of_nothing_and_argument_checks(mvx):
    """n == 0 is success with nothing to launch; the checks and codes are
    mvx_op_program's; the last-launch record is not touched."""
    before = (mvx.last_kernel(), mvx.last_kernel_symbol(), mvx.last_launch()[:2])
    a, b = SL._fake(1, 0), SL._fake(2, 0)
    rc, p = mvx.op_plan(SUM, FLOAT, [a, b], a, 0, 1, 0)
    assert (rc, p.symbol, p.blocks) == (0, b"", 0)
    assert mvx.op_plan(SUM, FLOAT, [a, b], a, 5, 0, 0)[0] == mvx.MPI_ERR_ARG      # two leaves, no step
    assert mvx.op_plan(SUM, FLOAT, [a, b], a, 5, 2, 0)[0] == mvx.MPI_ERR_ARG      # a step past leaf 1
    assert mvx.op_plan(99, FLOAT, [a, b], a, 5, 1, 0)[0] == mvx.MPI_ERR_OP
    assert mvx.op_plan(105, FLOAT, [a, b], a, 5, 1, 0)[0] == 329                  # BAND on a float
    assert mvx.op_plan(SUM, FLOAT, [a, b], a, 5, 1, 0)[0] == 0
    assert (mvx.last_kernel(), mvx.last_kernel_symbol(), mvx.last_launch()[:2]) == before


# ------------------------------------ the alignment rule, through the plan

# a type of every element size: (op, dtype, bytes)
SIZES = [(SUM, 1, 1), (SUM, 4, 2), (SUM, 6, 4), (SUM, 8, 8), (SUM, 12, 16), (MAXLOC, 22, 32)]


@pytest.mark.parametrize("op,dtype,E", SIZES, ids=["%dB" % s[2] for s in SIZES])
def test_split_for_every_element_size_and_residue(mvx, launch, op, dtype, E):
    """The plain op, cached build (U = 4, never a body kernel), every residue
    m of the destination mod 16.  All operands on m: a head of ((16 - m) & 15)
    / E elements when that is a whole number, then whole chunks, a block per
    1024 of them -- n is 2049 chunks' worth, so any head takes the grid from
    3 blocks to 2.  One operand elsewhere, or no whole number of elements up
    to the boundary: a block per 256 elements."""
    launch(None, -1)
    assert mvx.dtype_info(dtype)[0] == E
    chunk = max(16, E)
    n = 2049 * chunk // E
    for m in range(16):
        pre = (16 - m) & 15
        if pre % E == 0:
            head = min(pre // E, n)
            want = max(1, -(-((n - head) * E // chunk) // 1024))
        else:
            want = -(-n // 256)
        inout, in_ = SL._fake(2, m), SL._fake(1, m)
        rc, p = mvx.op_plan(op, dtype, [inout, in_], inout, n, 1, 0)
        assert (rc, p.blocks) == (0, want), (m, p.blocks, want)
        assert want == (3 if m == 0 else 2 if pre % E == 0 else -(-n // 256))
        other = SL._fake(1, (m + (E if E < 16 else 8)) % 16)
        rc, p = mvx.op_plan(op, dtype, [inout, other], inout, n, 1, 0)
        assert (rc, p.blocks) == (0, -(-n // 256)), (m, p.blocks)


# ------------------------------------------------- the op-side knob groups

@pytest.mark.parametrize("group", knob_worker.PLAN_GROUPS)
def test_knob_group_planned(group):
    """Knobs are read once per process: a fresh one per group, with the
    group's variables set, runs the group's checks on plans."""
    env = dict(os.environ)
    env.update(knob_worker.ENV[group])
    r = subprocess.run([sys.executable, WORKER, group, "--plan"], env=env, timeout=knob_worker.TIMEOUT[group],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    tail = r.stdout[-3000:]
    assert r.returncode == 0, "group %s failed (exit status %d):\n%s" % (group, r.returncode, tail)
    lines = r.stdout.strip().splitlines()
    last = lines[-1].split() if lines else []
    assert len(last) == 4 and last[:2] == ["knobs", "ok"] and last[3] == "checks" and int(last[2]) > 0, tail
    assert int(last[2]) == sum(ln.startswith("ok ") for ln in lines), tail
