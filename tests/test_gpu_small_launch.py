"""GPU: every op kernel family at small, ragged sizes (mvx.set_launch).

The default launch policy gives a body kernel only exact multiples of a
block's work and every kernel one block per unit of work, so the `c <
P.nvec` guards, the last partial block and the second trip of every
grid-stride loop run nowhere else in the suite.  Here set_launch(cap, 4)
makes every launch non-temporal (body dispatch at a few chunks) and caps the
grid at 1 to 3 blocks; set_launch(cap, -1) forces the cached builds.  Sizes
are counts of 16-byte chunks (32-byte elements for MPI_LONG_DOUBLE_INT); no
buffer exceeds about 1 MiB.  Every launch is compared with the CPU oracle,
its kernel symbol asserted, and the 256-byte guard bands around the
destination checked (tests/small_launch.py).
"""
import numpy as np
import pytest

import mvxtest as T
import small_launch as SL
from small_launch import (BODY_NVEC, BODY_PAIRS, COMBINE_FAMILIES, COMBINE_NVEC, MISALIGNED_N, PXI_NVEC, SHAPE_CHAIN,
                          SHAPE_TREE)

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("cap", [None, 1, 3])
@pytest.mark.parametrize("op,dtype", BODY_PAIRS)
def test_body_kernels_ragged_sizes_and_grid_stride(mvx, launch, op, dtype, cap):
    """k_tree_body (k = 4, 8) and k_chain_body (k = 4 .. 8; 5 to 7 on the
    8-leaf kernel's run-time leaf count) at sizes around one and two blocks'
    work: 1025 chunks at cap 1 is three trips of a U = 2 block, the last
    holding one chunk; 3372 at cap 3 two full rounds and a ragged third."""
    launch(cap, 4)
    E = mvx.dtype_info(dtype)[0]
    for nvec in BODY_NVEC:
        n = nvec * 16 // E
        for shape, ks in ((SHAPE_TREE, (4, 8)), (SHAPE_CHAIN, (4, 5, 6, 7, 8))):
            for k in ks:
                sym, blocks = SL.combine(mvx, op, dtype, k, shape, n, seed=k)
                pre, suf = SL.body_symbol(op, k, shape)
                assert sym.startswith(pre) and sym.endswith(suf), (sym, nvec, k, shape)
                _capped(blocks, cap)
                if cap is None:
                    assert blocks == (nvec + 511) // 512


@pytest.mark.parametrize("cap", [None, 1, 3])
@pytest.mark.parametrize("op", [110, 111])
def test_long_double_int_pair_body_ragged(mvx, oracle, launch, op, cap):
    """k_pxi_loc_body<O, 4 | 8, 1> (trees) and <O, 2, 1> (the plain op) on
    MPI_LONG_DOUBLE_INT, 30 % tied values: sizes that are no multiple of a
    block's 128 elements leave lanes past the end running the DPP step on
    unloaded registers, next to lane pairs that store."""
    launch(cap, 4)
    for n in PXI_NVEC:
        for k in (4, 8):
            sym, blocks = SL.combine(mvx, op, 22, k, SHAPE_TREE, n, seed=k, ties=0.3)
            assert sym == "k_pxi_loc_body<%d, %d, 1>" % (op - 100, k), sym
            _capped(blocks, cap)
        sym, blocks = SL.apply(mvx, oracle, op, 22, n, seed=n, ties=0.3)
        assert sym == "k_pxi_loc_body<%d, 2, 1>" % (op - 100), sym
        _capped(blocks, cap)
        if cap is None:
            assert blocks == (2 * n + 255) // 256


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("cap", [None, 1, 2])
@pytest.mark.parametrize("fam", COMBINE_FAMILIES, ids=[f[0] for f in COMBINE_FAMILIES])
def test_combine_families_head_tail_and_stride(mvx, launch, fam, cap, nt):
    """k_combine, cached and non-temporal builds: the MPI_FLOAT operands sit 4
    bytes off the 16-byte grid (a head of 3 elements, so no body kernel), n =
    3 + 4 nvec + 2 -- the head / tail loop, the vector loop's second chunk
    guard and, under a cap, its further trips; then operands misaligned
    against each other (vec_ok = 0), where the scalar loop strides."""
    _, k, shape, folded, kmax, u0, u1, prog = fam
    launch(cap, 4 if nt else -1)
    want = "k_combine<2, float, %d, %d, %d, %d>" % (kmax, u1 if nt else u0, nt, prog)
    # (one float from each of two operands is 12 bytes of traffic, under the
    # 16-byte threshold: the one launch here that stays cached)
    small = "k_combine<2, float, %d, %d, 0, %d>" % (kmax, u0, prog)
    u = u1 if nt else u0
    for nvec in COMBINE_NVEC:
        n = 3 + 4 * nvec + 2
        sym, blocks = SL.combine(mvx, 102, 10, k, shape, n, offset=4, folded=folded, seed=nvec % 7)
        assert sym == want, (sym, want, nvec)
        _capped(blocks, cap)
        if cap is None:
            assert blocks == max(1, (nvec + 256 * u - 1) // (256 * u))
    for n in MISALIGNED_N:
        sym, blocks = SL.combine(mvx, 102, 10, k, shape, n, folded=folded, seed=n % 5, misalign=True)
        assert sym == (small if (k + 1) * n * 4 < 16 else want), (sym, want, n)
        _capped(blocks, cap)


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("cap", [None, 1, 2])
def test_apply_in_place_head_tail_and_stride(mvx, oracle, launch, cap, nt):
    """mvx_op_apply itself (dst aliases the first operand), U = 4, at the
    same sizes."""
    launch(cap, 4 if nt else -1)
    want = "k_combine<2, float, 2, 4, %d, 0>" % nt
    for nvec in COMBINE_NVEC:
        sym, blocks = SL.apply(mvx, oracle, 102, 10, 3 + 4 * nvec + 2, offset=4, seed=nvec % 7)
        assert sym == want, sym
        _capped(blocks, cap)
    for n in MISALIGNED_N:
        sym, blocks = SL.apply(mvx, oracle, 102, 10, n, seed=n % 5, misalign=True)
        assert sym == (want if 3 * n * 4 >= 16 else "k_combine<2, float, 2, 4, 0, 0>"), sym    # 12 bytes: cached
        _capped(blocks, cap)


@pytest.mark.parametrize("nt", [1, 0])
@pytest.mark.parametrize("cap", [None, 1, 2])
@pytest.mark.parametrize("k", [4, 8])
def test_long_double_sum_trees_small(mvx, launch, k, cap, nt):
    """MPI_LONG_DOUBLE SUM trees (x87 emulation: alu-heavy, no body kernel,
    U = 1 in both builds) keep k_combine's fixed tree at every size, aligned
    or 8 bytes off the grid (16-byte elements: no whole element on it)."""
    launch(cap, 4 if nt else -1)
    for nvec in (1, 255, 256, 257, 1025, 4099):
        for off in (0, 8):
            if off and nvec > 257:
                continue
            sym, blocks = SL.combine(mvx, 102, 12, k, SHAPE_TREE, nvec, offset=off, seed=k + nvec % 3)
            assert sym.startswith("k_combine<2, ") and sym.endswith(", %d, 1, %d, 1>" % (k, nt)), sym
            _capped(blocks, cap)
            if cap is None:
                assert blocks == (nvec + 255) // 256


# ------------------------------------------------------ exhaustive byte table

def _byte_cases():
    return [(op, dt) for dt, ops in SL.BYTE_OPS.items() for op in ops]


@pytest.mark.parametrize("op,dtype", _byte_cases())
def test_byte_table_exhaustive(mvx, oracle, launch, op, dtype):
    """All 65,536 (a, b) byte pairs of every 1-byte op -- the SWAR borrow
    trick of SUM, the biased signed MAX / MIN, the packed-16 PROD, swar_nz --
    through the plain op, the 8-leaf tree body and the 4-leaf chain body
    (CF8 inside k_tree_body / k_chain_body), against the plain numpy table
    (small_launch.byte_table; test_cpu_byte_table.py ties the oracle to it)."""
    import torch
    a, b = SL.byte_pairs()
    want = SL.byte_table(op, dtype)
    n = a.size
    launch(None, 4)

    def guarded(x, seed):
        host = np.random.default_rng(seed).integers(0, 256, n + 2 * SL.GUARD, dtype=np.uint8)
        host[SL.GUARD:SL.GUARD + n] = x
        return torch.from_numpy(host.copy()).cuda(), host

    def check(buf, host, what):
        got = T.from_dev(buf)
        bad = np.flatnonzero(got[SL.GUARD:SL.GUARD + n] != want)
        assert bad.size == 0, (what, bad.size, [(int(a[i]), int(b[i]), int(got[SL.GUARD + i]), int(want[i]))
                                                for i in bad[:4]])
        host[SL.GUARD:SL.GUARD + n] = want
        assert np.array_equal(got, host), (what, "guard bands")

    # the plain op, each operand in either role (inout = in op inout)
    for x, y in ((a, b), (b, a)):
        buf, host = guarded(y, 1)
        dx = torch.from_numpy(x.copy()).cuda()
        assert mvx.op_apply(op, dtype, dx, buf[SL.GUARD:SL.GUARD + n], n) == 0
        torch.cuda.synchronize()
        sym = mvx.last_kernel_symbol()
        assert sym.startswith("k_combine<%d, " % (op - 100)) and sym.endswith(", 2, 4, 1, 0>"), sym
        check(buf, host, sym)
    fill = SL.byte_filler(op)
    rest = b if fill is None else np.full(n, fill, np.uint8)
    for k, shape in ((8, SHAPE_TREE), (4, SHAPE_CHAIN)):
        srcs = [torch.from_numpy(x.copy()).cuda() for x in [a, b] + [rest] * (k - 2)]
        buf, host = guarded(np.zeros(n, np.uint8), 2)
        assert mvx.op_combine(op, dtype, srcs, buf[SL.GUARD:SL.GUARD + n], n, shape=shape) == 0
        torch.cuda.synchronize()
        sym = mvx.last_kernel_symbol()
        pre, suf = SL.body_symbol(op, k, shape)
        assert sym.startswith(pre) and sym.endswith(suf), sym
        check(buf, host, sym)
