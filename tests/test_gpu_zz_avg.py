"""GPU: MVX_AVG (168), the ranks' mean, through the kernels and the collectives.

float / double: the oracle's MPI_SUM program on the same leaves, divided in
numpy in the same dtype; bit for bit, NaN for NaN.  The narrow floats: inputs
whose float32 sum is exact whatever the association (small integers times a
power of two; 8-bit values that are multiples of 2^-9 up to 448 -- every
finite E4M3 byte, and the E5M2 bytes of that range), so the expected byte is
round_once(float32(exact sum) / float32(count)); bit for bit.

The file's name makes it the last one collected: no existing test changes place.
"""
import functools

import numpy as np
import pytest

import acc32_ref as A
import fp8_ref
import mvxtest as T
import plan_exec as PX
import small_launch as SL

pytestmark = pytest.mark.gpu

AVG, SUM, SUM_ACC32 = 168, 102, 164
MPI_INT, MPI_FLOAT, MPI_DOUBLE, E4M3 = 6, 10, 11, 72
ESIZE = {10: 4, 11: 8, **A.ESIZE}
NAMES = {10: "f32", 11: "f64", **A.NAMES}
TYPES = [10, 11] + list(A.TYPES)
TM = PX.tree_mask
# name: (k, tree_mask, chain_mask, the folded leaf)
SHAPES = {"apply": (2, 1, 0, None), "tree3-fold": (3, TM(3), 0, 1), "tree8": (8, TM(8), 0, None),
          "chain6": (6, 0, PX.chain_mask(6), None), "tree4-chain": (5, TM(4), 1 << 4, None)}


def _leaf(dtype, n, seed):
    """(bytes, exact float64 values or None)."""
    rng = np.random.default_rng(seed)
    if dtype in (MPI_FLOAT, MPI_DOUBLE):
        return np.ascontiguousarray(T.rand_vec(dtype, n, seed)).view(np.uint8), None
    if dtype in fp8_ref.TYPES:
        u = rng.integers(0, 256, n).astype(np.uint8)
        if dtype == E4M3:
            u[(u & 0x7f) == 0x7f] = 0x7e                    # NaN -> 448
        else:
            u = (u & 0x83) | (rng.integers(8, 24, n).astype(np.uint8) << 2)      # 2^-7 .. 448
        return u, fp8_ref.widen(dtype, u)
    v = (rng.integers(-8, 9, n) * 0.125).astype(np.float32)
    return A.round_to(dtype, v), v.astype(np.float64)


def _mean(dtype, leaves, folds, tm, cm, n, divisor):
    """The reference: leaves / folds as _leaf() gives them."""
    if dtype in (MPI_FLOAT, MPI_DOUBLE):
        s = PX.run_program(SUM, dtype, [x for x, _ in leaves], [f[0] if f else None for f in folds], tm, cm, n)
        npt = np.float32 if dtype == MPI_FLOAT else np.float64
        with np.errstate(all="ignore"):
            return (s.view(npt) / npt(divisor)).view(np.uint8)
    exact = functools.reduce(np.add, [v for _, v in leaves] + [f[1] for f in folds if f])   # an all -0 sum stays -0
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
    return A.round_to(dtype, exact.astype(np.float32) / np.float32(divisor))


def _same(dtype, got, ref, what):
    if dtype in (MPI_FLOAT, MPI_DOUBLE):
        T.assert_same(SUM, dtype, got, ref.view(np.float32 if dtype == MPI_FLOAT else np.float64))
    else:
        assert np.array_equal(got, ref), (what, np.flatnonzero(got != ref)[:5])


@pytest.fixture
def launch(mvx):
    try:
        yield lambda nt: mvx.set_launch(SL.DEFAULT_CAP, 4 if nt else -1)
    finally:
        mvx.set_launch(SL.DEFAULT_CAP, SL.DEFAULT_NT_LOG2)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("dtype", TYPES, ids=[NAMES[d] for d in TYPES])
def test_programs_divide_once_before_the_store(mvx, launch, dtype, shape):
    """n = 1 (scalar only), 17 with every operand one element off the 16-byte
    grid (head, body, tail), 4099 (chunks and a tail), cached and non-temporal;
    513 whole chunks: the body kernels' two blocks, the second ragged."""
    import torch
    e = ESIZE[dtype]
    k, tm, cm, fq = SHAPES[shape]
    divisor = k + (fq is not None)
    for n, off, nt in ((1, 0, 0), (17, e, 0), (4099, 0, 0), (4099, e, 1), (513 * 16 // e, 0, 1)):
        launch(nt)
        leaves = [_leaf(dtype, n, 10 * n + q) for q in range(k)]
        folds = [_leaf(dtype, n, 10 * n + 9) if q == fq else None for q in range(k)]
        ref = _mean(dtype, leaves, folds, tm, cm, n, divisor)
        dS = [SL._place(x, off, q)[1] for q, (x, _) in enumerate(leaves)]
        dF = [SL._place(f[0], off, 20 + q)[1] if f else None for q, f in enumerate(folds)]
        if shape == "apply":      # in place: inout = (in + inout) / 2
            buf, dst, host = SL._place(leaves[0][0], off, 0)
            rc = mvx.op_apply(AVG, dtype, dS[1], dst, n)
        else:
            buf, dst, host = SL._place(np.zeros(n * e, np.uint8), off, 40)
            rc = mvx.op_program(AVG, dtype, dS, dst, n, tm, cm, folds=dF if fq is not None else None)
        torch.cuda.synchronize()
        assert rc == 0, rc
        sym = mvx.last_kernel_symbol()
        assert "<14, " in sym, sym
        if nt and not off and shape in ("tree8", "chain6"):
            assert sym.startswith("k_tree_body" if shape == "tree8" else "k_chain_body"), sym
        got = T.from_dev(buf)
        lo, nb = SL.GUARD + off, n * e
        _same(dtype, got[lo:lo + nb], ref, (sym, n, off, nt))
        assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + nb:], host[lo + nb:]), sym


def _split(n, p):
    return [n // p + (1 if r < n % p else 0) for r in range(p)]


@pytest.mark.parametrize("dtype", [MPI_FLOAT, E4M3], ids=["f32", "e4m3"])
@pytest.mark.parametrize("p", [1, 2, 3, 8, 9, 33])
def test_collectives_divide_by_the_contributions(mvx, p, dtype):
    """Allreduce, Reduce and Reduce_scatter divide by p, Scan's rank r by
    r + 1; p = 9 and 33 combine more than 8 leaves (the last launch divides).
    MPI_FLOAT: MPI_SUM's plans, run with the oracle's op, divided in numpy."""
    import torch
    e = ESIZE[dtype]
    comm = mvx.Comm.local_ranks(p, 0)
    colls = {"ar": mvx.COLL_ALLREDUCE, "red": mvx.COLL_REDUCE, "rs": mvx.COLL_REDUCE_SCATTER, "scan": mvx.COLL_SCAN}
    try:
        for n in (5, 4096):
            cnts, root = _split(n, p), p // 2
            S = [_leaf(dtype, n, 100 * p + r) for r in range(p)]
            dS = [T.to_dev(s) for s, _ in S]
            for coll, cid in colls.items():
                sizes = [max(c, 1) for c in cnts] if coll == "rs" else [n] * p
                dR = [torch.full((s * e,), 0x5C, dtype=torch.uint8, device="cuda") for s in sizes]
                r0, rcs = {"ar": lambda: comm.allreduce_multi(dS, dR, n, dtype, AVG),
                           "red": lambda: comm.reduce_multi(dS, dR, n, dtype, AVG, root),
                           "rs": lambda: comm.reduce_scatter_multi(dS, dR, cnts, dtype, AVG),
                           "scan": lambda: comm.scan_multi(dS, dR, n, dtype, AVG)}[coll]()
                assert r0 == 0 and rcs == [0] * p, (coll, n, r0, rcs)
                if dtype == MPI_FLOAT:
                    plans = [mvx.plan(cid, p, r, 0 if coll == "rs" else n, dtype, SUM, root,
                                      cnts if coll == "rs" else None) for r in range(p)]
                    sums = PX.run_plans(plans, [s for s, _ in S], [np.zeros(s * e, np.uint8) for s in sizes])
                else:
                    prefix = np.cumsum([v for _, v in S], axis=0)
                off = np.cumsum([0] + cnts)
                for r in range(p):
                    if coll == "red" and r != root:
                        continue
                    lo, m = (off[r], cnts[r]) if coll == "rs" else (0, n)
                    d = r + 1 if coll == "scan" else p
                    if dtype == MPI_FLOAT:
                        with np.errstate(all="ignore"):
                            ref = (sums[r][:m * e].view(np.float32) / np.float32(d)).view(np.uint8)
                    else:
                        exact = prefix[r if coll == "scan" else p - 1][lo:lo + m]
                        ref = A.round_to(dtype, exact.astype(np.float32) / np.float32(d))
                    got = T.from_dev(dR[r])
                    _same(dtype, got[:m * e], ref, (coll, p, n, r))
                    assert (got[m * e:] == 0x5C).all(), (coll, p, n, r)
    finally:
        comm.free()


def test_eight_ranks_of_448_in_e4m3(mvx):
    """The sum, per step or in f32, has no E4M3 value: NaN (of either sign --
    the narrowing instruction's is 0xFF); the mean is 448."""
    import torch
    p, n = 8, 64
    comm = mvx.Comm.local_ranks(p, 0)
    try:
        dS = [T.to_dev(np.full(n, 0x7e, np.uint8)) for _ in range(p)]
        for op, want, mask in ((SUM, 0x7f, 0x7f), (SUM_ACC32, 0x7f, 0x7f), (AVG, 0x7e, 0xff)):
            dR = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(p)]
            assert comm.allreduce_multi(dS, dR, n, E4M3, op) == (0, [0] * p)
            for r in range(p):
                assert ((T.from_dev(dR[r]) & mask) == want).all(), (op, r)
    finally:
        comm.free()


def test_return_codes(mvx):
    """An undefined pair inside an Allreduce: 329 on every rank, and what the
    receive buffers then hold is what MPI_BAND on MPI_FLOAT leaves there (the
    transfers of an undefined pair; no arithmetic), the sends untouched.
    mvx_op_program_avg's argument checks."""
    import torch
    p, n = 4, 16
    comm = mvx.Comm.local_ranks(p, 0)
    try:
        S = [np.random.default_rng(r).integers(0, 256, 4 * n).astype(np.uint8) for r in range(p)]
        dS = [T.to_dev(s) for s in S]
        left = {}
        for dtype, op in ((MPI_INT, AVG), (MPI_FLOAT, 105)):
            dR = [torch.full((4 * n,), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(p)]
            assert comm.allreduce_multi(dS, dR, n, dtype, op) == (0, [329] * p)
            left[op] = [T.from_dev(x) for x in dR]
        for r in range(p):
            assert np.array_equal(left[AVG][r], left[105][r]) and np.array_equal(T.from_dev(dS[r]), S[r])
    finally:
        comm.free()
    d = T.to_dev(np.zeros(256, np.uint8))
    a = d.data_ptr()
    assert mvx.op_program_avg(MPI_FLOAT, [a, a + 64], a + 128, 4, 1, 0, 2) == 0
    assert mvx.op_program_avg(MPI_FLOAT, [a, a + 64], a + 128, 4, 1, 0, 0) == 12               # divisor 0
    assert mvx.op_program_avg(E4M3, [a, a + 64], a + 128, 4, 1, 0, 2, side=1) == 12            # F32_OUT: no such side
    assert mvx.op_program_avg(MPI_FLOAT, [a, a + 64], a + 128, 4, 1, 0, 2, side=2) == 12       # no f32 temporaries
    assert mvx.op_program_avg(E4M3, [a, a + 66], a + 128, 4, 1, 0, 2, side=2) == 12            # a misaligned f32 leaf
    assert mvx.op_program_avg(E4M3, [a, a + 64], a + 128, 4, 1, 0, 2, side=2) == 0
    assert mvx.op_program_avg(MPI_INT, [a, a + 64], a + 128, 4, 1, 0, 2) == 329
    torch.cuda.synchronize()
