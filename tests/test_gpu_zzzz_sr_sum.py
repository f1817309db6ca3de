"""GPU: the stochastically rounded f32 sum (MVX_SR_SUM = 170, mvx_op_create_sr_sum) through the
kernels and the collectives, bit for bit against sr_ref (the definition in numpy) applied to the
exact sum.  Leaves are small multiples of a power of two, so every f32 partial sum is exact and the
value narrowed does not depend on the association.  The file's name makes it the last one collected."""
import itertools

import numpy as np
import pytest

import acc32_ref as A
import mvxtest as T
import plan_exec as PX
import small_launch as SL
import sr_ref as R

pytestmark = pytest.mark.gpu

SR, F32_IN, SEEDS, FIRSTS = 170, 2, (0x0123456789abcdef, 2 ** 64 - 1), (0, 1, 3, 2 ** 32 - 5)
TM, CM, f32 = PX.tree_mask, PX.chain_mask, np.float32
TYPES = pytest.mark.parametrize("t", A.TYPES, ids=lambda t: A.NAMES[t])


def leaves(t, k, n, seed, special=True):
    """k float32 arrays of values of type t: leaf 0 on the grid, leaf 1 eighths of its gap q, the rest
    whole gaps.  special: elements 0..7 sum just above the largest finite value (either sign), to +0,
    -0, inf, NaN, into the subnormal range and to the largest finite value itself."""
    m, emin, _, top = R.FMT[t]
    rng = np.random.default_rng(seed)
    sign, q = rng.choice([-1.0, 1.0], n), np.ldexp(1.0, rng.integers(emin + 3, emin + 9, n) - m)
    L = [sign * (2 ** m + rng.integers(0, 2 ** m, n)) * q, sign * rng.integers(0, 8, n) * q / 8]
    L += [rng.integers(-1, 2, n) * q for _ in range(k - 2)]
    qt, sub = 2.0 ** (np.frexp(top)[1] - 1 - m), 2.0 ** (emin - m)
    for i, (a, b) in enumerate([(top, 3 * qt / 8), (-top, -5 * qt / 8), (0.0, 0.0), (-0.0, -0.0), (np.inf, 1.0),
                                (np.nan, 1.0), (3 * sub, sub), (top, 0.0)][:n if special else 0]):
        for x in L[2:]:
            x[i] = a if a == 0 else 0.0          # (every leaf -0: the sum is -0)
        L[0][i], L[1][i] = a, b
    return [x.astype(f32) for x in L]


def exact_sum(L):
    with np.errstate(all="ignore"):
        s = L[0].astype(np.float64)
        for x in L[1:]:
            s = s + x
        assert np.array_equal(s.astype(f32).astype(np.float64), s, equal_nan=True)
        return s.astype(f32)


def run(mvx, t, L, F, tm, cm, n, first, seed, off=0, dst_off=None, side=0):
    """One launch over leaves L (f32 arrays: narrowed to t, or given as floats under F32_IN), operands
    `off` elements off the 16-byte grid.  Returns (result bytes, kernel symbol)."""
    import torch
    e, es = A.ESIZE[t], 4 if side else A.ESIZE[t]
    enc = (lambda x: x.view(np.uint8)) if side else (lambda x: A.round_to(t, x))
    dS = [SL._place(enc(x), off * es, q)[1] for q, x in enumerate(L)]
    dF = [SL._place(enc(x), off * es, 20 + q)[1] if x is not None else None for q, x in enumerate(F)] if F else None
    do = (off if dst_off is None else dst_off) * e
    buf, dst, host = SL._place(np.zeros(n * e, np.uint8), do, 40)
    assert mvx.op_program_sr(t, dS, dst, n, tm, cm, seed, first, side=side, folds=dF) == 0
    torch.cuda.synchronize()
    got, lo = T.from_dev(buf), SL.GUARD + do
    assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + n * e:], host[lo + n * e:])
    return got[lo:lo + n * e], mvx.last_kernel_symbol()


# name: (k, tree_mask, chain_mask, folded leaves, side)
SHAPES = {"k2": (2, 1, 0, (), 0), "tree8": (8, TM(8), 0, (), 0), "chain5-fold": (5, 0, CM(5), (1, 4), 0),
          "f32in": (2, 1, 0, (), F32_IN)}


@pytest.mark.parametrize("shape", list(SHAPES))
@TYPES
def test_bits(mvx, t, shape):
    """Every n against the definition: all operands aligned, shifted by 1 and by 3 elements (a head
    before the chunks) and the destination alone shifted (the element path), every first index, both
    seeds -- all of them at 4099, three at each smaller size.  Under F32_IN the leaves are two halves
    of arbitrary f32 values, the type's subnormal range included."""
    k, tm, cm, fq, side = SHAPES[shape]
    m, emin, _, top = R.FMT[t]
    combos = list(itertools.product(((0, None), (1, None), (3, None), (0, 1)), FIRSTS, SEEDS))
    for a, n in enumerate((1, 3, 63, 64, 257, 4099)):
        L = leaves(t, k + len(fq), n, 7 * n + k)
        if side:
            rng = np.random.default_rng(n)
            v = (rng.choice([-1, 1], n) * (1 + rng.random(n)) * 2.0 ** rng.uniform(max(emin - m - 10, -126), np.log2(top) - 1, n))
            v = np.concatenate([exact_sum(L)[:8], v.astype(f32)])[:n]
            hi = (v.view(np.uint32) & 0xfffff000).view(f32)
            with np.errstate(invalid="ignore"):
                L = [hi, np.where(np.isfinite(v), v - hi, 0).astype(f32)]
        F = [L[k + fq.index(q)] if q in fq else None for q in range(k)]
        v = exact_sum(L)
        for (off, dst_off), first, seed in combos if n == 4099 else combos[a::8]:
            got, sym = run(mvx, t, L[:k], F, tm, cm, n, first, seed, off, dst_off, side)
            assert ("k_combine_f32<16, " if side else "k_combine<16, ") in sym, sym
            A.assert_same(A.SUM, t, got, R.sr_round(t, v, first, seed), (sym, n, off, dst_off, first, hex(seed)))


@TYPES
def test_same_bits_whatever_the_launch(mvx, t):
    """4099 elements of an 8-leaf tree: one launch, two launches cut at element 1001, one block, the
    non-temporal build; then whole chunks through k_tree_body and k_chain_body.  All the definition's."""
    n, first, seed = 4099, 2 ** 32 - 5, SEEDS[0]
    L = leaves(t, 8, n, 5)
    ref = R.sr_round(t, exact_sum(L), first, seed)
    try:
        for cap, nt in ((SL.DEFAULT_CAP, -1), (1, -1), (SL.DEFAULT_CAP, 4)):
            mvx.set_launch(cap, nt)
            got, sym = run(mvx, t, L, None, TM(8), 0, n, first, seed)
            A.assert_same(A.SUM, t, got, ref, (sym, cap, nt))
            parts = [run(mvx, t, [x[a:b] for x in L], None, TM(8), 0, b - a, first + a, seed)[0] for a, b in ((0, 1001), (1001, n))]
            assert np.array_equal(np.concatenate(parts), got), (cap, nt)
        n = 513 * 16 // A.ESIZE[t]
        L = leaves(t, 8, n, 6)
        for (tm, cm, base), first in itertools.product(((TM(8), 0, "k_tree_body<16, "), (0, CM(8), "k_chain_body<16, ")), (0, 3)):
            got, sym = run(mvx, t, L, None, tm, cm, n, first, seed)
            assert sym.startswith(base), sym
            A.assert_same(A.SUM, t, got, R.sr_round(t, exact_sum(L), first, seed), (sym, first))
    finally:
        mvx.set_launch(SL.DEFAULT_CAP, SL.DEFAULT_NT_LOG2)


@TYPES
def test_unbiased_and_exact_on_the_grid(mvx, t):
    """65536 sums at f = 0.3 and f = 1/256 of the gap above 1.0: the share rounded up is within 5
    standard deviations of floor(f * 2^nb) / 2^nb (0.009 at f = 0.3); sums on the grid stay."""
    m, _, nb, _ = R.FMT[t]
    n, q = 65536, 2.0 ** -m
    for f in (0.3, 1 / 256):
        v = np.full(n, 1 + f * q, f32)
        p = np.floor((float(v[0]) - 1) / q * 2 ** nb) / 2 ** nb
        w = A.widen(t, run(mvx, t, [np.ones(n, f32), v - 1], None, 1, 0, n, 0, SEEDS[0], side=F32_IN)[0])
        assert np.isin(w, (1, 1 + q)).all() and abs((w > 1).mean() - p) <= 5 * np.sqrt(p * (1 - p) / n), (f, (w > 1).mean(), p)
    L = leaves(t, 2, n, 3)[:1] + [np.zeros(n, f32)]
    got, sym = run(mvx, t, L, None, 1, 0, n, 1, SEEDS[1])
    A.assert_same(A.SUM, t, got, A.round_to(t, exact_sum(L)), sym)


@TYPES
def test_collectives(mvx, t):
    """Allreduce, Reduce_scatter and Scan at p = 3 and 8, Allreduce at p = 17 (more than 8 leaves):
    every rank holds the definition's bits of the exact sum, indexed by the reduced vector.  At p = 3
    also from pinned host buffers and under the pipelined exchange; a freed handle is MPI_ERR_OP."""
    import torch
    e, seed = A.ESIZE[t], SEEDS[0]
    rc, op = mvx.op_create_sr_sum(seed)
    assert rc == 0
    for p in (3, 8, 17):
        comm = mvx.Comm.local_ranks(p, 0)
        try:
            for n, pin, pipe in ((5, 0, 0), (8193, 0, 0)) + (((8193, 1, 0), (8193, 0, 1)) if p == 3 else ()):
                S = leaves(t, p, n, p + n, special=False)      # finite values: every partial sum exact
                cnts = [n // p + (1 if r < n % p else 0) for r in range(p)]
                disp = np.concatenate([[0], np.cumsum(cnts)]) * e
                place = (lambda a: torch.from_numpy(a).pin_memory()) if pin else T.to_dev
                dS = [place(A.round_to(t, x)) for x in S]
                assert comm.set_exchange(mvx.EXCH_PIPE if pipe else mvx.EXCH_P2P, 3) == 0
                full = R.sr_round(t, exact_sum(S), 0, seed)
                for coll in ("ar", "rs", "scan") if p < 17 else ("ar",):
                    dR = [place(np.full((max(c, 1) if coll == "rs" else n) * e, 0x5C, np.uint8)) for c in cnts]
                    r0, rcs = {"ar": lambda: comm.allreduce_multi(dS, dR, n, t, op),
                               "rs": lambda: comm.reduce_scatter_multi(dS, dR, cnts, t, op),
                               "scan": lambda: comm.scan_multi(dS, dR, n, t, op)}[coll]()
                    assert r0 == 0 and rcs == [0] * p, (coll, p, n, r0, rcs)
                    assert not pipe or coll == "scan" or comm.last_exchange() == mvx.EXCH_PIPE
                    torch.cuda.synchronize()
                    for r in range(p):
                        want = {"ar": full, "rs": full[disp[r]:disp[r + 1]],
                                "scan": R.sr_round(t, exact_sum(S[:r + 1]), 0, seed)}[coll]
                        A.assert_same(A.SUM, t, dR[r].cpu().numpy()[:want.size], want, (coll, p, n, pin, pipe, r))
            assert mvx.MPI_Op_free(op) == (0, 0)
            assert comm.allreduce_multi(dS, dR, n, t, op) == (0, [9] * p)          # freed
            assert comm.allreduce_multi(dS, dR, n, t, SR) == (0, [9] * p)          # 170 is no MPI-level op
            rc, op = mvx.op_create_sr_sum(seed)
            assert rc == 0
        finally:
            comm.free()
    assert mvx.MPI_Op_free(op) == (0, 0)
