"""GPU: the per-rank scaled sum with fused amax (MVX_SCALED_SUM = 169,
mvx_op_create_scaled_sum) through the kernels and the collectives.

The reference is numpy float32 over the program in the plan's order: every
leaf widened exactly and multiplied by its scale, float32 adds, one multiply
by out_scale, narrowed once by acc32_ref's roundings; amax is the unsigned
maximum of bits(v) & 0x7fffffff before the narrowing.  Bit for bit, NaN for
NaN.  The file's name makes it the last one collected.
"""
import numpy as np
import pytest

import acc32_ref as A
import mvxtest as T
import plan_exec as PX
import small_launch as SL

pytestmark = pytest.mark.gpu

SCALED, SUM, SUM_ACC32, F32_OUT, F32_IN = 169, 102, 164, 1, 2
MPI_INT, MPI_FLOAT, MPI_REAL, BF16, E4M3 = 6, 10, 26, 65, 72
TYPES = [MPI_FLOAT, MPI_REAL] + list(A.TYPES)
NAMES = {MPI_FLOAT: "f32", MPI_REAL: "real", **A.NAMES}
ESIZE = {MPI_FLOAT: 4, MPI_REAL: 4, **A.ESIZE}
TM, CM = PX.tree_mask, PX.chain_mask
f32 = np.float32


def widen(t, u8):
    return u8.view(f32).copy() if ESIZE[t] == 4 else A.widen(t, u8)


def narrow(t, v):
    return np.ascontiguousarray(v, f32).view(np.uint8) if ESIZE[t] == 4 else A.round_to(t, v)


def leaf(t, n, seed, ints=False):
    """Random finite elements (ints: small integers, exact in every type) as bytes."""
    rng = np.random.default_rng(seed)
    return narrow(t, (rng.integers(-4, 5, n) if ints else 2 * rng.standard_normal(n)).astype(f32))


def scaled(t, leaves, scales, folds=None, fscales=None):
    """The leaves of the f32 program: widened, scaled, folded."""
    with np.errstate(all="ignore"):
        y = [widen(t, x) * f32(s) for x, s in zip(leaves, scales)]
        return [v if folds is None or folds[q] is None else v + widen(t, folds[q]) * f32(fscales[q])
                for q, v in enumerate(y)]


def amax_of(v):
    b = v.view(np.uint32) & 0x7fffffff
    return int(b.max())


def same(t, got, v, what):
    if ESIZE[t] == 4:
        A.assert_same_f32(got, v, what)
    else:
        A.assert_same(A.SUM, t, got, A.round_to(t, v), what)


def check_amax(word, v, what):
    want = amax_of(v)
    assert (word > 0x7f800000) if want > 0x7f800000 else (word == want), (what, hex(word), hex(want))


@pytest.fixture
def launch(mvx):
    try:
        yield lambda nt: mvx.set_launch(SL.DEFAULT_CAP, 4 if nt else -1)
    finally:
        mvx.set_launch(SL.DEFAULT_CAP, SL.DEFAULT_NT_LOG2)


# name: (k, tree_mask, chain_mask, folded leaves)
SHAPES = {"k1": (1, 0, 0, ()), "k1-fold": (1, 0, 0, (0,)), "k2": (2, 1, 0, ()), "tree3-fold": (3, TM(3), 0, (1,)),
          "chain3": (3, 0, CM(3), ()), "tree8": (8, TM(8), 0, ()), "chain8": (8, 0, CM(8), ()),
          "chain8-fold": (8, 0, CM(8), (0, 7))}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("t", TYPES, ids=[NAMES[t] for t in TYPES])
def test_program_scales_sums_rescales_and_takes_amax(mvx, launch, t, shape):
    """n = 1, 17 one element off the 16-byte grid, 4099 aligned and shifted,
    513 whole chunks non-temporal (the body kernels); amax requested or NULL
    (a sentinel word behind it stays); random scales of either sign, then
    powers of two on small integers against the float64 sum."""
    import torch
    e = ESIZE[t]
    k, tm, cm, fq = SHAPES[shape]
    rng = np.random.default_rng(k)
    for n, off, nt, want_amax, exact in ((1, 0, 0, 1, 0), (17, e, 0, 1, 0), (4099, 0, 0, 0, 0), (4099, e, 1, 1, 0),
                                        (513 * 16 // e, 0, 1, 1, 0), (4099, 0, 0, 1, 1)):
        launch(nt)
        ls, fs = ((2.0 ** rng.integers(-2, 3, k) for _ in "lf") if exact else (3 * rng.standard_normal(k) for _ in "lf"))
        ls, fs, osc = [float(f32(x)) for x in ls], [float(f32(x)) for x in fs], 0.25 if exact else -1.7
        L = [leaf(t, n, 10 * n + q, exact) for q in range(k)]
        F = [leaf(t, n, 10 * n + 9 + q, exact) if q in fq else None for q in range(k)]
        with np.errstate(all="ignore"):
            v = A.masked_f32(A.SUM, scaled(t, L, ls, F, fs), tm, cm) * f32(osc)
        if exact:   # every f32 step was exact: the float64 sum, narrowed once
            d = sum(widen(t, x).astype(np.float64) * s for x, s in zip(L, ls))
            d += sum(widen(t, x).astype(np.float64) * s for x, s in zip(F, fs) if x is not None)
            assert np.array_equal(v.astype(np.float64), d * osc)
        dS = [SL._place(x, off, q)[1] for q, x in enumerate(L)]
        dF = [SL._place(x, off, 20 + q)[1] if x is not None else None for q, x in enumerate(F)]
        buf, dst, host = SL._place(np.zeros(n * e, np.uint8), off, 40)
        words = torch.from_numpy(np.array([0, 0x5EED5EED], np.uint32).view(np.int32)).cuda()
        rc = mvx.op_program_scaled(t, dS, dst, n, tm, cm, ls, osc, words if want_amax else None,
                                   folds=dF if fq else None, fold_scale=fs if fq else None)
        torch.cuda.synchronize()
        sym = mvx.last_kernel_symbol()
        assert rc == 0 and "<15, " in sym, (rc, sym)
        if nt and not off and shape in ("tree8", "chain8"):
            assert sym.startswith("k_tree_body" if shape == "tree8" else "k_chain_body"), sym
        got, w = T.from_dev(buf), T.from_dev(words).view(np.uint32)
        lo, nb = SL.GUARD + off, n * e
        same(t, got[lo:lo + nb], v, (sym, n, off, nt))
        assert np.array_equal(got[:lo], host[:lo]) and np.array_equal(got[lo + nb:], host[lo + nb:]), sym
        assert w[1] == 0x5EED5EED and (want_amax or w[0] == 0), (sym, w)
        if want_amax:
            check_amax(int(w[0]), v, (sym, n, off))


@pytest.mark.parametrize("t", [MPI_FLOAT] + list(A.TYPES), ids=lambda t: NAMES[t])
def test_unit_scales_are_the_f32_sum(mvx, t):
    """Op 169 through mvx_op_program: MVX_SUM_ACC32's bits (MPI_SUM's on
    MPI_FLOAT) over every bit pattern, NaN for NaN; a lone leaf is copied,
    NaN payloads and all."""
    import torch
    n, e, twin = 1031, ESIZE[t], SUM if t == MPI_FLOAT else SUM_ACC32
    bits = [np.random.default_rng(q).integers(0, 256, n * e).astype(np.uint8) for q in range(8)]   # every pattern
    dS = [T.to_dev(b) for b in bits]
    for k, tm, cm in ((1, 0, 0), (2, 1, 0), (8, TM(8), 0), (5, 0, CM(5))):
        out = []
        for op in (SCALED, twin):
            d = torch.zeros(n * e, dtype=torch.uint8, device="cuda")
            assert mvx.op_program(op, t, dS[:k], d, n, tm, cm) == 0
            out.append(T.from_dev(d))
        if t == MPI_FLOAT:
            A.assert_same_f32(out[0], out[1].view(f32), k)
        else:
            A.assert_same(A.SUM, t, out[0], out[1], k)
        assert k > 1 or np.array_equal(out[0], bits[0])


def test_eight_full_scale_e4m3_and_the_f32_sides(mvx):
    """Eight 448s at scale 2^-3 are 448 where MVX_SUM_ACC32 is NaN, amax 448.0;
    out_scale 2 overflows to NaN with amax 896.0; a NaN leaf leaves a NaN
    word.  Then a 9-leaf tree as its executor cuts it: MVX_F32_OUT launches
    with the leaves' scales, MVX_F32_IN with out_scale and amax."""
    import torch
    n = 64
    dS = [T.to_dev(np.full(n, 0x7e, np.uint8)) for _ in range(8)]
    nan_leaf = T.to_dev(np.array([0x7e] * (n - 1) + [0x7f], np.uint8))
    for srcs, osc, want, amax in ((dS, 1.0, 0x7e, 448.0), (dS, 2.0, 0x7f, 896.0), (dS[:7] + [nan_leaf], 1.0, None, None)):
        d, w = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        assert mvx.op_program_scaled(E4M3, srcs, d, n, TM(8), 0, [0.125] * 8, osc, w) == 0
        got, word = T.from_dev(d), T.from_dev(w).view(np.uint32)[0]
        if want is None:
            assert word > 0x7f800000 and (got[-1] & 0x7f) == 0x7f and (got[:-1] == 0x7e).all()
        else:
            assert ((got & 0x7f) == want).all() and word == np.array(amax, f32).view(np.uint32), (osc, got[:4], hex(word))
    assert mvx.op_program(SUM_ACC32, E4M3, dS, d, n, TM(8), 0) == 0 and ((T.from_dev(d) & 0x7f) == 0x7f).all()
    for t, n in ((BF16, 1001), (MPI_FLOAT, 1001), (E4M3, 1003)):
        L, ls = [leaf(t, n, 70 + q) for q in range(9)], [float(f32(0.3 * q - 1)) for q in range(9)]
        y = scaled(t, L, ls)
        v = (A.masked_f32(A.SUM, y[:8], TM(8), 0) + y[8]) * f32(3.0)
        dL = [T.to_dev(x) for x in L]
        t0, t1 = (torch.zeros(n, dtype=torch.float32, device="cuda") for _ in "01")
        d, w = torch.zeros(n * ESIZE[t], dtype=torch.uint8, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        assert mvx.op_program_scaled(t, dL[:8], t0, n, TM(8), 0, ls[:8], 9.0, w, side=F32_OUT) == 0
        assert mvx.op_program_scaled(t, dL[8:], t1, n, 0, 0, ls[8:], 9.0, w, side=F32_OUT) == 0
        assert T.from_dev(w)[0] == 0                                  # F32_OUT: neither out_scale nor amax
        assert mvx.op_program_scaled(t, [t0, t1], d, n, 1, 0, [7.0, 7.0], 3.0, w, side=F32_IN) == 0
        same(t, T.from_dev(d), v, t)
        check_amax(int(T.from_dev(w).view(np.uint32)[0]), v, t)


def _expected(mvx, plans, S, scales, osc):
    """Per rank: (the f32 value of its combine, or None; its receive buffer's bytes) by the plans."""
    t, p = plans[0].dtype, len(plans)
    vals, recv = [None] * p, [None] * p
    for r, P in enumerate(plans):
        if not P.has_combine or P.c_cnt == 0:
            continue
        lo, hi = P.c_src_off * P.esize, (P.c_src_off + P.c_cnt) * P.esize
        y = scaled(t, [S[P.leaf[q]][lo:hi] for q in range(P.k)], [scales[P.leaf[q]] for q in range(P.k)],
                   [S[P.leaf_fold[q]][lo:hi] if P.leaf_fold[q] >= 0 else None for q in range(P.k)],
                   [scales[max(P.leaf_fold[q], 0)] for q in range(P.k)])
        with np.errstate(all="ignore"):
            for s, e in P.segments():
                h = 1
                while h < e - s:
                    for q in range(s, e - h, 2 * h):
                        y[q] = y[q] + y[q + h]
                    h *= 2
            for s, _ in P.segments()[1:]:
                y[0] = y[0] + y[s]
            vals[r] = y[0] * f32(osc)
    for r, P in enumerate(plans):
        for d in range(p):   # where rank d's receive buffer takes r's block from: (offset, count)
            if P.b_send[d].cnt:
                recv[d] = (recv[d] or []) + [(P.b_send[d].off, P.b_send[d].cnt, r)]
        if vals[r] is not None and not P.c_dst_tmp:
            recv[r] = (recv[r] or []) + [(P.c_dst_off, P.c_cnt, r)]
    return vals, recv


@pytest.mark.parametrize("t", [E4M3, BF16], ids=["e4m3", "bf16"])
@pytest.mark.parametrize("p", [2, 3, 8, 9, 17])
def test_collectives(mvx, monkeypatch, p, t):
    """All four collectives, counts on both sides of the Allreduce switch,
    distinct scales per rank (Scan's rank r uses ranks 0..r's): every rank's
    bytes, and the amax word (one handle, so one word: the largest of the
    ranks' own blocks).  Under MVX_GRAPH=1 too: no graph is used."""
    import torch
    e, scales, osc = ESIZE[t], [float(f32(0.37 * r - 1.1)) for r in range(p)], 0.75
    w = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc, op = mvx.op_create_scaled_sum(scales, osc, w)
    assert rc == 0
    monkeypatch.setenv("MVX_GRAPH", "1")
    comm = mvx.Comm.local_ranks(p, 0)
    colls = {"ar": mvx.COLL_ALLREDUCE, "red": mvx.COLL_REDUCE, "rs": mvx.COLL_REDUCE_SCATTER, "scan": mvx.COLL_SCAN}
    try:
        for n in (5, 8193):
            cnts, root = [n // p + (1 if r < n % p else 0) for r in range(p)], p // 2
            S = [leaf(t, n, 100 * p + r) for r in range(p)]
            dS = [T.to_dev(s) for s in S]
            for coll, cid in colls.items():
                sizes = [max(c, 1) for c in cnts] if coll == "rs" else [n] * p
                dR = [torch.full((s * e,), 0x5C, dtype=torch.uint8, device="cuda") for s in sizes]
                w.zero_()
                r0, rcs = {"ar": lambda: comm.allreduce_multi(dS, dR, n, t, op),
                           "red": lambda: comm.reduce_multi(dS, dR, n, t, op, root),
                           "rs": lambda: comm.reduce_scatter_multi(dS, dR, cnts, t, op),
                           "scan": lambda: comm.scan_multi(dS, dR, n, t, op)}[coll]()
                assert r0 == 0 and rcs == [0] * p and comm.last_graph()[0] == 0, (coll, n, r0, rcs)
                plans = [mvx.plan(cid, p, r, 0 if coll == "rs" else n, t, op, root, cnts if coll == "rs" else None)
                         for r in range(p)]
                vals, recv = _expected(mvx, plans, S, scales, osc)
                for r in range(p):
                    got, seen = T.from_dev(dR[r]), np.zeros(sizes[r] * e, bool)
                    for off, cnt, src in recv[r] or []:
                        same(t, got[off * e:(off + cnt) * e], vals[src][:cnt], (coll, p, n, r, src))
                        seen[off * e:(off + cnt) * e] = True
                    want = 0 if (coll == "red" and r != root) else (cnts[r] if coll == "rs" else n)
                    assert seen.sum() == want * e and (got[~seen] == 0x5C).all(), (coll, p, n, r)
                check_amax(int(T.from_dev(w).view(np.uint32)[0]), np.concatenate([v for v in vals if v is not None]),
                           (coll, p, n))
        # a communicator of another size: MPI_ERR_ARG on every rank, nothing moves; MPI_INT: 329, MPI_BAND's bytes
        other = mvx.Comm.local_ranks(p + 1, 0)
        try:
            dS1 = dS + [dS[0]]
            dR1 = [torch.full((n * e,), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(p + 1)]
            assert other.allreduce_multi(dS1, dR1, n, t, op) == (0, [12] * (p + 1))
            assert all((T.from_dev(x) == 0x5C).all() for x in dR1) and np.array_equal(T.from_dev(dS[0]), S[0])
        finally:
            other.free()
        left = []
        for dt, o in ((MPI_INT, op), (MPI_FLOAT, 105)):
            dR = [torch.full((64,), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(p)]
            r0, rcs = comm.allreduce_multi(dS, dR, 1, dt, o)
            assert r0 == 0 and 329 in rcs and set(rcs) <= {0, 329}, rcs     # 329 on the ranks that call the op
            left.append([rcs] + [T.from_dev(x) for x in dR])
        assert all(np.array_equal(a, b) for a, b in zip(*left))
        assert comm.allreduce_multi(dS, dR, 1, t, SCALED) == (0, [9] * p)      # 169 is no MPI-level op
    finally:
        comm.free()
        mvx.MPI_Op_free(op)
