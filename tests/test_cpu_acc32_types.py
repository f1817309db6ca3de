"""CPU: the extension ops MVX_SUM_ACC32 (164) and MVX_PROD_ACC32 (165): the
handles and the (op, type) verdicts, the plans (MPI_SUM's / MPI_PROD's but for
the handle), the launch plans, and the test reference tests/acc32_ref.py --
against the oracle's MPI_FLOAT collectives on the widened inputs, against
exact float64 sums, against the per-step references on two operands, and on
hand-made cases where one rounding and a rounding per step differ.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import acc32_ref as A
import fp8_ref
import half_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MPI_FLOAT, MPI_INT = 10, 6
MPI_ERR_OP, NOT_DEFINED = 9, 329
PERM_OP = 844                                   # MVX_ERR_PERM_OP, what MPI_Op_free answers for MPI_SUM
PS = [1, 2, 3, 4, 5, 6, 7, 8, 12, 33, 64]
PS_ORACLE = [1, 2, 3, 4, 5, 6, 7, 8, 12]
TNAME = {64: "_Float16", 65: "bf16", 72: "f8e4m3", 73: "f8e5m2"}


def _colls(mvx):
    return {"ar": mvx.COLL_ALLREDUCE, "red": mvx.COLL_REDUCE, "rs": mvx.COLL_REDUCE_SCATTER, "scan": mvx.COLL_SCAN}


def _cnts(n, p):
    return [n // p + (1 if r < n % p else 0) for r in range(p)]


# ------------------------------------------------------- handles and verdicts

def test_constants_and_headers(mvx):
    assert (mvx.MVX_SUM_ACC32, mvx.MVX_PROD_ACC32) == (164, 165) == A.OPS
    assert mvx.OP_NAMES[164] == "MVX_SUM_ACC32" and mvx.OP_NAMES[165] == "MVX_PROD_ACC32"
    assert mvx.DEFINED_ACC32 == {164: [64, 65, 72, 73], 165: [64, 65, 72, 73]}
    for table in (mvx.DEFINED, mvx.DEFINED_EXT, mvx.DEFINED_EXT8):       # untouched
        assert 164 not in table and 165 not in table
    for header in ("mvx_mpi.h", "mvx_embed.h"):
        text = open(os.path.join(ROOT, "include", header)).read()
        assert re.search(r"#define\s+MVX_SUM_ACC32\s+164\b", text), header
        assert re.search(r"#define\s+MVX_PROD_ACC32\s+165\b", text), header


def _verdict(mvx, op, h):
    return mvx.hip().mvx_op_apply(op, h, None, None, 0, None)


def test_defined_on_the_four_narrow_floats_and_nowhere_else(mvx):
    made = []
    try:
        for op in A.OPS:
            for h in mvx.DEVICE_TYPES:
                want = 0 if h in A.TYPES else NOT_DEFINED
                assert _verdict(mvx, op, h) == want, (op, h)
                assert mvx.hip().mvx_op_supported(op, h) == (1 if h in A.TYPES else 0), (op, h)
            for h in A.TYPES:
                rc, c2 = mvx.MPI_Type_contiguous(2, h)
                assert rc == 0
                made.append(c2)
                e = A.ESIZE[h]
                rc, st = mvx.MPI_Type_struct(2, [1, 1], [0, 4], [h, MPI_INT])
                assert rc == 0
                made.append(st)
                rc, vec = mvx.MPI_Type_vector(3, 1, 2, h)
                assert rc == 0 and mvx.MPI_Type_extent(vec) == (0, 5 * e)
                made.append(vec)
                for d in (c2, st, vec):
                    assert _verdict(mvx, op, d) == NOT_DEFINED and mvx.hip().mvx_op_supported(op, d) == 0, (op, h, d)
    finally:
        for d in made:
            mvx.MPI_Type_free(d)


def test_neighbouring_and_pinned_handles_stay_errors(mvx):
    for op in (99, 112, 163, 166, 77):
        for h in A.TYPES + (MPI_FLOAT,):
            assert _verdict(mvx, op, h) == MPI_ERR_OP, (op, h)
            assert mvx.hip().mvx_op_supported(op, h) == 0


def test_permanent_predefined_and_symmetric(mvx):
    assert mvx.MPI_Op_free(102) == (PERM_OP, 102)
    for op in A.OPS:
        assert mvx.MPI_Op_free(op) == (PERM_OP, op)
        for h in A.TYPES:
            P = mvx.plan(mvx.COLL_ALLREDUCE, 5, 2, 100, h, op)
            assert P.opkind == mvx.OPKIND_PREDEFINED and P.symmetric == 1 and P.op == op
        # undefined pair: the inout operand is kept, so roles matter (as MPI_BAND on MPI_FLOAT)
        assert mvx.plan(mvx.COLL_ALLREDUCE, 5, 2, 100, MPI_FLOAT, op).symmetric == 0


# ---------------------------------------------------------------------- plans

def _counts(e):
    """Elements around the reference's byte thresholds at e bytes each."""
    out = {1, 3, 5, 40, 300}
    for nbytes in (1 << 10, 2 << 10, 4 << 10, 8 << 10, 16 << 10, 32 << 10, 64 << 10, 512 << 10):
        out |= {nbytes // e - 1, nbytes // e, nbytes // e + 1}
    return sorted(out)


def _image(P, op):
    Q = type(P)()
    ctypes.memmove(ctypes.byref(Q), ctypes.byref(P), ctypes.sizeof(P))
    Q.op = op
    return bytes(Q)


@pytest.mark.parametrize("p", PS)
def test_plans_are_sum_and_prod_plans_but_for_the_handle(mvx, p):
    seen = set()
    for h in A.TYPES:
        for cname, coll in _colls(mvx).items():
            root = p // 2 if cname == "red" else 0
            for n in _counts(A.ESIZE[h]):
                rc = _cnts(n, p) if cname == "rs" else None
                for op in A.OPS:
                    for r in range(p):
                        got = mvx.plan(coll, p, r, n, h, op, root, recvcnts=rc)
                        ref = mvx.plan(coll, p, r, n, h, A.BASE[op], root, recvcnts=rc)
                        assert got.op == op and ref.op == A.BASE[op]
                        assert _image(got, 0) == _image(ref, 0), (h, cname, n, op, r)
                    seen.add((coll, got.alg))
    if p >= 4:      # both sides of the switches were visited
        assert {(mvx.COLL_ALLREDUCE, mvx.ALG_RECDBL), (mvx.COLL_ALLREDUCE, mvx.ALG_RABENSEIFNER),
                (mvx.COLL_REDUCE, mvx.ALG_BINOMIAL), (mvx.COLL_REDUCE, mvx.ALG_RABENSEIFNER),
                (mvx.COLL_REDUCE_SCATTER, mvx.ALG_RS_HALVING), (mvx.COLL_REDUCE_SCATTER, mvx.ALG_RS_PAIRWISE)} <= seen


def _launch(mvx, op, h, k, n, tmask, cmask, offs, foffs=None):
    srcs = [(q + 1 << 32) + 256 + o for q, o in enumerate(offs[:k])]
    folds = [((20 + q) << 32) + 256 + o if o is not None else None for q, o in enumerate(foffs)] if foffs else None
    rc, pl = mvx.op_plan(op, h, srcs, (40 << 32) + 256 + offs[k], n, tmask, cmask, folds=folds)
    assert rc == 0
    return pl.symbol.decode(), pl.tag.decode(), pl.blocks, pl.dynamic_lds


@pytest.mark.parametrize("op,h", A.PAIRS, ids=A.IDS)
def test_launch_plan_is_sums_family_and_split_in_the_new_unit(mvx, op, h):
    """mvx_op_plan: the kernel MPI_SUM / MPI_PROD gets for the same pointers
    and n, instantiated for the new op (12 / 13 in the template's first
    argument), the same grid and LDS reservation."""
    hip = mvx.hip()
    e = A.ESIZE[h]
    o_new, o_old = op - 164 + 12, A.BASE[op] - 100
    cases = []
    for n in (1, 17, 4099, (64 << 20) // e):
        cases += [(2, n, 1, 0, [0] * 3, None), (2, n, 1, 0, [2 * e] * 3, None), (2, n, 1, 0, [0, e, 0], None),
                  (8, n, hip.mvx_tree_mask(8), 0, [0] * 9, None), (4, n, hip.mvx_tree_mask(4), 0, [0] * 5, None),
                  (4, n, 0, hip.mvx_chain_mask(4), [0] * 5, None), (6, n, 0, hip.mvx_chain_mask(6), [0] * 7, None),
                  (8, n, 0, hip.mvx_chain_mask(8), [4] * 9, None), (3, n, hip.mvx_tree_mask(3), 0, [0] * 4, None),
                  (3, n, hip.mvx_tree_mask(3), 0, [0] * 4, [None, 0, None]),
                  (7, n, hip.mvx_tree_mask(7), 0, [0] * 8, [None, 0, None, 0, None, 0, None]),
                  (5, n, hip.mvx_tree_mask(4), 1 << 4, [0, e, 0, 0, 0, 0], None)]
    bases = set()
    for k, n, tm, cm, offs, foffs in cases:
        sym, tag, blocks, lds = _launch(mvx, op, h, k, n, tm, cm, offs, foffs)
        rsym, rtag, rblocks, rlds = _launch(mvx, A.BASE[op], h, k, n, tm, cm, offs, foffs)
        base, rest = sym.split("<", 1)
        rbase, rrest = rsym.split("<", 1)
        assert base == rbase and TNAME[h] in sym, (sym, rsym)
        assert rest.startswith("%d, " % o_new) and rrest.startswith("%d, " % o_old), (sym, rsym)
        assert rest[len("%d" % o_new):] == rrest[len("%d" % o_old):], (sym, rsym)
        assert (blocks, lds) == (rblocks, rlds), (sym, blocks, rblocks, lds, rlds)
        assert tag.startswith(("sum" if op == 164 else "prod") + "_acc32_") and tag != rtag
        bases.add(base)
    assert bases == {"k_combine", "k_tree_body", "k_chain_body"}


# ------------------------------------------- the reference against the oracle

def _oracle_float(oracle, cname, F, n, cnts, op, root):
    p = len(F)
    sizes = [max(c, 1) for c in cnts] if cname == "rs" else [n] * p
    R = [np.zeros(s, np.float32) for s in sizes]
    S8, R8 = [f.view(np.uint8) for f in F], [r.view(np.uint8) for r in R]
    if cname == "ar":
        rc = oracle.allreduce(S8, R8, n, MPI_FLOAT, op)
    elif cname == "red":
        rc = oracle.reduce(S8, R8, n, MPI_FLOAT, op, root)
    elif cname == "rs":
        rc = oracle.reduce_scatter(S8, R8, cnts, MPI_FLOAT, op)
    else:
        rc = oracle.scan(S8, R8, n, MPI_FLOAT, op)
    assert rc == [0] * p
    return R


@pytest.mark.parametrize("p", PS_ORACLE)
@pytest.mark.parametrize("h", A.TYPES, ids=[A.NAMES[h] for h in A.TYPES])
def test_reference_equals_the_oracles_float_collective_narrowed(mvx, oracle, p, h):
    """acc32_ref.run_plans == narrow(the oracle's MPI_FLOAT SUM / PROD
    collective on the exactly widened sends), at counts where the narrow type
    and MPI_FLOAT take the same algorithm (asserted): the float32 steps, their
    order and the operand roles are the reference's own, and the narrowing is
    the only thing added."""
    e = A.ESIZE[h]
    for cname, cid in _colls(mvx).items():
        for n in (1, 5, 300):
            assert mvx.algorithm(cid, p, n, h) == mvx.algorithm(cid, p, n, MPI_FLOAT)
            if cname != "scan":
                assert mvx.algorithm(cid, p, n, h) == oracle.algorithm(cid, p, n, MPI_FLOAT)
            cnts = _cnts(n, p)
            S = [A.coll_vec(h, n, 77 * p + 5 * r + n) for r in range(p)]
            F = [A.widen(h, s) for s in S]
            sizes = [max(c, 1) for c in cnts] if cname == "rs" else [n] * p
            for op in A.OPS:
                for root in (range(p) if cname == "red" else [0]):
                    plans = [mvx.plan(cid, p, r, 0 if cname == "rs" else n, h, op, root,
                                      cnts if cname == "rs" else None) for r in range(p)]
                    got = A.run_plans(plans, S, [np.full(s * e, 0x5C, np.uint8) for s in sizes])
                    R = _oracle_float(oracle, cname, F, n, cnts, A.BASE[op], root)
                    for r in range(p):
                        m = cnts[r] if cname == "rs" else n
                        if (cname == "red" and r != root) or m == 0:
                            continue
                        A.assert_same(op, h, got[r][:m * e], A.round_to(h, R[r][:m]), (cname, p, n, op, root, r))


# ----------------------------------------------------------------- properties

@pytest.mark.parametrize("p", [2, 3, 7, 9, 16, 33, 64])
def test_e4m3_sum_is_exact_before_narrowing(mvx, p):
    """Every finite E4M3 value is a multiple of 2^-9 of magnitude <= 448: a
    sum of 64 is a multiple of 2^-9 below 2^15, 24 bits, exact in float32
    whatever the association.  So the result is the float64 sum rounded once."""
    h, n = fp8_ref.E4M3, 300
    rng = np.random.default_rng(p)
    cnts = _cnts(n, p)
    S = [rng.integers(0, 256, n).astype(np.uint8) for _ in range(p)]
    for s in S:
        s[(s & 0x7f) == 0x7f] = 0x7e                     # finite operands (NaN has no exact sum)
    W = [fp8_ref.widen(h, s) for s in S]
    prefix = [W[0]]                                      # float64 sums, exact (a zero's sign is order-free too:
    for w in W[1:]:                                      # -0 only where every operand is -0)
        prefix.append(prefix[-1] + w)
    exact = prefix[-1]
    assert np.abs(exact).max() > 448                     # some sums overflow the format: NaN on both sides
    want = fp8_ref.encode(h, exact)
    for cname, cid in _colls(mvx).items():
        plans = [mvx.plan(cid, p, r, 0 if cname == "rs" else n, h, 164, p - 1, cnts if cname == "rs" else None)
                 for r in range(p)]
        sizes = [max(c, 1) for c in cnts] if cname == "rs" else [n] * p
        got = A.run_plans(plans, S, [np.full(s, 0x5C, np.uint8) for s in sizes])
        off = np.cumsum([0] + cnts)
        for r in range(p):
            if cname == "ar" or (cname == "red" and r == p - 1):
                A.assert_same(164, h, got[r], want, (cname, p, r))
            elif cname == "rs" and cnts[r]:
                A.assert_same(164, h, got[r][:cnts[r]], want[off[r]:off[r + 1]], (cname, p, r))
            elif cname == "scan":
                A.assert_same(164, h, got[r], fp8_ref.encode(h, prefix[r]), (cname, p, r))


def _per_step(h, op, leaves, cmask):
    m = half_ref if h in half_ref.TYPES else fp8_ref
    return m.run_program(A.BASE[op], h, [x.copy() for x in leaves], None, 0, cmask, 1)


def test_one_rounding_differs_from_a_rounding_per_step():
    """Hand-made chains ((a op b) op c) ...: the per-step references and the
    wide one must differ, and the wide one gives the correctly rounded exact
    result."""
    F16, BF16, E4M3, E5M2 = 64, 65, 72, 73

    def leaf(h, v):
        m = half_ref if h in half_ref.TYPES else fp8_ref
        return np.ascontiguousarray(m.narrow(h, np.array([v], np.float32))).view(np.uint8)

    cases = [
        # max + max - max: NaN (E4M3) or inf per step, max itself in f32 (BF16 has f32's range: no such case)
        (E4M3, 164, [448.0, 448.0, -448.0], 448.0),
        (E5M2, 164, [57344.0, 57344.0, -57344.0], 57344.0),
        (F16, 164, [65504.0, 65504.0, -65504.0], 65504.0),
        # addends below half an ulp of the running value vanish one by one, not together
        (E4M3, 164, [16.0, 0.5, 0.5, 0.5], 18.0),
        (E5M2, 164, [8.0, 0.5, 0.5, 0.5], 10.0),
        (F16, 164, [2048.0, 0.5, 0.5, 0.5], 2050.0),
        (BF16, 164, [1.0, 2.0 ** -9, 2.0 ** -9, 2.0 ** -9], 1.0 + 2.0 ** -7),
        # products: an intermediate overflow or underflow that the f32 range absorbs
        (E4M3, 165, [256.0, 2.0, 0.5], 256.0),
        (E5M2, 165, [2.0 ** -16, 0.5, 4.0], 2.0 ** -15),
        (F16, 165, [2.0 ** -24, 0.5, 4.0], 2.0 ** -23),
        # 1.26960754...: just above the midpoint of 1.265625 and 1.2734375; per step (1 + 2^-7)^2 loses its 2^-14
        (BF16, 165, [1.0 + 2.0 ** -7, 1.0 + 2.0 ** -7, 1.25], 1.2734375),
    ]
    for h, op, vals, want in cases:
        leaves = [leaf(h, v) for v in vals]
        cm = A.chain_mask(len(vals))
        wide = A.run_program(op, h, leaves, None, 0, cm, 1)
        step = np.ascontiguousarray(_per_step(h, op, leaves, cm)).view(np.uint8)
        assert not np.array_equal(wide, step), (h, op, vals)
        assert np.array_equal(wide, leaf(h, want)), (h, op, vals, wide, leaf(h, want))
    # eight smallest E4M3 subnormals: 8 * 2^-9 = 2^-6 is a value of the format and
    # so is every partial sum -- here the two definitions agree
    ones = [np.array([1], np.uint8)] * 8
    assert np.array_equal(A.run_program(164, E4M3, ones, None, A.tree_mask(8), 0, 1), np.array([0x08], np.uint8))
    assert np.array_equal(_per_step(E4M3, 164, ones, A.chain_mask(8)), np.array([0x08], np.uint8))


@pytest.mark.parametrize("op,h", A.PAIRS, ids=A.IDS)
def test_two_operands_equal_the_per_step_op(op, h):
    """One float32 step rounded once is the correctly rounded result: with
    two leaves and no fold the wide ops equal MPI_SUM / MPI_PROD -- all 65,536
    byte pairs of an 8-bit type, all 65,536 patterns of a 16-bit type against
    partners(), either role."""
    if h in fp8_ref.TYPES:
        v = np.arange(256, dtype=np.uint8)
        a, b = np.repeat(v, 256), np.tile(v, 256)
        pairs = [(a, b)]
        per_step = fp8_ref.op
    else:
        allp = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        pairs = []
        for q in half_ref.partners(h):
            pairs += [(allp, np.full(65536, q, np.uint16)), (np.full(65536, q, np.uint16), allp)]
        per_step = half_ref.op
    for io, inv in pairs:
        want = per_step(A.BASE[op], h, inv, io)
        got = A.run_program(op, h, [io.view(np.uint8), inv.view(np.uint8)], None, 1, 0, io.size)
        A.assert_same(op, h, got, np.ascontiguousarray(want).view(np.uint8), (op, h))


# ------------------------------------------ scratch slots of the wide executor

@pytest.mark.parametrize("p", list(range(9, 65)))
def test_wide_executor_stays_within_its_scratch_slots(mvx, p):
    """Programs over more than 8 leaves: widening raw leaves to f32 takes
    scratch slots of its own.  mvx_plan_wide_slots replays the executor's
    launches without a device; the slots it takes stay within what
    mvxi_wide_temps reserves, for every rank of every collective, and the
    per-step ops take no more than the wide ones."""
    wide_seen = False
    for cname, coll in _colls(mvx).items():
        root = p - 1 if cname == "red" else 0
        for n in (1, 7, 300, 20001, 1 << 20):
            rc = [n // p + 1] * p if cname == "rs" else None
            for r in range(p):
                used = {}
                for h, op in ((72, 164), (64, 165), (72, 102), (MPI_FLOAT, 102)):
                    P = mvx.plan(coll, p, r, n, h, op, root, recvcnts=rc)
                    budget, used[h, op] = P.wide_slots()
                    assert used[h, op] <= budget, (cname, n, r, h, op, P.k, budget, used)
                    assert (budget > 0) == (P.k > 8) and (used[h, op] > 0) == (P.k > 8)
                    wide_seen |= P.k > 8
                assert used[72, 102] <= used[72, 164]
    assert wide_seen
