"""GPU: derived datatypes and communicators of up to 64 ranks through the
executor of programs over more than 8 leaves (mvx_combine.c: combine_wide,
tree_eval, chain_eval; combine_user step by step; combine_packed around both).

Virtual communicators (p ranks' buffers on one GPU) against the oracle's replay
of the reference schedule.  Recv buffers are pre-filled with 0x5C and compared
whole with np.array_equal, so the bytes outside a type map must keep the
caller's pattern; the per-rank codes must be the oracle's.  No tolerance and no
exempt element anywhere in this file.

* MAXLOC / MINLOC on a struct of every first-member kind mvx_ops.hip's
  derived_kind() knows (INT, FLOAT, SHORT, LONG, LONG_LONG_INT, DOUBLE,
  LONG_DOUBLE; two dense, five packed), p = 3, 8 (one launch) and 9, 16, 17,
  33, 64, device and host buffers, every collective, the counts on both sides
  of every algorithm switch.  Both ops are idempotent and associative, so the
  data makes every rank the only winner at some elements and the winner of a
  tie by its loc at others: a dropped leaf changes the result.
* user functions on the packed struct {int; hole; double} at p = 9, 17, 33, 64:
  idsum, and idmix, which is neither commutative nor associative, so a change
  of operand role or grouping in the packed wide path changes the bits.
* an undefined (op, type) on a packed type at p = 16, 33: the 329s of the
  oracle's ranks, the data moved as the reference moves it.
* basic types at the communicator sizes the wide executor is not run at
  elsewhere (17, 31, 32, 63, 64), MPI_LONG_DOUBLE SUM at every wide size, and
  the noncommutative user ops at 33 and 64 ranks (chain_swap bits >= 32).

Every case asserts from the plans that a program of more than 8 leaves (and,
for a type with holes, a packed one) is what ran.
"""
import numpy as np
import pytest

import mvxtest as T
import test_gpu_exec as X
import typemap_util as TM
import uops
from wide_pairs import PAIR_KINDS, PAIR_LAYOUT, pair_sends

pytestmark = pytest.mark.gpu

I, D, XF = 6, 11, 12
COLLS = ["ar", "red", "rs", "scan"]
PS = [3, 8, 9, 16, 17, 33, 64]
ALL_PS = [3, 8, 9, 16, 17, 31, 32, 33, 63, 64]
FILL = 0x5C
H_ORACLE = 250                      # the oracle's handle for the user function under test


@pytest.fixture(scope="module")
def comms(mvx):
    cs = {p: mvx.Comm.local_ranks(p, 0) for p in ALL_PS}
    yield cs
    for c in cs.values():
        c.free()


@pytest.fixture(scope="module")
def types(mvx, oracle):
    t = {k: TM.both(mvx, oracle, "struct", 2, [1, 1], v[1], v[0]) for k, v in PAIR_KINDS.items()}
    t["int_hole_double"] = TM.both(mvx, oracle, "struct", 2, [1, 1], [0, 8], [I, D])
    t["vec_int"] = TM.both(mvx, oracle, "vector", 3, 2, 5, I)
    yield t
    TM.free_all(mvx, oracle, t.values())


# ------------------------------------------------------------------ helpers

def _cid(mvx, coll):
    return {"ar": mvx.COLL_ALLREDUCE, "red": mvx.COLL_REDUCE, "rs": mvx.COLL_REDUCE_SCATTER,
            "scan": mvx.COLL_SCAN}[coll]


def _call(comm, coll, sends, recvs, n, dt, op, root, cnts):
    if coll == "ar":
        return comm.allreduce_multi(sends, recvs, n, dt, op)
    if coll == "red":
        return comm.reduce_multi(sends, recvs, n, dt, op, root)
    if coll == "scan":
        return comm.scan_multi(sends, recvs, n, dt, op)
    return comm.reduce_scatter_multi(sends, recvs, cnts, dt, op)


def _replay(oracle, coll, S, R, n, dt, op, root, cnts):
    if coll == "ar":
        return oracle.allreduce(S, R, n, dt, op)
    if coll == "red":
        return oracle.reduce(S, R, n, dt, op, root)
    if coll == "scan":
        return oracle.scan(S, R, n, dt, op)
    return oracle.reduce_scatter(S, R, cnts, dt, op)


def _plans(mvx, coll, p, n, cnts, dt, op, root, opkind=None):
    """Every rank's plan; before anything runs, the scratch slots a program of
    more than 8 leaves takes stay within what the executor reserves for it."""
    plans = [mvx.plan(_cid(mvx, coll), p, r, 0 if coll == "rs" else n, dt, op, root,
                      cnts if coll == "rs" else None, opkind=opkind) for r in range(p)]
    for P in plans:
        if P.has_combine and P.k > 8 and opkind is None:
            budget, used = P.wide_slots()
            assert used <= budget, (coll, p, P.rank, budget, used)
    return plans


def _place(where, arrays):
    import torch
    if where == "device":
        return [torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda() for a in arrays]
    return [np.ascontiguousarray(a).view(np.uint8).copy() for a in arrays]


def _bytes(buf):
    return buf if isinstance(buf, np.ndarray) else T.from_dev(buf)


def _ragged(coll, p, n):
    """(total elements of a send, per-rank recv counts or None)."""
    if coll != "rs":
        return n, None
    cnts = [n + (r % 2) for r in range(p)]
    return sum(cnts), cnts


def _check(mvx, oracle, comm, where, coll, S, sends, n, cnts, ext, dt, op, ref_op, root, what):
    """One collective on the device against the replay: overall code 0, the
    oracle's per-rank codes (returned), every rank's whole recv buffer."""
    p = len(S)
    R0 = [np.full(max(k, 1) * ext, FILL, np.uint8) for k in (cnts if cnts else [n] * p)]
    recvs = _place(where, R0)
    r, rcs = _call(comm, coll, sends, recvs, n, dt, op, root, cnts)
    assert r == 0, (what, r)                 # MPI_ERR_TYPE, the documented refusal, included
    ref = [x.copy() for x in R0]
    rref = _replay(oracle, coll, S, ref, n, dt, ref_op, root, cnts)
    assert rcs == rref, (what, rcs, rref)
    for q in range(p):
        got = _bytes(recvs[q])
        assert np.array_equal(got, ref[q]), (what, "rank", q, "first bytes", np.flatnonzero(got != ref[q])[:8])
    return rref


def _switch(mvx, cid, p, dt):
    """The smallest count whose algorithm differs from count 3's (None: no switch)."""
    a0 = mvx.algorithm(cid, p, 3, dt)
    for c in range(4, 4097):
        if mvx.algorithm(cid, p, c, dt) != a0:
            return c
    return None


def _far_count(mvx, oracle, cid, p, dt):
    """A count on the far side of the Allreduce / Reduce algorithm switch.  A
    communicator of 3 has none (one algorithm at every count): it takes the
    count of p = 8, as an anchor at the same size."""
    c = _switch(mvx, cid, p, dt)
    if p >= 8:
        assert c is not None
        assert mvx.algorithm(cid, p, c, dt) == oracle.algorithm(cid, p, c, dt) != mvx.algorithm(cid, p, 3, dt)
    return c if c is not None else _switch(mvx, cid, 8, dt)


# ------------------------------------------- A1: pair structs, MAXLOC / MINLOC

def test_pair_struct_layouts(mvx, types):
    """The table of the cases: which structs are dense and which move packed,
    from the library's own layout and from the plans' packed flag."""
    for kind, (ext, size) in PAIR_LAYOUT.items():
        h = types[kind]
        assert (mvx.MPI_Type_extent(h)[1], mvx.MPI_Type_size(h)[1]) == (ext, size), kind
        dense = bool(mvx.type_layout(h)["dense"])
        assert dense == (size == ext), kind
        assert mvx.hip().mvx_op_element_size(111, h) == ext, kind      # never the MPI_ERR_TYPE refusal
        for p in (3, 64):
            P = mvx.plan(mvx.COLL_ALLREDUCE, p, 0, 301, h, 111)
            assert bool(P.packed) == (not dense), (kind, p)
    assert sorted(k for k, (e, s) in PAIR_LAYOUT.items() if s < e) == [
        "double_int", "long_int", "longdouble_int", "longlong_int", "short_int"]


def _pair_runs(mvx, oracle, coll, p, h, size):
    """[(count, root)] of a (type, p, collective) case."""
    if coll == "ar":
        return [(n, 0) for n in (1, 3, 301, _far_count(mvx, oracle, mvx.COLL_ALLREDUCE, p, h))]
    if coll == "red":
        far = _far_count(mvx, oracle, mvx.COLL_REDUCE, p, h)
        return [(n, root) for n in (3, far) for root in sorted({0, p // 2, p - 1})]
    if coll == "rs":
        return [(3, 0), ((512 << 10) // (p * size) + 1, 0)]
    return [(257, 0)]


@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("kind", list(PAIR_KINDS))
def test_pair_structs_maxloc_minloc(mvx, oracle, comms, types, kind, coll, p, where):
    """MAXLOC and MINLOC on a struct of each first-member kind, over sends in
    which every rank decides some element (wide_pairs.pair_sends).  Allreduce
    at counts 1, 3, 301 and past its algorithm switch; Reduce at three roots,
    count 3 and past its switch; Reduce_scatter ragged, at 3 per rank (halving)
    and just above 512 KiB in all (pairwise); Scan at 257."""
    h = types[kind]
    ext, size = PAIR_LAYOUT[kind]
    packed = size < ext
    algs = set()
    sent = {}
    for n0, root in _pair_runs(mvx, oracle, coll, p, h, size):
        n, cnts = _ragged(coll, p, n0)
        if n0 not in sent:                                  # a Reduce's roots share their sends
            S = pair_sends(kind, p, n, 1000 * p + 7 * n0 + len(kind))
            sent = {n0: (list(S), _place(where, S))}
        S, sends = sent[n0]
        for op in (111, 110):
            what = (kind, coll, p, where, n0, root, op)
            plans = _plans(mvx, coll, p, n, cnts, h, op, root)
            assert {bool(P.packed) for P in plans if P.has_combine} == {packed}, what
            if p >= 16:
                assert max(P.k for P in plans) > 8, what    # a program of more than 8 leaves ran
            algs.add(plans[0].alg)
            if coll == "rs":
                assert plans[0].alg == oracle.algorithm(3, p, n, h), what
            rref = _check(mvx, oracle, comms[p], where, coll, S, sends, n, cnts, ext, h, op, op, root, what)
            assert rref == [0] * p, what
    if coll == "rs":
        assert algs == {mvx.ALG_RS_HALVING, mvx.ALG_RS_PAIRWISE}, algs
    elif coll != "scan" and p >= 8:
        assert len(algs) == 2, algs


# ----------------------------------- A2: user functions on a packed struct

ID_OPS = [("idsum", 1), ("idmix", 0), ("idmix", 1)]
ID_MODES = [("device_fn", "device"), ("host_fn", "device"), ("host_fn", "host")]


@pytest.mark.parametrize("p", [9, 17, 33, 64])
@pytest.mark.parametrize("fn,where", ID_MODES, ids=["%s-%s" % m for m in ID_MODES])
@pytest.mark.parametrize("name,commute", ID_OPS, ids=["%s-commute%d" % o for o in ID_OPS])
def test_user_functions_on_a_packed_struct(mvx, oracle, comms, types, name, commute, fn, where, p):
    """struct {int; hole; double} moves packed; the user function sees it at
    its extent (combine_packed around combine_user, 2 k scratch slots).  idmix
    registered noncommutative takes the reference's role swaps, registered
    commutative its commutative branches; the hole keeps the caller's bytes."""
    h = types["int_hole_double"]
    ext = uops.IDPAIR_EXTENT
    assert mvx.MPI_Type_extent(h)[1] == ext and not mvx.type_layout(h)["dense"]
    if fn == "device_fn":
        rc, uop = mvx.op_create_device(uops.dev_fn(name), commute)
    else:
        rc, uop = mvx.MPI_Op_create(uops.host_fn(name), commute)
    assert rc == 0
    assert oracle.user_op_set(H_ORACLE, uops.host_fn(name), commute) == 0
    kind = mvx.OPKIND_USER_COMMUTE if commute else mvx.OPKIND_USER_NONCOMMUTE
    seen_wide = False
    try:
        for coll, n0, root in (("ar", 33, 0), ("red", 33, 1), ("red", 33, p - 1), ("rs", 200, 0), ("scan", 33, 0)):
            n, cnts = _ragged(coll, p, n0)
            what = (name, commute, fn, where, p, coll, root)
            plans = _plans(mvx, coll, p, n, cnts, h, uop, root, opkind=kind)
            assert all(P.packed for P in plans if P.has_combine), what
            wide = any(P.k > 8 and P.packed for P in plans)
            assert wide or p < 16, what
            seen_wide |= wide
            S = [uops.rand_idpair(n, 31 * p + r + n0) for r in range(p)]
            rref = _check(mvx, oracle, comms[p], where, coll, S, _place(where, S), n, cnts, ext, h, uop, H_ORACLE,
                          root, what)
            assert rref == [0] * p, what
        assert seen_wide
    finally:
        mvx.MPI_Op_free(uop)


# --------------------------------------- A3: an undefined op on a packed type

@pytest.mark.parametrize("where", ["device", "host"])
@pytest.mark.parametrize("p", [16, 33])
@pytest.mark.parametrize("tname,op", [("double_int", 102), ("vec_int", 111)])
def test_undefined_op_on_a_packed_type(mvx, oracle, comms, types, tname, op, p, where):
    """MPI_SUM on {double; int} and MAXLOC on vector(3, 2, 5, INT): 329 from
    exactly the oracle's ranks; the data moves as the reference moves it (the
    packed leaf 0 of every combine, mvxi_combine's keep branch), and the bytes
    outside the type map keep the caller's pattern."""
    h = types[tname]
    ext = mvx.MPI_Type_extent(h)[1]
    assert mvx.type_layout(h)["span_hi"] <= ext and not mvx.type_layout(h)["dense"]
    seen = 0
    for coll, n0, root in (("ar", 3, 0), ("ar", 301, 0), ("red", 3, p // 2), ("red", 301, p - 1), ("rs", 3, 0),
                           ("scan", 257, 0)):
        n, cnts = _ragged(coll, p, n0)
        what = (tname, op, p, where, coll, n0)
        plans = _plans(mvx, coll, p, n, cnts, h, op, root)
        assert all(P.packed for P in plans if P.has_combine) and max(P.k for P in plans) > 8, what
        rng = np.random.default_rng(97 * p + n0 + op)
        S = [rng.integers(0, 256, n * ext, dtype=np.uint8) for _ in range(p)]
        rref = _check(mvx, oracle, comms[p], where, coll, S, _place(where, S), n, cnts, ext, h, op, op, root, what)
        # every rank that calls the op answers 329: all of them but in a Scan,
        # whose replay reports none (its codes are compared like the others)
        assert set(rref) <= {0, 329} and (329 in rref) == (coll != "scan"), (what, rref)
        seen += rref.count(329)
    assert seen >= 5 * (p // 2)


# ------------------------- A4: basic types at the sizes the device has not run

def _exact(got_u8, ref, what):
    """Every bit of the type map: whole elements, or a pair's value and loc
    (the 4 bytes after a {double; int} pair's loc are no part of the type)."""
    ref = np.ascontiguousarray(ref)
    got = np.asarray(got_u8).view(np.uint8)
    assert got.nbytes == ref.nbytes, what
    got = got.view(ref.dtype)
    for f in (ref.dtype.names or [None]):
        g = np.ascontiguousarray(got[f] if f else got).view(np.uint8)
        e = np.ascontiguousarray(ref[f] if f else ref).view(np.uint8)
        assert np.array_equal(g, e), (what, f, "first bytes", np.flatnonzero(g != e)[:8])


WIDE_RUNS = (("ar", 7), ("ar", 20000), ("red", 9), ("red", 20000), ("rs", 3), ("rs", 9000), ("scan", 300))
WIDE_IDS = ["%s%d" % r for r in WIDE_RUNS]


def _basic_sends(dtype, p, n, seed):
    """Every rank's mvxtest.rand_vec, as test_gpu_exec draws them; above 2^20
    elements in all (where drawing them, the x87 patterns above all, would
    take longer than the collective) the ranks take windows of one vector,
    997 elements apart, so that no two leaves agree at an element."""
    if p * n <= 1 << 20:
        return [T.rand_vec(dtype, n, seed + r) for r in range(p)]
    base = T.rand_vec(dtype, n + 997 * (p - 1), seed)
    return [T.clone(base[997 * r:997 * r + n]) for r in range(p)]


def _basic_run(mvx, oracle, comm, p, op, dtype, coll, n0):
    import torch
    E = mvx.dtype_info(dtype)[0]
    n, cnts = _ragged(coll, p, n0)
    root = p // 2
    what = (op, dtype, p, coll, n0)
    plans = _plans(mvx, coll, p, n, cnts, dtype, op, root)
    S = _basic_sends(dtype, p, n, 7 * p + n0)
    sends = [T.to_dev(s) for s in S]
    sizes = cnts if cnts else [n] * p
    recvs = [torch.full((k * E,), FILL, dtype=torch.uint8, device="cuda") for k in sizes]
    r, rcs = _call(comm, coll, sends, recvs, n, dtype, op, root, cnts)
    assert r == 0, what
    R0 = [np.zeros(k, S[0].dtype) for k in sizes]
    rref = X._oracle_coll(oracle, coll, S, R0, cnts if cnts else n, dtype, op, root)
    assert rcs == rref == [0] * p, (what, rcs, rref)
    for q in range(p):
        got = T.from_dev(recvs[q])
        if coll == "red" and q != root:
            assert (got == FILL).all(), (what, q)          # a non-root's recvbuf is untouched
        else:
            _exact(got, R0[q], what + (q,))
    return plans


@pytest.mark.parametrize("coll,n0", WIDE_RUNS, ids=WIDE_IDS)
@pytest.mark.parametrize("p", [17, 31, 32, 63, 64])
@pytest.mark.parametrize("op,dtype", X.WIDE_CASES)
def test_basic_types_at_17_to_64_ranks(mvx, oracle, comms, op, dtype, p, coll, n0):
    """test_gpu_exec's wide cases at the sizes between and above its own: the
    8 x 8 tree (p = 64), groups truncated at 63 and 31, trees of 17 and 32,
    Scan with six and seven segments."""
    plans = _basic_run(mvx, oracle, comms[p], p, op, dtype, coll, n0)
    assert max(P.k for P in plans) > 8
    if coll == "scan":
        assert max(len(P.segments()) for P in plans) == p.bit_length()      # 5, 5, 6, 6, 7


@pytest.mark.parametrize("coll,n0", WIDE_RUNS, ids=WIDE_IDS)
@pytest.mark.parametrize("p", [9, 16, 17, 31, 32, 33, 63, 64])
def test_long_double_sum_over_more_than_8_leaves(mvx, oracle, comms, p, coll, n0):
    """MPI_LONG_DOUBLE SUM has a family rule of its own (alu_heavy: no body
    kernels, one element per lane); every bit of the x87 slot, padding
    included, at every wide size."""
    plans = _basic_run(mvx, oracle, comms[p], p, 102, XF, coll, n0)
    # 9 ranks fold to 8 leaves in the power-of-two algorithms: wide there only in
    # the binomial Reduce, the pairwise Reduce_scatter and Scan
    assert (max(P.k for P in plans) > 8) == (p >= 16 or (coll, n0) in {("red", 9), ("rs", 9000), ("scan", 300)})


@pytest.mark.parametrize("p", [33, 64])
@pytest.mark.parametrize("device_fn", [False, True], ids=["host_fn", "device_fn"])
@pytest.mark.parametrize("name", ["mix", "affine"])
def test_noncommutative_user_ops_at_33_and_64_ranks(mvx, oracle, comms, name, device_fn, p):
    """combine_user step by step over up to 64 scratch copies; at p = 64 the
    role swaps of leaves 32.. are bits >= 32 of the 64-bit chain_swap mask."""
    import torch
    if device_fn:
        rc, uop = mvx.op_create_device(uops.dev_fn(name), 0)
    else:
        rc, uop = mvx.MPI_Op_create(uops.host_fn(name), 0)
    assert rc == 0
    assert oracle.user_op_set(H_ORACLE, uops.host_fn(name), 0) == 0
    dt = uops.UOPS[name][0]
    high_swaps = False
    try:
        for coll, n0 in (("ar", 33), ("red", 33), ("rs", 200), ("scan", 33)):
            n, cnts = _ragged(coll, p, n0)
            what = (name, device_fn, p, coll)
            plans = _plans(mvx, coll, p, n, cnts, dt, uop, 1, opkind=mvx.OPKIND_USER_NONCOMMUTE)
            assert max(P.k for P in plans) > 8, what
            high_swaps |= any(P.chain_swap >> 32 for P in plans)
            S = [uops.rand_for(name, n, 31 * p + r) for r in range(p)]
            E = S[0].itemsize
            sends = [T.to_dev(s) for s in S]
            sizes = cnts if cnts else [n] * p
            recvs = [torch.full((k * E,), FILL, dtype=torch.uint8, device="cuda") for k in sizes]
            r, rcs = _call(comms[p], coll, sends, recvs, n, dt, uop, 1, cnts)
            assert r == 0 and rcs == [0] * p, what
            R0 = [np.zeros(k, S[0].dtype) for k in sizes]
            assert X._oracle_coll(oracle, coll, S, R0, cnts if cnts else n, dt, H_ORACLE, 1) == [0] * p
            for q in range(p):
                got = T.from_dev(recvs[q])
                if coll == "red" and q != 1:
                    assert (got == FILL).all(), (what, q)
                else:
                    assert T.bytes_equal(got, R0[q]), (what, q)
        assert high_swaps or p < 64
    finally:
        mvx.MPI_Op_free(uop)
