"""GPU: the collectives with MVX_SUM_ACC32 / MVX_PROD_ACC32 on the four narrow
floating types.

Virtual communicators (p ranks' buffers on one GPU) run every rank's plan on
the device.  Three references:

* tests/acc32_ref.py evaluates the same plans in float32, straight from the
  plan (it knows nothing of the executor's groups of 8), and rounds once;
* the reference itself: the oracle's MPI_FLOAT SUM / PROD collective on the
  exactly widened sends, narrowed -- at counts where both take the same
  algorithm;
* for E4M3 SUM, whose float32 value is exact, the float64 sum rounded once.

And the paths around the kernels: programs over more than 8 leaves (f32
temporaries), host buffers, the blocking calls, the undefined pairs.
"""
import os

import numpy as np
import pytest

import acc32_ref as A
import fp8_ref
import mvxtest as T

pytestmark = pytest.mark.gpu

MPI_FLOAT, MPI_INT = 10, 6
PS = [1, 2, 3, 4, 5, 6, 7, 8, 12]
COUNTS = [1, 5, 333, 4096, 8192, 40000]
PIN_COUNTS = [1, 5, 300]
NAN_CAP = 0.10
COLLS = ["ar", "red", "rs", "scan"]
TYPE_IDS = [A.NAMES[d] for d in A.TYPES]


@pytest.fixture(scope="module")
def comms(mvx):
    cs = {p: mvx.Comm.local_ranks(p, 0) for p in PS}
    yield cs
    for c in cs.values():
        c.free()


@pytest.fixture(scope="module")
def wide(mvx):
    cs = {p: mvx.Comm.local_ranks(p, 0) for p in (9, 16, 33)}
    yield cs
    for c in cs.values():
        c.free()


def _split(n, p):
    return [n // p + (1 if r < n % p else 0) for r in range(p)]


def _coll_id(mvx, coll):
    return {"ar": mvx.COLL_ALLREDUCE, "red": mvx.COLL_REDUCE, "rs": mvx.COLL_REDUCE_SCATTER,
            "scan": mvx.COLL_SCAN}[coll]


def _roots(coll, p):
    if coll != "red":
        return [0]
    return list(range(p)) if p <= 4 else sorted({0, p // 2, p - 1})


def _sizes(coll, p, n, cnts):
    return [max(c, 1) for c in cnts] if coll == "rs" else [n] * p


def _device(comm, coll, p, dsends, n, cnts, dtype, op, root):
    """One collective on the device: (per-rank recv bytes, per-rank codes)."""
    import torch
    e = A.ESIZE.get(dtype, 4)
    drs = [torch.full((s * e,), 0x5C, dtype=torch.uint8, device="cuda") for s in _sizes(coll, p, n, cnts)]
    if coll == "ar":
        r, rcs = comm.allreduce_multi(dsends, drs, n, dtype, op)
    elif coll == "red":
        r, rcs = comm.reduce_multi(dsends, drs, n, dtype, op, root)
    elif coll == "rs":
        r, rcs = comm.reduce_scatter_multi(dsends, drs, cnts, dtype, op)
    else:
        r, rcs = comm.scan_multi(dsends, drs, n, dtype, op)
    assert r == 0, (coll, p, n, r)
    return [T.from_dev(x) for x in drs], rcs


def _checked_ranks(coll, p, cnts, root):
    """(rank, elements) whose recv buffer the collective defines."""
    if coll == "red":
        return [(root, None)]
    if coll == "rs":
        return [(r, cnts[r]) for r in range(p) if cnts[r]]
    return [(r, None) for r in range(p)]


def _plans(mvx, coll, p, n, cnts, dtype, op, root):
    return [mvx.plan(_coll_id(mvx, coll), p, r, 0 if coll == "rs" else n, dtype, op, root,
                     cnts if coll == "rs" else None) for r in range(p)]


def _reference(mvx, coll, p, S, n, cnts, dtype, op, root):
    e = A.ESIZE[dtype]
    return A.run_plans(_plans(mvx, coll, p, n, cnts, dtype, op, root), S,
                       [np.full(s * e, 0x5C, np.uint8) for s in _sizes(coll, p, n, cnts)])


def test_counts_lie_on_either_side_of_an_algorithm_switch(mvx):
    for cid in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE):
        for dtype in fp8_ref.TYPES:
            for p in (8, 12):
                assert mvx.algorithm(cid, p, 4096, dtype) != mvx.algorithm(cid, p, 8192, dtype)


@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("dtype", A.TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("p", PS)
def test_collectives_match_the_plans_evaluated_in_f32(mvx, comms, p, dtype, coll):
    """Allreduce, Reduce at several roots, Reduce_scatter and Scan, both ops:
    the device == acc32_ref's evaluation of each rank's plan, and the bytes
    past the result keep their pattern."""
    e = A.ESIZE[dtype]
    nan = {op: [0, 0] for op in A.OPS}
    for n in COUNTS:
        cnts = _split(n, p)
        S = [A.coll_vec(dtype, n, 1000 * p + 17 * r + n) for r in range(p)]
        dS = [T.to_dev(s) for s in S]
        for op in A.OPS:
            for root in _roots(coll, p):
                ref = _reference(mvx, coll, p, S, n, cnts, dtype, op, root)
                got, rcs = _device(comms[p], coll, p, dS, n, cnts, dtype, op, root)
                assert rcs == [0] * p
                for r, cnt in _checked_ranks(coll, p, cnts, root):
                    nb = (cnt if cnt is not None else n) * e
                    A.assert_same(op, dtype, got[r][:nb], ref[r][:nb], (coll, p, n, op, root, r))
                    assert np.array_equal(got[r][nb:], ref[r][nb:])
                    nan[op][0] += int(A.isnan(dtype, ref[r][:nb]).sum())
                    nan[op][1] += nb // e
    for op, (bad, total) in nan.items():
        assert bad < NAN_CAP * total, ("NaN-exempt share of the reference results", op, bad, total)


def _oracle_float(oracle, coll, F, n, cnts, op, root):
    """The oracle's MPI_FLOAT collective over float32 sends: per-rank results."""
    p = len(F)
    R = [np.zeros(s, np.float32) for s in _sizes(coll, p, n, cnts)]
    S8, R8 = [f.view(np.uint8) for f in F], [r.view(np.uint8) for r in R]
    if coll == "ar":
        rc = oracle.allreduce(S8, R8, n, MPI_FLOAT, op)
    elif coll == "red":
        rc = oracle.reduce(S8, R8, n, MPI_FLOAT, op, root)
    elif coll == "rs":
        rc = oracle.reduce_scatter(S8, R8, cnts, MPI_FLOAT, op)
    else:
        rc = oracle.scan(S8, R8, n, MPI_FLOAT, op)
    assert rc == [0] * p
    return R


@pytest.mark.parametrize("dtype", A.TYPES, ids=TYPE_IDS)
@pytest.mark.parametrize("p", PS)
def test_device_equals_the_reference_float_collective_narrowed(mvx, oracle, comms, p, dtype):
    """The device result == narrow(the oracle's MPI_FLOAT SUM / PROD collective
    on the widened sends), where both run the same algorithm (asserted): the
    combine order and roles are the reference's, not merely this project's
    plans'."""
    e = A.ESIZE[dtype]
    for coll in COLLS:
        for n in PIN_COUNTS:
            cid = _coll_id(mvx, coll)
            assert mvx.algorithm(cid, p, n, dtype) == mvx.algorithm(cid, p, n, MPI_FLOAT)
            if coll != "scan":
                assert mvx.algorithm(cid, p, n, dtype) == oracle.algorithm(cid, p, n, MPI_FLOAT)
            cnts = _split(n, p)
            S = [A.coll_vec(dtype, n, 77 * p + 5 * r + n) for r in range(p)]
            F = [A.widen(dtype, s) for s in S]
            dS = [T.to_dev(s) for s in S]
            for op in A.OPS:
                for root in (range(p) if coll == "red" else [0]):
                    got, rcs = _device(comms[p], coll, p, dS, n, cnts, dtype, op, root)
                    assert rcs == [0] * p
                    R = _oracle_float(oracle, coll, F, n, cnts, A.BASE[op], root)
                    for r, cnt in _checked_ranks(coll, p, cnts, root):
                        m = cnt if cnt is not None else n
                        A.assert_same(op, dtype, got[r][:m * e], A.round_to(dtype, R[r][:m]), (coll, p, n, op, root, r))


# ------------------------------------------------ programs over more than 8 leaves

# per collective: a count below p (single elements), ragged ones, and one
# inside the long-message algorithms.  p = 9 and 33 leave a group of 8 with a
# single trailing leaf (9 = 8 + 1, 33 = 4 * 8 + 1) and fold a non-power-of-two
# remainder (9 - 8, 33 - 32); p = 16 is the plain two-round tree.
WIDE_RUNS = (("ar", 7), ("ar", 20001), ("red", 9), ("red", 20001), ("rs", 3), ("rs", 9000), ("scan", 301))


@pytest.mark.parametrize("p", [9, 16, 33])
@pytest.mark.parametrize("dtype", A.TYPES, ids=TYPE_IDS)
def test_wide_communicators_keep_f32_between_the_launches(mvx, wide, p, dtype):
    """Combines of more than 8 leaves: groups of <= 8-leaf launches whose
    intermediates are f32 temporaries.  The device == acc32_ref, which
    evaluates the whole plan at once; for E4M3 SUM also == the float64 sum
    rounded once."""
    e = A.ESIZE[dtype]
    seen_wide = False
    nan = {op: [0, 0] for op in A.OPS}
    for coll, n0 in WIDE_RUNS:
        cnts = [n0 + (r % 2) for r in range(p)] if coll == "rs" else None
        n = sum(cnts) if cnts else n0
        S = [A.coll_vec(dtype, n, 31 * p + r + n, special=0.002) for r in range(p)]
        dS = [T.to_dev(s) for s in S]
        for op in A.OPS:
            for root in ([0, p - 1] if coll == "red" else [0]):
                plans = _plans(mvx, coll, p, n, cnts, dtype, op, root)
                seen_wide |= any(P.k > 8 for P in plans)
                ref = _reference(mvx, coll, p, S, n, cnts, dtype, op, root)
                got, rcs = _device(wide[p], coll, p, dS, n, cnts, dtype, op, root)
                assert rcs == [0] * p, (coll, p, n, op, rcs)
                for r, cnt in _checked_ranks(coll, p, cnts, root):
                    nb = (cnt if cnt is not None else n) * e
                    A.assert_same(op, dtype, got[r][:nb], ref[r][:nb], (coll, p, n, op, root, r))
                    assert np.array_equal(got[r][nb:], ref[r][nb:])
                    nan[op][0] += int(A.isnan(dtype, ref[r][:nb]).sum())
                    nan[op][1] += nb // e
                if dtype == fp8_ref.E4M3 and op == 164 and coll in ("ar", "red"):
                    exact = fp8_ref.widen(dtype, S[0])
                    for s in S[1:]:
                        exact = exact + fp8_ref.widen(dtype, s)
                    A.assert_same(op, dtype, got[root][:n], fp8_ref.encode(dtype, exact), ("float64 sum", coll, p, n))
    assert seen_wide
    for op, (bad, total) in nan.items():
        assert bad < NAN_CAP * total, ("NaN-exempt share of the reference results", op, bad, total)


# ------------------------------------------------------- host buffers, errors

@pytest.mark.parametrize("dtype", A.TYPES, ids=TYPE_IDS)
def test_host_buffers_pageable_and_pinned(mvx, comms, dtype):
    import torch
    p, n = 3, 5000
    e = A.ESIZE[dtype]
    S = [A.coll_vec(dtype, n, 3 * r + 1) for r in range(p)]
    for op in A.OPS:
        ref = _reference(mvx, "ar", p, S, n, None, dtype, op, 0)
        for pinned in (False, True):
            if pinned:
                sends = [torch.from_numpy(s.copy()).pin_memory() for s in S]
                recvs = [torch.zeros(n * e, dtype=torch.uint8).pin_memory() for _ in range(p)]
            else:
                sends = [s.copy() for s in S]
                recvs = [np.zeros(n * e, np.uint8) for _ in range(p)]
            r, rcs = comms[p].allreduce_multi(sends, recvs, n, dtype, op)
            assert r == 0 and rcs == [0] * p
            for q in range(p):
                got = recvs[q].numpy() if pinned else recvs[q]
                A.assert_same(op, dtype, got, ref[q], ("allreduce", op, pinned, q))


def test_blocking_calls_on_host_and_device_buffers(mvx):
    """MPI_Allreduce / MPI_Reduce / MPI_Scan / MPI_Reduce_scatter themselves
    (the RCCL communicator path, one rank) take the handles."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29534")
    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
    comm = mvx.Comm.from_torch_distributed(0)
    try:
        for dtype in A.TYPES:
            n = 10001
            e = A.ESIZE[dtype]
            a = A.coll_vec(dtype, n, 7)
            for op in A.OPS:
                out = np.zeros(n * e, np.uint8)
                assert mvx.MPI_Allreduce(a, out, n, dtype, op, comm) == 0
                assert np.array_equal(out, a)
                da = torch.from_numpy(a.copy()).cuda()
                db = torch.zeros_like(da)
                assert mvx.MPI_Allreduce(da, db, n, dtype, op, comm) == 0
                assert np.array_equal(db.cpu().numpy(), a)
                for call in (lambda o: mvx.MPI_Reduce(a, o, n, dtype, op, 0, comm),
                             lambda o: mvx.MPI_Scan(a, o, n, dtype, op, comm),
                             lambda o: mvx.MPI_Reduce_scatter(a, o, [n], dtype, op, comm)):
                    out = np.zeros(n * e, np.uint8)
                    assert call(out) == 0
                    assert np.array_equal(out, a)
                assert mvx.MPI_Allreduce(a, out, n // 4, MPI_FLOAT, op, comm) == 0      # p = 1 never calls the op
        for bad in (163, 166):
            assert mvx.error_class(mvx.MPI_Allreduce(a, out, 4, fp8_ref.E4M3, bad, comm)) == 9
    finally:
        comm.free()


def test_undefined_pairs_answer_329_like_band_on_float(mvx, comms):
    """MVX_SUM_ACC32 on MPI_FLOAT, MPI_INT and a vector of E5M2: 329 from the
    ranks that answer it for MPI_BAND on MPI_FLOAT, the sends untouched; at
    p = 1 and at count 0 nobody calls the op."""
    import torch
    rc, vt = mvx.MPI_Type_vector(3, 1, 2, fp8_ref.E5M2)
    assert rc == 0 and mvx.MPI_Type_commit(vt) == 0
    try:
        for p in (4, 7):
            S = [np.random.default_rng(r).integers(0, 256, 64 * 5).astype(np.uint8) for r in range(p)]
            dS = [T.to_dev(s) for s in S]

            def run(dtype, op, cnt=16):
                y = [torch.full((64 * 5,), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(p)]
                return [comms[p].allreduce_multi(dS, y, cnt, dtype, op),
                        comms[p].reduce_multi(dS, y, cnt, dtype, op, 1),
                        comms[p].reduce_scatter_multi(dS, y, [cnt // 4] * p, dtype, op),
                        comms[p].scan_multi(dS, y, cnt, dtype, op)]
            band = run(MPI_FLOAT, 105)
            assert any(329 in rcs for _, rcs in band)
            for op in A.OPS:
                for dtype in (MPI_FLOAT, MPI_INT):
                    assert run(dtype, op) == band, (p, op, dtype)
                # the derived type: the ranks that report MPI_BAND on it
                assert run(vt, op) == run(vt, 105), (p, op)
                assert comms[p].allreduce_multi(dS, dS, 0, MPI_FLOAT, op) == (0, [0] * p)
            for q in range(p):
                assert np.array_equal(T.from_dev(dS[q]), S[q])
        a = T.to_dev(np.zeros(64, np.uint8))
        y = torch.zeros(64, dtype=torch.uint8, device="cuda")
        for op in A.OPS:
            assert comms[1].allreduce_multi([a], [y], 16, MPI_FLOAT, op) == (0, [0])
    finally:
        assert mvx.MPI_Type_free(vt)[0] == 0
