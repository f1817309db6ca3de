"""GPU: the collectives on the extension datatypes MVX_FLOAT8_E4M3 /
MVX_FLOAT8_E5M2.

Virtual communicators (p ranks' buffers on one GPU) run every rank's plan on
the device.  Two references:

* tests/fp8_ref.py evaluates the same plans with its own op -- every op,
  every rounding step in the plan's order;
* for the ops without rounding (MAX, MIN, LAND, LOR, LXOR) the reference
  itself: the inputs widened exactly to float, the oracle's MPI_FLOAT
  collective (oracle/coll_sim.c replays the reference's schedule), the
  result located by value and compared by the chosen operand's bits.  That
  pins operand roles (NaN, +-0) to the reference rather than to this
  project's plans.

And the paths around the op kernels: user ops (the function receives the
handle), a derived type with holes, host buffers, the undefined ops.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import fp8_ref as H
import mvxtest as T

pytestmark = pytest.mark.gpu

MPI_UNSIGNED_CHAR = 2
PS = [1, 2, 3, 4, 5, 6, 7, 8, 12]
# below p, a ragged few hundred, one on each side of the switch at which
# Allreduce and Reduce leave recursive doubling / the binomial tree at p >= 8
# (8192 and 4097 bytes), and a size well inside the long-message algorithms
COUNTS = [1, 5, 333, 4096, 8192, 40000]
PIN_COUNTS = [1, 5, 300]
PIN_OPS = (100, 101, 104, 106, 108)
NAN_CAP = 0.10
COLLS = ["ar", "red", "rs", "scan"]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def comms(mvx):
    cs = {p: mvx.Comm.local_ranks(p, 0) for p in PS}
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


def _device(comm, coll, p, dsends, n, cnts, dtype, op, root):
    """One collective on the device: (per-rank recv bytes, per-rank codes)."""
    import torch
    sizes = [max(c, 1) for c in cnts] if coll == "rs" else [n] * p
    drs = [torch.full((s,), 0x5C, dtype=torch.uint8, device="cuda") for s in sizes]
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


def test_counts_lie_on_either_side_of_an_algorithm_switch(mvx):
    for cid in (mvx.COLL_ALLREDUCE, mvx.COLL_REDUCE):
        for dtype in H.TYPES:
            for p in (8, 12):
                assert mvx.algorithm(cid, p, 4096, dtype) != mvx.algorithm(cid, p, 8192, dtype)


@pytest.mark.parametrize("coll", COLLS)
@pytest.mark.parametrize("dtype", H.TYPES, ids=[H.NAMES[d] for d in H.TYPES])
@pytest.mark.parametrize("p", PS)
def test_collectives_match_the_plans_evaluated_by_the_reference_op(mvx, comms, p, dtype, coll):
    """Allreduce, Reduce at several roots, Reduce_scatter and Scan, all seven
    ops: the device == fp8_ref's evaluation of each rank's plan."""
    nan = {102: [0, 0], 103: [0, 0]}
    for n in COUNTS:
        cnts = _split(n, p)
        S = [H.coll_vec(dtype, n, 1000 * p + 17 * r + n) for r in range(p)]
        dS = [T.to_dev(s) for s in S]
        for op in H.OPS:
            for root in _roots(coll, p):
                got, rcs = _device(comms[p], coll, p, dS, n, cnts, dtype, op, root)
                assert rcs == [0] * p
                plans = [mvx.plan(_coll_id(mvx, coll), p, r, 0 if coll == "rs" else n, dtype, op, root,
                                  cnts if coll == "rs" else None) for r in range(p)]
                sizes = [max(c, 1) for c in cnts] if coll == "rs" else [n] * p
                ref = H.run_plans(plans, S, [np.full(s, 0x5C, np.uint8) for s in sizes])
                for r, cnt in _checked_ranks(coll, p, cnts, root):
                    nb = cnt if cnt is not None else n
                    H.assert_same(op, dtype, got[r][:nb], ref[r][:nb], (coll, p, n, op, root, r))
                    assert np.array_equal(got[r][nb:], ref[r][nb:])
                    if op in nan:
                        nan[op][0] += int(H.isnan(dtype, ref[r][:nb]).sum())
                        nan[op][1] += nb
    for op, (bad, total) in nan.items():
        assert bad < NAN_CAP * total, ("NaN-exempt share of the reference results", op, bad, total)


def _oracle_float(oracle, coll, F, n, cnts, op, root):
    """The oracle's MPI_FLOAT collective over float32 sends: per-rank results."""
    p = len(F)
    sizes = [max(c, 1) for c in cnts] if coll == "rs" else [n] * p
    R = [np.zeros(s, np.float32) for s in sizes]
    S8, R8 = [f.view(np.uint8) for f in F], [r.view(np.uint8) for r in R]
    if coll == "ar":
        rc = oracle.allreduce(S8, R8, n, 10, op)
    elif coll == "red":
        rc = oracle.reduce(S8, R8, n, 10, op, root)
    elif coll == "rs":
        rc = oracle.reduce_scatter(S8, R8, cnts, 10, op)
    else:
        rc = oracle.scan(S8, R8, n, 10, op)
    assert rc == [0] * p
    return R


@pytest.mark.parametrize("dtype", H.TYPES, ids=[H.NAMES[d] for d in H.TYPES])
@pytest.mark.parametrize("p", PS)
def test_roles_match_the_reference_float_collective(mvx, oracle, comms, p, dtype):
    """MAX, MIN and the logical ops never round, so the result on an 8-bit
    float is the narrowed result of the same collective on the widened
    inputs -- provided both run the same algorithm, which these counts do
    (asserted).  One element in three is a NaN, a zero of either sign, an
    extreme value or 1, so operand roles decide many results.  Every NaN of
    the inputs is the one pattern narrow() gives, so the comparison is by
    bits."""
    for coll in COLLS:
        for n in PIN_COUNTS:
            cid = _coll_id(mvx, coll)
            assert mvx.algorithm(cid, p, n, dtype) == mvx.algorithm(cid, p, n, 10)
            if coll != "scan":
                assert mvx.algorithm(cid, p, n, dtype) == oracle.algorithm(cid, p, n, 10)
            cnts = _split(n, p)
            S = [H.coll_vec(dtype, n, 77 * p + 5 * r + n, special=0.33) for r in range(p)]
            F = [H.widen(dtype, s).astype(np.float32) for s in S]
            dS = [T.to_dev(s) for s in S]
            for op in PIN_OPS:
                for root in (range(p) if coll == "red" else [0]):
                    got, rcs = _device(comms[p], coll, p, dS, n, cnts, dtype, op, root)
                    assert rcs == [0] * p
                    R = _oracle_float(oracle, coll, F, n, cnts, op, root)
                    for r, cnt in _checked_ranks(coll, p, cnts, root):
                        m = cnt if cnt is not None else n
                        want = H.narrow(dtype, R[r][:m])
                        assert np.array_equal(got[r][:m], want), (coll, p, n, op, root, r)


# ---------------------------------------------------------------- user ops

_dev = None


def _dev_fn(name):
    """Address of a device function of tests/fp8_user_ops_dev.hip (hipcc for
    gfx950, built once per session)."""
    global _dev
    if _dev is None:
        so = os.path.join(tempfile.mkdtemp(prefix="mvx_fp8_duops_"), "libfp8duops.so")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                               os.path.join(HERE, "fp8_user_ops_dev.hip"), "-o", so])
        _dev = ctypes.CDLL(so)
    return ctypes.cast(getattr(_dev, name), ctypes.c_void_p).value


@pytest.mark.parametrize("where", ["device", "host"])
def test_user_ops_on_e4m3_receive_the_handle(mvx, comms, where):
    """A device-function op and a host MPI_User_function (MPI_Op_create) on
    MVX_FLOAT8_E4M3: the larger byte (order-free, so the expected result is
    numpy's maximum over the ranks); the function must be handed datatype
    72."""
    seen = []

    def host_bitmax(invec, inoutvec, len_ptr, type_ptr):
        n = len_ptr[0]
        seen.append(type_ptr[0])
        a = np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(invec))
        b = np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(inoutvec))
        np.maximum(a, b, out=b)

    if where == "device":
        rc, uop = mvx.op_create_device(_dev_fn("duop_e4m3_bitmax"), 1)
    else:
        rc, uop = mvx.MPI_Op_create(host_bitmax, 1)
    assert rc == 0
    try:
        for p in (2, 3, 8):
            for n in (5, 2049):
                cnts = _split(n, p)
                S = [H.rand_bits(H.E4M3, n, 31 * p + r + n, special=0.5) for r in range(p)]
                dS = [T.to_dev(s) for s in S]
                full = np.maximum.reduce(S)
                for coll in COLLS:
                    got, rcs = _device(comms[p], coll, p, dS, n, cnts, H.E4M3, uop, p - 1)
                    assert rcs == [0] * p, (coll, p, n, rcs)
                    off = np.cumsum([0] + cnts)
                    for r, cnt in _checked_ranks(coll, p, cnts, p - 1):
                        if coll == "rs":
                            want = full[off[r]:off[r] + cnt]
                        elif coll == "scan":
                            want = np.maximum.reduce(S[:r + 1])
                        else:
                            want = full
                        assert np.array_equal(got[r][:want.size], want), (coll, p, n, r)
        assert where == "device" or (seen and set(seen) == {H.E4M3})
    finally:
        assert mvx.MPI_Op_free(uop)[0] == 0


def test_user_op_on_a_vector_of_e5m2_keeps_the_holes(mvx, comms):
    """vector(3, 1, 2, MVX_FLOAT8_E5M2): extent 5, size 3, holes at bytes 1
    and 3.  The type moves packed and the op sees the extent layout; the
    holes of every recv buffer keep the caller's bytes."""
    import torch
    rc, vt = mvx.MPI_Type_vector(3, 1, 2, H.E5M2)
    assert rc == 0 and mvx.MPI_Type_commit(vt) == 0
    assert mvx.MPI_Type_extent(vt) == (0, 5) and mvx.MPI_Type_size(vt) == (0, 3)
    rc, uop = mvx.op_create_device(_dev_fn("duop_vec3_bytemax"), 1)
    assert rc == 0
    rc, vs = mvx.MPI_Type_vector(3, 1, 2, MPI_UNSIGNED_CHAR)
    assert rc == 0 and mvx.MPI_Type_commit(vs) == 0
    try:
        for p in (2, 4, 7):
            for n in (1, 333):
                S = [np.random.default_rng(p + 9 * r + n).integers(0, 256, 5 * n).astype(np.uint8)
                     for r in range(p)]
                drs = [torch.full((5 * n,), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(p)]
                r, rcs = comms[p].allreduce_multi([T.to_dev(s) for s in S], drs, n, vt, uop)
                assert r == 0 and rcs == [0] * p
                want = np.maximum.reduce(S).reshape(n, 5)
                want[:, 1] = want[:, 3] = 0x5C
                for q in range(p):
                    assert np.array_equal(T.from_dev(drs[q]).reshape(n, 5), want), (p, n, q)
                # no predefined op on the derived type: 329 from the ranks that
                # report it for the same vector of MPI_UNSIGNED_CHAR
                r, rcs = comms[p].allreduce_multi([T.to_dev(s) for s in S], drs, n, vt, 102)
                r2, rcs2 = comms[p].allreduce_multi([T.to_dev(s) for s in S], drs, n, vs, 102)
                assert r == r2 == 0 and rcs == rcs2 and set(rcs) <= {0, 329} and 329 in rcs
    finally:
        assert mvx.MPI_Op_free(uop)[0] == 0
        assert mvx.MPI_Type_free(vt)[0] == 0
        assert mvx.MPI_Type_free(vs)[0] == 0


# ------------------------------------------------------- host buffers, errors

@pytest.mark.parametrize("dtype", H.TYPES, ids=[H.NAMES[d] for d in H.TYPES])
def test_host_buffers_pageable_and_pinned(mvx, comms, dtype):
    """Host operands through the collectives and through MPIR_SUM itself
    (the predefined op as an MPI_User_function, mvx_hostop.c)."""
    import torch
    p, n = 3, 5000
    S = [H.coll_vec(dtype, n, 3 * r + 1) for r in range(p)]
    plans = [mvx.plan(mvx.COLL_ALLREDUCE, p, r, n, dtype, 102) for r in range(p)]
    ref = H.run_plans(plans, S, [np.zeros(n, np.uint8) for _ in range(p)])
    for pinned in (False, True):
        if pinned:
            sends = [torch.from_numpy(s.copy()).pin_memory() for s in S]
            recvs = [torch.zeros(n, dtype=torch.uint8).pin_memory() for _ in range(p)]
        else:
            sends = [s.copy() for s in S]
            recvs = [np.zeros(n, np.uint8) for _ in range(p)]
        r, rcs = comms[p].allreduce_multi(sends, recvs, n, dtype, 102)
        assert r == 0 and rcs == [0] * p
        for q in range(p):
            got = recvs[q].numpy() if pinned else recvs[q]
            H.assert_same(102, dtype, got, ref[q], ("allreduce", pinned, q))
        # MPIR_SUM(in, inout): inout = in + inout
        a, b = H.coll_vec(dtype, n, 40), H.coll_vec(dtype, n, 41)
        want = H.op(102, dtype, a, b)
        if pinned:
            ha, hb = torch.from_numpy(a.copy()).pin_memory(), torch.from_numpy(b.copy()).pin_memory()
        else:
            ha, hb = a.copy(), b.copy()
        mvx.MPIR_call("MPIR_SUM", ha, hb, n, dtype)
        assert mvx.op_errno() == 0
        H.assert_same(102, dtype, hb.numpy() if pinned else hb, want, ("MPIR_SUM", pinned))
        assert np.array_equal(ha.numpy() if pinned else ha, a)
    # an undefined op through the same entry: 329 in MPIR_Op_errno, inout untouched
    a, b = H.coll_vec(dtype, 64, 1), H.coll_vec(dtype, 64, 2)
    hb = b.copy()
    mvx.MPIR_call("MPIR_BAND", a.copy(), hb, 64, dtype)
    assert mvx.op_errno() == 329 and np.array_equal(hb, b)


def test_blocking_allreduce_on_host_and_device_buffers(mvx):
    """MPI_Allreduce itself (the RCCL communicator path, one rank) takes the
    handles: host and device buffers, and the undefined op at p = 1."""
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    if not dist.is_initialized():
        dist.init_process_group("gloo", rank=0, world_size=1)
    comm = mvx.Comm.from_torch_distributed(0)
    try:
        for dtype in H.TYPES:
            n = 10001
            a = H.coll_vec(dtype, n, 7)
            out = np.zeros(n, np.uint8)
            assert mvx.MPI_Allreduce(a, out, n, dtype, 102, comm) == 0
            assert np.array_equal(out, a)
            da = torch.from_numpy(a.copy()).cuda()
            db = torch.zeros_like(da)
            assert mvx.MPI_Allreduce(da, db, n, dtype, 100, comm) == 0
            assert np.array_equal(db.cpu().numpy(), a)
            assert mvx.MPI_Allreduce(da, db, n, dtype, 105, comm) == 0      # p = 1 never calls the op
            assert mvx.MPI_Reduce(a, out, n, dtype, 103, 0, comm) == 0
            assert mvx.MPI_Scan(a, out, n, dtype, 108, comm) == 0
            assert mvx.MPI_Reduce_scatter(a, out, [n], dtype, 104, comm) == 0
    finally:
        comm.free()


def test_undefined_ops_answer_329_on_every_rank(mvx, comms):
    import torch
    for dtype in H.TYPES:
        S = [H.coll_vec(dtype, 64, r) for r in range(4)]
        dS = [T.to_dev(s) for s in S]
        for op in H.UNDEFINED_OPS:
            y = [torch.full((64,), 0x5C, dtype=torch.uint8, device="cuda") for _ in range(4)]
            assert comms[4].allreduce_multi(dS, y, 64, dtype, op) == (0, [329] * 4)
            assert comms[4].reduce_scatter_multi(dS, y, [16] * 4, dtype, op) == (0, [329] * 4)
            r, rcs = comms[4].reduce_multi(dS, y, 64, dtype, op, 0)
            assert r == 0 and rcs[0] == 329
            assert comms[1].allreduce_multi(dS[:1], y[:1], 64, dtype, op) == (0, [0])     # p = 1: no op call
            assert comms[4].allreduce_multi(dS, y, 0, dtype, op) == (0, [0] * 4)
        for q in range(4):
            assert np.array_equal(T.from_dev(dS[q]), S[q])
