"""TEST HELPER: the seeded sweep of the four narrow floating types
(MVX_FLOAT16, MVX_BFLOAT16, MVX_FLOAT8_E4M3, MVX_FLOAT8_E5M2) and of
MVX_SUM_ACC32 / MVX_PROD_ACC32 over every executor path -- the case list, its
CPU references and the GPU runner.  tests/test_cpu_narrow_sweep.py checks the
list and the references against each other; tests/test_gpu_z_narrow_sweep.py
runs the same list on the device.

A case is one collective on a virtual communicator: p from 1 to 64, the p2p
or the pipelined exchange (2-6 slices), either device flavour, every send and
recv buffer device, pageable or page-locked and shifted 0-15 elements into an
allocation whose other bytes are guards, an op that is defined, undefined
(329 from the ranks that call it) or no op at all (class 9).

References, none of them taken from the device:

R1  each rank's mvx.plan evaluated by half_ref / fp8_ref / acc32_ref;
R2  the oracle's replay of the reference schedule (oracle/coll_sim.c), which
    knows nothing of this project's plans -- MAX / MIN / LAND / LOR / LXOR:
    the MPI_FLOAT collective on the widened sends, narrowed; the ACC32 ops:
    MPI_FLOAT SUM / PROD on the widened sends, rounded once; SUM / PROD with
    per-step rounding: a user op (a Python callback around half_ref.op_u8 /
    fp8_ref.op_u8) on the unsigned carrier type of the same size.  It applies
    where both sides take the same algorithm, decided from mvx.algorithm and
    oracle.algorithm (applies());
R3  E4M3 with MVX_SUM_ACC32 on Allreduce / Reduce: the float64 sum of the
    widened sends, encoded once.

An undefined op's return codes and moved bytes are the oracle's for MPI_MINLOC
on the carrier type, which no rank's (*uop) call defines either: the same
element size, so the same algorithm at every count, and the calls leave their
inout operand alone.  Where MPI_FLOAT takes that algorithm too, the codes must
also be those of the same op on MPI_FLOAT.
"""
import ctypes
import os

import numpy as np

import acc32_ref as A
import fp8_ref
import half_ref

N_CASES = int(os.environ.get("MVX_FUZZ_NARROW_CASES", "320"))
N_DEFAULT = 320
SEED = int(os.environ.get("MVX_FUZZ_NARROW_SEED", "20261127"))
BATCH = 40
TYPES = A.TYPES                                     # 64, 65, 72, 73
ESIZE = A.ESIZE
PS = [1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 31, 32, 33, 63, 64]
DEFINED = half_ref.OPS                              # the seven ops of MPI_FLOAT
ROUNDING = (102, 103)                               # SUM / PROD: every step rounds
PIN_OPS = (100, 101, 104, 106, 108)                 # never round
ACC = A.OPS                                         # 164, 165
UNDEFINED = half_ref.UNDEFINED_OPS
INVALID = (163, 166)
# the ops that round carry most of the weight: theirs are the bits that move
_OPS = PIN_OPS + ROUNDING + ACC + UNDEFINED + INVALID
_W = [1.0] * 5 + [2.5] * 2 + [3.0] * 2 + [0.2] * 5 + [0.2] * 2
OP_WEIGHTS = np.array(_W) / sum(_W)
MPI_FLOAT, MPI_MINLOC = 10, 110
CARRIER = {1: 2, 2: 5}                              # MPI_UNSIGNED_CHAR, MPI_UNSIGNED_SHORT
USER_OP = 250                                       # the oracle's handle of the callback
GUARD = 0x5C
TAIL = 16                                           # guard bytes past every recv buffer
WIDE_MAX = 20001                                    # elements a rank holds at p >= 17
SLICE = 256                                         # elements: PIPE's slice granule (mvx_exec.c)


def _ref(dtype, op=102):
    if op in ACC:
        return A
    return half_ref if dtype in half_ref.TYPES else fp8_ref


def _case(rng, i):
    dtype = TYPES[i % len(TYPES)]
    p = int(rng.choice(PS))
    coll = str(rng.choice(["ar", "ar", "red", "rs", "scan"]))
    op = int(rng.choice(_OPS, p=OP_WEIGHTS))
    r = rng.random()
    if r < 0.06:
        n = 0
    elif r < 0.40:
        n = int(rng.integers(1, 301))
    elif r < 0.92:
        n = int(np.exp2(rng.uniform(8, 15)))
    else:
        n = int(np.exp2(rng.uniform(15, 17)))
    if p >= 17:
        n = min(n, WIDE_MAX)
    cnts = None
    if coll == "rs":
        if p >= 17:
            n = min(n, WIDE_MAX - 3 * p)
        base = n // p
        cnts = [int(max(0, base + rng.integers(-3, 4))) if rng.random() < 0.8 else 0 for _ in range(p)]
    exch = "pipe" if rng.random() < 0.55 else "p2p"
    slices = int(rng.integers(2, 7))
    smp = bool(rng.random() < 0.3)
    # PIPE (and the residue of a wide ACC32 combine's own leaf) needs a call
    # whose buffers are all in HBM, which independent draws give to few calls
    # of many ranks: a share of the cases draws "dev" for every buffer, the
    # larger the more leaves the call combines
    if rng.random() < (0.4 if p < 9 else 0.8 if op in ACC else 0.6):
        kinds = ["dev"] * (2 * p)
    else:
        kinds = [str(rng.choice(["dev", "dev", "host", "pin"])) for _ in range(2 * p)]
    shift = [int(rng.integers(1, 16)) if rng.random() < 0.5 else 0 for _ in range(2 * p)]
    return dict(id="sweep-%d" % i, p=p, coll=coll, dtype=dtype, op=op, n=n, cnts=cnts, exch=exch, slices=slices,
                smp=smp, kinds=kinds, shift=shift, root=int(rng.integers(0, p)), seed=int(rng.integers(1 << 30)))


def cases(n=None):
    """The first n cases of the list (a longer list keeps the shorter one)."""
    rng = np.random.default_rng(SEED)
    return [_case(rng, i) for i in range(N_CASES if n is None else n)]


def fixed_acc32_edge(dtype):
    """MVX_SUM_ACC32 over more than 8 leaves with the send buffer 1, 2 and 3
    elements into its allocation (the 2-byte types: 1), the recv buffer
    shifted otherwise, p2p and pipe with 3 slices."""
    out = []
    for p in (9, 33):
        for coll in ("ar", "rs"):
            for s in ((1, 2, 3) if ESIZE[dtype] == 1 else (1,)):
                for exch in ("p2p", "pipe"):
                    cnts = [9000 + r % 2 for r in range(p)] if coll == "rs" else None
                    out.append(dict(id="acc32-edge-%d-p%d-%s-s%d-%s" % (dtype, p, coll, s, exch), p=p, coll=coll,
                                    dtype=dtype, op=164, n=WIDE_MAX, cnts=cnts, exch=exch, slices=3, smp=False,
                                    kinds=["dev"] * (2 * p), shift=[s, (s + 5) % 16] * p, root=0,
                                    seed=7000 + 100 * p + s))
    return out


def fixed_wide_sum(dtype):
    """SUM with per-step rounding at p = 17 and 64, unshifted, p2p."""
    out = []
    for p in (17, 64):
        for coll in ("ar", "red", "rs"):
            for n in (7, WIDE_MAX):
                cnts = [n // p + (1 if r < n % p else 0) for r in range(p)] if coll == "rs" else None
                out.append(dict(id="wide-sum-%d-p%d-%s-%d" % (dtype, p, coll, n), p=p, coll=coll, dtype=dtype, op=102,
                                n=n, cnts=cnts, exch="p2p", slices=2, smp=False, kinds=["dev"] * (2 * p),
                                shift=[0] * (2 * p), root=p - 1, seed=9000 + p + n))
    return out


def fixed_e4m3_exact():
    """E4M3 with MVX_SUM_ACC32 on Allreduce and Reduce at every p of the
    sweep, where the float64 sum encoded once (R3) is the whole truth: count
    7 from the types' usual inputs, p2p, and count 700 over the format's full
    finite range (inputs()), shifted, pipe with 3 slices (a span of 700
    crosses two 256-element slices)."""
    out = []
    for p in PS:
        for coll in ("ar", "red"):
            out.append(dict(id="e4m3-exact-p%d-%s-7" % (p, coll), p=p, coll=coll, dtype=fp8_ref.E4M3, op=164, n=7,
                            cnts=None, exch="p2p", slices=2, smp=False, kinds=["dev"] * (2 * p),
                            shift=[0] * (2 * p), root=p - 1, seed=11000 + p))
            out.append(dict(id="e4m3-exact-p%d-%s-700" % (p, coll), p=p, coll=coll, dtype=fp8_ref.E4M3, op=164,
                            n=700, cnts=None, exch="pipe", slices=3, smp=False, kinds=["dev"] * (2 * p),
                            shift=[1, 2] * p, root=p // 2, seed=12000 + p, full=True))
    return out


# ------------------------------------------------------------- what a case is

class Derived:
    pass


def derive(mvx, c):
    """Everything about a case that follows from the planner alone."""
    d = Derived()
    p, coll, dtype, op = c["p"], c["coll"], c["dtype"], c["op"]
    d.E = ESIZE[dtype]
    d.cid = {"ar": mvx.COLL_ALLREDUCE, "red": mvx.COLL_REDUCE, "rs": mvx.COLL_REDUCE_SCATTER,
             "scan": mvx.COLL_SCAN}[coll]
    d.tun = mvx.smp_tuning() if c["smp"] else mvx.tuning_from_env(smp=False)
    d.tot = sum(c["cnts"]) if c["cnts"] else c["n"]
    d.rcount = [(c["cnts"][q] if c["cnts"] else c["n"]) for q in range(p)]
    d.kind = ("invalid" if op in INVALID else "undefined" if op in UNDEFINED else "acc" if op in ACC else "defined")
    d.plans = None
    d.alg = mvx.algorithm(d.cid, p, d.tot, dtype, tuning=d.tun)
    if d.kind != "invalid":
        d.plans = [mvx.plan(d.cid, p, r, 0 if coll == "rs" else c["n"], dtype, op, c["root"], c["cnts"],
                            tuning=d.tun) for r in range(p)]
        assert d.plans[0].alg == d.alg
    # the bytes each buffer holds in the call (mvx_api.c call_sizes): an empty
    # buffer's kind is never asked
    d.nsend = [d.tot] * p
    d.nrecv = [0 if (coll == "red" and q != c["root"]) else d.rcount[q] for q in range(p)]
    d.all_dev = all(c["kinds"][2 * q] == "dev" or not d.nsend[q] for q in range(p)) and \
        all(c["kinds"][2 * q + 1] == "dev" or not d.nrecv[q] for q in range(p))
    # does the executor run?  not without an op, not for an empty plan, and an
    # undefined op moves nothing in Scan nor under the _SMP_ collops' pre-check
    d.runs = d.kind != "invalid" and d.alg != mvx.ALG_NONE
    if d.kind == "undefined" and (coll == "scan" or (c["smp"] and coll in ("ar", "red"))):
        d.runs = False
    d.span = 0
    if d.runs:
        for P in d.plans:
            s = P.c_cnt if P.has_combine else 0
            for q in range(p):
                s = max(s, P.a_send[q].cnt, P.a_recv[q].cnt, P.b_send[q].cnt, P.b_recv[q].cnt)
            d.span = max(d.span, s)
    d.pipe_eligible = bool(d.runs and c["exch"] == "pipe" and d.all_dev and d.span > SLICE)
    d.wide = bool(d.runs and op in ACC and any(P.has_combine and P.k > 8 for P in d.plans))
    # the residues mod 4 of the wide ranks' own leaf (mvx_exec.c exec_layout:
    # sendbuf + c_src_off), in calls that read the caller's buffers in place
    d.wide_residues = set()
    if d.wide and d.all_dev:
        for q, P in enumerate(d.plans):
            if P.has_combine and P.k > 8 and P.c_cnt:
                d.wide_residues.add(((c["shift"][2 * q] + P.c_src_off) * d.E) % 4)
    return d


_E4M3_FINITE = np.array([u for u in range(256) if u & 0x7f != 0x7f], np.uint8)


def _full_range_e4m3(c, d):
    """Sends over the whole finite range of E4M3, 2^-9 to 448 of either sign:
    partial sums of up to 63 x 448 next to addends of 2^-9 need all 24 bits of
    a float32 significand.  Element 0 is the sharpest such sum wherever it
    stays finite: +448 and -448 on equally many ranks, a zero if one is left
    over, and 2^-9 on the last rank -- 2^-9 exactly; element 1 has the 2^-9
    on rank 0 instead.  (Results beyond 448 are the format's NaN, by R3 too.)"""
    p = c["p"]
    S = [_E4M3_FINITE[np.random.default_rng(c["seed"] + q).integers(0, _E4M3_FINITE.size, d.tot)]
         for q in range(p)]
    if p >= 3 and d.tot >= 2:
        for e, tiny in ((0, p - 1), (1, 0)):
            others = [q for q in range(p) if q != tiny]
            half = len(others) // 2
            for i, q in enumerate(others):
                S[q][e] = 0x7E if i < half else 0xFE if i < 2 * half else 0x00
            S[tiny][e] = 0x01
    return S


def inputs(c, d):
    """Every rank's send vector, as bytes."""
    if c.get("full"):
        return _full_range_e4m3(c, d)
    special = 0.002 if c["p"] >= 17 else None
    return [A.coll_vec(c["dtype"], d.tot, c["seed"] + q, special) for q in range(c["p"])]


def checked(c, d):
    """(rank, elements) whose recv buffer the collective defines."""
    if c["coll"] == "red":
        return [(c["root"], c["n"])]
    return [(q, d.rcount[q]) for q in range(c["p"]) if d.rcount[q]]


def _blank(c, d):
    return [np.full(max(d.rcount[q], 1) * d.E, GUARD, np.uint8) for q in range(c["p"])]


# ------------------------------------------------------------------ references

def r1(c, d, S):
    """The ranks' plans evaluated on the CPU: per-rank recv bytes."""
    return _ref(c["dtype"], c["op"]).run_plans(d.plans, S, _blank(c, d))


def _oracle_call(oracle, c, s8, r8, dtype, op):
    oracle.smp_set(1 if c["smp"] else 0)
    try:
        if c["coll"] == "ar":
            return oracle.allreduce(s8, r8, c["n"], dtype, op)
        if c["coll"] == "red":
            return oracle.reduce(s8, r8, c["n"], dtype, op, c["root"])
        if c["coll"] == "scan":
            return oracle.scan(s8, r8, c["n"], dtype, op)
        return oracle.reduce_scatter(s8, r8, c["cnts"], dtype, op)
    finally:
        oracle.smp_set(0)


_callbacks = {}
_USER_FN = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int),
                            ctypes.POINTER(ctypes.c_int))


def _callback(op, dtype):
    """An MPI_User_function whose body is half_ref.op_u8 / fp8_ref.op_u8."""
    if (op, dtype) not in _callbacks:
        ref, E = _ref(dtype), ESIZE[dtype]

        def fn(invec, inoutvec, len_ptr, type_ptr):
            n = len_ptr[0]
            if n > 0:
                a = np.ctypeslib.as_array((ctypes.c_uint8 * (n * E)).from_address(invec))
                b = np.ctypeslib.as_array((ctypes.c_uint8 * (n * E)).from_address(inoutvec))
                ref.op_u8(op, dtype, a, b, n)

        _callbacks[op, dtype] = _USER_FN(fn)
    return ctypes.cast(_callbacks[op, dtype], ctypes.c_void_p).value


def applies(mvx, oracle, c, d, ref_dtype, ref_op, ref_kind):
    """Does the oracle's collective on (ref_dtype, ref_op) take the algorithm
    the narrow type's plans take?  mvx.algorithm for both types under the
    case's flavour, and oracle.algorithm for the reference's own choice.
    oracle.algorithm reports the choice of intra_Allreduce / intra_Reduce and
    knows no flavour; the _SMP_ leader path in front of it (coll_sim.c
    smp_leader) is restated here: count * extent below the threshold.  A
    wrong answer here cannot let anything pass: R2 is still the oracle's own
    run under the case's flavour, so a True too many makes R1 == R2 fail on
    the CPU, and a False too many only drops an R2, whose share the CPU test
    bounds from below."""
    p = c["p"]
    if mvx.algorithm(d.cid, p, d.tot, ref_dtype, opkind=ref_kind, tuning=d.tun) != d.alg:
        return False
    if d.alg == mvx.ALG_SMP_LEADER:
        thr = d.tun.shmem_coll_allreduce_threshold if c["coll"] == "ar" else d.tun.shmem_coll_reduce_threshold
        return bool(c["smp"]) and d.tot * oracle.dtype_info(ref_dtype)[0] < thr
    if d.alg in (mvx.ALG_NONE, mvx.ALG_SCAN_RECDBL):         # Scan has one algorithm
        return True
    return oracle.algorithm(d.cid, p, d.tot, ref_dtype, ref_op) == d.alg


def r2(mvx, oracle, c, d, S):
    """The oracle's replay of the reference schedule: per-rank recv bytes, or
    None where it takes another algorithm."""
    p, dtype, op = c["p"], c["dtype"], c["op"]
    if op in ROUNDING:
        carrier = CARRIER[d.E]
        assert oracle.user_op_set(USER_OP, _callback(op, dtype), 1) == 0
        if not applies(mvx, oracle, c, d, carrier, USER_OP, mvx.OPKIND_USER_COMMUTE):
            return None
        R = _blank(c, d)
        rc = _oracle_call(oracle, c, [s.copy() for s in S], R, carrier, USER_OP)
        assert rc == [0] * p
        return R
    fop = A.BASE.get(op, op)
    if not applies(mvx, oracle, c, d, MPI_FLOAT, fop, mvx.OPKIND_PREDEFINED):
        return None
    F = [A.widen(dtype, s) for s in S]
    R = [np.zeros(max(d.rcount[q], 1), np.float32) for q in range(p)]
    rc = _oracle_call(oracle, c, [f.view(np.uint8) for f in F], [x.view(np.uint8) for x in R], MPI_FLOAT, fop)
    assert rc == [0] * p
    out = _blank(c, d)
    for q, m in checked(c, d):
        if op in ACC:
            out[q][:m * d.E] = A.round_to(dtype, R[q][:m])
        else:
            out[q][:m * d.E] = np.ascontiguousarray(_ref(dtype).narrow(dtype, R[q][:m])).view(np.uint8)
    return out


def r3(c, d, S):
    """E4M3 MVX_SUM_ACC32 on Allreduce / Reduce: the float64 sum of the
    widened sends encoded once (every partial sum is exact in float32), or
    None."""
    if not (c["dtype"] == fp8_ref.E4M3 and c["op"] == 164 and c["coll"] in ("ar", "red") and c["n"]):
        return None
    exact = fp8_ref.widen(c["dtype"], S[0])
    for s in S[1:]:
        exact = exact + fp8_ref.widen(c["dtype"], s)
    return fp8_ref.encode(c["dtype"], exact)


def undefined_expect(mvx, oracle, c, d, S):
    """An undefined op: (per-rank codes, per-rank recv bytes) of the oracle's
    MPI_MINLOC on the carrier type, and the codes of the same op on MPI_FLOAT
    (None where MPI_FLOAT takes another algorithm)."""
    p = c["p"]
    R = _blank(c, d)
    rcs = _oracle_call(oracle, c, [s.copy() for s in S], R, CARRIER[d.E], MPI_MINLOC)
    rcs_float = None
    if applies(mvx, oracle, c, d, MPI_FLOAT, c["op"], mvx.OPKIND_PREDEFINED):
        F = [A.widen(c["dtype"], s).view(np.uint8) for s in S]
        RF = [np.zeros(max(d.rcount[q], 1) * 4, np.uint8) for q in range(p)]
        rcs_float = _oracle_call(oracle, c, F, RF, MPI_FLOAT, c["op"])
    return rcs, R, rcs_float


def assert_same(c, got, ref, what):
    """The type's own comparison: bit for bit, NaN for NaN in SUM / PROD."""
    op = c["op"]
    _ref(c["dtype"], op).assert_same(op, c["dtype"], got, ref, (c["id"], what))


def nan_count(c, ref):
    return int(A.isnan(c["dtype"], ref).sum())


# ------------------------------------------------------------------ GPU runner

def _place(a_u8, kind, shift, E, fill, tail):
    """A buffer of kind `kind` holding bytes a_u8, `shift` elements into an
    allocation otherwise filled with `fill`; returns (buffer, allocation)."""
    import torch
    off, nb = shift * E, a_u8.nbytes
    whole = np.full(off + nb + tail, fill, np.uint8)
    whole[off:off + nb] = a_u8
    if kind == "pin":
        t = torch.empty(whole.size, dtype=torch.uint8, pin_memory=True)
        t.numpy()[:] = whole
        whole = t
    elif kind == "dev":
        whole = torch.from_numpy(whole).to("cuda")
    return whole[off:off + max(nb, 1)], whole


def _back(whole):
    import torch
    if isinstance(whole, torch.Tensor):
        if whole.is_cuda:
            torch.cuda.synchronize()
        return whole.cpu().numpy()
    return whole


def run_case(mvx, oracle, comms, c, record=None):
    """One case on the device against R1, R2 and R3, with its return codes,
    guard bytes and untouched sends.  `record` collects {id, dtype, eligible,
    ran}: whether the call was PIPE-eligible and what last_exchange said."""
    p, coll, dtype, op = c["p"], c["coll"], c["dtype"], c["op"]
    d = derive(mvx, c)
    E = d.E
    S = inputs(c, d)
    if p not in comms:
        comms[p] = mvx.Comm.local_ranks(p, 0)
    comm = comms[p]
    assert comm.set_exchange(mvx.EXCH_PIPE if c["exch"] == "pipe" else mvx.EXCH_P2P, c["slices"]) == 0
    assert comm.set_tuning(d.tun) == 0
    sends, recvs, swhole, rwhole = [], [], [], []
    for q in range(p):
        b, w = _place(S[q], c["kinds"][2 * q], c["shift"][2 * q], E, 0, 1)
        sends.append(b)
        swhole.append(w)
        b, w = _place(np.full(d.rcount[q] * E, GUARD, np.uint8), c["kinds"][2 * q + 1], c["shift"][2 * q + 1], E,
                      GUARD, TAIL)
        recvs.append(b)
        rwhole.append(w)
    if coll == "ar":
        r, rcs = comm.allreduce_multi(sends, recvs, c["n"], dtype, op)
    elif coll == "red":
        r, rcs = comm.reduce_multi(sends, recvs, c["n"], dtype, op, c["root"])
    elif coll == "scan":
        r, rcs = comm.scan_multi(sends, recvs, c["n"], dtype, op)
    else:
        r, rcs = comm.reduce_scatter_multi(sends, recvs, c["cnts"], dtype, op)
    assert r == 0, (r, c["id"])
    if record is not None and d.runs:
        record.append(dict(id=c["id"], dtype=dtype, eligible=d.pipe_eligible,
                           ran=comm.last_exchange() == mvx.EXCH_PIPE))
    got = []
    for q in range(p):
        off = c["shift"][2 * q + 1] * E
        w = _back(rwhole[q])
        nb = d.rcount[q] * E
        assert (w[:off] == GUARD).all(), ("bytes before recv written", q, c["id"])
        assert (w[off + nb:] == GUARD).all(), ("bytes past the result written", q, c["id"])
        got.append(w[off:off + nb])
        off = c["shift"][2 * q] * E
        w = _back(swhole[q])
        assert np.array_equal(w[off:off + S[q].size], S[q]) and not w[:off].any() and not w[off + S[q].size:].any(), \
            ("send changed", q, c["id"])
    if d.kind == "invalid":
        assert [mvx.error_class(x) for x in rcs] == [9] * p, (rcs, c["id"])
        assert all((g == GUARD).all() for g in got), ("recv written without an op", c["id"])
        return d
    if coll == "red":
        for q in range(p):
            assert q == c["root"] or (got[q] == GUARD).all(), ("non-root recv written", q, c["id"])
    if d.kind == "undefined":
        want_rcs, want, rcs_float = undefined_expect(mvx, oracle, c, d, S)
        assert list(rcs) == want_rcs, (rcs, want_rcs, c["id"])
        assert rcs_float is None or list(rcs) == rcs_float, (rcs, rcs_float, c["id"])
        for q in range(p):
            assert np.array_equal(got[q], want[q][:d.rcount[q] * E]), ("undefined op's bytes", q, c["id"])
        return d
    assert list(rcs) == [0] * p, (rcs, c["id"])
    refs = [("R1", r1(c, d, S)), ("R2", r2(mvx, oracle, c, d, S))]
    for name, ref in refs:
        if ref is None:
            continue
        for q, m in checked(c, d):
            if op in PIN_OPS and name == "R2":
                assert np.array_equal(got[q][:m * E], ref[q][:m * E]), (c["id"], name, q)
            else:
                assert_same(c, got[q][:m * E], ref[q][:m * E], (name, q))
    exact = r3(c, d, S)
    if exact is not None:
        for q, m in checked(c, d):
            assert_same(c, got[q][:m], exact, ("R3", q))
    return d
