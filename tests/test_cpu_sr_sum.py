"""CPU: the stochastically rounded f32 sum (mvx_op_create_sr_sum; device-layer op
index MVX_SR_SUM = 170): the reference's hash and lack of bias, the handle, the
(op, type) verdicts and the launch plans (op index 16, under 170 alone)."""
import numpy as np
import pytest

import acc32_ref as A
import sr_ref as R

SR, SUM, SUM_ACC32, MPI_INT, MPI_FLOAT, ERR_OP, NOT_DEFINED = 170, 102, 164, 6, 10, 9, 329
TYPES = pytest.mark.parametrize("t", A.TYPES, ids=lambda t: A.NAMES[t])


def test_hash_known_answers():
    for g, seed, want in ((0, 0, 0xb8dbb7ba), (5, 0x0123456789abcdef, 0x22b57a34), (2 ** 32 + 7, 2 ** 64 - 1, 0x5173939a)):
        assert int(R.H(g, seed)) == want == int(R.H(np.array([g], np.uint64), seed)[0]), (g, hex(seed))


@TYPES
def test_reference_is_unbiased(t):
    """65536 elements at f = 0.3 and f = 1/256 of the gap above 1.0: the share rounded up is within 4
    standard deviations of floor(f * 2^nb) / 2^nb; representable values never move."""
    m, _, nb, _ = R.FMT[t]
    n, q = 65536, 2.0 ** -m
    for f in (0.3, 1 / 256):
        v = np.full(n, 1 + f * q, np.float32)
        p = np.floor((float(v[0]) - 1) / q * 2 ** nb) / 2 ** nb
        for seed in (0, 1, 0x0123456789abcdef, 2 ** 64 - 1):
            for base in (0, 3, 2 ** 32 - 5, 2 ** 40 + 1):
                w = A.widen(t, R.sr_round(t, v, base, seed))
                assert np.isin(w, (1, 1 + q)).all() and abs((w > 1).mean() - p) <= 4 * np.sqrt(p * (1 - p) / n), (f, seed, base)
    on = np.arange(n, dtype=np.float32) % 13 * np.float32(0.25) - 1
    assert np.array_equal(R.sr_round(t, on, 7, 1), A.round_to(t, on))


def test_handle_and_verdicts(mvx):
    hip = mvx.hip()
    assert mvx.MVX_SR_SUM == SR and mvx.DEFINED_SR == {SR: [64, 65, 72, 73]}
    rc, h = mvx.op_create_sr_sum(2 ** 64 - 1)
    assert rc == 0 and h >= 200
    P, Q = (mvx.plan(mvx.COLL_ALLREDUCE, 3, 0, 10, 72, o) for o in (h, SUM))
    assert P.opkind == mvx.OPKIND_PREDEFINED and P.symmetric == 1 and (P.k, P.c_cnt) == (Q.k, Q.c_cnt)
    assert mvx.plan(mvx.COLL_ALLREDUCE, 3, 0, 10, MPI_FLOAT, h).symmetric == 0
    assert mvx.MPI_Op_free(h) == (0, 0) and mvx.MPI_Op_free(h)[0] == ERR_OP      # freed: invalid again
    assert mvx.MPI_Op_free(SR)[0] == ERR_OP                                      # 170 is no MPI-level op
    for t in mvx.DEVICE_TYPES:
        ok = t in A.TYPES
        assert hip.mvx_op_supported(SR, t) == ok and hip.mvx_op_element_size(SR, t) == (A.ESIZE[t] if ok else 0), t
        assert hip.mvx_op_apply(SR, t, None, None, 0, None) == (0 if ok else NOT_DEFINED), t
    for t in (MPI_FLOAT, MPI_INT):
        assert hip.mvx_op_program_sr(t, None, None, 1, 0, 0, None, 4, 0, 1, 0, None) == NOT_DEFINED


@TYPES
def test_launch_plan_names_op_index_16(mvx, t):
    """The tree and the chain over 8 leaves and the apply, small and past the non-temporal threshold:
    MVX_SUM_ACC32's kernel, grid and LDS with 16 as the first template argument, MPI_SUM's plan as it
    was; a chain over 4 runs the masked program over 8."""
    hip, e, dst = mvx.hip(), A.ESIZE[t], (40 << 32) + 256
    for n in (17, 4099, (64 << 20) // e):
        for k, tm, cm in ((8, hip.mvx_tree_mask(8), 0), (8, 0, hip.mvx_chain_mask(8)), (2, 1, 0), (4, 0, hip.mvx_chain_mask(4))):
            got = {}
            for o in (SR, SUM_ACC32, SUM):
                rc, pl = mvx.op_plan(o, t, [(q + 1 << 32) + 256 for q in range(k)], dst, n, tm, cm)
                assert rc == 0
                got[o] = (pl.symbol.decode().split("<", 1), pl.blocks, pl.dynamic_lds)
            (base, rest), (abase, arest) = got[SR][0], got[SUM_ACC32][0]
            assert rest.startswith("16, ") and arest.startswith("12, ") and got[SUM][0][1].startswith("2, "), got
            if k == 4:
                assert base == "k_combine" and ", 8, 1, " in rest, got[SR]
            else:
                assert base == abase and rest[3:] == arest[3:] and got[SR][1:] == got[SUM_ACC32][1:], got
