"""CPU: the narrow-type sweep's case list and references, before anything is
launched (tests/narrow_sweep.py; tests/test_gpu_z_narrow_sweep.py runs the same
list on the device).

The plan evaluators (R1: half_ref / fp8_ref / acc32_ref on mvx.plan) must
equal the oracle's replay of the reference schedule (R2) wherever both take
the same algorithm, and the float64 sum (R3) wherever that is defined -- at p
up to 64 and under the _SMP_ flavour, where no other test compares them.  The
list must reach what it is for: every (type, op), every p, both flavours,
every buffer kind, the residues of a wide ACC32 combine's leaf, the pipelined
exchange."""
import collections

import numpy as np
import pytest

import narrow_sweep as N
from test_gpu_fp8_coll import NAN_CAP        # the cap the types' collective tests hold their inputs to

NAMES = N.A.NAMES


@pytest.fixture(scope="module")
def survey(mvx, oracle):
    """Every case's references computed once; what the tests below ask."""
    out = []
    for c in N.cases():
        d = N.derive(mvx, c)
        s = dict(c=c, d=d, r2=False, r3=False, nan=0, total=0)
        out.append(s)
        if d.kind == "invalid":
            continue
        S = N.inputs(c, d)
        if d.kind == "undefined":
            want_rcs, _, rcs_float = N.undefined_expect(mvx, oracle, c, d, S)
            # the ranks whose plan calls the op are the ranks of the replay
            mine = [329 if (P.calls_uop and d.alg != mvx.ALG_NONE) else 0 for P in d.plans]
            assert mine == want_rcs, (c["id"], mine, want_rcs)
            assert rcs_float is None or rcs_float == want_rcs, (c["id"], rcs_float, want_rcs)
            s["float_rc"] = rcs_float is not None
            continue
        R1 = N.r1(c, d, S)
        R2 = N.r2(mvx, oracle, c, d, S)
        R3 = N.r3(c, d, S)
        for q, m in N.checked(c, d):
            nb = m * d.E
            if R2 is not None:
                N.assert_same(c, R1[q][:nb], R2[q][:nb], ("R1 == R2", q))
            if R3 is not None:
                N.assert_same(c, R1[q][:nb], R3, ("R1 == R3", q))
            if c["op"] in N.ROUNDING + N.ACC:
                s["nan"] += N.nan_count(c, R1[q][:nb])
                s["total"] += m
        s["r2"], s["r3"] = R2 is not None, R3 is not None
    return out


def test_r2_reaches_most_cases_and_every_wide_p(survey):
    defined = [s for s in survey if s["d"].kind in ("defined", "acc")]
    assert 2 * sum(s["r2"] for s in defined) >= len(defined), (sum(s["r2"] for s in defined), len(defined))
    if N.N_CASES < N.N_DEFAULT:
        return
    for p in [p for p in N.PS if p >= 16]:
        assert any(s["r2"] and s["c"]["p"] == p and s["c"]["op"] in N.ROUNDING for s in survey), p
    assert any(s["r3"] for s in survey)


def test_nan_exempt_share_stays_under_the_cap(survey):
    """A condition on the inputs: a NaN result is compared as NaN only."""
    acc = collections.defaultdict(lambda: [0, 0])
    for s in survey:
        acc[s["c"]["op"], s["c"]["dtype"]][0] += s["nan"]
        acc[s["c"]["op"], s["c"]["dtype"]][1] += s["total"]
    for key, (bad, total) in acc.items():
        assert bad < NAN_CAP * total or not total, ("NaN-exempt share of R1", key, bad, total)


@pytest.mark.skipif(N.N_CASES < N.N_DEFAULT, reason="coverage is asked of the default list")
def test_the_list_covers_types_ops_sizes_flavours_and_kinds(survey):
    cs = [s["c"] for s in survey]
    pairs = {(c["dtype"], c["op"]) for c in cs}
    assert not [(t, o) for t in N.TYPES for o in N.DEFINED + N.ACC if (t, o) not in pairs]
    assert {c["p"] for c in cs} == set(N.PS)
    assert {c["smp"] for c in cs} == {False, True}
    assert {c["exch"] for c in cs} == {"p2p", "pipe"}
    assert {c["coll"] for c in cs} == {"ar", "red", "rs", "scan"}
    assert any(c["op"] in N.UNDEFINED for c in cs) and any(c["op"] in N.INVALID for c in cs)
    # a buffer's kind counts where the call asks it: not for an empty buffer
    # (count 0, the recv of a non-root Reduce), not in a call that ends early
    for t in N.TYPES:
        for side in (0, 1):
            kinds = set()
            for s in survey:
                c, d = s["c"], s["d"]
                if c["dtype"] == t and d.runs:
                    size = d.nrecv if side else d.nsend
                    kinds |= {c["kinds"][2 * q + side] for q in range(c["p"]) if size[q]}
            assert kinds == {"dev", "host", "pin"}, (t, side, kinds)
    # some undefined-op cases also have the codes of the same op on MPI_FLOAT
    assert any(s.get("float_rc") for s in survey)
    # 1-byte types meet every shift residue mod 16, 2-byte types every even one
    for t in N.TYPES:
        res = set()
        for c in cs:
            if c["dtype"] == t:
                res |= {(s * N.ESIZE[t]) % 16 for s in c["shift"]}
        assert res == set(range(0, 16, N.ESIZE[t])), (t, res)


@pytest.mark.skipif(N.N_CASES < N.N_DEFAULT, reason="coverage is asked of the default list")
def test_wide_acc32_cases_meet_every_residue_within_the_slot_budget(survey):
    """Combines of more than 8 leaves in f32 temporaries: the residue mod 4 of
    the leaf that places them (mvxi_wide_residue) takes every value the type
    allows, and every such plan's launches stay inside their reserved slots."""
    seen = collections.defaultdict(set)
    for s in survey:
        d = s["d"]
        if not d.wide:
            continue
        seen[s["c"]["dtype"]] |= d.wide_residues
        for P in d.plans:
            if P.has_combine and P.k > 8:
                budget, used = P.wide_slots()
                assert used <= budget, (s["c"]["id"], P.rank, used, budget)
    for t in N.TYPES:
        want = {1, 2, 3} if N.ESIZE[t] == 1 else {2}
        assert want <= seen[t], (NAMES[t], seen[t])


@pytest.mark.skipif(N.N_CASES < N.N_DEFAULT, reason="coverage is asked of the default list")
def test_pipe_eligible_cases_exist_for_every_type(survey):
    for t in N.TYPES:
        el = [s for s in survey if s["d"].pipe_eligible and s["c"]["dtype"] == t]
        assert len(el) >= 6, (NAMES[t], len(el))
        assert sum(s["c"]["op"] in N.ACC and s["c"]["p"] >= 9 for s in el) >= 2, NAMES[t]


def test_e4m3_acc32_sum_is_the_float64_sum_at_every_p(mvx, oracle):
    """The fixed E4M3 / MVX_SUM_ACC32 family: R1 == R3 on Allreduce and Reduce
    at every p of the sweep, R1 == R2 where R2 applies; over the full finite
    range the crafted elements give 2^-9 exactly, and enough sums stay finite
    (within 448) for the comparison to be one of values: a quarter at least,
    at p = 64 too, where overflow to NaN is the commonest result."""
    seen = set()
    for c in N.fixed_e4m3_exact():
        d = N.derive(mvx, c)
        S = N.inputs(c, d)
        R1, R2, R3 = N.r1(c, d, S), N.r2(mvx, oracle, c, d, S), N.r3(c, d, S)
        assert R3 is not None, c["id"]
        for q, m in N.checked(c, d):
            N.assert_same(c, R1[q][:m], R3, ("R1 == R3", q))
            assert np.array_equal(R1[q][:m], R3) or N.nan_count(c, R3), c["id"]
            if R2 is not None:
                N.assert_same(c, R1[q][:m], R2[q][:m], ("R1 == R2", q))
            seen.add((c["p"], c["coll"]))
        if c.get("full"):
            assert 4 * N.nan_count(c, R3) <= 3 * R3.size, (c["id"], N.nan_count(c, R3))
            assert c["p"] < 3 or list(R3[:2]) == [0x01, 0x01], (c["id"], R3[:2])
            # Reduce keeps the whole vector in one range: two slices at every p
            assert d.pipe_eligible or c["coll"] != "red", c["id"]
    assert seen == {(p, coll) for p in N.PS for coll in ("ar", "red")}


@pytest.mark.parametrize("dtype", N.TYPES, ids=[NAMES[t] for t in N.TYPES])
def test_fixed_cases_references_agree(mvx, oracle, dtype):
    """The two fixed families of the GPU file: R1 == R2 where R2 applies,
    R1 == R3 for E4M3; the ACC32 edge cases at p = 33 are wide (at p = 9 the
    ninth rank is a pre-fold of an 8-leaf program), a wide leaf's residue is
    the send shift's, and the pipe ones are PIPE-eligible."""
    some_r2 = False
    for c in N.fixed_acc32_edge(dtype) + N.fixed_wide_sum(dtype):
        d = N.derive(mvx, c)
        S = N.inputs(c, d)
        R1, R2, R3 = N.r1(c, d, S), N.r2(mvx, oracle, c, d, S), N.r3(c, d, S)
        for q, m in N.checked(c, d):
            if R2 is not None:
                N.assert_same(c, R1[q][:m * d.E], R2[q][:m * d.E], ("R1 == R2", q))
            if R3 is not None:
                N.assert_same(c, R1[q][:m * d.E], R3, ("R1 == R3", q))
        if c["op"] == 164:
            assert d.pipe_eligible == (c["exch"] == "pipe"), c["id"]
            assert d.wide == (c["p"] == 33), c["id"]
            assert not d.wide or (c["shift"][0] * d.E) % 4 in d.wide_residues, (c["id"], d.wide_residues)
            assert c["shift"][0] != c["shift"][1]
        else:
            some_r2 |= R2 is not None
    assert some_r2


def test_list_is_stable_under_its_length():
    a, b = N.cases(50), N.cases(20)
    assert a[:20] == b
    assert np.all([c["n"] <= N.WIDE_MAX and (not c["cnts"] or sum(c["cnts"]) <= N.WIDE_MAX)
                   for c in N.cases() if c["p"] >= 17])
