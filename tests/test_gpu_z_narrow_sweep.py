"""GPU: the narrow floating types and the f32-accumulating ops through every
executor path (tests/narrow_sweep.py: the case list, the references R1 / R2 /
R3 and the runner; tests/test_cpu_narrow_sweep.py checks the list and the
references against each other without a device).

Each case is one call on a virtual communicator of up to 64 ranks; every
rank's result must equal each reference that applies, its return code the
reference's, the guard bytes around every recv buffer and every send must be
as they were.  MVX_FUZZ_NARROW_CASES / MVX_FUZZ_NARROW_SEED widen or move the
sweep.  Two fixed families name the sharpest edges outright: MVX_SUM_ACC32
over more than 8 leaves from send buffers 1, 2 and 3 bytes off a word (the
f32 temporaries' placement, mvxi_wide_residue), SUM with per-step rounding at
p = 17 and 64, and E4M3 MVX_SUM_ACC32 against the float64 sum at every p.

The file's name sorts after every other GPU file on purpose: a sweep is the
last thing to run, and adding it moves no earlier test's place in the run
order.  It depends on no test before it and none depends on it."""
import pytest

import narrow_sweep as N

pytestmark = pytest.mark.gpu

IDS = [N.A.NAMES[t] for t in N.TYPES]


@pytest.fixture(scope="module")
def comms():
    cs = {}
    yield cs
    for c in cs.values():
        c.free()


@pytest.fixture(scope="module")
def record():
    return []


@pytest.fixture(scope="module")
def sweep():
    return N.cases()


@pytest.mark.parametrize("batch", range((N.N_CASES + N.BATCH - 1) // N.BATCH))
def test_random_sweep(mvx, oracle, comms, record, sweep, batch):
    for c in sweep[batch * N.BATCH:(batch + 1) * N.BATCH]:
        N.run_case(mvx, oracle, comms, c, record)


@pytest.mark.parametrize("dtype", N.TYPES, ids=IDS)
def test_acc32_sum_over_9_and_33_leaves_from_shifted_sends(mvx, oracle, comms, record, dtype):
    """Allreduce and Reduce_scatter of 20001 (9000 + r % 2 a rank) elements
    with MVX_SUM_ACC32, every send buffer 1, 2 or 3 elements into its
    allocation and the recv buffer shifted otherwise, p2p and pipe with 3
    slices: at p = 33 the f32 temporaries start at each residue the type
    allows (at p = 9 the ninth rank is a pre-fold of an 8-leaf program)."""
    for c in N.fixed_acc32_edge(dtype):
        d = N.run_case(mvx, oracle, comms, c, record)
        assert d.wide == (c["p"] == 33), c["id"]
        assert not d.wide or (c["shift"][0] * d.E) % 4 in d.wide_residues, c["id"]


@pytest.mark.parametrize("dtype", N.TYPES, ids=IDS)
def test_sum_rounds_every_step_at_17_and_64_ranks(mvx, oracle, comms, record, dtype):
    """SUM at p = 17 and 64, counts 7 and 20001: groups of 8 into narrow
    temporaries, then a tree or chain over those -- any other association
    changes bits.  Against the plans (R1) and, where the algorithms coincide,
    the oracle's replay with the type's op as a user function (R2)."""
    for c in N.fixed_wide_sum(dtype):
        N.run_case(mvx, oracle, comms, c, record)


def test_e4m3_acc32_sum_equals_the_float64_sum_at_every_p(mvx, oracle, comms, record):
    """E4M3 with MVX_SUM_ACC32, Allreduce and Reduce at every p from 1 to 64:
    the device == the float64 sum of the widened sends encoded once (R3, with
    R1 and R2) -- count 7, and count 700 over the format's whole finite range
    through pipe with 3 slices, where partial sums of 63 x 448 next to 2^-9
    take every bit of a float32 significand."""
    for c in N.fixed_e4m3_exact():
        N.run_case(mvx, oracle, comms, c, record)


def test_every_pipe_eligible_case_ran_the_pipelined_exchange(mvx, oracle, comms, record, sweep):
    """From the runner's record: a call with the pipe exchange set, all its
    buffers in HBM and a span above one 256-element slice reported EXCH_PIPE,
    and every type has such a call.  (Cases this process has not run yet --
    the file's tests deselected -- run here first.)"""
    done = {r["id"] for r in record}
    for c in sweep:
        if c["id"] not in done and N.derive(mvx, c).pipe_eligible:
            N.run_case(mvx, oracle, comms, c, record)
    missed = [r["id"] for r in record if r["eligible"] and not r["ran"]]
    assert not missed, missed
    stray = [r["id"] for r in record if r["ran"] and not r["eligible"]]
    assert not stray, stray
    for t in N.TYPES:
        assert any(r["ran"] for r in record if r["dtype"] == t), N.A.NAMES[t]
    print("narrow sweep: %d calls ran the executor, %d of them PIPE" % (len(record), sum(r["ran"] for r in record)))
