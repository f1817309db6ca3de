"""GPU: every reduction kernel of the reference's own datatypes, launched on
edge values and on random data with random pair padding.

One test case per (op, kernel set) of tests/kernel_matrix.py: every k_combine
family (the plain op, programs over 3 and 4 leaves on the KMAX = 4 kernels,
masked programs over 5 to 7, folded trees and chains, the fixed trees and full
chains) in the cached and the non-temporal build, aligned, with a head and a
tail, and with mutually misaligned operands; a second case per set for its
body kernels (k_tree_body, k_chain_body, k_pxi_loc_body) at 1, 257 and 513
chunks.  At most kernel_matrix.MAX_LAUNCHES launches per case, no buffer above
64 KiB.  tests/test_cpu_kernel_matrix.py holds the list complete.

Every launch goes through tests/small_launch.py: the result against the CPU
oracle (plan_exec.combine_cpu / oracle.op) on whole elements -- so a result's
padding must be leaf 0's for op_combine and the inout operand's for op_apply,
and the x87 types byte for byte; the 256-byte guard bands; the plan for the
addresses used against what ran; and the kernel symbol the case names.  The
one exemption is mvxtest.assert_same's: a SUM or PROD lane of float, double
or complex that is NaN in the oracle need only be NaN; at most
edge_values.NAN_CAP of a launch's lanes are, asserted on the oracle's result
before the launch.

The handle sweep runs every defined (op, handle) once through mvx_op_apply on
the edge cross: the handles that share a kernel (MPI_UNSIGNED_LONG with
MPI_LONG for SUM, not for MAX) at the extremes of each width and signedness.
"""
import pytest

import edge_values as EV
import kernel_matrix as KM
import mvxtest as T
import small_launch as SL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handles(mvx, oracle):
    H = KM.Handles(mvx, oracle)
    yield H
    H.free()


@pytest.fixture
def launch_defaults(mvx):
    try:
        yield
    finally:
        KM.restore(mvx)


def _run_part(mvx, oracle, handles, sc, part):
    Ls = KM.launches(sc, part)
    assert 0 < len(Ls) <= KM.MAX_LAUNCHES
    h = handles(sc.spec)
    ran = {KM.run(mvx, oracle, SL, sc, h, L) for L in Ls}
    assert ran == {L.symbol for L in Ls}


@pytest.mark.parametrize("sc", KM.SETS, ids=KM.set_id)
def test_combine_families_on_edges_and_padding(mvx, oracle, handles, launch_defaults, sc):
    _run_part(mvx, oracle, handles, sc, "combine")


@pytest.mark.parametrize("sc", [sc for sc in KM.SETS if KM.has_body(sc)], ids=KM.set_id)
def test_body_kernels_on_edges_and_padding(mvx, oracle, handles, launch_defaults, sc):
    _run_part(mvx, oracle, handles, sc, "body")


@pytest.mark.parametrize("op", T.ALL_OPS)
def test_every_defined_handle_on_the_edge_cross(mvx, oracle, handles, launch_defaults, op):
    """One mvx_op_apply per defined (op, handle), default launch policy."""
    specs = KM.sweep_pairs(mvx)[op]
    assert 0 < len(specs) <= KM.MAX_LAUNCHES
    for spec in specs:
        a, b = EV.operands(spec)
        h = handles(spec)
        if EV.has_nan_rule(op, spec):
            ref = T.clone(b)
            assert oracle.op(op, h, SL._u8(a), SL._u8(ref), len(a)) == 0
            assert EV.nan_share(ref) <= EV.NAN_CAP, (op, spec)
        sym, _ = SL.apply(mvx, oracle, op, h, len(a), data=(a, b))
        assert sym.startswith("k_combine<%d, " % (op - 100)) or sym.startswith("k_pxi_loc_body<%d, 2, " % (op - 100)), sym
