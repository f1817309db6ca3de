"""TEST HELPER: the launch matrix of the reduction kernels of the reference's
own datatypes -- one case list, planned (tests/test_cpu_kernel_matrix.py) or
launched (tests/test_gpu_kernel_matrix.py).

SETS names every kernel set of mvx_ops_{cmp,arith,logic,loc}.hip once: (op,
a representative datatype, the compiler's spelling of the element type).  The
CPU test checks the list against what mvx_op_plan answers for every defined
(op, handle), so a set added later without an entry here fails there.

`launches(sc, part)` is the fixed list of launches of one set: every kernel
family (FAMILIES; BODIES for the body kernels) at two sizes (three for the
bodies), each once on edge data (edge_values.edge_leaves) and once on
mvxtest.rand_vec data with random padding.  Placement (aligned whole chunks /
every operand off the 16-byte grid by the same amount, with a head and a tail
/ every operand at an offset of its own), build (set_launch(cap, 4):
non-temporal, body dispatch; set_launch(cap, -1): cached) and grid cap
(default, 1, 3) rotate over families and sets instead of multiplying.  Each
launch names the kernel symbol it must run, restated here from
mvx_ops_tab.h / choose_family, not asked of the planner.

`run(...)` performs one launch through small_launch (`R` = small_launch) or
plans it (`R` = small_launch.PLAN): the result against the CPU oracle on
whole elements, the guard bands, plan == launch, and the symbol.
"""
import collections
import re

import numpy as np

import edge_values as EV
import small_launch as SL
from small_launch import SHAPE_CHAIN, SHAPE_TREE

MAX_LAUNCHES = 64                      # per parametrized GPU test case
ALIGNED, SHIFTED, MISALIGNED = "aligned", "shifted", "misaligned"

SetCase = collections.namedtuple("SetCase", "op spec tname")

_U = [(2, "unsigned char"), (5, "unsigned short"), (7, "unsigned int"), (9, "unsigned long")]
_S = [(1, "signed char"), (4, "short"), (6, "int"), (8, "long")]
_FL = [(10, "float"), (11, "double")]
_LD = [(12, "xf::xf80")]
_CX = [(23, "mvx::cf32"), (24, "mvx::cf64")]
_LG = [(25, "mvx::flog")]
_LOC = [(("h", 17), "mvx::pfi"), (("h", 18), "mvx::pdi"), (("h", 19), "mvx::pli"), (("h", 20), "mvx::psi"),
        (("h", 21), "mvx::pii"), (("h", 22), "xf::pxi"), (("c2", 1), "mvx::pp<signed char>"),
        (("c2", 4), "mvx::pp<short>"), (("c2", 8), "mvx::pp<long>"), (("c2", 10), "mvx::pp<float>"),
        (("c2", 11), "mvx::pp<double>"), (("c2", 12), "mvx::pp<xf::xf80>")]
# the element kinds of each op's switch (mvx_ops_tab.h: SIGNED_INT, ARITH_INT,
# FLOATS, CMPLX, LDBL, LOGICAL, PAIRS, LDBL_INT, CONTIG_PAIRS); integer SUM,
# PROD, logical and bitwise ops run the unsigned kernel of the width
_BY_OP = {100: _S + _U + _FL + _LD, 101: _S + _U + _FL + _LD,
          102: _U + _FL + _CX + _LD, 103: _U + _FL + _CX + _LD,
          104: _U + _FL + _LD + _LG, 106: _U + _FL + _LD + _LG, 108: _U + _FL + _LD + _LG,
          105: _U, 107: _U, 109: _U}
SETS = [SetCase(op, ("h", h), t) for op in sorted(_BY_OP) for h, t in _BY_OP[op]] + \
       [SetCase(op, spec, t) for op in (110, 111) for spec, t in _LOC]
HEAVY = ("xf::xf80", "xf::pxi", "mvx::pp<xf::xf80>")       # alu_heavy<T>: no tree / chain body, U = 1


def set_id(sc):
    return "op%d-%s%d-%s" % (sc.op, sc.spec[0], sc.spec[1], sc.tname.replace(" ", "_"))


def has_body(sc):
    return sc.tname not in HEAVY or sc.tname == "xf::pxi"


# (name, k, shape, folded, KMAX, U of the cached build, U of the non-temporal
# build, PROG) -- tests/test_gpu_acc32_ops.py::FAMILIES
FAMILIES = [
    ("apply", 2, SHAPE_TREE, False, 2, 4, 4, 0),
    ("tree3", 3, SHAPE_TREE, False, 4, 2, 2, 0),
    ("tree3-folded", 3, SHAPE_TREE, True, 4, 2, 2, 0),
    ("chain4-folded", 4, SHAPE_CHAIN, True, 4, 2, 2, 0),
    ("chain5-folded", 5, SHAPE_CHAIN, True, 8, 1, 1, 0),
    ("tree6", 6, SHAPE_TREE, False, 8, 1, 1, 0),
    ("tree7-folded", 7, SHAPE_TREE, True, 8, 1, 1, 0),
    ("tree8-folded", 8, SHAPE_TREE, True, 8, 1, 1, 0),
    ("tree4", 4, SHAPE_TREE, False, 4, 1, 2, 1),
    ("tree8", 8, SHAPE_TREE, False, 8, 1, 2, 1),
    ("chain4", 4, SHAPE_CHAIN, False, 8, 1, 1, 0),
    ("chain6", 6, SHAPE_CHAIN, False, 8, 1, 1, 0),
    ("chain8", 8, SHAPE_CHAIN, False, 8, 1, 1, 0),
]
# the body kernels: aligned whole chunks, non-temporal, unfolded.  k_tree_body
# at 4 and 8 leaves, k_chain_body<.., 4, ..>, k_chain_body<.., 8, ..> at 5 and
# 8 leaves; MPI_LONG_DOUBLE_INT MAXLOC / MINLOC: k_pxi_loc_body at 2, 4 and 8
BODIES = [f for f in FAMILIES if f[0] in ("tree4", "tree8", "chain4", "chain8")] + \
         [("chain5", 5, SHAPE_CHAIN, False, 8, 1, 1, 0)]
PXI_BODIES = [f for f in FAMILIES if f[0] in ("apply", "tree4", "tree8")]
BODY_NVEC = (1, 257, 513)
CAPS = (None, 1, 3)

Launch = collections.namedtuple("Launch", "fam k shape folded placement offset nt cap n edge rot symbol")


def _fixed(fam):
    """The full unfolded trees and chains choose_family gives a kernel of their own."""
    _, k, shape, folded = fam[:4]
    return not folded and ((shape == SHAPE_TREE and k in (4, 8)) or (shape == SHAPE_CHAIN and k >= 4))


def expected_symbol(sc, fam, placement, nt):
    """The kernel template of one launch (mvx_ops_tab.h kfam / kchain / kset,
    mvx_ops.hip choose_family / plan)."""
    _, k, shape, folded, kmax, u0, u1, prog = fam
    o = sc.op - 100
    heavy = sc.tname in HEAVY
    if nt and placement == ALIGNED and not folded:
        if sc.tname == "xf::pxi" and (k == 2 or (shape == SHAPE_TREE and k in (4, 8))):
            return "k_pxi_loc_body<%d, %d, 1>" % (o, k)
        if not heavy and shape == SHAPE_TREE and k in (4, 8):
            return "k_tree_body<%d, %s, %d, 2>" % (o, sc.tname, k)
        if not heavy and shape == SHAPE_CHAIN and k >= 4:
            return "k_chain_body<%d, %s, %d, 2>" % (o, sc.tname, 4 if k == 4 else 8)
    if heavy and (prog == 1 or kmax == 4):
        u0 = u1 = 1
    return "k_combine<%d, %s, %d, %d, %d, %d>" % (o, sc.tname, kmax, u1 if nt else u0, 1 if nt else 0, prog)


def esize(sc):
    return EV.np_dtype(sc.spec).itemsize


def _size(E, placement, nvec, rot):
    """(n, offset): nvec chunks in the placement's shape.  Shifted: every
    operand `offset` bytes off the grid, a head of (16 - offset) / E elements
    and a tail one short of a chunk (elements of 16 bytes or more have no
    whole element up to the boundary: all go the element path)."""
    V = max(16, E) // E
    if placement == ALIGNED:
        return nvec * V, 0
    if placement == MISALIGNED:
        return nvec * V + 1, 0
    if V == 1:
        return nvec, 8
    offset = E * (1 + rot % (V - 1))
    return (16 - offset) // E + nvec * V + (V - 1), offset


def launches(sc, part):
    """The launches of one kernel set: part "combine" (k_combine, every
    family) or "body" (the body kernels; empty where the set has none)."""
    E = esize(sc)
    V = max(16, E) // E
    si = SETS.index(sc)
    n_edge = len(EV.operands(sc.spec)[0])
    out = []
    if part == "body":
        if not has_body(sc):
            return out
        for fi, fam in enumerate(PXI_BODIES if sc.tname == "xf::pxi" else BODIES):
            for ni, nvec in enumerate(BODY_NVEC):
                for edge in (1, 0):
                    j = len(out)
                    out.append(Launch(fam[0], fam[1], fam[2], False, ALIGNED, 0, 1, CAPS[(si + j) % 3], nvec * V, edge,
                                      si + j, expected_symbol(sc, fam, ALIGNED, 1)))
        return out
    for fi, fam in enumerate(FAMILIES):
        combos = [(ALIGNED, 0), (SHIFTED, 1), (MISALIGNED, 0), (ALIGNED, 1), (SHIFTED, 0), (MISALIGNED, 1)]
        if _fixed(fam) or (sc.tname == "xf::pxi" and fam[1] == 2):
            combos.remove((ALIGNED, 1))                 # that is the body kernel's launch
        for j in range(4):                              # two sizes, edge and random data
            placement, nt = combos[(si + fi + j) % len(combos)]
            rot = si + 4 * fi + j
            nvec = 257 if j // 2 else max(1, (n_edge - 2 * V) // V)      # the edge cross, cut to the placement's shape
            n, offset = _size(E, placement, nvec, rot)
            out.append(Launch(fam[0], fam[1], fam[2], fam[3], placement, offset, nt, CAPS[(si // 6 + si + fi + j) % 3], n,
                              1 - j % 2, rot, expected_symbol(sc, fam, placement, nt)))
    return out


def leaves_of(sc, L):
    """(S, F) of a launch: edge data or random data, padding random either way."""
    if L.edge:
        return EV.edge_leaves(sc.op, sc.spec, L.k, L.folded, L.n, L.rot, seed=L.rot % 7)
    return EV.rand_leaves(sc.op, sc.spec, L.k, L.folded, L.n, seed=L.rot)


def reference(oracle, sc, handle, L, S, F):
    """The oracle's result of a launch, as elements."""
    u8 = [SL._u8(x) for x in S]
    f8 = [SL._u8(x) if x is not None else None for x in F]
    return SL.combine_cpu(sc.op, handle, S[0].dtype.itemsize, u8, f8, L.shape, L.n).view(S[0].dtype)


def check_nan_cap(sc, ref, what):
    """SUM / PROD on float, double, complex: the NaN-exempt share of the
    oracle's result, asserted on the CPU before anything is launched."""
    if EV.has_nan_rule(sc.op, sc.spec):
        share = EV.nan_share(ref)
        assert share <= EV.NAN_CAP, ("NaN share of the oracle's result", share, set_id(sc), what)


def run(mvx, oracle, R, sc, handle, L):
    """One launch (R = small_launch) or its plan (R = small_launch.PLAN)."""
    mvx.set_launch(L.cap or SL.DEFAULT_CAP, 4 if L.nt else -1)
    data = None
    if R is SL:
        S, F = leaves_of(sc, L)
        assert all(x.nbytes <= EV.MAX_BYTES for x in S), L
        check_nan_cap(sc, reference(oracle, sc, handle, L, S, F), L)
        data = (S, F)
    mis = L.placement == MISALIGNED
    try:
        if L.fam == "apply" and L.rot % 2 == 0:         # mvx_op_apply in place: leaf 0 is the inout operand
            sym, blocks = R.apply(mvx, oracle, sc.op, handle, L.n, offset=L.offset, misalign=mis,
                                  data=(data[0][1], data[0][0]) if data else None)
        else:
            sym, blocks = R.combine(mvx, sc.op, handle, L.k, L.shape, L.n, offset=L.offset, folded=L.folded,
                                    misalign=mis, data=data)
    except AssertionError as e:                         # name the launch, and the operands of the first bad element
        m = re.search(r"\(elem (\d+)\)|elements differ, first (\d+):", str(e))
        i = int(m.group(1) or m.group(2)) if m else None
        at = [(q, x[i] if x.dtype.names is None else x[i].item(), None if F[q] is None else F[q][i])
              for q, x in enumerate(S)] if i is not None and data else None
        raise AssertionError("%s\n  in %s of %s\n  leaves (q, element, fold partner) at %s: %s"
                             % (e, L, set_id(sc), i, at)) from None
    assert sym == L.symbol, (sym, L)
    assert blocks >= 1 and (L.cap is None or blocks <= L.cap), (blocks, L)
    return sym


class Handles:
    """Datatype handles of specs: the contiguous count-2 types are made in the
    product's and the oracle's table (derived_util.make_both) on first use."""

    def __init__(self, mvx, oracle):
        self.mvx, self.oracle, self.made = mvx, oracle, {}

    def __call__(self, spec):
        import derived_util as D
        if spec[0] == "h":
            return spec[1]
        if spec not in self.made:
            rc, h = D.make_both(self.mvx, self.oracle, 2, spec[1])
            assert rc == 0, (spec, rc)
            self.made[spec] = h
        return self.made[spec]

    def free(self):
        import derived_util as D
        for h in self.made.values():
            D.free_both(self.mvx, self.oracle, h)
        self.made = {}


def sweep_pairs(mvx):
    """Every defined (op, spec): the reference's table and, for MAXLOC /
    MINLOC, the contiguous count-2 types."""
    import derived_util as D
    out = {op: [("h", h) for h in hs] for op, hs in mvx.DEFINED.items()}
    for op in (110, 111):
        out[op] = out[op] + [("c2", b) for b in D.PAIR_BASES]
    return out


def restore(mvx):
    mvx.set_launch(SL.DEFAULT_CAP, SL.DEFAULT_NT_LOG2)
