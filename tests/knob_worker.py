#!/usr/bin/env python3
"""TEST HELPER: one group of kernel-selecting environment knobs, in a fresh
process (libmvx_hip.so reads each knob once into a static).

Launched by tests/test_gpu_knobs.py with ENV[group] added to the environment:

  knob_worker.py GROUP

Runs small launches (tests/small_launch.py) or pack / unpack round trips
(tests/typemap_util.py), each compared with the CPU oracle bit for bit, and
checks the kernel the dispatch reports against what the knobs select
(config, choose_family and plan in mvx_ops.hip, kfam in mvx_ops_tab.h, pack
in mvx_pack.hip).  Prints one line per check and, last, `knobs ok <n>
checks`; any failure is an uncaught exception (non-zero exit).

Launched by tests/test_cpu_launch_plan.py, for the op-side groups only:

  knob_worker.py GROUP --plan

The same checks on what mvx_op_plan answers (small_launch.PLAN): nothing is
launched, no device and no torch are needed.  The groups take the runner as
their last argument, small_launch itself or small_launch.PLAN.  Without a
device the LDS reservations are sized for a 64 KiB part, so they are checked
as zero or not zero, never as a byte count.

Knobs that would hide one another sit in different groups: MVX_NO_BODY would
hide MVX_CHAIN_RT and MVX_PXI_U, MVX_PROG_GENERIC the fixed trees the
MVX_CAP_TREE reservation belongs to, MVX_PROG_U the 4-byte side of
MVX_PROG4, MVX_PACK_UNITS everything else on the datatype side.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]

ENV = {
    "prog_u": {"MVX_PROG_U": "2", "MVX_CHAIN_RT": "0", "MVX_NT_MIN_BYTES": "4096", "MVX_BLOCK_CAP": "2",
               "MVX_PXI_U": "2", "MVX_PXI_CAP": "3", "MVX_PXI_APPLY_CAP": "0"},
    "generic": {"MVX_PROG_GENERIC": "1"},
    "no_body": {"MVX_NO_BODY": "1", "MVX_PROG4": "0", "MVX_CAP_APPLY": "3", "MVX_CAP_PROG": "3",
                "MVX_CAP_TREE": "0"},
    "no_merge_no_tiles": {"MVX_UNPACK_MERGE": "0", "MVX_PACK_TILES": "0"},
    "no_tab_no_swizzle": {"MVX_UNPACK_CHUNK_TAB": "0", "MVX_PACK_CHUNK_TAB": "0", "MVX_LDS_SWIZZLE": "0"},
    "no_units": {"MVX_PACK_UNITS": "0"},
}
PLAN_GROUPS = ("prog_u", "generic", "no_body")      # the op side: also runs as `GROUP --plan`
# seconds per process: start-up (torch, the HIP runtime) and a few seconds of work
TIMEOUT = {"prog_u": 240, "generic": 240, "no_body": 240, "no_merge_no_tiles": 300, "no_tab_no_swizzle": 300,
           "no_units": 300}

SUM, PROD, MAX, BAND, MINLOC, MAXLOC = 102, 103, 100, 105, 110, 111
CHAR, INT, LONG, FLOAT, PXI = 1, 6, 8, 10, 22
TREE, CHAIN = 0, 1
NVEC = (1, 257, 513, 1025, 3372)             # whole 16-byte chunks, as test_gpu_small_launch.py
PXI_NVEC = (1, 127, 128, 129, 255, 257, 1000)

_checks = 0


def ok(what, cond, detail=""):
    global _checks
    if not cond:
        raise AssertionError("%s: %s" % (what, detail))
    _checks += 1
    print("ok %s %s" % (what, detail), flush=True)


def ends(sym, *tail):
    return sym.startswith("k_combine<") and sym.endswith(", " + ", ".join(str(t) for t in tail) + ">")


# ------------------------------------------------------------------ op side
# R: the runner -- small_launch (launches and checks bits) or small_launch.PLAN

def group_prog_u(mvx, oracle, R):
    # MVX_NT_MIN_BYTES=4096, MVX_BLOCK_CAP=2 -- first, before set_launch replaces them
    sym, blocks = R.apply(mvx, oracle, SUM, FLOAT, 341, seed=1)            # 4092 bytes of traffic
    ok("nt_min_bytes below", ends(sym, 2, 4, 0, 0), sym)
    sym, blocks = R.apply(mvx, oracle, SUM, FLOAT, 342, seed=2)            # 4104
    ok("nt_min_bytes at", ends(sym, 2, 4, 1, 0) and blocks <= 2, sym)
    sym, blocks = R.apply(mvx, oracle, SUM, FLOAT, 3 + 4 * 4099 + 2, offset=4, seed=3)
    ok("block_cap apply", ends(sym, 2, 4, 1, 0) and blocks == 2, "%s blocks %d" % (sym, blocks))
    sym, blocks = R.combine(mvx, SUM, FLOAT, 8, TREE, 4 * 3372, seed=4)
    ok("block_cap body", sym.startswith("k_tree_body<2, float, 8, 2>") and blocks == 2, "%s blocks %d" % (sym, blocks))
    # MVX_PROG_U=2: 4-byte types' programs at KMAX 8, U 2, both builds
    for nt in (0, 1):
        mvx.set_launch(0, 4 if nt else -1)
        for dtype in (FLOAT, INT):
            for k, shape, folded in ((5, TREE, False), (6, TREE, False), (7, TREE, False), (8, TREE, True),
                                     (3, TREE, False), (3, CHAIN, False)):
                for n, off in ((4 * 513, 0), (3 + 4 * 1 + 2, 4), (3 + 4 * 1025 + 2, 4)):
                    sym, blocks = R.combine(mvx, SUM, dtype, k, shape, n, offset=off, folded=folded, seed=k)
                    ok("prog_u", ends(sym, 8, 2, nt, 0) and blocks <= 2, "%s k %d n %d" % (sym, k, n))
        # an 8-byte type keeps its default kernels
        for n in (2 * 513, 2 * 1025 + 1):
            sym, _ = R.combine(mvx, SUM, LONG, 3, TREE, n, seed=3)
            ok("prog_u 8-byte k3", ends(sym, 4, 2, nt, 0), sym)
            sym, _ = R.combine(mvx, SUM, LONG, 6, TREE, n, seed=6)
            ok("prog_u 8-byte k6", ends(sym, 8, 1, nt, 0), sym)
    # MVX_CHAIN_RT=0: aligned chains of 5 to 7 leave the 8-leaf chain body
    for k in (5, 6, 7):
        for nvec in NVEC:
            sym, _ = R.combine(mvx, SUM, FLOAT, k, CHAIN, 4 * nvec, seed=k)
            ok("chain_rt f32", ends(sym, 8, 2, 1, 0), sym)
            sym, _ = R.combine(mvx, BAND, LONG, k, CHAIN, 2 * nvec, seed=k)
            ok("chain_rt i64", ends(sym, 8, 1, 1, 0), sym)
    for k in (4, 8):                          # which full chains keep
        sym, _ = R.combine(mvx, SUM, FLOAT, k, CHAIN, 4 * 1025, seed=k)
        ok("chain_rt full chain", sym == "k_chain_body<2, float, %d, 2>" % k, sym)
    # MVX_PXI_U=2 (MVX_PXI_CAP=3, MVX_PXI_APPLY_CAP=0: bits)
    for n in PXI_NVEC:
        sym, blocks = R.combine(mvx, MAXLOC, PXI, 8, TREE, n, seed=n, ties=0.3)
        ok("pxi_u", sym == "k_pxi_loc_body<11, 8, 2>" and blocks <= 2, "%s n %d" % (sym, n))
        sym, blocks = R.combine(mvx, MINLOC, PXI, 4, TREE, n, seed=n + 1, ties=0.3)
        ok("pxi_u", sym == "k_pxi_loc_body<10, 4, 2>" and blocks <= 2, "%s n %d" % (sym, n))
        for op in (MINLOC, MAXLOC):
            sym, _ = R.apply(mvx, oracle, op, PXI, n, seed=n, ties=0.3)
            ok("pxi apply", sym == "k_pxi_loc_body<%d, 2, 1>" % (op - 100), sym)
            ok("pxi_apply_cap", R.launched_lds(mvx) == 0, "dynamic LDS %d" % R.launched_lds(mvx))


def group_generic(mvx, oracle, R):
    # MVX_PROG_GENERIC=1: no fixed-tree kernel and no body kernel
    for nt in (1, 0):
        mvx.set_launch(0, 4 if nt else -1)
        for op, dtype in ((SUM, FLOAT), (BAND, LONG), (MAX, CHAR)):
            E = mvx.dtype_info(dtype)[0]
            for nvec in NVEC:
                for shape in (TREE, CHAIN):
                    sym, _ = R.combine(mvx, op, dtype, 8, shape, nvec * 16 // E, seed=nvec % 5)
                    ok("generic k8", ends(sym, 8, 1, nt, 0), sym)
                    sym, _ = R.combine(mvx, op, dtype, 4, shape, nvec * 16 // E, seed=nvec % 3)
                    ok("generic k4", ends(sym, 4, 2, nt, 0), sym)
            for k in (5, 6, 7):
                sym, _ = R.combine(mvx, op, dtype, k, CHAIN, 1025 * 16 // E, seed=k)
                ok("generic chain", ends(sym, 8, 1, nt, 0), sym)


def group_no_body(mvx, oracle, R):
    mvx.set_launch(0, 4)
    # MVX_NO_BODY=1; MVX_CAP_TREE=0 / MVX_CAP_PROG=3 / MVX_CAP_APPLY=3: the reservation, and bits
    for op, dtype in ((SUM, FLOAT), (BAND, LONG), (PROD, 2)):
        E = mvx.dtype_info(dtype)[0]
        for nvec in NVEC:
            for k in (4, 8):
                sym, _ = R.combine(mvx, op, dtype, k, TREE, nvec * 16 // E, seed=k)
                ok("no_body tree", ends(sym, k, 2, 1, 1) and R.launched_lds(mvx) == 0, sym)
                sym, _ = R.combine(mvx, op, dtype, k, CHAIN, nvec * 16 // E, seed=k)
                ok("no_body chain", ends(sym, 8, 1, 1, 0) and R.launched_lds(mvx) > 0, sym)
    for n in PXI_NVEC:
        for op in (MINLOC, MAXLOC):
            sym, _ = R.apply(mvx, oracle, op, PXI, n, seed=n, ties=0.3)
            ok("no_body pxi apply", ends(sym, 2, 4, 1, 0) and R.launched_lds(mvx) > 0, sym)
            for k in (4, 8):
                sym, _ = R.combine(mvx, op, PXI, k, TREE, n, seed=n, ties=0.3)
                ok("no_body pxi tree", ends(sym, k, 1, 1, 1), sym)
    sym, _ = R.apply(mvx, oracle, SUM, FLOAT, 3 + 4 * 4099 + 2, offset=4, seed=5)
    ok("cap_apply", ends(sym, 2, 4, 1, 0) and R.launched_lds(mvx) > 0, "dynamic LDS %d" % R.launched_lds(mvx))
    # MVX_PROG4=0: three leaves (and four folded) on the KMAX = 8 program
    for dtype in (FLOAT, LONG):
        E = mvx.dtype_info(dtype)[0]
        for k, shape, folded in ((3, TREE, False), (3, CHAIN, False), (4, TREE, True), (4, CHAIN, True)):
            for n, off in ((513 * 16 // E, 0), (1 + 1025 * 16 // E, 0), (3 + 16 // E + 2, 4 if E == 4 else 8)):
                sym, _ = R.combine(mvx, SUM, dtype, k, shape, n, offset=off, folded=folded, seed=k)
                ok("prog4 off", ends(sym, 8, 1, 1, 0), sym)


# ------------------------------------------------------------ datatype side

def _type_runs(mvx, oracle):
    """(name, pack, pack 4 bytes off, unpack, unpack from 4 bytes off: the kernels) of every
    round trip: the whole-word list, one type of more than 2048 units, 30
    seeded random maps; counts 1, 3, 1000, 4099; origin phases 0 and 4."""
    import numpy as np

    import typemap_util as TM
    made = TM.whole_word_types(mvx, oracle) + TM.large_types(mvx, oracle)[:1]
    cases = [("list%d" % i, h) for i, h in enumerate(made)]
    rng = np.random.default_rng(777)
    for i in range(30):
        h, m = TM.random_type(mvx, oracle, rng)
        made += m
        cases.append(("rand%d" % i, h))
    runs = []
    for name, h in cases:
        for n in (1, 3, 1000, 4099):
            for phase in (0, 4):
                syms = TM.roundtrip(mvx, oracle, h, n, phase, seed=h)
                runs.append((name,) + syms)
                ok("roundtrip %s n %d phase %d" % (name, n, phase), True, " | ".join(syms))
    TM.free_all(mvx, oracle, made)
    return runs, TM


def group_no_merge_no_tiles(mvx, oracle, SL):
    runs, TM = _type_runs(mvx, oracle)
    ok("unpack_merge off", not any(s.startswith("k_unpack_merge") for r in runs for s in r[1:]))
    ok("pack_tiles off", not any(s.startswith("k_pack_tiles") for r in runs for s in r[1:]))
    # what the aligned streams run instead
    ok("unit unpack ran", any(r[3].startswith("k_pack_units<false, ") for r in runs))
    ok("piece unpack ran", any(r[3] == "k_pack<false>" for r in runs))
    ok("unit pack ran", any(r[1].startswith("k_pack_units<true, ") for r in runs))
    ok("piece pack ran", any(r[1] == "k_pack<true>" for r in runs))


def group_no_tab_no_swizzle(mvx, oracle, SL):
    runs, TM = _type_runs(mvx, oracle)
    seen = {"k_unpack_merge": set(), "k_pack_tiles": set()}
    for r in runs:
        name = r[0]
        for s in r[1:]:
            kern, a = TM.parse_symbol(s)
            if kern in seen:
                if not (a["TAB"] is False and a["SWZ"] is False):
                    raise AssertionError("%s ran %s" % (name, s))
                seen[kern].add(a["W"])
    ok("chunk tables and swizzle off in every unpack", {1, 2} <= seen["k_unpack_merge"], sorted(seen["k_unpack_merge"]))
    ok("chunk tables and swizzle off in every pack", {1, 2} <= seen["k_pack_tiles"], sorted(seen["k_pack_tiles"]))


def group_no_units(mvx, oracle, SL):
    runs, TM = _type_runs(mvx, oracle)
    ok("pack_units off", all(s in ("k_pack<true>", "k_pack<false>") for r in runs for s in r[1:]))


def main():
    import faulthandler
    import importlib
    faulthandler.enable()
    group = sys.argv[1]
    plan_only = sys.argv[2:] == ["--plan"]
    assert plan_only or not sys.argv[2:], sys.argv
    for name, val in ENV[group].items():      # the knobs must come from the environment
        assert os.environ.get(name) == val, (name, os.environ.get(name))
    for other in ENV.values():
        for name in other:
            assert name in ENV[group] or name not in os.environ, "stray knob %s" % name
    import small_launch as SL
    from oracle import oracle as O
    O.lib()
    mvx = importlib.import_module("mvapich-cce_amd")
    if plan_only:
        assert group in PLAN_GROUPS, group
    globals()["group_" + group](mvx, O, SL.PLAN if plan_only else SL)
    print("knobs ok %d checks" % _checks, flush=True)


if __name__ == "__main__":
    main()
