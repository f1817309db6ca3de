"""CPU: the launch matrix of tests/kernel_matrix.py is complete, and the edge
operands of tests/edge_values.py are what they claim -- no device.

Completeness: every kernel symbol mvx_op_plan can answer, over every defined
(op, handle) -- the reference's table, the contiguous count-2 types, the
extension types -- every family, placement and build, is produced by one of
the matrix's own launches, planned.  Excused are only the extension types'
kernels, which their own files launch family by family (EXTENSION_FILES), and
the kernels an environment knob alone selects (KNOB_ONLY), which the default
planner never answers with and tests/knob_worker.py covers.  A kernel set
added to mvx_ops_tab.h without a case in kernel_matrix.SETS fails here.

The edge lists are checked by bit-pattern predicates; the NaN-exempt share of
the oracle's SUM and PROD results is held under edge_values.NAN_CAP for every
launch of the matrix, here as well as before each launch on the device.
"""
import os
import re

import numpy as np
import pytest

import derived_util as D
import edge_values as EV
import kernel_matrix as KM
import mvxtest as T
import small_launch as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the extension types' element spellings, and where every family of theirs is launched
EXTENSION_FILES = {"_Float16": "tests/test_gpu_half_ops.py", "mvx::bf16": "tests/test_gpu_half_ops.py",
                   "mvx::f8e4m3": "tests/test_gpu_fp8_ops.py", "mvx::f8e5m2": "tests/test_gpu_fp8_ops.py"}
ACC32_FILE = "tests/test_gpu_acc32_ops.py"      # O = 12, 13 on the same four types
# kernels only an environment knob selects (mvx_ops_tab.h Config); tests/knob_worker.py launches them
KNOB_ONLY = [
    re.compile(r"k_combine<\d+, (float|int|unsigned int|mvx::flog), 8, 2, [01], 0>"),    # MVX_PROG_U=2: KSet::prog2
    re.compile(r"k_pxi_loc_body<\d+, [48], 2>"),                                          # MVX_PXI_U=2
]
EXT_TYPES = [64, 65, 72, 73]


@pytest.fixture(scope="module")
def handles(mvx, oracle):
    H = KM.Handles(mvx, oracle)
    yield H
    H.free()
    KM.restore(mvx)


def _all_families():
    return KM.FAMILIES + [f for f in KM.BODIES if f not in KM.FAMILIES]


def _enumerate(mvx, handles):
    """{symbol: (op, handle)} over everything that can be planned."""
    specs = [("h", h) for h in T.ALL_TYPES + EXT_TYPES] + [("c2", b) for b in D.PAIR_BASES]
    seen = {}
    for op in T.ALL_OPS + [164, 165]:
        for spec in specs:
            h = handles(spec)
            if not mvx.hip().mvx_op_supported(op, h):
                continue
            E = mvx.dtype_info(h)[0]
            for fam in _all_families():
                _, k, shape, folded = fam[:4]
                for placement in (KM.ALIGNED, KM.SHIFTED, KM.MISALIGNED):
                    for nt in (1, 0):
                        mvx.set_launch(SL.DEFAULT_CAP, 4 if nt else -1)
                        for nvec in (1, 257):
                            n, offset = KM._size(E, placement, nvec, k)
                            sym, _ = SL.plan_combine(mvx, op, h, k, shape, n, offset=offset, folded=folded,
                                                     misalign=placement == KM.MISALIGNED)
                            seen.setdefault(sym, (op, spec))
    return seen


def _matrix_symbols(mvx, oracle, handles, sets):
    out = {}
    for sc in sets:
        h = handles(sc.spec)
        for part in ("combine", "body"):
            for L in KM.launches(sc, part):
                out.setdefault(KM.run(mvx, oracle, SL.PLAN, sc, h, L), (KM.set_id(sc), L.fam))
    return out


def _excused(sym):
    m = re.match(r"\w+<(\d+), ([^,]+(?:<[^>]*>)?)", sym)
    if m and (m.group(2) in EXTENSION_FILES or int(m.group(1)) in (12, 13)):
        path = ACC32_FILE if int(m.group(1)) in (12, 13) else EXTENSION_FILES[m.group(2)]
        assert os.path.exists(os.path.join(ROOT, path)), path
        return True
    return False


def test_every_plannable_kernel_has_a_matrix_case(mvx, oracle, handles):
    seen = _enumerate(mvx, handles)
    ours = _matrix_symbols(mvx, oracle, handles, KM.SETS)
    assert not [s for s in seen if any(p.fullmatch(s) for p in KNOB_ONLY)], "a knob-only kernel under default knobs"
    missing = sorted(s for s in seen if s not in ours and not _excused(s))
    assert not missing, ("kernels no matrix case launches", len(missing), missing[:8], [seen[s] for s in missing[:8]])
    stray = sorted(s for s in ours if s not in seen)
    assert not stray, ("matrix symbols the enumeration never planned", stray[:8])
    native = [s for s in seen if not _excused(s)]
    ncases = sum(len(KM.launches(sc, p)) for sc in KM.SETS for p in ("combine", "body"))
    print("distinct symbols: %d planned, %d of the reference's types, all in the matrix; %d kernel sets, %d launches"
          % (len(seen), len(native), len(KM.SETS), ncases))
    assert len(KM.SETS) == 100 and len(set(KM.SETS)) == 100


def test_dropping_a_matrix_case_is_noticed(mvx, oracle, handles):
    """The completeness check has teeth: without one set, its kernels are missing."""
    seen = _enumerate(mvx, handles)
    gone = KM.SETS[37]
    ours = _matrix_symbols(mvx, oracle, handles, [sc for sc in KM.SETS if sc != gone])
    missing = [s for s in seen if s not in ours and not _excused(s)]
    assert missing and all(gone.tname in s for s in missing), (KM.set_id(gone), missing[:4])


def test_every_set_is_the_planners_and_handles_map_to_one(mvx, handles):
    """Each SETS entry's representative runs the set it names, and every
    defined (op, handle) runs some set of SETS (the handle sweep's kernels)."""
    mvx.set_launch(SL.DEFAULT_CAP, -1)
    cached = {KM.expected_symbol(sc, KM.FAMILIES[0], KM.MISALIGNED, 0) for sc in KM.SETS}
    assert len(cached) == len(KM.SETS)
    for op, specs in KM.sweep_pairs(mvx).items():
        for spec in specs:
            sym, _ = SL.plan_apply(mvx, None, op, handles(spec), 64, misalign=True)
            assert sym in cached, (op, spec, sym)


@pytest.mark.parametrize("part", ["combine", "body"])
def test_launch_bounds(part):
    """At most MAX_LAUNCHES launches per GPU test case, no operand above 64
    KiB, and the placements, builds and caps all occur."""
    combos = set()
    for sc in KM.SETS:
        Ls = KM.launches(sc, part)
        assert len(Ls) <= KM.MAX_LAUNCHES
        E = KM.esize(sc)
        for L in Ls:
            assert 0 < L.n * E <= EV.MAX_BYTES, L
            combos.add((L.fam, L.placement, L.nt, L.cap))
            if L.placement == KM.SHIFTED and E < 16:
                head = (16 - L.offset) // E
                assert 0 < L.offset < 16 and L.offset % E == 0 and head >= 1 and (L.n - head) % (16 // E) >= 1, L
        for fam in {L.fam for L in Ls}:
            assert {L.nt for L in Ls if L.fam == fam} == ({1} if part == "body" else {0, 1}), (KM.set_id(sc), fam)
    if part == "combine":
        for fam in KM.FAMILIES:
            for placement in (KM.ALIGNED, KM.SHIFTED, KM.MISALIGNED):
                assert {c[3] for c in combos if c[:2] == (fam[0], placement)} == set(KM.CAPS), (fam[0], placement)


# ------------------------------------------------------------- the edge values

def _bits(x):
    return x.view(np.uint32 if x.dtype.itemsize == 4 else np.uint64)


@pytest.mark.parametrize("ft", [np.float32, np.float64])
def test_float_edges_by_bit_pattern(ft):
    e = EV.float_edges(ft)
    _, eb, m = EV._fmt(ft)
    b = _bits(e).astype(object)
    sign, expo, frac = b >> (eb + m), (b >> m) & ((1 << eb) - 1), b & ((1 << m) - 1)
    X, B = (1 << eb) - 1, (1 << (eb - 1)) - 1
    cls = dict(zip(EV.FLOAT_EDGE_NAMES, zip(sign, expo, frac)))
    assert len(cls) == 24
    quiet = 1 << (m - 1)
    assert cls["+qnan"] == (0, X, quiet)
    s, x, f = cls["-qnan-payload"]
    assert (s, x) == (1, X) and f & quiet and f & (quiet - 1)            # quiet, with a payload
    assert cls["+inf"] == (0, X, 0) and cls["-inf"] == (1, X, 0)
    assert cls["+0"] == (0, 0, 0) and cls["-0"] == (1, 0, 0)
    assert cls["+minsub"] == (0, 0, 1) and cls["-minsub"] == (1, 0, 1) and cls["maxsub"] == (0, 0, (1 << m) - 1)
    assert cls["+minnorm"] == (0, 1, 0) and cls["-minnorm"] == (1, 1, 0) and cls["2minnorm"] == (0, 2, 0)
    assert cls["+max"] == (0, X - 1, (1 << m) - 1) and cls["-max"] == (1, X - 1, (1 << m) - 1)
    assert cls["max/2"] == (0, X - 2, (1 << m) - 1)
    assert cls["1+ulp"] == (0, B, 1) and cls["1-ulp"] == (0, B - 1, (1 << m) - 1) and cls["ulp/2"] == (0, B - m - 1, 0)
    assert cls["1"] == (0, B, 0) and cls["-1"] == (1, B, 0) and cls["-2"] == (1, B + 1, 0)
    assert cls["0.5"] == (0, B - 1, 0) and cls["1.5"] == (0, B, quiet) and cls["3"] == (0, B + 1, quiet)
    a, b2 = EV.cross(e)
    assert len({(int(x), int(y)) for x, y in zip(_bits(a), _bits(b2))}) == 576      # every value meets every value


@pytest.mark.parametrize("dt", [np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64])
def test_int_edges_by_bit_pattern(dt):
    w = 8 * np.dtype(dt).itemsize
    e = EV.int_edges(dt)
    bits = {int(x) for x in e.view(np.dtype("u%d" % (w // 8)))}
    top, ones = 1 << (w - 1), (1 << w) - 1
    assert {0, 1, 2, ones, top, top - 1, top >> 1, (top >> 1) - 1} <= bits
    assert {int("01" * (w // 2), 2), int("10" * (w // 2), 2)} <= bits
    info = np.iinfo(dt)
    assert info.min in e and info.max in e
    if info.min == 0:
        assert (e.astype(object) > top - 1).sum() >= 4                   # above the signed maximum
    else:
        assert -1 in e and (e < 0).sum() >= 4


PAIR_SPECS = [("h", h) for h in (17, 18, 19, 20, 21, 29, 32, 33)] + [("c2", b) for b in D.PAIR_BASES if b != 12]


def _relation(x, y):
    """0 equal, 1 less, 2 greater, 3 unordered."""
    with np.errstate(invalid="ignore"):
        return np.where(x == y, 0, np.where(x < y, 1, np.where(x > y, 2, 3)))


@pytest.mark.parametrize("spec", PAIR_SPECS, ids=lambda s: "%s%d" % s)
def test_pair_operands_relations_and_padding(spec):
    a, b = EV.operands(spec)
    rv, rl = _relation(a["v"], b["v"]), _relation(a["l"], b["l"])
    vkinds = (0, 1, 2, 3) if a["v"].dtype.kind == "f" else (0, 1, 2)
    for v in vkinds:
        for l in (0, 1, 2):
            assert ((rv == v) & (rl == l)).any(), ("value relation %d never meets loc relation %d" % (v, l))
    if a["l"].dtype.kind == "f":
        assert np.isnan(a["l"]).any() and np.isnan(b["l"]).any() and (rl == 3).any()      # a NaN loc is a case
    if spec[0] == "h" and spec[1] in EV.STRUCT_PAIRS:
        info = np.iinfo(np.int32)
        for x in (a["l"], b["l"]):
            assert info.min in x and info.max in x and (x < 0).any()
    pm = EV.pad_mask(a.dtype)
    assert int(pm.sum()) == {18: 4, 19: 4, 20: 2}.get(spec[1] if spec[0] == "h" else 0, 0)
    if pm.any():
        pa = a.view(np.uint8).reshape(len(a), -1)[:, pm]
        pb = b.view(np.uint8).reshape(len(b), -1)[:, pm]
        assert (pa != 0).all() and (pb != 0).all() and (pa != pb).all()
        assert len(np.unique(pa)) > 200                                   # random, not one filler byte
        for S, F in (EV.edge_leaves(111, spec, 5, True, 100, 3), EV.rand_leaves(111, spec, 5, True, 100, 3)):
            for x in S + [f for f in F if f is not None]:
                assert (x.view(np.uint8).reshape(len(x), -1)[:, pm] != 0).all()


@pytest.mark.parametrize("spec", [("h", 18), ("h", 19), ("h", 20)], ids=lambda s: "h%d" % s[1])
@pytest.mark.parametrize("op", [110, 111])
def test_oracle_leaves_the_inout_padding_alone(oracle, op, spec):
    """The reference's MAXLOC / MINLOC loops assign value and loc only: the
    result's padding is the inout operand's, whichever side wins."""
    a, b = EV.operands(spec)
    ref = T.clone(b)
    assert oracle.op(op, spec[1], SL._u8(a), SL._u8(ref), len(a)) == 0
    pm = EV.pad_mask(a.dtype)
    rows = lambda x: x.view(np.uint8).reshape(len(x), -1)
    assert np.array_equal(rows(ref)[:, pm], rows(b)[:, pm])
    took_in = (ref["v"] != b["v"]) | (ref["l"] != b["l"])
    assert took_in.any() and not np.array_equal(rows(ref)[took_in][:, pm], rows(a)[took_in][:, pm])


def test_complex_operands_have_at_most_one_nan_lane():
    for h, ft in ((23, np.float32), (24, np.float64)):
        a, b = EV.operands(("h", h))
        lanes = np.stack([a.view(ft)[0::2], a.view(ft)[1::2], b.view(ft)[0::2], b.view(ft)[1::2]])
        assert np.isnan(lanes).sum(0).max() == 1
        with np.errstate(all="ignore"):
            assert (np.isinf(lanes[0]) & (lanes[2] == 0)).any()                              # inf * 0
            assert (np.isinf(lanes[0]) & np.isinf(lanes[2]) & (lanes[0] != lanes[2])).any()    # inf - inf


def test_x87_operands_are_cut_not_changed():
    a, b = EV.operands(("h", 12), seed=5)
    fa, fb = T.xf_operands(4096, 5)
    assert len(a) == 2048 and a.nbytes <= EV.MAX_BYTES
    # the generator is seeded per call: the same classes, a smaller draw
    assert set(np.unique(fa["se"] & 0x7fff)) >= {0, 0x7fff} and {0, 0x7fff} <= set(np.unique(a.view(T.XF_DT)["se"] & 0x7fff))
    a, b = EV.operands(("h", 22))
    assert len(a) == 1024 and a.dtype.itemsize == 32
    a, b = EV.operands(("c2", 12))
    assert len(a) == 1024 and a.dtype.itemsize == 32 and (a["v"] == b["v"]).any()


FLOAT_SETS = [sc for sc in KM.SETS if EV.has_nan_rule(sc.op, sc.spec)]


@pytest.mark.parametrize("sc", FLOAT_SETS, ids=KM.set_id)
def test_nan_share_of_every_launch_is_capped(oracle, sc):
    """SUM / PROD on float, double and the complex types: at most NAN_CAP of
    the oracle's result lanes are NaN, for the two-operand cross and for every
    launch of the matrix (the same assertion runs before each device launch)."""
    assert len(FLOAT_SETS) == 8
    a, b = EV.operands(sc.spec)
    ref = T.clone(b)
    assert oracle.op(sc.op, sc.spec[1], SL._u8(a), SL._u8(ref), len(a)) == 0
    share = EV.nan_share(ref)
    print(KM.set_id(sc), "two operands: %.3f" % share)
    assert 0 < share <= EV.NAN_CAP                  # NaN results are there, and a minority
    worst = 0.0
    for part in ("combine", "body"):
        for L in KM.launches(sc, part):
            S, F = KM.leaves_of(sc, L)
            ref = KM.reference(oracle, sc, sc.spec[1], L, S, F)
            worst = max(worst, EV.nan_share(ref))
            KM.check_nan_cap(sc, ref, L)
    print(KM.set_id(sc), "worst launch: %.3f" % worst)


def test_sweep_covers_every_defined_pair(mvx, oracle, handles):
    """The handle sweep's list is the reference's table (oracle: rc 0) plus
    the contiguous count-2 types, and nothing undefined."""
    pairs = KM.sweep_pairs(mvx)
    n = 0
    for op in T.ALL_OPS:
        for h in T.ALL_TYPES:
            assert (T.oracle_rc(oracle, op, h) == 0) == (("h", h) in pairs[op]), (op, h)
        for spec in pairs[op]:
            assert len(EV.operands(spec)[0]) > 0
            assert T.oracle_rc(oracle, op, handles(spec)) == 0, (op, spec)
            n += 1
    print("defined pairs in the sweep:", n)
    assert n >= 166
