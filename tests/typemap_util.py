"""TEST HELPER: derived-type builders and the guarded pack / unpack check,
shared by tests/test_gpu_types.py and tests/knob_worker.py."""
import re

import numpy as np

import mvxtest as T

I, D, F, C, B, S = 6, 11, 10, 1, 3, 4       # MPI_INT, DOUBLE, FLOAT, CHAR, BYTE, SHORT
GUARD = 256


def both(mvx, oracle, ctor, *args):
    """The type built identically on both sides (the handles agree), committed."""
    rm, hm = getattr(mvx, "MPI_Type_" + ctor)(*args)
    ro, ho = getattr(oracle, "type_" + ctor)(*args)
    assert rm == ro == 0 and hm == ho, (ctor, args, rm, ro)
    assert mvx.MPI_Type_commit(hm) == 0 and oracle.type_commit(ho) == 0
    return hm


def free_all(mvx, oracle, made):
    for h in reversed(list(made)):
        mvx.MPI_Type_free(h)
        oracle.type_free(h)


def whole_word_types(mvx, oracle):
    """Types whose maps leave holes inside 64-byte sectors (whole-word unpack,
    tiled pack): 8-, 4-, 2- and 1-byte units, one reaching below its origin."""
    return [
        both(mvx, oracle, "vector", 8, 1, 4, D),              # 8 B of every 32
        both(mvx, oracle, "vector", 2, 1, 2, F),              # every other float
        both(mvx, oracle, "struct", 2, [1, 1], [0, 8], [I, D]),  # {int; hole; double}
        both(mvx, oracle, "hvector", 3, 1, -20, I),           # reaches below the origin
        both(mvx, oracle, "hindexed", 3, [1, 2, 1], [0, 12, 40], F),
        both(mvx, oracle, "vector", 2, 1, 2, C),              # every other byte (1-byte units)
        both(mvx, oracle, "struct", 2, [1, 1], [0, 4], [C, I]),  # {char; hole; int}
        both(mvx, oracle, "hvector", 3, 1, 6, S),             # shorts 6 bytes apart (2-byte units)
        both(mvx, oracle, "hindexed", 3, [3, 1, 2], [1, 9, 13], C),   # bytes from 1, odd spans
    ]


def large_types(mvx, oracle):
    """More than 2048 units per element: 2 chars of every 3, 1100 and 1400
    blocks (extents 3299 and 4199 bytes; the first within the LDS-swizzle
    model's reach)."""
    return [
        both(mvx, oracle, "hindexed", 1100, [2] * 1100, [3 * i for i in range(1100)], C),
        both(mvx, oracle, "hindexed", 1400, [2] * 1400, [3 * i for i in range(1400)], C),
    ]


def row_types(mvx, oracle):
    """Types that reach what the two lists above leave out of launch_merge's
    and launch_tiles' kernel choice (mvx_pack.hip)."""
    return [
        both(mvx, oracle, "hvector", 2, 2, 32, D),            # 16 B of every 32: 16-byte units
        # 3 chars of every 4, 2100 units in 2799 bytes: offsets from global
        # memory, and inside the swizzle model's reach with conflicts to save
        both(mvx, oracle, "hindexed", 700, [3] * 700, [4 * i for i in range(700)], C),
        # every other byte, 129 units: a chunk table would take 129 phases x
        # 16 entries (> 2048), so the 1-byte units step through LDS offsets
        both(mvx, oracle, "vector", 129, 1, 2, C),
    ]


def revisiting_types(mvx, oracle):
    """[(handle, byte offsets of one element's map in packed order)]: maps
    that read bytes more than once (legal for a send, meaningless for a
    receive: pack only).  Only such a map puts more units than bytes into an
    element's hull, which the tiled pack needs for its remaining kernel rows:
    more than 2048 units in a hull of at most 2048 bytes, or 1-byte units
    without a chunk table in an element small enough for 64 to share a tile."""
    out = []
    for cnt, mod, step, base, esz in ((129, 50, 2, C, 1),       # 129 x 1 B in 99 bytes
                                      (2200, 400, 2, C, 1),     # 2200 x 1 B in 799 bytes
                                      (2100, 301, 1, F, 4)):    # 2100 x 4 B in 1204 bytes
        displs = [step * esz * (i % mod) for i in range(cnt)]
        h = both(mvx, oracle, "hindexed", cnt, [1] * cnt, displs, base)
        out.append((h, np.concatenate([np.arange(d, d + esz) for d in displs])))
    return out


def pack_only(mvx, h, offsets, n, phase, seed=0):
    """Pack n elements of a revisiting type into an aligned packed buffer and
    one 4 bytes off: both equal the stream gathered in numpy from the byte
    offsets.  Returns the two kernels."""
    import torch
    ext = mvx.MPI_Type_extent(h)[1]
    size = mvx.MPI_Type_size(h)[1]
    assert size == offsets.size and offsets.min() >= 0
    off = GUARD + phase
    nb = off + (n - 1) * ext + int(offsets.max()) + 1 + GUARD
    x = np.random.default_rng(n * 5 + phase + 17 * seed).integers(0, 256, nb, dtype=np.uint8)
    want = x[off + (np.arange(n)[:, None] * ext + offsets[None, :])].reshape(-1)
    dx = torch.from_numpy(x).cuda()
    syms = []
    for shift in (0, 4):
        dp = torch.full((n * size + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
        assert mvx.type_pack(h, dx.data_ptr() + off, dp.data_ptr() + GUARD + shift, n) == 0
        syms.append(mvx.type_last_kernel_symbol())
        got = T.from_dev(dp)
        lo = GUARD + shift
        assert np.array_equal(got[lo:lo + n * size], want), (syms[-1], n, phase)
        assert (got[:lo] == 0x5A).all() and (got[lo + n * size:] == 0x5A).all(), (syms[-1], n, phase, "guards")
    return tuple(syms)


def random_type(mvx, oracle, rng):
    """A random hindexed / struct type of 1-, 2-, 4- and 8-byte pieces:
    blocks in random order (the type map's order is the packed order),
    gaps, sometimes reaching below the origin, sometimes nested in an
    hvector whose stride leaves a gap.  Returns the handles to free."""
    base = [(C, 1), (B, 1), (4, 2), (I, 4), (F, 4), (D, 8)]
    nb = int(rng.integers(1, 6))
    kind = "struct" if rng.random() < 0.4 else "hindexed"
    if kind == "hindexed":
        bt, bs = base[int(rng.integers(len(base)))]
        types = [bt] * nb
        sizes = [bs] * nb
    else:
        pick = [base[int(i)] for i in rng.integers(len(base), size=nb)]
        types = [p[0] for p in pick]
        sizes = [p[1] for p in pick]
    lens = [int(x) for x in rng.integers(1, 5, size=nb)]
    displs, cur = [], 0
    for s, ln in zip(sizes, lens):
        cur += int(rng.integers(0, 4)) * s          # a gap of whole pieces
        cur = (cur + s - 1) // s * s
        displs.append(cur)
        cur += s * ln
    if rng.random() < 0.25:                         # reach below the origin
        shift = 8 * int(rng.integers(1, 4))
        displs = [d - shift for d in displs]
    order = rng.permutation(nb)
    displs = [displs[i] for i in order]
    lens = [lens[i] for i in order]
    types = [types[i] for i in order]
    if kind == "hindexed":
        h = both(mvx, oracle, "hindexed", nb, lens, displs, types[0])
    else:
        h = both(mvx, oracle, "struct", nb, lens, displs, types)
    made = [h]
    if rng.random() < 0.3:
        ext = mvx.MPI_Type_extent(h)[1]
        stride = ext + 8 * int(rng.integers(0, 3))
        h = both(mvx, oracle, "hvector", int(rng.integers(2, 4)), 1, stride, h)
        made.append(h)
    return h, made


def roundtrip(mvx, oracle, h, n, phase, seed=0):
    """Pack n elements whose origin sits `phase` bytes off a 16-byte word into
    an aligned packed buffer and into one 4 bytes off (equal streams), unpack
    the aligned stream into a patterned buffer with guard bands and compare
    with the oracle's type-map copy: type-map bytes land, holes and guards
    keep their pattern; the same unpack from the stream 4 bytes off.  Returns
    the launched kernels (mvx_type_last_kernel_symbol) as (aligned pack, pack
    4 bytes off, unpack, unpack from 4 bytes off)."""
    import torch
    ext = mvx.MPI_Type_extent(h)[1]
    size = mvx.MPI_Type_size(h)[1]
    L = mvx.type_layout(h)
    lo = min(0, L["span_lo"])
    off = GUARD + phase - lo
    off += -(off - phase) % 16                       # the origin exactly `phase` off the grid
    nb = off + (n - 1) * ext + L["span_hi"] + GUARD
    rng = np.random.default_rng(n * 7 + phase + 31 * seed)
    x = rng.integers(0, 256, nb, dtype=np.uint8)
    y0 = rng.integers(0, 256, nb, dtype=np.uint8)
    dx = torch.from_numpy(x).cuda()
    dy = torch.from_numpy(y0).cuda()
    dp = torch.zeros(max(n * size, 16), dtype=torch.uint8, device="cuda")
    dq = torch.zeros(max(n * size, 16) + 16, dtype=torch.uint8, device="cuda")
    assert dx.data_ptr() % 16 == 0 and dp.data_ptr() % 16 == 0 and dq.data_ptr() % 16 == 0
    assert mvx.type_pack(h, dx.data_ptr() + off, dp, n) == 0
    s_pack = mvx.type_last_kernel_symbol()
    assert mvx.type_pack(h, dx.data_ptr() + off, dq.data_ptr() + 4, n) == 0
    s_pack4 = mvx.type_last_kernel_symbol()
    assert torch.equal(dq[4:4 + n * size], dp[:n * size]), (s_pack, s_pack4, n, phase)
    assert mvx.type_unpack(h, dp, dy.data_ptr() + off, n) == 0
    s_unpack = mvx.type_last_kernel_symbol()
    ref = y0.copy()
    assert oracle.type_copy(ref[off:], x[off:], n, h) == 0
    got = T.from_dev(dy)
    assert np.array_equal(got, ref), (s_unpack, L, n, phase, np.flatnonzero(got != ref)[:8])
    # and from the packed copy 4 bytes off (no whole-word unpack there)
    dz = torch.from_numpy(y0).cuda()
    assert mvx.type_unpack(h, dq.data_ptr() + 4, dz.data_ptr() + off, n) == 0
    s_unpack4 = mvx.type_last_kernel_symbol()
    got = T.from_dev(dz)
    assert np.array_equal(got, ref), (s_unpack4, L, n, phase, np.flatnonzero(got != ref)[:8])
    return s_pack, s_pack4, s_unpack, s_unpack4


_SYM = re.compile(r"^(k_\w+)<(.*)>$")


def parse_symbol(sym):
    """("k_unpack_merge", dict(W=.., LDSU=.., SWZ=.., TAB=..)) of a tile
    kernel's symbol; other kernels give (name, {}) ("memcpy": ("memcpy", {}))."""
    m = _SYM.match(sym)
    if not m:
        return sym, {}
    name, args = m.group(1), [a.strip() for a in m.group(2).split(",")]
    tf = {"true": True, "false": False}
    if name == "k_unpack_merge":       # <W, TILE, LDSU, SWZ, TAB>
        assert args[1] == "8192", sym
        return name, dict(W=int(args[0]), LDSU=tf[args[2]], SWZ=tf[args[3]], TAB=tf[args[4]])
    if name == "k_pack_tiles":         # <W, TILE, LDSU, TAB, SWZ>
        assert args[1] == "8192", sym
        return name, dict(W=int(args[0]), LDSU=tf[args[2]], TAB=tf[args[3]], SWZ=tf[args[4]])
    if name == "k_pack_units":         # <PACK, W, U, LDS>
        assert args[2] == "4", sym
        return name, dict(PACK=tf[args[0]], W=int(args[1]), LDS=tf[args[3]])
    return name, {}
