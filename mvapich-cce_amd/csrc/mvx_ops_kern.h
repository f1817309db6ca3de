#pragma once
// mvx_ops_kern.h -- the kernels of the device side of the MPI local reduction
// path and what they take (Params, BodyParams), written for gfx950 (CDNA4,
// wave64).  The ops on elements and chunks are in mvx_ops_fn.h; the host-side
// tables that name every instantiation are in mvx_ops_tab.h, which mvx_ops.hip
// and the per-op table units mvx_ops_{cmp,arith,logic,loc,half,fp8,acc32,avg,scaled,sr}.hip include.
// Built into libmvx_hip.so; C-ABI in include/mvx_hip.h.
//
// One kernel template covers every predefined op x type of the reference
// (src/coll/global_ops.c:56-1745) and every combine order of its collectives
// (src/coll/intra_fns_new.c): a launch reads k leaf operands (optionally each
// pre-folded with a partner, the non-power-of-two fold of intra_fns_new.c
// 5548-5577 / 4641-4671 / 6283-6312), reduces them in registers by a small
// combine program (tree steps by level, then a chain; include/mvx_hip.h)
// whose left operand always plays the reference's `inoutvec` role, and
// writes the result once.  A k-way combine is one HBM pass instead
// of the reference's log2(p) or p-1 passes over the block.
//
// Element-wise: no MFMA, no LDS.  Every lane moves 16 bytes per operand per
// chunk (global_load_dwordx4), chunks are lane-contiguous so a wave touches
// 1 KiB per load instruction, several chunks per lane are in flight before
// the first use, and the store is one dwordx4 per chunk.  Pair types
// (MAXLOC/MINLOC) are 8 or 16 bytes, so a 16-byte lane load always holds
// whole pairs: no LDS transposition is needed.
//
// Numerics follow the reference's x86-64 gcc -O2 build: IEEE round-to-nearest
// f32/f64 with denormals (no flush), no contraction (-ffp-contract=off keeps
// the complex product of global_ops.c:518-519 unfused), MAX/MIN as the
// select `(b > a) ? b : a` of coll.h:14-19 (not v_max: NaN and signed-zero
// roles matter), integer arithmetic in unsigned form (the reference's signed
// wrap, without UB).
#include "mvx_hip.h"
#include "mvx_ops_fn.h"

namespace mvx {

// ---------------------------------------------------------------------------
// launch parameters (passed by value, ~180 bytes of kernarg)

struct Params {
    const char *src[MVX_COMBINE_KMAX];
    const char *fold[MVX_COMBINE_KMAX];
    char *dst;
    long n;      // elements
    long head;   // scalar elements before the 16-byte aligned body
    long nvec;   // chunks in the body (16 bytes, or one element if wider)
    int k;       // leaves
    int vec_ok;  // all pointers share their alignment mod 16
    unsigned tree_mask;   // bit l*8+q: y[q] = op(y[q], y[q + 2^l]), levels 0..2
    unsigned chain_mask;  // bit q (q >= 1): y[0] = op(y[0], y[q]) after the tree
    int divisor;          // OAVG alone reads it: the rank contributions of the whole program
};
// the scaled sum's kernels: the same, with its scales and amax word behind
struct SParams : Params {
    Scl sc;
};
// the stochastically rounded sum's: its seed and the index of dst[0] behind
struct RParams : Params {
    Sr sr;
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // one dwordx4

// whole-element store: the pair padding is an explicit member carried from
// leaf 0, so the element path writes the same bytes as the 16-byte path
template <typename T>
__device__ __forceinline__ void store_elt(T *d, const T &r) { *d = r; }

// The combine program.  KMAX = 2 is the plain op (y0 = y0 op y1); for
// KMAX = 8 every step is fixed at compile time and switched on by a
// wave-uniform mask bit, so the leaves stay in registers.
template <int O, typename T, int KMAX>
__device__ __forceinline__ void reduce_leaves(T (&y)[KMAX], int k, unsigned tree_mask,
                                              unsigned chain_mask)
{
    if constexpr (KMAX == 2) {
        if (k == 2) y[0] = F<O, T>::f(y[0], y[1]);
    } else {
#pragma unroll
        for (int l = 0; (1 << l) < KMAX; ++l) {
#pragma unroll
            for (int q = 0; q + (1 << l) < KMAX; ++q)
                if (tree_mask & (1u << (l * 8 + q))) y[q] = F<O, T>::f(y[q], y[q + (1 << l)]);
        }
#pragma unroll
        for (int q = 1; q < KMAX; ++q)
            if (chain_mask & (1u << q)) y[0] = F<O, T>::f(y[0], y[q]);
    }
}

// U = 16-byte chunks per lane per iteration (loads in flight per operand).
// NT = non-temporal loads and stores (global_load/store_dwordx4 ... nt): for
// a launch that streams far more than the 256 MiB Infinity Cache, keeping the
// once-touched lines out of the caches measured 6.59 vs 5.68 TB/s on the
// config-2 kernel (tools/tune_sum.hip, cold caches).
template <int NT>
__device__ __forceinline__ u32x4 ld(const u32x4 *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// OPAQUE: an empty asm makes the stored dwordx4 opaque first.  Where the
// value was assembled from narrower fields (the x87 types' 16-bit sign and
// exponent) the optimiser otherwise re-typed the store and dropped its
// non-temporal hint (the x87 MAXLOC / MINLOC trees stored cached); for the
// other types the store already keeps it and their code stays as measured.
template <int NT, bool OPAQUE = false>
__device__ __forceinline__ void st(u32x4 *p, u32x4 v)
{
    if constexpr (NT) {
        if constexpr (OPAQUE) __asm__("" : "+v"(v));
        __builtin_nontemporal_store(v, p);
    } else {
        *p = v;
    }
}

template <typename T, int NT>
__device__ __forceinline__ Chunk<T> ld_chunk(const u32x4 *base, long c)
{
    u32x4 r[CG<T>::w];
#pragma unroll
    for (int w = 0; w < CG<T>::w; ++w) r[w] = ld<NT>(base + c * CG<T>::w + w);
    Chunk<T> x;
    __builtin_memcpy(&x, r, sizeof x);
    return x;
}

template <typename T, int NT>
__device__ __forceinline__ void st_chunk(u32x4 *base, long c, const Chunk<T> &x)
{
    u32x4 r[CG<T>::w];
    __builtin_memcpy(r, &x, sizeof x);
#pragma unroll
    for (int w = 0; w < CG<T>::w; ++w) st<NT, alu_heavy<T>::v>(base + c * CG<T>::w + w, r[w]);
}

// The f32-accumulating ops' batch x[U][KMAX] of loaded chunks: the fold
// partners' chunks are kept, and each chunk's program -- folds included -- is
// evaluated in f32 (acc_chunk), the result left in x[u][0].
template <int O, typename T, int KMAX, int U, int NT, int PROG>
__device__ __forceinline__ void batch_acc(Chunk<T> (&x)[U][KMAX], const u32x4 *(&fold)[KMAX], long c0,
                                          long nvec, int k, unsigned tree_mask, unsigned chain_mask, int divisor)
{
    Chunk<T> xf[U][KMAX];
    unsigned fmask = 0;
    if constexpr (PROG == 0) {
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (q < k && fold[q]) {
                fmask |= 1u << q;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const long c = c0 + (long)u * 256;
                    if (c < nvec) xf[u][q] = ld_chunk<T, NT>(fold[q], c);
                }
            }
        }
    }
    // a lone leaf is copied as it is (scalar_elem_acc)
    if (PROG == 0 && k == 1 && !fmask && (O != OAVG || divisor == 1)) return;
#pragma unroll
    for (int u = 0; u < U; ++u) acc_chunk<O, T, KMAX, PROG>(x[u], xf[u], fmask, k, tree_mask, chain_mask, divisor);
}

// OSCL's batch_acc, through scl_chunk: the amax of the chunks inside the body
// goes into am (chunks past the end are computed on unloaded registers, and
// count for nothing).
template <typename T, int KMAX, int U, int NT, int PROG>
__device__ __forceinline__ void batch_scl(Chunk<T> (&x)[U][KMAX], const u32x4 *(&fold)[KMAX], long c0,
                                          long nvec, int k, unsigned tree_mask, unsigned chain_mask,
                                          const Scl &sc, unsigned &am)
{
    Chunk<T> xf[U][KMAX];
    unsigned fmask = 0;
    if constexpr (PROG == 0) {
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (q < k && fold[q]) {
                fmask |= 1u << q;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const long c = c0 + (long)u * 256;
                    if (c < nvec) xf[u][q] = ld_chunk<T, NT>(fold[q], c);
                }
            }
        }
    }
    // a lone leaf that no scale touches is copied as it is (scalar_elem_scl); it still counts for amax
    if (PROG == 0 && k == 1 && !fmask && scl_unit(sc)) {
        if (sc.amax) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned m = amax_chunk(x[u][0]);
                if (c0 + (long)u * 256 < nvec) am = m > am ? m : am;
            }
        }
        return;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const unsigned m = scl_chunk<T, KMAX, PROG>(x[u], xf[u], fmask, k, tree_mask, chain_mask, sc);
        if (c0 + (long)u * 256 < nvec) am = m > am ? m : am;
    }
}

// OSR's batch_acc, through sr_chunk: chunk c of the body begins at element i0 +
// c * V of the reduced vector, o elements into a group of L (sr_word_bits).
template <typename T, int KMAX, int U, int NT, int PROG>
__device__ __forceinline__ void batch_sr(Chunk<T> (&x)[U][KMAX], const u32x4 *(&fold)[KMAX], long c0,
                                         long nvec, int k, unsigned tree_mask, unsigned chain_mask,
                                         const Sr &sr, uint64_t i0, int o, SrC &cc)
{
    Chunk<T> xf[U][KMAX];
    unsigned fmask = 0;
    if constexpr (PROG == 0) {
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (q < k && fold[q]) {
                fmask |= 1u << q;
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const long c = c0 + (long)u * 256;
                    if (c < nvec) xf[u][q] = ld_chunk<T, NT>(fold[q], c);
                }
            }
        }
    }
    // a lone leaf is copied as it is (scalar_elem_sr)
    if (PROG == 0 && k == 1 && !fmask) return;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        uint32_t rb[4];
        sr_word_bits<T, 4>(sr, i0 + (uint64_t)(c0 + (long)u * 256) * CG<T>::v, o, cc, rb);
        sr_chunk<T, KMAX, PROG>(x[u], xf[u], fmask, k, tree_mask, chain_mask, rb);
    }
}

// The fixed full tree over the aligned body only: what a large C3 / C5
// combine is once the plan's blocks are 16-byte aligned and whole (no head,
// no tail, no folded leaves).  Its prologue is a handful of scalar loads
// (k_combine's head / tail / misalignment paths are gone), which matters at
// the few resident blocks per CU the residency cap leaves
// (tools/tune_occ.hip: the same loop behind k_combine's prologue ran 2 us
// slower per 50 us launch).
struct BodyParams {
    const u32x4 *src[8];
    u32x4 *dst;
    long nvec;   // chunks
    int k;       // leaves (k_chain_body<..., 8, ...>: 5 to 8)
    int divisor; // Params::divisor
};
struct SBodyParams : BodyParams {
    Scl sc;      // SParams::sc (no leaf of a body launch is folded: fscale is not read)
};
struct RBodyParams : BodyParams {
    Sr sr;       // RParams::sr (a body launch has no head: chunk c begins at element sr.first + c * V)
};

// 56 KiB of static LDS per block: 2 resident blocks (8 waves) per CU.
// tools/tune_occ.hip, profiles/r02/tune_occ_lds.jsonl: the 8-leaf f32 tree
// at U = 2 runs 47.8 / 94.5 us (8 x 32 / 64 MiB leaves, 79 / 80 % of HBM
// peak) at 2 blocks per CU against 50.0 / 100.3 us at 3, 4 or 5 -- fewer,
// fuller waves keep each HBM channel on fewer rows.  (LDS reservations of
// 41-52 KiB, which the runtime's occupancy query calls 3 blocks per CU, run
// like 3; 53 KiB and up like 2.)
#define BODY_LDS_CAP (56 * 1024)
#ifndef BODY_ST_NT
#define BODY_ST_NT 1   // non-temporal result stores (cached: C4 204.8 -> 215.0 us, C5 96.1 -> 97.1, C3 unchanged)
#endif

template <typename T, int DIR>
__device__ __forceinline__ float ld_f32side(const char *p, long i)
{
    if constexpr (DIR == 0) return widen_elt(reinterpret_cast<const T *>(p) + i);
    else return reinterpret_cast<const float *>(p)[i];
}

// ---------------------------------------------------------------------------
// The kernels that take Params / BodyParams are defined in mvx_ops_kern_def.h,
// which is read three times: once for every op there was (MVX_KP = Params), once
// more for the scaled sum, whose kernels take the same structs with its
// scales behind (SParams, SBodyParams) as overloads of the same templates, and
// once for the stochastically rounded sum (RParams, RBodyParams: its seed and
// first index).
// A field added to Params itself moves the hidden arguments behind it into
// another cache line of the kernarg segment, which every launch of every
// kernel then fetches (0.3 us a launch on the 256 MiB MPI_SUM); and a body
// function shared by two thin kernels compiles to other code than the kernel
// did.  Read again, the existing kernels stay what they were, byte for byte.
#define MVX_KP Params
#define MVX_KBP BodyParams
#include "mvx_ops_kern_def.h"
#undef MVX_KP
#undef MVX_KBP
#define MVX_KP SParams
#define MVX_KBP SBodyParams
#include "mvx_ops_kern_def.h"
#undef MVX_KP
#undef MVX_KBP
#define MVX_KP RParams
#define MVX_KBP RBodyParams
#include "mvx_ops_kern_def.h"
#undef MVX_KP
#undef MVX_KBP

// MPI_LONG_DOUBLE_INT MAXLOC / MINLOC (global_ops.c:1365-1378 / 1605-1618)
// as lane PAIRS.  An element is 32 bytes: the x87 value in the first 16
// (significand, sign / exponent, slot padding), the int loc and padding in
// the second.  One element per lane made every load instruction touch 2 KiB
// with half of each 128-byte line (the tree ran at 65 % of HBM peak whatever
// its occupancy, profiles/r03/bench_kernels_x87_cap_sweep.jsonl); here lane
// 2j holds the value half of element j and lane 2j+1 its loc half, so each
// load and store is 1 KiB contiguous per wave.  The even lane compares, one
// DPP quad permutation hands the result to its odd partner, and each lane
// selects its own half: value and sign / exponent from the winner with a's
// slot padding (even), loc as the reference sets it (odd).
template <bool MIN>
__device__ __forceinline__ u32x4 loc_half(u32x4 a, u32x4 b, bool odd)
{
    xf80 va, vb;
    __builtin_memcpy(&va, &a, sizeof va);
    __builtin_memcpy(&vb, &b, sizeof vb);
    // meaningful in even lanes: 1 = b wins, 2 = equal values, 0 = keep a
    const xf::xord o = xf::order(va, vb);
    const bool win = !o.un & (MIN ? o.gt : !(o.gt | o.eq));
    int code = win ? 1 : ((!o.un & o.eq) ? 2 : 0);
    code = __builtin_amdgcn_update_dpp(0, code, 0xA0, 0xF, 0xF, false);   // quad_perm [0, 0, 2, 2]
    const bool take = code == 1;
    const int32_t la = (int32_t)a.x, lb = (int32_t)b.x;
    const uint32_t lsel = code == 2 ? (uint32_t)(la < lb ? la : lb) : (take ? b.x : a.x);
    u32x4 r = a;
    r.x = odd ? lsel : (take ? b.x : a.x);
    r.y = odd ? a.y : (take ? b.y : a.y);
    r.z = odd ? a.z : (take ? ((b.z & 0xffffu) | (a.z & 0xffff0000u)) : a.z);
    return r;
}

// the full tree over KMAX leaves; BodyParams.nvec counts elements (32 B)
template <int O, int KMAX, int U>
__global__ void __launch_bounds__(256)
k_pxi_loc_body(const BodyParams P)
{
    // the launch may reserve dynamic LDS to cap resident blocks per CU
    extern __shared__ char lds_cap[];
    if (P.nvec < 0) lds_cap[threadIdx.x] = 0;
    constexpr bool MIN = O == OMINLOC;
    const long n = 2 * P.nvec;                 // 16-byte halves; even, so pairs stay whole
    const bool odd = threadIdx.x & 1;
    const long nthr = (long)gridDim.x * 256;
    for (long c0 = (long)blockIdx.x * (256 * U) + threadIdx.x; c0 < n; c0 += nthr * U) {
        u32x4 x[U][KMAX];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long c = c0 + (long)u * 256;
            if (c < n)
#pragma unroll
                for (int q = 0; q < KMAX; ++q) x[u][q] = ld<1>(P.src[q] + c);
        }
        // every lane runs the tree (lanes past the end on unloaded
        // registers, never stored), so the DPP partner is always active
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int h = 1; h < KMAX; h <<= 1)
#pragma unroll
                for (int q = 0; q + h < KMAX; q += 2 * h) x[u][q] = loc_half<MIN>(x[u][q], x[u][q + h], odd);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long c = c0 + (long)u * 256;
            if (c < n) st<BODY_ST_NT, true>(P.dst + c, x[u][0]);
        }
    }
}

}  // namespace mvx
