#pragma once
// mvx_ops_kern.h -- the kernels of the device side of the MPI local reduction
// path and what they take (Params, BodyParams), written for gfx950 (CDNA4,
// wave64).  The ops on elements and chunks are in mvx_ops_fn.h; the host-side
// tables that name every instantiation are in mvx_ops_tab.h, which mvx_ops.hip
// and the per-op table units mvx_ops_{cmp,arith,logic,loc,half,fp8,acc32}.hip include.
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
// launch parameters (passed by value, ~170 bytes of kernarg)

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

// the same element of every leaf through the f32-accumulating program
// (acc_op): widened, folded and combined in f32, narrowed once.  A single
// unfolded leaf has no step: it is copied, bits and all (a NaN's payload
// would not survive the way to f32 and back), as the per-step ops copy it.
template <int O, typename T, int KMAX>
__device__ __forceinline__ void scalar_elem_acc(const Params &P, long i)
{
    if (P.k == 1 && !P.fold[0]) {
        store_elt(reinterpret_cast<T *>(P.dst) + i, reinterpret_cast<const T *>(P.src[0])[i]);
        return;
    }
    float y[KMAX][1];
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
        if (q < P.k) {
            y[q][0] = widen_elt(reinterpret_cast<const T *>(P.src[q]) + i);
            if (P.fold[q]) y[q][0] = accf<O>(y[q][0], widen_elt(reinterpret_cast<const T *>(P.fold[q]) + i));
        }
    }
    acc_steps<O, KMAX, 1, 0>(y, P.k, P.tree_mask, P.chain_mask);
    narrow_elt(reinterpret_cast<T *>(P.dst) + i, y[0][0]);
}

template <int O, typename T, int KMAX>
__device__ __forceinline__ void scalar_elem(const Params &P, long i)
{
    if constexpr (acc_op<O>::v) {
        scalar_elem_acc<O, T, KMAX>(P, i);
    } else {
        T y[KMAX];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (q < P.k) {
                y[q] = reinterpret_cast<const T *>(P.src[q])[i];
                if (P.fold[q]) y[q] = F<O, T>::f(y[q], reinterpret_cast<const T *>(P.fold[q])[i]);
            }
        }
        reduce_leaves<O, T, KMAX>(y, P.k, P.tree_mask, P.chain_mask);
        store_elt(reinterpret_cast<T *>(P.dst) + i, y[0]);
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
                                          long nvec, int k, unsigned tree_mask, unsigned chain_mask)
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
    if (PROG == 0 && k == 1 && !fmask) return;     // a lone leaf is copied as it is (scalar_elem_acc)
#pragma unroll
    for (int u = 0; u < U; ++u) acc_chunk<O, T, KMAX, PROG>(x[u], xf[u], fmask, k, tree_mask, chain_mask);
}

// PROG = 0: the program comes from the masks (any chain of trees over
// k <= KMAX leaves); PROG = 1: the full balanced tree over exactly KMAX
// leaves, steps fixed at compile time -- the Allreduce / Reduce order at
// p = 4 and 8 (Rabenseifner), where the generic form evaluated and
// discarded 24 masked steps for the 7 the tree needs.
template <int O, typename T, int KMAX, int U, int NT, int PROG = 0>
__global__ void __launch_bounds__(256)
k_combine(const Params P)
{
    // the launch may reserve dynamic LDS to cap resident blocks per CU
    // (plan(), Config::cap_*); the kernel never uses it -- the reference here
    // (never taken) marks the kernel as one that takes dynamic LDS
    extern __shared__ char lds_cap[];
    if (P.n < 0) lds_cap[threadIdx.x] = 0;
    constexpr int V = CG<T>::v;
    const long tid = (long)blockIdx.x * 256 + threadIdx.x;
    const long nthr = (long)gridDim.x * 256;

    if (!P.vec_ok) {  // operands misaligned against each other: element loads
        for (long i = tid; i < P.n; i += nthr) scalar_elem<O, T, KMAX>(P, i);
        return;
    }
    {   // head and tail elements outside the aligned body
        const long tail0 = P.head + P.nvec * V;
        const long nscal = P.head + (P.n - tail0);
        for (long s = tid; s < nscal; s += nthr) {
            const long i = s < P.head ? s : tail0 + (s - P.head);
            scalar_elem<O, T, KMAX>(P, i);
        }
    }
    const u32x4 *src[KMAX];
    const u32x4 *fold[KMAX];
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
        src[q] = reinterpret_cast<const u32x4 *>(P.src[q] + P.head * (long)sizeof(T));
        fold[q] = P.fold[q] ? reinterpret_cast<const u32x4 *>(P.fold[q] + P.head * (long)sizeof(T)) : nullptr;
    }
    u32x4 *dst = reinterpret_cast<u32x4 *>(P.dst + P.head * (long)sizeof(T));
    const int k = P.k;
    const unsigned tmask = P.tree_mask, cmask = P.chain_mask;

    for (long c0 = (long)blockIdx.x * (256 * U) + threadIdx.x; c0 < P.nvec; c0 += nthr * U) {
        Chunk<T> x[U][KMAX];
        // issue every load of the iteration before the first use
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long c = c0 + (long)u * 256;
            if (c < P.nvec) {
#pragma unroll
                for (int q = 0; q < KMAX; ++q)
                    if (PROG == 1 || q < k) x[u][q] = ld_chunk<T, NT>(src[q], c);
            }
        }
        if constexpr (acc_op<O>::v) {
            batch_acc<O, T, KMAX, U, NT, PROG>(x, fold, c0, P.nvec, k, tmask, cmask);
        } else {
#pragma unroll
            for (int q = 0; q < KMAX; ++q) {
                // fixed trees are launched without folded leaves (mvx_op_program):
                // no branch between the loads and the tree keeps every load of
                // the iteration in flight before the first add
                if (PROG == 0 && q < k && fold[q]) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const long c = c0 + (long)u * 256;
                        if (c < P.nvec) {
                            const Chunk<T> f = ld_chunk<T, NT>(fold[q], c);
                            CF<O, T>::f(x[u][q], f);
                        }
                    }
                }
            }
            // the combine program: each wave-uniform step is tested once and
            // applied to all U*V elements of the batch (chunks past the end
            // compute on unloaded registers and are never stored)
            if constexpr (KMAX == 2) {
                if (k == 2) {
#pragma unroll
                    for (int u = 0; u < U; ++u)
                        CF<O, T>::f(x[u][0], x[u][1]);
                }
            } else if constexpr (PROG == 1) {
#pragma unroll
                for (int h = 1; h < KMAX; h <<= 1)
#pragma unroll
                    for (int q = 0; q + h < KMAX; q += 2 * h)
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            CF<O, T>::f(x[u][q], x[u][q + h]);
            } else {
#pragma unroll
                for (int l = 0; (1 << l) < KMAX; ++l) {
#pragma unroll
                    for (int q = 0; q + (1 << l) < KMAX; ++q) {
                        if (tmask & (1u << (l * 8 + q))) {
#pragma unroll
                            for (int u = 0; u < U; ++u)
                                CF<O, T>::f(x[u][q], x[u][q + (1 << l)]);
                        }
                    }
                }
#pragma unroll
                for (int q = 1; q < KMAX; ++q) {
                    if (cmask & (1u << q)) {
#pragma unroll
                        for (int u = 0; u < U; ++u)
                            CF<O, T>::f(x[u][0], x[u][q]);
                    }
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long c = c0 + (long)u * 256;
            if (c < P.nvec) st_chunk<T, NT>(dst, c, x[u][0]);
        }
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

template <int O, typename T, int KMAX, int U>
__global__ void __launch_bounds__(256)
k_tree_body(const BodyParams P)
{
    __shared__ char lds_cap[BODY_LDS_CAP];
    if (P.nvec < 0) lds_cap[threadIdx.x] = 0;
    const long nthr = (long)gridDim.x * 256;
    for (long c0 = (long)blockIdx.x * (256 * U) + threadIdx.x; c0 < P.nvec; c0 += nthr * U) {
        Chunk<T> x[U][KMAX];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long c = c0 + (long)u * 256;
            if (c < P.nvec)
#pragma unroll
                for (int q = 0; q < KMAX; ++q) x[u][q] = ld_chunk<T, 1>(P.src[q], c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long c = c0 + (long)u * 256;
            if (c < P.nvec) {
                if constexpr (acc_op<O>::v) {
                    acc_chunk<O, T, KMAX, 1>(x[u], x[u], 0u, KMAX, 0u, 0u);
                } else {
#pragma unroll
                    for (int h = 1; h < KMAX; h <<= 1)
#pragma unroll
                        for (int q = 0; q + h < KMAX; q += 2 * h)
                            CF<O, T>::f(x[u][q], x[u][q + h]);
                }
                st_chunk<T, BODY_ST_NT>(P.dst, c, x[u][0]);
            }
        }
    }
}

// The same over a full CHAIN ((y0 op y1) op y2) ..., the pairwise
// Reduce_scatter's order (C4: k = 4, p = 4).  The 8-leaf instantiation
// takes chains of 5 to 8 leaves (P.k, a wave-uniform test per leaf): the
// pairwise chains at p = 5, 6, 7, which otherwise run the masked program at
// one chunk per lane.
template <int O, typename T, int KMAX, int U>
__global__ void __launch_bounds__(256)
k_chain_body(const BodyParams P)
{
    __shared__ char lds_cap[BODY_LDS_CAP];
    if (P.nvec < 0) lds_cap[threadIdx.x] = 0;
    const int k = KMAX == 8 ? P.k : KMAX;
    const long nthr = (long)gridDim.x * 256;
    for (long c0 = (long)blockIdx.x * (256 * U) + threadIdx.x; c0 < P.nvec; c0 += nthr * U) {
        Chunk<T> x[U][KMAX];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long c = c0 + (long)u * 256;
            if (c < P.nvec)
#pragma unroll
                for (int q = 0; q < KMAX; ++q)
                    if (q < k) x[u][q] = ld_chunk<T, 1>(P.src[q], c);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long c = c0 + (long)u * 256;
            if (c < P.nvec) {
                if constexpr (acc_op<O>::v) {
                    acc_chunk<O, T, KMAX, 0>(x[u], x[u], 0u, k, 0u, (1u << k) - 2u);
                } else {
#pragma unroll
                    for (int q = 1; q < KMAX; ++q)
                        if (q < k) CF<O, T>::f(x[u][0], x[u][q]);
                }
                st_chunk<T, BODY_ST_NT>(P.dst, c, x[u][0]);
            }
        }
    }
}

// The masked program of an f32-accumulating op with one side in f32: what a
// program over more than 8 leaves is cut into (mvx_combine.c), its
// intermediates being f32 temporaries.  DIR = 0: narrow leaves (folds
// allowed), f32 result, not narrowed; DIR = 1: f32 leaves, the result narrowed
// once.  A lane takes one 32-bit word of each narrow operand against L floats
// of each f32 one (a dwordx4 for the 8-bit types, a dwordx2 for the 16-bit
// ones).  Params: head elements lead to nvec such words where the narrow
// side is 4-byte and the f32 side 4 * L-byte aligned (vec_ok), else every
// element goes alone.
template <typename T, int DIR>
__device__ __forceinline__ float ld_f32side(const char *p, long i)
{
    if constexpr (DIR == 0) return widen_elt(reinterpret_cast<const T *>(p) + i);
    else return reinterpret_cast<const float *>(p)[i];
}

template <int O, typename T, int DIR>
__global__ void __launch_bounds__(256)
k_combine_f32(const Params P)
{
    constexpr int L = Wide<T>::L;
    constexpr int KMAX = MVX_COMBINE_KMAX;
    typedef float fL __attribute__((ext_vector_type(L)));
    const long tid = (long)blockIdx.x * 256 + threadIdx.x;
    const long nthr = (long)gridDim.x * 256;
    const int k = P.k;
    const unsigned tmask = P.tree_mask, cmask = P.chain_mask;
    {   // every element (operands misaligned), or the head and the tail
        const long tail0 = P.vec_ok ? P.head + P.nvec * L : 0;
        const long nscal = P.vec_ok ? P.head + (P.n - tail0) : P.n;
        for (long s = tid; s < nscal; s += nthr) {
            const long i = !P.vec_ok || s < P.head ? s : tail0 + (s - P.head);
            float y[KMAX][1];
#pragma unroll
            for (int q = 0; q < KMAX; ++q) {
                if (q < k) {
                    y[q][0] = ld_f32side<T, DIR>(P.src[q], i);
                    if (DIR == 0 && P.fold[q]) y[q][0] = accf<O>(y[q][0], ld_f32side<T, 0>(P.fold[q], i));
                }
            }
            acc_steps<O, KMAX, 1, 0>(y, k, tmask, cmask);
            if constexpr (DIR == 0) reinterpret_cast<float *>(P.dst)[i] = y[0][0];
            else narrow_elt(reinterpret_cast<T *>(P.dst) + i, y[0][0]);
        }
        if (!P.vec_ok) return;
    }
    const long nb = P.head * (long)sizeof(T), fb = P.head * 4;   // the body's byte offset on either side
    for (long c = tid; c < P.nvec; c += nthr) {
        float y[KMAX][L];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (q < k) {
                if constexpr (DIR == 0) {
                    Wide<T>::widen(reinterpret_cast<const uint32_t *>(P.src[q] + nb)[c], y[q]);
                    if (P.fold[q]) {
                        float f[L];
                        Wide<T>::widen(reinterpret_cast<const uint32_t *>(P.fold[q] + nb)[c], f);
#pragma unroll
                        for (int j = 0; j < L; ++j) y[q][j] = accf<O>(y[q][j], f[j]);
                    }
                } else {
                    const fL v = reinterpret_cast<const fL *>(P.src[q] + fb)[c];
#pragma unroll
                    for (int j = 0; j < L; ++j) y[q][j] = v[j];
                }
            }
        }
        acc_steps<O, KMAX, L, 0>(y, k, tmask, cmask);
        if constexpr (DIR == 0) {
            fL v;
#pragma unroll
            for (int j = 0; j < L; ++j) v[j] = y[0][j];
            reinterpret_cast<fL *>(P.dst + fb)[c] = v;
        } else {
            reinterpret_cast<uint32_t *>(P.dst + nb)[c] = Wide<T>::narrow(y[0]);
        }
    }
}

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
