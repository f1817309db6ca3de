// mvx_ops_kern_def.h -- the kernels of mvx_ops_kern.h that take MVX_KP (Params,
// SParams or RParams) or MVX_KBP (BodyParams, SBodyParams or RBodyParams), and the element path
// they share.  No include guard: mvx_ops_kern.h reads it once per pair of
// types, inside namespace mvx (the reason is given there).

// the same element of every leaf through the f32-accumulating program
// (acc_op): widened, folded and combined in f32, narrowed once.  A single
// unfolded leaf has no step: it is copied, bits and all (a NaN's payload
// would not survive the way to f32 and back), as the per-step ops copy it
// (OAVG: unless it is to be divided).
template <int O, typename T, int KMAX>
__device__ __forceinline__ void scalar_elem_acc(const MVX_KP &P, long i)
{
    if (P.k == 1 && !P.fold[0] && (O != OAVG || P.divisor == 1)) {
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
    narrow_elt(reinterpret_cast<T *>(P.dst) + i, avg_fin<O>(y[0][0], P.divisor));
}

template <int O, typename T, int KMAX>
__device__ __forceinline__ void scalar_elem(const MVX_KP &P, long i)
{
    if constexpr (acc_op<O, T>::v) {
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
        if constexpr (O == OAVG) y[0] = avg_fin<O>(y[0], P.divisor);
        store_elt(reinterpret_cast<T *>(P.dst) + i, y[0]);
    }
}

// OSCL's scalar_elem_acc: the leaves scaled as they are widened, the value
// rescaled once; am is the lane's running amax (untouched without an amax word)
template <int O, typename T, int KMAX>
__device__ __forceinline__ void scalar_elem_scl(const MVX_KP &P, long i, unsigned &am)
{
    const Scl &sc = scl_of<O>(P);
    if (P.k == 1 && !P.fold[0] && scl_unit(sc)) {   // copied, bits and all; it still counts for amax
        store_elt(reinterpret_cast<T *>(P.dst) + i, reinterpret_cast<const T *>(P.src[0])[i]);
        if (sc.amax) {
            const float v[1] = {widen_elt(reinterpret_cast<const T *>(P.src[0]) + i)};
            am = scl_amax(am, v);
        }
        return;
    }
    float y[KMAX][1];
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
        if (q < P.k) {
            y[q][0] = widen_elt(reinterpret_cast<const T *>(P.src[q]) + i) * sc.lscale[q];
            if (P.fold[q]) y[q][0] = accf<OSCL>(y[q][0], widen_elt(reinterpret_cast<const T *>(P.fold[q]) + i) * sc.fscale[q]);
        }
    }
    acc_steps<OSCL, KMAX, 1, 0>(y, P.k, P.tree_mask, P.chain_mask);
    y[0][0] *= sc.oscale;
    if (sc.amax) am = scl_amax(am, y[0]);
    narrow_elt(reinterpret_cast<T *>(P.dst) + i, y[0][0]);
}

// OSR's scalar_elem_acc: the same f32 value, narrowed with the bits of element
// sr.first + i of the reduced vector
template <int O, typename T, int KMAX>
__device__ __forceinline__ void scalar_elem_sr(const MVX_KP &P, long i)
{
    const Sr &sr = sr_of<O>(P);
    if (P.k == 1 && !P.fold[0]) {   // copied, bits and all
        store_elt(reinterpret_cast<T *>(P.dst) + i, reinterpret_cast<const T *>(P.src[0])[i]);
        return;
    }
    float y[KMAX][1];
#pragma unroll
    for (int q = 0; q < KMAX; ++q) {
        if (q < P.k) {
            y[q][0] = widen_elt(reinterpret_cast<const T *>(P.src[q]) + i);
            if (P.fold[q]) y[q][0] = accf<OSR>(y[q][0], widen_elt(reinterpret_cast<const T *>(P.fold[q]) + i));
        }
    }
    acc_steps<OSR, KMAX, 1, 0>(y, P.k, P.tree_mask, P.chain_mask);
    narrow_elt_sr(reinterpret_cast<T *>(P.dst) + i, y[0][0], sr_elt_bits<T>(sr, sr.first + (uint64_t)i));
}

// PROG = 0: the program comes from the masks (any chain of trees over
// k <= KMAX leaves); PROG = 1: the full balanced tree over exactly KMAX
// leaves, steps fixed at compile time -- the Allreduce / Reduce order at
// p = 4 and 8 (Rabenseifner), where the generic form evaluated and
// discarded 24 masked steps for the 7 the tree needs.
template <int O, typename T, int KMAX, int U, int NT, int PROG = 0>
__global__ void __launch_bounds__(256)
k_combine(const MVX_KP P)
{
    // the launch may reserve dynamic LDS to cap resident blocks per CU
    // (plan(), Config::cap_*); the kernel never uses it -- the reference here
    // (never taken) marks the kernel as one that takes dynamic LDS
    extern __shared__ char lds_cap[];
    if (P.n < 0) lds_cap[threadIdx.x] = 0;
    constexpr int V = CG<T>::v;
    const long tid = (long)blockIdx.x * 256 + threadIdx.x;
    const long nthr = (long)gridDim.x * 256;
    unsigned am = 0;   // OSCL: the lane's amax over everything it stores
    [[maybe_unused]] SrC cc = src_none();   // OSR: the lane's hash constant

    if (!P.vec_ok) {  // operands misaligned against each other: element loads
        for (long i = tid; i < P.n; i += nthr) {
            if constexpr (O == OSCL) scalar_elem_scl<O, T, KMAX>(P, i, am);
            else if constexpr (O == OSR) scalar_elem_sr<O, T, KMAX>(P, i);
            else scalar_elem<O, T, KMAX>(P, i);
        }
        if constexpr (O == OSCL) {
            if (scl_of<O>(P).amax) amax_commit(scl_of<O>(P).amax, am);
        }
        return;
    }
    {   // head and tail elements outside the aligned body
        const long tail0 = P.head + P.nvec * V;
        const long nscal = P.head + (P.n - tail0);
        for (long s = tid; s < nscal; s += nthr) {
            const long i = s < P.head ? s : tail0 + (s - P.head);
            if constexpr (O == OSCL) scalar_elem_scl<O, T, KMAX>(P, i, am);
            else if constexpr (O == OSR) scalar_elem_sr<O, T, KMAX>(P, i);
            else scalar_elem<O, T, KMAX>(P, i);
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
        if constexpr (acc_op<O, T>::v) {
            if constexpr (O == OSCL) batch_scl<T, KMAX, U, NT, PROG>(x, fold, c0, P.nvec, k, tmask, cmask, scl_of<O>(P), am);
            else if constexpr (O == OSR) {
                const uint64_t i0 = sr_of<O>(P).first + (uint64_t)P.head;   // the body's first element
                batch_sr<T, KMAX, U, NT, PROG>(x, fold, c0, P.nvec, k, tmask, cmask, sr_of<O>(P), i0,
                                               (int)(i0 & (Wide<T>::L - 1)), cc);
            }
            else batch_acc<O, T, KMAX, U, NT, PROG>(x, fold, c0, P.nvec, k, tmask, cmask, P.divisor);
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
            // OAVG: the program's value divided once
#pragma unroll
            for (int u = 0; u < U; ++u) avg_chunk<O, T>(x[u][0], P.divisor);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long c = c0 + (long)u * 256;
            if (c < P.nvec) st_chunk<T, NT>(dst, c, x[u][0]);
        }
    }
    if constexpr (O == OSCL) {
        if (scl_of<O>(P).amax) amax_commit(scl_of<O>(P).amax, am);
    }
}

template <int O, typename T, int KMAX, int U>
__global__ void __launch_bounds__(256)
k_tree_body(const MVX_KBP P)
{
    __shared__ char lds_cap[BODY_LDS_CAP];
    if (P.nvec < 0) lds_cap[threadIdx.x] = 0;
    const long nthr = (long)gridDim.x * 256;
    unsigned am = 0;
    [[maybe_unused]] SrC cc = src_none();
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
                if constexpr (acc_op<O, T>::v) {
                    if constexpr (O == OSCL) {
                        const unsigned m = scl_chunk<T, KMAX, 1>(x[u], x[u], 0u, KMAX, 0u, 0u, scl_of<O>(P));
                        am = m > am ? m : am;
                    } else if constexpr (O == OSR) {
                        uint32_t rb[4];
                        sr_word_bits<T, 4>(sr_of<O>(P), sr_of<O>(P).first + (uint64_t)c * CG<T>::v,
                                           (int)(sr_of<O>(P).first & (Wide<T>::L - 1)), cc, rb);
                        sr_chunk<T, KMAX, 1>(x[u], x[u], 0u, KMAX, 0u, 0u, rb);
                    } else {
                        acc_chunk<O, T, KMAX, 1>(x[u], x[u], 0u, KMAX, 0u, 0u, P.divisor);
                    }
                } else {
#pragma unroll
                    for (int h = 1; h < KMAX; h <<= 1)
#pragma unroll
                        for (int q = 0; q + h < KMAX; q += 2 * h)
                            CF<O, T>::f(x[u][q], x[u][q + h]);
                    avg_chunk<O, T>(x[u][0], P.divisor);
                }
                st_chunk<T, BODY_ST_NT>(P.dst, c, x[u][0]);
            }
        }
    }
    if constexpr (O == OSCL) {
        if (scl_of<O>(P).amax) amax_commit(scl_of<O>(P).amax, am);
    }
}

// The same over a full CHAIN ((y0 op y1) op y2) ..., the pairwise
// Reduce_scatter's order (C4: k = 4, p = 4).  The 8-leaf instantiation
// takes chains of 5 to 8 leaves (P.k, a wave-uniform test per leaf): the
// pairwise chains at p = 5, 6, 7, which otherwise run the masked program at
// one chunk per lane.
template <int O, typename T, int KMAX, int U>
__global__ void __launch_bounds__(256)
k_chain_body(const MVX_KBP P)
{
    __shared__ char lds_cap[BODY_LDS_CAP];
    if (P.nvec < 0) lds_cap[threadIdx.x] = 0;
    const int k = KMAX == 8 ? P.k : KMAX;
    const long nthr = (long)gridDim.x * 256;
    unsigned am = 0;
    [[maybe_unused]] SrC cc = src_none();
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
                if constexpr (acc_op<O, T>::v) {
                    if constexpr (O == OSCL) {
                        const unsigned m = scl_chunk<T, KMAX, 0>(x[u], x[u], 0u, k, 0u, (1u << k) - 2u, scl_of<O>(P));
                        am = m > am ? m : am;
                    } else if constexpr (O == OSR) {
                        uint32_t rb[4];
                        sr_word_bits<T, 4>(sr_of<O>(P), sr_of<O>(P).first + (uint64_t)c * CG<T>::v,
                                           (int)(sr_of<O>(P).first & (Wide<T>::L - 1)), cc, rb);
                        sr_chunk<T, KMAX, 0>(x[u], x[u], 0u, k, 0u, (1u << k) - 2u, rb);
                    } else {
                        acc_chunk<O, T, KMAX, 0>(x[u], x[u], 0u, k, 0u, (1u << k) - 2u, P.divisor);
                    }
                } else {
#pragma unroll
                    for (int q = 1; q < KMAX; ++q)
                        if (q < k) CF<O, T>::f(x[u][0], x[u][q]);
                    avg_chunk<O, T>(x[u][0], P.divisor);
                }
                st_chunk<T, BODY_ST_NT>(P.dst, c, x[u][0]);
            }
        }
    }
    if constexpr (O == OSCL) {
        if (scl_of<O>(P).amax) amax_commit(scl_of<O>(P).amax, am);
    }
}

// The masked program of an f32-accumulating op with one side in f32: what a
// program over more than 8 leaves is cut into (mvx_combine.c), its
// intermediates being f32 temporaries.  DIR = 0: narrow leaves (folds
// allowed), f32 result, not narrowed; DIR = 1: f32 leaves, the result narrowed
// once (OAVG, the last launch of such a program: divided, then narrowed; OSCL:
// DIR = 0 scales the leaves, DIR = 1 rescales the value and takes amax; OSR:
// DIR = 1 alone, narrowed with the elements' bits).  A lane takes one 32-bit word of each narrow operand against L floats
// of each f32 one (a dwordx4 for the 8-bit types, a dwordx2 for the 16-bit
// ones).  Params: head elements lead to nvec such words where the narrow
// side is 4-byte and the f32 side 4 * L-byte aligned (vec_ok), else every
// element goes alone.
template <int O, typename T, int DIR>
__global__ void __launch_bounds__(256)
k_combine_f32(const MVX_KP P)
{
    constexpr int L = Wide<T>::L;
    constexpr int KMAX = MVX_COMBINE_KMAX;
    typedef float fL __attribute__((ext_vector_type(L)));
    const long tid = (long)blockIdx.x * 256 + threadIdx.x;
    const long nthr = (long)gridDim.x * 256;
    const int k = P.k;
    const unsigned tmask = P.tree_mask, cmask = P.chain_mask;
    constexpr bool SCL_IN = O == OSCL && DIR == 0, SCL_OUT = O == OSCL && DIR == 1;
    unsigned am = 0;
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
                    if constexpr (SCL_IN) y[q][0] *= scl_of<O>(P).lscale[q];
                    if (DIR == 0 && P.fold[q]) {
                        float f = ld_f32side<T, 0>(P.fold[q], i);
                        if constexpr (SCL_IN) f *= scl_of<O>(P).fscale[q];
                        y[q][0] = accf<O>(y[q][0], f);
                    }
                }
            }
            acc_steps<O, KMAX, 1, 0>(y, k, tmask, cmask);
            y[0][0] = avg_fin<O>(y[0][0], P.divisor);
            if constexpr (SCL_OUT) {
                y[0][0] *= scl_of<O>(P).oscale;
                if (scl_of<O>(P).amax) am = scl_amax(am, y[0]);
            }
            if constexpr (DIR == 0) reinterpret_cast<float *>(P.dst)[i] = y[0][0];
            else if constexpr (O == OSR)
                narrow_elt_sr(reinterpret_cast<T *>(P.dst) + i, y[0][0],
                              sr_elt_bits<T>(sr_of<O>(P), sr_of<O>(P).first + (uint64_t)i));
            else narrow_elt(reinterpret_cast<T *>(P.dst) + i, y[0][0]);
        }
        if (!P.vec_ok) {
            if constexpr (SCL_OUT) {
                if (scl_of<O>(P).amax) amax_commit(scl_of<O>(P).amax, am);
            }
            return;
        }
    }
    const long nb = P.head * (long)sizeof(T), fb = P.head * 4;   // the body's byte offset on either side
    [[maybe_unused]] SrC cc = src_none();
    for (long c = tid; c < P.nvec; c += nthr) {
        float y[KMAX][L];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (q < k) {
                if constexpr (DIR == 0) {
                    Wide<T>::widen(reinterpret_cast<const uint32_t *>(P.src[q] + nb)[c], y[q]);
                    if constexpr (SCL_IN) {
#pragma unroll
                        for (int j = 0; j < L; ++j) y[q][j] *= scl_of<O>(P).lscale[q];
                    }
                    if (P.fold[q]) {
                        float f[L];
                        Wide<T>::widen(reinterpret_cast<const uint32_t *>(P.fold[q] + nb)[c], f);
                        if constexpr (SCL_IN) {
#pragma unroll
                            for (int j = 0; j < L; ++j) f[j] *= scl_of<O>(P).fscale[q];
                        }
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
#pragma unroll
        for (int j = 0; j < L; ++j) y[0][j] = avg_fin<O>(y[0][j], P.divisor);
        if constexpr (SCL_OUT) {
#pragma unroll
            for (int j = 0; j < L; ++j) y[0][j] *= scl_of<O>(P).oscale;
            if (scl_of<O>(P).amax) am = scl_amax(am, y[0]);
        }
        if constexpr (DIR == 0) {
            fL v;
#pragma unroll
            for (int j = 0; j < L; ++j) v[j] = y[0][j];
            reinterpret_cast<fL *>(P.dst + fb)[c] = v;
        } else if constexpr (O == OSR) {
            const uint64_t i0 = sr_of<O>(P).first + (uint64_t)P.head;
            uint32_t rb[1];
            sr_word_bits<T, 1>(sr_of<O>(P), i0 + (uint64_t)c * L, (int)(i0 & (L - 1)), cc, rb);
            reinterpret_cast<uint32_t *>(P.dst + nb)[c] = sr_narrow<T>(y[0], rb[0]);
        } else {
            reinterpret_cast<uint32_t *>(P.dst + nb)[c] = Wide<T>::narrow(y[0]);
        }
    }
    if constexpr (SCL_OUT) {
        if (scl_of<O>(P).amax) amax_commit(scl_of<O>(P).amax, am);
    }
}
