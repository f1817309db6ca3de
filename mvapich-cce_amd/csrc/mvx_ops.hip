// mvx_ops.hip -- the device side of the MPI local reduction path, written for
// gfx950 (CDNA4, wave64): the (op, datatype) dispatch, the knobs (config), the
// launch policy and the C-ABI of include/mvx_hip.h.  The policy is three pure
// host functions -- choose_family, split (the alignment rule) and plan -- that
// never touch the device or a buffer; run() is the one place that launches.
// mvx_op_plan answers with the plan alone.  The kernels are in mvx_ops_kern.h
// (design notes at its top), their host-side tables in mvx_ops_tab.h and
// mvx_ops_{cmp,arith,logic,loc,half,fp8,acc32}.hip.
#include <stdlib.h>

#include "mvx_dtype.h"
#include "mvx_ops_tab.h"

namespace mvx {

// a handle's dte_type, where the Fortran types share one with a C type
// (initfutil.c:238-245, 261, 279: INTEGER is MPIR_INT, REAL MPIR_FLOAT,
// DOUBLE PRECISION MPIR_DOUBLE); the old types of derived types switch on it
static int dte_of(int h)
{
    switch (h) {
    case MPI_INTEGER: return MPI_INT;
    case MPI_REAL: return MPI_FLOAT;
    case MPI_DOUBLE_PRECISION: return MPI_DOUBLE;
    default: return h;
    }
}

// the op kind of a derived handle (mvx_dtype.hip): MAXLOC / MINLOC are the
// only ops with derived cases -- a count-2 contiguous type over one base
// (stride-2 {value, loc} scalars, global_ops.c:1387-1503 / 1625-1740), and an
// MPIR_STRUCT type by the dte_type of its old_types[0], read as that base's C
// pair struct (1280-1384 / 1520-1620); every other case is 329
static int derived_kind(const dt::Info &d)
{
    if (d.kind == dt::K_STRUCT) {
        switch (dte_of(d.old)) {
        case MPI_INT: return EK_PII;             // MPIR_2int_loctype
        case MPI_FLOAT: return EK_PFI;
        case MPI_LONG: case MPI_LONG_LONG_INT: return EK_PLI;
        case MPI_SHORT: return EK_PSI;
        case MPI_DOUBLE: return EK_PDI;
        case MPI_LONG_DOUBLE: return EK_LDBL_INT;
        default: return EK_DERIVED;
        }
    }
    if (d.kind != dt::K_CONTIG || d.count != 2) return EK_DERIVED;
    switch (dte_of(d.old)) {      // the base's dte_type, global_ops.c:1395-1497
    case MPI_INT: return EK_PII;
    case MPI_LONG: case MPI_LONG_LONG_INT: return EK_PP64;
    case MPI_SHORT: return EK_PP16;
    case MPI_CHAR: return EK_PP8;
    case MPI_FLOAT: return EK_PPF;
    case MPI_DOUBLE: return EK_PPD;
    case MPI_LONG_DOUBLE: return EK_PPX;
    default: return EK_DERIVED;
    }
}

static int ekind(int dtype)
{
    if (dtype >= MVX_TYPE_DERIVED_BASE) {
        dt::Info d;
        return dt::info(dtype, &d) ? derived_kind(d) : EK_NONE;
    }
    switch (dtype) {
    case MPI_CHAR: return EK_I8;
    case MPI_UNSIGNED_CHAR: return EK_U8;
    case MPI_BYTE: return EK_BYTE;
    case MPI_SHORT: return EK_I16;
    case MPI_UNSIGNED_SHORT: return EK_U16;
    case MPI_INT: return EK_I32;
    case MPI_UNSIGNED: return EK_U32;
    case MPI_LONG: case MPI_LONG_LONG_INT: return EK_I64;
    case MPI_UNSIGNED_LONG: return EK_U64;
    case MPI_FLOAT: return EK_F32;
    case MPI_DOUBLE: return EK_F64;
    case MPI_COMPLEX: return EK_C32;
    case MPI_DOUBLE_COMPLEX: return EK_C64;
    case MPI_FLOAT_INT: return EK_PFI;
    case MPI_DOUBLE_INT: return EK_PDI;
    case MPI_LONG_INT: return EK_PLI;
    case MPI_SHORT_INT: return EK_PSI;
    case MPI_2INT: return EK_PII;
    case MPI_LONG_DOUBLE: return EK_LDBL;
    case MPI_LONG_DOUBLE_INT: return EK_LDBL_INT;
    case MPI_INTEGER: return EK_I32;
    case MPI_REAL: return EK_F32;
    case MPI_DOUBLE_PRECISION: return EK_F64;
    case MPI_LOGICAL: return EK_LOGICAL;
    case MVX_FLOAT16: return EK_F16;          // extension (mvx_mpi.h)
    case MVX_BFLOAT16: return EK_BF16;
    case MVX_FLOAT8_E4M3: return EK_F8E4M3;
    case MVX_FLOAT8_E5M2: return EK_F8E5M2;
    // the Fortran pairs: contiguous(2, x), the MAXLOC / MINLOC stride-2 case
    // of x's dte_type (global_ops.c:1387-1503); no case for COMPLEX (1498)
    case MPI_2INTEGER: return EK_PII;
    case MPI_2REAL: return EK_PPF;
    case MPI_2DOUBLE_PRECISION: return EK_PPD;
    case MPI_2COMPLEX: case MPI_2DOUBLE_COMPLEX: return EK_DERIVED;
    default: return EK_NONE;
    }
}

// Returns the kernel set, or NULL with *rc set to the reference's answer for
// that (op, type): 329 where the op's switch has no case for it
// (global_ops.c:158-161 and every sibling default), and MPI_ERR_OP for a
// handle outside MPI_MAX..MPI_MAXLOC that is not one of the two extension
// ops.  Those (MVX_SUM_ACC32, MVX_PROD_ACC32) have a case for the four
// narrow floating types alone.
static bool acc32(int op) { return op == MVX_SUM_ACC32 || op == MVX_PROD_ACC32; }

static const KSet *lookup(int op, int dtype, int *rc)
{
    int ek = ekind(dtype);
    *rc = MVX_ERR_OP_NOT_DEFINED;
    if (acc32(op)) return lookup_acc32(op, ek);
    if (ek == EK_LOGICAL && (op == MPI_BAND || op == MPI_BOR || op == MPI_BXOR))
        ek = EK_U32;                 // bitwise on the MPI_Fint word
    if (ek == EK_F16 || ek == EK_BF16) {
        if (op < MPI_MAX || op > MPI_MAXLOC) *rc = MPI_ERR_OP;
        return lookup_half(op, ek);
    }
    if (ek == EK_F8E4M3 || ek == EK_F8E5M2) {
        if (op < MPI_MAX || op > MPI_MAXLOC) *rc = MPI_ERR_OP;
        return lookup_fp8(op, ek);
    }

    switch (op) {
    case MPI_MAX: case MPI_MIN:
        return lookup_cmp(op, ek);
    case MPI_SUM: case MPI_PROD:
        return lookup_arith(op, ek);
    case MPI_LAND: case MPI_LOR: case MPI_LXOR: case MPI_BAND: case MPI_BOR: case MPI_BXOR:
        if (ek == EK_LOGICAL && flog_sync()) { *rc = MPI_ERR_OTHER; return nullptr; }
        return lookup_logic(op, ek);
    case MPI_MAXLOC: case MPI_MINLOC:
        return lookup_loc(op, ek);
    default:
        *rc = MPI_ERR_OP;
        return nullptr;
    }
}

// The knobs (Config, mvx_ops_tab.h) by name.  A value counts when the rule
// says so: '*' any, '+' only a positive one, '=' only `v` itself.
static Config g_cfg;
static const struct { const char *name; long Config::*field; char rule; long v; } KNOBS[] = {
    {"MVX_NT_MIN_BYTES", &Config::nt_min_bytes, '*', 0},
    {"MVX_BLOCK_CAP", &Config::block_cap, '+', 0},
    {"MVX_PROG_U", &Config::prog_u, '=', 2},
    {"MVX_PROG_GENERIC", &Config::generic_only, '=', 1},
    {"MVX_PROG4", &Config::prog4, '=', 0},
    {"MVX_CHAIN_RT", &Config::chain_rt, '=', 0},
    {"MVX_NO_BODY", &Config::no_body, '=', 1},
    {"MVX_CAP_APPLY", &Config::cap_apply, '*', 0},
    {"MVX_CAP_PROG", &Config::cap_prog, '*', 0},
    {"MVX_CAP_TREE", &Config::cap_tree, '*', 0},
    {"MVX_PXI_U", &Config::pxi_u, '*', 0},
    {"MVX_PXI_CAP", &Config::pxi_cap, '*', 0},
    {"MVX_PXI_APPLY_CAP", &Config::pxi_apply_cap, '*', 0},
};

const Config &config()
{
    static bool done = false;
    if (done) return g_cfg;
    done = true;
    for (const auto &kn : KNOBS) {
        const char *e = getenv(kn.name);
        if (!e) continue;
        // the byte threshold is a long; every other knob is read as an int
        const long v = kn.field == &Config::nt_min_bytes ? atol(e) : (long)atoi(e);
        if (kn.rule == '*' || (kn.rule == '+' && v > 0) || (kn.rule == '=' && v == kn.v)) g_cfg.*kn.field = v;
    }
    return g_cfg;
}

// LDS per CU of the device the kernels run on, from its architecture name
// (the runtime's per-multiprocessor attribute reports the 64 KiB per-block
// limit instead): gfx950 has 160 KiB; earlier CDNA parts 64 KiB.  A
// reservation sized for 160 KiB on a 64 KiB part would cap the kernel at one
// resident block per CU, so the reservation follows the part.
static size_t lds_per_cu()
{
    static size_t v = 0;
    if (v) return v;
    int dev = 0;
    hipDeviceProp_t pr;
    v = 64 * 1024;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess) {
        if (!strncmp(pr.gcnArchName, "gfx950", 6)) v = 160 * 1024;
    } else {
        (void)hipGetLastError();
    }
    return v;
}

// dynamic LDS per block that leaves room for `cap` blocks per CU and not one
// more (the kernels do not touch it): the middle of the range,
// 2 * LDS / (2 * cap + 1), clear of the allocator's rounding at the edges; at
// most 64 KiB (no function attribute needed).
static size_t cap_lds(int cap)
{
    const size_t lds = lds_per_cu();
    if (cap < 2) return 0;
    const size_t b = (lds * 2 / (size_t)(2 * cap + 1)) & ~(size_t)1023;
    return b > 64 * 1024 ? 64 * 1024 : b;
}

// ---------------------------------------------------------------------------
// the launch policy: which template runs, with how many blocks and which LDS
// reservation.  Pure host arithmetic on addresses and sizes.

// The kernel family of a program over k leaves (k <= 2: the plain op).
static const KFam &choose_family(const KSet *ks, const Config &cfg, int k, unsigned tree_mask,
                                 unsigned chain_mask, bool folded)
{
    if (k <= 2) return ks->apply;
    const bool fixed = !cfg.generic_only && !folded;
    if (fixed && chain_mask == 0 && (k == 8 || k == 4) && tree_mask == mvx_tree_mask(k))
        return k == 8 ? ks->tree8 : ks->tree4;
    /* chains of 5-7 leaves (pairwise Reduce_scatter at p = 5..7): the 8-leaf
     * chain body with a run-time leaf count, else its masked program */
    if (fixed && tree_mask == 0 && k >= 4 && chain_mask == mvx_chain_mask(k) && (k == 4 || cfg.chain_rt || k == 8))
        return k == 4 ? ks->chain4 : ks->chain8;
    if (cfg.prog_u == 2 && ks->prog2.var[V_CACHED].fn) return ks->prog2;
    if (k <= 4 && cfg.prog4) return ks->prog4;
    return ks->prog;
}

// The alignment rule, and nothing else -- the rule the work on mutually
// misaligned operands will change.  The 16-byte path needs the destination,
// every source and every fold partner on one residue m mod 16, and a whole
// number of elements up to the next 16-byte boundary: then `head` scalar
// elements lead to `nvec` whole chunks (the rest is the scalar tail);
// otherwise every element goes the scalar way.  Reads P's addresses and n.
struct Split { long head, nvec; int vec_ok; };
static Split split(const Params &P, int esize, int chunk)
{
    const uintptr_t m = (uintptr_t)P.dst & 15;
    bool same = true;
    for (int q = 0; q < P.k; ++q) {
        if (((uintptr_t)P.src[q] & 15) != m) same = false;
        if (P.fold[q] && ((uintptr_t)P.fold[q] & 15) != m) same = false;
    }
    const long pre = (long)((16 - m) & 15);
    if (!same || pre % esize != 0) return {0, 0, 0};
    const long head = pre / esize < P.n ? pre / esize : P.n;
    return {head, (P.n - head) * esize / chunk, 1};
}

// What run() launches, and what mvx_op_plan / mvx_hip_last_* report.
struct Plan {
    const void *fn;
    SymFn name;
    char tag[96];          // "sum_f32_k2_nt"
    unsigned blocks;
    size_t lds;            // dynamic LDS bytes: the residency cap
    bool body;             // the kernel takes BodyParams
};

// P with split()'s answer in it; nfold of its leaves are folded.
static Plan plan(const KSet *ks, const KFam &F, const Params &P, int nfold, const Config &cfg)
{
    const int es = ks->esize;
    const int nt = (long)(P.k + nfold + 1) * P.n * es >= cfg.nt_min_bytes;
    const KVar &B = F.var[V_BODY];
    const bool body = nt && B.fn && !cfg.no_body && P.k >= B.kmin && P.k <= B.kmax && P.vec_ok && P.head == 0 &&
                      P.nvec > 0 && P.nvec * ks->chunk == P.n * es && !nfold;
    const KVar &V = body ? B : F.var[nt];
    const long per_block = (long)V.unroll * 256;
    long work = body ? (P.nvec * V.units + per_block - 1) / per_block
                     : P.vec_ok ? (P.nvec + per_block - 1) / per_block : (P.n + 255) / 256;
    if (work < 1) work = 1;
    const long fam_cap[FAM_N] = {cfg.cap_apply, cfg.cap_prog, cfg.cap_tree};
    Plan pl;
    pl.fn = V.fn;
    pl.name = V.name;
    snprintf(pl.tag, sizeof pl.tag, "%s_k%d%s", ks->name, P.k, nt ? "_nt" : "");
    pl.blocks = (unsigned)(work < cfg.block_cap ? work : cfg.block_cap);
    pl.lds = body ? cap_lds(V.cap) : nt ? cap_lds((int)fam_cap[F.fam]) : 0;
    pl.body = body;
    return pl;
}

// choose_family, split and plan for the leaves and program in P
static Plan plan_params(const KSet *ks, Params &P)
{
    const Config &cfg = config();
    int nfold = 0;
    for (int q = 0; q < P.k; ++q) nfold += P.fold[q] != nullptr;
    const KFam &F = choose_family(ks, cfg, P.k, P.tree_mask, P.chain_mask, nfold > 0);
    const Split s = split(P, ks->esize, ks->chunk);
    P.head = s.head;
    P.nvec = s.nvec;
    P.vec_ok = s.vec_ok;
    return plan(ks, F, P, nfold, cfg);
}

static Plan g_last;        // the last launch (not thread-safe)

static int run(const Plan &pl, const Params &P, hipStream_t stream)
{
    BodyParams B;
    void *args[] = {const_cast<Params *>(&P)};
    if (pl.body) {
        memset(&B, 0, sizeof B);
        for (int q = 0; q < P.k; ++q) B.src[q] = reinterpret_cast<const u32x4 *>(P.src[q]);
        B.dst = reinterpret_cast<u32x4 *>(P.dst);
        B.nvec = P.nvec;
        B.k = P.k;
        args[0] = &B;
    }
    hipError_t e = hipLaunchKernel(pl.fn, dim3(pl.blocks), dim3(256), args, pl.lds, stream);
    g_last = pl;
    return e == hipSuccess ? MPI_SUCCESS : MPI_ERR_OTHER;
}

// The argument checks of mvx_op_program, then P: MPI_SUCCESS (*ksp null for
// n == 0: nothing to do) or the error code
static int program_params(int op, int dtype, const void *const *srcs, const void *const *fold, int k,
                          unsigned tree_mask, unsigned chain_mask, const void *dst, size_t n,
                          const KSet **ksp, Params &P)
{
    int rc;
    const KSet *ks = lookup(op, dtype, &rc);
    *ksp = nullptr;
    if (!ks) return rc;
    if (k < 1 || k > MVX_COMBINE_KMAX || !srcs) return MPI_ERR_ARG;
    /* every step must stay inside the k leaves */
    for (int l = 0; l < 3; ++l)
        for (int q = 0; q < 8; ++q)
            if ((tree_mask >> (l * 8 + q) & 1u) && q + (1 << l) >= k) return MPI_ERR_ARG;
    if ((tree_mask >> 24) || (chain_mask & 1u) || (chain_mask >> k)) return MPI_ERR_ARG;
    if (n == 0) return MPI_SUCCESS;
    memset(&P, 0, sizeof P);
    for (int q = 0; q < k; ++q) {
        P.src[q] = (const char *)srcs[q];
        P.fold[q] = fold ? (const char *)fold[q] : nullptr;
    }
    P.dst = (char *)dst;
    P.n = (long)n;
    P.k = k;
    P.tree_mask = tree_mask;
    P.chain_mask = chain_mask;
    /* the only programs over <= 2 leaves: nothing, or y0 op y1 */
    if (k == 2 && !(tree_mask & 1u) && !(chain_mask & 2u)) return MPI_ERR_ARG;
    *ksp = ks;
    return MPI_SUCCESS;
}

// The one-side-f32 program (k_combine_f32).  The narrow operands -- the
// leaves and fold partners (f32_out), or the destination -- must share their
// residue mod 4 with a whole number of elements up to the next word; `head`
// elements then lead to `nvec` words of L elements, provided every f32
// operand is 4 * L-byte aligned from element `head` on.  Otherwise every
// element goes alone.
static Split split_f32(const Params &P, int esize, bool f32_out)
{
    const int L = 4 / esize;
    const uintptr_t m = (uintptr_t)(f32_out ? P.src[0] : P.dst) & 3;
    const long pre = (long)((4 - m) & 3);
    if (pre % esize != 0) return {0, 0, 0};
    const long head = pre / esize < P.n ? pre / esize : P.n;
    const uintptr_t fa = (uintptr_t)(4 * L - 1);
    if (f32_out) {
        for (int q = 0; q < P.k; ++q)
            if (((uintptr_t)P.src[q] & 3) != m || (P.fold[q] && ((uintptr_t)P.fold[q] & 3) != m)) return {0, 0, 0};
        if (((uintptr_t)P.dst + 4 * (uintptr_t)head) & fa) return {0, 0, 0};
    } else {
        for (int q = 0; q < P.k; ++q)
            if (((uintptr_t)P.src[q] + 4 * (uintptr_t)head) & fa) return {0, 0, 0};
    }
    return {head, (P.n - head) / L, 1};
}

static Plan plan_f32(const KSet *ks, Params &P, bool f32_out, const Config &cfg)
{
    const KVar &V = ks->f32side[f32_out ? 0 : 1];
    const Split s = split_f32(P, ks->esize, f32_out);
    P.head = s.head;
    P.nvec = s.nvec;
    P.vec_ok = s.vec_ok;
    long work = ((s.vec_ok ? s.nvec : P.n) + 255) / 256;
    if (work < 1) work = 1;
    Plan pl;
    pl.fn = V.fn;
    pl.name = V.name;
    snprintf(pl.tag, sizeof pl.tag, "%s_k%d_%s", ks->name, P.k, f32_out ? "to_f32" : "from_f32");
    pl.blocks = (unsigned)(work < cfg.block_cap ? work : cfg.block_cap);
    pl.lds = 0;
    pl.body = false;
    return pl;
}

}  // namespace mvx

using namespace mvx;


extern "C" int mvx_op_supported(int op, int dtype)
{
    int rc;
    return lookup(op, dtype, &rc) != nullptr;
}

extern "C" int mvx_op_element_size(int op, int dtype)
{
    int rc;
    const KSet *ks = lookup(op, dtype, &rc);
    return ks ? ks->esize : 0;
}

extern "C" int mvx_op_apply(int op, int dtype, const void *in, void *inout,
                            size_t n, void *stream)
{
    int rc;
    const KSet *ks = lookup(op, dtype, &rc);
    if (!ks) return rc;
    if (n == 0) return MPI_SUCCESS;
    Params P;
    memset(&P, 0, sizeof P);
    P.src[0] = (const char *)inout;   // a: the inout operand
    P.src[1] = (const char *)in;      // b
    P.dst = (char *)inout;
    P.n = (long)n;
    P.k = 2;
    return run(plan_params(ks, P), P, (hipStream_t)stream);
}

extern "C" int mvx_op_program(int op, int dtype, const void *const *srcs,
                              const void *const *fold, int k, unsigned tree_mask,
                              unsigned chain_mask, void *dst, size_t n, void *stream)
{
    const KSet *ks;
    Params P;
    const int rc = program_params(op, dtype, srcs, fold, k, tree_mask, chain_mask, dst, n, &ks, P);
    if (rc != MPI_SUCCESS || !ks) return rc;
    return run(plan_params(ks, P), P, (hipStream_t)stream);
}

extern "C" int mvx_op_program_f32(int op, int dtype, const void *const *srcs, const void *const *fold, int k,
                                  unsigned tree_mask, unsigned chain_mask, void *dst, size_t n, int side,
                                  void *stream)
{
    const KSet *ks;
    Params P;
    const int rc = program_params(op, dtype, srcs, fold, k, tree_mask, chain_mask, dst, n, &ks, P);
    if (rc != MPI_SUCCESS) return rc;
    /* only the f32-accumulating ops have an f32 side */
    if (!acc32(op) || (side != MVX_F32_OUT && side != MVX_F32_IN)) return MPI_ERR_ARG;
    if (!ks) return MPI_SUCCESS;
    /* f32 operands are floats: 4-byte aligned; f32 leaves are never folded */
    for (int q = 0; q < k; ++q) {
        if (side == MVX_F32_IN && (P.fold[q] || ((uintptr_t)P.src[q] & 3))) return MPI_ERR_ARG;
    }
    if (side == MVX_F32_OUT && ((uintptr_t)P.dst & 3)) return MPI_ERR_ARG;
    return run(plan_f32(ks, P, side == MVX_F32_OUT, config()), P, (hipStream_t)stream);
}

extern "C" int mvx_op_plan(int op, int dtype, const void *const *srcs, const void *const *fold, int k,
                           unsigned tree_mask, unsigned chain_mask, const void *dst, size_t n,
                           struct mvx_launch_plan *out)
{
    const KSet *ks;
    Params P;
    const int rc = program_params(op, dtype, srcs, fold, k, tree_mask, chain_mask, dst, n, &ks, P);
    if (rc != MPI_SUCCESS) return rc;
    if (!out) return MPI_ERR_ARG;
    memset(out, 0, sizeof *out);
    out->symbol = "";
    if (!ks) return MPI_SUCCESS;
    const Plan pl = plan_params(ks, P);
    out->symbol = pl.name();
    memcpy(out->tag, pl.tag, sizeof out->tag);
    out->blocks = pl.blocks;
    out->dynamic_lds = pl.lds;
    return MPI_SUCCESS;
}

extern "C" unsigned mvx_tree_mask(int k)
{
    unsigned m = 0;
    for (int l = 0; (1 << l) < k && l < 3; ++l)
        for (int q = 0; q + (1 << l) < k; q += 2 << l) m |= 1u << (l * 8 + q);
    return m;
}

extern "C" unsigned mvx_chain_mask(int k)
{
    return k >= 2 && k <= 32 ? (unsigned)(((1ull << k) - 1) & ~1ull) : 0u;
}

extern "C" int mvx_op_combine(int op, int dtype, const void *const *srcs,
                              const void *const *fold, int k, int shape,
                              void *dst, size_t n, void *stream)
{
    if (shape != MVX_SHAPE_TREE && shape != MVX_SHAPE_CHAIN) {
        int rc;
        return lookup(op, dtype, &rc) ? MPI_ERR_ARG : rc;
    }
    return mvx_op_program(op, dtype, srcs, fold, k,
                          shape == MVX_SHAPE_TREE ? mvx_tree_mask(k) : 0u,
                          shape == MVX_SHAPE_CHAIN ? mvx_chain_mask(k) : 0u, dst, n, stream);
}

extern "C" void mvx_hip_set_launch(int block_cap, int nt_min_bytes_log2)
{
    config();
    if (block_cap > 0) g_cfg.block_cap = block_cap;
    if (nt_min_bytes_log2 > 0) g_cfg.nt_min_bytes = 1L << nt_min_bytes_log2;
    if (nt_min_bytes_log2 < 0) g_cfg.nt_min_bytes = 1L << 62;   // never non-temporal
}

extern "C" const char *mvx_hip_last_kernel(void) { return g_last.tag; }

extern "C" const char *mvx_hip_last_kernel_symbol(void) { return g_last.name ? g_last.name() : ""; }

extern "C" void mvx_hip_last_launch(unsigned *blocks, size_t *dynamic_lds, int *blocks_per_cu)
{
    if (blocks) *blocks = g_last.blocks;
    if (dynamic_lds) *dynamic_lds = g_last.lds;
    if (blocks_per_cu) {
        int occ = 0;
        if (!g_last.fn ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, g_last.fn, 256, g_last.lds) != hipSuccess) {
            (void)hipGetLastError();
            occ = 0;
        }
        *blocks_per_cu = occ;
    }
}
