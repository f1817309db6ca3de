#pragma once
// mvx_ops_tab.h -- the host-side tables of the reduction kernels: the knobs
// (Config), the descriptor of one kernel instantiation (KVar), the families
// and sets built from them, the element kinds and the per-op table units'
// lookup functions.  Included by mvx_ops.hip (dispatch and launch policy) and
// by mvx_ops_{cmp,arith,logic,loc,half,fp8,acc32}.hip, which instantiate the kernels of
// mvx_ops_kern.h through the macros below, one translation unit each so that
// they compile in parallel.
#include <stdio.h>
#include <string.h>
#include <type_traits>

#include "mvx_mpi.h"
#include "mvx_ops_kern.h"

// ---------------------------------------------------------------------------
// dispatch: (op, datatype handle) -> kernel set

namespace mvx {

// The op-side knobs, filled once from the environment (config(), mvx_ops.hip,
// where the table of their names and parsing rules is); mvx_hip_set_launch
// writes block_cap and nt_min_bytes afterwards.  All A/B switches but the
// first two.  The launch policy reads it at every launch; pxi_* are read
// here, by kfam / kset, when a kernel set is first built.
struct Config {
    // Non-temporal above this many bytes touched by one launch (all operands +
    // the result); below it the result is likely re-read from L2 / MALL.
    long nt_min_bytes = 64L << 20;     // MVX_NT_MIN_BYTES
    // Grid: one pass over the data (a block per 256*U chunks) up to this cap,
    // grid-stride beyond it; a full pass measured best on the config-2 kernel.
    long block_cap = 1 << 20;          // MVX_BLOCK_CAP (counts only when positive)
    long prog_u = 1;                   // MVX_PROG_U=2: 4-byte types' programs on KSet::prog2 (U = 2)
    long generic_only = 0;             // MVX_PROG_GENERIC=1: no fixed-tree kernels
    long prog4 = 1;                    // MVX_PROG4=0: programs over 3-4 leaves on the KMAX = 8 kernels
    long chain_rt = 1;                 // MVX_CHAIN_RT=0: chains of 5-7 leaves on the masked program
    long no_body = 0;                  // MVX_NO_BODY=1: fixed trees and chains through k_combine
    // resident blocks per CU for the non-temporal launches of each family (0 =
    // as many as registers allow)
    long cap_apply = 0;                // MVX_CAP_APPLY
    long cap_prog = 0;                 // MVX_CAP_PROG
    long cap_tree = 2;                 // MVX_CAP_TREE
    // k_pxi_loc_body: one element per lane pair at 4 resident blocks per CU: 8 x
    // 64 MiB MAXLOC tree 96.4 us (78 % of HBM peak) against 115-117 us one
    // element per lane; U = 2 at 3 blocks 96.2-96.9, uncapped 99-101
    // (profiles/r03/bench_kernels_x87_pair_sweep.jsonl)
    long pxi_u = 1;                    // MVX_PXI_U=2: the trees' body at two chunks per lane
    long pxi_cap = 4;                  // MVX_PXI_CAP: the trees' body, resident blocks per CU
    long pxi_apply_cap = 4;            // MVX_PXI_APPLY_CAP: the same for the plain op's body
};
const Config &config();

typedef const char *(*SymFn)();

// The launched template as rocprofv3 names it ("k_combine<2, float, 2, 4, 1,
// 0>", "k_pxi_loc_body<11, 8, 1>"): the kernel's base name, O, the compiler's
// own spelling of T (void: the kernel has no type argument) and the remaining
// template arguments, so profiles and PMC summaries can be matched to what
// actually ran.
inline constexpr char K_COMBINE[] = "k_combine", K_TREE_BODY[] = "k_tree_body",
                      K_CHAIN_BODY[] = "k_chain_body", K_PXI_LOC_BODY[] = "k_pxi_loc_body",
                      K_COMBINE_F32[] = "k_combine_f32";

template <const char *BASE, int O, typename T, int... A>
static const char *ksym()
{
    static char buf[160];
    if (!buf[0]) {
        const char *pf = __PRETTY_FUNCTION__;
        const char *t = strstr(pf, ", T = ");
        const char *e = t ? strstr(t, ", A = ") : nullptr;
        const int args[] = {A..., 0};
        int len = snprintf(buf, sizeof buf, "%s<%d", BASE, O);
        if (!std::is_void<T>::value)
            len += snprintf(buf + len, sizeof buf - len, ", %.*s", (t && e) ? (int)(e - t - 6) : 1, (t && e) ? t + 6 : "?");
        for (size_t i = 0; i < sizeof...(A); ++i) len += snprintf(buf + len, sizeof buf - len, ", %d", args[i]);
        snprintf(buf + len, sizeof buf - len, ">");
    }
    return buf;
}

// One kernel instantiation as the launch policy sees it.
struct KVar {
    const void *fn;        // the kernel; null: the family has no such variant
    SymFn name;
    int unroll;            // chunks per lane per iteration (U)
    bool body;             // takes BodyParams (large aligned launches only), else Params
    int units;             // 16-byte units one thread moves per element (k_pxi_loc_body: 2)
    int cap;               // its own resident blocks per CU, by a dynamic LDS reservation (0: the family's)
    int kmin, kmax;        // the leaf counts it takes
};

// A kernel family: the cached build, the non-temporal one (NT) and, for large
// aligned launches, an optional body kernel (k_tree_body / k_chain_body /
// k_pxi_loc_body); fam is its residency class
enum { FAM_APPLY = 0, FAM_PROG, FAM_TREE, FAM_N };
enum { V_CACHED = 0, V_NT, V_BODY, V_N };
struct KFam {
    KVar var[V_N];
    int fam;
};

struct KSet {
    KFam apply;            // KMAX 2 (k <= 2)
    KFam prog;             // KMAX 8 combine program (masks)
    KFam prog2;            // 4-byte types: the U = 2 program (MVX_PROG_U=2); empty otherwise
    KFam prog4;            // programs over 3 or 4 leaves: KMAX 4 at U = 2 (MVX_PROG4=0: prog)
    KFam tree8, tree4;     // PROG = 1: full trees over 8 / 4 leaves
    KFam chain8, chain4;   // full chains over 8 / 4 leaves: k_chain_body, else the masked program
    KVar f32side[2];       // the f32-accumulating ops: k_combine_f32, f32 result [0] / f32 leaves [1]; else empty
    int esize;
    int chunk;             // bytes per chunk (16, or the element if wider)
    const char *name;
};

template <int O, typename T, int KMAX, int U, int NT, int PROG>
static KVar kvar_combine()
{
    return {(const void *)&k_combine<O, T, KMAX, U, NT, PROG>, &ksym<K_COMBINE, O, T, KMAX, U, NT, PROG>,
            U, false, 1, 0, 1, KMAX};
}

// k_pxi_loc_body over KMAX leaves at `cap` resident blocks per CU
template <int O, int KMAX, int U>
static KVar kvar_pxi_body(int cap)
{
    return {(const void *)&k_pxi_loc_body<O, KMAX, U>, &ksym<K_PXI_LOC_BODY, O, void, KMAX, U>,
            U, true, 2, cap, KMAX, KMAX};
}

template <int O, typename T, int KMAX, int U0, int U1, int PROG>
static KFam kfam(int fam)
{
    KFam f = {};
    f.var[V_CACHED] = kvar_combine<O, T, KMAX, U0, 0, PROG>();
    f.var[V_NT] = kvar_combine<O, T, KMAX, U1, 1, PROG>();
    f.fam = (fam == FAM_TREE && alu_heavy<T>::v) ? FAM_PROG : fam;
    if constexpr (PROG == 1 && !alu_heavy<T>::v) {
        f.var[V_BODY] = {(const void *)&k_tree_body<O, T, KMAX, U1>, &ksym<K_TREE_BODY, O, T, KMAX, U1>,
                         U1, true, 1, 0, KMAX, KMAX};
    } else if constexpr (PROG == 1 && std::is_same<T, pxi>::value && (O == OMAXLOC || O == OMINLOC)) {
        const Config &c = config();
        f.var[V_BODY] = c.pxi_u == 2 ? kvar_pxi_body<O, KMAX, 2>((int)c.pxi_cap)
                                     : kvar_pxi_body<O, KMAX, 1>((int)c.pxi_cap);
    }
    return f;
}

// a full chain: the masked program, with k_chain_body for large aligned
// launches (the 8-leaf one takes 5 to 8 leaves)
template <int O, typename T, int KMAX>
static KFam kchain()
{
    KFam f = kfam<O, T, MVX_COMBINE_KMAX, 1, 1, 0>(FAM_PROG);
    if constexpr (!alu_heavy<T>::v) {
        f.var[V_BODY] = {(const void *)&k_chain_body<O, T, KMAX, 2>, &ksym<K_CHAIN_BODY, O, T, KMAX, 2>,
                         2, true, 1, 0, KMAX == 8 ? 5 : KMAX, KMAX};
    }
    return f;
}

// Chunks in flight per lane, and (plan()) resident blocks per CU, for the
// non-temporal (large) launches -- round 2, tools/tune_occ.hip,
// profiles/r02/tune_occ.jsonl: at full occupancy a streaming launch keeps ~10x
// the bytes in flight Little's law needs and every HBM channel juggles rows
// from all the streams; fewer resident blocks with more loads each measured
// k = 8, 8 x 32 MiB: U1 uncapped 76.5 %, U2 at 2 blocks / CU 79.0 %;
// k = 8, 8 x 64 MiB: 77.0 % -> 79.9 % (BODY_LDS_CAP).  The plain op (k = 2)
// and the masked program gain nothing from a cap and keep U = 4 / 1 at full
// occupancy, as do the cached (small-launch) builds.
template <int O, typename T>
static KSet kset(const char *name)
{
    KSet s;
    s.apply = kfam<O, T, 2, 4, 4, 0>(FAM_APPLY);
    if constexpr (std::is_same<T, pxi>::value && (O == OMAXLOC || O == OMINLOC)) {
        // the plain op on MPI_LONG_DOUBLE_INT as lane pairs too (the trees'
        // k_pxi_loc_body with KMAX = 2): one 32-byte element per lane ran it
        // at 0.56 of HBM peak (profiles/r05/bench_kernels_all.jsonl)
        s.apply.var[V_BODY] = kvar_pxi_body<O, 2, 1>((int)config().pxi_apply_cap);
    }
    // (a 2-leaf body at U = 3 and 2 blocks per CU ran 123.8 vs 126.4 us in
    // the standalone sweep, profiles/r02/tune_occ_k2.jsonl, but 124.8 vs
    // 123.5-124.8 us in the product: not adopted)
    s.prog = kfam<O, T, MVX_COMBINE_KMAX, 1, 1, 0>(FAM_PROG);
    if constexpr (alu_heavy<T>::v) {
        // x87 (integer-emulated, ALU-bound) trees: U = 1 keeps 53-57 VGPRs
        // and 7-8 waves per SIMD (U = 2: 98, 4 waves); SUM tree k = 8 57.6 ->
        // 53.3 us (profiles/r02/bench_kernels_x87.jsonl)
        s.tree8 = kfam<O, T, 8, 1, 1, 1>(FAM_TREE);
        s.tree4 = kfam<O, T, 4, 1, 1, 1>(FAM_TREE);
    } else {
        s.tree8 = kfam<O, T, 8, 1, 2, 1>(FAM_TREE);
        s.tree4 = kfam<O, T, 4, 1, 2, 1>(FAM_TREE);
    }
    s.chain8 = kchain<O, T, 8>();
    s.chain4 = kchain<O, T, 4>();
    if constexpr (alu_heavy<T>::v) {
        s.prog4 = kfam<O, T, 4, 1, 1, 0>(FAM_PROG);
    } else {
        s.prog4 = kfam<O, T, 4, 2, 2, 0>(FAM_PROG);
    }
    if constexpr (sizeof(T) == 4) {
        s.prog2 = kfam<O, T, MVX_COMBINE_KMAX, 2, 2, 0>(FAM_PROG);
    } else {
        s.prog2 = {};
    }
    s.f32side[0] = s.f32side[1] = KVar{};
    if constexpr (acc_op<O>::v) {
        s.f32side[0] = {(const void *)&k_combine_f32<O, T, 0>, &ksym<K_COMBINE_F32, O, T, 0>, 1, false, 1, 0, 1, MVX_COMBINE_KMAX};
        s.f32side[1] = {(const void *)&k_combine_f32<O, T, 1>, &ksym<K_COMBINE_F32, O, T, 1>, 1, false, 1, 0, 1, MVX_COMBINE_KMAX};
    }
    s.esize = (int)sizeof(T);
    s.chunk = CG<T>::bytes;
    s.name = name;
    return s;
}

// element kinds of the datatype handles (mvx_mpi.h / reference mpi.h:64-115)
enum { EK_NONE = 0, EK_I8, EK_U8, EK_BYTE, EK_I16, EK_U16, EK_I32, EK_U32,
       EK_I64, EK_U64, EK_F32, EK_F64, EK_C32, EK_C64, EK_PFI, EK_PDI, EK_PLI,
       EK_PSI, EK_PII, EK_LDBL, EK_LDBL_INT,
       // derived contiguous types: count-2 pairs of one base, and the rest
       EK_PP8, EK_PP16, EK_PP64, EK_PPF, EK_PPD, EK_PPX, EK_DERIVED,
       EK_LOGICAL,
       // extension: MVX_FLOAT16, MVX_BFLOAT16, MVX_FLOAT8_E4M3, MVX_FLOAT8_E5M2
       EK_F16, EK_BF16, EK_F8E4M3, EK_F8E5M2 };

// Integer SUM/PROD/logical/bitwise results do not depend on signedness in
// two's complement, so those share the unsigned kernel of the same width;
// MAX/MIN compare and keep the signed kernels.
#define ARITH_INT(O, NAME)                                                   \
    case EK_I8: case EK_U8:   { static KSet s = kset<O, uint8_t>(NAME "_u8"); return &s; } \
    case EK_I16: case EK_U16: { static KSet s = kset<O, uint16_t>(NAME "_u16"); return &s; } \
    case EK_I32: case EK_U32: { static KSet s = kset<O, uint32_t>(NAME "_u32"); return &s; } \
    case EK_I64: case EK_U64: { static KSet s = kset<O, uint64_t>(NAME "_u64"); return &s; }
#define FLOATS(O, NAME)                                                      \
    case EK_F32: { static KSet s = kset<O, float>(NAME "_f32"); return &s; } \
    case EK_F64: { static KSet s = kset<O, double>(NAME "_f64"); return &s; }
#define HALFS(O, NAME)                                                       \
    case EK_F16:  { static KSet s = kset<O, f16>(NAME "_f16"); return &s; }  \
    case EK_BF16: { static KSet s = kset<O, bf16>(NAME "_bf16"); return &s; }
#define FP8S(O, NAME)                                                        \
    case EK_F8E4M3: { static KSet s = kset<O, f8e4m3>(NAME "_f8e4m3"); return &s; } \
    case EK_F8E5M2: { static KSet s = kset<O, f8e5m2>(NAME "_f8e5m2"); return &s; }
#define CMPLX(O, NAME)                                                       \
    case EK_C32: { static KSet s = kset<O, cf32>(NAME "_c32"); return &s; }  \
    case EK_C64: { static KSet s = kset<O, cf64>(NAME "_c64"); return &s; }
#define SIGNED_INT(O, NAME)                                                  \
    case EK_I8:  { static KSet s = kset<O, int8_t>(NAME "_i8"); return &s; } \
    case EK_U8:  { static KSet s = kset<O, uint8_t>(NAME "_u8"); return &s; } \
    case EK_I16: { static KSet s = kset<O, int16_t>(NAME "_i16"); return &s; } \
    case EK_U16: { static KSet s = kset<O, uint16_t>(NAME "_u16"); return &s; } \
    case EK_I32: { static KSet s = kset<O, int32_t>(NAME "_i32"); return &s; } \
    case EK_U32: { static KSet s = kset<O, uint32_t>(NAME "_u32"); return &s; } \
    case EK_I64: { static KSet s = kset<O, int64_t>(NAME "_i64"); return &s; } \
    case EK_U64: { static KSet s = kset<O, uint64_t>(NAME "_u64"); return &s; }
#define PAIRS(O, NAME)                                                       \
    case EK_PFI: { static KSet s = kset<O, pfi>(NAME "_float_int"); return &s; } \
    case EK_PDI: { static KSet s = kset<O, pdi>(NAME "_double_int"); return &s; } \
    case EK_PLI: { static KSet s = kset<O, pli>(NAME "_long_int"); return &s; } \
    case EK_PSI: { static KSet s = kset<O, psi>(NAME "_short_int"); return &s; } \
    case EK_PII: { static KSet s = kset<O, pii>(NAME "_2int"); return &s; }

#define LDBL(O, NAME)                                                        \
    case EK_LDBL: { static KSet s = kset<O, xf80>(NAME "_f80"); return &s; }
#define LDBL_INT(O, NAME)                                                    \
    case EK_LDBL_INT: { static KSet s = kset<O, pxi>(NAME "_long_double_int"); return &s; }
#define LOGICAL(O, NAME)                                                     \
    case EK_LOGICAL: { static KSet s = kset<O, flog>(NAME "_logical"); return &s; }
#define CONTIG_PAIRS(O, NAME)                                                \
    case EK_PP8:  { static KSet s = kset<O, pp<int8_t>>(NAME "_2char"); return &s; } \
    case EK_PP16: { static KSet s = kset<O, pp<int16_t>>(NAME "_2short"); return &s; } \
    case EK_PP64: { static KSet s = kset<O, pp<int64_t>>(NAME "_2long"); return &s; } \
    case EK_PPF:  { static KSet s = kset<O, pp<float>>(NAME "_2float"); return &s; } \
    case EK_PPD:  { static KSet s = kset<O, pp<double>>(NAME "_2double"); return &s; } \
    case EK_PPX:  { static KSet s = kset<O, pp<xf80>>(NAME "_2long_double"); return &s; }

// the per-op kernel tables, one translation unit each (nullptr: no case for
// that element kind in the op's switch -> the reference's 329)
const KSet *lookup_cmp(int op, int ek);     // MAX, MIN           mvx_ops_cmp.hip
const KSet *lookup_arith(int op, int ek);   // SUM, PROD          mvx_ops_arith.hip
const KSet *lookup_logic(int op, int ek);   // L* and B* ops      mvx_ops_logic.hip
int flog_sync();                            // MPI_LOGICAL's words on this device (mvx_ops_logic.hip)
const KSet *lookup_loc(int op, int ek);     // MAXLOC, MINLOC     mvx_ops_loc.hip
const KSet *lookup_half(int op, int ek);    // every op on the 16-bit floats  mvx_ops_half.hip
const KSet *lookup_fp8(int op, int ek);     // every op on the 8-bit floats   mvx_ops_fp8.hip
const KSet *lookup_acc32(int op, int ek);   // MVX_SUM_ACC32, MVX_PROD_ACC32  mvx_ops_acc32.hip

}  // namespace mvx
