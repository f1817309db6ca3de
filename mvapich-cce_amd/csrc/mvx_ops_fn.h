#pragma once
// mvx_ops_fn.h -- the ops of the MPI local reduction path on elements and on
// chunks (what one lane moves per operand per step): element layouts, F<op, T>,
// Chunk / CG, the chunk op CF with its SWAR, packed-16 and 8-bit float forms.
// Last, the wide accumulator of the f32-accumulating ops (Wide, acc_steps,
// acc_chunk), MVX_AVG's finalising division (avg_fin, avg_chunk) and the
// scaled sum's scales and amax (Scl, scl_amax, wave_umax) and the stochastically
// rounded sum's counter-based bits and integer narrowing (Sr, sr_word_bits,
// sr_code).  Device code only; the kernels that use them are in
// mvx_ops_kern.h (design notes there).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "mvx_xf80.h"

namespace mvx {

enum { OMAX = 0, OMIN, OSUM, OPROD, OLAND, OBAND, OLOR, OBOR, OLXOR, OBXOR,
       OMINLOC, OMAXLOC,
       // extension (MVX_SUM_ACC32 / MVX_PROD_ACC32): the whole combine program
       // in binary32, narrowed once (the end of this file)
       OSUMA, OPRODA,
       // extension (MVX_AVG): the SUM program's value divided once by the rank
       // contributions it consumed (the end of this file)
       OAVG,
       // extension (MVX_SCALED_SUM): the f32 SUM program over leaves multiplied
       // by their ranks' scales, its value rescaled once, with a fused amax
       // (the end of this file)
       OSCL,
       // extension (MVX_SR_SUM): MVX_SUM_ACC32's f32 value narrowed by stochastic
       // rounding, the random bits a function of (seed, element index) alone
       // (the end of this file)
       OSR };
static_assert(OAVG == 14 && OSCL == 15 && OSR == 16, "");

// Element layouts: the reference's C types on x86-64 LP64.
struct cf32 { float re, im; };                          // global_ops.c:43-46
struct cf64 { double re, im; };                         // global_ops.c:48-51
struct pfi { float v; int32_t l; };                     // initdte.c:74-78
// The padding is an explicit member so the inout operand's padding bytes are
// carried through the register copy and written back unchanged (an unnamed
// hole is `undef` to LLVM); the reference never writes them either
// (global_ops.c:1335-1346 assign value and loc only).
struct pdi { double v; int32_t l; int32_t pad; };       // 16 B
struct pli { int64_t v; int32_t l; int32_t pad; };      // 16 B
struct psi { int16_t v; int16_t pad; int32_t l; };      // 8 B
struct pii { int32_t v; int32_t l; };                   // MPI_2INT
static_assert(sizeof(pdi) == 16 && sizeof(pli) == 16 && sizeof(psi) == 8, "");
// contiguous count-2 types over one base type (MPI_2INT's family, e.g.
// MPI_Type_contiguous(2, MPI_FLOAT)): value and loc both of the base type,
// global_ops.c:1387-1503 / 1625-1740
template <typename B> struct pp { B v; B l; };
static_assert(sizeof(pp<int8_t>) == 2 && sizeof(pp<double>) == 16, "");

// x87 long double (16-byte slot) and MPI_LONG_DOUBLE_INT (32 bytes):
// integer emulation of the x87 unit, mvx_xf80.h
using xf::xf80;
using xf::pxi;
static_assert(sizeof(xf80) == 16 && sizeof(pxi) == 32, "");
template <typename B> struct pp;

// the x87 types: every op is dozens of integer instructions, so their
// combines are ALU-bound and keep full occupancy (no k_tree_body, no
// residency cap: the 8-leaf x87 SUM tree ran 109.7 us at 2 blocks per CU
// against 74.4 us uncapped, profiles/r02/bench_kernels_x87.jsonl).  The
// MPI_LONG_DOUBLE_INT MAXLOC / MINLOC trees have their own body kernel,
// k_pxi_loc_body (one element per lane pair).
template <typename T> struct alu_heavy { static constexpr bool v = false; };
template <> struct alu_heavy<xf80> { static constexpr bool v = true; };
template <> struct alu_heavy<pxi> { static constexpr bool v = true; };
template <> struct alu_heavy<pp<xf80>> { static constexpr bool v = true; };

// ---------------------------------------------------------------------------
// the ops: F<op, T>::f(a, b) returns the new inout value (a = inout, b = in)

template <int O, typename T> struct F;

template <typename T> struct F<OMAX, T> {     // coll.h:17-18
    static __device__ __forceinline__ T f(T a, T b) { return (b > a) ? b : a; }
};
template <typename T> struct F<OMIN, T> {     // coll.h:14-15
    static __device__ __forceinline__ T f(T a, T b) { return (a > b) ? b : a; }
};

template <typename T> __device__ __forceinline__ T add_(T a, T b) { return (T)(a + b); }
template <typename T> __device__ __forceinline__ T mul_(T a, T b) { return (T)(a * b); }
// promote narrow unsigned before multiplying so the product cannot overflow int
template <> __device__ __forceinline__ uint8_t mul_(uint8_t a, uint8_t b)
{ return (uint8_t)((uint32_t)a * (uint32_t)b); }
template <> __device__ __forceinline__ uint16_t mul_(uint16_t a, uint16_t b)
{ return (uint16_t)((uint32_t)a * (uint32_t)b); }

template <typename T> struct F<OSUM, T> {
    static __device__ __forceinline__ T f(T a, T b) { return add_(a, b); }
};
template <> struct F<OSUM, cf32> {
    static __device__ __forceinline__ cf32 f(cf32 a, cf32 b)
    { cf32 r; r.re = a.re + b.re; r.im = a.im + b.im; return r; }
};
template <> struct F<OSUM, cf64> {
    static __device__ __forceinline__ cf64 f(cf64 a, cf64 b)
    { cf64 r; r.re = a.re + b.re; r.im = a.im + b.im; return r; }
};
template <typename T> struct F<OPROD, T> {
    static __device__ __forceinline__ T f(T a, T b) { return mul_(a, b); }
};
template <> struct F<OPROD, cf32> {            // global_ops.c:513-521
    static __device__ __forceinline__ cf32 f(cf32 c, cf32 b)
    { cf32 r; r.re = c.re * b.re - c.im * b.im; r.im = c.im * b.re + c.re * b.im; return r; }
};
template <> struct F<OPROD, cf64> {            // global_ops.c:523-531
    static __device__ __forceinline__ cf64 f(cf64 c, cf64 b)
    { cf64 r; r.re = c.re * b.re - c.im * b.im; r.im = c.im * b.re + c.re * b.im; return r; }
};
template <typename T> struct F<OLAND, T> {
    static __device__ __forceinline__ T f(T a, T b) { return (a != T(0) && b != T(0)) ? T(1) : T(0); }
};
template <typename T> struct F<OLOR, T> {
    static __device__ __forceinline__ T f(T a, T b) { return (a != T(0) || b != T(0)) ? T(1) : T(0); }
};
template <typename T> struct F<OLXOR, T> {
    static __device__ __forceinline__ T f(T a, T b) { return ((a != T(0)) != (b != T(0))) ? T(1) : T(0); }
};
template <typename T> struct F<OBAND, T> {
    static __device__ __forceinline__ T f(T a, T b) { return (T)(a & b); }
};
template <typename T> struct F<OBOR, T> {
    static __device__ __forceinline__ T f(T a, T b) { return (T)(a | b); }
};
template <typename T> struct F<OBXOR, T> {
    static __device__ __forceinline__ T f(T a, T b) { return (T)(a ^ b); }
};
// MAXLOC / MINLOC: global_ops.c:1297-1309 and 1524-1536, as selects
// (no divergent branches): equal values keep a's value and the smaller loc;
// otherwise b wins only if strictly larger (smaller); a NaN on either side
// compares false both ways, so a is kept.  The padding member comes from a.
template <typename T, bool MIN>
__device__ __forceinline__ T loc_op(T a, T b)
{
    const bool eq = a.v == b.v;
    const bool take = MIN ? (a.v > b.v) : (a.v < b.v);
    const decltype(a.l) lmin = (a.l > b.l) ? b.l : a.l;   // MPIR_MIN, coll.h:14-15
    T r = a;
    r.v = take ? b.v : a.v;
    r.l = eq ? lmin : (take ? b.l : a.l);
    return r;
}
template <typename T> struct F<OMAXLOC, T> {
    static __device__ __forceinline__ T f(T a, T b) { return loc_op<T, false>(a, b); }
};
template <typename T> struct F<OMINLOC, T> {
    static __device__ __forceinline__ T f(T a, T b) { return loc_op<T, true>(a, b); }
};
// contiguous(2, MPI_CHAR): the same op on 32-bit values.  On int8_t members
// the compiler chained the steps of a program as byte-select (SDWA)
// instructions and compared a sign-extended byte -- the value a previous step
// had selected -- with a zero-extended one (v_cmp_eq_u16_sdwa sext(x), y):
// equal negative values compared unequal and the loc = min rule was skipped
// from the second step on (element path of the 3- and 4-leaf programs;
// tests/test_gpu_kernel_matrix.py).  The empty asm makes the four widened
// values opaque, so every compare and select is a 32-bit one.
template <bool MIN>
__device__ __forceinline__ pp<int8_t> loc_op8(pp<int8_t> a, pp<int8_t> b)
{
    int av = a.v, al = a.l, bv = b.v, bl = b.l;
    __asm__("" : "+v"(av), "+v"(al), "+v"(bv), "+v"(bl));
    const bool eq = av == bv;
    const bool take = MIN ? (av > bv) : (av < bv);
    const int lmin = (al > bl) ? bl : al;
    pp<int8_t> r;
    r.v = (int8_t)(take ? bv : av);
    r.l = (int8_t)(eq ? lmin : (take ? bl : al));
    return r;
}
template <> struct F<OMAXLOC, pp<int8_t>> {
    static __device__ __forceinline__ pp<int8_t> f(pp<int8_t> a, pp<int8_t> b) { return loc_op8<false>(a, b); }
};
template <> struct F<OMINLOC, pp<int8_t>> {
    static __device__ __forceinline__ pp<int8_t> f(pp<int8_t> a, pp<int8_t> b) { return loc_op8<true>(a, b); }
};

// the x87 types (global_ops.c:149-155 and the HAVE_LONG_DOUBLE case of every
// op; 1365-1378 / 1605-1618 for LONG_DOUBLE_INT)
template <> struct F<OMAX, xf80> { static __device__ __forceinline__ xf80 f(xf80 a, xf80 b) { return xf::max(a, b); } };
template <> struct F<OMIN, xf80> { static __device__ __forceinline__ xf80 f(xf80 a, xf80 b) { return xf::min(a, b); } };
template <> struct F<OSUM, xf80> { static __device__ __forceinline__ xf80 f(xf80 a, xf80 b) { return xf::add(a, b); } };
template <> struct F<OPROD, xf80> { static __device__ __forceinline__ xf80 f(xf80 a, xf80 b) { return xf::mul(a, b); } };
template <> struct F<OLAND, xf80> { static __device__ __forceinline__ xf80 f(xf80 a, xf80 b) { return xf::land(a, b); } };
template <> struct F<OLOR, xf80> { static __device__ __forceinline__ xf80 f(xf80 a, xf80 b) { return xf::lor(a, b); } };
template <> struct F<OLXOR, xf80> { static __device__ __forceinline__ xf80 f(xf80 a, xf80 b) { return xf::lxor(a, b); } };
template <> struct F<OMAXLOC, pxi> { static __device__ __forceinline__ pxi f(pxi a, pxi b) { return xf::loc<false>(a, b); } };
template <> struct F<OMINLOC, pxi> { static __device__ __forceinline__ pxi f(pxi a, pxi b) { return xf::loc<true>(a, b); } };

// contiguous(2, MPI_LONG_DOUBLE) pairs (global_ops.c:1483-1496, 1720-1733):
// x87 compares of the values; equal -> loc = MPIR_MIN(a.l, b.l) (x87 select);
// b strictly larger (smaller) -> both of b's 10-byte values.  Each slot's
// padding stays the inout operand's.
template <bool MIN>
__device__ __forceinline__ pp<xf80> xloc2(pp<xf80> a, pp<xf80> b)
{
    const int c = xf::cmp(a.v, b.v);
    pp<xf80> r = a;
    if (c == 0) {
        r.l = xf::min(a.l, b.l);
    } else if (c == (MIN ? 1 : -1)) {
        r.v = xf::with_bits(a.v, b.v.m, b.v.se);
        r.l = xf::with_bits(a.l, b.l.m, b.l.se);
    }
    return r;
}
template <> struct F<OMAXLOC, pp<xf80>> { static __device__ __forceinline__ pp<xf80> f(pp<xf80> a, pp<xf80> b) { return xloc2<false>(a, b); } };
template <> struct F<OMINLOC, pp<xf80>> { static __device__ __forceinline__ pp<xf80> f(pp<xf80> a, pp<xf80> b) { return xloc2<true>(a, b); } };

// EXTENSION beyond the reference: the 16-bit floating types MVX_FLOAT16 and
// MVX_BFLOAT16 (include/mvx_mpi.h), treated as global_ops.c would treat one
// more C floating type next to float and double.  f16 is the compiler's IEEE
// binary16 and takes the generic ops above: every step is one correctly
// rounded half-precision instruction, subnormals kept.  bf16 is the upper
// half of a binary32: widened exactly by a shift, combined in f32 and
// narrowed round-to-nearest-even by the __bf16 conversion -- a sum or a
// product of two bf16 values rounded to f32 and then to bf16 equals the
// directly rounded one (24 >= 2 * 8 + 2; the product is exact in f32).  No
// step's f32 value is carried into the next.  MAX / MIN compare the widened
// values and keep the chosen operand's 16 bits; the logical ops store 1.0
// (0x3F80) or 0.
typedef _Float16 f16;
struct bf16 { uint16_t u; };
static_assert(sizeof(f16) == 2 && sizeof(bf16) == 2, "");

__device__ __forceinline__ float bits_f32(uint32_t w)
{
    float f;
    __builtin_memcpy(&f, &w, 4);
    return f;
}
__device__ __forceinline__ bf16 bf_narrow(float f)
{
    const __bf16 h = (__bf16)f;
    bf16 r;
    __builtin_memcpy(&r.u, &h, 2);
    return r;
}
template <int O>
__device__ __forceinline__ bf16 bf_op(bf16 a, bf16 b)
{
    const float x = bits_f32((uint32_t)a.u << 16), y = bits_f32((uint32_t)b.u << 16);
    bf16 t;
    if constexpr (O == OMAX) return (y > x) ? b : a;
    else if constexpr (O == OMIN) return (x > y) ? b : a;
    else if constexpr (O == OSUM) return bf_narrow(x + y);
    else if constexpr (O == OPROD) return bf_narrow(x * y);
    else if constexpr (O == OLAND) { t.u = (x != 0.0f && y != 0.0f) ? 0x3f80 : 0; return t; }
    else if constexpr (O == OLOR) { t.u = (x != 0.0f || y != 0.0f) ? 0x3f80 : 0; return t; }
    else { static_assert(O == OLXOR, ""); t.u = ((x != 0.0f) != (y != 0.0f)) ? 0x3f80 : 0; return t; }
}
#define MVX_BF16_OP(O)                                                        \
    template <> struct F<O, bf16> {                                           \
        static __device__ __forceinline__ bf16 f(bf16 a, bf16 b) { return bf_op<O>(a, b); } \
    };
MVX_BF16_OP(OMAX) MVX_BF16_OP(OMIN) MVX_BF16_OP(OSUM) MVX_BF16_OP(OPROD)
MVX_BF16_OP(OLAND) MVX_BF16_OP(OLOR) MVX_BF16_OP(OLXOR)
#undef MVX_BF16_OP

#ifdef MVX_OPS_LOGICAL_TU   // one TU owns the .TRUE. / .FALSE. words (mvx_ops_logic.hip)
// MPI_LOGICAL (dte_type MPIR_LOGICAL, one MPI_Fint): LAND / LOR / LXOR
// compare each word with the Fortran .TRUE. and store .TRUE. or .FALSE.
// (global_ops.c:646-655, 875-884, 1104-1113 with mpi_fort.h:11-19:
// FROM_FLOG(x) = x == MPIR_F_TRUE, TO_FLOG(v) = v ? MPIR_F_TRUE :
// MPIR_F_FALSE).  BAND / BOR / BXOR are bitwise on the word (678-684 ...)
// and run the 32-bit integer kernels.
struct flog { int32_t v; };
__constant__ int32_t g_flog[2] = {1, 0};     // MPIR_F_TRUE, MPIR_F_FALSE (gfortran)
__device__ __forceinline__ flog to_flog(bool t) { flog r; r.v = t ? g_flog[0] : g_flog[1]; return r; }
template <> struct F<OLAND, flog> {
    static __device__ __forceinline__ flog f(flog a, flog b) { return to_flog(a.v == g_flog[0] && b.v == g_flog[0]); }
};
template <> struct F<OLOR, flog> {
    static __device__ __forceinline__ flog f(flog a, flog b) { return to_flog(a.v == g_flog[0] || b.v == g_flog[0]); }
};
template <> struct F<OLXOR, flog> {
    static __device__ __forceinline__ flog f(flog a, flog b) { return to_flog((a.v == g_flog[0]) != (b.v == g_flog[0])); }
};
#endif

// A chunk is what one lane moves per operand per step: 16 bytes of
// elements, or one element of a wider type (MPI_LONG_DOUBLE_INT, 32 bytes:
// two dwordx4).  Moved to/from the registers by memcpy (a well-defined bit
// copy that keeps pair padding bytes; union punning lets clang drop the
// element writes).
template <typename T> struct CG {
    static constexpr int bytes = sizeof(T) > 16 ? (int)sizeof(T) : 16;
    static constexpr int w = bytes / 16;          // dwordx4 per chunk
    static constexpr int v = bytes / (int)sizeof(T);  // elements per chunk
};

template <typename T> struct Chunk {
    T e[CG<T>::v];
};
// 1-byte elements stay in their four 32-bit words (the SWAR chunk op, CF8):
// as 16 byte members the loads and stores were split into bytes and packed
// again around every op
template <> struct Chunk<uint8_t> { uint32_t w[4]; };
template <> struct Chunk<int8_t> { uint32_t w[4]; };

// The op over a whole chunk, a = op(a, b) element by element.  One-byte
// types run as SWAR on the chunk's four 32-bit words: element by element
// the compiler extracted, combined and re-packed every byte, and the 1-byte
// apply kernels ran at 0.65-0.73 of HBM peak against 0.78-0.81 for every
// wider type (tools/bench_kernels.py all, profiles/r05/bench_kernels_all.jsonl).
template <int O, typename T>
struct CF {
    static __device__ __forceinline__ void f(Chunk<T> &a, const Chunk<T> &b)
    {
#pragma unroll
        for (int j = 0; j < CG<T>::v; ++j) a.e[j] = F<O, T>::f(a.e[j], b.e[j]);
    }
};

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));   // one packed-16 register

// per byte of a word: 0x80 if the byte is nonzero, else 0
__device__ __forceinline__ uint32_t swar_nz(uint32_t x)
{
    return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}

// bytes as two packed-16 lanes each (even bytes, odd bytes), op lane-wise,
// low 8 bits of each lane kept: unsigned MAX / MIN, wrapping PROD
template <int O>
__device__ __forceinline__ uint32_t swar_p16(uint32_t a, uint32_t b)
{
    const uint32_t ae = a & 0x00ff00ffu, ao = (a >> 8) & 0x00ff00ffu;
    const uint32_t be = b & 0x00ff00ffu, bo = (b >> 8) & 0x00ff00ffu;
    u16x2 xe, xo, ye, yo, re, ro;
    __builtin_memcpy(&xe, &ae, 4); __builtin_memcpy(&xo, &ao, 4);
    __builtin_memcpy(&ye, &be, 4); __builtin_memcpy(&yo, &bo, 4);
    if constexpr (O == OMAX) { re = __builtin_elementwise_max(xe, ye); ro = __builtin_elementwise_max(xo, yo); }
    else if constexpr (O == OMIN) { re = __builtin_elementwise_min(xe, ye); ro = __builtin_elementwise_min(xo, yo); }
    else { re = xe * ye; ro = xo * yo; }
    uint32_t e, o;
    __builtin_memcpy(&e, &re, 4); __builtin_memcpy(&o, &ro, 4);
    return (e & 0x00ff00ffu) | ((o & 0x00ff00ffu) << 8);
}

// one word of four 1-byte elements, op O; SIGNED: int8_t MAX / MIN
template <int O, bool SIGNED>
__device__ __forceinline__ uint32_t swar8(uint32_t a, uint32_t b)
{
    if constexpr (O == OBAND) return a & b;
    else if constexpr (O == OBOR) return a | b;
    else if constexpr (O == OBXOR) return a ^ b;
    else if constexpr (O == OSUM) return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
    else if constexpr (O == OLAND) return (swar_nz(a) & swar_nz(b)) >> 7;
    else if constexpr (O == OLOR) return (swar_nz(a) | swar_nz(b)) >> 7;
    else if constexpr (O == OLXOR) return (swar_nz(a) ^ swar_nz(b)) >> 7;
    else if constexpr (SIGNED) return swar_p16<O>(a ^ 0x80808080u, b ^ 0x80808080u) ^ 0x80808080u;   // biased order
    else return swar_p16<O>(a, b);
}

template <int O, bool SIGNED>
struct CF8 {
    template <typename T>
    static __device__ __forceinline__ void f(Chunk<T> &a, const Chunk<T> &b)
    {
#pragma unroll
        for (int w = 0; w < 4; ++w) a.w[w] = swar8<O, SIGNED>(a.w[w], b.w[w]);
    }
};
template <int O> struct CF<O, uint8_t> {
    static __device__ __forceinline__ void f(Chunk<uint8_t> &a, const Chunk<uint8_t> &b) { CF8<O, false>::f(a, b); }
};
template <int O> struct CF<O, int8_t> {
    static __device__ __forceinline__ void f(Chunk<int8_t> &a, const Chunk<int8_t> &b) { CF8<O, true>::f(a, b); }
};

// The 16-bit floating types stay in their four 32-bit words too, two elements
// a word: W16<O, T>::f is the op on one word.
template <> struct Chunk<f16> { uint32_t w[4]; };
template <> struct Chunk<bf16> { uint32_t w[4]; };

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

template <int O, typename T> struct W16;

// f16: SUM / PROD are one packed instruction (v_pk_add_f16 / v_pk_mul_f16);
// MAX / MIN are a compare and a select per half, not v_pk_max / v_pk_min,
// whose NaN and signed-zero results are not the select's.
template <int O> struct W16<O, f16> {
    static __device__ __forceinline__ uint32_t f(uint32_t a, uint32_t b)
    {
        f16x2 x, y, r;
        __builtin_memcpy(&x, &a, 4);
        __builtin_memcpy(&y, &b, 4);
        if constexpr (O == OSUM) r = x + y;
        else if constexpr (O == OPROD) r = x * y;
        else { r.x = F<O, f16>::f(x.x, y.x); r.y = F<O, f16>::f(x.y, y.y); }
        uint32_t w;
        __builtin_memcpy(&w, &r, 4);
        return w;
    }
};

// bf16: the low half widens by a shift, the high half by a mask; SUM / PROD
// narrow both f32 results with one packed conversion (v_cvt_pk_bf16_f32);
// MAX / MIN select the original halves.
template <int O> struct W16<O, bf16> {
    static __device__ __forceinline__ uint32_t f(uint32_t a, uint32_t b)
    {
        const float xl = bits_f32(a << 16), xh = bits_f32(a & 0xffff0000u);
        const float yl = bits_f32(b << 16), yh = bits_f32(b & 0xffff0000u);
        if constexpr (O == OMAX || O == OMIN) {
            const bool tl = O == OMAX ? (yl > xl) : (xl > yl);
            const bool th = O == OMAX ? (yh > xh) : (xh > yh);
            return ((tl ? b : a) & 0xffffu) | ((th ? b : a) & 0xffff0000u);
        } else if constexpr (O == OSUM || O == OPROD) {
            f32x2 r;
            r.x = O == OSUM ? xl + yl : xl * yl;
            r.y = O == OSUM ? xh + yh : xh * yh;
            const bf16x2 h = __builtin_convertvector(r, bf16x2);
            uint32_t w;
            __builtin_memcpy(&w, &h, 4);
            return w;
        } else {
            const bool al = xl != 0.0f, ah = xh != 0.0f, bl = yl != 0.0f, bh = yh != 0.0f;
            bool tl, th;
            if constexpr (O == OLAND) { tl = al && bl; th = ah && bh; }
            else if constexpr (O == OLOR) { tl = al || bl; th = ah || bh; }
            else { static_assert(O == OLXOR, ""); tl = al != bl; th = ah != bh; }
            return (tl ? 0x3f80u : 0u) | (th ? 0x3f800000u : 0u);
        }
    }
};

template <int O, typename T>
struct CF16 {
    static __device__ __forceinline__ void f(Chunk<T> &a, const Chunk<T> &b)
    {
#pragma unroll
        for (int w = 0; w < 4; ++w) a.w[w] = W16<O, T>::f(a.w[w], b.w[w]);
    }
};
template <int O> struct CF<O, f16> {
    static __device__ __forceinline__ void f(Chunk<f16> &a, const Chunk<f16> &b) { CF16<O, f16>::f(a, b); }
};
template <int O> struct CF<O, bf16> {
    static __device__ __forceinline__ void f(Chunk<bf16> &a, const Chunk<bf16> &b) { CF16<O, bf16>::f(a, b); }
};

// EXTENSION beyond the reference: the 8-bit OCP floating types MVX_FLOAT8_E4M3
// (e4m3fn: bias 7, no infinities, NaN = 0x7F / 0xFF, largest finite 448) and
// MVX_FLOAT8_E5M2 (bias 15, IEEE-style), as one more C floating type each
// (DESIGN.md section 7).  gfx950 converts both natively: v_cvt_pk_f32_fp8 /
// _bf8 widen the pair of bytes in either half of a word exactly, and
// v_cvt_pk_fp8_f32 / _bf8_f32 narrow two f32 values round-to-nearest-even
// into either half of a word, keeping the other half -- so a word of four
// elements is never taken apart into bytes.  SUM / PROD work in f32 and narrow
// after every step: the f32 sum or product of two 8-bit floats narrowed once
// equals the directly rounded exact result (E4M3 sums and every product are
// exact in f32; for E5M2 sums 24 >= 2 * 3 + 2).  Overflow is not saturated,
// and the conversion itself sees to that: measured on the MI355X over all
// 65,536 operand pairs of either format, SUM and PROD, it gives NaN for a
// rounded E4M3 magnitude above 448 (the tie 464 goes to 448) and +-inf from
// the E5M2 tie 61440 on, as the OCP non-saturating conversion does.  (The
// ISA names one mode bit, FP16_OVFL, under which these conversions clamp
// instead; a compiled kernel's descriptor leaves it clear and nothing here
// writes mode registers.)  MAX / MIN compare the widened values and keep the
// chosen operand's byte.  The logical ops never widen: a byte is zero iff its
// seven magnitude bits are (-0 is zero, NaN is not), and they store 1.0
// (0x38 / 0x3C) or 0.
struct f8e4m3 { uint8_t u; };
struct f8e5m2 { uint8_t u; };
static_assert(sizeof(f8e4m3) == 1 && sizeof(f8e5m2) == 1, "");

template <typename T> struct fp8 {
    static constexpr bool e4m3 = std::is_same<T, f8e4m3>::value;
    // both elements of one half of a word (hi: bytes 2 and 3), exactly
    static __device__ __forceinline__ f32x2 widen(uint32_t w, bool hi)
    {
        if constexpr (e4m3) return hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
        else return hi ? __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false);
    }
    // r narrowed into one half of `old`, the other half kept (v_cvt_pk_*_f32
    // with op_sel)
    static __device__ __forceinline__ uint32_t narrow(f32x2 r, uint32_t old, bool hi)
    {
        if constexpr (e4m3) return (uint32_t)(hi ? __builtin_amdgcn_cvt_pk_fp8_f32(r.x, r.y, (int)old, true) : __builtin_amdgcn_cvt_pk_fp8_f32(r.x, r.y, (int)old, false));
        else return (uint32_t)(hi ? __builtin_amdgcn_cvt_pk_bf8_f32(r.x, r.y, (int)old, true) : __builtin_amdgcn_cvt_pk_bf8_f32(r.x, r.y, (int)old, false));
    }
};

// per byte of a word of 8-bit floats: 1.0 where t has 0x80, else 0 (0x38 =
// 0x40 - 0x08, 0x3C = 0x40 - 0x04: no borrow leaves a byte)
template <typename T>
__device__ __forceinline__ uint32_t fp8_truth(uint32_t t)
{
    return (t >> 1) - (t >> (fp8<T>::e4m3 ? 4 : 5));
}

// one word of four 8-bit floats; lanes: the bytes that count (the element
// path passes one element in byte 0 and the rest of the word is ignored)
template <int O, typename T>
__device__ __forceinline__ uint32_t fp8_word(uint32_t a, uint32_t b)
{
    if constexpr (O == OLAND || O == OLOR || O == OLXOR) {
        const uint32_t x = swar_nz(a & 0x7f7f7f7fu), y = swar_nz(b & 0x7f7f7f7fu);
        return fp8_truth<T>(O == OLAND ? (x & y) : O == OLOR ? (x | y) : (x ^ y));
    } else {
        const f32x2 xl = fp8<T>::widen(a, false), xh = fp8<T>::widen(a, true);
        const f32x2 yl = fp8<T>::widen(b, false), yh = fp8<T>::widen(b, true);
        if constexpr (O == OSUM || O == OPROD) {
            const f32x2 rl = O == OSUM ? xl + yl : xl * yl;
            const f32x2 rh = O == OSUM ? xh + yh : xh * yh;
            return fp8<T>::narrow(rh, fp8<T>::narrow(rl, 0u, false), true);
        } else {
            static_assert(O == OMAX || O == OMIN, "");
            // coll.h:14-19 on the decoded values: b's byte where the compare
            // holds (false for every NaN, and for -0 against +0), else a's
            const bool t0 = O == OMAX ? (yl.x > xl.x) : (xl.x > yl.x), t1 = O == OMAX ? (yl.y > xl.y) : (xl.y > yl.y);
            const bool t2 = O == OMAX ? (yh.x > xh.x) : (xh.x > yh.x), t3 = O == OMAX ? (yh.y > xh.y) : (xh.y > yh.y);
            const uint32_t m = (t0 ? 0xffu : 0u) | (t1 ? 0xff00u : 0u) | (t2 ? 0xff0000u : 0u) | (t3 ? 0xff000000u : 0u);
            return (a & ~m) | (b & m);
        }
    }
}

// the element path (heads, tails, mutually misaligned operands): the word op
// on byte 0
#define MVX_FP8_OP(O, T)                                                      \
    template <> struct F<O, T> {                                              \
        static __device__ __forceinline__ T f(T a, T b) { T r; r.u = (uint8_t)fp8_word<O, T>(a.u, b.u); return r; } \
    };
#define MVX_FP8_OPS(T)                                                        \
    MVX_FP8_OP(OMAX, T) MVX_FP8_OP(OMIN, T) MVX_FP8_OP(OSUM, T) MVX_FP8_OP(OPROD, T) \
    MVX_FP8_OP(OLAND, T) MVX_FP8_OP(OLOR, T) MVX_FP8_OP(OLXOR, T)
MVX_FP8_OPS(f8e4m3) MVX_FP8_OPS(f8e5m2)
#undef MVX_FP8_OPS
#undef MVX_FP8_OP

// the chunk stays in its four 32-bit words, 16 elements, as Chunk<uint8_t>
template <> struct Chunk<f8e4m3> { uint32_t w[4]; };
template <> struct Chunk<f8e5m2> { uint32_t w[4]; };

template <int O, typename T>
struct CFP8 {
    static __device__ __forceinline__ void f(Chunk<T> &a, const Chunk<T> &b)
    {
#pragma unroll
        for (int w = 0; w < 4; ++w) a.w[w] = fp8_word<O, T>(a.w[w], b.w[w]);
    }
};
template <int O> struct CF<O, f8e4m3> {
    static __device__ __forceinline__ void f(Chunk<f8e4m3> &a, const Chunk<f8e4m3> &b) { CFP8<O, f8e4m3>::f(a, b); }
};
template <int O> struct CF<O, f8e5m2> {
    static __device__ __forceinline__ void f(Chunk<f8e5m2> &a, const Chunk<f8e5m2> &b) { CFP8<O, f8e5m2>::f(a, b); }
};

// EXTENSION beyond the reference: MVX_SUM_ACC32 / MVX_PROD_ACC32 on the four
// narrow floating types.  A launch's whole combine
// program -- folds, tree steps, chain steps -- runs on binary32 values: every
// leaf is widened exactly, every step is one f32 add or multiply (round to
// nearest even, subnormals kept, nothing fused: -ffp-contract=off), and the
// result is narrowed once, by the narrowing the per-step ops use.  No narrow
// value exists in between.  A chunk is evaluated one 32-bit word of each leaf
// at a time -- Wide<T>::L f32 lanes per leaf, 4 for the 8-bit types and 2 for
// the 16-bit ones -- so 8 leaves x U chunks stay within the registers the
// per-step tree bodies use.
//
// MVX_AVG (OAVG), the ranks' mean: MPI_SUM's program, its value divided once
// by the number of rank contributions the whole program consumed (leaves plus
// fold partners; Params::divisor), then stored.  On float and double the
// program is F<OSUM, T>'s, step for step, and the division one correctly
// rounded IEEE division in T (a plain `/`: nothing here or in the Makefile
// allows a reciprocal or an approximate one; subnormals kept).  On the four
// narrow types the program is the f32 one above with accf = add, divided in
// binary32 and narrowed once -- the mean of eight E4M3 448s is 448, where the
// sum, per step or in f32, has no value to narrow to.  A divisor of 1 divides
// nothing, so a lone leaf keeps its bits.
template <typename T> struct narrow_float {
    static constexpr bool v = std::is_same<T, f16>::value || std::is_same<T, bf16>::value ||
                              std::is_same<T, f8e4m3>::value || std::is_same<T, f8e5m2>::value;
};
// the (op, type) pairs whose program runs on widened f32 values
template <int O, typename T> struct acc_op {
    static constexpr bool v = O == OSUMA || O == OPRODA || (O == OAVG && narrow_float<T>::v) || O == OSCL || O == OSR;
};

// MVX_SCALED_SUM (OSCL), the per-rank scaled sum: the f32 program above with
// accf = add, over leaves that are multiplied, right after they are widened,
// by the scale of the rank they came from (one f32 multiply each, fold
// partners by theirs); the program's value is multiplied once by oscale and
// narrowed once.  Where the caller asked for it, the largest magnitude of the
// values about to be narrowed is kept on the way: as the unsigned maximum of
// bits(v) & 0x7fffffff, which orders magnitudes as floats do and puts every
// NaN above infinity, so a NaN result leaves a NaN word.  A lane keeps its
// maximum in a register over everything it stores; at the end of the kernel a
// wave folds its 64 lanes with DPP row rotations and four v_readlane (no LDS:
// the body kernels' reservation is their residency cap) and one lane issues a
// single global_atomic_umax on the caller's word.  On float the leaves are
// their own f32 values (Wide<float>), so the same program serves it: MPI_SUM's
// per-step path cannot, the leaves change before the first step.
struct Scl {
    float lscale[8];      // per leaf: its rank's scale
    float fscale[8];      // per fold partner
    float oscale;         // the program's value, once
    unsigned *amax;       // device word for max |v| before narrowing, or null
};
// the scales in an OSCL kernel's launch parameters (SParams, SBodyParams); a
// template, so that the kernels written once for both parameter types name
// them only where O == OSCL is instantiated
template <int O, typename PT>
__device__ __forceinline__ const Scl &scl_of(const PT &P) { return P.sc; }

__device__ __forceinline__ uint32_t f32_bits(float f)
{
    uint32_t w;
    __builtin_memcpy(&w, &f, 4);
    return w;
}

template <int L>
__device__ __forceinline__ unsigned scl_amax(unsigned m, const float (&y)[L])
{
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const unsigned b = f32_bits(y[j]) & 0x7fffffffu;
        m = b > m ? b : m;
    }
    return m;
}

// the maximum over the wave's 64 lanes, in every lane; all lanes active
__device__ __forceinline__ unsigned wave_umax(unsigned m)
{
    unsigned t;
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x128, 0xF, 0xF, false); m = t > m ? t : m;   // row_ror:8
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x124, 0xF, 0xF, false); m = t > m ? t : m;   // row_ror:4
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x122, 0xF, 0xF, false); m = t > m ? t : m;   // row_ror:2
    t = (unsigned)__builtin_amdgcn_update_dpp(0, (int)m, 0x121, 0xF, 0xF, false); m = t > m ? t : m;   // row_ror:1
    unsigned r = (unsigned)__builtin_amdgcn_readlane((int)m, 0);
#pragma unroll
    for (int row = 1; row < 4; ++row) {
        t = (unsigned)__builtin_amdgcn_readlane((int)m, 16 * row);
        r = t > r ? t : r;
    }
    return r;
}

// the end of a kernel whose lanes kept a maximum each: at most one atomic per
// wave, and none from a wave whose maximum the word already holds.  The word
// only grows while kernels run, so a stale read can only cost an atomic that
// was not needed; without the read the 8 x 64 MiB tree's 32768 waves queued
// on one address for 390 us against 95 us (tools/bench_kernels.py scaled).
__device__ __forceinline__ void amax_commit(unsigned *amax, unsigned m)
{
    m = wave_umax(m);
    if ((threadIdx.x & 63) == 0 && m > __hip_atomic_load(amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(amax, m);
}

// a lone unfolded leaf that no scale touches is copied, bits and all
__device__ __forceinline__ bool scl_unit(const Scl &sc) { return sc.lscale[0] == 1.0f && sc.oscale == 1.0f; }

template <int O>
__device__ __forceinline__ float accf(float a, float b)
{
    static_assert(O == OSUMA || O == OPRODA || O == OAVG || O == OSCL || O == OSR, "");
    return O == OPRODA ? a * b : a + b;
}

template <> struct F<OAVG, float> : F<OSUM, float> {};
template <> struct F<OAVG, double> : F<OSUM, double> {};

// the finalising step between the program and the single store (V: float or
// double); every op but OAVG passes its value through
template <int O, typename V>
__device__ __forceinline__ V avg_fin(V y, int divisor)
{
    if constexpr (O == OAVG) return divisor == 1 ? y : y / (V)divisor;
    else return y;
}

// one word of a chunk <-> its L elements as f32 lanes
template <typename T> struct Wide;

template <typename T> struct WideFP8 {
    static constexpr int L = 4;
    static __device__ __forceinline__ void widen(uint32_t w, float (&y)[4])
    {
        const f32x2 lo = fp8<T>::widen(w, false), hi = fp8<T>::widen(w, true);
        y[0] = lo.x; y[1] = lo.y; y[2] = hi.x; y[3] = hi.y;
    }
    static __device__ __forceinline__ uint32_t narrow(const float (&y)[4])
    {
        f32x2 lo, hi;
        lo.x = y[0]; lo.y = y[1]; hi.x = y[2]; hi.y = y[3];
        return fp8<T>::narrow(hi, fp8<T>::narrow(lo, 0u, false), true);
    }
};
template <> struct Wide<f8e4m3> : WideFP8<f8e4m3> {};
template <> struct Wide<f8e5m2> : WideFP8<f8e5m2> {};

template <> struct Wide<bf16> {
    static constexpr int L = 2;
    static __device__ __forceinline__ void widen(uint32_t w, float (&y)[2])
    {
        y[0] = bits_f32(w << 16);
        y[1] = bits_f32(w & 0xffff0000u);
    }
    static __device__ __forceinline__ uint32_t narrow(const float (&y)[2])   // v_cvt_pk_bf16_f32
    {
        f32x2 r;
        r.x = y[0]; r.y = y[1];
        const bf16x2 h = __builtin_convertvector(r, bf16x2);
        uint32_t w;
        __builtin_memcpy(&w, &h, 4);
        return w;
    }
};

// float (the scaled sum alone): a word is its own f32 value
template <> struct Wide<float> {
    static constexpr int L = 1;
    static __device__ __forceinline__ void widen(uint32_t w, float (&y)[1]) { y[0] = bits_f32(w); }
    static __device__ __forceinline__ uint32_t narrow(const float (&y)[1]) { return f32_bits(y[0]); }
};

// f16: v_cvt_f32_f16 widens exactly (subnormals included); the pair of a
// word narrows with one v_cvt_pk_f16_f32 (the element path's single value with
// v_cvt_f16_f32), round-to-nearest-even under the kernel's default rounding
// mode, to a subnormal, +-inf or a NaN where the value asks for one
template <> struct Wide<f16> {
    static constexpr int L = 2;
    static __device__ __forceinline__ void widen(uint32_t w, float (&y)[2])
    {
        f16x2 h;
        __builtin_memcpy(&h, &w, 4);
        y[0] = (float)h.x;
        y[1] = (float)h.y;
    }
    static __device__ __forceinline__ uint32_t narrow(const float (&y)[2])
    {
        f16x2 h;
        h.x = (f16)y[0];
        h.y = (f16)y[1];
        uint32_t w;
        __builtin_memcpy(&w, &h, 4);
        return w;
    }
};

// the element path: one element in lane 0 of a word
template <typename T>
__device__ __forceinline__ float widen_elt(const T *p)
{
    uint32_t w = 0;
    __builtin_memcpy(&w, p, sizeof(T));
    float y[Wide<T>::L];
    Wide<T>::widen(w, y);
    return y[0];
}
template <typename T>
__device__ __forceinline__ void narrow_elt(T *p, float v)
{
    float y[Wide<T>::L] = {};
    y[0] = v;
    const uint32_t w = Wide<T>::narrow(y);
    __builtin_memcpy(p, &w, sizeof(T));
}

// The combine program (mvx_ops_kern.h: reduce_leaves) on L f32 lanes per
// leaf.  PROG = 1: the full balanced tree over KMAX leaves.
template <int O, int KMAX, int L, int PROG>
__device__ __forceinline__ void acc_steps(float (&y)[KMAX][L], int k, unsigned tree_mask, unsigned chain_mask)
{
    if constexpr (PROG == 1) {
#pragma unroll
        for (int h = 1; h < KMAX; h <<= 1)
#pragma unroll
            for (int q = 0; q + h < KMAX; q += 2 * h)
#pragma unroll
                for (int j = 0; j < L; ++j) y[q][j] = accf<O>(y[q][j], y[q + h][j]);
    } else if constexpr (KMAX == 2) {
        if (k == 2) {
#pragma unroll
            for (int j = 0; j < L; ++j) y[0][j] = accf<O>(y[0][j], y[1][j]);
        }
    } else {
#pragma unroll
        for (int l = 0; (1 << l) < KMAX; ++l) {
#pragma unroll
            for (int q = 0; q + (1 << l) < KMAX; ++q) {
                if (tree_mask & (1u << (l * 8 + q))) {
#pragma unroll
                    for (int j = 0; j < L; ++j) y[q][j] = accf<O>(y[q][j], y[q + (1 << l)][j]);
                }
            }
        }
#pragma unroll
        for (int q = 1; q < KMAX; ++q) {
            if (chain_mask & (1u << q)) {
#pragma unroll
                for (int j = 0; j < L; ++j) y[0][j] = accf<O>(y[0][j], y[q][j]);
            }
        }
    }
}

// One chunk of every leaf: x[0] = narrow(program(widen(x[q]) op widen(xf[q])
// where fold_mask has bit q)), a word at a time.  Leaves q >= k are never
// read (PROG = 1: k = KMAX).  OAVG divides the f32 value before narrowing it.
template <int O, typename T, int KMAX, int PROG>
__device__ __forceinline__ void acc_chunk(Chunk<T> (&x)[KMAX], const Chunk<T> (&xf)[KMAX], unsigned fold_mask,
                                          int k, unsigned tree_mask, unsigned chain_mask, int divisor)
{
    constexpr int L = Wide<T>::L;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        float y[KMAX][L];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (PROG == 1 || q < k) {
                Wide<T>::widen(x[q].w[w], y[q]);
                if (PROG == 0 && (fold_mask & (1u << q))) {
                    float f[L];
                    Wide<T>::widen(xf[q].w[w], f);
#pragma unroll
                    for (int j = 0; j < L; ++j) y[q][j] = accf<O>(y[q][j], f[j]);
                }
            }
        }
        acc_steps<O, KMAX, L, PROG>(y, k, tree_mask, chain_mask);
#pragma unroll
        for (int j = 0; j < L; ++j) y[0][j] = avg_fin<O>(y[0][j], divisor);
        x[0].w[w] = Wide<T>::narrow(y[0]);
    }
}

template <typename T>
__device__ __forceinline__ uint32_t chunk_word(const Chunk<T> &x, int w)
{
    if constexpr (std::is_same<T, float>::value) return f32_bits(x.e[w]);
    else return x.w[w];
}

// OSCL's acc_chunk: the leaves scaled as they are widened, the value rescaled
// once; returns the chunk's amax where sc.amax asks for one (else 0).  On float
// a word is an element (Wide<float>).
template <typename T, int KMAX, int PROG>
__device__ __forceinline__ unsigned scl_chunk(Chunk<T> (&x)[KMAX], const Chunk<T> (&xf)[KMAX], unsigned fold_mask,
                                              int k, unsigned tree_mask, unsigned chain_mask, const Scl &sc)
{
    constexpr int L = Wide<T>::L;
    unsigned am = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        float y[KMAX][L];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (PROG == 1 || q < k) {
                Wide<T>::widen(chunk_word(x[q], w), y[q]);
#pragma unroll
                for (int j = 0; j < L; ++j) y[q][j] *= sc.lscale[q];
                if (PROG == 0 && (fold_mask & (1u << q))) {
                    float f[L];
                    Wide<T>::widen(chunk_word(xf[q], w), f);
#pragma unroll
                    for (int j = 0; j < L; ++j) y[q][j] = accf<OSCL>(y[q][j], f[j] * sc.fscale[q]);
                }
            }
        }
        acc_steps<OSCL, KMAX, L, PROG>(y, k, tree_mask, chain_mask);
#pragma unroll
        for (int j = 0; j < L; ++j) y[0][j] *= sc.oscale;
        if (sc.amax) am = scl_amax(am, y[0]);
        if constexpr (std::is_same<T, float>::value) x[0].e[w] = y[0][0];
        else x[0].w[w] = Wide<T>::narrow(y[0]);
    }
    return am;
}

// OSCL's lone leaf that is copied: the amax of the chunk's widened elements
template <typename T>
__device__ __forceinline__ unsigned amax_chunk(const Chunk<T> &x)
{
    unsigned am = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        float y[Wide<T>::L];
        Wide<T>::widen(chunk_word(x, w), y);
        am = scl_amax(am, y);
    }
    return am;
}

// MVX_SR_SUM (OSR), the stochastically rounded sum: MVX_SUM_ACC32's program
// and f32 value, narrowed to one of its two neighbours in T with probability
// proportional to the distance to the other (DESIGN.md section 7 has the
// definition the bits are held to).  The random bits are no generator's state
// but a counter-based function of (seed, index of the element in the
// collective's reduced vector): whatever the grid, the kernel family, the
// operands' alignment or the cut of a launch, an element draws the same bits.
// One 32-bit hash H(g) serves the group g of L elements that share a word
// (L = 4 or 2), so the chunk path pays one hash a word -- or, where the words
// of a launch start `o` elements into a group, the hashes of both groups a
// word straddles, funnel-shifted (v_alignbit) into the word's bits; adjacent
// words share a hash, 5 for a chunk.  H's inner constant c depends on the high
// half of g alone and stays in a register from chunk to chunk (SrC).
struct Sr {
    uint32_t s0, s1;      // the seed's halves
    uint64_t first;       // index of dst[0] in the reduced vector
};
template <int O, typename PT>
__device__ __forceinline__ const Sr &sr_of(const PT &P) { return P.sr; }

__device__ __forceinline__ uint32_t fmix32(uint32_t h)
{
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}
__device__ __forceinline__ uint32_t sr_c(const Sr &sr, uint32_t hi) { return fmix32(hi ^ sr.s1 ^ 0x85EBCA77u); }
__device__ __forceinline__ uint32_t sr_h(const Sr &sr, uint32_t lo, uint32_t c)
{
    return fmix32((lo ^ sr.s0) * 0x9E3779B1u + c);
}
__device__ __forceinline__ uint32_t sr_hash(const Sr &sr, uint64_t g)
{
    return sr_h(sr, (uint32_t)g, sr_c(sr, (uint32_t)(g >> 32)));
}

// the target formats: mantissa bits, exponent bias, random bits an element
// draws, the code every magnitude past the largest finite one gets (inf; NaN
// on E4M3, which has no inf), bits of an element
template <typename T> struct SrFmt;
template <> struct SrFmt<f16> { static constexpr int M = 10, BIAS = 15, NB = 16, OVF = 0x7c00, BITS = 16; };
template <> struct SrFmt<bf16> { static constexpr int M = 7, BIAS = 127, NB = 16, OVF = 0x7f80, BITS = 16; };
template <> struct SrFmt<f8e4m3> { static constexpr int M = 3, BIAS = 7, NB = 8, OVF = 0x7f, BITS = 8; };
template <> struct SrFmt<f8e5m2> { static constexpr int M = 2, BIAS = 15, NB = 8, OVF = 0x7c, BITS = 8; };

// the lane's c, kept while the high half of the group index stays
struct SrC { uint32_t hi, c; };
__device__ __forceinline__ SrC src_none() { return {0xffffffffu, 0u}; }   // (no group index is that high)

// the bits of element i alone (heads, tails, the element path)
template <typename T>
__device__ __forceinline__ uint32_t sr_elt_bits(const Sr &sr, uint64_t i)
{
    constexpr int L = Wide<T>::L, NB = SrFmt<T>::NB;
    return (sr_hash(sr, i / L) >> (NB * (int)(i & (L - 1)))) & ((1u << NB) - 1);
}

// the bits of N consecutive words of elements, the first of which is element
// i0 of the reduced vector, o = i0 % L elements into its group (uniform over
// the launch: a scalar branch)
template <typename T, int N>
__device__ __forceinline__ void sr_word_bits(const Sr &sr, uint64_t i0, int o, SrC &cc, uint32_t (&rb)[N])
{
    constexpr int L = Wide<T>::L, NB = SrFmt<T>::NB;
    const uint64_t g0 = i0 / L;
    const uint32_t lo0 = (uint32_t)g0, hi0 = (uint32_t)(g0 >> 32);
    uint32_t h[N + 1];
    if (lo0 > 0xffffffffu - N) {          // the high half changes inside: c per hash
#pragma unroll
        for (int j = 0; j <= N; ++j) h[j] = sr_hash(sr, g0 + j);
    } else {
        if (hi0 != cc.hi) {
            cc.hi = hi0;
            cc.c = sr_c(sr, hi0);
        }
#pragma unroll
        for (int j = 0; j < N; ++j) h[j] = sr_h(sr, lo0 + j, cc.c);
        h[N] = o ? sr_h(sr, lo0 + N, cc.c) : 0u;
    }
    if (o) {
#pragma unroll
        for (int j = 0; j < N; ++j) rb[j] = __builtin_amdgcn_alignbit(h[j + 1], h[j], (uint32_t)(o * NB));
    } else {
#pragma unroll
        for (int j = 0; j < N; ++j) rb[j] = h[j];
    }
}

// A finite f32 value's bits u narrowed with r, NB random bits: integer
// arithmetic on the bit pattern.  With the significand M (implicit one set)
// shifted so that the target's last kept bit q lands on bit NB, the bits below
// are floor(f * 2^NB) and adding r carries into q exactly when t + r >= 2^NB;
// the carry runs on into the exponent, up to the overflow code.  Below the
// least normal exponent q stays 2^(emin - m): the shift grows by the distance
// (31 and more shift everything out: the value is below every chance), and
// the units are the subnormal's code.  bf16 has f32's exponents: its code is
// the upper half of u + r, subnormals and the carry into inf included.
template <typename T>
__device__ __forceinline__ uint32_t sr_code(uint32_t u, uint32_t r)
{
    typedef SrFmt<T> Fm;
    if constexpr (std::is_same<T, bf16>::value) {
        return (u + r) >> 16;
    } else {
        constexpr int SH = 23 - Fm::M, PRE = Fm::NB > SH ? Fm::NB - SH : 0, POST = SH > Fm::NB ? SH - Fm::NB : 0;
        const int et = (int)((u >> 23) & 0xffu) - (127 - Fm::BIAS);   // the target's biased exponent
        const uint32_t m = ((u & 0x7fffffu) | 0x800000u) << PRE;
        const int below = et < 1 ? 1 - et : 0;
        const int sh = below + POST < 31 ? below + POST : 31;
        const uint32_t units = ((m >> sh) + r) >> Fm::NB;
        uint32_t code = ((uint32_t)(et < 1 ? 0 : et - 1) << Fm::M) + units;
        code = code < (uint32_t)Fm::OVF ? code : (uint32_t)Fm::OVF;
        return code | ((u >> 31) << (Fm::BITS - 1));
    }
}

// a word's L f32 values narrowed with the word's bits rb (element j's in bits
// NB * j up); inf and NaN go the round-to-nearest way, as they always have
template <typename T>
__device__ __forceinline__ uint32_t sr_narrow(const float (&y)[Wide<T>::L], uint32_t rb)
{
    constexpr int L = Wide<T>::L, NB = SrFmt<T>::NB, BITS = SrFmt<T>::BITS;
    constexpr uint32_t RM = (1u << NB) - 1, EM = (1u << BITS) - 1;
    const uint32_t rne = Wide<T>::narrow(y);
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < L; ++j) {
        const uint32_t u = f32_bits(y[j]);
        const uint32_t code = sr_code<T>(u, (rb >> (NB * j)) & RM) & EM;
        const bool finite = (u & 0x7f800000u) != 0x7f800000u;
        w |= (finite ? code : (rne >> (BITS * j)) & EM) << (BITS * j);
    }
    return w;
}

// the element path's narrow_elt: r is the element's own bits
template <typename T>
__device__ __forceinline__ void narrow_elt_sr(T *p, float v, uint32_t r)
{
    float y[Wide<T>::L] = {};
    y[0] = v;
    const uint32_t w = sr_narrow<T>(y, r);
    __builtin_memcpy(p, &w, sizeof(T));
}

// OSR's acc_chunk: the f32 program of acc_chunk<OSUMA>, each word narrowed
// with its bits rb[w]
template <typename T, int KMAX, int PROG>
__device__ __forceinline__ void sr_chunk(Chunk<T> (&x)[KMAX], const Chunk<T> (&xf)[KMAX], unsigned fold_mask,
                                         int k, unsigned tree_mask, unsigned chain_mask, const uint32_t (&rb)[4])
{
    constexpr int L = Wide<T>::L;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        float y[KMAX][L];
#pragma unroll
        for (int q = 0; q < KMAX; ++q) {
            if (PROG == 1 || q < k) {
                Wide<T>::widen(x[q].w[w], y[q]);
                if (PROG == 0 && (fold_mask & (1u << q))) {
                    float f[L];
                    Wide<T>::widen(xf[q].w[w], f);
#pragma unroll
                    for (int j = 0; j < L; ++j) y[q][j] = accf<OSR>(y[q][j], f[j]);
                }
            }
        }
        acc_steps<OSR, KMAX, L, PROG>(y, k, tree_mask, chain_mask);
        x[0].w[w] = sr_narrow<T>(y[0], rb[w]);
    }
}

// OAVG on float and double: the finalising step on every element of the
// chunk that holds the per-step program's result
template <int O, typename T>
__device__ __forceinline__ void avg_chunk(Chunk<T> &x, int divisor)
{
    if constexpr (O == OAVG) {
#pragma unroll
        for (int j = 0; j < CG<T>::v; ++j) x.e[j] = avg_fin<O>(x.e[j], divisor);
    }
}

}  // namespace mvx
