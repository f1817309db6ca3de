#pragma once
// mvx_ops_fn.h -- the ops of the MPI local reduction path on elements and on
// chunks (what one lane moves per operand per step): element layouts, F<op, T>,
// Chunk / CG, the chunk op CF with its SWAR, packed-16 and 8-bit float forms.
// Last, the wide accumulator of the f32-accumulating ops (Wide, acc_steps,
// acc_chunk).  Device code only; the kernels that use them are in
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
       OSUMA, OPRODA };

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
template <int O> struct acc_op { static constexpr bool v = O == OSUMA || O == OPRODA; };

template <int O>
__device__ __forceinline__ float accf(float a, float b)
{
    static_assert(acc_op<O>::v, "");
    return O == OSUMA ? a + b : a * b;
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
// read (PROG = 1: k = KMAX).
template <int O, typename T, int KMAX, int PROG>
__device__ __forceinline__ void acc_chunk(Chunk<T> (&x)[KMAX], const Chunk<T> (&xf)[KMAX], unsigned fold_mask,
                                          int k, unsigned tree_mask, unsigned chain_mask)
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
        x[0].w[w] = Wide<T>::narrow(y[0]);
    }
}

}  // namespace mvx
