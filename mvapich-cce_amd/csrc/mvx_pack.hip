// mvx_pack.hip -- device pack / unpack of derived datatypes (libmvx_hip.so).
//
// The type engine (mvx_dtype.hip, host code) owns the handles and their maps;
// this file owns what a type needs on the device (PackCache, hung off the
// type through mvx_dtype.h), the four kernel families and the rules that
// choose one (pack(), at the end).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "mvx_mpi.h"
#include "mvx_hip.h"
#include "mvx_dtype.h"

namespace mvx {
namespace dt {

// A derived type's device side, made at its first pack or unpack and freed
// with the type (pack_cache_free).  Index w of the arrays: W = 16, 8, 4, 2, 1.
struct PackCache {
    PackView t;                 // the type: extent, size, map
    // the map on the device, split into pieces of <= 64 bytes
    void *dmap;
    long dmap_n;
    // the map as W-byte units: each unit's offset in the element, in packed
    // order; 0: not built; -1: the map does not split into W-byte units (2
    // and 1 serve the tile kernels only)
    int *dunits[5];
    long units[5];
    // after the units in dunits[w] (W <= 8): the offsets of the G = 16 / W
    // units of a 16-byte packed chunk, per chunk phase -- tabP[w] phases
    // (a period of tabP chunks holds whole elements), 0: no table
    long tabP[5];
    // the tile kernels' LDS swizzle for W (swz_pick): 0 none, else s -- bits
    // [s, s + 3) of a tile byte address XORed into its 16-byte slot index
    int swz[5];
    // the map's reach [mlo, mhi) around the element origin (its hull), and
    // whole-word unpack (merge_ok): 0 not decided, 1 yes, -1 no
    long mlo, mhi;
    int merge;
};

void pack_cache_free(PackCache *c)
{
    if (c->dmap) (void)hipFree(c->dmap);
    for (int w = 0; w < 5; ++w)
        if (c->dunits[w]) (void)hipFree(c->dunits[w]);
    delete c;
}

// The A/B knobs, all on by default and `NAME=0` off; each is read once per
// process, at its first use.
//   MVX_PACK_UNITS        0: the piece kernel only
//   MVX_PACK_TILES        0: no pack through LDS tiles, the unit kernel instead
//   MVX_PACK_CHUNK_TAB    0: k_pack_tiles steps its unit offsets per unit
//   MVX_UNPACK_MERGE      0: the unit kernel's byte-exact stores everywhere
//   MVX_UNPACK_CHUNK_TAB  0: k_unpack_merge steps its unit offsets per unit
//   MVX_LDS_SWIZZLE       0: the tile kernels keep their LDS layout linear
enum Knob { PACK_UNITS, PACK_TILES, PACK_CHUNK_TAB, UNPACK_MERGE, UNPACK_CHUNK_TAB, LDS_SWIZZLE, KNOBS };
static bool knob(Knob k)
{
    static const char *const name[KNOBS] = {"MVX_PACK_UNITS",   "MVX_PACK_TILES",       "MVX_PACK_CHUNK_TAB",
                                            "MVX_UNPACK_MERGE", "MVX_UNPACK_CHUNK_TAB", "MVX_LDS_SWIZZLE"};
    static int on[KNOBS];       // 0: not read yet, 1: off, 2: on
    if (!on[k]) {
        const char *e = getenv(name[k]);
        on[k] = e && atoi(e) == 0 ? 1 : 2;
    }
    return on[k] == 2;
}

static long gcd(long a, long b)
{
    while (b) { const long r = a % b; a = b; b = r; }
    return a;
}

// A run-time choice handed to f as a compile-time constant, f(K<v>()):
// `decltype(k)::value` is a template argument there.  The unit width:
template <int V> using K = std::integral_constant<int, V>;
template <class F> static int with_width(int W, F f)
{
    return W == 16 ? f(K<16>()) : W == 8 ? f(K<8>()) : W == 4 ? f(K<4>()) : W == 2 ? f(K<2>()) : f(K<1>());
}
// the six variants of a tile kernel, f(K<from>(), K<swz>()): a unit's offset
// from the unit table in global memory or in LDS, or from the chunk table
enum { OFF_GLOBAL, OFF_LDS, OFF_TAB };
template <class F> static void with_variant(int from, bool swz, F f)
{
    auto s = [&](auto fr) { swz ? f(fr, K<1>()) : f(fr, K<0>()); };
    from == OFF_TAB ? s(K<OFF_TAB>()) : from == OFF_LDS ? s(K<OFF_LDS>()) : s(K<OFF_GLOBAL>());
}

// ---- pack / unpack --------------------------------------------------------
// One work item = one piece (<= 64 bytes) of one element's type map.
// Consecutive threads take consecutive pieces, so the packed side is
// written contiguously; each thread copies with the widest access its
// addresses allow.

struct DBlk { long off, poff; int len, pad; };

// The last pack / unpack kernel launched, as rocprofv3 names the template
// (mvx_type_last_kernel_symbol; "memcpy" for a basic type): each spelling is
// formatted once and kept, so a launch only stores a pointer.
static const char *g_last_sym = "";
static const char *tf(bool b) { return b ? "true" : "false"; }
// b0..b2: the kernel's three bool template arguments in template order
static const char *sym_tile(bool unpack, int W, int tile, bool b0, bool b1, bool b2)
{
    static char buf[2][5][8][64];
    const int wi = W == 16 ? 0 : W == 8 ? 1 : W == 4 ? 2 : W == 2 ? 3 : 4;
    char *s = buf[unpack][wi][b0 * 4 + b1 * 2 + b2];
    if (!s[0])
        snprintf(s, 64, "%s<%d, %d, %s, %s, %s>", unpack ? "k_unpack_merge" : "k_pack_tiles", W, tile, tf(b0), tf(b1),
                 tf(b2));
    return s;
}
static const char *sym_units(bool pack, int W, int U, bool lds)
{
    static char buf[2][3][2][64];
    char *s = buf[pack][W == 16 ? 0 : W == 8 ? 1 : 2][lds];
    if (!s[0]) snprintf(s, 64, "k_pack_units<%s, %d, %d, %s>", tf(pack), W, U, tf(lds));
    return s;
}

template <bool PACK>
__global__ void __launch_bounds__(256)
k_pack(const char *__restrict__ src, char *__restrict__ dst, const DBlk *__restrict__ map, long nblk,
       long count, long extent, long size)
{
    const long items = count * nblk;
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < items; t += (long)gridDim.x * 256) {
        const long i = t / nblk;
        const DBlk m = map[t - i * nblk];
        const char *s = PACK ? src + i * extent + m.off : src + i * size + m.poff;
        char *d = PACK ? dst + i * size + m.poff : dst + i * extent + m.off;
        const uintptr_t a = (uintptr_t)s | (uintptr_t)d | (uintptr_t)m.len;
        if ((a & 15) == 0) {
            for (int b = 0; b < m.len; b += 16) *(uint4 *)(d + b) = *(const uint4 *)(s + b);
        } else if ((a & 3) == 0) {
            for (int b = 0; b < m.len; b += 4) *(uint32_t *)(d + b) = *(const uint32_t *)(s + b);
        } else {
            for (int b = 0; b < m.len; ++b) d[b] = s[b];
        }
    }
}

// Units of W bytes (tools/bench_pack.py: the piece kernel above reached
// 0.25-0.39 of HBM peak on every shape, 64 KiB of the packed stream per
// wave spread over 64 pieces and a 64-bit division per piece).  Lane l of
// the grid takes packed units l, l + T, l + 2T, ... (T the grid's threads):
// one wave reads or writes 64 consecutive units of the packed stream, and on
// the extent side the units of one block are consecutive too.  The unit's
// (element, unit-in-element) pair advances by the grid stride's (D, R) with
// no division after the first; U units per lane are in flight at once.
typedef uint32_t pu32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t pu32x4 __attribute__((ext_vector_type(4)));
template <int W> struct UnitT;
template <> struct UnitT<1> { typedef uint8_t t; };
template <> struct UnitT<2> { typedef uint16_t t; };
template <> struct UnitT<4> { typedef uint32_t t; };
template <> struct UnitT<8> { typedef pu32x2 t; };
template <> struct UnitT<16> { typedef pu32x4 t; };

#define UNITS_LDS 2048   // unit tables this small are read from LDS
#define CHUNK_TAB_MAX 2048   // chunk tables (PackCache::tabP) up to this many entries

template <bool PACK, int W, int U, bool LDS>
__global__ void __launch_bounds__(256)
k_pack_units(const char *__restrict__ src, char *__restrict__ dst, const int *__restrict__ uoff, long upe,
             long count, long extent, long D, long R)
{
    typedef typename UnitT<W>::t V;
    __shared__ int s_uoff[LDS ? UNITS_LDS : 1];
    if constexpr (LDS) {
        for (int u = threadIdx.x; u < (int)upe; u += 256) s_uoff[u] = uoff[u];
        __syncthreads();
    }
    const long T = (long)gridDim.x * 256;
    const long N = count * upe;
    const long DX = D * extent;                   // the element offset's advance per grid stride
    long q = (long)blockIdx.x * 256 + threadIdx.x;
    long i = q / upe, j = q - i * upe;
    long ix = i * extent;                         // i * extent, carried
    while (q < N) {
        // (a flag per unit, not a null destination: a pointer that may be
        // null was addressed through flat stores, each waiting for every load)
        V v[U];
        long to[U];
        bool ok[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            ok[k] = q < N;
            to[k] = 0;
            if (ok[k]) {
                const long e = ix + (LDS ? s_uoff[j] : uoff[j]);
                const char *from = PACK ? src + e : src + q * W;
                to[k] = PACK ? q * W : e;
                v[k] = __builtin_nontemporal_load((const V *)from);
            }
            q += T;
            ix += DX;
            j += R;
            if (j >= upe) { j -= upe; ix += extent; }
        }
#pragma unroll
        for (int k = 0; k < U; ++k)
            if (ok[k]) __builtin_nontemporal_store(v[k], (V *)(dst + to[k]));
    }
}

// LDS bank conflicts of the tile kernels' unit accesses, modelled
// (MI355X_MICROARCH.md LDS: 1-, 2- and 4-byte reads and every write bank
// (a / 4) mod 32 over 32-lane groups, 8-byte reads mod 64): lane l of a group
// takes chunk l, units G l .. G l + G - 1 of the stream, so when an element's
// units repeat every 128 or 256 bytes of the extent layout, lanes a few
// apart hit one bank (struct {char; hole; int}: 7-way, every other float:
// 8-way).  Swizzle candidates s = 7, 8, 9 (tile byte a lives at
// a ^ (((a >> s) & 7) << 4): 16-byte slots permuted within 128-byte rows,
// so whole 16-byte words stay whole) against none, averaged over a few
// group starts and element offsets in the tile; the best if it saves a
// fifth of the extra cycles, else 0.
static int swz_pick(const std::vector<int> &u, long upe, long ext, int W)
{
    const int G = 16 / W, banks = W == 8 ? 64 : 32;
    const int cand[4] = {0, 7, 8, 9};
    const long starts[4] = {0, 13, 32, 77}, offs[3] = {0, 5, 10};
    double cost[4] = {0, 0, 0, 0};
    if (ext <= 0 || ext > 4096 || upe <= 0) return 0;
    for (int ci = 0; ci < 4; ++ci)
        for (long st : starts)
            for (long e0 : offs)
                for (int g = 0; g < G; ++g) {
                    long dw[32];
                    int per[64] = {0}, worst = 1;
                    for (int l = 0; l < 32; ++l) {
                        const long q = (st + l) * G + g, e = q / upe, j = q % upe;
                        long a = e * ext + e0 + u[(size_t)j] + 4096;    // (offsets may be negative)
                        if (cand[ci]) a ^= ((a >> cand[ci]) & 7) << 4;
                        dw[l] = a / 4;
                    }
                    std::sort(dw, dw + 32);                        // distinct dwords per bank
                    for (int l = 0; l < 32; ++l)
                        if (!l || dw[l] != dw[l - 1]) {
                            const int c = ++per[dw[l] % banks];
                            if (c > worst) worst = c;
                        }
                    cost[ci] += worst - 1;
                }
    int best = 0;
    for (int ci = 1; ci < 4; ++ci)
        if (cost[ci] < cost[best]) best = ci;
    return best && cost[best] <= 0.8 * cost[0] ? cand[best] : 0;
}

// the unit table for W (index wi), built once per type; false if the map
// does not split into W-byte units
static bool unit_table(PackCache &pc, int W, int wi)
{
    const PackView &t = pc.t;
    if (pc.units[wi] < 0) return false;
    if (pc.dunits[wi]) return true;
    std::vector<int> u;
    bool ok = t.extent > 0 && t.extent % W == 0 && t.size % W == 0 && t.size / W <= (1L << 22);
    for (long b = 0; ok && b < t.nblk; ++b) {
        const Blk &m = t.map[b];
        if (((m.off % W) + W) % W || m.len % W || m.off < INT32_MIN || m.off + m.len > INT32_MAX) { ok = false; break; }
        for (long o = 0; o < m.len; o += W) u.push_back((int)(m.off + o));
    }
    if (!ok || u.empty()) { pc.units[wi] = -1; return false; }
    const long upe = (long)u.size();
    pc.tabP[wi] = 0;
    if (W <= 8) {
        // chunk c, unit g: unit q = c G + g of the stream; with c = k P + p,
        // its element is k EPP + (p G + g) / upe and its offset in that
        // element u[(p G + g) % upe] (EPP = P G / upe elements per period)
        const long G = 16 / W, P = upe / gcd(upe, G);
        if (P * G <= CHUNK_TAB_MAX && (P * G / upe + 1) * t.extent < INT32_MAX / 2) {
            for (long q = 0; q < P * G; ++q) u.push_back((int)((q / upe) * t.extent + u[(size_t)(q % upe)]));
            pc.tabP[wi] = P;
        }
    }
    pc.swz[wi] = W <= 8 ? swz_pick(u, upe, t.extent, W) : 0;
    if (hipMalloc(&pc.dunits[wi], u.size() * sizeof(int)) != hipSuccess) {
        pc.dunits[wi] = nullptr;
        pc.units[wi] = -1;
        return false;
    }
    if (hipMemcpy(pc.dunits[wi], u.data(), u.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(pc.dunits[wi]);
        pc.dunits[wi] = nullptr;
        pc.units[wi] = -1;
        return false;
    }
    pc.units[wi] = upe;
    return true;
}

template <bool PACK, int W>
static int launch_units(const PackCache &pc, int wi, const void *src, void *dst, long count, hipStream_t st)
{
    constexpr int U = 4;
    const long upe = pc.units[wi], N = count * upe, extent = pc.t.extent;
    long blocks = (N + 256L * U - 1) / (256L * U);
    if (blocks > 65536) blocks = 65536;
    if (blocks < 1) blocks = 1;
    const long T = blocks * 256;
    g_last_sym = sym_units(PACK, W, U, upe <= UNITS_LDS);
    auto go = [&](auto lds) {
        hipLaunchKernelGGL((k_pack_units<PACK, W, U, decltype(lds)::value != 0>), dim3((unsigned)blocks), dim3(256), 0,
                           st, (const char *)src, (char *)dst, (const int *)pc.dunits[wi], upe, count, extent, T / upe,
                           T % upe);
    };
    upe <= UNITS_LDS ? go(K<1>()) : go(K<0>());
    return hipGetLastError() == hipSuccess ? MPI_SUCCESS : MPI_ERR_OTHER;
}

// ---- unpack by whole words ------------------------------------------------
// The unit kernel's unpack stores W bytes per unit: where the type map
// leaves holes inside a 64-byte DRAM sector, every such store is a partial
// write the memory must merge with the sector's old bytes.  This variant
// merges on the CU instead: a workgroup owns a 16-byte-aligned tile of the
// destination, loads it whole into LDS, writes the tile's units (read from
// the packed stream, contiguous per tile) over it in LDS, and stores the
// tile back whole -- full-line reads and writes only.  The hole bytes go
// back as they were read, so this is for destinations no one else writes
// meanwhile (MVX_UNPACK_MERGE=0 keeps the byte-exact stores).  Words that
// reach outside the hull of the whole buffer's type maps (its first and
// last) are never written whole: their units are stored directly.
#define MERGE_TILE 8192              // destination bytes per workgroup (LDS)
#define MERGE_UNITS_LDS 2048

template <int W> __device__ inline typename UnitT<W>::t unit_of(const pu32x4 &v, int g);
template <> __device__ inline uint32_t unit_of<4>(const pu32x4 &v, int g) { return v[g]; }
template <> __device__ inline pu32x2 unit_of<8>(const pu32x4 &v, int g)
{
    pu32x2 r;
    r.x = v[2 * g];
    r.y = v[2 * g + 1];
    return r;
}
template <> __device__ inline pu32x4 unit_of<16>(const pu32x4 &v, int) { return v; }
template <> __device__ inline uint16_t unit_of<2>(const pu32x4 &v, int g)
{
    return (uint16_t)(v[g >> 1] >> (16 * (g & 1)));
}
template <> __device__ inline uint8_t unit_of<1>(const pu32x4 &v, int g)
{
    return (uint8_t)(v[g >> 2] >> (8 * (g & 3)));
}

// the LDS byte address of tile byte a under the swizzle (PackCache::swz)
template <bool SWZ> __device__ inline int lds_at(int a, int s) { return SWZ ? a ^ (((a >> s) & 7) << 4) : a; }

// unit g (W bytes) of a 16-byte chunk being assembled
template <int W> __device__ inline void set_unit(pu32x4 &v, int g, typename UnitT<W>::t x);
template <> __device__ inline void set_unit<8>(pu32x4 &v, int g, pu32x2 x)
{
    v[2 * g] = x.x;
    v[2 * g + 1] = x.y;
}
template <> __device__ inline void set_unit<16>(pu32x4 &v, int, pu32x4 x) { v = x; }
template <> __device__ inline void set_unit<4>(pu32x4 &v, int g, uint32_t x) { v[g] = x; }
template <> __device__ inline void set_unit<2>(pu32x4 &v, int g, uint16_t x)
{
    const int s = 16 * (g & 1);
    v[g >> 1] = (v[g >> 1] & ~(0xffffu << s)) | ((uint32_t)x << s);
}
template <> __device__ inline void set_unit<1>(pu32x4 &v, int g, uint8_t x)
{
    const int s = 8 * (g & 3);
    v[g >> 2] = (v[g >> 2] & ~(0xffu << s)) | ((uint32_t)x << s);
}

// The unit offsets come from LDS (LDSU, up to MERGE_UNITS_LDS units per
// element) or from global memory: a template argument, not a run-time
// select -- a select between the two made the compiler address both through
// flat loads and stores in the inner loop.  Units outside the tile go to a
// trash word past its end (a select on the LDS address, no branch), and the
// hull's two edge words are stored byte by byte, so every unit of the tile
// is one LDS store.
template <int W, int TILE, bool LDSU, bool SWZ, bool TAB>
__global__ void __launch_bounds__(256)
k_unpack_merge(const char *__restrict__ packed, char *__restrict__ dst, const int *__restrict__ uoff, long upe,
               long n, long ext, long lo, long hi, uintptr_t a0, uintptr_t h0, uintptr_t h1, int swz, long tabP)
{
    typedef typename UnitT<W>::t V;
    __shared__ pu32x4 s_tile[TILE / 16 + 1];            // + the trash word
    __shared__ __attribute__((aligned(16))) int s_uoff[LDSU || TAB ? MERGE_UNITS_LDS : 1];
    if (TAB)                                            // the chunk table (k_pack_tiles)
        for (int u = threadIdx.x; u < (int)(tabP * (16 / W)); u += 256) s_uoff[u] = uoff[upe + u];
    else if (LDSU)
        for (int u = threadIdx.x; u < (int)upe; u += 256) s_uoff[u] = uoff[u];
    const uintptr_t t0 = a0 + (uintptr_t)blockIdx.x * TILE;                // this tile's first word
    const uintptr_t tend = t0 + TILE < ((h1 + 15) & ~(uintptr_t)15) ? t0 + TILE
                                                                           : ((h1 + 15) & ~(uintptr_t)15);
    const int nw = (int)((tend - t0) / 16);
    for (int w = threadIdx.x; w < nw; w += 256)
        *(pu32x4 *)((char *)s_tile + lds_at<SWZ>(16 * w, swz)) =
            __builtin_nontemporal_load((const pu32x4 *)(t0 + 16 * (uintptr_t)w));
    __syncthreads();
    // the elements whose maps reach into [t0, tend): relative to dst
    const long a = (long)(t0 - (uintptr_t)dst), b = (long)(tend - (uintptr_t)dst);
    long ilo = a - hi >= 0 ? (a - hi) / ext + 1 : 0;
    long ihi = b - lo > 0 ? (b - lo + ext - 1) / ext : 0;
    if (ihi > n) ihi = n;
    // the units of those elements, read 16 bytes of the packed stream (G
    // units) per lane, two chunks in flight; a chunk that runs past the
    // stream's end is read unit by unit.  Offsets from here are 32-bit and
    // relative to the tile (an element's reach and the extent are bounded,
    // merge_ok): unit j of element ilo + ir lands at ir * ext + e0 + uoff[j]
    constexpr int G = 16 / W;
    const int up = (int)upe, ext32 = (int)ext, span = (int)(tend - t0);
    const int e0 = (int)(ilo * ext - a);
    const long q0 = ilo * upe, qn = n * upe, c0 = q0 / G, c1 = (ihi * upe + G - 1) / G;
    // TAB: chunk c0 + d is phase (p0 + d) % P of period k0 + (p0 + d) / P,
    // whose first element is (k0 + ...) EPP; relative to element ilo: b0
    const unsigned P = (unsigned)tabP, p0 = TAB ? (unsigned)(c0 % (long)P) : 0;
    const int epp = TAB ? (int)((long)P * G / upe) : 0;
    const int b0 = TAB ? (int)(c0 / (long)P * epp - ilo) : 0;
    for (long c = c0 + threadIdx.x; c < c1; c += 512) {
        pu32x4 v[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long cc = c + 256 * u;
            if (cc < c1 && (cc + 1) * G <= qn) v[u] = __builtin_nontemporal_load((const pu32x4 *)(packed + 16 * cc));
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const long cc = c + 256 * u;
            if (cc >= c1) continue;
            const int valid = qn - cc * G < G ? (int)(qn - cc * G) : G;   // units of the chunk in the stream
            if (valid < G) {                       // the stream's last, partial chunk: unit by unit
                v[u] = pu32x4{0, 0, 0, 0};
                for (int g = 0; g < valid; ++g) set_unit<W>(v[u], g, *(const V *)(packed + (cc * G + g) * W));
            }
            int rel[G];
            if constexpr (TAB) {
                const unsigned cr = (unsigned)(cc - c0) + p0, kk = cr / P, p = cr - kk * P;
                const int base = (b0 + (int)kk * epp) * ext32 + e0;
#pragma unroll
                for (int g4 = 0; g4 < G; g4 += 4) {
                    if constexpr (G >= 4) {
                        const pu32x4 t4 = *(const pu32x4 *)&s_uoff[p * G + g4];
#pragma unroll
                        for (int g = 0; g < 4; ++g) rel[g4 + g] = base + (int)t4[g];
                    } else {
#pragma unroll
                        for (int g = 0; g < G; ++g) rel[g] = base + s_uoff[p * G + g];
                    }
                }
            } else {
                // > -G: the first chunk may start in elements before ilo
                // (several when an element has fewer than G units), whose
                // units all land below the tile (ilo is the first element
                // reaching it); ir is the floor of qr / up, so j is a unit
                // index in every case
                const int qr = (int)(cc * G - q0);
                int ir = qr >= 0 ? (int)((unsigned)qr / (unsigned)up) : -(int)((unsigned)(up - 1 - qr) / (unsigned)up);
                int j = qr - ir * up;
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    rel[g] = ir * ext32 + e0 + (LDSU ? s_uoff[j] : uoff[j]);
                    if (++j == up) { j = 0; ++ir; }
                }
            }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const bool in = (g < valid) & ((unsigned)rel[g] < (unsigned)span);
                *(V *)((char *)s_tile + (in ? lds_at<SWZ>(rel[g], swz) : TILE)) = unit_of<W>(v[u], g);
            }
        }
    }
    __syncthreads();
    for (int w = threadIdx.x; w < nw; w += 256) {
        const uintptr_t at = t0 + 16 * (uintptr_t)w;
        if (at >= h0 && at + 16 <= h1) {
            __builtin_nontemporal_store(*(const pu32x4 *)((const char *)s_tile + lds_at<SWZ>(16 * w, swz)),
                                        (pu32x4 *)at);
        } else {                                   // an edge word of the hull: its hull bytes only
            const uintptr_t b0 = at > h0 ? at : h0, b1 = at + 16 < h1 ? at + 16 : h1;
            const char *word = (const char *)s_tile + lds_at<SWZ>(16 * w, swz);
            for (uintptr_t b = b0; b < b1; ++b) *(char *)b = word[b - at];
        }
    }
}

// Whether whole-word unpack pays for a map of reach [l, h) around the element
// origin: the maps of neighbouring elements must not interleave (each
// destination byte has one writer), and the map must leave holes inside 64-B
// sectors (partial writes), with no 64-B sector of the hull wholly untouched
// (one that a byte-exact unpack would not touch at all but the merge would
// read and write).
static bool merge_pays(const PackView &t, long l, long h)
{
    if (!t.nblk || t.extent <= 0 || t.extent > (1L << 30)) return false;   // 32-bit tile offsets
    if (h - l > t.extent) return false;
    const long reps = 64 / gcd(t.extent, 64), span = t.extent * reps;
    if (span > (1L << 20)) return false;
    std::vector<unsigned char> cov((size_t)span + 64, 0);
    for (long r = 0; r < reps; ++r)
        for (const Blk *b = t.map; b < t.map + t.nblk; ++b)
            for (long o = 0; o < b->len; ++o) {
                const long x = ((r * t.extent + b->off + o - l) % span + span) % span;
                cov[(size_t)x] = 1;
            }
    bool partial = false;
    for (long s = 0; s < span; s += 64) {
        int c = 0;
        for (long k = s; k < s + 64 && k < span; ++k) c += cov[(size_t)k];
        if (c == 0) return false;
        if (c < 64) partial = true;
    }
    return partial;
}

// decided once per type
static bool merge_ok(PackCache &pc)
{
    if (!pc.merge) pc.merge = merge_pays(pc.t, pc.mlo, pc.mhi) ? 1 : -1;
    return pc.merge > 0;
}

template <int W>
static int launch_merge(const PackCache &pc, int wi, const void *src, void *dst, long count, hipStream_t st)
{
    const long upe = pc.units[wi], ext = pc.t.extent, lo = pc.mlo, hi = pc.mhi;
    const uintptr_t h0 = (uintptr_t)dst + lo, h1 = (uintptr_t)dst + (count - 1) * ext + hi;
    const uintptr_t a0 = h0 & ~(uintptr_t)15;
    // 8 KiB tiles (4 KiB ran 30-40 % slower, 16 KiB 0-8 % slower:
    // profiles/r06/pack_tile_sizes.txt, pack_tile_sizes_noflat.txt)
    const long tiles = (long)((((h1 + 15) & ~(uintptr_t)15) - a0 + MERGE_TILE - 1) / MERGE_TILE);
    if (tiles < 1 || tiles > INT32_MAX) return MPI_ERR_OTHER;
    const int sw = knob(LDS_SWIZZLE) ? pc.swz[wi] : 0;
    // the chunk table for 1- and 2-byte units (as k_pack_tiles; MVX_PACK_CHUNK_TAB)
    const bool tb = knob(UNPACK_CHUNK_TAB) && W <= 2 && pc.tabP[wi] > 0;
    with_variant(tb ? OFF_TAB : upe <= MERGE_UNITS_LDS ? OFF_LDS : OFF_GLOBAL, sw != 0, [&](auto from, auto swz) {
        constexpr bool LU = decltype(from)::value == OFF_LDS, TB = decltype(from)::value == OFF_TAB;
        constexpr bool SW = decltype(swz)::value != 0;
        g_last_sym = sym_tile(true, W, MERGE_TILE, LU, SW, TB);
        hipLaunchKernelGGL((k_unpack_merge<W, MERGE_TILE, LU, SW, TB>), dim3((unsigned)tiles), dim3(256), 0, st,
                           (const char *)src, (char *)dst, (const int *)pc.dunits[wi], upe, count, ext, lo, hi, a0,
                           h0, h1, sw, pc.tabP[wi]);
    });
    return hipGetLastError() == hipSuccess ? MPI_SUCCESS : MPI_ERR_OTHER;
}

// ---- pack by whole words ----------------------------------------------------
// The unit kernel's pack reads 4 or 8 bytes per lane from the extent layout
// and writes as many to the packed stream: four or two times the memory
// instructions of 16-byte accesses, with each read instruction spread over
// several lines.  This variant gives a workgroup a run of whole elements:
// it loads their hull into LDS with 16-byte loads (whole aligned words: a
// word holding one hull byte lies in the same page, so the read is safe),
// then each lane gathers G = 16 / W units from LDS into one 16-byte chunk of
// the packed stream and stores it whole.  A run's packed bytes start on a
// 64-byte boundary (its element count is a multiple of 64 / gcd(size, 64));
// the stream's last, partial chunk is stored unit by unit.  (The kernel
// needs only 16-byte tile starts; pack_ept makes them 64-byte ones.)
#define PACK_TILE 8192               // LDS bytes of extent layout per workgroup

// TAB: the chunk table (PackCache::tabP phases after the unit offsets) in LDS
// instead of the unit offsets: a chunk's G unit offsets are one vector LDS
// read and one add each, with no per-unit element / unit-index stepping
template <int W, int TILE, bool LDSU, bool TAB, bool SWZ>
__global__ void __launch_bounds__(256)
k_pack_tiles(const char *__restrict__ src, char *__restrict__ dst, const int *__restrict__ uoff, long upe, long n,
             long ext, long lo, long hi, long ept, long tabP, int swz)
{
    typedef typename UnitT<W>::t V;
    constexpr int G = 16 / W;
    __shared__ pu32x4 s_tile[TILE / 16];
    __shared__ __attribute__((aligned(16))) int s_uoff[LDSU || TAB ? MERGE_UNITS_LDS : 1];   // LDSU: as in k_unpack_merge
    if (TAB)
        for (int u = threadIdx.x; u < (int)(tabP * G); u += 256) s_uoff[u] = uoff[upe + u];
    else if (LDSU)
        for (int u = threadIdx.x; u < (int)upe; u += 256) s_uoff[u] = uoff[u];
    const long i0 = (long)blockIdx.x * ept;
    const long i1 = i0 + ept < n ? i0 + ept : n;
    const uintptr_t a0 = ((uintptr_t)src + i0 * ext + lo) & ~(uintptr_t)15;
    const uintptr_t a1 = ((uintptr_t)src + (i1 - 1) * ext + hi + 15) & ~(uintptr_t)15;
    const int nw = (int)((a1 - a0) / 16);
    for (int w = threadIdx.x; w < nw; w += 256)
        *(pu32x4 *)((char *)s_tile + lds_at<SWZ>(16 * w, swz)) =
            __builtin_nontemporal_load((const pu32x4 *)(a0 + 16 * (uintptr_t)w));
    __syncthreads();
    const long qn = n * upe, qlo = i0 * upe, qhi = i1 * upe;
    const long c0 = qlo / G, c1 = (qhi + G - 1) / G;      // qlo is a multiple of G (ept)
    // 32-bit, tile-relative from here (pack_ept bounds the extent): unit j
    // of element i0 + ir sits at ir * ext + e0 + uoff[j] in the tile
    const int up = (int)upe, ext32 = (int)ext;
    const int e0 = (int)(i0 * ext - (long)(a0 - (uintptr_t)src));
    // TAB: chunk c0 + k P + p is phase p of period k, whose first element is
    // i0 + k EPP -- the tile starts a period: i0 is a multiple of pack_ept's
    // step 64 / gcd(size, 64), which EPP = G / gcd(upe, G) divides
    const unsigned P = (unsigned)tabP;
    const int epp = TAB ? (int)((long)P * G / upe) : 0;
    for (long c = c0 + threadIdx.x; c < c1; c += 256) {
        if (TAB && (c + 1) * G <= qn) {
            const unsigned cr = (unsigned)(c - c0), kk = cr / P, p = cr - kk * P;
            const int base = (int)kk * epp * ext32 + e0;
            pu32x4 out = {0, 0, 0, 0};
#pragma unroll
            for (int g4 = 0; g4 < G; g4 += 4) {
                int o[4];
                if constexpr (G >= 4) {
                    const pu32x4 t4 = *(const pu32x4 *)&s_uoff[p * G + g4];
                    o[0] = (int)t4[0]; o[1] = (int)t4[1]; o[2] = (int)t4[2]; o[3] = (int)t4[3];
                } else {
#pragma unroll
                    for (int g = 0; g < G; ++g) o[g] = s_uoff[p * G + g];
                }
#pragma unroll
                for (int g = 0; g < (G < 4 ? G : 4); ++g)
                    set_unit<W>(out, g4 + g, *(const V *)((const char *)s_tile + lds_at<SWZ>(base + o[g], swz)));
            }
            __builtin_nontemporal_store(out, (pu32x4 *)(dst + 16 * c));
            continue;
        }
        const unsigned qr = (unsigned)(c * G - qlo);
        int ir = (int)(qr / (unsigned)up), j = (int)qr - ir * up;
        if ((c + 1) * G <= qn) {
            pu32x4 out = {0, 0, 0, 0};
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const int rel = ir * ext32 + e0 + (LDSU ? s_uoff[j] : uoff[j]);
                set_unit<W>(out, g, *(const V *)((const char *)s_tile + lds_at<SWZ>(rel, swz)));
                if (++j == up) { j = 0; ++ir; }
            }
            __builtin_nontemporal_store(out, (pu32x4 *)(dst + 16 * c));
        } else {
            for (long q = c * G; q < qn; ++q) {
                const int rel = ir * ext32 + e0 + (LDSU ? s_uoff[j] : uoff[j]);
                *(V *)(dst + q * W) = *(const V *)((const char *)s_tile + lds_at<SWZ>(rel, swz));
                if (++j == up) { j = 0; ++ir; }
            }
        }
    }
}

// elements per tile (a multiple of 64 / gcd(size, 64): each tile's packed
// bytes start on a 64-byte sector, so no two workgroups write one sector;
// its hull within the tile with the alignment slack), or 0: no tiling
static long pack_ept(const PackCache &pc)
{
    // 8 KiB tiles leave room for 8 resident workgroups per CU; 16 KiB (6 per
    // CU, LDS-bound) and 4 KiB (too little work per tile) ran slower
    // (profiles/r06/pack_tile_sizes.txt, pack_tile_sizes_noflat.txt)
    const long TILE = PACK_TILE, lo = pc.mlo, hi = pc.mhi;
    const PackView &t = pc.t;
    if (t.extent <= 0 || t.extent > (1L << 30) || t.size <= 0 || hi - lo > TILE / 4) return 0;
    const long step = 64 / gcd(t.size, 64);
    // hull of e elements: (e - 1) * ext + (hi - lo), plus up to 30 bytes of
    // word alignment; spans reaching below the element (lo < 0) included
    long e = (TILE - 32 - (hi - lo)) / t.extent + 1;
    e -= e % step;
    return e >= step ? e : 0;
}

template <int W>
static int launch_tiles(const PackCache &pc, int wi, const void *src, void *dst, long count, long ept, hipStream_t st)
{
    const long tiles = (count + ept - 1) / ept;
    if (tiles < 1 || tiles > INT32_MAX) return MPI_ERR_OTHER;
    // the chunk table for W = 2 and 1 only: with 2 or 4 units per chunk it
    // did not pay, profiles/r06/pack_chunk_tab_ab.txt
    const bool tb = knob(PACK_CHUNK_TAB) && W <= 2 && pc.tabP[wi] > 0, lu = pc.units[wi] <= MERGE_UNITS_LDS;
    // the swizzle for 1- and 2-byte units only: G = 16 / W LDS reads per
    // chunk; at W = 4 it cost its address arithmetic and gained nothing
    // (struct {int; hole; double} 74.5-75.1 -> 75.6-75.9 us, whose unpack it
    // takes 114.8 -> 113.9; profiles/r06/lds_swizzle_ab.txt)
    const int sw = knob(LDS_SWIZZLE) && W <= 2 ? pc.swz[wi] : 0;
    with_variant(tb ? OFF_TAB : lu ? OFF_LDS : OFF_GLOBAL, sw != 0, [&](auto from, auto swz) {
        constexpr bool LU = decltype(from)::value == OFF_LDS, TB = decltype(from)::value == OFF_TAB;
        constexpr bool SW = decltype(swz)::value != 0;
        g_last_sym = sym_tile(false, W, PACK_TILE, LU, TB, SW);
        hipLaunchKernelGGL((k_pack_tiles<W, PACK_TILE, LU, TB, SW>), dim3((unsigned)tiles), dim3(256), 0, st,
                           (const char *)src, (char *)dst, (const int *)pc.dunits[wi], pc.units[wi], count,
                           pc.t.extent, pc.mlo, pc.mhi, ept, pc.tabP[wi], sw);
    });
    return hipGetLastError() == hipSuccess ? MPI_SUCCESS : MPI_ERR_OTHER;
}

static int device_map(PackCache &pc)
{
    if (pc.dmap) return MPI_SUCCESS;
    std::vector<DBlk> v;
    long poff = 0;
    for (const Blk *b = pc.t.map; b < pc.t.map + pc.t.nblk; ++b)
        for (long o = 0; o < b->len; o += 64) {
            const long len = b->len - o < 64 ? b->len - o : 64;
            v.push_back({b->off + o, poff, (int)len, 0});
            poff += len;
        }
    if (v.empty()) return MPI_SUCCESS;
    if (hipMalloc(&pc.dmap, v.size() * sizeof(DBlk)) != hipSuccess) { pc.dmap = nullptr; return MPI_ERR_OTHER; }
    if (hipMemcpy(pc.dmap, v.data(), v.size() * sizeof(DBlk), hipMemcpyHostToDevice) != hipSuccess)
        return MPI_ERR_OTHER;
    pc.dmap_n = (long)v.size();
    return MPI_SUCCESS;
}

// Which kernel moves `count` elements of handle h, each rule stated once.
//   basic handles: one block -> hipMemcpyAsync ("memcpy"); the padded pair
//     structs -> MPI_ERR_TYPE (they move whole, mvx_dtype.h dense)
//   derived handles, MVX_PACK_UNITS on: the widths W = 16, 8, 4, then (small
//     elements only, size <= 4096) 2, 1, skipping a width that src or dst is
//     not aligned to or that the map has no unit table for.  The first left:
//       pack, W < 16, tiles on, dst 16-aligned, pack_ept > 0  -> k_pack_tiles
//       unpack, merge on, src 16-aligned, merge_ok            -> k_unpack_merge
//       else W >= 4                                           -> k_pack_units
//       else (W <= 2 serve the tile kernels only) no further width is tried
//   no width decided: the piece kernel k_pack
static int pack(int h, const void *src, void *dst, size_t count, hipStream_t st, bool packing)
{
    PackView t;
    if (!pack_view(h, &t)) return MPI_ERR_TYPE;
    if (!count || !t.size) return MPI_SUCCESS;
    if (!t.cache) {
        // a basic type is its own packed form
        g_last_sym = "memcpy";
        if (t.nblk == 1)
            return hipMemcpyAsync(dst, src, count * (size_t)t.size, hipMemcpyDeviceToDevice, st) == hipSuccess
                   ? MPI_SUCCESS : MPI_ERR_OTHER;
        return MPI_ERR_TYPE;
    }
    if (!*t.cache) {
        *t.cache = new PackCache();
        (*t.cache)->t = t;
        hull(t.map, t.nblk, &(*t.cache)->mlo, &(*t.cache)->mhi);
    }
    PackCache &pc = **t.cache;
    const long n = (long)count;
    const uintptr_t al = (uintptr_t)src | (uintptr_t)dst;
    static const int Ws[5] = {16, 8, 4, 2, 1};
    for (int wi = 0; knob(PACK_UNITS) && wi < 5; ++wi) {
        const int W = Ws[wi];
        if (W <= 2 && t.size > 4096) break;
        if (al % W || !unit_table(pc, W, wi)) continue;
        long ept = 0;
        if (packing && W < 16 && knob(PACK_TILES) && (uintptr_t)dst % 16 == 0) ept = pack_ept(pc);
        const bool tiles = ept > 0;
        const bool merge = !packing && knob(UNPACK_MERGE) && (uintptr_t)src % 16 == 0 && merge_ok(pc);
        if (W <= 2 && !tiles && !merge) break;
        return with_width(W, [&](auto w) {
            constexpr int CW = decltype(w)::value;
            if constexpr (CW < 16)
                if (tiles) return launch_tiles<CW>(pc, wi, src, dst, n, ept, st);
            if (merge) return launch_merge<CW>(pc, wi, src, dst, n, st);
            if constexpr (CW >= 4)
                return packing ? launch_units<true, CW>(pc, wi, src, dst, n, st)
                               : launch_units<false, CW>(pc, wi, src, dst, n, st);
            else
                return (int)MPI_ERR_INTERN;     // not reached: W <= 2 left the loop above
        });
    }
    int rc = device_map(pc);
    if (rc) return rc;
    const long items = n * pc.dmap_n;
    long blocks = (items + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    g_last_sym = packing ? "k_pack<true>" : "k_pack<false>";
    hipLaunchKernelGGL((packing ? k_pack<true> : k_pack<false>), dim3((unsigned)blocks), dim3(256), 0, st,
                       (const char *)src, (char *)dst, (const DBlk *)pc.dmap, pc.dmap_n, n, t.extent, t.size);
    return hipGetLastError() == hipSuccess ? MPI_SUCCESS : MPI_ERR_OTHER;
}

}  // namespace dt
}  // namespace mvx

using namespace mvx::dt;

extern "C" int mvx_type_pack(int type, const void *origin, void *packed, size_t count, void *stream)
{
    return pack(type, origin, packed, count, (hipStream_t)stream, true);
}

extern "C" int mvx_type_unpack(int type, const void *packed, void *origin, size_t count, void *stream)
{
    return pack(type, packed, origin, count, (hipStream_t)stream, false);
}

extern "C" const char *mvx_type_last_kernel_symbol(void) { return g_last_sym; }
