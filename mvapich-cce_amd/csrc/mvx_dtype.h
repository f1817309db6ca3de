// mvx_dtype.h -- internal interfaces of the datatype engine (mvx_dtype.hip,
// host code only) inside libmvx_hip.so: to the op kernels (mvx_ops.hip) and
// to the device pack / unpack path (mvx_pack.hip).  The C-ABI is in
// include/mvx_hip.h.
#ifndef MVX_DTYPE_INTERNAL_H
#define MVX_DTYPE_INTERNAL_H

namespace mvx {
namespace dt {

// the reference's dte_type of a handle (mpid/ch2/datatype.h): vector and
// indexed constructors produce HVECTOR / HINDEXED (type_vec.c:101-107,
// type_ind.c:119-129)
enum Kind { K_BASIC = 0, K_CONTIG, K_HVECTOR, K_HINDEXED, K_STRUCT, K_UB, K_LB };

struct Info {
    int kind;
    int old;        // CONTIG: old type after flattening; HVECTOR / HINDEXED:
                    // the old type; STRUCT: old_types[0]; BASIC: itself
    int count;      // CONTIG: replication count
    int is_contig;  // the reference's is_contig
    int dense;      // 1: elements are `extent` bytes from the origin, moved
                    // whole (basic types, contiguous types of them); 0: the
                    // type map has holes -- moved packed (mvx_type_pack)
    long extent, size, lb, ub;
    long span_lo, span_hi;   // lowest / one past highest type-map byte of one element
};

// basic or derived handle; false for an unknown handle
bool info(int handle, Info *out);

// ---- to the pack / unpack path (mvx_pack.hip) -----------------------------
struct Blk { long off, len; };      // one block of a type map
struct PackCache;                   // a derived type's device side, defined in mvx_pack.hip

struct PackView {
    long extent, size, nblk;    // nblk: blocks of one element's map, in order, merged
    const Blk *map;             // derived handles: the blocks, valid while the type lives
    PackCache **cache;          // derived handles: where the type keeps its cache (null
                                // until its first pack or unpack); basic handles: null
};
#pragma GCC visibility push(hidden)     // libmvx_hip.so exports none of these
// basic or derived handle; false for an unknown handle
bool pack_view(int handle, PackView *out);
// the hull of a map: its lowest byte and one past its highest (0, 0 if empty)
void hull(const Blk *map, long nblk, long *lo, long *hi);
// mvx_pack.hip: frees a cache, device memory included, when its type is freed
// (the type engine's one touch of the device)
void pack_cache_free(PackCache *c);
#pragma GCC visibility pop

}  // namespace dt
}  // namespace mvx

#endif
