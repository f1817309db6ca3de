// mvx_ops_half.hip -- kernel table of the 16-bit floating types MVX_FLOAT16
// and MVX_BFLOAT16 (an extension beyond the reference, include/mvx_mpi.h):
// the seven ops MPI_FLOAT has.  One translation unit of libmvx_hip.so of its
// own -- 14 kernel sets, fewer than any of the other tables hold -- so the
// kernel instantiations compile in parallel (mvx_ops_tab.h).
#include "mvx_ops_tab.h"

namespace mvx {

const KSet *lookup_half(int op, int ek)
{
    switch (op) {
    case MPI_MAX: switch (ek) { HALFS(OMAX, "max") default: return nullptr; }
    case MPI_MIN: switch (ek) { HALFS(OMIN, "min") default: return nullptr; }
    case MPI_SUM: switch (ek) { HALFS(OSUM, "sum") default: return nullptr; }
    case MPI_PROD: switch (ek) { HALFS(OPROD, "prod") default: return nullptr; }
    case MPI_LAND: switch (ek) { HALFS(OLAND, "land") default: return nullptr; }
    case MPI_LOR: switch (ek) { HALFS(OLOR, "lor") default: return nullptr; }
    case MPI_LXOR: switch (ek) { HALFS(OLXOR, "lxor") default: return nullptr; }
    default:
        return nullptr;     // B* ops, MAXLOC, MINLOC: 329, as on MPI_FLOAT
    }
}

}  // namespace mvx
