// mvx_ops_fp8.hip -- kernel table of the 8-bit OCP floating types
// MVX_FLOAT8_E4M3 and MVX_FLOAT8_E5M2 (an extension beyond the reference,
// include/mvx_mpi.h): the seven ops MPI_FLOAT has.  One translation unit of
// libmvx_hip.so of its own, 14 kernel sets like mvx_ops_half.hip, so the
// kernel instantiations compile in parallel (mvx_ops_tab.h).
#include "mvx_ops_tab.h"

namespace mvx {

const KSet *lookup_fp8(int op, int ek)
{
    switch (op) {
    case MPI_MAX: switch (ek) { FP8S(OMAX, "max") default: return nullptr; }
    case MPI_MIN: switch (ek) { FP8S(OMIN, "min") default: return nullptr; }
    case MPI_SUM: switch (ek) { FP8S(OSUM, "sum") default: return nullptr; }
    case MPI_PROD: switch (ek) { FP8S(OPROD, "prod") default: return nullptr; }
    case MPI_LAND: switch (ek) { FP8S(OLAND, "land") default: return nullptr; }
    case MPI_LOR: switch (ek) { FP8S(OLOR, "lor") default: return nullptr; }
    case MPI_LXOR: switch (ek) { FP8S(OLXOR, "lxor") default: return nullptr; }
    default:
        return nullptr;     // B* ops, MAXLOC, MINLOC: 329, as on MPI_FLOAT
    }
}

}  // namespace mvx
