// mvx_ops_acc32.hip -- kernel table of the f32-accumulating ops MVX_SUM_ACC32
// and MVX_PROD_ACC32 (an extension beyond the reference, include/mvx_mpi.h)
// on the four narrow floating types: 8 kernel sets, each with the families
// kset builds and the two one-side-f32 programs of k_combine_f32.  One
// translation unit of libmvx_hip.so of its own, like mvx_ops_half.hip and
// mvx_ops_fp8.hip, so the kernel instantiations compile in parallel
// (mvx_ops_tab.h).
#include "mvx_ops_tab.h"

namespace mvx {

#define ACC32S(O, NAME)                                                      \
    case EK_F16:    { static KSet s = kset<O, f16>(NAME "_f16"); return &s; } \
    case EK_BF16:   { static KSet s = kset<O, bf16>(NAME "_bf16"); return &s; } \
    case EK_F8E4M3: { static KSet s = kset<O, f8e4m3>(NAME "_f8e4m3"); return &s; } \
    case EK_F8E5M2: { static KSet s = kset<O, f8e5m2>(NAME "_f8e5m2"); return &s; }

const KSet *lookup_acc32(int op, int ek)
{
    switch (op) {
    case MVX_SUM_ACC32: switch (ek) { ACC32S(OSUMA, "sum_acc32") default: return nullptr; }
    case MVX_PROD_ACC32: switch (ek) { ACC32S(OPRODA, "prod_acc32") default: return nullptr; }
    default:
        return nullptr;
    }
}

}  // namespace mvx
