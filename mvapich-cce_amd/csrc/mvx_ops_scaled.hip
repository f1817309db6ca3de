// mvx_ops_scaled.hip -- kernel table of MVX_SCALED_SUM, the per-rank scaled
// sum with a fused amax (an extension beyond the reference, include/mvx_hip.h):
// MVX_SUM_ACC32's f32 combine program over leaves that are multiplied by
// their ranks' scales as they are widened, its value multiplied once by an
// output scale, its largest magnitude taken before the single narrowing
// (mvx_ops_fn.h: Scl, scl_chunk, amax_commit).  Five kernel sets: the four
// narrow floating types, with both f32-side forms of k_combine_f32 for
// programs over more than 8 leaves, and float, whose chunks go through the
// same f32 program one word an element.  One translation unit of
// libmvx_hip.so of its own, like mvx_ops_avg.hip, so the kernel
// instantiations compile in parallel (mvx_ops_tab.h).
#include "mvx_ops_tab.h"

namespace mvx {

const KSet *lookup_scaled(int ek)
{
    switch (ek) {
    case EK_F32: { static KSet s = kset<OSCL, float>("scaled_f32"); return &s; }
    HALFS(OSCL, "scaled")
    FP8S(OSCL, "scaled")
    default:
        return nullptr;
    }
}

}  // namespace mvx
