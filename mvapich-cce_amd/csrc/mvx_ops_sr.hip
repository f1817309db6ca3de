// mvx_ops_sr.hip -- kernel table of MVX_SR_SUM, the stochastically rounded
// f32 sum (an extension beyond the reference, include/mvx_hip.h):
// MVX_SUM_ACC32's f32 combine program, its value narrowed to one of its two
// neighbours by random bits that are a counter-based function of the seed and
// of the element's index in the reduced vector (mvx_ops_fn.h: Sr,
// sr_word_bits, sr_code).  Four kernel sets, the narrow floating types, each
// with the f32-leaves form of k_combine_f32 for the last launch of a program
// over more than 8 leaves, and without the KMAX = 4 kernels (mvx_ops_tab.h).
// One translation unit of libmvx_hip.so of its own, like mvx_ops_scaled.hip,
// so the kernel instantiations compile in parallel (mvx_ops_tab.h).
#include "mvx_ops_tab.h"

namespace mvx {

const KSet *lookup_sr(int ek)
{
    switch (ek) {
    HALFS(OSR, "sr")
    FP8S(OSR, "sr")
    default:
        return nullptr;
    }
}

}  // namespace mvx
