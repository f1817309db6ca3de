// mvx_ops_avg.hip -- kernel table of MVX_AVG, the ranks' mean (an extension
// beyond the reference, include/mvx_mpi.h): MPI_SUM's combine program with its
// value divided once, before the single store, by the number of rank
// contributions the program consumed (mvx_ops_fn.h: avg_fin).  Six kernel
// sets: float and double run MPI_SUM's per-step program and divide in their
// own format; the four narrow floating types run the f32 program of
// MVX_SUM_ACC32, divide in binary32 and narrow once, and have the f32-leaves
// form of k_combine_f32 for the last launch of a program over more than 8
// leaves.  One translation unit of libmvx_hip.so of its own, like
// mvx_ops_acc32.hip, so the kernel instantiations compile in parallel
// (mvx_ops_tab.h).
#include "mvx_ops_tab.h"

namespace mvx {

const KSet *lookup_avg(int ek)
{
    switch (ek) {
    FLOATS(OAVG, "avg")
    HALFS(OAVG, "avg")
    FP8S(OAVG, "avg")
    default:
        return nullptr;
    }
}

}  // namespace mvx
