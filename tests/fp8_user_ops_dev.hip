// TEST INFRASTRUCTURE: MVX_Device_functions (include/mvx_coll.h,
// mvx_op_create_device) for tests/test_gpu_fp8_coll.py.  Both take the
// larger of the two bytes as unsigned integers -- commutative and
// associative, so the result does not depend on the combine order -- and
// refuse a datatype handle other than the one the caller must have passed.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace {

// elements of W bytes; the even bytes are the type map (W = 1: a basic
// 1-byte type; W = 5: vector(3, 1, 2, MVX_FLOAT8_E5M2), whose bytes 1 and 3
// are holes the function must leave alone)
__global__ void __launch_bounds__(256) k_bitmax(const uint8_t *in, uint8_t *inout, size_t nbytes, int W)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nbytes; i += (size_t)gridDim.x * 256)
        if (((i % (size_t)W) & 1) == 0 && in[i] > inout[i]) inout[i] = in[i];
}

int launch(const void *in, void *inout, size_t len, int W, void *stream)
{
    if (len == 0) return 0;
    size_t blocks = (len * W + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_bitmax, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const uint8_t *)in, (uint8_t *)inout, len * W, W);
    return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace

// on MVX_FLOAT8_E4M3 (72)
extern "C" int duop_e4m3_bitmax(const void *in, void *inout, size_t len, int dt, void *s)
{
    return dt == 72 ? launch(in, inout, len, 1, s) : 1;
}

// on a derived type of extent 5 (a handle from the constructors: >= 256)
extern "C" int duop_vec3_bytemax(const void *in, void *inout, size_t len, int dt, void *s)
{
    return dt >= 256 ? launch(in, inout, len, 5, s) : 1;
}
