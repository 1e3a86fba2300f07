// The AOV-guided upsampler (dr_accum_upscale): one kernel, one thread per pixel of the W x H output.  The kernel is the thread-to-pixel mapping
// and a call of up_pixel (device_upscale.hpp), which holds the pixel's arithmetic and indexing and runs unchanged in the host build.  A low tap
// is shared by the 4 div^2 threads around it: neighbouring lanes of a wave, served by the vector L1.
#include <hip/hip_runtime.h>

#include "device_upscale.hpp"
#include "kernels.hpp"

namespace dr {

namespace {

// consecutive threads walk a row of the output (coalesced writes, coalesced reads of the full guides)
__global__ __launch_bounds__(256) void up_kernel(UpLaunch L) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)L.W * L.H) return;
  const int Y = (int)(idx / L.W), X = (int)(idx - (long long)Y * L.W);
  up_pixel(L, X, Y, nullptr);
}

}  // namespace

void launch_upscale(hipStream_t stream, const UpLaunch& L) {
  const long long n = (long long)L.W * L.H;
  if (n <= 0) return;
  hipLaunchKernelGGL(up_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, L);
}

}  // namespace dr
