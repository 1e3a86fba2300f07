// The known-answer kernels of the shading step (dr_kat_sample .. dr_kat_store): one element per lane, the bodies in device_kat_shade.hpp.
#include <hip/hip_runtime.h>

#include "device_kat_shade.hpp"
#include "kernels.hpp"

namespace dr {

__global__ __launch_bounds__(256) void kat_sample_kernel(int n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* p_plain,
                                                         uint32_t* n_plain, float* p_merged, uint32_t* n_merged) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_sample_lane(i, seed, warm, kind, p_plain, n_plain, p_merged, n_merged);
}
__global__ __launch_bounds__(256) void kat_outside_kernel(int n, const float* d2, int32_t* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_outside_lane(i, d2, out);
}
__global__ __launch_bounds__(256) void kat_tex_kernel(RenderParams P, int n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_tex_lane(P, i, tex, u, v, rgba);
}
__global__ __launch_bounds__(256) void kat_bounce_kernel(RenderParams P, int n, const int32_t* slot, const float* o, const float* d, const float* t,
                                                         const float* atten, const uint64_t* seed, const int32_t* warm, int32_t* alive2, float* o2,
                                                         float* d2, float* atten2, uint32_t* next2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_bounce_lane(P, i, slot, o, d, t, atten, seed, warm, alive2, o2, d2, atten2, next2, n);
}
__global__ __launch_bounds__(256) void kat_miss_kernel(RenderParams P, int n, const float* d, const float* atten, float* rgb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_miss_lane(P, i, d, atten, rgb);
}
__global__ __launch_bounds__(256) void kat_camera_kernel(RenderParams P, int n, const int32_t* x, const int32_t* y, const int32_t* s, float* origin2,
                                                         float* dir2, uint32_t* next2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_camera_lane(P, i, x, y, s, origin2, dir2, next2, n);
}
__global__ __launch_bounds__(256) void kat_store_kernel(RenderParams P, int n, const float* color) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  kat_store_lane(P, i, color);
}

static dim3 kat_grid(int n) { return dim3((unsigned)((n + 255) / 256)); }

void launch_kat_sample(hipStream_t stream, int n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* p_plain, uint32_t* n_plain,
                       float* p_merged, uint32_t* n_merged) {
  hipLaunchKernelGGL(kat_sample_kernel, kat_grid(n), dim3(256), 0, stream, n, seed, warm, kind, p_plain, n_plain, p_merged, n_merged);
}
void launch_kat_outside(hipStream_t stream, int n, const float* d2, int32_t* out) {
  hipLaunchKernelGGL(kat_outside_kernel, kat_grid(n), dim3(256), 0, stream, n, d2, out);
}
void launch_kat_tex(hipStream_t stream, const RenderParams& P, int n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba) {
  hipLaunchKernelGGL(kat_tex_kernel, kat_grid(n), dim3(256), 0, stream, P, n, tex, u, v, rgba);
}
void launch_kat_bounce(hipStream_t stream, const RenderParams& P, int n, const int32_t* slot, const float* o, const float* d, const float* t,
                       const float* atten, const uint64_t* seed, const int32_t* warm, int32_t* alive2, float* o2, float* d2, float* atten2,
                       uint32_t* next2) {
  hipLaunchKernelGGL(kat_bounce_kernel, kat_grid(n), dim3(256), 0, stream, P, n, slot, o, d, t, atten, seed, warm, alive2, o2, d2, atten2, next2);
}
void launch_kat_miss(hipStream_t stream, const RenderParams& P, int n, const float* d, const float* atten, float* rgb) {
  hipLaunchKernelGGL(kat_miss_kernel, kat_grid(n), dim3(256), 0, stream, P, n, d, atten, rgb);
}
void launch_kat_camera(hipStream_t stream, const RenderParams& P, int n, const int32_t* x, const int32_t* y, const int32_t* s, float* origin2,
                       float* dir2, uint32_t* next2) {
  hipLaunchKernelGGL(kat_camera_kernel, kat_grid(n), dim3(256), 0, stream, P, n, x, y, s, origin2, dir2, next2);
}
void launch_kat_store(hipStream_t stream, const RenderParams& P, int n, const float* color) {
  hipLaunchKernelGGL(kat_store_kernel, kat_grid(n), dim3(256), 0, stream, P, n, color);
}

}  // namespace dr
