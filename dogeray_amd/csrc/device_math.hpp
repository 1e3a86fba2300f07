// Vectors of three floats and the float -> int conversion of the device functions (device_core.hpp has the arithmetic contract).
#pragma once
#include "device_prims.hpp"

// tools/instr_budget.py builds the render kernels with -DDR_ISA_MARKS=1 -save-temps and counts the instructions between these comments
#ifndef DR_ISA_MARKS
#define DR_ISA_MARKS 0
#endif
#if DR_ISA_MARKS
#define DR_MARK(s) asm volatile("; DRMARK " s)
#else
#define DR_MARK(s) do {} while (0)
#endif

namespace dr {

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 mk(float a, float b, float c) { V3 r; r.x = a; r.y = b; r.z = c; return r; }
__device__ __forceinline__ V3 splat(float a) { return mk(a, a, a); }
__device__ __forceinline__ V3 ld3(const float* p) { return mk(p[0], p[1], p[2]); }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ V3 operator/(V3 a, V3 b) { return mk(a.x / b.x, a.y / b.y, a.z / b.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}
__device__ __forceinline__ float length(V3 a) { return __builtin_sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 normalized(V3 v) {              // getNormalizedVec K:179
  float inv = 1.0f / __builtin_sqrtf(dot(v, v));
  return mk(v.x * inv, v.y * inv, v.z * inv);
}

// float -> int as CUDA's cvt.rzi.s32.f32: saturating, NaN -> 0 (K:802,1083-1085)
__device__ __forceinline__ int f2i(float f) {
  if (f != f) return 0;
  if (f >= 2147483648.0f) return 2147483647;
  if (f <= -2147483648.0f) return (-2147483647 - 1);
  return (int)f;
}

}  // namespace dr
