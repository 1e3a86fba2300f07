// The seam between the GPU and the host build of the device functions: every primitive that is an instruction, a builtin or a question to the
// wave on gfx950 and plain C++ on a CPU.  This file holds the device spellings; tools/host_kernel/host_prims.hpp holds the host's, name for name
// (tools/host_kernel.cpp: the same arithmetic compiled for the host -- a CPU baseline and a CPU-side check, never in the product library).  The
// switch below is the only place where the product's headers ask which of the two builds they are in.
#pragma once
#ifdef DR_HOST_BUILD
#include "host_prims.hpp"
#else
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dr {

// ---- RNG
__device__ __forceinline__ double bits_double(uint32_t hi, uint32_t lo) {      // the double with these two words
  // (the high word is a constant: set where it is used -- hoisted out of the kernel's main loop, the two constants of Xorwow::z_plus_half would
  // occupy two registers through every node and leaf step, where there are none to spare)
  asm volatile("v_mov_b32 %0, %1" : "=v"(hi) : "s"(hi));
  const uint64_t b = ((uint64_t)hi << 32) | lo;
  double r; __builtin_memcpy(&r, &b, 8);
  return r;
}
__device__ __forceinline__ uint32_t xorwow_combine(uint32_t t, uint32_t v4) {      // XORWOW's new word: (v4 ^ (v4 << 4)) ^ (t ^ (t << 1))
  // t << 1 as t + t and the three-way xor as ONE v_bitop3_b32: both at the fast class's 2.4 cycles; spelled in plain C++ the compiler turns t + t back
  // into a 4.2-cycle shift and emits three v_xor (7 instead of 8 instructions per output, -0.4 % of the frame: profiles/r4_m_rejection_loop.txt)
  uint32_t t2; asm("v_add_u32 %0, %1, %1" : "=v"(t2) : "v"(t));
  return __builtin_amdgcn_bitop3_b32(t, t2, v4 << 4, 0x96) ^ v4;
}

// ---- the wave
// p in some lane of the wave (wave-uniform).  A macro: through a function the compiler orders the operands of the mask's s_and_b64 differently
#define DR_WAVE_ANY(p) (__builtin_amdgcn_ballot_w64(p) != 0ull)
__device__ __forceinline__ bool first_active_lane() { return __lane_id() == (unsigned)__ffsll((long long)__ballot(1)) - 1u; }
// this lane's bit of a wave mask, as the condition of a branch or a select: the mask goes into exec as it is (s_and_saveexec_b64), no VALU instruction.
// The mask MUST be wave-uniform, and the call sits where all 64 lanes are active (the step at the top level of the persistent kernel's loop).
__device__ __forceinline__ bool lane_bit(unsigned long long wave_mask) { return __builtin_amdgcn_inverse_ballot_w64(wave_mask); }
// the number of set bits of a wave mask as a SCALAR int (s_bcnt1_i32_b64), so that a compare with it is an s_cmp: __popcll(m) >= n compiles to a 64-bit
// compare, which the scalar unit does not have -- a v_cmp_gt_u64 on an SGPR pair
__device__ __forceinline__ int wave_count(unsigned long long wave_mask) { int n; asm("s_bcnt1_i32_b64 %0, %1" : "=s"(n) : "s"(wave_mask) : "scc"); return n; }
// a wave-uniform int that the compiler keeps in a VGPR, back on the scalar unit (v_readfirstlane_b32): what is compared with it is then scalar too
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
#define DR_PIN(s) asm volatile("; " s)      // a comment in the assembly that the compiler moves nothing across (the host: nothing)
// the leaf step of the wide walk may test the primitive before the box, the wave deciding together (device_wide.hpp wide_leaf_compute); the host keeps the reference's order
constexpr bool LEAF_PRIM_FIRST = true;
// What the lean persistent build hands its shade / refill phase about a hit (kernels_render.hip; measured in profiles/hit_inputs_ab.txt;
// the macros serve the variant libraries of tools/exp_variant.sh):
//  HIT_UV_CARRIED: the barycentrics u, v of the accepted triangle hit travel from the leaf step to the phase in two stash words, and the phase
//                  (device_shade.hpp shade_prepare_hit) takes them as given instead of forming them again from the primitive record;
//  HIT_FETCH_LAZY: the phase takes a hit's type from its shade record and loads the primitive record (with HIT_UV_CARRIED) and the texture coordinates
//                  only in a wave where some lane reads them.
#ifndef DR_HIT_UV_CARRIED
#define DR_HIT_UV_CARRIED 1
#endif
#ifndef DR_HIT_FETCH_LAZY
#define DR_HIT_FETCH_LAZY 1
#endif
constexpr bool HIT_UV_CARRIED = DR_HIT_UV_CARRIED != 0;
constexpr bool HIT_FETCH_LAZY = DR_HIT_FETCH_LAZY != 0;

// ---- 128-bit loads through a buffer descriptor (device_walk.hpp ld_unit has the reason)
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t WalkRsrc;
__device__ __forceinline__ WalkRsrc make_rsrc(const void* p, uint32_t bytes) { return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, (int)bytes, 0x00020000); }
__device__ __forceinline__ u32x4 ld_unit_raw(WalkRsrc r, unsigned byte_off) { return __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0); }
// the two halves of device_wide.hpp wide_fetch's pin: a register tuple that holds no value yet and costs no instruction, and loads kept in front of their first use
__device__ __forceinline__ void no_value(u32x4& v) { asm volatile("" : "=v"(v)); }
__device__ __forceinline__ void pin_loads(u32x4& a, u32x4& b, u32x4& c, u32x4& d) { asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); }
// a value the compiler sees as a register and nothing more (no instruction): what is added to it stays an addition -- a load's immediate offset
__device__ __forceinline__ unsigned one_register(unsigned v) { asm("" : "+v"(v)); return v; }

// ---- three-input bit operations (one v_bitop3_b32 each on the device; spelled out, the compiler re-associates them into slower pairs)
__device__ __forceinline__ unsigned bit_select(unsigned if0, unsigned if1, unsigned m) { return __builtin_amdgcn_bitop3_b32(if0, if1, m, 0xd8); }      // m ? if1 : if0, bit by bit
__device__ __forceinline__ unsigned bit_and_or(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xea); }
__device__ __forceinline__ unsigned bit_andn(unsigned a, unsigned b, unsigned c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0x08); }
// the number of the lowest set bit, -1 for 0: v_ffbl_b32 as it is (__builtin_ctz leaves 0 undefined, the defined form costs a v_min_u32 more and gives 32)
__device__ __forceinline__ int lowest_bit(unsigned w) { int j; asm("v_ffbl_b32 %0, %1" : "=v"(j) : "v"(w)); return j; }
// max(v, -1) as ONE v_max_i32: spelled in C++ the compiler makes a compare and a select of it
__device__ __forceinline__ int at_least_minus_one(int v) { int r; asm("v_max_i32 %0, -1, %1" : "=v"(r) : "v"(v)); return r; }

// ---- The four plane bytes of a word as f16 denormals: (byte0, byte2) and (byte1, byte3), each pair in one register
typedef _Float16 DrHalf2 __attribute__((ext_vector_type(2)));
struct PlanePairs { DrHalf2 even, odd; };
__device__ __forceinline__ PlanePairs plane_pairs(unsigned w) {
  PlanePairs p;
  p.even = __builtin_bit_cast(DrHalf2, w & 0x00ff00ffu);
  p.odd = __builtin_bit_cast(DrHalf2, __builtin_amdgcn_perm(0u, w, 0x0c030c01u));      // bytes {1, zero, 3, zero} of w: one v_perm_b32
  return p;
}
__device__ __forceinline__ float plane_t(const PlanePairs& p, int k, float a, float b) {     // v_fma_mix_f32: the f16 operand is widened inside the instruction
  const _Float16 h = (k & 1) ? ((k & 2) ? p.odd.y : p.odd.x) : ((k & 2) ? p.even.y : p.even.x);
  return __builtin_fmaf((float)h, a, b);
}

// ---- the camera rays' entry table (device_cert.hpp)
__device__ __forceinline__ void entry_min(uint32_t* p, uint32_t v) {
  // read first: leaves arrive in spatial order and some hundreds of them touch a tile, nearly all of them inside what the tile has already
  if (v < *p) atomicMin(p, v);
}
#define ENTRY_MUTANT(k) false      // (a wrong rule on purpose: the host build's test hook)

}  // namespace dr
#endif
