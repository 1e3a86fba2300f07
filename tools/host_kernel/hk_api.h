/* The entries of tools/libhostkernel.so that the stand-alone sanitizer drivers (the tools/..._sanitize_driver.cpp files) call, as plain C prototypes.  host_kernel.cpp
   includes this file too, so a definition that drifts from its prototype here no longer compiles.  What each entry does stands at its definition. */
#ifndef HK_API_H
#define HK_API_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

void* hk_scene_load(const char* rts_path, const char* texdir);
void hk_scene_free(void* hv);
const char* hk_last_error(void);

int hk_trace(void* hv, int traversal, int tree, int mode, long long n, const float* o, const float* d, const float* tmax, float* t, int32_t* idx,
             int32_t* occluded, int32_t* slot, int32_t* visits);
int hk_ray_surface(void* hv, int tree, long long n, const float* o, const float* d, const float* t, const int32_t* slot, int32_t* material, float* distance,
                   float* normal, float* uv, float* albedo);
int hk_radiance(void* hv, int traversal, int tree, long long n, const float* o, const float* d, const uint64_t* seed, const int32_t* skip, int spp,
                int max_depth, float background, int backtex, uint64_t base_seed, float* radiance, int32_t* bounces);
int hk_nearest(void* hv, int walk, int tree, long long n, const float* p, const float* rmax, float* distance, float* d2, int32_t* object, int32_t* material,
               float* point, float* uv, int32_t* visits, int nthreads);
int hk_nearest_brute(void* hv, long long n, const float* p, const float* rmax, float* distance, float* d2, int32_t* object, int32_t* material, float* point,
                     float* uv, int nthreads);
int hk_allhits_max(void);
int hk_allhits(void* hv, int walk, int tree, long long n, const float* o, const float* d, const float* tmax, int max_hits, int kind_mask, int zero_margin,
               int32_t* count, float* t, int32_t* object, int32_t* material, float* distance, float* normal, float* uv, float* albedo, int32_t* visits, int nthreads);
int hk_allhits_brute(void* hv, long long n, const float* o, const float* d, const float* tmax, int max_hits, int kind_mask, int32_t* count, float* t, int32_t* object,
                     int nthreads);

int hk_kat_sample(long long n, const uint64_t* seed, const int32_t* warm, const int32_t* kind, float* point_plain, uint32_t* next_plain, float* point_merged,
                  uint32_t* next_merged);
int hk_kat_outside(long long n, const float* d2, int32_t* out);
int hk_kat_tex(void* hv, long long n, const int32_t* tex, const float* u, const float* v, uint32_t* rgba);
int hk_kat_bounce(void* hv, long long n, const int32_t* object_index, const float* o, const float* d, const float* t, const float* atten, const uint64_t* seed,
                  const int32_t* warm, int32_t* alive, float* o_out, float* d_out, float* atten_out, uint32_t* next);
int hk_kat_miss(void* hv, long long n, const float* d, const float* atten, int backtex, float background, float* rgb);
int hk_kat_camera(const float* settings13, int W, int H, uint64_t frame_seed, uint32_t seed_stride, long long n, const int32_t* x, const int32_t* y,
                  const int32_t* sample, float* origin, float* dir, uint32_t* next);
int hk_kat_store(long long n, const float* color, int spp, int32_t* out);

#ifdef __cplusplus
}
#endif
#endif
