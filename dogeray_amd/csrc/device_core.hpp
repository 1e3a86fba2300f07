// Device functions of the path-tracing megakernel (gfx950).
//
// Each function states which reference function it replaces (kernel.cu, K:<line>).  The
// arithmetic (operation order, float/double promotion, comparison direction) follows the
// reference expression by expression, because a one-ulp difference flips hit/miss branches
// and rejection loops; what changes is where operands come from (SoA records, per-ray
// precomputation) and how lanes are scheduled.  Build with -ffp-contract=off: no FMA
// contraction, IEEE division and square root.
//
// This file is the umbrella: the functions live in one header per concern, each including what it needs.
//   device_prims.hpp      the primitives with a GPU and a CPU spelling (the one switch between the device and the host build)
//   device_math.hpp       V3, f2i, DR_MARK
//   device_rng.hpp        XORWOW, the restated uniform draws, the rejection samplers
//   device_intersect.hpp  slab test, triangle, sphere, primitive records, Hit, Ctr
//   device_walk.hpp       the threaded and the ordered walk
//   device_wide.hpp       the wide walk
//   device_cert.hpp       the camera rays' grazing certificate and entry table
//   device_surface.hpp    reflect / refract, texture fetch, surface normal
//   device_shade.hpp      one bounce, one path, the camera ray, the pixel's store
//   device_aov.hpp        the first hit of a pixel's pinhole ray
//   device_aov_lens.hpp   the first hits of a pixel's own camera rays, averaged
// device_coop.hpp (wave-level code of the persistent kernel) is device only and not part of the umbrella: kernels_render.hip includes it itself.
#pragma once
#include "device_prims.hpp"
#include "device_math.hpp"
#include "device_rng.hpp"
#include "device_intersect.hpp"
#include "device_walk.hpp"
#include "device_wide.hpp"
#include "device_cert.hpp"
#include "device_surface.hpp"
#include "device_shade.hpp"
#include "device_aov.hpp"
#include "device_aov_lens.hpp"
