// What raster.hip and zonal.hip share: the face record, the rounding margin of a face's bounding
// box and the raster handle itself (opaque in include/mswegnn.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/mswegnn.h"

namespace msw_raster_detail {

constexpr int kNegAB = 1, kNegBC = 2, kNegCA = 4;  // FaceRec::flags: the edge's first vertex is not the lower one
constexpr int kAreaPos = 16;                       // area2 > 0 (listed faces have area2 != 0)

struct alignas(64) FaceRec {
  double ax, ay, bx, by, cx, cy;
  int32_t flags;
  int32_t row;
  double pad;
};
static_assert(sizeof(FaceRec) == 64, "one 64-byte record per face");

// How far outside a face's bounding box a pixel that the fp64 predicates accept can lie.  An edge
// function is L * (distance to the edge's line) with a rounding error below 8 eps L D (D the
// larger side of the bounding box, L <= sqrt(2) D an edge, eps = 2^-53: the differences are taken
// first, so the error scales with the face, not with the size of the coordinates); three lines
// each off by 8 eps D move a corner of angle theta by that over sin(theta / 2) <= 2 D / h, h =
// |area2| / L the smallest altitude: below 2^-47 D^3 / |area2|.  2^-40 leaves a factor of 100.
// Capped at D: a face thinner than 2^-40 of its length is listed as if it were twice as large.
__host__ __device__ inline double face_margin(double D, double area2) {
  const double m = 0x1p-40 * D * (D * D / fabs(area2));
  return m <= D ? m : D;  // also a NaN or infinite m
}

}  // namespace msw_raster_detail

struct msw_raster {
  int device = -1;
  msw_raster_grid g{};
  int64_t num_faces = 0;
  int32_t min_row = 0, max_row = -1;  // over face_row >= 0 (max_row -1: no face has a value)
  msw_raster_detail::FaceRec* d_rec = nullptr;
  int32_t* d_bptr = nullptr;
  int32_t* d_bface = nullptr;
  int32_t* d_prow = nullptr;
  msw_raster_stats stats{};
};
