// Point location in the triangles of one mesh scale, shared by raster.hip (pixel centres of a
// regular grid) and meshgraph.hip (arbitrary points): the bucket grid, bucket_of, the edge function,
// the walk of one point through its bucket and the host build of the face records and the bucket
// CSR (semantics: include/mswegnn.h, "Raster products").
//
// Host: one 64-byte record per face (the three vertices, the canonical-order flag of each edge,
// the sign of area2, face_row) and a uniform bucket grid over the mesh, a CSR of face indices per
// bucket, ascending within a bucket -- the first hit of a lane's walk is the lowest face index, so
// the lane stops there.  A face is listed in every bucket that its bounding box, widened by a
// rounding margin (face_margin), touches; bucket_of is one monotone function of a coordinate used
// for the faces' ends on the host and for the points on the device, so a point between a face's
// ends lands in a bucket between theirs whatever the rounding.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/mswegnn.h"
#include "engine.h"
#include "raster_handle.h"

// Every operation rounds on its own, as written (host and device): the edge functions, area2 and
// bucket_of are restated operation for operation by the tests.
#pragma clang fp contract(off)

namespace msw_raster_detail {

constexpr int64_t kMaxFaces = (int64_t)1 << 26;
constexpr int kMaxBucketsPerAxis = 8192;

// The bucket grid: [gx0, gx1] x [gy0, gy1] cut into nbx x nby buckets.
struct Buckets {
  double gx0, gx1, gy0, gy1, invx, invy;
  int nbx, nby;
};

// Monotone non-decreasing in v (a subtraction, a multiplication by a non-negative constant, floor
// and a clamp are each monotone under rounding), the same operations on the host and the device.
__host__ __device__ __forceinline__ int bucket_of(double v, double g0, double inv, int nb) {
  const double t = floor((v - g0) * inv);
  return t >= (double)(nb - 1) ? nb - 1 : (t > 0.0 ? (int)t : 0);
}

// E(u -> v) at (px, py); neg: u is not the lower vertex index, so the edge is taken from v.
__host__ __device__ __forceinline__ double edge_fn(double ux, double uy, double vx, double vy, bool neg, double px,
                                                   double py) {
  const double p_x = neg ? vx : ux, p_y = neg ? vy : uy, q_x = neg ? ux : vx, q_y = neg ? uy : vy;
  const double e = (q_x - p_x) * (py - p_y) - (q_y - p_y) * (px - p_x);
  return neg ? -e : e;
}

// face_row of the lowest face that contains (px, py), or -1: the bucket of the point, its faces
// ascending, stopping at the first hit.  A point outside the bucket grid (a NaN or an infinite
// coordinate is outside: every comparison fails) gets -1 without touching memory.
__device__ __forceinline__ int locate_walk(const FaceRec* rec, const int32_t* bptr, const int32_t* bface,
                                           const Buckets& b, double px, double py) {
  int row = -1;
  if (px >= b.gx0 && px <= b.gx1 && py >= b.gy0 && py <= b.gy1) {
    const int bk = bucket_of(py, b.gy0, b.invy, b.nby) * b.nbx + bucket_of(px, b.gx0, b.invx, b.nbx);
    int k = bptr[bk];
    const int kend = bptr[bk + 1];
    while (k < kend) {
      const FaceRec r = rec[bface[k++]];
      const double e0 = edge_fn(r.ax, r.ay, r.bx, r.by, r.flags & kNegAB, px, py);
      const double e1 = edge_fn(r.bx, r.by, r.cx, r.cy, r.flags & kNegBC, px, py);
      const double e2 = edge_fn(r.cx, r.cy, r.ax, r.ay, r.flags & kNegCA, px, py);
      const bool in = (r.flags & kAreaPos) ? (e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0)
                                           : (e0 <= 0.0 && e1 <= 0.0 && e2 <= 0.0);
      if (in) {
        row = r.row;
        break;
      }
    }
  }
  return row;
}

// The checks on the host geometry that come before build_host.
inline int check_geometry(const double* node_xy, int64_t num_nodes, const int32_t* face_nodes,
                          const int32_t* face_row, int64_t num_faces) {
  for (int64_t v = 0; v < 2 * num_nodes; ++v)
    if (!std::isfinite(node_xy[v])) return msw::set_error(MSW_ERR_INVALID, "node coordinate not finite");
  for (int64_t k = 0; k < 3 * num_faces; ++k)
    if (face_nodes[k] < 0 || face_nodes[k] >= num_nodes)
      return msw::set_error(MSW_ERR_INVALID, "vertex index outside [0, num_nodes)");
  if (face_row)
    for (int64_t f = 0; f < num_faces; ++f)
      if (face_row[f] < -1) return msw::set_error(MSW_ERR_INVALID, "face_row below -1");
  return MSW_OK;
}

// The host side of a locator after its checks: the face records and the bucket CSR.
struct HostBuild {
  std::vector<FaceRec> rec;
  std::vector<int32_t> bptr, bface;
  Buckets b{};
  int64_t longest = 0;
  int32_t min_row = 0, max_row = -1;  // over face_row >= 0 (max_row -1: no face has a value)
};

inline int build_host(const double* node_xy, const int32_t* face_nodes, const int32_t* face_row, int64_t num_faces,
                      HostBuild& hb) {
  // ---- the face records, each listed face's widened bounding box, the bucket grid's extent
  const double inf = std::numeric_limits<double>::infinity();
  std::vector<FaceRec>& rec = hb.rec;
  rec.resize((size_t)num_faces);
  std::vector<double> box((size_t)num_faces * 4);  // xlo, xhi, ylo, yhi; listed faces only
  std::vector<char> listed((size_t)num_faces, 0);
  Buckets& b = hb.b;
  b = Buckets{inf, -inf, inf, -inf, 0.0, 0.0, 1, 1};
  int32_t min_row = INT32_MAX, max_row = -1;
  double sum_w = 0.0, sum_h = 0.0;
  int64_t nlisted = 0;
  for (int64_t f = 0; f < num_faces; ++f) {
    const int32_t ia = face_nodes[3 * f], ib = face_nodes[3 * f + 1], ic = face_nodes[3 * f + 2];
    FaceRec& r = rec[(size_t)f];
    r.ax = node_xy[2 * (int64_t)ia], r.ay = node_xy[2 * (int64_t)ia + 1];
    r.bx = node_xy[2 * (int64_t)ib], r.by = node_xy[2 * (int64_t)ib + 1];
    r.cx = node_xy[2 * (int64_t)ic], r.cy = node_xy[2 * (int64_t)ic + 1];
    r.pad = 0.0;
    r.row = face_row ? face_row[f] : (int32_t)f;
    if (r.row >= 0) min_row = std::min(min_row, r.row), max_row = std::max(max_row, r.row);
    const double area2 = (r.bx - r.ax) * (r.cy - r.ay) - (r.by - r.ay) * (r.cx - r.ax);
    r.flags = (ia > ib ? kNegAB : 0) | (ib > ic ? kNegBC : 0) | (ic > ia ? kNegCA : 0) | (area2 > 0.0 ? kAreaPos : 0);
    if (!(area2 > 0.0) && !(area2 < 0.0)) continue;  // contains nothing: in no bucket
    const double xlo = std::min({r.ax, r.bx, r.cx}), xhi = std::max({r.ax, r.bx, r.cx});
    const double ylo = std::min({r.ay, r.by, r.cy}), yhi = std::max({r.ay, r.by, r.cy});
    const double m = face_margin(std::max(xhi - xlo, yhi - ylo), area2);
    double* bx = &box[(size_t)f * 4];
    bx[0] = xlo - m, bx[1] = xhi + m, bx[2] = ylo - m, bx[3] = yhi + m;
    if (!std::isfinite(bx[0]) || !std::isfinite(bx[1]) || !std::isfinite(bx[2]) || !std::isfinite(bx[3]))
      return msw::set_error(MSW_ERR_INVALID, "face extent not finite");
    listed[(size_t)f] = 1;
    ++nlisted;
    sum_w += xhi - xlo, sum_h += yhi - ylo;
    b.gx0 = std::min(b.gx0, bx[0]), b.gx1 = std::max(b.gx1, bx[1]);
    b.gy0 = std::min(b.gy0, bx[2]), b.gy1 = std::max(b.gy1, bx[3]);
  }
  // ---- bucket size: the mean bounding box of a face, doubled until the lists fit their budget
  std::vector<int32_t>& bptr = hb.bptr;
  std::vector<int32_t>& bface = hb.bface;
  int64_t& longest = hb.longest;
  if (nlisted) {
    auto count_of = [](double extent, double cell) {
      const double n = cell > 0.0 ? std::ceil(extent / cell) : 1.0;
      return (int)std::min<double>(std::max(n, 1.0), (double)kMaxBucketsPerAxis);
    };
    b.nbx = count_of(b.gx1 - b.gx0, sum_w / (double)nlisted);
    b.nby = count_of(b.gy1 - b.gy0, sum_h / (double)nlisted);
    const int64_t entry_budget = 16 * nlisted + 4096, bucket_budget = 4 * nlisted + 4096;
    for (;;) {
      b.invx = b.gx1 > b.gx0 ? (double)b.nbx / (b.gx1 - b.gx0) : 0.0;
      b.invy = b.gy1 > b.gy0 ? (double)b.nby / (b.gy1 - b.gy0) : 0.0;
      if (!std::isfinite(b.invx) || !std::isfinite(b.invy)) b.invx = b.invy = 0.0, b.nbx = b.nby = 1;
      int64_t entries = 0;
      for (int64_t f = 0; f < num_faces; ++f) {
        if (!listed[(size_t)f]) continue;
        const double* bx = &box[(size_t)f * 4];
        entries += (int64_t)(bucket_of(bx[1], b.gx0, b.invx, b.nbx) - bucket_of(bx[0], b.gx0, b.invx, b.nbx) + 1) *
                   (bucket_of(bx[3], b.gy0, b.invy, b.nby) - bucket_of(bx[2], b.gy0, b.invy, b.nby) + 1);
      }
      if ((entries <= entry_budget && (int64_t)b.nbx * b.nby <= bucket_budget) || (b.nbx == 1 && b.nby == 1)) break;
      b.nbx = (b.nbx + 1) / 2, b.nby = (b.nby + 1) / 2;
    }
    const int64_t nb = (int64_t)b.nbx * b.nby;
    bptr.assign((size_t)nb + 1, 0);
    auto walk = [&](auto&& visit) {  // faces in ascending order: every bucket's list comes out ascending
      for (int64_t f = 0; f < num_faces; ++f) {
        if (!listed[(size_t)f]) continue;
        const double* bx = &box[(size_t)f * 4];
        const int ix0 = bucket_of(bx[0], b.gx0, b.invx, b.nbx), ix1 = bucket_of(bx[1], b.gx0, b.invx, b.nbx);
        const int iy0 = bucket_of(bx[2], b.gy0, b.invy, b.nby), iy1 = bucket_of(bx[3], b.gy0, b.invy, b.nby);
        for (int iy = iy0; iy <= iy1; ++iy)
          for (int ix = ix0; ix <= ix1; ++ix) visit((int64_t)iy * b.nbx + ix, (int32_t)f);
      }
    };
    walk([&](int64_t k, int32_t) { ++bptr[(size_t)k + 1]; });
    for (int64_t k = 0; k < nb; ++k) {
      longest = std::max<int64_t>(longest, bptr[(size_t)k + 1]);
      bptr[(size_t)k + 1] += bptr[(size_t)k];
    }
    bface.resize((size_t)bptr[(size_t)nb]);
    std::vector<int32_t> fill(bptr.begin(), bptr.end() - 1);
    walk([&](int64_t k, int32_t f) { bface[(size_t)fill[(size_t)k]++] = f; });
  } else {
    bptr.assign(2, 0);  // gx0 > gx1: every point is outside
  }
  hb.min_row = max_row >= 0 ? min_row : 0;
  hb.max_row = max_row;
  return MSW_OK;
}

}  // namespace msw_raster_detail
