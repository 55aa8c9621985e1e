// Mesh graphs: arbitrary points located in the triangles of one mesh scale, and the dual graph of
// one scale from its coordinates and vertex lists alone (semantics: include/mswegnn.h, "Mesh
// graphs").  mswegnn/meshgraph.py assembles both into a multiscale Graph in the reference's layout.
//
// Locator.  The host build of the rasters (locate_common.h: one 64-byte record per face, a bucket
// grid with ascending lists) without a grid of pixels.
// k_locate_points.  Lane = point, a round = 64 consecutive points, grid-stride over the rounds; the
// walk of k_raster_locate (locate_walk).  Points in mesh order share buckets and face records
// through the cache, shuffled points do not.  No LDS, no atomics.
//
// Dual graph.  Host: the checks that need one face at a time, and a vertex -> incident-face CSR by
// a counting pass over the faces in ascending order.
// k_mesh_faces.  Lane = face: centroid, area, and for each of its three edges the other face that
// holds both vertices, found by walking the star of the edge's lower vertex (a handful of 12-byte
// vertex lists); the lane writes its number of neighbours, or a negative code where the mesh is not
// a manifold.  The host checks the codes and takes the prefix sum: a face's dual edges and its
// boundary slots each start where the lower faces' end.
// k_mesh_edges.  Lane = face: its neighbours in ascending order become its columns, so the rows
// ascend and each row's columns ascend; the lengths from the centroids; its boundary slots.
// No LDS, no atomics: every output element has one writer that is a function of the mesh alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/mswegnn.h"
#include "engine.h"
#include "locate_common.h"

// Every operation rounds on its own, as written: the centroids, the areas and the lengths are
// restated operation for operation by the tests (mswegnn.mesh computes them in the same order).
#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kGridCap = 4096;  // workgroups: 16 per CU (4 waves per SIMD), each looping over its rounds

using namespace msw_raster_detail;

struct Launch {
  int grid, iters;
};

// Rounds of 64 consecutive items (points or faces) under the cap: both kernels' launches.
Launch pick_rounds(int64_t n) {
  const int64_t rounds = (n + kWave - 1) / kWave;
  Launch l{};
  l.grid = (int)std::min<int64_t>(rounds, kGridCap);
  l.iters = l.grid ? (int)((rounds + l.grid - 1) / l.grid) : 0;
  return l;
}

int report_launch(int64_t n, int32_t* grid, int32_t* per_wg, int32_t* iters) {
  if (!grid || !per_wg || !iters) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n < 0) return msw::set_error(MSW_ERR_INVALID, "negative count");
  const Launch l = pick_rounds(n);
  *grid = l.grid;
  *per_wg = kWave;
  *iters = l.iters;
  return MSW_OK;
}

// ---------------------------------------------------------------------------------- locator
struct PointArgs {
  const FaceRec* rec;
  const int32_t* bptr;   // [nbx * nby + 1]
  const int32_t* bface;  // face indices, ascending within a bucket
  const double* xy;      // [n][2]
  int32_t* out;          // [n]
  int64_t n;
  Buckets b;
};

__global__ __launch_bounds__(kWave) void k_locate_points(PointArgs a) {
  const int lane = threadIdx.x;
  const int64_t rounds = (a.n + kWave - 1) / kWave;
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t i = rb * kWave + lane;
    if (i >= a.n) continue;
    const double px = a.xy[2 * i], py = a.xy[2 * i + 1];
    a.out[i] = locate_walk(a.rec, a.bptr, a.bface, a.b, px, py);
  }
}

}  // namespace

struct msw_locator {
  int device = -1;
  int64_t num_faces = 0;
  FaceRec* d_rec = nullptr;
  int32_t* d_bptr = nullptr;
  int32_t* d_bface = nullptr;
  Buckets b{};
  msw_locator_stats stats{};
};

namespace {

void release(msw_locator* l) {
  (void)hipSetDevice(l->device);
  (void)hipFree(l->d_rec);
  (void)hipFree(l->d_bptr);
  (void)hipFree(l->d_bface);
  delete l;
}

}  // namespace

extern "C" int msw_locate_launch(int64_t n, int32_t* grid, int32_t* points_per_wg, int32_t* iters) {
  return report_launch(n, grid, points_per_wg, iters);
}

extern "C" int msw_locator_create(const double* node_xy, int64_t num_nodes, const int32_t* face_nodes,
                                  const int32_t* face_row, int64_t num_faces, int device, msw_locator** out) {
  if (!out) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *out = nullptr;
  if ((num_nodes > 0 && !node_xy) || (num_faces > 0 && !face_nodes))
    return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (num_nodes < 0 || num_nodes > INT32_MAX || num_faces < 0 || device < 0)
    return msw::set_error(MSW_ERR_INVALID, "num_nodes, num_faces or device out of range");
  if (num_faces > kMaxFaces) return msw::set_error(MSW_ERR_UNSUPPORTED, "more than 2^26 faces");
  const auto t0 = std::chrono::steady_clock::now();
  if (const int rc = check_geometry(node_xy, num_nodes, face_nodes, face_row, num_faces)) return rc;
  HostBuild hb;
  if (const int rc = build_host(node_xy, face_nodes, face_row, num_faces, hb)) return rc;

  msw_locator* l = new msw_locator;
  l->device = device;
  l->num_faces = num_faces;
  l->b = hb.b;
  l->stats.buckets = (int64_t)hb.b.nbx * hb.b.nby;
  l->stats.buckets_x = hb.b.nbx;
  l->stats.buckets_y = hb.b.nby;
  l->stats.list_entries = (int64_t)hb.bface.size();
  l->stats.longest_list = hb.longest;
  l->stats.host_build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  hipError_t e = hipSetDevice(device);
  auto upload = [&](auto** d, const void* h, size_t bytes) {
    if (e != hipSuccess || !bytes) return;
    e = hipMalloc((void**)d, bytes);
    if (e == hipSuccess) l->stats.device_bytes += (int64_t)bytes;
    if (e == hipSuccess) e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
  };
  upload(&l->d_rec, hb.rec.data(), hb.rec.size() * sizeof(FaceRec));
  upload(&l->d_bptr, hb.bptr.data(), hb.bptr.size() * sizeof(int32_t));
  upload(&l->d_bface, hb.bface.data(), hb.bface.size() * sizeof(int32_t));
  if (e != hipSuccess) {
    release(l);
    return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  }
  *out = l;
  return MSW_OK;
}

extern "C" int msw_locator_destroy(msw_locator* loc) {
  if (loc) release(loc);
  return MSW_OK;
}

extern "C" int msw_locator_get_stats(const msw_locator* loc, msw_locator_stats* stats) {
  if (!loc || !stats) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *stats = loc->stats;
  return MSW_OK;
}

extern "C" int msw_locate_points(const msw_locator* loc, const double* xy, int64_t n, int32_t* rows, void* stream) {
  if (!loc) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n < 0) return msw::set_error(MSW_ERR_INVALID, "negative count");
  if (n == 0) return MSW_OK;
  if (!xy || !rows) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (reinterpret_cast<uintptr_t>(xy) % 8 || reinterpret_cast<uintptr_t>(rows) % 4)
    return msw::set_error(MSW_ERR_INVALID, "xy or rows misaligned");
  PointArgs a{};
  a.rec = loc->d_rec, a.bptr = loc->d_bptr, a.bface = loc->d_bface;
  a.xy = xy, a.out = rows, a.n = n, a.b = loc->b;
  hipLaunchKernelGGL(k_locate_points, dim3(pick_rounds(n).grid), dim3(kWave), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  return MSW_OK;
}

// ---------------------------------------------------------------------------------- dual graph
namespace {

constexpr int kEdgeCrowded = -1;  // an edge of the face is shared by more than two faces
constexpr int kTwiceShared = -2;  // the face shares more than one edge with another face

struct FaceArgs {
  const double* xy;       // [V][2]
  const int32_t* fn;      // [nf][3]
  const int32_t* vptr;    // [V + 1]
  const int32_t* vface;   // [3 nf]: the faces round each vertex, ascending
  int64_t nf;
  double* centroid;       // [nf][2]
  double* area;           // [nf]
  int32_t* adjacent;      // [nf][3]
  int32_t* deg;           // [nf]: neighbours, or a negative code
};

__global__ __launch_bounds__(kWave) void k_mesh_faces(FaceArgs a) {
  const int lane = threadIdx.x;
  const int64_t rounds = (a.nf + kWave - 1) / kWave;
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t f = rb * kWave + lane;
    if (f >= a.nf) continue;
    const int32_t v[3] = {a.fn[3 * f], a.fn[3 * f + 1], a.fn[3 * f + 2]};
    const double ax = a.xy[2 * (int64_t)v[0]], ay = a.xy[2 * (int64_t)v[0] + 1];
    const double bx = a.xy[2 * (int64_t)v[1]], by = a.xy[2 * (int64_t)v[1] + 1];
    const double cx = a.xy[2 * (int64_t)v[2]], cy = a.xy[2 * (int64_t)v[2] + 1];
    a.centroid[2 * f] = ((ax + bx) + cx) / 3.0;
    a.centroid[2 * f + 1] = ((ay + by) + cy) / 3.0;
    a.area[f] = 0.5 * fabs((bx - ax) * (cy - ay) - (cx - ax) * (by - ay));
    int32_t adj[3];
    int deg = 0;
    bool crowded = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // edges (a, b), (b, c), (c, a)
      const int32_t u = v[k], w = v[(k + 1) % 3];
      const int32_t lo = u < w ? u : w, hi = u < w ? w : u;
      int32_t other = -1;
      const int32_t end = a.vptr[lo + 1];
      for (int32_t s = a.vptr[lo]; s < end; ++s) {
        const int32_t g = a.vface[s];
        if (g == (int32_t)f) continue;
        const int32_t* gn = a.fn + 3 * (int64_t)g;
        if (gn[0] == hi || gn[1] == hi || gn[2] == hi) {
          crowded |= other >= 0;
          if (other < 0) other = g;
        }
      }
      adj[k] = other;
      deg += other >= 0;
    }
    const bool twice = (adj[0] >= 0 && (adj[0] == adj[1] || adj[0] == adj[2])) || (adj[1] >= 0 && adj[1] == adj[2]);
    a.adjacent[3 * f] = adj[0], a.adjacent[3 * f + 1] = adj[1], a.adjacent[3 * f + 2] = adj[2];
    a.deg[f] = crowded ? kEdgeCrowded : (twice ? kTwiceShared : deg);
  }
}

// sqrt rounded to nearest, as IEEE 754 asks and a host's does.  The device's sqrt is within one ulp;
// r = x - s * s comes exact out of one fma, and x lies beyond the midpoint to the upper neighbour
// s + u iff r > s * u, at or below the midpoint to the lower one s - u' iff r <= -s * u' (r, s * u
// and s * u' are whole multiples of u'^2, which decides the u^2 / 4 of the squared midpoints).
__device__ __forceinline__ double sqrt_rn(double x) {
  const double s = sqrt(x);
  if (!(s > 0x1p-500) || !(s < 0x1p500)) return s;  // 0, NaN, inf; magnitudes where s * u is not exact
  const double r = fma(-s, s, x);
  const double up = nextafter(s, (double)INFINITY), dn = nextafter(s, 0.0);
  if (r > s * (up - s)) return up;
  if (r <= -(s * (s - dn))) return dn;
  return s;
}

struct EdgeArgs {
  const double* centroid;   // [nf][2]
  const int32_t* adjacent;  // [nf][3]
  const int32_t* eptr;      // [nf + 1]: the dual edges of the faces below f; its boundary slots: 3 f - eptr[f]
  int64_t nf, E;
  int64_t* edge_index;      // [2][E]
  double* edge_length;      // [E]
  int32_t* boundary;        // [3 nf - E][2]: (face, slot)
};

__global__ __launch_bounds__(kWave) void k_mesh_edges(EdgeArgs a) {
  const int lane = threadIdx.x;
  const int64_t rounds = (a.nf + kWave - 1) / kWave;
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t f = rb * kWave + lane;
    if (f >= a.nf) continue;
    const int32_t adj[3] = {a.adjacent[3 * f], a.adjacent[3 * f + 1], a.adjacent[3 * f + 2]};
    const int64_t e0 = a.eptr[f];
    int64_t bslot = 3 * f - e0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (adj[k] < 0) {
        a.boundary[2 * bslot] = (int32_t)f, a.boundary[2 * bslot + 1] = k;
        ++bslot;
      }
    // ascending as unsigned: -1 (no neighbour) sorts last
    uint32_t g0 = (uint32_t)adj[0], g1 = (uint32_t)adj[1], g2 = (uint32_t)adj[2], t;
    if (g0 > g1) t = g0, g0 = g1, g1 = t;
    if (g1 > g2) t = g1, g1 = g2, g2 = t;
    if (g0 > g1) t = g0, g0 = g1, g1 = t;
    const uint32_t g[3] = {g0, g1, g2};
    const double fx = a.centroid[2 * f], fy = a.centroid[2 * f + 1];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if ((int32_t)g[j] < 0) continue;
      const double dx = a.centroid[2 * (int64_t)g[j]] - fx, dy = a.centroid[2 * (int64_t)g[j] + 1] - fy;
      a.edge_index[e0 + j] = f;
      a.edge_index[a.E + e0 + j] = (int64_t)g[j];
      a.edge_length[e0 + j] = sqrt_rn(dx * dx + dy * dy);
    }
  }
}

}  // namespace

struct msw_mesh_dual {
  int device = -1;
  int64_t num_faces = 0, num_edges = 0, num_boundary = 0;
  double* d_centroid = nullptr;
  double* d_area = nullptr;
  int32_t* d_adjacent = nullptr;
  int64_t* d_edge_index = nullptr;
  double* d_edge_length = nullptr;
  int32_t* d_boundary = nullptr;
  msw_mesh_dual_stats stats{};
};

namespace {

void release(msw_mesh_dual* d) {
  (void)hipSetDevice(d->device);
  (void)hipFree(d->d_centroid);
  (void)hipFree(d->d_area);
  (void)hipFree(d->d_adjacent);
  (void)hipFree(d->d_edge_index);
  (void)hipFree(d->d_edge_length);
  (void)hipFree(d->d_boundary);
  delete d;
}

int refuse(int64_t face, const char* what) {
  char msg[160];
  std::snprintf(msg, sizeof msg, "face %lld: %s", (long long)face, what);
  return msw::set_error(MSW_ERR_INVALID, msg);
}

}  // namespace

extern "C" int msw_mesh_dual_launch(int64_t num_faces, int32_t* grid, int32_t* faces_per_wg, int32_t* iters) {
  return report_launch(num_faces, grid, faces_per_wg, iters);
}

extern "C" int msw_mesh_dual_create(const double* node_xy, int64_t num_nodes, const int32_t* face_nodes,
                                    int64_t num_faces, int device, void* stream, msw_mesh_dual** out) {
  if (!out) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *out = nullptr;
  if ((num_nodes > 0 && !node_xy) || (num_faces > 0 && !face_nodes))
    return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (num_nodes < 0 || num_nodes > INT32_MAX || num_faces < 0 || device < 0)
    return msw::set_error(MSW_ERR_INVALID, "num_nodes, num_faces or device out of range");
  if (num_faces > kMaxFaces) return msw::set_error(MSW_ERR_UNSUPPORTED, "more than 2^26 faces");
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t nf = num_faces, V = num_nodes;

  // ---- the checks of one face at a time, faces ascending: the first refusal names the lowest face
  for (int64_t f = 0; f < nf; ++f) {
    const int32_t ia = face_nodes[3 * f], ib = face_nodes[3 * f + 1], ic = face_nodes[3 * f + 2];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V)
      return refuse(f, "vertex index outside [0, num_nodes)");
    if (ia == ib || ib == ic || ic == ia) return refuse(f, "repeats a vertex");
    const double ax = node_xy[2 * (int64_t)ia], ay = node_xy[2 * (int64_t)ia + 1];
    const double bx = node_xy[2 * (int64_t)ib], by = node_xy[2 * (int64_t)ib + 1];
    const double cx = node_xy[2 * (int64_t)ic], cy = node_xy[2 * (int64_t)ic + 1];
    if (!std::isfinite(ax) || !std::isfinite(ay) || !std::isfinite(bx) || !std::isfinite(by) || !std::isfinite(cx) ||
        !std::isfinite(cy))
      return refuse(f, "a coordinate is not finite");
    const double area2 = (bx - ax) * (cy - ay) - (cx - ax) * (by - ay);
    if (!std::isfinite(area2) || area2 == 0.0) return refuse(f, "area2 is zero or not finite");
  }
  for (int64_t v = 0; v < 2 * V; ++v)  // a vertex that no face uses
    if (!std::isfinite(node_xy[v])) return msw::set_error(MSW_ERR_INVALID, "node coordinate not finite");

  // ---- vertex -> incident faces, by a counting pass over the faces ascending: every list ascends
  std::vector<int32_t> vptr((size_t)V + 1, 0), vface((size_t)(3 * nf));
  for (int64_t k = 0; k < 3 * nf; ++k) ++vptr[(size_t)face_nodes[k] + 1];
  int64_t longest = 0;
  for (int64_t v = 0; v < V; ++v) {
    longest = std::max<int64_t>(longest, vptr[(size_t)v + 1]);
    vptr[(size_t)v + 1] += vptr[(size_t)v];
  }
  {
    std::vector<int32_t> fill(vptr.begin(), vptr.end() - 1);
    for (int64_t k = 0; k < 3 * nf; ++k) vface[(size_t)fill[(size_t)face_nodes[k]]++] = (int32_t)(k / 3);
  }

  msw_mesh_dual* d = new msw_mesh_dual;
  d->device = device;
  d->num_faces = nf;
  d->stats.num_faces = nf;
  d->stats.longest_star = longest;
  double host_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSetDevice(device);
  double* d_xy = nullptr;
  int32_t *d_fn = nullptr, *d_vptr = nullptr, *d_vface = nullptr, *d_eptr = nullptr;
  auto alloc = [&](auto** p, size_t bytes, bool owned) {
    if (e != hipSuccess || !bytes) return;
    e = hipMalloc((void**)p, bytes);
    if (e == hipSuccess && owned) d->stats.device_bytes += (int64_t)bytes;
  };
  auto upload = [&](auto** p, const void* h, size_t bytes) {
    alloc(p, bytes, false);
    if (e == hipSuccess && bytes) e = hipMemcpyAsync(*p, h, bytes, hipMemcpyHostToDevice, st);
  };
  int64_t bad = -1;
  int bad_code = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  if (nf) {
    upload(&d_xy, node_xy, (size_t)V * 2 * sizeof(double));
    upload(&d_fn, face_nodes, (size_t)nf * 3 * sizeof(int32_t));
    upload(&d_vptr, vptr.data(), vptr.size() * sizeof(int32_t));
    upload(&d_vface, vface.data(), vface.size() * sizeof(int32_t));
    alloc(&d_eptr, (size_t)(nf + 1) * sizeof(int32_t), false);
    alloc(&d->d_centroid, (size_t)nf * 2 * sizeof(double), true);
    alloc(&d->d_area, (size_t)nf * sizeof(double), true);
    alloc(&d->d_adjacent, (size_t)nf * 3 * sizeof(int32_t), true);
    for (auto& v : ev)
      if (e == hipSuccess) e = hipEventCreate(&v);
    const int grid = pick_rounds(nf).grid;
    std::vector<int32_t> host((size_t)nf + 1, 0);
    if (e == hipSuccess) {
      FaceArgs a{};
      a.xy = d_xy, a.fn = d_fn, a.vptr = d_vptr, a.vface = d_vface, a.nf = nf;
      a.centroid = d->d_centroid, a.area = d->d_area, a.adjacent = d->d_adjacent, a.deg = d_eptr;
      (void)hipEventRecord(ev[0], st);
      hipLaunchKernelGGL(k_mesh_faces, dim3(grid), dim3(kWave), 0, st, a);
      e = hipGetLastError();
      (void)hipEventRecord(ev[1], st);
    }
    if (e == hipSuccess)
      e = hipMemcpyAsync(host.data(), d_eptr, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
      const auto t1 = std::chrono::steady_clock::now();
      int64_t sum = 0;  // at most 3 * 2^26
      for (int64_t f = 0; f < nf; ++f) {
        const int32_t n = host[(size_t)f];
        if (n < 0) {
          bad = f, bad_code = n;
          break;
        }
        host[(size_t)f] = (int32_t)sum;
        sum += n;
      }
      host[(size_t)nf] = (int32_t)sum;
      d->num_edges = sum;
      d->num_boundary = 3 * nf - sum;
      host_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    }
    if (e == hipSuccess && bad < 0) {
      alloc(&d->d_edge_index, (size_t)d->num_edges * 2 * sizeof(int64_t), true);
      alloc(&d->d_edge_length, (size_t)d->num_edges * sizeof(double), true);
      alloc(&d->d_boundary, (size_t)d->num_boundary * 2 * sizeof(int32_t), true);
      if (e == hipSuccess)
        e = hipMemcpyAsync(d_eptr, host.data(), (size_t)(nf + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) {
        EdgeArgs a{};
        a.centroid = d->d_centroid, a.adjacent = d->d_adjacent, a.eptr = d_eptr, a.nf = nf, a.E = d->num_edges;
        a.edge_index = d->d_edge_index, a.edge_length = d->d_edge_length, a.boundary = d->d_boundary;
        (void)hipEventRecord(ev[2], st);
        hipLaunchKernelGGL(k_mesh_edges, dim3(grid), dim3(kWave), 0, st, a);
        e = hipGetLastError();
        (void)hipEventRecord(ev[3], st);
      }
      if (e == hipSuccess) e = hipStreamSynchronize(st);  // host is read by the copy until here
      float ms0 = 0.f, ms1 = 0.f;
      if (e == hipSuccess && hipEventElapsedTime(&ms0, ev[0], ev[1]) == hipSuccess &&
          hipEventElapsedTime(&ms1, ev[2], ev[3]) == hipSuccess)
        d->stats.faces_us = 1e3 * (double)ms0, d->stats.edges_us = 1e3 * (double)ms1;
    }
    if (e != hipSuccess) (void)hipStreamSynchronize(st);  // no copy may outlive the host arrays
  }
  for (auto& v : ev)
    if (v) (void)hipEventDestroy(v);
  (void)hipFree(d_xy);
  (void)hipFree(d_fn);
  (void)hipFree(d_vptr);
  (void)hipFree(d_vface);
  (void)hipFree(d_eptr);
  if (e != hipSuccess) {
    release(d);
    return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  }
  if (bad >= 0) {
    release(d);
    return refuse(bad, bad_code == kEdgeCrowded ? "an edge is shared by more than two faces"
                                                : "shares more than one edge with another face");
  }
  d->stats.num_edges = d->num_edges;
  d->stats.num_boundary = d->num_boundary;
  d->stats.host_build_seconds = host_s;
  d->stats.create_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = d;
  return MSW_OK;
}

extern "C" int msw_mesh_dual_destroy(msw_mesh_dual* dual) {
  if (dual) release(dual);
  return MSW_OK;
}

extern "C" int msw_mesh_dual_arrays(const msw_mesh_dual* dual, const double** centroid, const double** area,
                                    const int32_t** adjacent, const int64_t** edge_index,
                                    const double** edge_length, int64_t* num_edges, const int32_t** boundary,
                                    int64_t* num_boundary) {
  if (!dual || !centroid || !area || !adjacent || !edge_index || !edge_length || !num_edges || !boundary ||
      !num_boundary)
    return msw::set_error(MSW_ERR_INVALID, "null argument");
  *centroid = dual->d_centroid, *area = dual->d_area, *adjacent = dual->d_adjacent;
  *edge_index = dual->d_edge_index, *edge_length = dual->d_edge_length, *num_edges = dual->num_edges;
  *boundary = dual->d_boundary, *num_boundary = dual->num_boundary;
  return MSW_OK;
}

extern "C" int msw_mesh_dual_get_stats(const msw_mesh_dual* dual, msw_mesh_dual_stats* stats) {
  if (!dual || !stats) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *stats = dual->stats;
  return MSW_OK;
}
