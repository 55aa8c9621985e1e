// Raster products: per-cell maps and rollout frames resampled onto a regular grid (semantics:
// include/mswegnn.h, "Raster products").  Locating the pixel centres in the mesh's triangles is
// the work; it is done once per (mesh, grid) at msw_raster_create and kept as pixel_rows, and
// every later product is a gather through it.
//
// Host: the face records and the bucket grid of locate_common.h (build_host), which meshgraph.hip
// shares for arbitrary points.
//
// k_raster_locate.  One workgroup = one wave = one 8 x 8 pixel block (lanes of a wave share
// buckets and face records through the cache), grid-stride over the blocks.  A pixel outside the
// bucket grid gets -1 without touching memory.  No LDS, no atomics.
// k_raster_sample.  Lane = pixel, a round = 64 consecutive pixels; pixel_rows is read once per
// pixel for all layers, four gathers in flight, each layer's store one coalesced line of the wave.
// k_raster_frames.  Lane = pixel; its row's steps come four at a time (one 16-byte load where
// pred, T and t_begin allow, else scalar loads) and go out as four stores into four frames, each
// coalesced across the wave.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/mswegnn.h"
#include "engine.h"
#include "locate_common.h"
#include "raster_handle.h"

// Every operation rounds on its own, as written (host and device): the pixel centres here, the
// edge functions, area2 and bucket_of in locate_common.h are restated operation for operation by
// the tests.
#pragma clang fp contract(off)

namespace {

constexpr int kWave = 64;
constexpr int kGridCap = 4096;  // workgroups: 16 per CU (4 waves per SIMD), each looping over its rounds
constexpr int kBlock = 8;       // a wave is a kBlock x kBlock pixel block

using namespace msw_raster_detail;  // FaceRec (raster_handle.h); Buckets, locate_walk, build_host (locate_common.h)

struct LocateArgs {
  const FaceRec* rec;
  const int32_t* bptr;   // [nbx * nby + 1]
  const int32_t* bface;  // face indices, ascending within a bucket
  int32_t* out;          // [H][W]
  double x0, y0, dx, dy;
  int W, H;
  Buckets b;
  int bw;                // pixel blocks per row of blocks
  int64_t nblocks;
};

__global__ __launch_bounds__(kWave) void k_raster_locate(LocateArgs a) {
  const int lane = threadIdx.x;
  for (int64_t blk = blockIdx.x; blk < a.nblocks; blk += gridDim.x) {  // uniform per workgroup
    const int by = (int)(blk / a.bw), bx = (int)(blk - (int64_t)by * a.bw);
    const int i = bx * kBlock + (lane & (kBlock - 1)), j = by * kBlock + (lane >> 3);
    if (i >= a.W || j >= a.H) continue;
    const double px = a.x0 + (double)i * a.dx, py = a.y0 + (double)j * a.dy;
    a.out[(int64_t)j * a.W + i] = locate_walk(a.rec, a.bptr, a.bface, a.b, px, py);
  }
}

struct SampleArgs {
  const int32_t* prow;
  int64_t P;              // pixels
  const uint32_t* layers;
  int L;
  int64_t stride, off;
  uint32_t nodata;
  uint32_t* out;          // [L][P]
};

__global__ __launch_bounds__(kWave) void k_raster_sample(SampleArgs a) {
  const int lane = threadIdx.x;
  const int64_t rounds = (a.P + kWave - 1) / kWave;
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t i = rb * kWave + lane;
    if (i >= a.P) continue;
    const int r = a.prow[i];
    const uint32_t* src = a.layers + a.off + (r >= 0 ? r : 0);  // not dereferenced when r < 0
    for (int l0 = 0; l0 < a.L; l0 += 4) {                        // uniform
      uint32_t v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = (r >= 0 && l0 + e < a.L) ? src[(int64_t)(l0 + e) * a.stride] : a.nodata;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (l0 + e < a.L) a.out[(int64_t)(l0 + e) * a.P + i] = v[e];
    }
  }
}

struct FrameArgs {
  const int32_t* prow;
  int64_t P;
  const uint32_t* pred;  // [N][2][T] as words
  int T, var, tb, tc;
  int64_t off;
  uint32_t nodata;
  uint32_t* out;         // [tc][P]
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <bool VEC>
__global__ __launch_bounds__(kWave) void k_raster_frames(FrameArgs a) {
  const int lane = threadIdx.x;
  const int64_t rounds = (a.P + kWave - 1) / kWave;
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t i = rb * kWave + lane;
    if (i >= a.P) continue;
    const int r = a.prow[i];
    // step t_begin of the row's var half; not dereferenced when r < 0
    const uint32_t* src = a.pred + ((a.off + (r >= 0 ? r : 0)) * 2 + a.var) * (int64_t)a.T + a.tb;
    for (int k0 = 0; k0 < a.tc; k0 += 4) {  // uniform
      uint32_t v[4] = {a.nodata, a.nodata, a.nodata, a.nodata};
      if (r >= 0) {
        if constexpr (VEC) {
          // T and t_begin + k0 are multiples of 4: the four words lie inside the row's half
          const u32x4 w = *reinterpret_cast<const u32x4*>(src + k0);
          v[0] = w[0], v[1] = w[1], v[2] = w[2], v[3] = w[3];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e)
            if (k0 + e < a.tc) v[e] = src[k0 + e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (k0 + e < a.tc) a.out[(int64_t)(k0 + e) * a.P + i] = v[e];
    }
  }
}

struct Launch {
  int grid, iters, bw;
  int64_t nblocks;
};

// The locate launch of a W x H grid: msw_raster_launch reports it, msw_raster_create uses it.
Launch pick_locate(int W, int H) {
  Launch l{};
  l.bw = (W + kBlock - 1) / kBlock;
  l.nblocks = (int64_t)l.bw * ((H + kBlock - 1) / kBlock);
  l.grid = (int)std::min<int64_t>(l.nblocks, kGridCap);
  l.iters = (int)((l.nblocks + l.grid - 1) / l.grid);
  return l;
}

int pixel_grid(int64_t P) { return (int)std::min<int64_t>((P + kWave - 1) / kWave, kGridCap); }

int check_grid(int32_t W, int32_t H) {
  if (W < 1 || H < 1) return msw::set_error(MSW_ERR_INVALID, "width and height must be at least 1");
  if ((int64_t)W * H > INT32_MAX) return msw::set_error(MSW_ERR_INVALID, "width * height exceeds 2^31 - 1");
  return MSW_OK;
}

}  // namespace

namespace {

void release(msw_raster* r) {
  (void)hipSetDevice(r->device);
  (void)hipFree(r->d_rec);
  (void)hipFree(r->d_bptr);
  (void)hipFree(r->d_bface);
  (void)hipFree(r->d_prow);
  delete r;
}

int check_rows(const msw_raster* r, int64_t row_offset, int64_t num_rows) {
  if (r->max_row < 0) return MSW_OK;  // nothing is ever read
  if (row_offset < -(int64_t)r->min_row || row_offset >= num_rows - r->max_row)
    return msw::set_error(MSW_ERR_INVALID, "row_offset + face_row outside [0, num_rows)");
  return MSW_OK;
}

}  // namespace

extern "C" int msw_raster_launch(int32_t width, int32_t height, int32_t* grid, int32_t* pixels_per_wg,
                                 int32_t* iters) {
  if (!grid || !pixels_per_wg || !iters) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (const int rc = check_grid(width, height)) return rc;
  const Launch l = pick_locate(width, height);
  *grid = l.grid;
  *pixels_per_wg = kBlock * kBlock;
  *iters = l.iters;
  return MSW_OK;
}

extern "C" int msw_raster_create(const double* node_xy, int64_t num_nodes, const int32_t* face_nodes,
                                 const int32_t* face_row, int64_t num_faces, const msw_raster_grid* grid,
                                 int device, void* stream, msw_raster** out) {
  if (!out) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!grid || (num_nodes > 0 && !node_xy) || (num_faces > 0 && !face_nodes))
    return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (num_nodes < 0 || num_nodes > INT32_MAX || num_faces < 0 || device < 0)
    return msw::set_error(MSW_ERR_INVALID, "num_nodes, num_faces or device out of range");
  if (num_faces > kMaxFaces) return msw::set_error(MSW_ERR_UNSUPPORTED, "more than 2^26 faces");
  const msw_raster_grid g = *grid;
  if (!std::isfinite(g.x0) || !std::isfinite(g.y0) || !std::isfinite(g.dx) || !std::isfinite(g.dy))
    return msw::set_error(MSW_ERR_INVALID, "grid origin or pixel size not finite");
  if (g.dx == 0.0 || g.dy == 0.0) return msw::set_error(MSW_ERR_INVALID, "pixel size zero");
  if (const int rc = check_grid(g.width, g.height)) return rc;
  if (!std::isfinite(g.x0 + (double)(g.width - 1) * g.dx) || !std::isfinite(g.y0 + (double)(g.height - 1) * g.dy))
    return msw::set_error(MSW_ERR_INVALID, "pixel centres not finite");
  const auto t0 = std::chrono::steady_clock::now();
  if (const int rc = check_geometry(node_xy, num_nodes, face_nodes, face_row, num_faces)) return rc;

  HostBuild hb;
  if (const int rc = build_host(node_xy, face_nodes, face_row, num_faces, hb)) return rc;
  const Buckets& b = hb.b;

  msw_raster* rs = new msw_raster;
  rs->device = device;
  rs->g = g;
  rs->num_faces = num_faces;
  rs->min_row = hb.min_row;
  rs->max_row = hb.max_row;
  rs->stats.buckets = (int64_t)b.nbx * b.nby;
  rs->stats.buckets_x = b.nbx;
  rs->stats.buckets_y = b.nby;
  rs->stats.list_entries = (int64_t)hb.bface.size();
  rs->stats.longest_list = hb.longest;
  rs->stats.host_build_seconds =
      std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

  const int64_t P = (int64_t)g.width * g.height;
  hipError_t e = hipSetDevice(device);
  auto upload = [&](auto** d, const void* h, size_t bytes) {
    if (e != hipSuccess || !bytes) return;
    e = hipMalloc((void**)d, bytes);
    if (e == hipSuccess) rs->stats.device_bytes += (int64_t)bytes;
    if (e == hipSuccess && h) e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
  };
  upload(&rs->d_rec, hb.rec.data(), hb.rec.size() * sizeof(FaceRec));
  upload(&rs->d_bptr, hb.bptr.data(), hb.bptr.size() * sizeof(int32_t));
  upload(&rs->d_bface, hb.bface.data(), hb.bface.size() * sizeof(int32_t));
  upload(&rs->d_prow, nullptr, (size_t)P * sizeof(int32_t));
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  if (e == hipSuccess) e = hipEventCreate(&ev0);
  if (e == hipSuccess) e = hipEventCreate(&ev1);
  if (e == hipSuccess) {
    hipStream_t st = (hipStream_t)stream;
    const Launch l = pick_locate(g.width, g.height);
    LocateArgs a{};
    a.rec = rs->d_rec, a.bptr = rs->d_bptr, a.bface = rs->d_bface, a.out = rs->d_prow;
    a.x0 = g.x0, a.y0 = g.y0, a.dx = g.dx, a.dy = g.dy;
    a.W = g.width, a.H = g.height;
    a.b = b;
    a.bw = l.bw, a.nblocks = l.nblocks;
    (void)hipEventRecord(ev0, st);
    hipLaunchKernelGGL(k_raster_locate, dim3(l.grid), dim3(kWave), 0, st, a);
    e = hipGetLastError();
    (void)hipEventRecord(ev1, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    float ms = 0.f;
    if (e == hipSuccess && hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) rs->stats.locate_us = 1e3 * (double)ms;
  }
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  if (e != hipSuccess) {
    release(rs);
    return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  }
  *out = rs;
  return MSW_OK;
}

extern "C" int msw_raster_destroy(msw_raster* raster) {
  if (raster) release(raster);
  return MSW_OK;
}

extern "C" int msw_raster_pixel_rows(const msw_raster* raster, const int32_t** pixel_rows) {
  if (!raster || !pixel_rows) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *pixel_rows = raster->d_prow;
  return MSW_OK;
}

extern "C" int msw_raster_get_stats(const msw_raster* raster, msw_raster_stats* stats) {
  if (!raster || !stats) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *stats = raster->stats;
  return MSW_OK;
}

extern "C" int msw_raster_sample(const msw_raster* raster, const void* layers, int32_t num_layers,
                                 int64_t layer_stride, int64_t row_offset, int64_t num_rows, uint32_t nodata_bits,
                                 void* out, void* stream) {
  if (!raster || !layers || !out) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (num_layers < 0 || layer_stride < 0 || num_rows < 0)
    return msw::set_error(MSW_ERR_INVALID, "num_layers, layer_stride or num_rows negative");
  if (num_layers > 1 && layer_stride > INT64_MAX / 8 / num_layers)
    return msw::set_error(MSW_ERR_INVALID, "layer_stride too large");
  if (const int rc = check_rows(raster, row_offset, num_rows)) return rc;
  if (num_layers == 0) return MSW_OK;
  SampleArgs a{};
  a.prow = raster->d_prow;
  a.P = (int64_t)raster->g.width * raster->g.height;
  a.layers = static_cast<const uint32_t*>(layers);
  a.L = num_layers;
  a.stride = layer_stride;
  a.off = raster->max_row >= 0 ? row_offset : 0;
  a.nodata = nodata_bits;
  a.out = static_cast<uint32_t*>(out);
  hipLaunchKernelGGL(k_raster_sample, dim3(pixel_grid(a.P)), dim3(kWave), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  return MSW_OK;
}

extern "C" int msw_raster_frames(const msw_raster* raster, const float* pred, int64_t N, int32_t T, int32_t var,
                                 int32_t t_begin, int32_t t_count, int64_t row_offset, uint32_t nodata_bits,
                                 void* out, void* stream) {
  if (!raster || !pred || !out) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (var != 0 && var != 1) return msw::set_error(MSW_ERR_INVALID, "var is 0 (depth) or 1 (discharge)");
  if (N < 0 || T < 0 || t_begin < 0 || t_count < 0 || (int64_t)t_begin + t_count > T)
    return msw::set_error(MSW_ERR_INVALID, "time window outside [0, T]");
  if (const int rc = check_rows(raster, row_offset, N)) return rc;
  if (t_count == 0) return MSW_OK;
  FrameArgs a{};
  a.prow = raster->d_prow;
  a.P = (int64_t)raster->g.width * raster->g.height;
  a.pred = reinterpret_cast<const uint32_t*>(pred);
  a.T = T, a.var = var, a.tb = t_begin, a.tc = t_count;
  a.off = raster->max_row >= 0 ? row_offset : 0;
  a.nodata = nodata_bits;
  a.out = static_cast<uint32_t*>(out);
  const bool vec = T % 4 == 0 && t_begin % 4 == 0 && reinterpret_cast<uintptr_t>(pred) % 16 == 0;
  const dim3 grid(pixel_grid(a.P));
  if (vec)
    hipLaunchKernelGGL(k_raster_frames<true>, grid, dim3(kWave), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_raster_frames<false>, grid, dim3(kWave), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  return MSW_OK;
}
