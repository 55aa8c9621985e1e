// Zonal statistics: raster layers and frame stacks reduced onto the cells of one mesh scale, the
// transpose of raster.hip (semantics: include/mswegnn.h, "Zonal statistics").  msw_raster_create
// has located every pixel centre (pixel_rows); msw_zonal_create turns that into a CSR of pixel
// indices per face, and every later call is a reduction over those lists.
//
// Create, on the device, no sort and no atomics:
// k_zonal_prepare.  Lane = face: face_row, the centre pixel and the face's pixel box -- the
// pixels whose centre can lie in the bounding box widened by face_margin (the bucket grid's own
// guarantee for a located pixel), over-covered by a pixel on each side; membership is decided by
// pixel_rows alone, so a box that is too large costs time, never a wrong entry.
// k_zonal_scan<FILL>.  Workgroup = wave = face, grid-stride: the box in row-major chunks of 64, a
// ballot of pixel_rows[p] == row per chunk; a lane's slot is the running base plus the popcount
// of the lower lanes, so a list comes out ascending.  Once to count, a prefix sum on the host
// (create is synchronous anyway), once to fill.
//
// The reduction, layers in groups of 8 (one read of a list entry serves 8 gathers).  The mapping is
// chosen per face, by the length n of its list alone, and each kind has its own launch (create
// keeps the faces with n > 32 as a list; a launch with nothing to do is not made):
//   k_zonal_reduce_lane, n <= 32: lane = face, 64 consecutive faces per round; the lane walks its
//            list front to back;
//   k_zonal_reduce_wave, n  > 32: workgroup = wave = face; lane k takes the entries k, k + 64, ...
//            front to back, then a butterfly over the lanes (xor 32, 16, 8, 4, 2, 1) -- no LDS.
// The order of the float64 sum is therefore a function of the list alone.  msw_zonal_frames is the
// same two kernels with the mean alone, written at [row][var][t] strides.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <vector>

#include "../../include/mswegnn.h"
#include "engine.h"
#include "raster_handle.h"

// Every operation rounds on its own, as written: the centre pixel is restated operation for
// operation by the tests.
#pragma clang fp contract(off)

using namespace msw_raster_detail;

namespace {

constexpr int kWave = 64;
constexpr int kGridCap = 4096;  // workgroups: 16 per CU, each looping over its rounds
// Lists up to this length are summed by the face's own lane.  The build variants "zonallane" (every
// list by its lane) and "zonalwave" (every list by the wave) exist to measure the choice
// (tools/zonal_bench.py --mappings); their sums follow another order than the header documents.
#ifndef MSW_ZONAL_SERIAL
#define MSW_ZONAL_SERIAL 32
#endif
constexpr int kSerial = MSW_ZONAL_SERIAL;
constexpr int kGroup = 8;       // layers per pass over a list

struct Box {
  int32_t i0, i1, j0, j1;  // inclusive; i1 < i0: empty
};

// The indices i in [0, n) with lo - 1 <= i <= hi + 1 (lo <= hi in pixel units, maybe infinite).
__device__ __forceinline__ void span(double lo, double hi, int n, int32_t& i0, int32_t& i1) {
  const double a = floor(lo) - 1.0, b = ceil(hi) + 1.0;
  if (!(b >= 0.0) || !(a <= (double)(n - 1))) {
    i0 = 0, i1 = -1;
    return;
  }
  i0 = a > 0.0 ? (int32_t)a : 0;
  i1 = b < (double)(n - 1) ? (int32_t)b : n - 1;
}

struct PrepareArgs {
  const FaceRec* rec;
  int64_t nf;
  double x0, y0, dx, dy;
  int W, H;
  int32_t* frow;
  int32_t* centre;
  Box* box;
};

__global__ __launch_bounds__(kWave) void k_zonal_prepare(PrepareArgs a) {
  for (int64_t f = (int64_t)blockIdx.x * kWave + threadIdx.x; f < a.nf; f += (int64_t)gridDim.x * kWave) {
    const FaceRec r = a.rec[f];
    a.frow[f] = r.row;
    const double cx = ((r.ax + r.bx) + r.cx) / 3.0, cy = ((r.ay + r.by) + r.cy) / 3.0;
    const double fi = floor((cx - a.x0) / a.dx + 0.5), fj = floor((cy - a.y0) / a.dy + 0.5);
    const bool in = fi >= 0.0 && fi < (double)a.W && fj >= 0.0 && fj < (double)a.H;
    a.centre[f] = in ? (int32_t)fj * a.W + (int32_t)fi : -1;
    Box b{0, -1, 0, -1};
    const double area2 = (r.bx - r.ax) * (r.cy - r.ay) - (r.by - r.ay) * (r.cx - r.ax);
    if (r.row >= 0 && (area2 > 0.0 || area2 < 0.0)) {
      const double xlo = fmin(fmin(r.ax, r.bx), r.cx), xhi = fmax(fmax(r.ax, r.bx), r.cx);
      const double ylo = fmin(fmin(r.ay, r.by), r.cy), yhi = fmax(fmax(r.ay, r.by), r.cy);
      const double m = face_margin(fmax(xhi - xlo, yhi - ylo), area2);
      const double u0 = (xlo - m - a.x0) / a.dx, u1 = (xhi + m - a.x0) / a.dx;
      const double v0 = (ylo - m - a.y0) / a.dy, v1 = (yhi + m - a.y0) / a.dy;
      span(fmin(u0, u1), fmax(u0, u1), a.W, b.i0, b.i1);
      span(fmin(v0, v1), fmax(v0, v1), a.H, b.j0, b.j1);
      if (b.j1 < b.j0) b.i0 = 0, b.i1 = -1;
    }
    a.box[f] = b;
  }
}

struct ScanArgs {
  const int32_t* prow;  // [H][W]
  const int32_t* frow;
  const Box* box;
  int64_t nf;
  int W;
  int32_t* fptr;        // count pass: [f] = the list's length; fill pass: the lists' starts
  int32_t* pix;
};

template <bool FILL>
__global__ __launch_bounds__(kWave) void k_zonal_scan(ScanArgs a) {
  const int lane = threadIdx.x;
  for (int64_t f = blockIdx.x; f < a.nf; f += gridDim.x) {  // uniform per workgroup
    const int row = a.frow[f];
    const Box b = a.box[f];
    int base = FILL ? a.fptr[f] : 0;
    if (row >= 0 && b.i1 >= b.i0) {
      const uint32_t bw = (uint32_t)(b.i1 - b.i0 + 1);
      const uint32_t total = bw * (uint32_t)(b.j1 - b.j0 + 1);  // <= width * height < 2^31
      for (uint32_t q0 = 0; q0 < total; q0 += kWave) {
        const uint32_t q = q0 + lane;
        bool hit = false;
        int32_t p = 0;
        if (q < total) {
          const uint32_t jj = q / bw, ii = q - jj * bw;
          p = (int32_t)((int64_t)(b.j0 + (int32_t)jj) * a.W + b.i0 + (int32_t)ii);
          hit = a.prow[p] == row;
        }
        const unsigned long long mask = __ballot(hit);
        if (FILL && hit) a.pix[base + __popcll(mask & ((1ull << lane) - 1ull))] = p;
        base += __popcll(mask);
      }
    }
    if (!FILL && lane == 0) a.fptr[f] = base;
  }
}

struct ReduceArgs {
  const int32_t* fptr;
  const int32_t* pix;
  const int32_t* centre;
  const int32_t* frow;
  const int32_t* wide;  // the faces whose lists are longer than kSerial, ascending
  int64_t nf, nwide;
  const uint32_t* in;  // [L][stride] words
  int L;
  int64_t stride;
  uint32_t* mean;      // any of the four may be null
  int32_t* count;
  uint32_t* vmin;
  uint32_t* vmax;
  int64_t out_base, out_row, out_layer;  // element = out_base + row * out_row + layer * out_layer
  uint32_t nodata;
  int fill;
};

// IEEE order on non-NaN words as unsigned keys, -0.0 below +0.0; word_of inverts key_of.
__device__ __forceinline__ uint32_t key_of(uint32_t w) { return w ^ ((w >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ uint32_t word_of(uint32_t k) { return k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu); }

// The running statistics of kGroup layers of one list (or of one lane's share of it).
struct Acc {
  double s[kGroup];
  int32_t n[kGroup];
  uint32_t lo[kGroup], hi[kGroup];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int u = 0; u < kGroup; ++u) s[u] = 0.0, n[u] = 0, lo[u] = 0xFFFFFFFFu, hi[u] = 0u;
  }
  __device__ __forceinline__ void add(int u, uint32_t w) {  // u: a constant after unrolling
    const float v = __uint_as_float(w);
    if (v == v) {  // a NaN is skipped
      s[u] += (double)v;
      ++n[u];
      const uint32_t k = key_of(w);
      lo[u] = min(lo[u], k), hi[u] = max(hi[u], k);
    }
  }
};

// Layers l0 .. l0 + kGroup - 1 of the face with row r and centre pixel c: the outputs' words.
__device__ __forceinline__ void write_cell(const ReduceArgs& a, const Acc& acc, int l0, int r, int c) {
#pragma unroll
  for (int u = 0; u < kGroup; ++u) {
    if (l0 + u >= a.L) break;  // uniform
    uint32_t m, lo, hi;
    if (acc.n[u] > 0) {
      m = __float_as_uint((float)(acc.s[u] / (double)acc.n[u]));
      lo = word_of(acc.lo[u]), hi = word_of(acc.hi[u]);
    } else {
      m = lo = hi = (a.fill && c >= 0) ? a.in[(int64_t)(l0 + u) * a.stride + c] : a.nodata;
    }
    const int64_t o = a.out_base + (int64_t)r * a.out_row + (int64_t)(l0 + u) * a.out_layer;
    if (a.mean) a.mean[o] = m;
    if (a.count) a.count[o] = acc.n[u];
    if (a.vmin) a.vmin[o] = lo;
    if (a.vmax) a.vmax[o] = hi;
  }
}

// Lists of up to kSerial entries: lane = face, a round = 64 consecutive faces.
__global__ __launch_bounds__(kWave) void k_zonal_reduce_lane(ReduceArgs a) {
  const int lane = threadIdx.x;
  const int64_t rounds = (a.nf + kWave - 1) / kWave;
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t f = rb * kWave + lane;
    int r = -1, b = 0, n = 0, c = -1;
    if (f < a.nf) r = a.frow[f];
    if (r >= 0) b = a.fptr[f], n = a.fptr[f + 1] - b, c = a.centre[f];
    if (r < 0 || n > kSerial) continue;  // no value, or the wave launch's
    for (int l0 = 0; l0 < a.L; l0 += kGroup) {
      const uint32_t* src = a.in + (int64_t)l0 * a.stride;
      Acc acc;
      acc.clear();
      for (int e = 0; e < n; ++e) {  // front to back
        const int p = a.pix[b + e];
#pragma unroll
        for (int u = 0; u < kGroup; ++u)
          if (l0 + u < a.L) acc.add(u, src[(int64_t)u * a.stride + p]);
      }
      write_cell(a, acc, l0, r, c);
    }
  }
}

// Longer lists: workgroup = wave = face, over the handle's list of such faces.
__global__ __launch_bounds__(kWave) void k_zonal_reduce_wave(ReduceArgs a) {
  const int lane = threadIdx.x;
  for (int64_t i = blockIdx.x; i < a.nwide; i += gridDim.x) {  // uniform per workgroup
    const int f = a.wide[i];
    const int r = a.frow[f], b = a.fptr[f], n = a.fptr[f + 1] - b, c = a.centre[f];
    for (int l0 = 0; l0 < a.L; l0 += kGroup) {
      const uint32_t* src = a.in + (int64_t)l0 * a.stride;
      Acc acc;
      acc.clear();
      for (int e = lane; e < n; e += 2 * kWave) {  // two entries of the lane's share in flight
        const bool two = e + kWave < n;
        const int p0 = a.pix[b + e], p1 = two ? a.pix[b + e + kWave] : p0;
        uint32_t w0[kGroup], w1[kGroup];
#pragma unroll
        for (int u = 0; u < kGroup; ++u)
          if (l0 + u < a.L) w0[u] = src[(int64_t)u * a.stride + p0], w1[u] = src[(int64_t)u * a.stride + p1];
#pragma unroll
        for (int u = 0; u < kGroup; ++u)
          if (l0 + u < a.L) {
            acc.add(u, w0[u]);
            if (two) acc.add(u, w1[u]);
          }
      }
#pragma unroll
      for (int u = 0; u < kGroup; ++u) {
        if (l0 + u >= a.L) break;  // uniform
#pragma unroll
        for (int d = kWave / 2; d >= 1; d >>= 1) {  // x + y == y + x: every lane ends with the same bits
          acc.s[u] += __shfl_xor(acc.s[u], d);
          acc.n[u] += __shfl_xor(acc.n[u], d);
          acc.lo[u] = min(acc.lo[u], (uint32_t)__shfl_xor((int)acc.lo[u], d));
          acc.hi[u] = max(acc.hi[u], (uint32_t)__shfl_xor((int)acc.hi[u], d));
        }
      }
      if (lane == 0) write_cell(a, acc, l0, r, c);
    }
  }
}

struct Launch {
  int grid, iters;
};

// The reduce launch over num_faces faces: msw_zonal_launch reports it, the launcher uses it.
Launch pick_reduce(int64_t nf) {
  const int64_t rounds = (nf + kWave - 1) / kWave;
  Launch l{};
  l.grid = (int)std::min<int64_t>(rounds, kGridCap);
  l.iters = l.grid ? (int)((rounds + l.grid - 1) / l.grid) : 0;
  return l;
}

// Two faces with the same face_row >= 0?
bool rows_shared(const std::vector<int32_t>& rows, int32_t max_row) {
  if (max_row < 0) return false;
  if ((int64_t)max_row < 64 * (int64_t)rows.size() + 4096) {
    std::vector<char> seen((size_t)max_row + 1, 0);
    for (const int32_t r : rows)
      if (r >= 0) {
        if (seen[(size_t)r]) return true;
        seen[(size_t)r] = 1;
      }
    return false;
  }
  std::vector<int32_t> v;
  for (const int32_t r : rows)
    if (r >= 0) v.push_back(r);
  std::sort(v.begin(), v.end());
  return std::adjacent_find(v.begin(), v.end()) != v.end();
}

}  // namespace

struct msw_zonal {
  int device = -1;
  int32_t width = 0, height = 0;
  int64_t num_faces = 0;
  int32_t min_row = 0, max_row = -1;  // the raster handle's
  int32_t* d_frow = nullptr;
  int32_t* d_fptr = nullptr;
  int32_t* d_pix = nullptr;
  int32_t* d_centre = nullptr;
  int32_t* d_wide = nullptr;  // faces with lists longer than kSerial
  int64_t num_short = 0;      // valued faces with lists up to kSerial
  msw_zonal_stats stats{};
};

namespace {

void release(msw_zonal* z) {
  (void)hipSetDevice(z->device);
  (void)hipFree(z->d_frow);
  (void)hipFree(z->d_fptr);
  (void)hipFree(z->d_pix);
  (void)hipFree(z->d_centre);
  (void)hipFree(z->d_wide);
  delete z;
}

int check_rows(const msw_zonal* z, int64_t row_offset, int64_t num_rows) {
  if (z->max_row < 0) return MSW_OK;  // nothing is ever written
  if (row_offset < -(int64_t)z->min_row || row_offset >= num_rows - z->max_row)
    return msw::set_error(MSW_ERR_INVALID, "row_offset + face_row outside [0, num_rows)");
  return MSW_OK;
}

int launch_reduce(const msw_zonal* z, ReduceArgs& a, void* stream) {
  a.fptr = z->d_fptr, a.pix = z->d_pix, a.centre = z->d_centre, a.frow = z->d_frow, a.wide = z->d_wide;
  a.nf = z->num_faces, a.nwide = z->stats.wave_faces;
  hipError_t e = hipSuccess;
  if (z->num_short) {
    hipLaunchKernelGGL(k_zonal_reduce_lane, dim3(pick_reduce(a.nf).grid), dim3(kWave), 0, (hipStream_t)stream, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess && a.nwide) {
    const int grid = (int)std::min<int64_t>(a.nwide, kGridCap);
    hipLaunchKernelGGL(k_zonal_reduce_wave, dim3(grid), dim3(kWave), 0, (hipStream_t)stream, a);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  return MSW_OK;
}

}  // namespace

extern "C" int msw_zonal_launch(int64_t num_faces, int32_t* grid, int32_t* faces_per_wg, int32_t* iters) {
  if (!grid || !faces_per_wg || !iters) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (num_faces < 0) return msw::set_error(MSW_ERR_INVALID, "num_faces negative");
  const Launch l = pick_reduce(num_faces);
  *grid = l.grid;
  *faces_per_wg = kWave;
  *iters = l.iters;
  return MSW_OK;
}

extern "C" int msw_zonal_create(const msw_raster* raster, void* stream, msw_zonal** out) {
  if (!out) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!raster) return msw::set_error(MSW_ERR_INVALID, "null argument");
  const auto t0 = std::chrono::steady_clock::now();
  const int64_t nf = raster->num_faces;
  const msw_raster_grid g = raster->g;
  hipStream_t st = (hipStream_t)stream;

  msw_zonal* z = new msw_zonal;
  z->device = raster->device;
  z->width = g.width, z->height = g.height;
  z->num_faces = nf;
  z->min_row = raster->min_row, z->max_row = raster->max_row;
  z->stats.num_faces = nf;

  Box* d_box = nullptr;
  hipError_t e = hipSetDevice(z->device);
  auto alloc = [&](auto** d, size_t bytes, bool owned) {
    if (e != hipSuccess) return;
    e = hipMalloc((void**)d, bytes);
    if (e == hipSuccess && owned) z->stats.device_bytes += (int64_t)bytes;
  };
  alloc(&z->d_frow, (size_t)std::max<int64_t>(nf, 1) * sizeof(int32_t), true);
  alloc(&z->d_centre, (size_t)std::max<int64_t>(nf, 1) * sizeof(int32_t), true);
  alloc(&z->d_fptr, (size_t)(nf + 1) * sizeof(int32_t), true);
  alloc(&d_box, (size_t)std::max<int64_t>(nf, 1) * sizeof(Box), false);

  const int scan_grid = (int)std::min<int64_t>(nf, kGridCap);
  std::vector<int32_t> host((size_t)nf + 1, 0);
  bool shared = false;
  if (e == hipSuccess && nf) {
    PrepareArgs p{};
    p.rec = raster->d_rec, p.nf = nf;
    p.x0 = g.x0, p.y0 = g.y0, p.dx = g.dx, p.dy = g.dy, p.W = g.width, p.H = g.height;
    p.frow = z->d_frow, p.centre = z->d_centre, p.box = d_box;
    hipLaunchKernelGGL(k_zonal_prepare, dim3(pick_reduce(nf).grid), dim3(kWave), 0, st, p);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), z->d_frow, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
      host.pop_back();
      shared = rows_shared(host, z->max_row);
      host.push_back(0);
    }
  }
  std::vector<int32_t> valued;  // 1 where face_row >= 0
  std::vector<int32_t> wide;    // the faces of the wave launch
  if (e == hipSuccess && !shared && nf) {
    valued.resize((size_t)nf);
    for (int64_t f = 0; f < nf; ++f) valued[(size_t)f] = host[(size_t)f] >= 0;
    ScanArgs s{};
    s.prow = raster->d_prow, s.frow = z->d_frow, s.box = d_box, s.nf = nf, s.W = g.width;
    s.fptr = z->d_fptr, s.pix = nullptr;
    hipLaunchKernelGGL(k_zonal_scan<false>, dim3(scan_grid), dim3(kWave), 0, st, s);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host.data(), z->d_fptr, (size_t)nf * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) {
      int64_t sum = 0;  // at most width * height < 2^31: a pixel is in one list
      for (int64_t f = 0; f < nf; ++f) {
        const int32_t n = host[(size_t)f];
        z->stats.longest_list = std::max<int64_t>(z->stats.longest_list, n);
        z->stats.empty_faces += valued[(size_t)f] && n == 0;
        if (n > kSerial) wide.push_back((int32_t)f);
        else z->num_short += valued[(size_t)f];
        host[(size_t)f] = (int32_t)sum;
        sum += n;
      }
      host[(size_t)nf] = (int32_t)sum;
      z->stats.listed_pixels = sum;
    }
  }
  if (e == hipSuccess && !shared) {
    alloc(&z->d_pix, (size_t)std::max<int64_t>(z->stats.listed_pixels, 1) * sizeof(int32_t), true);
    z->stats.wave_faces = (int64_t)wide.size();
    alloc(&z->d_wide, std::max<size_t>(wide.size(), 1) * sizeof(int32_t), true);
    if (e == hipSuccess)
      e = hipMemcpyAsync(z->d_fptr, host.data(), (size_t)(nf + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && !wide.empty())
      e = hipMemcpyAsync(z->d_wide, wide.data(), wide.size() * sizeof(int32_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && z->stats.listed_pixels) {
      ScanArgs s{};
      s.prow = raster->d_prow, s.frow = z->d_frow, s.box = d_box, s.nf = nf, s.W = g.width;
      s.fptr = z->d_fptr, s.pix = z->d_pix;
      hipLaunchKernelGGL(k_zonal_scan<true>, dim3(scan_grid), dim3(kWave), 0, st, s);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  (void)hipFree(d_box);
  if (e != hipSuccess) {
    release(z);
    return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  }
  if (shared) {
    release(z);
    return msw::set_error(MSW_ERR_UNSUPPORTED, "two faces share a face_row: the lists are keyed by face");
  }
  z->stats.build_us = 1e6 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  *out = z;
  return MSW_OK;
}

extern "C" int msw_zonal_destroy(msw_zonal* zonal) {
  if (zonal) release(zonal);
  return MSW_OK;
}

extern "C" int msw_zonal_lists(const msw_zonal* zonal, const int32_t** face_ptr, const int32_t** pixels,
                               const int32_t** centre_pixel) {
  if (!zonal || !face_ptr || !pixels || !centre_pixel) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *face_ptr = zonal->d_fptr;
  *pixels = zonal->d_pix;
  *centre_pixel = zonal->d_centre;
  return MSW_OK;
}

extern "C" int msw_zonal_get_stats(const msw_zonal* zonal, msw_zonal_stats* stats) {
  if (!zonal || !stats) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *stats = zonal->stats;
  return MSW_OK;
}

extern "C" int msw_zonal_reduce(const msw_zonal* zonal, const float* layers, int32_t num_layers, int64_t layer_stride,
                                int64_t row_offset, int64_t num_rows, int64_t out_stride, int32_t fill_centre,
                                uint32_t nodata_bits, float* mean, int32_t* count, float* vmin, float* vmax,
                                void* stream) {
  if (!zonal || !layers) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (!mean && !count && !vmin && !vmax) return msw::set_error(MSW_ERR_INVALID, "no output");
  if (num_layers < 0 || layer_stride < 0 || num_rows < 0 || out_stride < 0)
    return msw::set_error(MSW_ERR_INVALID, "num_layers, layer_stride, num_rows or out_stride negative");
  if (num_layers > 1 && (layer_stride > INT64_MAX / 8 / num_layers || out_stride > INT64_MAX / 8 / num_layers))
    return msw::set_error(MSW_ERR_INVALID, "layer_stride or out_stride too large");
  if (const int rc = check_rows(zonal, row_offset, num_rows)) return rc;
  if (num_layers == 0) return MSW_OK;
  ReduceArgs a{};
  a.in = reinterpret_cast<const uint32_t*>(layers);
  a.L = num_layers;
  a.stride = layer_stride;
  a.mean = reinterpret_cast<uint32_t*>(mean), a.count = count;
  a.vmin = reinterpret_cast<uint32_t*>(vmin), a.vmax = reinterpret_cast<uint32_t*>(vmax);
  a.out_base = row_offset, a.out_row = 1, a.out_layer = out_stride;
  a.nodata = nodata_bits;
  a.fill = fill_centre != 0;
  return launch_reduce(zonal, a, stream);
}

extern "C" int msw_zonal_frames(const msw_zonal* zonal, const float* frames, int64_t frame_stride, float* pred,
                                int64_t N, int32_t T, int32_t var, int32_t t_begin, int32_t t_count,
                                int64_t row_offset, int32_t fill_centre, uint32_t nodata_bits, void* stream) {
  if (!zonal || !frames || !pred) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (var != 0 && var != 1) return msw::set_error(MSW_ERR_INVALID, "var is 0 (depth) or 1 (discharge)");
  if (N < 0 || T < 0 || t_begin < 0 || t_count < 0 || (int64_t)t_begin + t_count > T)
    return msw::set_error(MSW_ERR_INVALID, "time window outside [0, T]");
  if (frame_stride < 0 || (t_count > 1 && frame_stride > INT64_MAX / 8 / t_count))
    return msw::set_error(MSW_ERR_INVALID, "frame_stride negative or too large");
  if (const int rc = check_rows(zonal, row_offset, N)) return rc;
  if (t_count == 0) return MSW_OK;
  ReduceArgs a{};
  a.in = reinterpret_cast<const uint32_t*>(frames);
  a.L = t_count;
  a.stride = frame_stride;
  a.mean = reinterpret_cast<uint32_t*>(pred);
  const int64_t off = zonal->max_row >= 0 ? row_offset : 0;  // checked against N above
  a.out_base = (off * 2 + var) * (int64_t)T + t_begin, a.out_row = 2 * (int64_t)T, a.out_layer = 1;
  a.nodata = nodata_bits;
  a.fill = fill_centre != 0;
  return launch_reduce(zonal, a, stream);
}
