// Locality order: rows sorted along a Hilbert curve inside each (graph, scale) segment, the base
// row order of msw_plan_create_ordered (semantics: include/mswegnn.h, "Locality order").
//
// k_hilbert_keys.  Lane = row, a round = 256 consecutive rows, grid-stride over the rounds.  The
// row's segment (its box) by a binary search over seg_ptr; the cell from separate float64
// operations (sc = 65536.0 / side, fx = (x - x0) * sc, clamp, floor); the key by the bit loop
//     d = 0;  for (s = 32768; s > 0; s >>= 1) {
//         rx = (ix & s) != 0;  ry = (iy & s) != 0;  d += s * s * ((3 * rx) ^ ry);
//         if (!ry) { if (rx) { ix = 65535 - ix; iy = 65535 - iy; }  swap(ix, iy); } }
// (tests/locality_cases.py hilbert_keys_ref restates both, bit for bit).  No LDS, no atomics.
//
// Stable LSD radix sort of (key, row) pairs, 8-bit digits: four passes over the key, then the
// segment index of the row as further digits (one pass up to 256 segments; none for one segment),
// so one sort serves every segment and the last pass leaves each segment in place.  A pass is
// three launches over one geometry (pick_launch): every 256-thread workgroup owns one contiguous
// run of `iters` rounds of 256 items.
//   k_radix_count    the run's digit histogram in LDS -> table[digit][workgroup] (digit-major)
//   k_radix_scan     one workgroup: exclusive scan of the table in place
//   k_radix_scatter  an item's place = table[digit][workgroup] + items of that digit earlier in the
//                    run: the running per-workgroup counter (LDS, advanced once a round by thread =
//                    digit), the counts of the lower waves of the round, and the item's rank among
//                    the equal digits of its wave's 64 items from eight __ballot masks.
// Every count is a sum of integers and every item has one writer and one place: no output bit
// depends on an order of execution.  No global atomics; the LDS atomics of the count add integers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mswegnn.h"
#include "engine.h"

// Every operation rounds on its own, as written (the key's quantisation is restated by the tests).
#pragma clang fp contract(off)

namespace {

constexpr int kWG = 256;        // threads of a workgroup = items of a round = digit values
constexpr int kWaves = kWG / 64;
constexpr int kGridCap = 1024;  // workgroups: 4 per CU; the digit table holds 256 x grid counters
constexpr int kScanWG = 1024;
constexpr int64_t kMaxRows = 1LL << 26;

struct Launch {
  int grid, iters;
};

// Rounds of 256 consecutive items, `iters` consecutive rounds per workgroup, under the cap.
Launch pick_launch(int64_t n) {
  const int64_t rounds = (n + kWG - 1) / kWG;
  Launch l{0, 0};
  if (!rounds) return l;
  const int64_t g = std::min<int64_t>(rounds, kGridCap);
  l.iters = (int)((rounds + g - 1) / g);
  l.grid = (int)((rounds + l.iters - 1) / l.iters);
  return l;
}

struct Box {
  double x0, y0, side;
};

// The segment of row r: seg_ptr[j] <= r < seg_ptr[j + 1] (empty segments hold no row).
__device__ __forceinline__ int segment_of(const int32_t* seg_ptr, int num_segs, uint32_t r) {
  int lo = 0, hi = num_segs;  // first j in (0, num_segs] with seg_ptr[j] > r, minus one
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((uint32_t)seg_ptr[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ uint32_t cell_of(double v, double lo, double sc) {
  const double f = (v - lo) * sc;
  return f < 0.0 ? 0u : (f >= 65536.0 ? 65535u : (uint32_t)(int)floor(f));
}

__device__ __forceinline__ uint32_t hilbert_index(uint32_t x, uint32_t y) {
  uint32_t d = 0;
#pragma unroll
  for (uint32_t s = 32768u; s > 0; s >>= 1) {
    const uint32_t rx = (x & s) != 0, ry = (y & s) != 0;
    d += s * s * ((3u * rx) ^ ry);
    if (!ry) {
      if (rx) x = 65535u - x, y = 65535u - y;
      const uint32_t t = x;
      x = y, y = t;
    }
  }
  return d;
}

struct KeyArgs {
  const double* xy;         // [n][2]
  uint32_t* keys;           // [n]
  int64_t n;
  const int32_t* seg_ptr;   // [num_segs + 1] (device); unused with one segment
  const Box* boxes;         // [num_segs] (device); unused with one segment
  int num_segs;
  Box box0;                 // the box of a single segment
};

__global__ __launch_bounds__(kWG) void k_hilbert_keys(KeyArgs a) {
  const int64_t rounds = (a.n + kWG - 1) / kWG;
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t i = rb * kWG + threadIdx.x;
    if (i >= a.n) continue;
    const double x = a.xy[2 * i], y = a.xy[2 * i + 1];
    Box b = a.box0;
    if (a.num_segs > 1) b = a.boxes[segment_of(a.seg_ptr, a.num_segs, (uint32_t)i)];
    const double sc = 65536.0 / b.side;
    uint32_t key = 0xFFFFFFFFu;
    if (isfinite(x) && isfinite(y)) key = hilbert_index(cell_of(x, b.x0, sc), cell_of(y, b.y0, sc));
    a.keys[i] = key;
  }
}

struct PassArgs {
  const uint32_t* keys_in;  // NULL: the digit comes from the row's segment
  const uint32_t* vals_in;  // NULL: item i is row i (the first pass)
  uint32_t* keys_out;       // NULL: the keys are not needed after this pass
  uint32_t* vals_out;
  uint32_t* table;          // [256][grid]
  const int32_t* seg_ptr;   // [num_segs + 1] (device)
  int64_t n;
  int num_segs, iters, shift;
};

__device__ __forceinline__ uint32_t digit_of(const PassArgs& a, uint32_t key, uint32_t val) {
  const uint32_t word = a.keys_in ? key : (uint32_t)segment_of(a.seg_ptr, a.num_segs, val);
  return (word >> a.shift) & 255u;
}

__global__ __launch_bounds__(kWG) void k_radix_count(PassArgs a) {
  __shared__ uint32_t hist[kWG];
  const int tid = threadIdx.x;
  hist[tid] = 0;
  __syncthreads();
  const int64_t run0 = (int64_t)blockIdx.x * a.iters * kWG;
  for (int it = 0; it < a.iters; ++it) {
    const int64_t i = run0 + (int64_t)it * kWG + tid;
    if (i >= a.n) break;
    const uint32_t key = a.keys_in ? a.keys_in[i] : 0u, val = a.vals_in ? a.vals_in[i] : (uint32_t)i;
    atomicAdd(&hist[digit_of(a, key, val)], 1u);
  }
  __syncthreads();
  a.table[(size_t)tid * gridDim.x + blockIdx.x] = hist[tid];
}

// Exclusive scan of table[0 .. total) in place, total a multiple of 4: one workgroup, 4096 entries
// a step (one 16-byte load per thread), a wave scan by shuffles and the 16 wave totals through LDS.
__global__ __launch_bounds__(kScanWG) void k_radix_scan(uint32_t* table, int total) {
  __shared__ uint32_t wsum[kScanWG / 64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  uint32_t carry = 0;
  for (int base = 0; base < total; base += 4 * kScanWG) {  // uniform
    const int idx = base + 4 * tid;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (idx < total) v = *reinterpret_cast<const uint4*>(table + idx);
    const uint32_t mine = v.x + v.y + v.z + v.w;
    uint32_t incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t up = __shfl_up(incl, o);
      if (lane >= o) incl += up;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kScanWG / 64; ++k) {
      const uint32_t t = wsum[k];
      before += k < w ? t : 0u;
      all += t;
    }
    const uint32_t e = carry + before + (incl - mine);
    if (idx < total) *reinterpret_cast<uint4*>(table + idx) = make_uint4(e, e + v.x, e + v.x + v.y, e + v.x + v.y + v.z);
    carry += all;
    __syncthreads();
  }
}

__global__ __launch_bounds__(kWG) void k_radix_scatter(PassArgs a) {
  __shared__ uint32_t place[kWG];          // next free place of each digit for this workgroup
  __shared__ uint32_t wcnt[kWaves][kWG];   // items of each digit in each wave of the round
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  place[tid] = a.table[(size_t)tid * gridDim.x + blockIdx.x];
#pragma unroll
  for (int k = 0; k < kWaves; ++k) wcnt[k][tid] = 0;
  __syncthreads();
  const int64_t run0 = (int64_t)blockIdx.x * a.iters * kWG;
  for (int it = 0; it < a.iters; ++it) {
    const int64_t r0 = run0 + (int64_t)it * kWG;
    if (r0 >= a.n) break;  // uniform per workgroup
    const int64_t i = r0 + tid;
    const bool valid = i < a.n;
    uint32_t key = 0, val = 0, d = 0;
    if (valid) {
      key = a.keys_in ? a.keys_in[i] : 0u;
      val = a.vals_in ? a.vals_in[i] : (uint32_t)i;
      d = digit_of(a, key, val);
    }
    unsigned long long same = __ballot(valid);  // the lanes of this wave with my digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long m = __ballot(bit);
      same &= bit ? m : ~m;
    }
    const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
    if (valid && rank == 0) wcnt[w][d] = (uint32_t)__popcll(same);
    __syncthreads();
    if (valid) {
      uint32_t pos = place[d] + rank;
#pragma unroll
      for (int k = 0; k < kWaves; ++k) pos += k < w ? wcnt[k][d] : 0u;
      if ((int64_t)pos < a.n) {
        if (a.keys_out) a.keys_out[pos] = key;
        a.vals_out[pos] = val;
      }
    }
    __syncthreads();
    uint32_t add = 0;  // thread = digit: the round's items move the counter on
#pragma unroll
    for (int k = 0; k < kWaves; ++k) add += wcnt[k][tid], wcnt[k][tid] = 0;
    place[tid] += add;
    __syncthreads();
  }
}

// A box the keys are defined in: finite, side positive and sc = 65536.0 / side finite (a subnormal
// side would make sc infinite and 0 * sc a NaN with no cell).
bool good_box(double x0, double y0, double side) {
  return std::isfinite(x0) && std::isfinite(y0) && std::isfinite(side) && side > 0.0 && std::isfinite(65536.0 / side);
}

int check_segments(int64_t n, const int64_t* seg_ptr, int32_t num_segs) {
  if (num_segs < 1) return msw::set_error(MSW_ERR_INVALID, "num_segs < 1");
  if (seg_ptr[0] != 0 || seg_ptr[num_segs] != n) return msw::set_error(MSW_ERR_INVALID, "seg_ptr must span [0, n]");
  for (int j = 0; j < num_segs; ++j)
    if (seg_ptr[j + 1] < seg_ptr[j]) return msw::set_error(MSW_ERR_INVALID, "seg_ptr not monotone");
  return MSW_OK;
}

// Keys (given, or made from xy by k_hilbert_keys) -> order.  Host-synchronous; owns its scratch.
int order_impl(const double* xy, const uint32_t* keys_in, int64_t n, const int64_t* seg_ptr, int32_t num_segs,
               const double* boxes, int32_t* order, int device, void* stream, msw_locality_stats* stats) {
  if (stats) *stats = msw_locality_stats{};
  if ((!xy && !keys_in) || !seg_ptr || !order || (xy && !boxes)) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n < 0 || device < 0) return msw::set_error(MSW_ERR_INVALID, "negative count or device");
  if (n > kMaxRows) return msw::set_error(MSW_ERR_UNSUPPORTED, "more than 2^26 rows");
  if (const int rc = check_segments(n, seg_ptr, num_segs)) return rc;
  if (xy)
    for (int j = 0; j < num_segs; ++j)
      if (!good_box(boxes[3 * j], boxes[3 * j + 1], boxes[3 * j + 2]))
        return msw::set_error(MSW_ERR_INVALID, ("box of segment " + std::to_string(j) +
                                                ": must be finite, side positive and 65536 / side finite").c_str());
  if (reinterpret_cast<uintptr_t>(xy) % 8 || reinterpret_cast<uintptr_t>(keys_in) % 4 ||
      reinterpret_cast<uintptr_t>(order) % 4)
    return msw::set_error(MSW_ERR_INVALID, "xy, keys or order misaligned");
  if (n == 0) return MSW_OK;

  const Launch l = pick_launch(n);
  int seg_bits = 0;
  while ((1LL << seg_bits) < num_segs) ++seg_bits;
  const int passes = 4 + (seg_bits + 7) / 8;
  std::vector<int32_t> seg32(seg_ptr, seg_ptr + num_segs + 1);
  std::vector<Box> hbox;
  if (xy)
    for (int j = 0; j < num_segs; ++j) hbox.push_back(Box{boxes[3 * j], boxes[3 * j + 1], boxes[3 * j + 2]});

  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipSetDevice(device);
  int64_t bytes = 0;
  uint32_t *d_ka = nullptr, *d_kb = nullptr, *d_vals = nullptr, *d_table = nullptr;
  int32_t* d_seg = nullptr;
  Box* d_box = nullptr;
  auto alloc = [&](auto** p, size_t b) {
    if (e != hipSuccess || !b) return;
    e = hipMalloc((void**)p, b);
    if (e == hipSuccess) bytes += (int64_t)b;
  };
  const size_t table_entries = (size_t)kWG * l.grid;
  alloc(&d_ka, (size_t)n * 4);
  alloc(&d_kb, (size_t)n * 4);
  alloc(&d_vals, (size_t)n * 4);
  alloc(&d_table, table_entries * 4);
  alloc(&d_seg, seg32.size() * 4);
  if (xy && num_segs > 1) alloc(&d_box, hbox.size() * sizeof(Box));
  if (e == hipSuccess) e = hipMemcpyAsync(d_seg, seg32.data(), seg32.size() * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && d_box) e = hipMemcpyAsync(d_box, hbox.data(), hbox.size() * sizeof(Box), hipMemcpyHostToDevice, st);
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  for (auto& v : ev)
    if (e == hipSuccess) e = hipEventCreate(&v);
  if (e == hipSuccess) {
    (void)hipEventRecord(ev[0], st);
    if (xy) {
      KeyArgs k{};
      k.keys = d_kb;  // read by the first pass, rewritten by the second
      k.xy = xy, k.n = n, k.seg_ptr = d_seg, k.boxes = d_box, k.num_segs = num_segs, k.box0 = hbox[0];
      hipLaunchKernelGGL(k_hilbert_keys, dim3(l.grid), dim3(kWG), 0, st, k);
      e = hipGetLastError();
    }
    (void)hipEventRecord(ev[1], st);
  }
  uint32_t* const out = reinterpret_cast<uint32_t*>(order);
  for (int p = 0; p < passes && e == hipSuccess; ++p) {
    PassArgs a{};
    a.n = n, a.table = d_table, a.seg_ptr = d_seg, a.num_segs = num_segs, a.iters = l.iters;
    a.shift = 8 * (p & 3);
    if (p < 4) a.keys_in = p == 0 ? (xy ? d_kb : keys_in) : ((p & 1) ? d_ka : d_kb);
    if (p < 3) a.keys_out = (p & 1) ? d_kb : d_ka;
    // the last pass writes `order`: the passes alternate between it and the scratch rows
    const bool to_order = ((passes - 1 - p) & 1) == 0;
    a.vals_out = to_order ? out : d_vals;
    a.vals_in = p == 0 ? nullptr : (to_order ? d_vals : out);
    hipLaunchKernelGGL(k_radix_count, dim3(l.grid), dim3(kWG), 0, st, a);
    hipLaunchKernelGGL(k_radix_scan, dim3(1), dim3(kScanWG), 0, st, d_table, (int)table_entries);
    hipLaunchKernelGGL(k_radix_scatter, dim3(l.grid), dim3(kWG), 0, st, a);
    e = hipGetLastError();
  }
  if (e == hipSuccess) (void)hipEventRecord(ev[2], st);
  const hipError_t sync = hipStreamSynchronize(st);  // no copy may outlive the host arrays
  if (e == hipSuccess) e = sync;
  float ms0 = 0.f, ms1 = 0.f;
  if (e == hipSuccess && stats && hipEventElapsedTime(&ms0, ev[0], ev[1]) == hipSuccess &&
      hipEventElapsedTime(&ms1, ev[1], ev[2]) == hipSuccess)
    stats->keys_us = xy ? 1e3 * (double)ms0 : 0.0, stats->sort_us = 1e3 * (double)ms1;
  for (auto& v : ev)
    if (v) (void)hipEventDestroy(v);
  for (void* p : {(void*)d_ka, (void*)d_kb, (void*)d_vals, (void*)d_table, (void*)d_seg, (void*)d_box})
    (void)hipFree(p);
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  if (stats) {
    stats->n = n, stats->num_segs = num_segs, stats->scratch_bytes = bytes;
    stats->passes = passes, stats->grid = l.grid;
  }
  return MSW_OK;
}

}  // namespace

extern "C" int msw_locality_launch(int64_t n, int32_t* grid, int32_t* items_per_wg, int32_t* iters) {
  if (!grid || !items_per_wg || !iters) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n < 0) return msw::set_error(MSW_ERR_INVALID, "negative count");
  const Launch l = pick_launch(n);
  *grid = l.grid;
  *items_per_wg = kWG;
  *iters = l.iters;
  return MSW_OK;
}

extern "C" int msw_hilbert_keys(const double* xy, int64_t n, double x0, double y0, double side, uint32_t* keys,
                                void* stream) {
  if (n < 0) return msw::set_error(MSW_ERR_INVALID, "negative count");
  if (n > kMaxRows) return msw::set_error(MSW_ERR_UNSUPPORTED, "more than 2^26 rows");
  if (!good_box(x0, y0, side))
    return msw::set_error(MSW_ERR_INVALID, "box: must be finite, side positive and 65536 / side finite");
  if (n == 0) return MSW_OK;
  if (!xy || !keys) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (reinterpret_cast<uintptr_t>(xy) % 8 || reinterpret_cast<uintptr_t>(keys) % 4)
    return msw::set_error(MSW_ERR_INVALID, "xy or keys misaligned");
  KeyArgs k{};
  k.xy = xy, k.keys = keys, k.n = n, k.num_segs = 1, k.box0 = Box{x0, y0, side};
  hipLaunchKernelGGL(k_hilbert_keys, dim3(pick_launch(n).grid), dim3(kWG), 0, (hipStream_t)stream, k);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  return MSW_OK;
}

extern "C" int msw_locality_order(const double* xy, int64_t n, const int64_t* seg_ptr, int32_t num_segs,
                                  const double* boxes, int32_t* order, int device, void* stream,
                                  msw_locality_stats* stats) {
  if (!xy) return msw::set_error(MSW_ERR_INVALID, "null argument");
  return order_impl(xy, nullptr, n, seg_ptr, num_segs, boxes, order, device, stream, stats);
}

extern "C" int msw_locality_sort(const uint32_t* keys, int64_t n, const int64_t* seg_ptr, int32_t num_segs,
                                 int32_t* order, int device, void* stream, msw_locality_stats* stats) {
  if (!keys) return msw::set_error(MSW_ERR_INVALID, "null argument");
  return order_impl(nullptr, keys, n, seg_ptr, num_segs, nullptr, order, device, stream, stats);
}
