// On-device zone series: a rollout [N][2][T] reduced over space into per-(zone, step) series, the
// spatial sibling of the flood maps (floodmaps.hip).  A zone is an arbitrary list of graph rows
// (a district, a polder, one simulation of a batch; a gauge is a one-row zone); per zone and step:
//   volume     sum (double)a * (double)h        wet_area[k]   sum (double)a over rows with h > thr_k
//   h_max      max h                            wet_cells[k]  number of such rows
//   q_max      max |q|
// (the stored volume is what the reference's mass-conservation metric sums, training/loss.py:120-169).
// Every listed rollout value is read once.
//
// Order of additions.  The row list of a zone is cut into chunks of kChunk consecutive entries.  A
// chunk is summed in list order from 0; a zone of one chunk is written directly, a longer zone's
// chunk sums go to scratch and k_zone_combine adds them in chunk order.  Every term is exact in
// fp64 (a product of two floats, or a float), so the order is all that matters, and it depends on
// the list alone: not on the window, the grid or how a rollout was cut into calls.  No atomics.
//
// One workgroup = one wave.  A unit is one chunk x one tile of kTile steps; the wave first copies
// the chunk's row ids and areas to LDS, then stages its rows kRound at a time through registers
// into LDS -- a listed row is two runs of the tile's steps, loaded 16 bytes at a time when the
// base, T and the window's first step are multiples of 16 bytes (the last load of a run may reach
// past the window but never past the run: T is then a multiple of 4), else float by float -- and
// lane t adds step t of the staged rows in list order while the next round's loads are in flight.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mswegnn.h"
#include "engine.h"

namespace {

constexpr int kWave = 64;
constexpr int kTile = 64;        // steps of a unit: one per lane
constexpr int kRound = 16;       // rows staged at once: 16 * 2 * 64 floats = 8 KiB of LDS, 32 registers per lane
constexpr int kChunk = 256;      // list entries of a chunk (the unit of the summation order)
constexpr int kGridCap = 4096;   // workgroups: 16 per CU (4 waves per SIMD), each looping over its units
constexpr int kRowBatch = 4;     // rows whose LDS reads a lane issues before it adds them
constexpr int kMaxSlab = 1024;   // steps per launch at most; longer windows run as successive launches
constexpr int64_t kScratchBytes = 32ll << 20;  // partials of one launch (bounds the steps per launch)
constexpr int kSlotBytes = 8 + MSW_MAX_MAP_THRESHOLDS * (8 + 4) + 4 + 4;  // partials per (chunk, step)

struct Chunk {
  int64_t off;    // first entry in the row list
  int32_t count;  // entries (0: an empty zone, which still writes its zeros)
  int32_t zone;
  int32_t slot;   // row of the scratch arrays, or -1: the zone's only chunk, written directly
};

struct Multi {  // a zone of several chunks: scratch rows [first, first + n)
  int32_t zone, first, n;
};

struct Launch {
  int grid, iters;
};

struct Partials {  // [.][S] scratch arrays, one row per chunk of a multi-chunk zone
  double* vol;
  double* area;    // [MSW_MAX_MAP_THRESHOLDS][P][S]
  int32_t* cells;  // [MSW_MAX_MAP_THRESHOLDS][P][S]
  float *h, *q;
  int64_t P;
  int S;
};

struct SeriesArgs {
  const float* pred;  // [N][2][T]
  const float* area;  // [N] or NULL
  const int32_t* rows;
  const Chunk* chunks;
  const Multi* multi;
  int nchunks, nmulti;
  int T, tb, tc;      // window [tb, tb + tc) of this launch
  int col0;           // output column of step tb
  int T_out;
  int64_t Z;
  int vec;
  float thr[MSW_MAX_MAP_THRESHOLDS];
  msw_zone_series o;
  Partials p;
};

}  // namespace

struct msw_zones {
  int device = -1;  // -1: host-only (launch queries)
  int64_t Z = 0, num_rows = 0, nchunks = 0, nslots = 0, nmulti = 0;
  int S = kMaxSlab;  // steps per launch
  int32_t* d_rows = nullptr;
  Chunk* d_chunks = nullptr;
  Multi* d_multi = nullptr;
  char* d_scratch = nullptr;
};

namespace {

// The launch of one slab of tc <= zones->S steps: msw_zone_series_launch reports it, the launcher uses it.
Launch pick_launch(const msw_zones* z, int tc) {
  tc = std::min(tc, z->S);
  const int64_t units = tc > 0 ? z->nchunks * ((tc + kTile - 1) / kTile) : 0;
  Launch l;
  l.grid = (int)std::min<int64_t>(units, kGridCap);
  l.iters = l.grid ? (int)((units + l.grid - 1) / l.grid) : 0;
  return l;
}

template <int NTHR>
struct Acc {
  double vol, wa[NTHR > 0 ? NTHR : 1];
  int nc[NTHR > 0 ? NTHR : 1];
  float h, q;
};

// Store one (zone, column) of the outputs.
template <int NTHR>
__device__ __forceinline__ void store_out(const SeriesArgs& a, int zone, int col, const Acc<NTHR>& s) {
  const msw_zone_series& o = a.o;
  const int64_t i = (int64_t)zone * a.T_out + col;
  if (o.volume) o.volume[i] = s.vol;
  if (o.h_max) o.h_max[i] = s.h;
  if (o.q_max) o.q_max[i] = s.q;
#pragma unroll
  for (int k = 0; k < NTHR; ++k) {
    const int64_t j = ((int64_t)k * a.Z + zone) * a.T_out + col;
    if (o.wet_area) o.wet_area[j] = s.wa[k];
    if (o.wet_cells) o.wet_cells[j] = s.nc[k];
  }
}

// A round's nseg = 2 nr segments (row, variable) of w steps go to LDS, segment s at
// lds + s * kTile: unit u = lane, lane + 64, ... is 4 floats (16-byte loader) or 1 (scalar loader)
// at flattened index (segment, column); L units per segment, (segment, column) advance by
// (qs, rs) per pass without a division.
constexpr int kVecUnits = kRound * 2 * kTile / (kWave * 4);  // 16-byte units of a round per lane: 8
constexpr int kLoadBatch = 8;  // scalar loader: loads a lane has in flight before it stores them to LDS

struct Stage {
  int nseg, L, qs, rs;
};
typedef float f32x4 __attribute__((ext_vector_type(4)));

// 16-byte loader, first half: a whole round into the lane's registers.
__device__ __forceinline__ void load_round(const SeriesArgs& a, int64_t t_first, const int* s_row, const Stage& g,
                                           int lane, f32x4 (&v)[kVecUnits]) {
  int seg = lane / g.L, c = lane - seg * g.L;
#pragma unroll
  for (int i = 0; i < kVecUnits; ++i) {
    if (seg < g.nseg) {
      const float* p = a.pred + ((int64_t)s_row[seg >> 1] * 2 + (seg & 1)) * a.T + t_first + c * 4;
      v[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    }
    c += g.rs;
    seg += g.qs;
    if (c >= g.L) { c -= g.L; ++seg; }
  }
}

// Second half: the registers to LDS.
__device__ __forceinline__ void store_round(float* lds, const Stage& g, int lane, const f32x4 (&v)[kVecUnits]) {
  int seg = lane / g.L, c = lane - seg * g.L;
#pragma unroll
  for (int i = 0; i < kVecUnits; ++i) {
    if (seg < g.nseg) *reinterpret_cast<f32x4*>(lds + seg * kTile + c * 4) = v[i];
    c += g.rs;
    seg += g.qs;
    if (c >= g.L) { c -= g.L; ++seg; }
  }
}

// Scalar loader: a round to LDS, kLoadBatch floats per lane at a time.
__device__ __forceinline__ void stage_scalar(const SeriesArgs& a, int64_t t_first, const int* s_row, float* lds,
                                             const Stage& g, int lane) {
  int seg = lane / g.L, c = lane - seg * g.L;
  while (seg < g.nseg) {
    int s[kLoadBatch], cc[kLoadBatch];
    float v[kLoadBatch];
#pragma unroll
    for (int i = 0; i < kLoadBatch; ++i) {
      s[i] = seg;
      cc[i] = c;
      c += g.rs;
      seg += g.qs;
      if (c >= g.L) { c -= g.L; ++seg; }
    }
#pragma unroll
    for (int i = 0; i < kLoadBatch; ++i)
      if (s[i] < g.nseg)
        v[i] = __builtin_nontemporal_load(a.pred + ((int64_t)s_row[s[i] >> 1] * 2 + (s[i] & 1)) * a.T + t_first + cc[i]);
#pragma unroll
    for (int i = 0; i < kLoadBatch; ++i)
      if (s[i] < g.nseg) lds[s[i] * kTile + cc[i]] = v[i];
  }
}

// Lane t adds step t of the round's nr staged rows in list order; lanes past the tile's steps
// read words no load wrote and their sums are dropped.
template <int NTHR>
__device__ __forceinline__ void reduce_round(const SeriesArgs& a, const float* lds, const float* s_a, int nr, int lane,
                                             Acc<NTHR>& s) {
  for (int j = 0; j < nr; j += kRowBatch) {
    float hv[kRowBatch], qv[kRowBatch], av[kRowBatch];
#pragma unroll
    for (int i = 0; i < kRowBatch; ++i) {
      const int jj = min(j + i, nr - 1);
      hv[i] = lds[2 * jj * kTile + lane];
      qv[i] = fabsf(lds[(2 * jj + 1) * kTile + lane]);
      av[i] = s_a[jj];
    }
#pragma unroll
    for (int i = 0; i < kRowBatch; ++i) {
      if (j + i < nr) {
        const double ad = (double)av[i];
        s.vol += ad * (double)hv[i];  // the product is exact in fp64: fused or not, one rounding
        s.h = hv[i] > s.h ? hv[i] : s.h;
        s.q = qv[i] > s.q ? qv[i] : s.q;
#pragma unroll
        for (int k = 0; k < NTHR; ++k) {
          const bool wet = hv[i] > a.thr[k];
          s.wa[k] += wet ? ad : 0.0;
          s.nc[k] += wet ? 1 : 0;
        }
      }
    }
  }
}

// One chunk x one tile.  16-byte loader: the loads of round r + 1 are in flight while round r is
// added.  Scalar loader: load, then add.
template <bool VEC, int NTHR>
__device__ __forceinline__ void chunk_sum(const SeriesArgs& a, int64_t t_first, int count, int L, float* lds,
                                          const int* s_row, const float* s_a, int lane, Acc<NTHR>& s) {
  Stage g{2 * min(kRound, count), L, kWave / L, kWave % L};
  f32x4 v[kVecUnits];
  if constexpr (VEC)
    if (count > 0) load_round(a, t_first, s_row, g, lane, v);
  for (int r0 = 0; r0 < count; r0 += kRound) {
    const int nr = min(kRound, count - r0), next = min(kRound, count - r0 - kRound);
    g.nseg = 2 * nr;
    if constexpr (VEC)
      store_round(lds, g, lane, v);
    else
      stage_scalar(a, t_first, s_row + r0, lds, g, lane);
    __syncthreads();
    if constexpr (VEC) {
      if (next > 0) {
        g.nseg = 2 * next;
        load_round(a, t_first, s_row + r0 + kRound, g, lane, v);
      }
    }
    reduce_round<NTHR>(a, lds, s_a + r0, nr, lane, s);
    __syncthreads();  // the rows are consumed: the next round may overwrite them
  }
}

template <int NTHR>
__global__ __launch_bounds__(kWave) void k_zone_series(SeriesArgs a) {
  __shared__ __attribute__((aligned(16))) float lds[kRound * 2 * kTile];
  __shared__ int s_row[kChunk];  // the chunk's rows and their areas
  __shared__ float s_a[kChunk];
  const int lane = threadIdx.x;
  const int ntiles = (a.tc + kTile - 1) / kTile;
  const int64_t units = (int64_t)a.nchunks * ntiles;
  for (int64_t u = blockIdx.x; u < units; u += gridDim.x) {  // uniform per workgroup
    const int c = (int)(u / ntiles), t0 = (int)(u - (int64_t)c * ntiles) * kTile;
    const Chunk ch = a.chunks[c];
    const int w = min(kTile, a.tc - t0);  // steps of this tile
    for (int i = lane; i < ch.count; i += kWave) {
      const int row = a.rows[ch.off + i];
      s_row[i] = row;
      s_a[i] = a.area ? a.area[row] : 1.f;
    }
    __syncthreads();
    Acc<NTHR> s;
    s.vol = 0.0;
    s.h = -INFINITY;
    s.q = 0.f;
#pragma unroll
    for (int k = 0; k < NTHR; ++k) { s.wa[k] = 0.0; s.nc[k] = 0; }
    if (a.vec)
      chunk_sum<true, NTHR>(a, (int64_t)a.tb + t0, ch.count, (w + 3) >> 2, lds, s_row, s_a, lane, s);
    else
      chunk_sum<false, NTHR>(a, (int64_t)a.tb + t0, ch.count, w, lds, s_row, s_a, lane, s);
    if (lane < w) {
      const int t = t0 + lane;
      if (ch.slot < 0) {
        if (ch.count == 0) s.h = 0.f;
        store_out<NTHR>(a, ch.zone, a.col0 + t, s);
      } else {
        const Partials& p = a.p;
        const int64_t i = (int64_t)ch.slot * p.S + t;
        p.vol[i] = s.vol;
        p.h[i] = s.h;
        p.q[i] = s.q;
#pragma unroll
        for (int k = 0; k < NTHR; ++k) {
          const int64_t j = ((int64_t)k * p.P + ch.slot) * p.S + t;
          p.area[j] = s.wa[k];
          p.cells[j] = s.nc[k];
        }
      }
    }
  }
}

// The zones of several chunks: thread (zone, step) adds the chunk sums in chunk order.
template <int NTHR>
__global__ __launch_bounds__(256) void k_zone_combine(SeriesArgs a) {
  const Partials& p = a.p;
  const int64_t total = (int64_t)a.nmulti * a.tc;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int mz = (int)(i / a.tc), t = (int)(i - (int64_t)mz * a.tc);
    const Multi m = a.multi[mz];
    Acc<NTHR> s;
    s.vol = 0.0;
    s.h = -INFINITY;
    s.q = 0.f;
#pragma unroll
    for (int k = 0; k < NTHR; ++k) { s.wa[k] = 0.0; s.nc[k] = 0; }
    for (int c = m.first; c < m.first + m.n; ++c) {
      const int64_t j = (int64_t)c * p.S + t;
      s.vol += p.vol[j];
      s.h = fmaxf(s.h, p.h[j]);
      s.q = fmaxf(s.q, p.q[j]);
#pragma unroll
      for (int k = 0; k < NTHR; ++k) {
        const int64_t jk = ((int64_t)k * p.P + c) * p.S + t;
        s.wa[k] += p.area[jk];
        s.nc[k] += p.cells[jk];
      }
    }
    store_out<NTHR>(a, m.zone, a.col0 + t, s);
  }
}

template <int NTHR>
void launch(const SeriesArgs& a, const Launch& l, hipStream_t st) {
  hipLaunchKernelGGL((k_zone_series<NTHR>), dim3(l.grid), dim3(kWave), 0, st, a);
  if (a.nmulti) {
    const int64_t blocks = ((int64_t)a.nmulti * a.tc + 255) / 256;
    hipLaunchKernelGGL((k_zone_combine<NTHR>), dim3((int)std::min<int64_t>(blocks, kGridCap)), dim3(256), 0, st, a);
  }
}

void release(msw_zones* z) {
  if (z->device >= 0) {
    (void)hipSetDevice(z->device);
    (void)hipFree(z->d_rows);
    (void)hipFree(z->d_chunks);
    (void)hipFree(z->d_multi);
    (void)hipFree(z->d_scratch);
  }
  delete z;
}

}  // namespace

extern "C" int msw_zones_create(const int64_t* zone_ptr, const int32_t* zone_rows, int64_t num_zones,
                                int64_t num_rows, int device, msw_zones** out) {
  if (!out) return msw::set_error(MSW_ERR_INVALID, "null argument");
  *out = nullptr;
  if (!zone_ptr) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (num_zones < 0 || num_zones > INT32_MAX || num_rows < 0 || num_rows > INT32_MAX || device < -1)
    return msw::set_error(MSW_ERR_INVALID, "num_zones, num_rows or device out of range");
  if (zone_ptr[0] != 0) return msw::set_error(MSW_ERR_INVALID, "zone_ptr must start at 0");
  for (int64_t z = 0; z < num_zones; ++z)
    if (zone_ptr[z + 1] < zone_ptr[z]) return msw::set_error(MSW_ERR_INVALID, "zone_ptr is not monotone");
  const int64_t M = zone_ptr[num_zones];
  if (M > 0 && !zone_rows) return msw::set_error(MSW_ERR_INVALID, "null argument");
  for (int64_t i = 0; i < M; ++i)
    if (zone_rows[i] < 0 || zone_rows[i] >= num_rows)
      return msw::set_error(MSW_ERR_INVALID, "row id outside [0, num_rows)");

  // the work list: every zone cut into chunks of kChunk list entries
  std::vector<Chunk> chunks;
  std::vector<Multi> multi;
  int64_t slots = 0;
  for (int64_t z = 0; z < num_zones; ++z) {
    const int64_t m = zone_ptr[z + 1] - zone_ptr[z], n = std::max<int64_t>((m + kChunk - 1) / kChunk, 1);
    if (slots + n > INT32_MAX || (int64_t)chunks.size() + n > INT32_MAX)
      return msw::set_error(MSW_ERR_INVALID, "too many list entries");
    if (n > 1) multi.push_back({(int32_t)z, (int32_t)slots, (int32_t)n});
    for (int64_t c = 0; c < n; ++c) {
      const int64_t off = zone_ptr[z] + c * kChunk;
      chunks.push_back({off, (int32_t)std::min<int64_t>(kChunk, zone_ptr[z + 1] - off), (int32_t)z,
                        n > 1 ? (int32_t)(slots + c) : -1});
    }
    if (n > 1) slots += n;
  }
  msw_zones* zs = new msw_zones;
  zs->Z = num_zones;
  zs->num_rows = num_rows;
  zs->nchunks = (int64_t)chunks.size();
  zs->nslots = slots;
  zs->nmulti = (int64_t)multi.size();
  if (slots) {  // as many whole tiles per launch as the scratch budget holds
    const int64_t steps = kScratchBytes / (slots * kSlotBytes) / kTile * kTile;
    zs->S = (int)std::min<int64_t>(std::max<int64_t>(steps, kTile), kMaxSlab);
  }
  if (device >= 0) {
    zs->device = device;
    hipError_t e = hipSetDevice(device);
    auto upload = [&](auto** d, const void* h, size_t bytes) {
      if (e != hipSuccess || !bytes) return;
      e = hipMalloc((void**)d, bytes);
      if (e == hipSuccess && h) e = hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice);
    };
    upload(&zs->d_rows, zone_rows, (size_t)M * sizeof(int32_t));
    upload(&zs->d_chunks, chunks.data(), chunks.size() * sizeof(Chunk));
    upload(&zs->d_multi, multi.data(), multi.size() * sizeof(Multi));
    upload(&zs->d_scratch, nullptr, (size_t)slots * zs->S * kSlotBytes);
    if (e != hipSuccess) {
      release(zs);
      return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
    }
  }
  *out = zs;
  return MSW_OK;
}

extern "C" int msw_zones_destroy(msw_zones* zones) {
  if (zones) release(zones);
  return MSW_OK;
}

extern "C" int msw_zone_series_launch(const msw_zones* zones, int32_t t_count, int32_t* grid, int32_t* units_per_wg,
                                      int32_t* iters) {
  if (!zones || !grid || !units_per_wg || !iters) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (t_count < 0) return msw::set_error(MSW_ERR_INVALID, "t_count negative");
  const Launch l = pick_launch(zones, t_count);
  *grid = l.grid;
  *units_per_wg = 1;  // one wave per workgroup, one unit (chunk x tile) per round of its loop
  *iters = l.iters;
  return MSW_OK;
}

extern "C" int msw_zone_series_update(const msw_zones* zones, const float* pred, int32_t T, int32_t t_begin,
                                      int32_t t_count, const float* area, const float* thresholds, int32_t n_thr,
                                      int32_t T_out, int32_t t_out0, const msw_zone_series* out, void* stream) {
  if (!zones || !pred || !out || (n_thr > 0 && !thresholds)) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n_thr < 0 || n_thr > MSW_MAX_MAP_THRESHOLDS)
    return msw::set_error(MSW_ERR_INVALID, "n_thr out of range (0..4)");
  if (T < 0 || t_begin < 0 || t_count < 0 || (int64_t)t_begin + t_count > T)
    return msw::set_error(MSW_ERR_INVALID, "time window outside [0, T]");
  if (T_out < 0 || t_out0 < 0 || (int64_t)t_out0 + t_count > T_out)
    return msw::set_error(MSW_ERR_INVALID, "output columns outside [0, T_out]");
  if (t_count == 0 || zones->Z == 0) return MSW_OK;
  if (zones->device < 0) return msw::set_error(MSW_ERR_INVALID, "the zone set was created without a device");
  hipStream_t st = (hipStream_t)stream;
  // the threshold loop runs only for a threshold series that is produced
  const int nthr = out->wet_area || out->wet_cells ? n_thr : 0;
  SeriesArgs a{};
  a.pred = pred;
  a.area = area;
  a.rows = zones->d_rows;
  a.chunks = zones->d_chunks;
  a.multi = zones->d_multi;
  a.nchunks = (int)zones->nchunks;
  a.nmulti = (int)zones->nmulti;
  a.T = T;
  a.T_out = T_out;
  a.Z = zones->Z;
  for (int k = 0; k < nthr; ++k) a.thr[k] = thresholds[k];
  a.o = *out;
  Partials& p = a.p;
  p.P = zones->nslots;
  p.S = zones->S;
  const size_t cell = (size_t)p.P * p.S;  // 8-byte arrays first: every array stays aligned
  p.vol = reinterpret_cast<double*>(zones->d_scratch);
  p.area = p.vol + cell;
  p.cells = reinterpret_cast<int32_t*>(p.area + MSW_MAX_MAP_THRESHOLDS * cell);
  p.h = reinterpret_cast<float*>(p.cells + MSW_MAX_MAP_THRESHOLDS * cell);
  p.q = p.h + cell;
  for (int s0 = 0; s0 < t_count; s0 += zones->S) {  // launches on one stream: the scratch is reused in order
    a.tb = t_begin + s0;
    a.tc = std::min<int>(zones->S, t_count - s0);
    a.col0 = t_out0 + s0;
    a.vec = T % 4 == 0 && a.tb % 4 == 0 && reinterpret_cast<uintptr_t>(pred) % 16 == 0;
    const Launch l = pick_launch(zones, a.tc);
    switch (nthr) {
      case 0: launch<0>(a, l, st); break;
      case 1: launch<1>(a, l, st); break;
      case 2: launch<2>(a, l, st); break;
      case 3: launch<3>(a, l, st); break;
      default: launch<4>(a, l, st); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  }
  return MSW_OK;
}
