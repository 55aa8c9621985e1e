// On-device ensemble products: statistics ACROSS the members of an ensemble (one mesh, M boundary
// hydrographs / breaches / initial states), the third sibling of the flood maps (over time,
// floodmaps.hip) and the zone series (over space, series.hip).  Member m occupies rows
// row0[m] .. row0[m] + n - 1 of the rollout [N][2][T]; the list comes by value in the kernel
// arguments and its order is the member order of every sum and tie-break.
//
// k_ensemble_steps (streaming).  One workgroup = one wave.  A round takes R consecutive cells
// (R * t_count ~ 256 floats); a unit is V consecutive steps of one cell, V = 4 (16-byte loads:
// base, T and the window's first step multiples of 16 bytes; the last unit of a cell may reach
// past the window but never past the row's depth half: T is then a multiple of 4) or V = 1.  Lane
// l takes units l, l + 64, ... of the round, consecutive lanes consecutive addresses within a
// cell; per unit it walks the members in order, kBatch loads in flight, and keeps the fp64 sum,
// minimum, maximum and the threshold counts in registers: no LDS, no atomics, no scratch.  Only
// the depth half of a row is addressed.  Stores are consecutive along t (16 bytes per lane where
// the outputs' alignment allows).
//
// k_ensemble_maps (one shot).  One workgroup = one wave, lane = cell, a round = 64 cells.  The
// M values of a cell are loaded member by member (each load one coalesced line of the wave), the
// mean and the exceedance counts taken on the way, and parked in LDS four members to a 16-byte
// word per lane.  The rank of member m is the number of members before it in the stable ascending
// order, counted against all parked values (one compare per pair); the value whose rank is asked
// for is kept as it is.  Steps run through the same code as int32 keys with -1 -> INT_MAX.
// Members go in groups of 16 padded with the largest key: nothing branches on M inside a group.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/mswegnn.h"
#include "engine.h"

namespace {

constexpr int kWave = 64;
constexpr int kGridCap = 4096;     // workgroups: 16 per CU (4 waves per SIMD), each looping over its rounds
constexpr int kRoundFloats = 256;  // window floats of a round: 4 per lane
constexpr int kMaxCells = 64;      // cells of a round at most
constexpr int kBatch = 8;          // members whose loads a lane has in flight before it reduces them
constexpr int kQuads = MSW_MAX_ENSEMBLE_MEMBERS / 4;
constexpr int kGroup = 16;         // k_ensemble_maps: members loaded together, parked and compared together

struct Launch {
  int grid, cells_per_wg, iters;
};

// The launch of a window of tc steps: msw_ensemble_steps_launch reports it, the launcher uses it.
Launch pick_steps_launch(int64_t n, int tc) {
  Launch l{0, 0, 0};
  l.cells_per_wg = std::min(std::max(kRoundFloats / std::max(tc, 1), 1), kMaxCells);
  if (n == 0 || tc == 0) return l;
  const int64_t rounds = (n + l.cells_per_wg - 1) / l.cells_per_wg;
  l.grid = (int)std::min<int64_t>(rounds, kGridCap);
  l.iters = (int)((rounds + l.grid - 1) / l.grid);
  return l;
}

struct StepArgs {
  const float* pred;  // [N][2][T]
  int T, tb, tc;      // window [tb, tb + tc)
  int col0, T_out;    // output column of step tb, leading stride of the outputs
  int64_t n;
  int M;
  int R, L;           // cells of a round, units of a cell
  int ovec;           // 16-byte stores: T_out, col0 and every produced array multiples of 16 bytes
  float thr[MSW_MAX_MAP_THRESHOLDS];
  msw_ensemble_steps_out o;
  int64_t row0[MSW_MAX_ENSEMBLE_MEMBERS];
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int V>
struct Vec;
template <>
struct Vec<1> {
  typedef float type;
  static __device__ __forceinline__ float get(float v, int) { return v; }
};
template <>
struct Vec<4> {
  typedef f32x4 type;
  static __device__ __forceinline__ float get(const f32x4& v, int e) { return v[e]; }
};

// Store w <= V consecutive columns of one output row.
template <int V, typename T>
__device__ __forceinline__ void store_cols(T* dst, const T (&v)[V], int w, bool vec) {
  if constexpr (V == 4) {
    if (vec && w == 4) {
      typedef T t4 __attribute__((ext_vector_type(4)));
      t4 x = {v[0], v[1], v[2], v[3]};
      *reinterpret_cast<t4*>(dst) = x;
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e)
    if (e < w) dst[e] = v[e];
}

template <int V, int NTHR>
__global__ __launch_bounds__(kWave) void k_ensemble_steps(StepArgs a) {
  typedef typename Vec<V>::type vec_t;
  const int lane = threadIdx.x;
  const int64_t rounds = (a.n + a.R - 1) / a.R;
  const float fM = (float)a.M;
  const double dM = (double)fM;  // M <= 64: exact
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t base = rb * a.R;
    const int units = (int)min<int64_t>(a.R, a.n - base) * a.L;
    for (int u = lane; u < units; u += kWave) {
      const int r = u / a.L, t = (u - r * a.L) * V;  // cell of the round, first column of the unit
      const int64_t cell = base + r;
      const int w = min(V, a.tc - t);
      const float* p = a.pred + cell * 2 * a.T + a.tb + t;  // member m: + row0[m] * 2 T
      double sum[V];
      float mn[V], mx[V];
      int cnt[NTHR > 0 ? NTHR : 1][V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        sum[e] = 0.0;
        mn[e] = INFINITY;
        mx[e] = -INFINITY;
#pragma unroll
        for (int k = 0; k < NTHR; ++k) cnt[k][e] = 0;
      }
      for (int m0 = 0; m0 < a.M; m0 += kBatch) {  // uniform
        vec_t v[kBatch];
#pragma unroll
        for (int j = 0; j < kBatch; ++j)
          if (m0 + j < a.M)
            v[j] = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(p + a.row0[m0 + j] * 2 * a.T));
#pragma unroll
        for (int j = 0; j < kBatch; ++j) {
          if (m0 + j < a.M) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
              const float h = Vec<V>::get(v[j], e);
              sum[e] += (double)h;
              mn[e] = h < mn[e] ? h : mn[e];
              mx[e] = h > mx[e] ? h : mx[e];
#pragma unroll
              for (int k = 0; k < NTHR; ++k) cnt[k][e] += h > a.thr[k] ? 1 : 0;
            }
          }
        }
      }
      const int64_t i = cell * a.T_out + a.col0 + t;
      if (a.o.h_mean) {
        float mean[V];
#pragma unroll
        for (int e = 0; e < V; ++e) mean[e] = (float)(sum[e] / dM);
        store_cols<V>(a.o.h_mean + i, mean, w, a.ovec);
      }
      if (a.o.h_min) store_cols<V>(a.o.h_min + i, mn, w, a.ovec);
      if (a.o.h_max) store_cols<V>(a.o.h_max + i, mx, w, a.ovec);
      if constexpr (NTHR > 0) {
#pragma unroll
        for (int k = 0; k < NTHR; ++k)
          store_cols<V>(a.o.wet_members + (int64_t)k * a.n * a.T_out + i, cnt[k], w, a.ovec);
      }
    }
  }
}

template <int V>
void launch_steps(const StepArgs& a, int nthr, int grid, hipStream_t st) {
  switch (nthr) {
    case 0: hipLaunchKernelGGL((k_ensemble_steps<V, 0>), dim3(grid), dim3(kWave), 0, st, a); break;
    case 1: hipLaunchKernelGGL((k_ensemble_steps<V, 1>), dim3(grid), dim3(kWave), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_ensemble_steps<V, 2>), dim3(grid), dim3(kWave), 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_ensemble_steps<V, 3>), dim3(grid), dim3(kWave), 0, st, a); break;
    default: hipLaunchKernelGGL((k_ensemble_steps<V, 4>), dim3(grid), dim3(kWave), 0, st, a); break;
  }
}

// ---------------------------------------------------------------------------- order statistics
struct MapsArgs {
  const float* values;   // [M][n] or NULL
  const int32_t* steps;  // [M][n] or NULL
  int64_t n;
  int M, nranks;
  float thr[MSW_MAX_MAP_THRESHOLDS];
  int ranks[MSW_MAX_ENSEMBLE_RANKS];
  msw_ensemble_maps_out o;
};

__device__ __forceinline__ unsigned bits(float v) { return __float_as_uint(v); }
__device__ __forceinline__ unsigned bits(int v) { return (unsigned)v; }
template <typename K>
__device__ __forceinline__ K unbits(unsigned v);
template <>
__device__ __forceinline__ float unbits<float>(unsigned v) { return __uint_as_float(v); }
template <>
__device__ __forceinline__ int unbits<int>(unsigned v) { return (int)v; }

// Member m of this lane's cell sits in word m & 3 of the lane's 16-byte word of quad m >> 2.  A
// lane reads only the words it wrote itself, so the wave needs no barrier around them.
__device__ __forceinline__ int slot(int m, int lane) { return (((m >> 2) * kWave + lane) << 2) + (m & 3); }

// The parked keys whose ranks are a.ranks[0 .. nranks): member m's rank is the number of members
// m' with key' < key, or key' == key and m' < m -- counted as key' <= key over the members before
// m and key' < key from m on (a uniform choice per member: one compare each, no branch).  The
// members past M up to the group's end hold the largest key: never below a key.
template <typename K>
__device__ __forceinline__ void select(const MapsArgs& a, const unsigned* lds, int lane,
                                       K (&out)[MSW_MAX_ENSEMBLE_RANKS]) {
  const int G = (a.M + kGroup - 1) / kGroup;
  for (int m = 0; m < a.M; ++m) {  // uniform
    const K vm = unbits<K>(lds[slot(m, lane)]);
    int cnt = 0;
    for (int g = 0; g < G; ++g) {
      u32x4 w[kGroup / 4];  // the group's four LDS reads in flight at once
#pragma unroll
      for (int i = 0; i < kGroup / 4; ++i)
        w[i] = *reinterpret_cast<const u32x4*>(lds + (((g * (kGroup / 4) + i) * kWave + lane) << 2));
#pragma unroll
      for (int i = 0; i < kGroup / 4; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const K v = unbits<K>(w[i][e]);
          const bool before = g * kGroup + 4 * i + e < m;
          cnt += (before ? v <= vm : v < vm) ? 1 : 0;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < MSW_MAX_ENSEMBLE_RANKS; ++j) out[j] = j < a.nranks && cnt == a.ranks[j] ? vm : out[j];
  }
}

template <int NTHR>
__global__ __launch_bounds__(kWave) void k_ensemble_maps(MapsArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned lds[kQuads * kWave * 4];  // 16 KiB
  const int lane = threadIdx.x;
  const int64_t rounds = (a.n + kWave - 1) / kWave;
  const double dM = (double)(float)a.M;
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t i = rb * kWave + lane;
    const bool live = i < a.n;
    const int64_t ic = live ? i : a.n - 1;  // a lane past the end repeats the last cell and stores nothing
    // A group's loads go out together; a member past M repeats the last one's load and parks the
    // largest key, so that nothing below branches on the member count.
    if (a.values) {
      double sum = 0.0;
      int cnt[NTHR > 0 ? NTHR : 1];
#pragma unroll
      for (int k = 0; k < NTHR; ++k) cnt[k] = 0;
      for (int m0 = 0; m0 < a.M; m0 += kGroup) {
        float v[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j)
          v[j] = __builtin_nontemporal_load(a.values + (int64_t)min(m0 + j, a.M - 1) * a.n + ic);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
          const bool member = m0 + j < a.M;
          sum += member ? (double)v[j] : 0.0;
#pragma unroll
          for (int k = 0; k < NTHR; ++k) cnt[k] += member && v[j] > a.thr[k] ? 1 : 0;
          lds[slot(m0 + j, lane)] = bits(member ? v[j] : INFINITY);
        }
      }
      float rv[MSW_MAX_ENSEMBLE_RANKS];
#pragma unroll
      for (int j = 0; j < MSW_MAX_ENSEMBLE_RANKS; ++j) rv[j] = 0.f;
      if (a.o.rank_values) select<float>(a, lds, lane, rv);
      if (live) {
        if (a.o.mean) a.o.mean[i] = (float)(sum / dM);
        if constexpr (NTHR > 0) {
#pragma unroll
          for (int k = 0; k < NTHR; ++k) a.o.exceed_members[(int64_t)k * a.n + i] = cnt[k];
        }
        if (a.o.rank_values) {
#pragma unroll
          for (int j = 0; j < MSW_MAX_ENSEMBLE_RANKS; ++j)
            if (j < a.nranks) a.o.rank_values[(int64_t)j * a.n + i] = rv[j];
        }
      }
    }
    if (a.steps) {
      int with = 0;
      for (int m0 = 0; m0 < a.M; m0 += kGroup) {
        int s[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j)
          s[j] = __builtin_nontemporal_load(a.steps + (int64_t)min(m0 + j, a.M - 1) * a.n + ic);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
          const bool member = m0 + j < a.M;
          with += member && s[j] >= 0 ? 1 : 0;
          lds[slot(m0 + j, lane)] = bits(member && s[j] >= 0 ? s[j] : INT_MAX);  // never: after every step
        }
      }
      int rs[MSW_MAX_ENSEMBLE_RANKS];
#pragma unroll
      for (int j = 0; j < MSW_MAX_ENSEMBLE_RANKS; ++j) rs[j] = 0;
      if (a.o.rank_steps) select<int>(a, lds, lane, rs);
      if (live) {
        if (a.o.members_with_step) a.o.members_with_step[i] = with;
        if (a.o.rank_steps) {
#pragma unroll
          for (int j = 0; j < MSW_MAX_ENSEMBLE_RANKS; ++j)
            if (j < a.nranks) a.o.rank_steps[(int64_t)j * a.n + i] = rs[j] == INT_MAX ? -1 : rs[j];
        }
      }
    }
  }
}

int check_common(const float* thresholds, int n_thr, int M, int64_t n) {
  if (n_thr > 0 && !thresholds) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n_thr < 0 || n_thr > MSW_MAX_MAP_THRESHOLDS)
    return msw::set_error(MSW_ERR_INVALID, "n_thr out of range (0..4)");
  if (M < 1 || M > MSW_MAX_ENSEMBLE_MEMBERS)
    return msw::set_error(MSW_ERR_INVALID, "M out of range (1..64)");
  if (n < 0) return msw::set_error(MSW_ERR_INVALID, "n negative");
  return MSW_OK;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int msw_ensemble_steps_launch(int64_t n, int32_t M, int32_t t_count, int32_t* grid, int32_t* cells_per_wg,
                                         int32_t* iters) {
  if (!grid || !cells_per_wg || !iters) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n < 0 || t_count < 0) return msw::set_error(MSW_ERR_INVALID, "n or t_count negative");
  if (M < 1 || M > MSW_MAX_ENSEMBLE_MEMBERS) return msw::set_error(MSW_ERR_INVALID, "M out of range (1..64)");
  const Launch l = pick_steps_launch(n, t_count);
  *grid = l.grid;
  *cells_per_wg = l.cells_per_wg;
  *iters = l.iters;
  return MSW_OK;
}

extern "C" int msw_ensemble_steps_update(const float* pred, int32_t T, int32_t t_begin, int32_t t_count,
                                         const int64_t* member_row0, int32_t M, int64_t n, const float* thresholds,
                                         int32_t n_thr, int32_t T_out, int32_t t_out0,
                                         const msw_ensemble_steps_out* out, void* stream) {
  if (!pred || !out || !member_row0) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (const int rc = check_common(thresholds, n_thr, M, n)) return rc;
  if (T < 0 || t_begin < 0 || t_count < 0 || (int64_t)t_begin + t_count > T)
    return msw::set_error(MSW_ERR_INVALID, "time window outside [0, T]");
  if (T_out < 0 || t_out0 < 0 || (int64_t)t_out0 + t_count > T_out)
    return msw::set_error(MSW_ERR_INVALID, "output columns outside [0, T_out]");
  for (int m = 0; m < M; ++m)
    if (member_row0[m] < 0) return msw::set_error(MSW_ERR_INVALID, "member_row0 negative");
  if (t_count == 0 || n == 0) return MSW_OK;
  // the threshold loop runs only when its output is produced
  const int nthr = out->wet_members ? n_thr : 0;
  if (!nthr && !out->h_mean && !out->h_min && !out->h_max) return MSW_OK;
  StepArgs a{};
  a.pred = pred;
  a.T = T;
  a.tb = t_begin;
  a.tc = t_count;
  a.col0 = t_out0;
  a.T_out = T_out;
  a.n = n;
  a.M = M;
  for (int k = 0; k < nthr; ++k) a.thr[k] = thresholds[k];
  a.o = *out;
  if (!nthr) a.o.wet_members = nullptr;
  for (int m = 0; m < M; ++m) a.row0[m] = member_row0[m];
  const Launch l = pick_steps_launch(n, t_count);
  const bool vec = T % 4 == 0 && t_begin % 4 == 0 && aligned16(pred);
  a.R = l.cells_per_wg;
  a.L = vec ? (t_count + 3) >> 2 : t_count;
  a.ovec = T_out % 4 == 0 && t_out0 % 4 == 0 && aligned16(a.o.wet_members) && aligned16(a.o.h_mean) &&
           aligned16(a.o.h_min) && aligned16(a.o.h_max);
  if (vec)
    launch_steps<4>(a, nthr, l.grid, (hipStream_t)stream);
  else
    launch_steps<1>(a, nthr, l.grid, (hipStream_t)stream);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  return MSW_OK;
}

extern "C" int msw_ensemble_maps(const float* values, const int32_t* steps, int32_t M, int64_t n,
                                 const float* thresholds, int32_t n_thr, const int32_t* ranks, int32_t n_ranks,
                                 const msw_ensemble_maps_out* out, void* stream) {
  if (!out || (n_ranks > 0 && !ranks)) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (const int rc = check_common(thresholds, n_thr, M, n)) return rc;
  if (n_ranks < 0 || n_ranks > MSW_MAX_ENSEMBLE_RANKS)
    return msw::set_error(MSW_ERR_INVALID, "n_ranks out of range (0..8)");
  for (int j = 0; j < n_ranks; ++j)
    if (ranks[j] < 0 || ranks[j] >= M) return msw::set_error(MSW_ERR_INVALID, "rank outside [0, M)");
  if (n == 0) return MSW_OK;
  MapsArgs a{};
  a.n = n;
  a.M = M;
  a.nranks = n_ranks;
  a.o = *out;
  const int nthr = values && a.o.exceed_members ? n_thr : 0;
  if (!nthr) a.o.exceed_members = nullptr;
  if (!n_ranks) a.o.rank_values = nullptr, a.o.rank_steps = nullptr;
  // an input none of whose outputs is produced is not read
  a.values = nthr || a.o.mean || a.o.rank_values ? values : nullptr;
  a.steps = a.o.members_with_step || a.o.rank_steps ? steps : nullptr;
  if (!a.values && !a.steps) return MSW_OK;
  for (int k = 0; k < nthr; ++k) a.thr[k] = thresholds[k];
  for (int j = 0; j < n_ranks; ++j) a.ranks[j] = ranks[j];
  const int grid = (int)std::min<int64_t>((n + kWave - 1) / kWave, kGridCap);
  hipStream_t st = (hipStream_t)stream;
  switch (nthr) {
    case 0: hipLaunchKernelGGL((k_ensemble_maps<0>), dim3(grid), dim3(kWave), 0, st, a); break;
    case 1: hipLaunchKernelGGL((k_ensemble_maps<1>), dim3(grid), dim3(kWave), 0, st, a); break;
    case 2: hipLaunchKernelGGL((k_ensemble_maps<2>), dim3(grid), dim3(kWave), 0, st, a); break;
    case 3: hipLaunchKernelGGL((k_ensemble_maps<3>), dim3(grid), dim3(kWave), 0, st, a); break;
    default: hipLaunchKernelGGL((k_ensemble_maps<4>), dim3(grid), dim3(kWave), 0, st, a); break;
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  return MSW_OK;
}
