// On-device flood maps: a rollout [N][2][T] reduced over time into per-cell hazard maps, where
// the rollout already lives.  What the reference builds on the host after a rollout:
//   flood-arrival time   WD_to_FAT                  utils/miscellaneous.py:56-68
//                        (counts the steps with h > thr; used at utils/visualization.py:672-673)
//   peak depth, discharge                           utils/visualization.py:592-598
//   velocity, Froude     get_velocity / get_Froude  utils/miscellaneous.py:44-54
//                        (used at utils/visualization.py:864-867)
// plus the first / last wet step per threshold and the step of each peak.  Every rollout value is
// read once; the maps carry over between calls, so a rollout can be fed piece by piece
// (mswegnn/floodmaps.py rollout_flood_maps) without ever being held whole.
//
// One workgroup = one wave.  A round takes R consecutive rows: with the whole [0, T) window they
// are ONE run of 2 T R floats in memory, copied to LDS with 16-byte loads (lane i at base + 16 i);
// the rows then sit in LDS at an odd pitch (2 tc + 1 words), and the 64 lanes reduce them as
// R rows x 64 / R consecutive time parts (lane = part * R + row: a half-wave reads one column of
// consecutive rows, conflict-free at the odd pitch).  The parts are merged in time order with
// shuffles, lanes 0..R-1 merge the carried-over state and store one coalesced line per map.
// Windows, odd T or a misaligned base take the scalar loader: lanes along the flattened
// (row, variable, step) index of the window, still consecutive addresses within a row.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/mswegnn.h"
#include "engine.h"

namespace {

constexpr int kWave = 64;
constexpr int kMaxRows = 32;      // rows of a round: at least two time parts per row
constexpr int kLdsFloats = 2112;  // staged rows of one round: R * (2 tc + 1) <= kLdsFloats (8.25 KiB):
                                  // LDS leaves room for 19 one-wave workgroups per CU, registers for 7 waves per SIMD
constexpr int kMaxTc = 1024;      // steps per launch (R = 1); longer windows run as carried-over slabs
constexpr int kGridCap = 4096;    // workgroups: 16 per CU (4 waves per SIMD), each looping over its rounds
constexpr int kLoadBatch = 8;     // loads a lane has in flight before it stores them to LDS
constexpr int kStepBatch = 4;     // steps whose LDS reads a lane issues before it reduces them
constexpr int kNoStep = INT_MAX;  // first_wet inside the kernel while the row has not been wet (-1 in memory)

struct Launch {
  int grid, rows_per_wg, iters;
};

// The launch of one slab of tc <= kMaxTc steps: msw_flood_maps_launch reports it, the launcher uses it.
Launch pick_launch(int64_t nrows, int tc) {
  Launch l{0, kMaxRows, 0};
  tc = std::min(std::max(tc, 1), kMaxTc);
  while (l.rows_per_wg > 1 && l.rows_per_wg * (2 * tc + 1) > kLdsFloats) l.rows_per_wg >>= 1;
  const int64_t rounds = (nrows + l.rows_per_wg - 1) / l.rows_per_wg;
  l.grid = (int)std::min<int64_t>(rounds, kGridCap);
  l.iters = l.grid ? (int)((rounds + l.grid - 1) / l.grid) : 0;
  return l;
}

struct MapArgs {
  const float* pred;  // [N][2][T]
  int T, tb, tc;      // window [tb, tb + tc) of this launch
  int t_off;          // global step of column tb
  int64_t row0, nrows;
  int R, log2R;
  int vec;  // 16-byte loader: whole window, even T, 16-byte aligned first row
  // loader constants (units of `vec ? 4 : 1` floats, 64 units per pass): segment length, the
  // segments' stride and offset in memory, the advance of (segment, column) per pass
  int L, gstride, goff, qs, rs;
  int first;
  float vel_eps;
  float thr[MSW_MAX_MAP_THRESHOLDS];
  msw_flood_maps m;
};

template <int NTHR>
struct State {
  float h, q, vel, fr;
  int th, tq;
  int cnt[NTHR > 0 ? NTHR : 1], fst[NTHR > 0 ? NTHR : 1], lst[NTHR > 0 ? NTHR : 1];
};

// `late` follows `s` in time: a maximum moves only to a strictly larger value (the earliest step
// keeps a tie), first_wet keeps the earlier step, last_wet and wet_steps advance.
template <bool VEL, int NTHR>
__device__ __forceinline__ void merge(State<NTHR>& s, const State<NTHR>& late) {
  if (late.h > s.h) { s.h = late.h; s.th = late.th; }
  if (late.q > s.q) { s.q = late.q; s.tq = late.tq; }
  if constexpr (VEL) {
    s.vel = late.vel > s.vel ? late.vel : s.vel;
    s.fr = late.fr > s.fr ? late.fr : s.fr;
  }
#pragma unroll
  for (int k = 0; k < NTHR; ++k) {
    s.cnt[k] += late.cnt[k];
    s.fst[k] = min(s.fst[k], late.fst[k]);
    s.lst[k] = max(s.lst[k], late.lst[k]);
  }
}

// One (row, step) into the running state of its part.
template <bool VEL, int NTHR>
__device__ __forceinline__ void step(State<NTHR>& s, float h, float q, int t, const MapArgs& a) {
  if (h > s.h) { s.h = h; s.th = t; }
  if (q > s.q) { s.q = q; s.tq = t; }
  if constexpr (VEL) {
    // get_velocity: q / h, 0 where h <= eps; get_Froude: vel / sqrt(g h), 0 where h <= 0.
    // Where vel is 0 and h > 0 the Froude number is 0 / sqrt(g h) = 0: no division needed.
    float vel = 0.f, fr = 0.f;
    if (h > a.vel_eps) {
      vel = q / h;
      fr = h > 0.f ? vel / sqrtf(9.81f * h) : 0.f;
    }
    s.vel = vel > s.vel ? vel : s.vel;
    s.fr = fr > s.fr ? fr : s.fr;
  }
#pragma unroll
  for (int k = 0; k < NTHR; ++k) {
    const bool wet = h > a.thr[k];
    s.cnt[k] += wet ? 1 : 0;
    s.fst[k] = min(s.fst[k], wet ? t : kNoStep);
    s.lst[k] = wet ? t : s.lst[k];
  }
}

// Copy the round's nseg segments to LDS.  Unit u = lane, lane + 64, ... is V floats at flattened
// index u V = (segment, column); (segment, column) advance by (qs, rs) per pass without a division.
template <int V>
__device__ __forceinline__ void stage(const MapArgs& a, const float* __restrict__ g, float* lds, int nseg, int lane) {
  const int sh = V == 4 ? 0 : 1;  // V = 4: a segment is a row (pitch L + 1); else (row, variable): one pad word per 2
  int seg = (lane * V) / a.L, c = lane * V - seg * a.L;
  while (seg < nseg) {
    int s[kLoadBatch], cc[kLoadBatch];
    float v[kLoadBatch][V];
#pragma unroll
    for (int i = 0; i < kLoadBatch; ++i) {
      s[i] = seg;
      cc[i] = c;
      c += a.rs;
      seg += a.qs;
      if (c >= a.L) { c -= a.L; ++seg; }
    }
#pragma unroll
    for (int i = 0; i < kLoadBatch; ++i) {
      if (s[i] < nseg) {
        const float* p = g + (size_t)s[i] * a.gstride + a.goff + cc[i];
        if constexpr (V == 4) {
          typedef float f32x4 __attribute__((ext_vector_type(4)));
          const f32x4 w = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
          v[i][0] = w.x; v[i][1] = w.y; v[i][2] = w.z; v[i][3] = w.w;
        } else {
          v[i][0] = __builtin_nontemporal_load(p);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kLoadBatch; ++i) {
      if (s[i] < nseg) {
        float* d = lds + s[i] * a.L + (s[i] >> sh) + cc[i];
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = v[i][j];
      }
    }
  }
}

template <bool VEL, int NTHR>
__global__ __launch_bounds__(kWave) void k_flood_maps(MapArgs a) {
  extern __shared__ float lds[];
  const int lane = threadIdx.x;
  const int R = a.R, tc = a.tc, pitch = 2 * tc + 1;
  const int r = lane & (R - 1), part = lane >> a.log2R;
  const int tp = (tc + (kWave >> a.log2R) - 1) >> (6 - a.log2R);  // steps per part
  const int i0 = min(part * tp, tc), i1 = min(i0 + tp, tc);
  const int64_t rounds = (a.nrows + R - 1) / R;
  for (int64_t rb = blockIdx.x; rb < rounds; rb += gridDim.x) {  // uniform per workgroup
    const int64_t base = rb * R;
    const int nr = (int)min<int64_t>(R, a.nrows - base);
    const float* g = a.pred + (size_t)(a.row0 + base) * 2 * a.T;
    if (a.vec)
      stage<4>(a, g, lds, nr, lane);
    else
      stage<1>(a, g, lds, 2 * nr, lane);
    __syncthreads();

    State<NTHR> s;
    s.h = s.q = s.vel = s.fr = -INFINITY;
    s.th = s.tq = 0;
#pragma unroll
    for (int k = 0; k < NTHR; ++k) { s.cnt[k] = 0; s.fst[k] = kNoStep; s.lst[k] = -1; }
    if (r < nr) {
      const float* row = lds + r * pitch;
      for (int i = i0; i < i1; i += kStepBatch) {  // kStepBatch steps' LDS reads in flight at once
        float hv[kStepBatch], qv[kStepBatch];
#pragma unroll
        for (int j = 0; j < kStepBatch; ++j) {
          const int ii = min(i + j, i1 - 1);
          hv[j] = row[ii];
          qv[j] = fabsf(row[tc + ii]);
        }
#pragma unroll
        for (int j = 0; j < kStepBatch; ++j)
          if (i + j < i1) step<VEL, NTHR>(s, hv[j], qv[j], a.t_off + i + j, a);
      }
    }
    __syncthreads();  // the rows are consumed: the next round may overwrite them

    // the parts of a row sit R lanes apart; the lower lane of a pair holds the earlier steps
    for (int off = R; off < kWave; off <<= 1) {
      State<NTHR> o = s;
      o.h = __shfl_xor(s.h, off); o.th = __shfl_xor(s.th, off);
      o.q = __shfl_xor(s.q, off); o.tq = __shfl_xor(s.tq, off);
      if constexpr (VEL) { o.vel = __shfl_xor(s.vel, off); o.fr = __shfl_xor(s.fr, off); }
#pragma unroll
      for (int k = 0; k < NTHR; ++k) {
        o.cnt[k] = __shfl_xor(s.cnt[k], off);
        o.fst[k] = __shfl_xor(s.fst[k], off);
        o.lst[k] = __shfl_xor(s.lst[k], off);
      }
      if (lane & off) {
        State<NTHR> e = o;
        merge<VEL, NTHR>(e, s);
        s = e;
      } else {
        merge<VEL, NTHR>(s, o);
      }
    }

    if (lane < nr) {  // lanes 0..R-1 are part 0 of rows 0..R-1
      const int64_t n = base + lane;
      const msw_flood_maps& m = a.m;
      if (!a.first) {
        State<NTHR> e = s;
        // a maximum whose array is not produced is not carried: -inf lets this call's value through
        e.h = m.h_max ? m.h_max[n] : -INFINITY;
        e.th = m.t_h_max ? m.t_h_max[n] : 0;
        e.q = m.q_max ? m.q_max[n] : -INFINITY;
        e.tq = m.t_q_max ? m.t_q_max[n] : 0;
        e.vel = VEL && m.vel_max ? m.vel_max[n] : -INFINITY;
        e.fr = VEL && m.froude_max ? m.froude_max[n] : -INFINITY;
#pragma unroll
        for (int k = 0; k < NTHR; ++k) {
          const int64_t j = (int64_t)k * a.nrows + n;
          e.cnt[k] = m.wet_steps ? m.wet_steps[j] : 0;
          const int f = m.first_wet ? m.first_wet[j] : -1;
          e.fst[k] = f < 0 ? kNoStep : f;
          e.lst[k] = m.last_wet ? m.last_wet[j] : -1;
        }
        merge<VEL, NTHR>(e, s);
        s = e;
      }
      if (m.h_max) m.h_max[n] = s.h;
      if (m.t_h_max) m.t_h_max[n] = s.th;
      if (m.q_max) m.q_max[n] = s.q;
      if (m.t_q_max) m.t_q_max[n] = s.tq;
      if constexpr (VEL) {
        if (m.vel_max) m.vel_max[n] = s.vel;
        if (m.froude_max) m.froude_max[n] = s.fr;
      }
#pragma unroll
      for (int k = 0; k < NTHR; ++k) {
        const int64_t j = (int64_t)k * a.nrows + n;
        if (m.wet_steps) m.wet_steps[j] = s.cnt[k];
        if (m.first_wet) m.first_wet[j] = s.fst[k] == kNoStep ? -1 : s.fst[k];
        if (m.last_wet) m.last_wet[j] = s.lst[k];
      }
    }
  }
}

template <bool VEL>
void launch_nthr(const MapArgs& a, int nthr, dim3 grid, size_t lds, hipStream_t st) {
  switch (nthr) {
    case 0: hipLaunchKernelGGL((k_flood_maps<VEL, 0>), grid, dim3(kWave), lds, st, a); break;
    case 1: hipLaunchKernelGGL((k_flood_maps<VEL, 1>), grid, dim3(kWave), lds, st, a); break;
    case 2: hipLaunchKernelGGL((k_flood_maps<VEL, 2>), grid, dim3(kWave), lds, st, a); break;
    case 3: hipLaunchKernelGGL((k_flood_maps<VEL, 3>), grid, dim3(kWave), lds, st, a); break;
    default: hipLaunchKernelGGL((k_flood_maps<VEL, 4>), grid, dim3(kWave), lds, st, a); break;
  }
}

}  // namespace

extern "C" int msw_flood_maps_launch(int64_t nrows, int32_t t_count, int32_t* grid, int32_t* rows_per_wg,
                                     int32_t* iters) {
  if (!grid || !rows_per_wg || !iters) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (nrows < 0 || t_count < 0) return msw::set_error(MSW_ERR_INVALID, "nrows or t_count negative");
  const Launch l = pick_launch(t_count ? nrows : 0, t_count);
  *grid = l.grid;
  *rows_per_wg = l.rows_per_wg;
  *iters = l.iters;
  return MSW_OK;
}

extern "C" int msw_flood_maps_update(const float* pred, int32_t T, int32_t t_begin, int32_t t_count,
                                     int32_t t_offset, int64_t row0, int64_t nrows, const float* thresholds,
                                     int32_t n_thr, float vel_eps, int32_t first, const msw_flood_maps* maps,
                                     void* stream) {
  if (!pred || !maps || (n_thr > 0 && !thresholds)) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n_thr < 0 || n_thr > MSW_MAX_MAP_THRESHOLDS)
    return msw::set_error(MSW_ERR_INVALID, "n_thr out of range (0..4)");
  if (T < 0 || t_begin < 0 || t_count < 0 || (int64_t)t_begin + t_count > T)
    return msw::set_error(MSW_ERR_INVALID, "time window outside [0, T]");
  if (row0 < 0 || nrows < 0) return msw::set_error(MSW_ERR_INVALID, "row0 or nrows negative");
  if (t_count == 0 || nrows == 0) return MSW_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool vel = maps->vel_max || maps->froude_max;
  // the threshold loop runs only for a threshold map that is produced
  const int nthr = maps->wet_steps || maps->first_wet || maps->last_wet ? n_thr : 0;
  for (int s0 = 0; s0 < t_count; s0 += kMaxTc) {  // slabs after the first continue the maps
    MapArgs a{};
    a.pred = pred;
    a.T = T;
    a.tb = t_begin + s0;
    a.tc = std::min<int>(kMaxTc, t_count - s0);
    a.t_off = t_offset + s0;
    a.row0 = row0;
    a.nrows = nrows;
    const Launch l = pick_launch(nrows, a.tc);
    a.R = l.rows_per_wg;
    while ((1 << a.log2R) < a.R) ++a.log2R;
    a.vec = a.tb == 0 && a.tc == T && T % 2 == 0 &&
            reinterpret_cast<uintptr_t>(pred + (size_t)row0 * 2 * T) % 16 == 0;
    a.L = a.vec ? 2 * T : a.tc;
    a.gstride = a.vec ? 2 * T : T;
    a.goff = a.vec ? 0 : a.tb;
    const int pass = kWave * (a.vec ? 4 : 1);  // floats per pass of the wave
    a.qs = pass / a.L;
    a.rs = pass % a.L;
    a.first = first && s0 == 0;
    a.vel_eps = vel_eps;
    for (int k = 0; k < nthr; ++k) a.thr[k] = thresholds[k];
    a.m = *maps;
    const size_t lds = (size_t)a.R * (2 * a.tc + 1) * sizeof(float);
    if (vel)
      launch_nthr<true>(a, nthr, dim3(l.grid), lds, st);
    else
      launch_nthr<false>(a, nthr, dim3(l.grid), lds, st);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  }
  return MSW_OK;
}
