// On-device ensemble scores: an ensemble (ensemble.hip: M members of one mesh, member m at rows
// row0[m] .. row0[m] + n - 1 of the rollout [N][2][T]) verified against a truth run -- the CRPS, the
// reliability table behind the Brier score, and spread against skill.  Per cell and step, in fp64
// on the converted float32 depths h_m and the truth y:
//   a = sum_m |h_m - y|                              S = sum_m h_m     e = S - M y
//   b = sum_{m<m'} |h_m - h_m'|                      v = M sum_m h_m^2 - S^2
//     = sum_m (2 rank_m - M + 1) h_m, rank_m the 0-based place of member m in the stable ascending
//       order, counted as k_ensemble_maps counts it (the integer coefficient times a float32 is
//       exact in fp64)
//   c_k = #{m : h_m > thr_k} (strict, float32)       o_k = y > thr_k
// The kernel never divides: sums[t] = sum over cells of (a, b, |e|, e^2, v); reliability[t][k][c]
// = (cells with c_k = c, those of them with o_k); cell_crps[cell] += M a - b, one addition per
// step in step order onto the carried value.  A NaN depth makes the five terms of its (cell, step)
// NaN and counts as "not above".
//
// Order of the additions.  The cells are cut into blocks of cpb consecutive cells, cpb a function
// of n alone (pick_launch).  A block's cells are added in cell order from 0 into the block's
// partial, a second kernel adds the partials in block order: the order depends on n alone -- not
// on the window, its tiling or how a rollout was cut into calls.  No atomics.
//
// k_ensemble_scores.  One workgroup = one wave = one block of cells; the window is cut into tiles
// of W <= 64 steps, walked in order.  A round takes G = 64 / W cells of the block: lane = (cell
// r, step t) with t fastest, consecutive lanes consecutive addresses.  A lane loads its M depths
// member by member (16 loads in flight), takes a, S, the squares and the counts on the way and
// parks the depths in LDS four members to a 16-byte word per lane (the slot layout of
// k_ensemble_maps: a lane reads only what it wrote); the ranks are counted against all parked
// values.  The lane's six terms and its packed counts go to LDS, and then lane t adds the round's
// cells of step t in cell order into its registers and into its own rows of the tile's table in
// LDS (no other lane touches them), and lane r adds the tile's steps of cell r in step order onto
// cell_crps.  After a tile's rounds the sums and the table go to the block's partials.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>

#include "../../include/mswegnn.h"
#include "engine.h"

namespace {

constexpr int kWave = 64;
constexpr int kGroup = 16;            // members loaded together, parked and compared together
constexpr int kSums = 5;              // a, b, |e|, e^2, v
constexpr int kTerms = kSums + 1;     // ... and M a - b
constexpr int kMinBlock = 16;         // cells of a block at least, and the step of its growth
constexpr int kMaxBlock = 32768;      // ... at most: a block's table counts stay below 2^16
constexpr int kBlocks = 2048;         // blocks at most while a block stays within kMaxBlock
constexpr int kTableWords = 4096;     // LDS words of a tile's table: 16 KiB
constexpr int kThreads = 256;         // k_scores_combine

struct Launch {
  int64_t nblocks;
  int cpb, W, ntiles, G, iters;
};

// The launch of a window of tc steps: msw_ensemble_scores_launch reports it, the launcher uses it.
// The blocks depend on n alone; the tile width on M (the table of a tile of W steps, at the
// largest number of thresholds, must fit its LDS) and on the window.
Launch pick_launch(int64_t n, int M, int tc) {
  Launch l{0, kMinBlock, 1, 0, kWave, 0};
  const int64_t grown = (n + (int64_t)kMinBlock * kBlocks - 1) / ((int64_t)kMinBlock * kBlocks) * kMinBlock;
  l.cpb = (int)std::min<int64_t>(std::max<int64_t>(grown, kMinBlock), kMaxBlock);
  l.nblocks = (n + l.cpb - 1) / l.cpb;
  if (n == 0 || tc == 0) return l;
  const int wmax = std::min(kWave, kTableWords / (MSW_MAX_MAP_THRESHOLDS * (M + 1)));
  l.ntiles = (tc + wmax - 1) / wmax;
  l.W = (tc + l.ntiles - 1) / l.ntiles;
  l.G = kWave / l.W;
  l.iters = (int)((std::min<int64_t>(l.cpb, n) + l.G - 1) / l.G);
  return l;
}

struct ScoreArgs {
  const float* pred;   // [N][2][T]
  const float* truth;  // [*][2][Tt]
  int T, tb, tc;       // window [tb, tb + tc)
  int Tt, tt0;         // the truth's leading stride and its column of step tb
  int64_t trow0;       // the truth's row of cell 0
  int64_t n;
  int M, cpb, W;
  int need_b;          // sums or cell_crps are produced: the ranks are counted
  float thr[MSW_MAX_MAP_THRESHOLDS];
  double* part;        // [nblocks][tc][kSums] or NULL
  unsigned* tpart;     // [nblocks][tc][NTHR][M + 1], cells | observed << 16
  double* cell_crps;   // [n] or NULL
  int64_t row0[MSW_MAX_ENSEMBLE_MEMBERS];
};

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// Member m of this lane's unit sits in word m & 3 of the lane's 16-byte word of quad m >> 2.
__device__ __forceinline__ int slot(int m, int lane) { return (((m >> 2) * kWave + lane) << 2) + (m & 3); }

// sum_m (2 rank_m - M + 1) h_m over the parked depths: member m's rank is the number of members m'
// with h' < h, or h' == h and m' < m -- counted as h' <= h over the members before m and h' < h
// from m on.  The members past M up to the group's end hold +inf: never below a depth.
__device__ __forceinline__ double pair_sum(const unsigned* keys, int M, int lane) {
  const int groups = (M + kGroup - 1) / kGroup;
  double b = 0.0;
  for (int m = 0; m < M; ++m) {  // uniform
    const float vm = __uint_as_float(keys[slot(m, lane)]);
    int cnt = 0;
    for (int g = 0; g < groups; ++g) {
      u32x4 w[kGroup / 4];  // the group's four LDS reads in flight at once
#pragma unroll
      for (int i = 0; i < kGroup / 4; ++i)
        w[i] = *reinterpret_cast<const u32x4*>(keys + (((g * (kGroup / 4) + i) * kWave + lane) << 2));
#pragma unroll
      for (int i = 0; i < kGroup / 4; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float v = __uint_as_float(w[i][e]);
          const bool before = g * kGroup + 4 * i + e < m;
          cnt += (before ? v <= vm : v < vm) ? 1 : 0;
        }
      }
    }
    b += (double)(2 * cnt - M + 1) * (double)vm;  // the product is exact: fused or not, one rounding
  }
  return b;
}

template <int NTHR>
__global__ __launch_bounds__(kWave) void k_ensemble_scores(ScoreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned dyn[];  // the parked depths, then the tile's table
  __shared__ double s_term[kTerms][kWave];
  __shared__ unsigned s_word[kWave];
  const int lane = threadIdx.x;
  const int bins = a.M + 1;
  unsigned* keys = dyn;
  unsigned* table = dyn + (a.M + kGroup - 1) / kGroup * kGroup * kWave;
  const int64_t cell0 = (int64_t)blockIdx.x * a.cpb;
  const int ncell = (int)min<int64_t>(a.cpb, a.n - cell0);
  const double dM = (double)a.M;
  const int W = a.W, G = kWave / W;
  // lane = (r, t); a lane past the round's units repeats a unit of the round and is never read
  const int r = min(lane / W, G - 1), t = lane - (lane / W) * W;
  for (int t0 = 0; t0 < a.tc; t0 += W) {  // the tiles, uniform
    const int w = min(W, a.tc - t0);
    const int words = w * NTHR * bins;
    for (int i = lane; i < words; i += kWave) table[i] = 0;  // read by no other lane before the round's barrier
    double acc[kSums];
#pragma unroll
    for (int j = 0; j < kSums; ++j) acc[j] = 0.0;
    const int tl = min(t, w - 1);
    for (int r0 = 0; r0 < ncell; r0 += G) {  // uniform
      const int64_t cell = cell0 + min(r0 + r, ncell - 1);
      const float* p = a.pred + cell * 2 * a.T + a.tb + t0 + tl;  // member m: + row0[m] * 2 T
      const float yf = __builtin_nontemporal_load(a.truth + (a.trow0 + cell) * 2 * a.Tt + a.tt0 + t0 + tl);
      const double y = (double)yf;
      const int gl = min(G, ncell - r0);  // cells of this round
      double carried = 0.0;               // lane r0 + lane's cell_crps: fetched under the round's work
      if (a.cell_crps && lane < gl) carried = a.cell_crps[cell0 + r0 + lane];
      double sa = 0.0, S = 0.0, Q = 0.0;
      int cnt[NTHR > 0 ? NTHR : 1];
#pragma unroll
      for (int k = 0; k < NTHR; ++k) cnt[k] = 0;
      // A group's loads go out together; a member past M repeats the last one's load and parks
      // +inf, so that nothing below branches on the member count.
      for (int m0 = 0; m0 < a.M; m0 += kGroup) {  // uniform
        float v[kGroup];
#pragma unroll
        for (int j = 0; j < kGroup; ++j)
          v[j] = __builtin_nontemporal_load(p + a.row0[min(m0 + j, a.M - 1)] * 2 * a.T);
#pragma unroll
        for (int j = 0; j < kGroup; ++j) {
          const bool member = m0 + j < a.M;
          const double h = (double)v[j];
          sa += member ? fabs(h - y) : 0.0;
          S += member ? h : 0.0;
          Q += member ? h * h : 0.0;  // the square is exact: fused or not, one rounding
#pragma unroll
          for (int k = 0; k < NTHR; ++k) cnt[k] += member && v[j] > a.thr[k] ? 1 : 0;
          keys[slot(m0 + j, lane)] = __float_as_uint(member ? v[j] : INFINITY);
        }
      }
      double sb = a.need_b ? pair_sum(keys, a.M, lane) : 0.0;
      const double e = S - dM * y;  // M y is exact
      double sv = __dsub_rn(__dmul_rn(dM, Q), __dmul_rn(S, S));
      if (sa != sa) sb = sv = sa;   // a NaN depth: every term of the unit is NaN
      s_term[0][lane] = sa;
      s_term[1][lane] = sb;
      s_term[2][lane] = fabs(e);
      s_term[3][lane] = __dmul_rn(e, e);
      s_term[4][lane] = sv;
      s_term[5][lane] = __dsub_rn(__dmul_rn(dM, sa), sb);
      if constexpr (NTHR > 0) {
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < NTHR; ++k) word |= ((unsigned)cnt[k] | (yf > a.thr[k] ? 0x80u : 0u)) << (8 * k);
        s_word[lane] = word;
      }
      __syncthreads();
      if (lane < w) {                     // step t0 + lane: the round's cells in cell order
        for (int g = 0; g < gl; ++g) {
          const int u = g * W + lane;
#pragma unroll
          for (int j = 0; j < kSums; ++j) acc[j] += s_term[j][u];
          if constexpr (NTHR > 0) {
            const unsigned word = s_word[u];
#pragma unroll
            for (int k = 0; k < NTHR; ++k) {
              const unsigned c = (word >> (8 * k)) & 0x7fu, o = (word >> (8 * k + 7)) & 1u;
              table[(lane * NTHR + k) * bins + c] += 1u + (o << 16);
            }
          }
        }
      }
      if (a.cell_crps && lane < gl) {     // cell r0 + lane: the tile's steps in step order onto the carried value
        for (int s = 0; s < w; ++s) carried += s_term[5][lane * W + s];
        a.cell_crps[cell0 + r0 + lane] = carried;
      }
      __syncthreads();  // the terms are consumed: the next round may overwrite them
    }
    const int64_t col = (int64_t)blockIdx.x * a.tc + t0;
    if (a.part && lane < w) {
#pragma unroll
      for (int j = 0; j < kSums; ++j) a.part[(col + lane) * kSums + j] = acc[j];
    }
    if constexpr (NTHR > 0) {
      for (int i = lane; i < words; i += kWave) a.tpart[col * NTHR * bins + i] = table[i];
    }
  }
}

// sums[col0 + t][j] = the blocks' partials added in block order; reliability[col0 + t][k][c] =
// (cells, observed) summed over the blocks.
__global__ __launch_bounds__(kThreads) void k_scores_combine(const double* __restrict__ part,
                                                             const unsigned* __restrict__ tpart, int64_t nblocks,
                                                             int tc, int nthr, int bins, int n_thr_out, int col0,
                                                             double* __restrict__ sums,
                                                             int64_t* __restrict__ reliability) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  const int64_t count = (int64_t)tc * kSums, tcount = (int64_t)tc * nthr * bins;
  if (part && i < count) {
    double v = 0.0;
    for (int64_t b = 0; b < nblocks; ++b) v += part[b * count + i];
    sums[(int64_t)col0 * kSums + i] = v;
  }
  if (tpart && i < tcount) {
    int64_t cells = 0, observed = 0;
    for (int64_t b = 0; b < nblocks; ++b) {
      const unsigned w = tpart[b * tcount + i];
      cells += w & 0xffffu;
      observed += w >> 16;
    }
    const int64_t t = i / ((int64_t)nthr * bins), kc = i - t * nthr * bins;
    const int64_t o = ((col0 + t) * n_thr_out * bins + kc) * 2;
    reliability[o] = cells;
    reliability[o + 1] = observed;
  }
}

}  // namespace

extern "C" int msw_ensemble_scores_launch(int64_t n, int32_t M, int32_t t_count, int32_t* grid, int32_t* cells_per_wg,
                                          int32_t* iters) {
  if (!grid || !cells_per_wg || !iters) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n < 0 || t_count < 0) return msw::set_error(MSW_ERR_INVALID, "n or t_count negative");
  if (M < 1 || M > MSW_MAX_ENSEMBLE_MEMBERS) return msw::set_error(MSW_ERR_INVALID, "M out of range (1..64)");
  const Launch l = pick_launch(n, M, t_count);
  if (l.nblocks > INT32_MAX) return msw::set_error(MSW_ERR_INVALID, "n too large");
  const bool any = n > 0 && t_count > 0;
  *grid = any ? (int32_t)l.nblocks : 0;
  *cells_per_wg = l.G;
  *iters = l.iters;
  return MSW_OK;
}

extern "C" int msw_ensemble_scores_update(const float* pred, int32_t T, int32_t t_begin, int32_t t_count,
                                          const int64_t* member_row0, int32_t M, int64_t n, const float* truth,
                                          int32_t T_truth, int32_t t_truth0, int64_t truth_row0,
                                          const float* thresholds, int32_t n_thr, int32_t T_out, int32_t t_out0,
                                          const msw_ensemble_scores_out* out, void* stream) {
  if (!pred || !truth || !out || !member_row0 || (n_thr > 0 && !thresholds))
    return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (n_thr < 0 || n_thr > MSW_MAX_MAP_THRESHOLDS)
    return msw::set_error(MSW_ERR_INVALID, "n_thr out of range (0..4)");
  if (M < 1 || M > MSW_MAX_ENSEMBLE_MEMBERS) return msw::set_error(MSW_ERR_INVALID, "M out of range (1..64)");
  if (n < 0) return msw::set_error(MSW_ERR_INVALID, "n negative");
  if (T < 0 || t_begin < 0 || t_count < 0 || (int64_t)t_begin + t_count > T)
    return msw::set_error(MSW_ERR_INVALID, "time window outside [0, T]");
  if (T_truth < 0 || t_truth0 < 0 || (int64_t)t_truth0 + t_count > T_truth)
    return msw::set_error(MSW_ERR_INVALID, "truth columns outside [0, T_truth]");
  if (T_out < 0 || t_out0 < 0 || (int64_t)t_out0 + t_count > T_out)
    return msw::set_error(MSW_ERR_INVALID, "output columns outside [0, T_out]");
  for (int m = 0; m < M; ++m)
    if (member_row0[m] < 0) return msw::set_error(MSW_ERR_INVALID, "member_row0 negative");
  if (truth_row0 < 0) return msw::set_error(MSW_ERR_INVALID, "truth_row0 negative");
  const Launch l = pick_launch(n, M, t_count);
  if (l.nblocks > INT32_MAX) return msw::set_error(MSW_ERR_INVALID, "n too large");
  if (t_count == 0 || n == 0) return MSW_OK;
  // the threshold loop and the table run only when the table is produced
  const int nthr = out->reliability ? n_thr : 0;
  if (!nthr && !out->sums && !out->cell_crps) return MSW_OK;
  hipStream_t st = (hipStream_t)stream;
  ScoreArgs a{};
  a.pred = pred;
  a.truth = truth;
  a.T = T;
  a.tb = t_begin;
  a.tc = t_count;
  a.Tt = T_truth;
  a.tt0 = t_truth0;
  a.trow0 = truth_row0;
  a.n = n;
  a.M = M;
  a.cpb = l.cpb;
  a.W = l.W;
  a.need_b = out->sums || out->cell_crps;
  for (int k = 0; k < nthr; ++k) a.thr[k] = thresholds[k];
  a.cell_crps = out->cell_crps;
  for (int m = 0; m < M; ++m) a.row0[m] = member_row0[m];
  // one stream-ordered scratch for the blocks' partials: the five sums, then the tables
  const int bins = M + 1;
  const size_t sums_bytes = out->sums ? (size_t)l.nblocks * t_count * kSums * sizeof(double) : 0;
  const size_t table_bytes = (size_t)l.nblocks * t_count * nthr * bins * sizeof(unsigned);
  char* scratch = nullptr;
  if (sums_bytes + table_bytes) {
    const hipError_t e = hipMallocAsync((void**)&scratch, sums_bytes + table_bytes, st);
    if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  }
  a.part = sums_bytes ? reinterpret_cast<double*>(scratch) : nullptr;
  a.tpart = table_bytes ? reinterpret_cast<unsigned*>(scratch + sums_bytes) : nullptr;
  const size_t lds = ((size_t)(M + kGroup - 1) / kGroup * kGroup * kWave + (size_t)l.W * nthr * bins) * sizeof(unsigned);
  const dim3 grid((unsigned)l.nblocks), block(kWave);
  switch (nthr) {
    case 0: hipLaunchKernelGGL((k_ensemble_scores<0>), grid, block, lds, st, a); break;
    case 1: hipLaunchKernelGGL((k_ensemble_scores<1>), grid, block, lds, st, a); break;
    case 2: hipLaunchKernelGGL((k_ensemble_scores<2>), grid, block, lds, st, a); break;
    case 3: hipLaunchKernelGGL((k_ensemble_scores<3>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL((k_ensemble_scores<4>), grid, block, lds, st, a); break;
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess && scratch) {
    const int64_t items = std::max<int64_t>((int64_t)t_count * kSums, (int64_t)t_count * nthr * bins);
    hipLaunchKernelGGL(k_scores_combine, dim3((unsigned)((items + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                       (const double*)a.part, (const unsigned*)a.tpart, l.nblocks, (int)t_count, nthr, bins,
                       (int)n_thr, (int)t_out0, out->sums, out->reliability);
    e = hipGetLastError();
  }
  const hipError_t f = scratch ? hipFreeAsync(scratch, st) : hipSuccess;
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  if (f != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(f));
  return MSW_OK;
}
