// The training loss on device: loss_function of the reference and its gradient,
// which training_step evaluates after each of its R curriculum rollout steps.
//   loss_function / get_multiscale_loss / mask_on_water / get_mean_error  training/loss.py:8-118
//   conservation_loss                                                    training/loss.py:120-169
//   get_inflow_volume                                                    utils/dataset.py:577-591
//   training_step                                                        training/train.py:125-145
// The closest relative is metrics.hip: fp64 partial sums per workgroup (waves combined in a fixed
// order), then one workgroup adds the partials in index order and finishes the arithmetic.  No
// atomics, no host synchronisation, no allocation; the order of every addition is fixed by the row
// count and the ranges alone.  The arithmetic, operation for operation, is written out in
// include/mswegnn.h (tests/loss_cases.py repeats it in numpy).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/mswegnn.h"
#include "engine.h"

// Every operation rounds on its own, as written: a multiply-add contracted into an fma would make
// the record differ from a restatement that repeats the documented operations one by one.
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxParts = 512;  // workgroups of the partial-sum launch at most (metrics.hip's cap)
constexpr int kSums = 4;        // n, S_h, S_v, V
constexpr int kRanges = MSW_MAX_LOSS_RANGES;

// The ranges by value.  pre[r] = rows of the ranges before r, so list entry v of range r is row
// start[r] + (v - pre[r]); pre[nr] = total.  end[r] serves the backward.
struct Ranges {
  int nr;
  int start[kRanges];
  int end[kRanges];
  int pre[kRanges + 1];
};

struct FwdArgs {
  const float* pred;
  const float* real;
  const float* area;      // null without the conservation term
  const float* input_h;
  long stride;
  int mae, mask;
  double* part;           // [grid][kSums]
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ double sgn(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : x); }

__global__ __launch_bounds__(kThreads) void k_loss_partial(FwdArgs a, Ranges rg) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __shared__ double wsum[kThreads / 64][kSums];
  const int total = rg.pre[rg.nr];
  double n = 0.0, sh = 0.0, sv = 0.0, vol = 0.0;
  int r0 = 0;  // the range of the block's first entry: uniform, only ever moves forward
  for (long b0 = (long)blockIdx.x * kThreads; b0 < total; b0 += (long)gridDim.x * kThreads) {
    while (r0 + 1 < rg.nr && b0 >= rg.pre[r0 + 1]) ++r0;
    const long v = b0 + threadIdx.x;
    if (v < total) {
      int r = r0;
      while (r + 1 < rg.nr && v >= rg.pre[r + 1]) ++r;
      const size_t i = (size_t)rg.start[r] + (size_t)(v - rg.pre[r]);
      const float2 p = reinterpret_cast<const float2*>(a.pred)[i];
      const float2 q = reinterpret_cast<const float2*>(a.real)[i];
      const double dh = (double)p.x - (double)q.x, dv = (double)p.y - (double)q.y;
      const bool sel = !a.mask || dh != 0.0 || dv != 0.0;
      const double th = a.mae ? fabs(dh) : dh * dh, tv = a.mae ? fabs(dv) : dv * dv;
      n += sel ? 1.0 : 0.0;
      sh += sel ? th : 0.0;
      sv += sel ? tv : 0.0;
      if (a.area) vol += (double)a.area[i] * ((double)p.x - (double)a.input_h[i * a.stride]);
    }
  }
  double acc[kSums] = {wave_sum(n), wave_sum(sh), wave_sum(sv), wave_sum(vol)};
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kSums; ++k) wsum[w][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kSums) {  // the waves' sums in wave order
    double b = 0.0;
#pragma unroll
    for (int q = 0; q < kThreads / 64; ++q) b += wsum[q][threadIdx.x];
    a.part[(size_t)blockIdx.x * kSums + threadIdx.x] = b;
  }
}

struct FinArgs {
  const double* part;
  int nparts;
  const float* pred;
  const float* area;
  const float* input_h;
  long stride;
  const long long* node_bc;
  const float* bc;
  const float* len;
  int n_bc;
  long num_rows;
  int mae;
  int num_graphs;
  double vs, c, seconds;
  float* loss_out;
  double* rec;
};

// One workgroup.  Thread k < 4 adds partial k of every workgroup in index order, thread 4 walks
// the BC cells, thread 5 the inflow; thread 0 then finishes in the order of the header comment.
__global__ __launch_bounds__(kThreads) void k_loss_finalize(FinArgs a) {
  __shared__ double stage[kMaxParts * kSums];
  __shared__ double tot[kSums + 2];
  for (int i = threadIdx.x; i < a.nparts * kSums; i += kThreads) stage[i] = a.part[i];
  __syncthreads();
  if (threadIdx.x < kSums) {
    double s = 0.0;
    for (int b = 0; b < a.nparts; ++b) s += stage[b * kSums + threadIdx.x];
    tot[threadIdx.x] = s;
  } else if (threadIdx.x == kSums) {
    double s = 0.0;
    if (a.c != 0.0) {
      for (int k = 0; k < a.n_bc; ++k) {
        const long long r = a.node_bc[k];
        if (r < 0 || r >= a.num_rows) continue;
        s += (double)a.area[r] * ((double)a.pred[(size_t)r * 2] - (double)a.input_h[(size_t)r * a.stride]);
      }
    }
    tot[kSums] = s;
  } else if (threadIdx.x == kSums + 1) {
    double s = 0.0;
    if (a.c != 0.0) {
      for (int k = 0; k < a.n_bc; ++k) s += (double)a.bc[k] * (double)a.len[k];
      s = s * a.seconds;
    }
    tot[kSums + 1] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double n = tot[0], sh = tot[1], sv = tot[2];
  const bool on = a.c != 0.0;
  const double vol = on ? tot[3] : 0.0, corr = tot[4], inflow = tot[5];
  const double lh = a.mae ? sh / n : sqrt(sh / n), lv = a.mae ? sv / n : sqrt(sv / n);
  const double data = (lh + a.vs * lv) / (1.0 + a.vs);
  const double cons = on ? ((vol - inflow) - corr) / 1e6 / (double)a.num_graphs : 0.0;
  const double loss = on ? data + a.c * fabs(cons) : data;
  const double wh = 1.0 / (1.0 + a.vs), wv = a.vs / (1.0 + a.vs);
  a.rec[0] = n;
  a.rec[1] = sh;
  a.rec[2] = sv;
  a.rec[3] = vol;
  a.rec[4] = corr;
  a.rec[5] = inflow;
  a.rec[6] = cons;
  a.rec[7] = loss;
  a.rec[8] = a.mae ? wh / n : wh / (n * lh);
  a.rec[9] = a.mae ? wv / n : wv / (n * lv);
  a.rec[10] = on ? a.c * sgn(cons) / (1e6 * (double)a.num_graphs) : 0.0;
  a.rec[11] = data;
  *a.loss_out = (float)loss;
}

struct BwdArgs {
  const float* pred;
  const float* real;
  const double* rec;
  const float* gout;
  const float* area;  // null without the conservation term
  float* gpred;
  float* gin;         // or null
  long num_rows;
  int mae, mask;
};

// One thread per row of [0, num_rows): rows of no range get zeros.
__global__ __launch_bounds__(kThreads) void k_loss_backward(BwdArgs a, Ranges rg) {
  const long b0 = (long)blockIdx.x * kThreads;
  const long i = b0 + threadIdx.x;
  int r = 0;
  while (r + 1 < rg.nr && b0 >= rg.end[r]) ++r;  // uniform
  if (i >= a.num_rows) return;
  while (r + 1 < rg.nr && i >= rg.end[r]) ++r;
  const bool in = i >= rg.start[r] && i < rg.end[r];
  float gh = 0.f, gv = 0.f, m = 0.f;
  if (in) {
    const double g = (double)*a.gout;
    const float2 p = reinterpret_cast<const float2*>(a.pred)[i];
    const float2 q = reinterpret_cast<const float2*>(a.real)[i];
    const double dh = (double)p.x - (double)q.x, dv = (double)p.y - (double)q.y;
    if (!a.mask || dh != 0.0 || dv != 0.0) {
      gh = (float)((g * a.rec[8]) * (a.mae ? sgn(dh) : dh));
      gv = (float)((g * a.rec[9]) * (a.mae ? sgn(dv) : dv));
    }
    if (a.area) {
      m = (float)((g * a.rec[10]) * (double)a.area[i]);
      gh += m;
    }
  }
  reinterpret_cast<float2*>(a.gpred)[i] = make_float2(gh, gv);
  if (a.gin) a.gin[i] = in ? -m : 0.f;
}

// The ghost cells leave the balance (loss.py:161): one thread, list order, so that a row listed
// twice is handled twice in a fixed order.
__global__ void k_loss_backward_bc(const double* rec, const float* gout, const float* area,
                                   const long long* node_bc, int n_bc, long num_rows, float* gpred, float* gin) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const double gc = (double)*gout * rec[10];
  for (int k = 0; k < n_bc; ++k) {
    const long long r = node_bc[k];
    if (r < 0 || r >= num_rows) continue;
    const float m = (float)(gc * (double)area[r]);
    gpred[(size_t)r * 2] -= m;
    if (gin) gin[r] += m;
  }
}

struct Launch {
  int grid, iters;
};

Launch pick_launch(int64_t total) {
  Launch l{0, 0};
  if (total <= 0) return l;
  const int64_t blocks = (total + kThreads - 1) / kThreads;
  l.grid = (int)std::min<int64_t>(kMaxParts, blocks);
  l.iters = (int)((blocks + l.grid - 1) / l.grid);
  return l;
}

// Every MSW_ERR_INVALID condition of the header, and the ranges as the kernels take them.
int check_desc(const msw_train_loss_desc* d, Ranges* rg) {
  if (!d) return msw::set_error(MSW_ERR_INVALID, "null desc");
  if (d->num_ranges < 1 || d->num_ranges > kRanges)
    return msw::set_error(MSW_ERR_INVALID, "num_ranges outside 1..64");
  if (d->num_rows < 0 || d->num_rows > INT32_MAX - (int64_t)kMaxParts * kThreads)
    return msw::set_error(MSW_ERR_INVALID, "num_rows negative or past the int32 row limit");
  if (d->type_loss != MSW_LOSS_RMSE && d->type_loss != MSW_LOSS_MAE)
    return msw::set_error(MSW_ERR_INVALID, "unknown type_loss");
  if (d->num_graphs < 1) return msw::set_error(MSW_ERR_INVALID, "num_graphs < 1");
  int64_t at = 0, total = 0;
  rg->nr = d->num_ranges;
  for (int r = 0; r < kRanges; ++r) rg->start[r] = rg->end[r] = rg->pre[r + 1] = 0;
  rg->pre[0] = 0;
  for (int r = 0; r < d->num_ranges; ++r) {
    const int64_t s = d->ranges[r][0], e = d->ranges[r][1];
    if (s < 0) return msw::set_error(MSW_ERR_INVALID, "range start negative");
    if (e < s) return msw::set_error(MSW_ERR_INVALID, "range end < start");
    if (e > d->num_rows) return msw::set_error(MSW_ERR_INVALID, "range end past num_rows");
    if (s < at) return msw::set_error(MSW_ERR_INVALID, "ranges not ascending and disjoint");
    at = e;
    rg->start[r] = (int)s;
    rg->end[r] = (int)e;
    rg->pre[r] = (int)total;
    total += e - s;
  }
  for (int r = d->num_ranges; r <= kRanges; ++r) rg->pre[r] = (int)total;
  if (d->conservation != 0.0) {
    if (!d->area || !d->input_h) return msw::set_error(MSW_ERR_INVALID, "conservation needs area and input_h");
    if (d->n_bc < 0) return msw::set_error(MSW_ERR_INVALID, "n_bc negative");
    if (d->n_bc > 0 && (!d->node_bc || !d->bc || !d->edge_bc_length))
      return msw::set_error(MSW_ERR_INVALID, "conservation with n_bc > 0 needs node_bc, bc and edge_bc_length");
  }
  return MSW_OK;
}

}  // namespace

extern "C" int msw_train_loss_launch(int64_t total_rows, int32_t* grid, int32_t* rows_per_wg, int32_t* iters) {
  if (!grid || !rows_per_wg || !iters) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (total_rows < 0) return msw::set_error(MSW_ERR_INVALID, "total_rows negative");
  const Launch l = pick_launch(total_rows);
  *grid = l.grid;
  *rows_per_wg = kThreads;
  *iters = l.iters;
  return MSW_OK;
}

extern "C" int msw_train_loss_workspace(const msw_train_loss_desc* desc, int64_t* scratch_doubles) {
  Ranges rg;
  if (!scratch_doubles) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (int rc = check_desc(desc, &rg)) return rc;
  *scratch_doubles = (int64_t)kSums * std::max(1, pick_launch(rg.pre[rg.nr]).grid);
  return MSW_OK;
}

extern "C" int msw_train_loss_forward(const msw_train_loss_desc* desc, const float* pred, const float* real,
                                      double* scratch, float* loss_out, double* record_out, void* stream) {
  Ranges rg;
  if (int rc = check_desc(desc, &rg)) return rc;
  if (!pred || !real || !scratch || !loss_out || !record_out) return msw::set_error(MSW_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  const bool on = desc->conservation != 0.0;
  const Launch l = pick_launch(rg.pre[rg.nr]);
  if (l.grid > 0) {
    FwdArgs a{};
    a.pred = pred;
    a.real = real;
    a.area = on ? desc->area : nullptr;
    a.input_h = desc->input_h;
    a.stride = (long)desc->input_h_stride;
    a.mae = desc->type_loss == MSW_LOSS_MAE;
    a.mask = desc->only_where_water != 0;
    a.part = scratch;
    hipLaunchKernelGGL(k_loss_partial, dim3(l.grid), dim3(kThreads), 0, st, a, rg);
  }
  FinArgs f{};
  f.part = scratch;
  f.nparts = l.grid;
  f.pred = pred;
  f.area = desc->area;
  f.input_h = desc->input_h;
  f.stride = (long)desc->input_h_stride;
  f.node_bc = reinterpret_cast<const long long*>(desc->node_bc);
  f.bc = desc->bc;
  f.len = desc->edge_bc_length;
  f.n_bc = on ? desc->n_bc : 0;
  f.num_rows = (long)desc->num_rows;
  f.mae = desc->type_loss == MSW_LOSS_MAE;
  f.num_graphs = desc->num_graphs;
  f.vs = desc->velocity_scaler;
  f.c = desc->conservation;
  f.seconds = desc->seconds_per_step;
  f.loss_out = loss_out;
  f.rec = record_out;
  hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(kThreads), 0, st, f);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  return MSW_OK;
}

extern "C" int msw_train_loss_backward(const msw_train_loss_desc* desc, const float* pred, const float* real,
                                       const double* record, const float* grad_out, float* grad_pred,
                                       float* grad_input_h, void* stream) {
  Ranges rg;
  if (int rc = check_desc(desc, &rg)) return rc;
  if (!pred || !real || !record || !grad_out || !grad_pred) return msw::set_error(MSW_ERR_INVALID, "null argument");
  if (desc->num_rows == 0) return MSW_OK;
  hipStream_t st = (hipStream_t)stream;
  const bool on = desc->conservation != 0.0;
  BwdArgs a{};
  a.pred = pred;
  a.real = real;
  a.rec = record;
  a.gout = grad_out;
  a.area = on ? desc->area : nullptr;
  a.gpred = grad_pred;
  a.gin = on ? grad_input_h : nullptr;
  a.num_rows = (long)desc->num_rows;
  a.mae = desc->type_loss == MSW_LOSS_MAE;
  a.mask = desc->only_where_water != 0;
  const unsigned grid = (unsigned)((desc->num_rows + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(k_loss_backward, dim3(grid), dim3(kThreads), 0, st, a, rg);
  if (on && desc->n_bc > 0)
    hipLaunchKernelGGL(k_loss_backward_bc, dim3(1), dim3(64), 0, st, record, grad_out, desc->area,
                       reinterpret_cast<const long long*>(desc->node_bc), desc->n_bc, (long)desc->num_rows,
                       grad_pred, a.gin);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return msw::set_error(MSW_ERR_HIP, hipGetErrorString(e));
  return MSW_OK;
}
