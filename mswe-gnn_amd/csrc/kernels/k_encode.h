// gfx950 kernels: node encoders (+ the deferred decoder).
// Part of kernels_impl.h (included inside namespace msw, in this order); see its header
// comment for the register layout and conventions.
#pragma once

// ---------------------------------------------------------------------------- encoder arguments
// The scale of the 64-row chunk that starts at row rb and that scale's fields.  k_encode_coop
// selects them from the whole small per-scale arrays, which arrive with its other arguments
// (EncTables, pinned at entry): a search loop and run-time-indexed argument reads were one
// dependent trip to the cold argument segment each.  (Scale starts ascend, so the last scale
// that starts at or before rb is the one the search found.)
struct EncScale {
  int s, n0, ns, vu_a;
  WReg reg;
};
// (k_encode keeps the search: its grid-stride loop would hold the tables in 48 SGPRs, which it
// does not have; STAGED = kStaged<NT>: the regions exist at F <= 32 only)
template <bool STAGED>
struct EncTables {  // EncodeArgs::n0 / ns / vu_a [0, 8) and sreg (3 ints per scale) as SGPR tuples
  i32xN<8> n0, ns, vu;
  i32xN<16> ra;
  i32xN<8> rb;
};
template <>
struct EncTables<false> {
  i32xN<8> n0, ns, vu;
};
static_assert(kMaxScales == 8 && sizeof(WReg) == 12, "EncTables: eight scales, {off, len, split} regions");
template <bool STAGED>
__device__ __forceinline__ EncTables<STAGED> enc_tables(const EncodeArgs& a) {
  if constexpr (STAGED)
    return EncTables<true>{kernarg_vec<8>(a.n0), kernarg_vec<8>(a.ns), kernarg_vec<8>(a.vu_a), kernarg_vec<16>(a.sreg),
                           kernarg_vec<8>(reinterpret_cast<const int*>(a.sreg) + 16)};
  else
    return EncTables<false>{kernarg_vec<8>(a.n0), kernarg_vec<8>(a.ns), kernarg_vec<8>(a.vu_a)};
}
// the lazy form: search, then run-time-indexed reads
__device__ __forceinline__ EncScale enc_scale(const EncodeArgs& a, int rb) {
  int s = 0;
  while (s + 1 < a.S && rb >= a.n0[s + 1]) ++s;
  return EncScale{s, a.n0[s], a.ns[s], a.vu_a[s], a.sreg[s]};
}
template <bool STAGED>
__device__ __forceinline__ EncScale enc_scale(const EncodeArgs& a, const EncTables<STAGED>& t, int rb) {
  if constexpr (!MSW_ARGS_HOIST) return enc_scale(a, rb);
  EncScale e{0, t.n0[0], t.ns[0], t.vu[0], WReg{0, 0, 0}};
  if constexpr (STAGED) e.reg = WReg{t.ra[0], t.ra[1], 0};
#pragma unroll
  for (int k = 1; k < kMaxScales; ++k) {
    const bool in = k < a.S && rb >= t.n0[k];
    e.s = in ? k : e.s;
    e.n0 = in ? t.n0[k] : e.n0;
    e.ns = in ? t.ns[k] : e.ns;
    e.vu_a = in ? t.vu[k] : e.vu_a;
    if constexpr (STAGED) {
      const int off = 3 * k < 16 ? t.ra[3 * k < 16 ? 3 * k : 0] : t.rb[3 * k >= 16 ? 3 * k - 16 : 0];
      const int len = 3 * k + 1 < 16 ? t.ra[3 * k + 1 < 16 ? 3 * k + 1 : 0] : t.rb[3 * k + 1 >= 16 ? 3 * k + 1 - 16 : 0];
      e.reg.off = in ? off : e.reg.off;
      e.reg.len = in ? len : e.reg.len;
    }
  }
  return e;
}
// what both encoders read before their first row load; TAB: the per-scale tables
#define MSW_ARGS_ENC(a)                                                                                       \
  (a).Npad, (a).S, (a).x, (a).x_internal, (a).c.perm, (a).c.nnf, (a).c.nstat_raw, (a).c.dyn, (a).c.W, (a).io, \
      (a).dec.on
#define MSW_ARGS_ENC_DEC(a) (a).dec.io, (a).dec_in, (a).dec.bc_slot
#define MSW_ARGS_ENC_TAB(t) (t).n0, (t).ns, (t).vu
#define MSW_ARGS_ENC_REG(t) (t).ra, (t).rb
// F = 64 (no regions): the scale starts and row counts as sixteen scalars -- the misaligned
// 8-int tuples cost a second round trip there (they are assembled from two loads' pieces) --
// and vu_a[s] read where it is used, at the kernel's end
#define MSW_ARGS_ENC_N(a)                                                                                  \
  (a).n0[0], (a).n0[1], (a).n0[2], (a).n0[3], (a).n0[4], (a).n0[5], (a).n0[6], (a).n0[7], (a).ns[0], (a).ns[1], \
      (a).ns[2], (a).ns[3], (a).ns[4], (a).ns[5], (a).ns[6], (a).ns[7]
__device__ __forceinline__ EncScale enc_scale_scalars(const EncodeArgs& a, int rb) {
  EncScale e{0, a.n0[0], a.ns[0], 0, WReg{0, 0, 0}};
#pragma unroll
  for (int k = 1; k < kMaxScales; ++k) {
    const bool in = k < a.S && rb >= a.n0[k];
    e.s = in ? k : e.s;
    e.n0 = in ? a.n0[k] : e.n0;
    e.ns = in ? a.ns[k] : e.ns;
  }
  e.vu_a = a.vu_a[e.s];
  return e;
}
// ---------------------------------------------------------------------------- encoder
// Static / dynamic node encoders incl. the water-level feature (MSGNN.forward
// gnn.py:284-294, GNN.forward :112-123) + projection of processor 0 + the x_s part of
// every unpooling layer's V.  One workgroup = 64 rows of one scale.
// DEC: the rollout variant that decodes the previous step first (EncodeArgs::dec.on); the
// other variant keeps the encoders' register budget (four waves per SIMD) for forward mode
// and the large meshes whose last hops decode.
// STREAM (grid-stride launches without DEC, EncodeArgs::stream): the rows go out with
// streaming stores (k_base.h st4_stream).
template <int NT, int ACT, bool DEC, bool STREAM = false>
__global__ __launch_bounds__(kBlock) void k_encode(EncodeArgs a) {
  constexpr bool ST = STREAM && !DEC;
  constexpr int F = 16 * NT;
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
  if constexpr (DEC)
    MSW_PIN(MSW_ARGS_ENC(a), MSW_ARGS_ENC_DEC(a));
  else
    MSW_PIN(MSW_ARGS_ENC(a));
  MSW_MARK(a.c, 0);
  Common c = a.c;
  // rollout mode: the step whose prediction this launch decodes (the previous one; -1 at
  // step 0, whose state k_init_state wrote).  The I/O record is read once, whole, as soon as
  // its pointer has arrived (nothing writes it during a decoding launch).
  // (MSW_ARGS_HOIST=0: every field read through the pointer where it is used)
  RolloutIO iocopy{};
  if constexpr (DEC && MSW_ARGS_HOIST) iocopy = *a.dec.io;
  const RolloutIO& iov = (DEC && !MSW_ARGS_HOIST) ? *a.dec.io : iocopy;
  const int dstep = DEC ? iov.step : -1;
  // rollout mode, decoder in the last hops (large meshes): advance the step they read
  if (!a.dec.on && a.io && blockIdx.x == 0 && threadIdx.x == 0) a.io->step += 1;
  const int nchunks = a.Npad / kRowsPerBlock;
  int staged = -1;  // scale whose region is in LDS
  // grid-stride over 64-row chunks (scale ranges are 64-aligned: a chunk has one scale);
  // the per-scale weight region is re-staged only when the scale changes
  for (int chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
    const int rb = chunk * kRowsPerBlock;
    const EncScale sc = enc_scale(a, rb);
    const int s = sc.s;
    const int n = rb + wave_id() * kRowsPerWave + j;
    const bool valid = (n - sc.n0) < sc.ns;
    const int ext = a.c.perm ? a.c.perm[n] : n;
    const int xrow = a.x_internal ? (valid ? n : sc.n0) : (valid ? ext : 0);
    const float* xr = a.x + (size_t)xrow * a.c.nnf;
    const int nstat = a.c.nstat_raw;
    float raw[4], dyn[4];
    float wlv;
    EpiPre<NT> pre;
    f32x4 xu[NT];
    // the decoder's inputs, loaded before the weight staging and whatever the step (at step
    // 0 nothing reads them): not behind the load of the step counter, whose dependent loads
    // (the BC values) are issued after the staging barrier, in flight during the decoder MLP
    if (DEC) {
      load_row<NT>(xu, a.dec_in + (size_t)n * F, g);
      pre.ext = ext;
      pre.bc = a.dec.bc_slot[n];
#pragma unroll
      for (int k = 0; k < kMaxDyn; ++k) pre.xd[k] = k < c.dyn ? xr[nstat + k] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = 4 * g + r;
      raw[r] = f < nstat ? xr[f] : 0.f;
      dyn[r] = f < a.c.dyn ? xr[nstat + f] : 0.f;
    }
    wlv = xr[nstat - 1] + xr[a.c.nnf - 2];  // water level = bed elevation + depth
    if constexpr (kBcHoist<NT>) {  // the next step's BC values before the weight staging
      if constexpr (DEC) MSW_PIN(iov.step, iov.bc, iov.bc_tstride, iov.type_bc);
      if (DEC && dstep >= 0) {
        pre.step = dstep;
        bc_prefetch<NT, true>(pre, iov, c);
      }
    }
    MSW_MARK(c, 1);
    if constexpr (kStaged<NT>) {
      if (s != staged) {  // uniform across the workgroup: every wave walks the same chunks
        if (staged >= 0) __syncthreads();  // everyone is done with the old region
        stage_glds(smem, a.c.W, sc.reg, 0, sc.reg.len);
        __syncthreads();
        staged = s;
      }
    }
    // weight reads straight from the LDS pointer (not through c.W, which the compiler cannot
    // prove to be LDS across the loop: it emitted flat loads, which wait on vmcnt too)
    const float* Wl = kStaged<NT> ? (const float*)smem : c.W;
    if (DEC && dstep >= 0) {  // decode the previous step; the encoders read the updated state
      if constexpr (!kBcHoist<NT>) {
        pre.step = dstep;
        bc_prefetch<NT, true>(pre, iov, c);
      }
      float nd[kMaxDyn];
      decode_state<NT, ACT, true>(xu, a.dec, c, Wl, pre, n, valid, lane, g, nd);
#pragma unroll
      for (int r = 0; r < 4; ++r) dyn[r] = nd_column(nd, g, r, c.dyn);
      float hn = 0.f;
#pragma unroll
      for (int k = 0; k < kMaxDyn; ++k) hn = (k == c.dyn - 2) ? nd[k] : hn;
      wlv = xr[nstat - 1] + hn;
    }
    if (DEC && a.decode_only) continue;
    MSW_MARK(c, 2);
    f32x4 xs[NT];
    {
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = (c.with_wl && 4 * g + r == nstat) ? wlv : raw[r];
      const f32x4 in[1] = {v};
      run_mlp<1, NT, NT, ACT>(in, xs, a.stat, Wl, lane, g);
      mask_pad<ACT, NT>(xs, c.fl, g);
      if (valid) store_row<NT, ST>(a.xs + (size_t)n * F, xs, NT, g);
    }
    MSW_MARK(c, 5);
    if (s == 0) {
      f32x4 xd[NT];
      const f32x4 in[1] = {f32x4{dyn[0], dyn[1], dyn[2], dyn[3]}};
      run_mlp<1, NT, NT, ACT>(in, xd, a.dynm, Wl, lane, g);
      mask_pad<ACT, NT>(xd, c.fl, g);
      if (valid && a.xd) store_row<NT, ST>(a.xd + (size_t)n * F, xd, NT, g);
      MSW_MARK(c, 6);
      np_project<NT, ST>(xs, xd, a.np0, Wl, n, valid, lane, g);
    }
    MSW_MARK(c, 8);
    if (sc.vu_a >= 0) side_proj<NT, NT, ST>(xs, a.vu_h1t, Wl + sc.vu_a, a.Vu, n, valid, lane, g);
  }
  MSW_MARK(c, 9);
}

// ---------------------------------------------------------------------------- forward decode
// Forward mode with the deferred decoder (schedule.hip sched_step): decode_rows -- the last hops'
// forward-mode epilogue, operation for operation -- on 16 stored last-layer rows per wave,
// after the whole schedule instead of inside four latency-bound last hops.  The decoder
// operands are read from the blob (a few KB, L2-resident): no staging barrier.
template <int NT, int ACT>
__global__ __launch_bounds__(kBlock) void k_decode_fwd(DecodeArgs a) {
  constexpr int F = 16 * NT;
  const int lane = threadIdx.x & 63, g = lane >> 4, j = lane & 15;
  MSW_PIN(a.Npad, a.in, a.c.perm, a.dec.X, a.c.nnf, a.c.dyn, a.c.W, a.dec.pre_act, a.dec.pre_slope, a.dec.resw_off,
          a.dec.y, a.dec.dec.l[0].tin, MSW_ARGS_MLP(a.dec.dec));
  const int n = wave_row0() + j;
  if (wave_row0() >= a.Npad) return;  // whole wave past the rows
  const bool valid = n < a.Npad;
  const int nn = valid ? n : 0;
  EpiPre<NT> pre;
  f32x4 xu[NT];
  load_row<NT>(xu, a.in + (size_t)nn * F, g);
  const Common& c = a.c;
  pre.ext = valid ? c.perm[nn] : -1;
  pre.step = 0;
  pre.bc = -1;
  const float* xr = a.dec.X + (size_t)(pre.ext > 0 ? pre.ext : 0) * c.nnf + (c.nnf - c.dyn);
#pragma unroll
  for (int k = 0; k < kMaxDyn; ++k) pre.xd[k] = k < c.dyn ? xr[k] : 0.f;
  decode_rows<NT, ACT>(xu, a.dec, c, pre, nn, valid, lane, g);
}
