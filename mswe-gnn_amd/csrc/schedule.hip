// What a step launches: the schedule of MSGNN.forward / GNN.forward in forward and rollout
// mode (sched_step), and the variant and residency rules that choose each launch's kernel
// (set_grid_cap, one cap_* per launch kind).  build_schedules is the entry.
//
// Reference semantics followed (sdat2/mSWE-GNN):
//   MSGNN.forward  models/gnn.py:267-350     GNN.forward  models/gnn.py:102-152
//   SWEGNN.forward models/gnn.py:387-445
#include <initializer_list>
#include <utility>

#include "plan.h"

using namespace msw;

namespace {

// The size rules, in one place.
// F = 64: the edge MLP runs alone (k_edge_mlp) from this many edge tiles up
constexpr int kSplitMlpTiles = 1024;
// fused (un)pooling: one 4-wave workgroup (two tiles) per CU, one round
constexpr int kMaxFusedPoolBlocks = 256;
// rollout: the decoder leaves the last hops for the next step's encoder below this many
// edge tiles of the finest scale (sched_step)
constexpr int kDeferMaxTiles = 65536;
// hops run one tile per wave below this many edge tiles, grid-stride from it (cap_hop)
constexpr int kHopLoopTiles = 65536;
// middle hops of scales with at least this many edge tiles run in the row layout
// (k_hop_rows; MSW_HOP_ROWS=0 keeps the edge tiles)
constexpr int kRowHopMinTiles = kHopLoopTiles;
// Dense row-tile hops (k_hop_dense) on scales of at most this many row tiles (two waves per
// SIMD in one round), and only while the chip holds them all at once: beyond, the launch is
// no longer latency-bound and the edge tiles' fewer, wider gathers win
// (profiles/densehop/ab_workloads.txt; MSW_HOP_DENSE=0 switches the kernel off)
constexpr int kDenseMaxTiles = 2048;
// F = 64: the cooperative encoder while rows / 16 x NT stays within this many waves (cap_encode)
constexpr long kEncCoopWaves = 4096;

NpDesc np_of(msw_plan* P, const Proc& pr) {
  NpDesc d{};
  d.a_u = pr.a_u; d.a_v = pr.a_v; d.a_o = pr.a_o; d.h1t = pr.h1t;
  d.U = P->U[pr.par]; d.V = P->V[pr.par]; d.O = P->O[pr.par];
  return d;
}
NpDesc np_none() {
  NpDesc d{};
  d.a_u = d.a_v = d.a_o = -1;
  d.h1t = 1;
  return d;
}

Common common_of(msw_plan* P) {
  Common c{};
  c.W = P->dW; c.perm = P->perm_d; c.nnf = P->nnf; c.dyn = P->dyn; c.p = P->p; c.zrow = P->zrow_d;
  c.xcd_max = (short)P->kn.xcd_max;
  c.fl = (short)P->F;
  c.nstat_raw = P->nstat_raw; c.with_wl = P->with_wl; c.prelu = P->prelu;
  return c;
}

DecDesc dec_of(msw_plan* P, const float* x_src, bool rollout, float* y) {
  DecDesc d{};
  d.on = 1;
  d.pre_act = P->model_type == 0 ? P->gnn_act : 0;
  d.pre_slope = P->gnn_slope;
  d.dec = P->dec;
  d.resw_off = P->resw_off;
  d.X = x_src;
  d.x_internal = rollout ? 1 : 0;
  d.y = y;
  d.io = rollout ? P->io_d : nullptr;
  d.bc_slot = P->bc_slot_d;
  return d;
}

// Partitioned mesh: refresh the halo rows of `bufs` on `scale` before a gathering launch.
void sched_exchange(msw_plan* P, std::vector<Launch>& q, int scale, std::initializer_list<std::pair<int, int>> bufs) {
  if (P->xch.empty() || P->xch[scale].peers.empty()) return;
  Launch L;
  L.kind = L_EXCHANGE;
  L.scale = scale;
  L.xch.c = common_of(P);
  L.xch.scale = scale;
  for (auto& b : bufs) {
    L.xch.buf[L.xch.nbuf] = b.first;
    L.xch.width[L.xch.nbuf] = b.second;
    ++L.xch.nbuf;
  }
  q.push_back(L);
}

// the layer's edge MLP runs alone (k_edge_mlp) and hop 1 as a k_hop launch
bool edge_mlp_split(const msw_plan* P, const Proc& pr) {
  if (P->NT != 4 || pr.K < 2 || P->part_rank >= 0) return false;  // F = 64 only (F = 32: -3.4 %)
  return P->kn.split_edge_mlp >= 0 ? P->kn.split_edge_mlp != 0 : P->sc[pr.scale].ntiles >= kSplitMlpTiles;
}

// Hop k (1..K) of layer pr as a k_hop launch: in -> out, running `epi` when `last`.
Launch hop_launch(msw_plan* P, const Proc& pr, int k, const float* in, float* out, bool last, const Epilogue& epi) {
  const ScaleCSR& g = P->sc[pr.scale];
  Launch L;
  L.kind = L_HOP;
  L.scale = pr.scale;
  HopArgs& h = L.hop;
  h.c = common_of(P);
  h.n0 = g.n0; h.recs = g.recs; h.ntiles = g.ntiles;
  h.nrows = g.ns; h.rptr = g.rptr; h.redge = g.redge;
  h.s = P->s; h.xs = P->xs;
  h.in = in; h.out = out;
  h.filt_a = pr.filt.empty() ? -1 : pr.filt[k - 1];
  h.grad = pr.with_gradient; h.upwind = pr.upwind;
  h.last = last;
  h.epi = epi;
  return L;
}

// The layer's epilogue on dense node tiles, after a last hop that ran as a middle hop.
Launch epi_launch(msw_plan* P, const Proc& pr, const float* in, float* out, const Epilogue& epi) {
  const ScaleCSR& g = P->sc[pr.scale];
  Launch L;
  L.kind = L_EPI;
  L.scale = pr.scale;
  EpiArgs& ea = L.ep;
  ea.c = common_of(P);
  ea.n0 = g.n0; ea.ns = g.ns; ea.ntiles = (g.ns + kRowsPerWave - 1) / kRowsPerWave;
  ea.in = in; ea.xs = P->xs; ea.out = out;
  ea.epi = epi;
  return L;
}

// One SWEGNN layer on its scale: fused edge-MLP + hop 1, then hops 2..K; the last hop
// runs `epi` (and stores its output to `out` if non-null).  out_0 is in O[par].
void sched_proc(msw_plan* P, std::vector<Launch>& q, const Proc& pr, float* out, const Epilogue& epi,
                const PoolFuse* pool = nullptr) {
  const ScaleCSR& g = P->sc[pr.scale];
  sched_exchange(P, q, pr.scale, {{pr.par ? B_U1 : B_U0, 16 * pr.h1t}, {pr.par ? B_O1 : B_O0, P->Fp}});
  Launch L1;
  L1.kind = L_EDGE_HOP;
  L1.scale = pr.scale;
  EdgeHopArgs& eh = L1.eh;
  eh.c = common_of(P); eh.n0 = g.n0; eh.recs = g.recs; eh.ntiles = g.ntiles; eh.xs = P->xs; eh.U = P->U[pr.par]; eh.V = P->V[pr.par]; eh.Pe = pr.Pe;
  eh.b1_off = pr.b1_off; eh.h1t = pr.h1t; eh.act1 = pr.act1; eh.slope1 = pr.slope1;
  eh.rest = pr.rest; eh.normalize = pr.normalize;
  eh.c.prelu = P->prelu & pr.prelu;
  eh.s = pr.K > 1 ? P->s : nullptr;
  eh.in = P->O[pr.par]; eh.own_zero = 0; eh.grad = pr.with_gradient; eh.upwind = pr.upwind;
  eh.filt_a = pr.filt.empty() ? -1 : pr.filt[0];
  eh.skip = nullptr;
  eh.last = pr.K == 1;
  eh.out = pr.K == 1 ? out : P->T[0];
  eh.epi = epi;
  if (pool) eh.pool = *pool;  // U / V / O of this layer formed in the launch (no pooling launch)
  // F = 64 scales beyond one round of the fused kernel (one wave per SIMD): the edge MLP
  // alone over dense edge chunks (k_edge_mlp, two waves per SIMD) + hop 1 as a k_hop launch
  // (MSW_SPLIT_EDGE_MLP=0/1 overrides the size rule)
  if (edge_mlp_split(P, pr)) {
    L1.kind = L_EDGE_MLP;
    eh.chunks = g.chunks; eh.nchunks = g.nchunks;
    q.push_back(L1);
    q.push_back(hop_launch(P, pr, 1, P->O[pr.par], P->T[0], false, epi));
  } else {
    q.push_back(L1);
  }
  // one launch per hop (hop chains -- several hops per launch with the halo recomputed --
  // measured 0.7-1.6 % slower under graph replay, profiles/r01_v7/ab_chains.txt)
  float* cur = P->T[0];
  for (int k = 2; k <= pr.K; ++k) {
    sched_exchange(P, q, pr.scale, {{cur == P->T[0] ? B_T0 : B_T1, P->Fp}});
    const bool last = k == pr.K;
    float* other = cur == P->T[0] ? P->T[1] : P->T[0];
    float* nxt = last ? out : other;
    // the last hop of a large scale: a middle hop into the free ping-pong buffer, then
    // the epilogue on dense node tiles (not on parts: their schedules must stay equal)
    // (only an epilogue with MFMA work gains: a bare store of the layer's output costs a
    // whole extra pass over the rows)
    const bool mfma_epi = epi.np.a_u >= 0 || epi.np.a_v >= 0 || epi.np.a_o >= 0 || epi.uu_a >= 0 || epi.dec.on;
    const bool split = last && mfma_epi && P->part_rank < 0 && P->kn.epi_split_tiles > 0 &&
                       g.ntiles >= P->kn.epi_split_tiles;
    q.push_back(hop_launch(P, pr, k, cur, split ? other : nxt, last && !split, epi));
    if (split) q.push_back(epi_launch(P, pr, other, nxt, epi));
    cur = nxt;
  }
}

// Mean pooling into coarse scale s fused into the first launch of the processor on s
// (k_edge_coop with EdgeHopArgs::pool): F = 32, the scale small enough for the two-wave
// cooperative edge hop in one round (set_grid_cap's k_edge_coop rule), not on parts (their
// halo exchange sits between the two launches).  MSW_POOL_FUSE=0 keeps the pooling launch.
bool pool_fusable(const msw_plan* P, int s, const Proc& pr) {
  if (!P->kn.pool_fuse || P->no_fuse || (P->NT != 2 && P->NT != 4) || P->part_rank >= 0 || s <= 0 || s >= P->S) return false;
  const ScaleCSR& g = P->sc[s];
  // K > 1: the launch is not the layer's last hop (k_edge_coop runs no unpool / decoder epilogue)
  if (pr.scale != s || pr.K < 2 || edge_mlp_split(P, pr) || !P->lv[s - 1].pool_slots || g.ntiles <= 0)
    return false;
  // the scales the cooperative kernels take in one round (F = 32: two waves per tile; F = 64:
  // four, or two with two tiles per workgroup)
  return P->kn.coop_waves > 0 && 2L * g.ntiles <= std::min(P->kn.coop_waves, kWaves * kMaxFusedPoolBlocks);
}

// The unpooling layer into fine scale s fused into the first launch of the processor on s
// (k_edge_coop with PoolFuse::parent), as pool_fusable, F = 32 only (at F = 64 its 384-MFMA
// unpooling MLP per side outweighs the launch it saves: zenodo4_f64 -2.5 %,
// profiles/r03/ab_unpool_fuse_f64.txt); MSW_UNPOOL_FUSE=0 keeps the unpooling launch.
bool unpool_fusable(const msw_plan* P, int s, const Proc& pr, const Proc& up) {
  if (!P->kn.unpool_fuse || P->no_fuse || P->NT != 2 || P->part_rank >= 0 || s < 0 || s + 1 >= P->S) return false;
  const ScaleCSR& g = P->sc[s];
  if (pr.scale != s || pr.K < 2 || edge_mlp_split(P, pr) || !P->lv[s].parent_slots || g.ntiles <= 0) return false;
  if (up.h1t > 2 * P->NT || up.K != 1) return false;
  return P->kn.coop_waves > 0 && 2L * g.ntiles <= std::min(P->kn.coop_waves, kWaves * kMaxFusedPoolBlocks);
}

// One forward.  Forward mode: the encoder reads graph rows of x (via perm) and the decoder
// writes y (both patched per call); rollout mode: the internal state X is updated in place
// by the decoder epilogue.
void sched_step(msw_plan* P, std::vector<Launch>& q, bool rollout) {
  q.clear();
  const int S = P->S;
  const Common c = common_of(P);
  Launch LE;
  LE.kind = L_ENCODE;
  EncodeArgs& ea = LE.enc;
  ea.c = c;
  ea.x = rollout ? P->X : nullptr; ea.x_internal = rollout ? 1 : 0; ea.Npad = P->Npad; ea.S = S;
  for (int s = 0; s < S; ++s) {
    ea.n0[s] = P->sc[s].n0;
    ea.ns[s] = P->sc[s].ns;
    ea.vu_a[s] = -1;
  }
  ea.n0[S] = P->Npad;
  ea.stat = P->stat; ea.dynm = P->dynm; ea.xs = P->xs; ea.xd = P->xd0;
  ea.np0 = np_of(P, P->procs[0]);
  ea.io = rollout ? P->io_d : nullptr;
  ea.vu_h1t = 1;
  if (P->model_type == 0 && S > 1) {
    for (int l = 0; l < S - 1; ++l) ea.vu_a[l] = P->unpools[S - 2 - l].a_vu;  // level l <- intra_scale_gnn[S-2-l]
    ea.vu_h1t = P->unpools[0].h1t;
    ea.Vu = P->Vu;
  }
  const DecDesc dd = dec_of(P, rollout ? P->X : nullptr, rollout, nullptr);
  // rollout mode: the decoder of step t runs in the encoder launch of step t + 1 (and in a
  // final decode-only launch after the last step, msw_rollout); its input is the last
  // layer's output, stored by that layer's last hop (x_up rows / the GNN's last layer)
  // Deferred where the step is latency-bound (zenodo4 +3.2 %, the batch of 8 +1.8 %); on
  // meshes whose finest scale has >= kDeferMaxTiles edge tiles the decoder stays in the last
  // hops' row epilogue (config 5: -1.2 % deferred; profiles/r02_v3/ab_defer_decode.txt).
  // MSW_DEFER_DECODE=0/1 overrides.
  // Forward mode (msw_forward, the reference's own step loop): the decoder leaves the last
  // hops for one row-local launch after the schedule (k_decode_fwd), by the same size rule.
  bool defer = P->sc[0].ntiles < kDeferMaxTiles;
  if (P->kn.defer_decode >= 0) defer = P->kn.defer_decode != 0;
  if (!rollout && !P->xch.empty()) defer = false;  // parts of a split mesh: decoded in their last hops
  ea.dec = dd;
  ea.dec.on = defer && rollout ? 1 : 0;
  ea.dec_in = P->model_type == 0 ? P->xup : P->xgnn;
  ea.decode_only = 0;
  q.push_back(LE);
  DecDesc dl = dd;  // the last hops' decoder: forward mode, or rollout mode not deferred
  dl.on = defer ? 0 : 1;
  if (P->model_type == 0) {
    Epilogue none{};
    none.np = np_none(); none.uu_a = -1; none.dec.on = 0;
    PoolFuse fuse{};
    for (int i = 0; i < S - 1; ++i) {  // fine -> coarse
      sched_proc(P, q, P->procs[i], P->xdown, none, fuse.slots ? &fuse : nullptr);
      const LevelMaps& m = P->lv[i];
      fuse = PoolFuse{};
      if (pool_fusable(P, i + 1, P->procs[i + 1])) {  // the next processor's first launch pools
        fuse.slots = m.pool_slots; fuse.child = m.pool_child; fuse.in = P->xdown;
        fuse.np = np_of(P, P->procs[i + 1]);
        continue;
      }
      Launch L;
      L.kind = L_POOL;
      L.scale = i + 1;
      PoolArgs& pa = L.pool;
      pa.c = c; pa.n0 = P->sc[i + 1].n0; pa.ns = P->sc[i + 1].ns;
      pa.rtiles = (pa.ns + 15) / 16; pa.etiles = m.pool_etiles;
      pa.rows = 1; pa.ntiles = pa.rtiles;  // set_grid_cap picks the layout
      pa.recs = m.pool_recs; pa.erecs = m.pool_erecs; pa.child = m.pool_child;
      pa.in = P->xdown; pa.xs = P->xs;
      pa.np = np_of(P, P->procs[i + 1]);
      q.push_back(L);
    }
    PoolFuse ufuse{};
    for (int i = 0; i < S; ++i) {      // coarse -> fine
      const int j = S - 1 + i, s = S - 1 - i;
      Epilogue e{};
      e.np = np_none();
      e.uu_a = -1;
      if (s > 0) {
        const Proc& up = P->unpools[i];
        e.uu_a = up.a_u; e.uu_h1t = up.h1t; e.Uu = P->Uu;
      }
      e.dec = dl;  // every scale's rows are decoded once final (gnn.py:335-348)
      sched_proc(P, q, P->procs[j], P->xup, e, i == 0 && fuse.slots ? &fuse : ufuse.parent ? &ufuse : nullptr);
      ufuse = PoolFuse{};
      if (s > 0) {                      // intra_scale_gnn[i] on level s-1 (+ skip) + projection
        const Proc& up = P->unpools[i];
        const ScaleCSR& fs = P->sc[s - 1];
        const LevelMaps& m = P->lv[s - 1];
        if (unpool_fusable(P, s - 1, P->procs[j + 1], up)) {  // the next processor's first launch unpools
          ufuse.parent = m.parent_slots; ufuse.cpad = P->sc[s].n0;
          ufuse.Uu = P->Uu; ufuse.Vu = P->Vu; ufuse.xc = P->xup; ufuse.skip = P->skip ? P->xdown : nullptr;
          ufuse.b1_off = up.b1_off; ufuse.h1t = up.h1t; ufuse.act1 = up.act1; ufuse.slope1 = up.slope1;
          ufuse.rest = up.rest; ufuse.normalize = up.normalize; ufuse.grad = up.with_gradient;
          ufuse.upwind = up.upwind; ufuse.post_act = 0; ufuse.post_slope = 0.f;
          ufuse.np = np_of(P, P->procs[j + 1]);
          continue;
        }
        Launch L;
        L.kind = L_EDGE_HOP;
        L.scale = s - 1;
        EdgeHopArgs& eh = L.eh;
        eh.c = c; eh.c.prelu = P->prelu & up.prelu;
        eh.n0 = fs.n0; eh.recs = m.un_recs; eh.ntiles = m.un_ntiles;
        eh.xs = P->xs; eh.U = P->Uu; eh.V = P->Vu;
        eh.Pe = nullptr; eh.b1_off = up.b1_off; eh.h1t = up.h1t; eh.act1 = up.act1;
        eh.slope1 = up.slope1; eh.rest = up.rest; eh.normalize = up.normalize; eh.s = nullptr;
        eh.in = P->xup; eh.own_zero = 1; eh.grad = up.with_gradient; eh.upwind = up.upwind;
        eh.filt_a = -1; eh.skip = P->skip ? P->xdown : nullptr; eh.out = nullptr; eh.last = 1;
        eh.epi.np = np_of(P, P->procs[j + 1]); eh.epi.uu_a = -1; eh.epi.dec.on = 0;
        q.push_back(L);
      }
    }
  } else {
    const int L = (int)P->procs.size();
    for (int j = 0; j < L; ++j) {
      Epilogue e{};
      e.post_act = P->gnn_act; e.post_slope = P->gnn_slope;
      e.np = j + 1 < L ? np_of(P, P->procs[j + 1]) : np_none();
      e.uu_a = -1;
      if (j + 1 == L) e.dec = dl; else e.dec.on = 0;
      sched_proc(P, q, P->procs[j], P->xgnn, e);
    }
  }
  if (defer && !rollout) {  // forward mode: the deferred decoder, after everything else
    Launch LD;
    LD.kind = L_DECODE;
    LD.scale = 0;
    DecodeArgs& da = LD.dec;
    da.c = c;
    da.c.xcd_max = 0;
    da.Npad = P->Npad;
    da.in = ea.dec_in;
    da.dec = dd;
    da.dec.on = 1;
    q.push_back(LD);
  }
  if (defer && rollout)  // the step counter the next step's encoder reads advances here
    for (Launch& L : q)
      if (L.kind == L_EDGE_HOP || L.kind == L_EDGE_MLP) {
        L.eh.step_inc = &P->io_d->step;
        break;
      }
}

// ---------------------------------------------------------------------------- variants
// Grid cap of a grid-stride launch: the workgroups the chip holds at once, so that each
// stages its weight region once (large meshes) and none waits for a second wave of blocks.
// MSW_GRID_CAP=n (tests): at most n; 0 (the occupancy query failed) stays 0.
// The keys below are deliberate carry-overs where they name another instantiation than the one
// launched (the encoder asks about the non-decoding, non-streaming k_encode; a cooperative
// edge hop with fused (un)pooling about the unfused kernel; the row-layout hop has no region;
// a middle hop asks with its layer's region though it stages none): another key could move a
// size threshold.
int resident_of(const msw_plan* P, const VariantKey& k, int floats) {
  const int r = with_nt(P->NT, [&](auto nt) { return resident_blocks<nt>(k, floats); });
  return P->kn.grid_cap > 0 ? std::min(r, P->kn.grid_cap) : r;
}
// max_blocks / fit_blocks: the grid-stride and the one-tile-per-wave variant of key k
template <class A>
void caps(const msw_plan* P, A& a, VariantKey k, int floats) {
  k.loop = 1;
  a.max_blocks = resident_of(P, k, floats);
  k.loop = 0;
  a.fit_blocks = resident_of(P, k, floats);
}
// MSW_HOP_ROWS=2: every middle hop in the row layout, at any size (parity tests)
bool row_hops_forced(const msw_plan* P) { return P->kn.hop_rows == 2; }

// set_grid_cap, one function per launch kind: the residency figures of a launch and the
// variant choices that go by them (cooperative / split / row-layout / streaming / direct)
void cap_encode(const msw_plan* P, EncodeArgs& a) {
  a.max_blocks = resident_of(P, {K_ENCODE, a.c.prelu}, a.lds_floats);
  // F = 64: four waves per row tile while that leaves <= 4 waves per SIMD (k_encode_coop;
  // zenodo4_f64 +5.0 %; at F = 32 the halved chains are too short for the seven LDS
  // exchanges: -2.5 %; MSW_ENC_COOP=0/1 overrides)
  bool coop = P->NT == 4 && (long)(a.Npad / kRowsPerWave) * P->NT <= kEncCoopWaves;
  if (P->kn.enc_coop >= 0) coop = P->NT >= 2 && P->kn.enc_coop != 0;
  a.coop = coop ? P->NT : 0;
  // grid-stride (more 64-row chunks than resident workgroups) without the decoder: the
  // encoder's rows (config 5: 1.26 GB per launch) go out as streaming stores
  a.stream = !a.coop && !a.dec.on && a.max_blocks > 0 && a.Npad / kRowsPerBlock > a.max_blocks;
}
void cap_edge_mlp(const msw_plan* P, EdgeHopArgs& a) {
  // k_edge_mlp: two waves per SIMD, one chunk each.  (A software-pipelined variant, one wave
  // per SIMD walking ~2 chunks with the next chunk's gathers in flight, spilled once the
  // operands were LDS-typed and lost: zenodo4_f64 27.76 / 27.91 vs 28.08 / 28.09 M,
  // profiles/r04/ab_f64_lds_operands.txt; removed in round 6.)  Waves 4..7 start 2 x 2 k
  // cycles late (k_edge_mlp 22.0 -> 21.2 us, profiles/r05/ab_f64_mlp_stagger.txt).
  a.stagger = kMlpStagger;
  a.max_blocks = resident_of(P, {K_EDGE_MLP, a.c.prelu}, a.reg.len);
}
void cap_edge_hop(const msw_plan* P, EdgeHopArgs& a) {
  const int coop_waves = P->kn.coop_waves;
  // the grid-stride variant stages the whole region, one tile per wave keeps the filter in registers
  a.max_blocks = resident_of(P, {K_EDGE_HOP, a.c.prelu, a.last, 1}, a.reg.len);
  a.fit_blocks = resident_of(P, {K_EDGE_HOP, a.c.prelu, a.last, 0}, a.reg_nf);
  // MSW_EH_LOOP=1: the grid-stride variant at any size (parity tests of the large-mesh path)
  if (P->kn.eh_loop && a.max_blocks > 0 && a.ntiles > kWaves) a.fit_blocks = 1;
  // two waves per tile (k_edge_coop) while the tiles leave most SIMDs idle: one tile
  // per wave at most, no grid-stride loop, an epilogue of projections only
  const bool loop = tile_loop(a);
  const bool epi_ok = !a.last || (!a.epi.dec.on && a.epi.uu_a < 0);
  // ... and its grid resident at once (a second round of workgroups costs more than the
  // halved MLP chain saves: measured +4.7 us on the finest unpooling of zenodo4)
  // (F = 32: two waves per tile; F = 64: four, one tile per workgroup)
  const int pw = P->NT == 2 ? 2 : P->NT == 4 ? 4 : 0;
  const int coop_fit = pw ? resident_of(P, {K_EDGE_COOP, a.c.prelu, a.last, 0, pw}, a.reg_nf) : 0;
  a.coop = (pw && !loop && epi_ok && coop_waves > 0 && (long)pw * a.ntiles <= coop_waves &&
            (pw * a.ntiles + kWaves - 1) / kWaves <= coop_fit) ? pw : 0;
  // F = 64 where four waves per tile do not fit one round: two, two tiles per workgroup
  // (zenodo4_f64 scale 1: 508 tiles in one round, +2.0 %; MSW_COOP2_F64=0 off, =2 also in
  // place of four, for tests)
  // fused pooling exists in the cooperative kernels only (pool_fusable): F = 32 two waves
  // per tile; F = 64 four, or two where four do not fit one round (below)
  if ((a.pool.slots || a.pool.parent) && P->NT == 2) a.coop = 2;
  const int c2 = P->kn.coop2_f64;
  if (c2 == 2 && a.coop == 4) a.coop = 0;
  a.wdirect = 0;
  if (P->NT == 4 && !a.coop && !loop && epi_ok && coop_waves > 0 && 2L * a.ntiles <= coop_waves && c2) {
    const int need = (2 * a.ntiles + kWaves - 1) / kWaves;
    const int wd = P->kn.coop2_direct;
    const VariantKey two{K_EDGE_COOP, a.c.prelu, a.last, 0, 2};
    if (need <= resident_of(P, two, a.reg_nf)) {
      a.coop = 2;
      a.wdirect = wd == 2 && a.reg.len > 0;
    } else if (wd != 0 && a.reg.len > 0 && need <= resident_of(P, two, 0)) {
      // the staged MLP region (96 KB) holds one workgroup per CU: read it from its blob
      // copy instead, two workgroups per CU, and the grid fits one round (the finest
      // unpooling of zenodo4_f64: 652 tiles; MSW_COOP2_DIRECT=0 off)
      a.coop = 2;
      a.wdirect = 1;
    }
  }
  if ((a.pool.slots || a.pool.parent) && !a.coop) a.coop = 2;  // F = 64 fused: two waves per tile, any grid
}
void cap_hop(const msw_plan* P, Launch& L) {
  HopArgs& h = L.hop;
  caps(P, h, {K_HOP, h.c.prelu, h.last}, h.reg.len);
  // one tile per wave below kHopLoopTiles: the grid-stride variant measured 1.1-1.6 % slower on the batch of 8 and
  // dk15, equal on the 1M-node mesh whose finest hop alone it runs 3 % faster
  // (profiles/r01_v7/ab_edge_waves.txt)
  // (waived under MSW_GRID_CAP, whose point is the grid-stride variant on a small mesh)
  if (h.ntiles < kHopLoopTiles && P->kn.grid_cap <= 0) h.max_blocks = 0;
  {  // F = 64: feature-split middle hops below the grid-stride size (k_hop_split;
     // zenodo4_f64 +4.6 %, F = 32 neutral; MSW_HOP_SPLIT=0/1 overrides the rule)
    bool sp = P->NT == 4 && h.max_blocks == 0;
    if (P->kn.hop_split >= 0) sp = P->kn.hop_split != 0;
    h.split = (sp && P->NT >= 2 && !h.last) ? 1 : 0;
  }
  // row layout for the grid-stride middle hops of large scales (k_hop_rows)
  h.rows = 0;
  if (P->kn.hop_rows != 0 && !h.last && (tile_loop(h) || row_hops_forced(P)) && h.rptr && h.redge) {
    h.rows = 1;
    h.split = 0;
    h.max_blocks = resident_of(P, {K_HOP_ROWS}, 0);
    // ... streaming its stores by the encoder's size rule: more 64-row chunks than the chip holds
    // encoder workgroups (below, the next hop re-reads the rows from cache)
    int enc_floats = 0;
    for (const Launch& E : P->sched_fwd)
      if (E.kind == L_ENCODE) enc_floats = E.enc.lds_floats;
    const int enc_fit = resident_of(P, {K_ENCODE, P->prelu}, enc_floats);
    h.stream = enc_fit > 0 && P->Npad / kRowsPerBlock > enc_fit;
  }
  // dense row-tile hop where the scale has its records (dense_hops): middle hops, and a last
  // hop whose epilogue is the post-activation and the store -- on every scale: with the pooling
  // fused into the next scale's first launch, the down-processors' last hops of the coarser
  // scales have such an epilogue too, and leave k_hop_coop
  L.dense = P->sc[L.scale].drecs && !h.rows && !tile_loop(h) && (!h.last || bare_epilogue(h.epi));
  if (L.dense) h.split = 0;
  // a last hop with an epilogue on few tiles: P = F / 16 waves per tile (k_hop_coop)
  const int pw = P->NT >= 2 ? P->NT : 0;
  h.coop = 0;
  if (h.last && !L.dense && pw && !tile_loop(h) && P->kn.coop_waves > 0 && (long)pw * h.ntiles <= P->kn.coop_waves &&
      (pw * h.ntiles + kWaves - 1) / kWaves <= resident_of(P, {K_HOP_COOP, h.c.prelu, 1, 0, pw}, h.reg.len))
    h.coop = pw;
}
void cap_pool(const msw_plan* P, PoolArgs& a) {
  // edge tiles while they all fit on the chip at once (latency-bound launch), else rows
  const int fe = resident_of(P, {K_POOL_EDGE}, a.reg.len);
  a.rows = !(fe > 0 && (a.etiles + kWaves - 1) / kWaves <= fe);
  a.ntiles = a.rows ? a.rtiles : a.etiles;
  caps(P, a, {K_POOL_ROWS}, a.reg.len);
  // two waves per edge tile (projection split) while that grid too is resident at once
  // (F = 32: two waves per tile, F = 64: four)
  const int pw = P->NT >= 2 ? P->NT : 0;
  a.coop = (!a.rows && pw && P->kn.coop_waves > 0 && (long)pw * a.etiles <= P->kn.coop_waves &&
            (pw * a.etiles + kWaves - 1) / kWaves <= fe) ? pw : 0;
  // 2F-wide first edge-MLP layer: 2 * F / 16 waves per tile (one U and one V output tile
  // each) while resident (zenodo4_f64 +1.8 %, zenodo4 +0.6 %, profiles/r02_s4/ab_pool_p8.txt,
  // ab_pool_wide_f32.txt); MSW_POOL_WIDE=0: F / 16 waves; bit-identical either way
  const bool wide = P->kn.pool_wide != 0;
  if (wide && pw && a.coop == pw && a.np.h1t == 2 * pw) {
    const int f8 = resident_of(P, {K_POOL_EDGE, 0, 0, 0, 2 * pw}, a.reg.len);
    if (f8 > 0 && a.etiles <= f8) a.coop = 2 * pw;
  }
}
void set_grid_cap(const msw_plan* P, Launch& L) {
  // XCD packing (Common::xcd_max) applies to the hop, edge-hop, pooling and row-epilogue
  // launches (the only one-round grids small enough to fit one XCD)
  if (L.kind != L_HOP && L.kind != L_EDGE_HOP && L.kind != L_POOL && L.kind != L_EPI) L.common().xcd_max = 0;
  switch (L.kind) {
    case L_ENCODE: return cap_encode(P, L.enc);
    case L_EDGE_MLP: return cap_edge_mlp(P, L.eh);
    case L_EDGE_HOP: return cap_edge_hop(P, L.eh);
    case L_HOP: return cap_hop(P, L);
    case L_EPI: return caps(P, L.ep, {K_EPI, L.ep.c.prelu, 1}, L.ep.reg.len);
    case L_POOL: return cap_pool(P, L.pool);
    default: return;  // exchanges and the forward decoder have no grid to cap
  }
}

// The first cooperative edge hop whose staged weight region exceeds the dynamic LDS
// prepare_kernels allowed its kernel (edge_coop_lds_cap), or nullptr.
const Launch* lds_overflow(const msw_plan* P) {
  for (const auto* q : {&P->sched_fwd, &P->sched_roll})
    for (const Launch& L : *q) {
      if (L.kind != L_EDGE_HOP || !(L.eh.coop == 2 || L.eh.coop == 4) || L.eh.wdirect) continue;
      const int fuse = L.eh.pool.slots ? 1 : L.eh.pool.parent ? 2 : 0;
      const int cap = with_nt(P->NT, [&](auto nt) { return edge_coop_lds_cap<nt>(L.eh.coop, fuse); });
      if (eh_lds_bytes(L.eh.reg_nf) > (size_t)cap) return &L;
    }
  return nullptr;
}

}  // namespace

bool msw::dense_hops(const msw_plan* P, const ScaleCSR& c) {
  if (P->NT > 2 || P->part_rank >= 0 || P->kn.grid_cap > 0 || P->kn.hop_dense == 0) return false;
  if (row_hops_forced(P) || (P->kn.hop_split > 0 && P->NT >= 2)) return false;  // those switches force their kernels
  const int nt = cdiv(c.ns, kRowsPerWave);
  if (nt <= 0 || c.ntiles <= 0 || nt > kDenseMaxTiles) return false;
  return nt <= resident_of(P, {K_HOP_DENSE, P->prelu, 1}, 0);  // one-wave workgroups
}

int msw::row_hop_min_tiles(const msw_plan* P) {
  return row_hops_forced(P) || P->kn.grid_cap > 0 ? 0 : kRowHopMinTiles;
}

// The launch schedules (forward / rollout), their per-launch weight regions and variant
// choices; the regions are appended to P->blob.
int msw::build_schedules(msw_plan* P) {
  const size_t blob0 = P->blob.h.size();
  for (;;) {
    sched_step(P, P->sched_fwd, false);
    sched_step(P, P->sched_roll, true);
    const bool mlp_only = P->NT > 2;  // F = 64: only the edge-MLP operands fit in LDS
    int rc;
    if ((rc = relocate(P, P->sched_fwd, mlp_only)) || (rc = relocate(P, P->sched_roll, mlp_only))) return rc;
    for (auto* q : {&P->sched_fwd, &P->sched_roll})
      for (Launch& L : *q) set_grid_cap(P, L);
    // every cooperative edge hop's staged region must fit the LDS its kernel was given; a
    // fused (un)pooling launch that does not (e.g. F = 32 with mlp_layers = 4: two edge MLPs
    // + the projection) falls back to the separate pooling / unpooling launches
    const Launch* bad = lds_overflow(P);
    if (!bad) return MSW_OK;
    if (P->no_fuse || !(bad->eh.pool.slots || bad->eh.pool.parent))
      return fail(MSW_ERR_UNSUPPORTED, "weights of a cooperative edge hop exceed its LDS budget (" +
                                           std::to_string(eh_lds_bytes(bad->eh.reg_nf)) + " B)");
    P->no_fuse = 1;
    P->blob.h.resize(blob0);  // drop the regions of the fused schedule
  }
}
