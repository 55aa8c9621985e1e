// Internal header of the host side of the C ABI (include/mswegnn.h): the plan's data model
// and the few functions that cross its translation units.
//
//   weights.hip   where an operand lies: weight packing, per-launch weight regions
//   schedule.hip  what a step launches: the schedule, the variant and residency rules
//   runtime.hip   running it: halo transports, dispatch, graph capture, forward / rollout
//   plan.hip      plan creation / destruction and the plan's queries
#pragma once
#include <rccl/rccl.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/mswegnn.h"
#include "engine.h"

namespace msw {

inline int fail(int code, const std::string& msg) { return set_error(code, msg.c_str()); }

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess)                                                               \
      return fail(MSW_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
  } while (0)

// The packed weights of a plan (weights.hip fills it, the kernels read its device copy).
struct Blob {
  std::vector<float> h;
  int alloc(size_t n) {  // 64-float (256 B) aligned chunk
    size_t off = (h.size() + 63) / 64 * 64;
    h.resize(off + n, 0.f);
    return (int)off;
  }
};

// The one dispatch on a plan's width: f(std::integral_constant<int, NT>) for NT = 1, 2, 4.
template <class F>
auto with_nt(int NT, F&& f) {
  switch (NT) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

inline hipError_t rowmlp_dispatch(int NT, const RowMlpArgs& ra, hipStream_t st = nullptr) {
  return with_nt(NT, [&](auto nt) { return launch_rowmlp<nt>(ra, st); });
}

}  // namespace msw

// ============================================================================ plan
struct ScaleCSR {
  int n0 = 0, ns = 0;           // internal rows [n0, n0+ns) (n0 is a multiple of 16)
  int E = 0;                    // edges of this scale
  msw::LaneRec* recs = nullptr;      // [ntiles][16]
  int ntiles = 0;
  msw::EdgeChunk* chunks = nullptr;  // [nchunks][16] dense edge chunks (k_edge_mlp)
  int nchunks = 0;
  int* rptr = nullptr;          // row-layout middle hops (k_hop_rows, large scales): CSR by
  int2* redge = nullptr;        // destination, {source row, s slot} per edge
  msw::DenseRec* drecs = nullptr;    // dense row-tile hops (k_hop_dense, latency-bound scales): inline
  int* dptr = nullptr;          // in-edge records per destination row, and the CSR by destination
  int2* dedge = nullptr;        // for rows past the inline record (plan.hip upload_dense)

  std::vector<int> porig;      // tile-padded edge slot -> original edge id, -1 = padding
  std::vector<msw::LaneRec> hrecs;   // host copy of recs (fused pooling slots, PoolSlot)
};

struct LevelMaps {              // level l: coarse scale l+1, fine scale l
  int I = 0;
  msw::PoolRec* pool_recs = nullptr; // per coarse row (scale l+1): its children (engine.h PoolRec)
  msw::LaneRec* pool_erecs = nullptr; // edge tiles of coarse nodes and their children (<= 16 per tile)
  int pool_etiles = 0;
  int* pool_child = nullptr;    // internal fine rows, reference order
  msw::PoolSlot* pool_slots = nullptr; // per edge slot of the coarse scale: children of its source /
                                  // destination (pooling fused into the coarse edge hop)
  int2* parent_slots = nullptr;   // per edge slot of the fine scale: parents of its source /
                                  // destination (unpooling fused into the fine edge hop)
  msw::LaneRec* un_recs = nullptr;   // fine nodes (scale l) and their coarse parents
  int un_ntiles = 0;
};

struct Proc {                   // one SWEGNN layer bound to a scale (or an intra level)
  int scale = 0;
  int K = 0, normalize = 1, with_filter = 1, with_gradient = 1, upwind = 0;
  int h1t = 1;
  int a_u = -1, a_v = -1, a_o = -1;  // projection operands ([x_s | x_d] -> U, V, O)
  int a_vu = -1;                // intra layers: V from x_s only (fine rows)
  float* Pe = nullptr;          // [E][16*h1t] (layers with edge features)
  int b1_off = -1;              // bias of the first edge-MLP layer
  int act1 = 0;
  float slope1 = 0.f;
  msw::MlpDev rest{};           // layers 2..L
  std::vector<int> filt;        // packed filters 1..K
  int prelu = 0;
  int par = 0;                  // buffer set (execution index & 1)
};

// One kernel launch of a step, arguments fixed at plan time (forward mode patches the
// input / output pointers per call).
enum LaunchKind { L_ENCODE, L_EDGE_HOP, L_HOP, L_POOL, L_EXCHANGE, L_EPI, L_EDGE_MLP, L_DECODE };

// Halo exchange before a gathering launch (partitioned meshes, msw_plan_create_part):
// refresh the halo rows of up to two of the plan's buffers on one scale.
enum BufId { B_U0, B_U1, B_O0, B_O1, B_T0, B_T1 };
struct ExchangeArgs {
  msw::Common c;
  int scale;
  int nbuf;
  int buf[2];    // BufId
  int width[2];  // floats per row
};
struct Launch {
  int kind;
  int scale;                    // destination scale (bench hook)
  int dense;                    // L_HOP: runs as the dense row-tile hop (k_hop_dense, DenseHopArgs
                                // formed at launch from the hop's arguments and the scale's records)
  union {
    msw::EncodeArgs enc;
    msw::EdgeHopArgs eh;
    msw::HopArgs hop;
    msw::PoolArgs pool;
    ExchangeArgs xch;
    msw::EpiArgs ep;
    msw::DecodeArgs dec;
  };
  Launch() { memset((void*)this, 0, sizeof(*this)); }
  // f(the argument struct of this launch's kind)
  template <class L, class F>
  static decltype(auto) visit(L& l, F&& f) {
    switch (l.kind) {
      case L_ENCODE: return f(l.enc);
      case L_EDGE_HOP:
      case L_EDGE_MLP: return f(l.eh);
      case L_HOP: return f(l.hop);
      case L_EXCHANGE: return f(l.xch);
      case L_EPI: return f(l.ep);
      case L_DECODE: return f(l.dec);
      default: return f(l.pool);
    }
  }
  msw::Common& common() {
    return visit(*this, [](auto& a) -> msw::Common& { return a.c; });
  }
  const msw::Common& common() const {
    return visit(*this, [](const auto& a) -> const msw::Common& { return a.c; });
  }
};

// Engine switches: read ONCE per plan (knobs_from_env) from MSW_* environment variables.
// Defaults are the measured-best settings; every switch flips a schedule between variants
// that are bit-identical (each has a -m gpu test that flips it), so a stray variable can
// change speed, never results.  bench.py records the MSW_* variables of its process.
struct Knobs {
  int split_edge_mlp = -1;  // MSW_SPLIT_EDGE_MLP  F = 64 split edge MLP: -1 size rule, 0 / 1 force
  int pool_fuse = 1;        // MSW_POOL_FUSE       mean pooling fused into the coarse first launch
  int unpool_fuse = 1;      // MSW_UNPOOL_FUSE     F = 32 unpooling fused into the fine first launch
  int defer_decode = -1;    // MSW_DEFER_DECODE    decoder in the next step's encoder: -1 size rule
  int hop_rows = -1;        // MSW_HOP_ROWS        row-layout middle hops: -1 size rule, 0 off, 2 all
  int coop2_direct = 1;     // MSW_COOP2_DIRECT    F = 64 two-wave edge hop, blob-read MLP: 0 / 1 / 2
  int coop2_f64 = 1;        // MSW_COOP2_F64       F = 64 two-wave edge hops: 0 off, 2 also for four
  int enc_coop = -1;        // MSW_ENC_COOP        cooperative encoder: -1 size rule, 0 / 1 force
  int eh_loop = 0;          // MSW_EH_LOOP         grid-stride fused edge hops at any size
  int hop_split = -1;       // MSW_HOP_SPLIT       feature-split middle hops: -1 = F = 64 rule
  int hop_dense = 1;        // MSW_HOP_DENSE       dense row-tile hops of latency-bound scales (F <= 32), 0 off
  int pool_wide = 1;        // MSW_POOL_WIDE       2F / 16 waves per pooling tile
  int tile_pack = 1;        // MSW_TILE_PACK       degree-aware destination order
  int xcd_max = 1;          // MSW_XCD_MAX         XCD packing of small grids (0 = all eight XCDs)
  int coop_waves = -1;      // MSW_COOP_WAVES      cooperative kernels while P x tiles <= this (-1 default)
  int epi_split_tiles = -1; // MSW_EPI_SPLIT_TILES row-epilogue threshold in edge tiles (-1 default)
  int trace_encode = 0;     // MSW_TRACE_ENCODE    diagnostic builds (-DMSW_TRACE): encoder marks only
  // A test switch, not a tuning switch: every residency figure of this plan (resident_of) is
  // clamped to n workgroups and the rules that go by absolute tile count (kHopLoopTiles,
  // kRowHopMinTiles) are waived, so a small mesh gets, launch for launch, the schedule of a mesh
  // too large for an n-workgroup chip -- every grid-stride kernel then makes several
  // iterations per wave (tests/test_gpu_gridstride.py).  Off when unset or <= 0.
  int grid_cap = 0;         // MSW_GRID_CAP        resident-grid cap in workgroups (tests)
};
// The switches of a plan of width NT = Fp / 16, every "-1 means the default" of a threshold
// resolved here and nowhere else: after this, coop_waves, epi_split_tiles and xcd_max are
// the values the rules go by.
inline Knobs knobs_from_env(int NT) {
  Knobs k;
  const struct { const char* name; int* v; } tab[] = {
      {"MSW_SPLIT_EDGE_MLP", &k.split_edge_mlp}, {"MSW_POOL_FUSE", &k.pool_fuse},
      {"MSW_UNPOOL_FUSE", &k.unpool_fuse}, {"MSW_DEFER_DECODE", &k.defer_decode}, {"MSW_HOP_ROWS", &k.hop_rows},
      {"MSW_COOP2_DIRECT", &k.coop2_direct}, {"MSW_COOP2_F64", &k.coop2_f64}, {"MSW_ENC_COOP", &k.enc_coop},
      {"MSW_EH_LOOP", &k.eh_loop},
      {"MSW_HOP_SPLIT", &k.hop_split}, {"MSW_HOP_DENSE", &k.hop_dense}, {"MSW_POOL_WIDE", &k.pool_wide}, {"MSW_TILE_PACK", &k.tile_pack},
      {"MSW_XCD_MAX", &k.xcd_max}, {"MSW_COOP_WAVES", &k.coop_waves},
      {"MSW_EPI_SPLIT_TILES", &k.epi_split_tiles}, {"MSW_TRACE_ENCODE", &k.trace_encode},
      {"MSW_GRID_CAP", &k.grid_cap}};
  for (const auto& t : tab)
    if (const char* e = getenv(t.name)) *t.v = atoi(e);
  // Cooperative kernels (several waves per tile: edge hop, last hop, pooling) while
  // waves-per-tile x tiles <= coop_waves (0: never).  F = 64: four-wave cooperative kernels on
  // every scale whose grid stays resident (zenodo4_f64 +3.3 %, profiles/r02_v1/ab_coop_f64.txt);
  // F = 32 keeps 1024 (no gain above)
  if (k.coop_waves < 0) k.coop_waves = NT == 4 ? 4096 : 1024;
  // A layer's last hop on a scale with at least this many edge tiles runs as a middle hop
  // + a row epilogue launch (engine.h EpiArgs; 0: never).  Measured on MI355X
  // (profiles/r01_v7/ab_epi_split.txt).
  if (k.epi_split_tiles < 0) k.epi_split_tiles = 8192;
  // small one-round grids on at most this many XCDs (engine.h Common::xcd; 0 = all eight,
  // more than eight means eight)
  k.xcd_max = std::min(std::max(0, k.xcd_max), msw::kXcds);
  return k;
}

struct msw_plan {
  int device = 0;
  // F: the model's hid_features -- only where the model's tensors are indexed (weight packing,
  // the width checks, msw_debug_buffer).  Fp = 16 NT: the row width every buffer, stride,
  // exchange row, LDS budget and kernel sees; Fp > F (33..63 -> 64) runs zero-padded.
  int F = 32, Fp = 32;
  int model_type = 0, NT = 2, S = 1, p = 3, nnf = 8, dyn = 6, nstat_raw = 2;
  int with_wl = 1, skip = 1;
  int N = 0, Npad = 0;
  int64_t E = 0;
  std::vector<int> perm, iperm;  // internal -> graph (-1 padding), graph -> internal
  std::vector<ScaleCSR> sc;
  std::vector<LevelMaps> lv;
  std::vector<Proc> procs, unpools;
  msw::MlpDev stat{}, dynm{}, dec{}, edge_enc{};
  int gnn_act = 0;
  float gnn_slope = 0.f;
  int resw_off = -1;
  int prelu = 0;
  msw::Blob blob;
  float* dW = nullptr;
  int* perm_d = nullptr;
  int* bc_slot_d = nullptr;
  float* zrow_d = nullptr;
  std::vector<int> bc_rows_set;
  msw::RolloutIO* io_d = nullptr;
  // Edge terms of the processors' first edge-MLP layer (edge encoder, gnn.py:281-282, then
  // Pe = W1[:, 4F:] . enc + b1 per processor): static for a graph, computed at plan creation
  // for msw_forward and recomputed at the start of every msw_rollout (edge_jobs, in order).
  std::vector<msw::RowMlpArgs> edge_jobs;
  // O / U / V of consecutive SWEGNN layers alternate between two sets (Proc::par): the
  // last hop of layer j reads O[j&1] (K = 1: also U/V[j&1]) while its epilogue writes the
  // projection of layer j+1.  T[0] / T[1] carry the intermediate hops.
  float *X = nullptr, *xs = nullptr, *xd0 = nullptr;
  float *O[2] = {nullptr, nullptr}, *T[2] = {nullptr, nullptr};
  float *xdown = nullptr, *xup = nullptr, *xgnn = nullptr;
  float *U[2] = {nullptr, nullptr}, *V[2] = {nullptr, nullptr};
  float *Uu = nullptr, *Vu = nullptr, *s = nullptr;
  int h1t_max = 1;
  int64_t dev_bytes = 0;
  int64_t forward_calls = 0, rollout_steps = 0;
  // RCCL transport: ncclSend / ncclRecv calls issued (eagerly or into a captured graph) and
  // rollout steps whose halo exchanges ran over RCCL (eager steps and graph replays)
  int64_t rccl_calls = 0, rccl_steps = 0;
  int kernels_per_step = 0;
  std::vector<Launch> sched_fwd, sched_roll;  // one forward step: forward / rollout mode
  int use_graph = 1;
  // partitioned mesh (msw_plan_create_part): per scale, the halo rows received from / the
  // owned rows sent to each peer (internal rows, concatenated in peer order)
  struct XchScale {
    int nrecv = 0, nsend = 0;
    int* recv_rows = nullptr;
    int* send_rows = nullptr;
    std::vector<msw::XchPeer> peers;
  };
  int part_rank = -1;
  std::vector<XchScale> xch;
  ncclComm_t comm = nullptr;
  float *xsend = nullptr, *xrecv = nullptr;
  hipStream_t cap_stream = nullptr;
  hipGraphExec_t step_exec = nullptr;   // one rollout step
  hipGraphExec_t multi_exec = nullptr;  // graph_steps consecutive steps (one graph launch)
  // Forward mode (msw_forward, the reference's own rollout loop calls it once per step): the
  // forward schedule captured once with fixed device I/O slots; a call copies x into fwd_x,
  // replays the graph and copies fwd_y out -- three stream operations instead of ~35 eager
  // launches (host-launch-bound at ~3.5 us each).
  hipGraphExec_t fwd_exec = nullptr;
  float *fwd_x = nullptr, *fwd_y = nullptr;
  // Steps per graph launch: consecutive launches of one graph leave a ~8.5 us gap on the
  // device (measured, rocprofv3 step breakdown), inside a graph the steps run back to back.
  int graph_steps = 16;
  Knobs kn;                 // engine switches of this plan, resolved (knobs_from_env)
  // set when a fused (un)pooling launch's weight region would not fit its kernel's LDS cap
  // (edge_coop_lds_cap): the schedule is rebuilt with the pooling / unpooling launches
  int no_fuse = 0;
  std::vector<void*> owned;
  // In-process group of partitioned plans (msw_group_rollout): the group's steps captured as
  // graphs too (every part's launches and the halo copies between their buffers), held by the
  // group's plan 0 and keyed by the members' identities and graph generations
  uint64_t uid = 0;              // unique per plan created in this process
  int graph_gen = 0;             // advanced whenever this plan's captured arguments go stale
  int group_graph = 1;           // msw_set_graph_capture(plans[0], 0): the group steps eagerly
  hipGraphExec_t group_one = nullptr, group_multi = nullptr;
  std::vector<uint64_t> group_key;
  void drop_group_graphs() {
    if (group_one) (void)hipGraphExecDestroy(group_one);
    if (group_multi) (void)hipGraphExecDestroy(group_multi);
    group_one = group_multi = nullptr;
    group_key.clear();
  }
  void drop_graphs() {
    if (step_exec) (void)hipGraphExecDestroy(step_exec);
    if (multi_exec) (void)hipGraphExecDestroy(multi_exec);
    if (fwd_exec) (void)hipGraphExecDestroy(fwd_exec);
    step_exec = multi_exec = fwd_exec = nullptr;
    drop_group_graphs();
    ++graph_gen;
  }
  ~msw_plan();  // runtime.hip (the RCCL communicator goes through the loader there)
};

namespace msw {

template <class T>
int palloc(msw_plan* P, T** p, size_t n) {
  if (n == 0) n = 1;
  HIP_TRY(hipMalloc((void**)p, n * sizeof(T)));
  P->dev_bytes += (int64_t)(n * sizeof(T));
  P->owned.push_back(*p);
  return MSW_OK;
}
template <class T>
int pupload(msw_plan* P, T** p, const std::vector<T>& v) {
  int rc = palloc(P, p, v.size());
  if (!rc && !v.empty()) HIP_TRY(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return rc;
}
// host I2 pairs (graph_build.h) into a device int2 array (same layout)
inline int pupload(msw_plan* P, int2** p, const std::vector<I2>& v) {
  static_assert(sizeof(I2) == sizeof(int2), "I2 mirrors int2");
  int rc = palloc(P, p, v.size());
  if (!rc && !v.empty()) HIP_TRY(hipMemcpy(*p, v.data(), v.size() * sizeof(I2), hipMemcpyHostToDevice));
  return rc;
}

// What launch_one launches (engine.h Pick), and msw_plan_schedule prints.  Inline: the eager
// launch path (runtime.hip launch_one) makes no cross-unit call of the plan's own.
template <int NT>
Pick pick_one(const Launch& L) {
  switch (L.kind) {
    case L_ENCODE: return pick_encode<NT>(L.enc);
    case L_EDGE_HOP: return pick_edge_hop<NT>(L.eh);
    case L_EDGE_MLP: return pick_edge_mlp<NT>(L.eh);
    case L_HOP: return L.dense ? pick_hop_dense<NT>(L.hop) : pick_hop<NT>(L.hop);
    case L_POOL: return pick_pool<NT>(L.pool);
    case L_EPI: return pick_epi<NT>(L.ep);
    case L_DECODE: return pick_decode<NT>(L.dec);
    default: return Pick{};
  }
}
inline Pick pick_one(const msw_plan* P, const Launch& L) {
  return with_nt(P->NT, [&](auto nt) { return pick_one<nt>(L); });
}

// weights.hip
// The model's weights packed into P->blob, its layers into P->procs / P->unpools (ef_raw: the
// graph's raw edge features).
int pack_model(msw_plan* P, const msw_model_desc* m, int ef_raw);
// Pe = W1[:, 4F:4F+feat_dim] . feat + b1 of a processor's first edge-MLP layer L1, as one
// NT -> 2 NT row-MLP layer packed into `tb`.
MlpDev pack_edge_term(const msw_plan* P, Blob& tb, const msw_linear& L1, int feat_dim);
// The operands each launch of q reads, copied into a contiguous blob region of its own.
int relocate(msw_plan* P, std::vector<Launch>& q, bool mlp_only);

// schedule.hip
// The scale runs its hops as dense row-tile hops (k_hop_dense).
bool dense_hops(const msw_plan* P, const ScaleCSR& c);
// Edge tiles from which build_host_graph gives a scale the row-layout CSR (0: every scale).
int row_hop_min_tiles(const msw_plan* P);
// P->sched_fwd and P->sched_roll with their weight regions and variant choices.
int build_schedules(msw_plan* P);

}  // namespace msw
