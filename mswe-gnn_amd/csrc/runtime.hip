// Running a plan: the RCCL loader and the two halo transports, the eager launch path
// (launch_one, schedule_dispatch), graph capture and replay (G steps per hipGraph launch, the
// remainder one step per launch), msw_forward / msw_rollout / msw_group_rollout, the kernel
// bench hook and tracing.  launch_one, schedule_dispatch and their callers stay in this one
// unit: the eager path costs ~3.5 us per launch on the host.
//
// Reference semantics followed (sdat2/mSWE-GNN): rollout_test training/train.py:67-95,
// update_batch_multiscale training/train.py:31-65 (batched node_ptr layout).
#include <dlfcn.h>

#include "plan.h"

using namespace msw;

namespace {

// RCCL, bound at run time: the copy already in the process (PyTorch's) or librccl.so.1.
struct RcclApi {
  ncclResult_t (*getUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*commInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*commDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*groupStart)() = nullptr;
  ncclResult_t (*groupEnd)() = nullptr;
  ncclResult_t (*send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  const char* (*errStr)(ncclResult_t) = nullptr;
  bool ok = false;
};
RcclApi& rccl() {
  static RcclApi api = [] {
    RcclApi a;
    void* h = RTLD_DEFAULT;
    if (!dlsym(h, "ncclSend")) {
      h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
      if (!h) return a;
    }
    a.getUniqueId = (decltype(a.getUniqueId))dlsym(h, "ncclGetUniqueId");
    a.commInitRank = (decltype(a.commInitRank))dlsym(h, "ncclCommInitRank");
    a.commDestroy = (decltype(a.commDestroy))dlsym(h, "ncclCommDestroy");
    a.groupStart = (decltype(a.groupStart))dlsym(h, "ncclGroupStart");
    a.groupEnd = (decltype(a.groupEnd))dlsym(h, "ncclGroupEnd");
    a.send = (decltype(a.send))dlsym(h, "ncclSend");
    a.recv = (decltype(a.recv))dlsym(h, "ncclRecv");
    a.errStr = (decltype(a.errStr))dlsym(h, "ncclGetErrorString");
    a.ok = a.getUniqueId && a.commInitRank && a.commDestroy && a.groupStart && a.groupEnd && a.send &&
           a.recv && a.errStr;
    return a;
  }();
  return api;
}

}  // namespace

msw_plan::~msw_plan() {
  drop_graphs();
  if (comm && rccl().ok) (void)rccl().commDestroy(comm);
  if (cap_stream) (void)hipStreamDestroy(cap_stream);
  for (void* q : owned) (void)hipFree(q);
}

namespace {

hipError_t launch_one(const msw_plan* P, const Launch& L, hipStream_t st) {
  if (L.kind == L_EXCHANGE) return hipErrorInvalidValue;  // run by schedule_dispatch / the group driver
  if (L.kind == L_HOP && L.dense) {  // k_hop_dense takes its own arguments
    const ScaleCSR& c = P->sc[L.scale];
    return launch_pick(pick_one(P, L), dense_args(L.hop, c.drecs, c.dptr, c.dedge), st);
  }
  return Launch::visit(L, [&](const auto& args) { return launch_pick(pick_one(P, L), args, st); });
}

float* buf_of(msw_plan* P, int id) {
  float* const b[] = {P->U[0], P->U[1], P->O[0], P->O[1], P->T[0], P->T[1]};  // BufId order
  return b[id >= B_U0 && id < B_T1 ? id : B_T1];
}

// RCCL transport: pack the rows every peer needs into one staging buffer, one grouped
// send/recv per peer, unpack into the halo rows.  Stream-ordered (capturable).
int rccl_exchange(msw_plan* P, const ExchangeArgs& a, hipStream_t st) {
  const msw_plan::XchScale& X = P->xch[a.scale];
  if (!P->comm) return fail(MSW_ERR_INVALID, "partitioned plan without a transport (msw_plan_set_comm)");
  RcclApi& r = rccl();
  for (int b = 0; b < a.nbuf; ++b) {
    float* buf = buf_of(P, a.buf[b]);
    const int w = a.width[b];
    HIP_TRY(launch_copy_rows(buf, X.send_rows, P->xsend, nullptr, X.nsend, w, st));
    ncclResult_t e = r.groupStart();
    for (const auto& pe : X.peers) {
      if (e == ncclSuccess && pe.scount > 0 &&
          (e = r.send(P->xsend + (size_t)pe.soff * w, (size_t)pe.scount * w, ncclFloat32, pe.peer, P->comm, st)) ==
              ncclSuccess)
        ++P->rccl_calls;
      if (e == ncclSuccess && pe.rcount > 0 &&
          (e = r.recv(P->xrecv + (size_t)pe.roff * w, (size_t)pe.rcount * w, ncclFloat32, pe.peer, P->comm, st)) ==
              ncclSuccess)
        ++P->rccl_calls;
    }
    const ncclResult_t e2 = r.groupEnd();
    if (e != ncclSuccess || e2 != ncclSuccess)
      return fail(MSW_ERR_HIP, std::string("RCCL halo exchange: ") + r.errStr(e != ncclSuccess ? e : e2));
    HIP_TRY(launch_copy_rows(P->xrecv, nullptr, buf, X.recv_rows, X.nrecv, w, st));
  }
  return MSW_OK;
}

int schedule_dispatch(msw_plan* P, const std::vector<Launch>& q, hipStream_t st) {
  for (const Launch& L : q) {
    if (L.kind == L_EXCHANGE) {
      int rc = rccl_exchange(P, L.xch, st);
      if (rc) return rc;
    } else {
      HIP_TRY(launch_one(P, L, st));
    }
  }
  P->kernels_per_step = (int)q.size();
  return MSW_OK;
}

// After a rollout's last step: the decoder of that step (the encoder launch of the rollout
// schedule with decode_only set: no encoders run).
int final_decode(msw_plan* P, hipStream_t st) {
  if (P->sched_roll.empty() || P->sched_roll[0].kind != L_ENCODE || !P->sched_roll[0].enc.dec.on)
    return MSW_OK;
  Launch L = P->sched_roll[0];
  L.enc.decode_only = 1;
  if (P->kn.trace_encode) L.enc.c.trace = nullptr;  // keep the last step's encoder marks
  HIP_TRY(launch_one(P, L, st));
  return MSW_OK;
}

// Forward mode: point the encoder at x (graph rows) and the decoder at x / y.
void patch_forward(std::vector<Launch>& q, const float* x, float* y) {
  for (Launch& L : q) {
    if (L.kind == L_ENCODE) L.enc.x = x;
    if (L.kind == L_DECODE) {
      L.dec.dec.X = x;
      L.dec.dec.y = y;
    }
    if (L.kind == L_EDGE_MLP) continue;  // carries its layer's epilogue and does not run it
    Launch::visit(L, [&](auto& a) {
      using A = std::decay_t<decltype(a)>;
      if constexpr (std::is_same_v<A, EdgeHopArgs> || std::is_same_v<A, HopArgs> || std::is_same_v<A, EpiArgs>)
        if (a.epi.dec.on) {
          a.epi.dec.X = x;
          a.epi.dec.y = y;
        }
    });
  }
}

// Re-launch one kernel of the rollout schedule (first of its kind on `scale`), with its
// rollout side effects removed: no epilogue (the output goes to a scratch buffer), no
// rollout step advance.
int bench_kernel(msw_plan* P, int kernel, int scale, int iters, int64_t* units, hipStream_t st) {
  if (scale < 0 || scale >= P->S) return fail(MSW_ERR_INVALID, "scale out of range");
  if (P->sched_roll.empty()) return fail(MSW_ERR_INVALID, "run a rollout before bench_kernel");
  static const int kind_of[] = {L_HOP, L_EDGE_HOP, L_POOL, L_ENCODE, L_EDGE_HOP};
  if (kernel < 0 || kernel > 4) return fail(MSW_ERR_INVALID, "unknown kernel id");
  const bool unpool = kernel == 4;  // the intra-scale (unpooling) layer into `scale`
  const Launch* src = nullptr;
  for (const Launch& L : P->sched_roll)
    if ((L.kind == kind_of[kernel] || (kernel == 1 && L.kind == L_EDGE_MLP)) &&
        (L.kind == L_ENCODE || L.scale == scale) &&
        (L.kind != L_EDGE_HOP || (L.eh.own_zero != 0) == unpool)) {
      if (!src) src = &L;
      if (L.kind == L_HOP && !L.hop.last) { src = &L; break; }  // prefer a middle hop
      if (L.kind != L_HOP) break;
    }
  if (!src) return fail(MSW_ERR_INVALID, "no such kernel on that scale");
  Launch L = *src;
  const ScaleCSR& g = P->sc[scale];
  int64_t rows = g.ns, edges = g.E;
  if (L.kind == L_HOP && L.hop.last) { L.hop.last = 0; L.hop.out = P->T[1]; }
  if (L.kind == L_EDGE_HOP && L.eh.last && !unpool) { L.eh.last = 0; L.eh.out = P->T[1]; }
  if (L.kind == L_EDGE_HOP || L.kind == L_EDGE_MLP) L.eh.step_inc = nullptr;  // the rollout's step counter stays put
  if (unpool) edges = P->lv[scale].I;  // the unpool epilogue only writes the next layer's U/V/O
  if (L.kind == L_POOL) edges = P->lv[scale - 1].I;
  if (L.kind == L_ENCODE) { L.enc.io = nullptr; L.enc.dec.on = 0; rows = P->N; edges = 0; }
  std::vector<Launch> q(1, L);
  for (int it = 0; it < iters; ++it) {
    int rc = schedule_dispatch(P, q, st);
    if (rc) return rc;
  }
  P->kernels_per_step = (int)P->sched_roll.size();
  if (units) { units[0] = rows; units[1] = edges; }
  return MSW_OK;
}

// BC slots (internal rows), the device I/O record and the initial state of a rollout, set
// by kernels whose arguments carry the values: no host buffer lifetime issue, no host sync.
int rollout_prologue(msw_plan* P, const float* x0, const float* bc, int32_t bc_tstride,
                     const int32_t* node_bc, int32_t n_bc, int32_t type_bc, int32_t T, float* out,
                     hipStream_t st) {
  if (!P || !x0 || !out) return fail(MSW_ERR_INVALID, "null argument");
  if (n_bc > 0 && (!bc || !node_bc)) return fail(MSW_ERR_INVALID, "BC arrays missing");
  if (n_bc > 0 && bc_tstride < T) return fail(MSW_ERR_INVALID, "BC has fewer time entries than T");
  if (type_bc != 1 && type_bc != 2) return fail(MSW_ERR_INVALID, "type_BC must be 1 or 2 (dataset.py:499-506)");
  HIP_TRY(hipSetDevice(P->device));
  std::vector<int> rows;
  for (int b = 0; b < n_bc; ++b) {
    if (node_bc[b] < 0 || node_bc[b] >= P->N) return fail(MSW_ERR_INVALID, "node_BC out of range");
    rows.push_back(P->iperm[node_bc[b]]);
  }
  if (rows != P->bc_rows_set) {
    // the old rows' slots back to -1, then slot i for the i-th new row
    for (const std::vector<int>* v : {&P->bc_rows_set, &rows})
      for (size_t i = 0; i < v->size(); i += kSlotBatch) {
        SlotArgs sa{};
        sa.slot = P->bc_slot_d;
        sa.n = (int)std::min(v->size() - i, (size_t)kSlotBatch);
        for (int k = 0; k < sa.n; ++k) { sa.row[k] = (*v)[i + k]; sa.val[k] = v == &rows ? (int)(i + k) : -1; }
        HIP_TRY(launch_set_slots(sa, st));
      }
    P->bc_rows_set = rows;
  }
  for (const RowMlpArgs& ra : P->edge_jobs) HIP_TRY(rowmlp_dispatch(P->NT, ra, st));
  RolloutIO io{};
  io.bc = bc; io.out = out; io.bc_tstride = bc_tstride; io.type_bc = type_bc; io.T = T; io.step = -1;
  HIP_TRY(launch_set_io(P->io_d, io, st));
  InitArgs ia{};
  ia.x0 = x0; ia.perm = P->perm_d; ia.N = P->Npad; ia.nnf = P->nnf;
  ia.dyn = P->dyn; ia.p = P->p; ia.X = P->X; ia.io = P->io_d; ia.bc_slot = P->bc_slot_d;
  HIP_TRY(launch_init_state(ia, st));
  return MSW_OK;
}

// Capture what `enqueue(stream)` launches on the plan's capture stream into `*exec`.
template <class Fn>
int capture_graph(msw_plan* P, hipGraphExec_t* exec, Fn enqueue) {
  if (!P->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&P->cap_stream, hipStreamNonBlocking));
  hipGraph_t graph = nullptr;
  HIP_TRY(hipStreamBeginCapture(P->cap_stream, hipStreamCaptureModeThreadLocal));
  const int rc = enqueue(P->cap_stream);
  const hipError_t ce = hipStreamEndCapture(P->cap_stream, &graph);
  if (rc) {
    if (graph) (void)hipGraphDestroy(graph);
    return rc;
  }
  if (ce != hipSuccess) return fail(MSW_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
  const hipError_t ie = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (ie != hipSuccess) {
    *exec = nullptr;
    return fail(MSW_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
  }
  return MSW_OK;
}

// T rollout steps, each `step(stream)`.  graphs: G = P->graph_steps consecutive steps are
// captured into *multi and one step into *one (each when first needed, on P's capture
// stream), then T / G launches of the first and T mod G of the second; the steps read their
// counters from the device-side I/O records the prologues wrote.  Otherwise step by step.
template <class Step>
int run_steps(msw_plan* P, bool graphs, hipGraphExec_t* multi, hipGraphExec_t* one, int T, hipStream_t st,
              Step step) {
  if (!graphs) {
    for (int t = 0; t < T; ++t)
      if (int rc = step(st)) return rc;
    return MSW_OK;
  }
  auto capture = [&](hipGraphExec_t* exec, int steps) -> int {
    return capture_graph(P, exec, [&](hipStream_t cs) {
      int rc = MSW_OK;
      for (int k = 0; k < steps && !rc; ++k) rc = step(cs);
      return rc;
    });
  };
  const int G = std::max(1, P->graph_steps);
  int rc;
  if (G > 1 && T >= G && !*multi && (rc = capture(multi, G))) return rc;
  if ((G == 1 || T % G) && !*one && (rc = capture(one, 1))) return rc;
  int t = 0;
  if (G > 1)
    for (; t + G <= T; t += G) HIP_TRY(hipGraphLaunch(*multi, st));
  for (; t < T; ++t) HIP_TRY(hipGraphLaunch(*one, st));
  return MSW_OK;
}

// In-process transport (msw_group_rollout): halo rows of plan k's buffer gathered straight
// from the owning plans' buffers, using each owner's send list for k.
int loopback_exchange(msw_plan* const* plans, int k, const ExchangeArgs& a, hipStream_t st) {
  msw_plan* P = plans[k];
  const msw_plan::XchScale& X = P->xch[a.scale];
  for (const auto& pe : X.peers) {
    if (pe.rcount == 0) continue;
    msw_plan* Q = plans[pe.peer];
    const msw_plan::XchScale& Y = Q->xch[a.scale];
    const XchPeer* back = nullptr;
    for (const auto& qe : Y.peers)
      if (qe.peer == k) back = &qe;
    if (!back || back->scount != pe.rcount)
      return fail(MSW_ERR_INVALID, "exchange lists of plans " + std::to_string(k) + " and " +
                                       std::to_string(pe.peer) + " disagree");
    for (int b = 0; b < a.nbuf; ++b) {
      if (Q == P) {  // self entry: staged, as the RCCL transport does (the row sets may overlap)
        HIP_TRY(launch_copy_rows(buf_of(P, a.buf[b]), Y.send_rows + back->soff, P->xsend, nullptr, pe.rcount,
                                 a.width[b], st));
        HIP_TRY(launch_copy_rows(P->xsend, nullptr, buf_of(P, a.buf[b]), X.recv_rows + pe.roff, pe.rcount,
                                 a.width[b], st));
      } else {
        HIP_TRY(launch_copy_rows(buf_of(Q, a.buf[b]), Y.send_rows + back->soff, buf_of(P, a.buf[b]),
                                 X.recv_rows + pe.roff, pe.rcount, a.width[b], st));
      }
    }
  }
  return MSW_OK;
}

int group_step(msw_plan* const* plans, int n, hipStream_t st) {
  const size_t L = plans[0]->sched_roll.size();
  for (size_t i = 0; i < L; ++i)
    for (int k = 0; k < n; ++k) {
      const Launch& l = plans[k]->sched_roll[i];
      if (l.kind == L_EXCHANGE) {
        int rc = loopback_exchange(plans, k, l.xch, st);
        if (rc) return rc;
      } else {
        HIP_TRY(launch_one(plans[k], l, st));
      }
    }
  return MSW_OK;
}

}  // namespace

// ============================================================================ C ABI
extern "C" {

int msw_comm_unique_id(char* uid128) {
  if (!uid128) return fail(MSW_ERR_INVALID, "null argument");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  if (!rccl().ok) return fail(MSW_ERR_UNSUPPORTED, "RCCL not found in the process nor as librccl.so.1");
  ncclUniqueId id;
  const ncclResult_t e = rccl().getUniqueId(&id);
  if (e != ncclSuccess) return fail(MSW_ERR_HIP, std::string("ncclGetUniqueId: ") + rccl().errStr(e));
  memcpy(uid128, &id, sizeof(id));
  return MSW_OK;
}

int msw_plan_set_comm(msw_plan* P, const char* uid128, int32_t nranks, int32_t rank) {
  if (!P || !uid128) return fail(MSW_ERR_INVALID, "null argument");
  if (P->part_rank < 0) return fail(MSW_ERR_INVALID, "plan is not partitioned (msw_plan_create_part)");
  if (rank != P->part_rank || nranks <= rank) return fail(MSW_ERR_INVALID, "rank does not match the plan's part");
  if (!rccl().ok) return fail(MSW_ERR_UNSUPPORTED, "RCCL not found in the process nor as librccl.so.1");
  HIP_TRY(hipSetDevice(P->device));
  if (P->comm) {
    (void)rccl().commDestroy(P->comm);
    P->comm = nullptr;
  }
  ncclUniqueId id;
  memcpy(&id, uid128, sizeof(id));
  const ncclResult_t e = rccl().commInitRank(&P->comm, nranks, id, rank);
  if (e != ncclSuccess) {
    P->comm = nullptr;
    return fail(MSW_ERR_HIP, std::string("ncclCommInitRank: ") + rccl().errStr(e));
  }
  return MSW_OK;
}

int msw_group_rollout(msw_plan* const* plans, int32_t num_plans, const float* const* x0,
                      const float* const* bc, const int32_t* bc_tstride, const int32_t* const* node_bc,
                      const int32_t* n_bc, int32_t type_bc, int32_t T, float* const* out, void* stream) {
  if (!plans || num_plans <= 0 || !x0 || !bc || !bc_tstride || !node_bc || !n_bc || !out)
    return fail(MSW_ERR_INVALID, "null argument");
  if (T < 0) return fail(MSW_ERR_INVALID, "T < 0");
  const msw_plan* P0 = plans[0];
  for (int k = 0; k < num_plans; ++k) {
    const msw_plan* P = plans[k];
    if (!P) return fail(MSW_ERR_INVALID, "null plan");
    if (P->part_rank != k) return fail(MSW_ERR_INVALID, "plans[k] must be the plan of part k");
    if (P->device != P0->device || P->NT != P0->NT) return fail(MSW_ERR_INVALID, "plans on different devices / widths");
    if (P->sched_roll.size() != P0->sched_roll.size())
      return fail(MSW_ERR_INVALID, "plans with different step schedules");
    for (size_t i = 0; i < P->sched_roll.size(); ++i)
      if (P->sched_roll[i].kind != P0->sched_roll[i].kind)
        return fail(MSW_ERR_INVALID, "plans with different step schedules");
    for (const auto& X : P->xch)
      for (const auto& pe : X.peers)
        if (pe.peer >= num_plans) return fail(MSW_ERR_INVALID, "exchange peer outside the group");
  }
  if (T == 0) return MSW_OK;
  hipStream_t st = (hipStream_t)stream;
  for (int k = 0; k < num_plans; ++k) {
    int rc = rollout_prologue(plans[k], x0[k], bc[k], bc_tstride[k], node_bc[k], n_bc[k], type_bc, T, out[k], st);
    if (rc) return rc;
  }
  msw_plan* G0 = plans[0];
  if (G0->group_graph) {
    // the group's graphs (every part's launches and the halo copies of the steps) are held by
    // plan 0 and go stale with any member's identity or graph generation
    std::vector<uint64_t> key;
    for (int k = 0; k < num_plans; ++k) {
      key.push_back(plans[k]->uid);
      key.push_back((uint64_t)plans[k]->graph_gen);
    }
    if (key != G0->group_key) {
      G0->drop_group_graphs();
      G0->group_key = key;
    }
  }
  if (int rc = run_steps(G0, G0->group_graph != 0, &G0->group_multi, &G0->group_one, T, st,
                         [&](hipStream_t s) { return group_step(plans, num_plans, s); }))
    return rc;
  for (int k = 0; k < num_plans; ++k)
    if (int rc = final_decode(plans[k], st)) return rc;
  for (int k = 0; k < num_plans; ++k) {
    plans[k]->rollout_steps += T;
    plans[k]->forward_calls += T;
  }
  return MSW_OK;
}

int msw_forward(msw_plan* P, const float* x, float* y, void* stream) {
  if (!P || !x || !y) return fail(MSW_ERR_INVALID, "null argument");
  HIP_TRY(hipSetDevice(P->device));
  hipStream_t st = (hipStream_t)stream;
  if (P->use_graph) {
    // the schedule reads fwd_x and writes fwd_y (graph numbering, like x and y)
    const size_t xb = (size_t)P->N * P->nnf * sizeof(float), yb = (size_t)P->N * 2 * sizeof(float);
    if (!P->fwd_exec) {
      if (!P->fwd_x) {
        int rc = palloc(P, &P->fwd_x, (size_t)P->N * P->nnf);
        if (!rc) rc = palloc(P, &P->fwd_y, (size_t)P->N * 2);
        if (rc) return rc;
      }
      patch_forward(P->sched_fwd, P->fwd_x, P->fwd_y);
      int rc = capture_graph(P, &P->fwd_exec, [&](hipStream_t cs) { return schedule_dispatch(P, P->sched_fwd, cs); });
      if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(P->fwd_x, x, xb, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGraphLaunch(P->fwd_exec, st));
    HIP_TRY(hipMemcpyAsync(y, P->fwd_y, yb, hipMemcpyDeviceToDevice, st));
  } else {
    patch_forward(P->sched_fwd, x, y);
    int rc = schedule_dispatch(P, P->sched_fwd, st);
    if (rc) return rc;
  }
  P->forward_calls++;
  return MSW_OK;
}

int msw_set_graph_capture(msw_plan* P, int enable) {
  if (!P) return fail(MSW_ERR_INVALID, "null plan");
  P->use_graph = enable ? 1 : 0;  // the plan's own rollout / forward graphs only
  return MSW_OK;
}

int msw_set_group_graph(msw_plan* P, int enable) {
  if (!P) return fail(MSW_ERR_INVALID, "null plan");
  P->group_graph = enable ? 1 : 0;
  P->drop_group_graphs();
  return MSW_OK;
}

int msw_rollout(msw_plan* P, const float* x0, const float* bc, int32_t bc_tstride,
                const int32_t* node_bc, int32_t n_bc, int32_t type_bc, int32_t T, float* out,
                void* stream) {
  if (!P || !x0 || (!out && T > 0)) return fail(MSW_ERR_INVALID, "null argument");
  if (T < 0) return fail(MSW_ERR_INVALID, "T < 0");
  if (T == 0) return MSW_OK;
  hipStream_t st = (hipStream_t)stream;
  int prc = rollout_prologue(P, x0, bc, bc_tstride, node_bc, n_bc, type_bc, T, out, st);
  if (prc) return prc;
  if (int rc = run_steps(P, P->use_graph != 0, &P->multi_exec, &P->step_exec, T, st,
                         [&](hipStream_t s) { return schedule_dispatch(P, P->sched_roll, s); }))
    return rc;
  if (int rc = final_decode(P, st)) return rc;
  P->rollout_steps += T;
  P->forward_calls += T;
  if (P->comm)
    for (const auto& X : P->xch)
      if (!X.peers.empty()) {
        P->rccl_steps += T;
        break;
      }
  return MSW_OK;
}

int msw_bench_kernel(msw_plan* P, int32_t kernel, int32_t scale, int32_t iters, int64_t* units,
                     void* stream) {
  if (!P || iters < 0) return fail(MSW_ERR_INVALID, "bad argument");
  HIP_TRY(hipSetDevice(P->device));
  hipStream_t st = (hipStream_t)stream;
  return bench_kernel(P, kernel, scale, iters, units, st);
}

int msw_set_trace(msw_plan* P, uint64_t* buf) {
  if (!P) return fail(MSW_ERR_INVALID, "null plan");
  // MSW_TRACE_ENCODE: the encoder launches only (a rollout then leaves the marks of its last
  // step's encoder: the deferred decoder + encoders, tools/trace_kernels.py)
  const bool enc_only = P->kn.trace_encode != 0;
  for (auto* q : {&P->sched_fwd, &P->sched_roll})
    for (Launch& L : *q)
      L.common().trace = (!enc_only || L.kind == L_ENCODE) ? reinterpret_cast<unsigned long long*>(buf) : nullptr;
  P->drop_graphs();  // the captured steps hold the old arguments
  return MSW_OK;
}

}  // extern "C"
