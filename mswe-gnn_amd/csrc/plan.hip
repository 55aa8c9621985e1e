// Host side of the C ABI (include/mswegnn.h), plan creation: the graph plan (16-row-aligned
// internal numbering, CSR by destination, edge tiles, pooling / unpooling maps) uploaded, the
// weights packed (weights.hip), the device buffers, the step schedules (schedule.hip) and the
// static edge features; plan destruction and the plan's queries.  Running a plan: runtime.hip.
//
// Reference semantics followed (sdat2/mSWE-GNN):
//   MSGNN.forward  models/gnn.py:267-350     GNN.forward  models/gnn.py:102-152
#include <atomic>
#include <cstdio>
#include <memory>

#include "plan.h"

using namespace msw;

namespace {

thread_local std::string g_err;

int build_graph_plan(msw_plan* P, const msw_graph_desc* g, const int64_t* row_order) {
  // the host plan (graph_build.h: numbering, CSRs, tiles, records -- also built by the
  // sanitizer harness tests/asan/host_plan_check.cpp), then its device copies
  HostGraph H;
  std::string err;
  int rc = build_host_graph(g, P->S, kRowsPerBlock, P->kn.tile_pack != 0, row_hop_min_tiles(P), H, err, row_order);
  if (rc) return fail(rc, err);
  P->N = H.N;
  P->E = H.E;
  P->Npad = H.Npad;
  P->perm = std::move(H.perm);
  P->iperm = std::move(H.iperm);
  const int S = P->S;
  P->sc.assign(S, ScaleCSR{});
  for (int s = 0; s < S; ++s) {
    HostScale& h = H.sc[s];
    ScaleCSR& c = P->sc[s];
    c.n0 = h.n0; c.ns = h.ns; c.E = h.E; c.ntiles = h.ntiles; c.nchunks = h.nchunks;
    if ((rc = pupload(P, &c.recs, h.recs))) return rc;
    if (c.nchunks > 0 && (rc = pupload(P, &c.chunks, h.chunks))) return rc;
    if (!h.rptr.empty() && ((rc = pupload(P, &c.rptr, h.rptr)) || (rc = pupload(P, &c.redge, h.redge)))) return rc;
    c.porig = std::move(h.porig);
    c.hrecs = std::move(h.recs);
  }
  P->lv.assign(S > 1 ? S - 1 : 0, LevelMaps{});
  for (int l = 0; l + 1 < S; ++l) {
    HostLevel& h = H.lv[l];
    LevelMaps& m = P->lv[l];
    m.I = h.I; m.pool_etiles = h.pool_etiles; m.un_ntiles = h.un_ntiles;
    if ((rc = pupload(P, &m.pool_erecs, h.pool_erecs)) || (rc = pupload(P, &m.pool_recs, h.pool_recs)) ||
        (rc = pupload(P, &m.pool_child, h.pool_child)) || (rc = pupload(P, &m.un_recs, h.un_recs)))
      return rc;
    if (!h.pool_slots.empty() && (rc = pupload(P, &m.pool_slots, h.pool_slots))) return rc;
    if (!h.parent_slots.empty() && (rc = pupload(P, &m.parent_slots, h.parent_slots))) return rc;
  }
  return MSW_OK;
}

// The inline in-edge records and the overflow CSR of the scales that run the dense hop.
int upload_dense(msw_plan* P) {
  for (ScaleCSR& c : P->sc) {
    if (!dense_hops(P, c)) continue;
    const HostDense d = build_dense(c.hrecs, c.n0, c.ns);
    int rc;
    if ((rc = pupload(P, &c.drecs, d.recs)) || (rc = pupload(P, &c.dptr, d.rptr)) || (rc = pupload(P, &c.dedge, d.redge)))
      return rc;
  }
  return MSW_OK;
}

// Partitioned mesh: per-scale receive / send row lists (local graph rows -> internal rows).
int build_exchange(msw_plan* P, const msw_exchange_desc* d) {
  // the lists (graph_build.h build_host_exchange, validated against the plan's numbering)
  HostGraph H;  // the numbering only
  H.N = P->N;
  H.iperm = P->iperm;
  H.sc.resize(P->S);
  for (int s = 0; s < P->S; ++s) { H.sc[s].n0 = P->sc[s].n0; H.sc[s].ns = P->sc[s].ns; }
  std::vector<HostXchScale> X;
  std::string err;
  int rc = build_host_exchange(H, P->part_rank, d, X, err);
  if (rc) return fail(rc, err);
  P->xch.assign(P->S, msw_plan::XchScale{});
  size_t most = 1;
  for (int s = 0; s < P->S; ++s) {
    msw_plan::XchScale& Y = P->xch[s];
    Y.nrecv = (int)X[s].recv_rows.size();
    Y.nsend = (int)X[s].send_rows.size();
    Y.peers = std::move(X[s].peers);
    if ((rc = pupload(P, &Y.recv_rows, X[s].recv_rows)) || (rc = pupload(P, &Y.send_rows, X[s].send_rows))) return rc;
    most = std::max(most, (size_t)std::max(Y.nrecv, Y.nsend));
  }
  const size_t floats = most * 2 * P->Fp;  // widest exchanged row: U (2 Fp)
  if ((rc = palloc(P, &P->xsend, floats)) || (rc = palloc(P, &P->xrecv, floats))) return rc;
  return MSW_OK;
}

// ---------------------------------------------------------------------------- plan creation
// The steps of plan_create_impl, in its order.

// The model's shape into the plan, and the shapes the engine does not run.
int check_model(msw_plan* P, const msw_model_desc* m) {
  P->model_type = m->model_type;
  P->F = m->hid_features;
  P->Fp = P->F > 32 ? 64 : P->F;
  P->NT = P->Fp / 16;
  P->S = m->model_type == 0 ? m->num_scales : 1;
  P->p = m->previous_t;
  P->nnf = m->num_node_features;
  P->dyn = 2 * P->p;
  P->nstat_raw = P->nnf - P->dyn;
  P->with_wl = m->with_WL;
  P->skip = m->skip_connections;
  P->gnn_act = m->gnn_act;
  P->gnn_slope = m->gnn_act_param;
  if (P->S < 1) return fail(MSW_ERR_INVALID, "num_scales < 1");
  // the kernels write the newest state pair at columns dyn - 2 and dyn - 1 of a row
  if (P->p < 1) return fail(MSW_ERR_UNSUPPORTED, "previous_t must be 1..8");
  if (P->nstat_raw < 1 || P->nstat_raw + P->with_wl > 16 || P->dyn > 16)
    return fail(MSW_ERR_UNSUPPORTED, "node feature layout (static / dynamic widths)");
  if (m->model_type == 0 && m->num_processors != 2 * P->S - 1)
    return fail(MSW_ERR_INVALID, "MSGNN needs 2S-1 processors");
  if (m->model_type == 0 && m->num_unpool != P->S - 1)
    return fail(MSW_ERR_INVALID, "MSGNN needs S-1 intra-scale layers");
  if (m->model_type == 1 && m->num_processors < 1) return fail(MSW_ERR_INVALID, "GNN needs >= 1 layer");
  return MSW_OK;
}

// The state, the per-layer row buffers and the rollout's device-side records, zeroed.
int alloc_buffers(msw_plan* P) {
  const int Npad = P->Npad;
  int rc;
  if ((rc = pupload(P, &P->perm_d, P->perm))) return rc;
  if ((rc = pupload(P, &P->zrow_d, std::vector<float>(kZeroRow, 0.f)))) return rc;
  std::vector<int> minus1(Npad, -1);
  if ((rc = pupload(P, &P->bc_slot_d, minus1))) return rc;
  if ((rc = palloc(P, &P->io_d, 1))) return rc;
  HIP_TRY(hipMemset(P->io_d, 0, sizeof(RolloutIO)));
  int Emax = 1;  // tile-padded edge slots of the largest scale
  for (auto& c : P->sc) Emax = std::max(Emax, c.ntiles * kRowsPerWave);
  const size_t NF = (size_t)Npad * P->Fp;
  const size_t NH = (size_t)Npad * 16 * P->h1t_max;
  float** bufs[] = {&P->xs, &P->xd0, &P->O[0], &P->O[1], &P->T[0], &P->T[1], &P->xdown, &P->xup, &P->xgnn};
  for (float** b : bufs) {
    if ((rc = palloc(P, b, NF))) return rc;
    HIP_TRY(hipMemset(*b, 0, NF * sizeof(float)));
  }
  float** hbufs[] = {&P->U[0], &P->V[0], &P->U[1], &P->V[1], &P->Uu, &P->Vu};
  for (float** b : hbufs) {
    if ((rc = palloc(P, b, NH))) return rc;
    HIP_TRY(hipMemset(*b, 0, NH * sizeof(float)));
  }
  if ((rc = palloc(P, &P->s, (size_t)Emax * P->Fp))) return rc;
  if ((rc = palloc(P, &P->X, (size_t)Npad * P->nnf))) return rc;
  HIP_TRY(hipMemset(P->X, 0, (size_t)Npad * P->nnf * sizeof(float)));
  if (P->E > 0)
    for (Proc& pr : P->procs)
      if ((rc = palloc(P, &pr.Pe, (size_t)std::max(P->sc[pr.scale].ntiles * kRowsPerWave, 1) * 16 * pr.h1t)))
        return rc;
  return MSW_OK;
}

// Launch schedules (forward / rollout) with their per-launch weight regions, then the
// weight upload.
int make_schedules(msw_plan* P) {
  HIP_TRY(with_nt(P->NT, [](auto nt) { return prepare_kernels<nt>(); }));
  int rc;
  if ((rc = upload_dense(P)) || (rc = build_schedules(P))) return rc;
  P->blob.alloc(256);  // slack: LDS-DMA chunks may read up to 255 floats past a region
  if ((rc = pupload(P, &P->dW, P->blob.h))) return rc;
  for (auto* q : {&P->sched_fwd, &P->sched_roll})
    for (Launch& L : *q) L.common().W = P->dW;
  return MSW_OK;
}

// Static per-edge features: edge encoder + edge part of each processor's layer 1.
int static_edge_features(msw_plan* P, const msw_graph_desc* g, const msw_model_desc* m) {
  if (P->E <= 0) return MSW_OK;
  const int ef_raw = g->num_edge_features;
  int rc;
  // tile-padded edge slots, scale by scale (ScaleCSR::porig); padding slots get zeros
  std::vector<int64_t> sbase(P->S + 1, 0);
  for (int s = 0; s < P->S; ++s) sbase[s + 1] = sbase[s] + (int64_t)P->sc[s].ntiles * kRowsPerWave;
  const int64_t E = sbase[P->S];
  std::vector<float> ea((size_t)std::max<int64_t>(E, 1) * ef_raw, 0.f);
  for (int s = 0; s < P->S; ++s)
    for (size_t q = 0; q < P->sc[s].porig.size(); ++q)
      if (P->sc[s].porig[q] >= 0)
        for (int f = 0; f < ef_raw; ++f)
          ea[(size_t)(sbase[s] + q) * ef_raw + f] = g->edge_attr[(size_t)P->sc[s].porig[q] * ef_raw + f];
  float* ea_d = nullptr;
  float* enc_d = nullptr;
  if ((rc = pupload(P, &ea_d, ea))) return rc;
  const float* feat = ea_d;
  int feat_stride = ef_raw, feat_dim = ef_raw;
  if (m->edge_mlp) {
    if ((rc = palloc(P, &enc_d, (size_t)E * P->Fp))) return rc;
    RowMlpArgs ra{};
    ra.mode = 0;
    ra.in = ea_d; ra.in_stride = ef_raw; ra.in_dim = ef_raw; ra.R = (int)E; ra.m = P->edge_enc;
    ra.W = P->dW; ra.out = enc_d; ra.out_stride = P->Fp; ra.out_tiles = P->NT;
    P->edge_jobs.push_back(ra);
    feat = enc_d; feat_stride = P->Fp; feat_dim = P->F;  // rows of Fp, the first F the model's
  }
  for (size_t j = 0; j < P->procs.size(); ++j) {
    Proc& pr = P->procs[j];
    Blob tb;  // Pe = W1[:, 4F:4F+ef] . feat + b1
    const MlpDev md = pack_edge_term(P, tb, m->processors[j].edge_mlp.layer[0], feat_dim);
    float* tw = nullptr;
    if ((rc = pupload(P, &tw, tb.h))) return rc;
    const ScaleCSR& c = P->sc[pr.scale];
    RowMlpArgs ra{};
    ra.mode = 1;
    ra.in = feat + (size_t)sbase[pr.scale] * feat_stride; ra.in_stride = feat_stride;
    ra.in_dim = feat_dim; ra.R = c.ntiles * kRowsPerWave; ra.m = md; ra.W = tw;
    ra.out = pr.Pe; ra.out_stride = 16 * pr.h1t; ra.out_tiles = pr.h1t;
    P->edge_jobs.push_back(ra);
  }
  for (const RowMlpArgs& ra : P->edge_jobs) HIP_TRY(rowmlp_dispatch(P->NT, ra));
  return MSW_OK;
}

int plan_create_impl(const msw_graph_desc* g, const msw_model_desc* m, int device,
                     const msw_exchange_desc* xch, int rank, const int64_t* row_order, msw_plan** out_plan) {
  if (!g || !m || !out_plan) return fail(MSW_ERR_INVALID, "null argument");
  *out_plan = nullptr;
  if (m->model_type != 0 && m->model_type != 1) return fail(MSW_ERR_INVALID, "model_type must be 0 (MSGNN) or 1 (GNN)");
  // 16, 32, 64 run at their own width; 33..63 zero-padded to 64 (the F = 64 kernels)
  if (m->hid_features != 16 && !(m->hid_features >= 32 && m->hid_features <= 64))
    return fail(MSW_ERR_UNSUPPORTED, "hid_features must be 16 or 32..64 (33..63 run zero-padded to 64)");
  if (m->learned_pooling) return fail(MSW_ERR_UNSUPPORTED, "learned_pooling=True is not implemented");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<msw_plan> P(new msw_plan());
  static std::atomic<uint64_t> next_uid{1};
  P->uid = next_uid++;
  P->device = device;
  int rc;
  if ((rc = check_model(P.get(), m))) return rc;
  P->kn = knobs_from_env(P->NT);
  P->part_rank = xch ? rank : -1;
  if ((rc = build_graph_plan(P.get(), g, row_order))) return rc;
  if (xch && (rc = build_exchange(P.get(), xch))) return rc;
  if ((rc = pack_model(P.get(), m, g->num_edge_features))) return rc;
  if ((rc = alloc_buffers(P.get()))) return rc;
  if ((rc = make_schedules(P.get()))) return rc;
  if ((rc = static_edge_features(P.get(), g, m))) return rc;
  HIP_TRY(hipDeviceSynchronize());
  if (xch) P->use_graph = 0;  // partitioned plans: the RCCL exchanges run eagerly
  *out_plan = P.release();
  return MSW_OK;
}

}  // namespace

int msw::set_error(int code, const char* msg) {
  g_err = msg ? msg : "";
  return code;
}

// ============================================================================ C ABI
extern "C" {

const char* msw_last_error(void) { return g_err.c_str(); }

int64_t msw_struct_size(const char* name) {
  static const struct { const char* name; int64_t size; } tab[] = {
#define MSW_SIZE(T) {#T, (int64_t)sizeof(T)}
      MSW_SIZE(msw_linear), MSW_SIZE(msw_mlp), MSW_SIZE(msw_swegnn), MSW_SIZE(msw_model_desc),
      MSW_SIZE(msw_graph_desc), MSW_SIZE(msw_plan_stats), MSW_SIZE(msw_exchange_desc),
      MSW_SIZE(msw_swegnn_train_desc), MSW_SIZE(msw_swegnn_grads), MSW_SIZE(msw_mlp_train_desc),
      MSW_SIZE(msw_mlp_grads), MSW_SIZE(msw_flood_maps), MSW_SIZE(msw_zone_series),
      MSW_SIZE(msw_train_loss_desc), MSW_SIZE(msw_ensemble_steps_out), MSW_SIZE(msw_ensemble_maps_out),
      MSW_SIZE(msw_ensemble_scores_out), MSW_SIZE(msw_raster_grid), MSW_SIZE(msw_raster_stats),
      MSW_SIZE(msw_zonal_stats), MSW_SIZE(msw_locator_stats), MSW_SIZE(msw_mesh_dual_stats),
      MSW_SIZE(msw_locality_stats)};
#undef MSW_SIZE
  for (const auto& t : tab)
    if (name && !strcmp(name, t.name)) return t.size;
  return -1;
}

int msw_abi_version(void) { return MSW_ABI_VERSION; }

int msw_plan_create(const msw_graph_desc* g, const msw_model_desc* m, int device, msw_plan** out_plan) {
  return plan_create_impl(g, m, device, nullptr, -1, nullptr, out_plan);
}

int msw_plan_create_ordered(const msw_graph_desc* g, const msw_model_desc* m, int device, const int64_t* row_order,
                            msw_plan** out_plan) {
  return plan_create_impl(g, m, device, nullptr, -1, row_order, out_plan);
}

int msw_plan_create_part(const msw_graph_desc* g, const msw_model_desc* m, int device,
                         const msw_exchange_desc* xch, int32_t rank, msw_plan** out_plan) {
  if (!xch || rank < 0) return fail(MSW_ERR_INVALID, "exchange descriptor missing or rank < 0");
  if (xch->num_entries < 0 || (xch->num_entries > 0 && (!xch->peer || !xch->scale || !xch->recv_ptr ||
                                                         !xch->send_ptr)))
    return fail(MSW_ERR_INVALID, "exchange descriptor arrays missing");
  return plan_create_impl(g, m, device, xch, rank, nullptr, out_plan);
}

int msw_plan_destroy(msw_plan* plan) {
  if (!plan) return MSW_OK;
  (void)hipSetDevice(plan->device);
  (void)hipDeviceSynchronize();
  delete plan;
  return MSW_OK;
}

int msw_debug_buffer(msw_plan* P, const char* name, float* dst, void* stream) {
  if (!P || !name || !dst) return fail(MSW_ERR_INVALID, "null argument");
  const float* src = nullptr;
  if (!strcmp(name, "x_s")) src = P->xs;
  else if (!strcmp(name, "x_d")) src = P->xd0;
  else if (!strcmp(name, "x_down")) src = P->model_type == 0 ? P->xdown : nullptr;
  else if (!strcmp(name, "x_up")) src = P->model_type == 0 ? P->xup : nullptr;
  if (!src) return fail(MSW_ERR_INVALID, std::string("unknown buffer ") + name);
  // debug only: synchronous host round trip into graph numbering
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  // rows of Fp on the device, the model's F columns of each into the caller's [N][F]
  std::vector<float> h((size_t)P->Npad * P->Fp), o((size_t)P->N * P->F);
  HIP_TRY(hipMemcpy(h.data(), src, h.size() * sizeof(float), hipMemcpyDeviceToHost));
  for (int i = 0; i < P->Npad; ++i)
    if (P->perm[i] >= 0)
      std::copy(h.begin() + (size_t)i * P->Fp, h.begin() + (size_t)i * P->Fp + P->F, o.begin() + (size_t)P->perm[i] * P->F);
  HIP_TRY(hipMemcpy(dst, o.data(), o.size() * sizeof(float), hipMemcpyHostToDevice));
  return MSW_OK;
}

int msw_plan_row_layout(const msw_plan* P, int32_t* perm, int64_t capacity, int64_t* npad) {
  if (!P || !npad || capacity < 0 || (capacity > 0 && !perm)) return fail(MSW_ERR_INVALID, "bad argument");
  *npad = P->Npad;
  std::copy(P->perm.begin(), P->perm.begin() + std::min<int64_t>(capacity, P->Npad), perm);
  return MSW_OK;
}

int msw_plan_schedule(const msw_plan* P, int32_t rollout, char* buf, int64_t cap, int64_t* needed) {
  if (!P || !needed || (cap > 0 && !buf) || cap < 0) return fail(MSW_ERR_INVALID, "bad argument");
  static const char* const kind_name[] = {"encode", "edge_hop", "hop", "pool", "exchange", "epi", "edge_mlp", "decode"};
  std::string out;
  for (const Launch& L : rollout ? P->sched_roll : P->sched_fwd) {
    Pick p = pick_one(P, L);
    if (L.kind == L_EXCHANGE) snprintf(p.name, sizeof(p.name), "exchange");
    // iterations of the wave that makes the most: rounds of grid x per_wg units
    const long round = (long)p.grid * p.per_wg;
    const long iters = round > 0 ? (p.units + round - 1) / round : 0;
    const int ragged = round > 0 && p.units % round != 0;
    char line[320];
    snprintf(line, sizeof(line),
             "kind=%s\tvariant=%s\tnt=%d\tscale=%d\tprelu=%d\tgrid=%d\twaves=%d\tunits=%ld\tper_wg=%d\titers=%ld\t"
             "ragged=%d\tlds=%zu\n",
             kind_name[L.kind], p.name, P->NT, L.scale, L.common().prelu, p.grid, p.waves, p.units, p.per_wg, iters,
             ragged, p.lds);
    out += line;
  }
  *needed = (int64_t)out.size() + 1;
  if (cap > 0) {
    const size_t n = std::min(out.size(), (size_t)cap - 1);
    memcpy(buf, out.data(), n);
    buf[n] = 0;
  }
  return MSW_OK;
}

int msw_plan_get_stats(const msw_plan* P, msw_plan_stats* s) {
  if (!P || !s) return fail(MSW_ERR_INVALID, "null argument");
  s->num_nodes = P->N;
  s->num_edges = P->E;
  s->num_scales = P->S;
  s->hid_features = P->F;
  s->padded_features = P->Fp;
  s->kernels_per_step = P->kernels_per_step;
  s->forward_calls = P->forward_calls;
  s->rollout_steps = P->rollout_steps;
  s->device_bytes = P->dev_bytes;
  s->graph_captured = P->step_exec != nullptr || P->multi_exec != nullptr || P->fwd_exec != nullptr;
  s->rccl_calls = P->rccl_calls;
  s->rccl_steps = P->rccl_steps;
  return MSW_OK;
}

}  // extern "C"
