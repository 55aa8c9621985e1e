/*
 * mswegnn.h -- C ABI of the MI355X (gfx950) multi-scale SWE-GNN rollout engine.
 *
 * Drop-in boundary for the hot path of sdat2/mSWE-GNN.  The reference
 * has no FFI/plugin layer: its hot path sits behind the Python nn.Module API
 *   MSGNN.forward(graph)   models/gnn.py:267-350
 *   GNN.forward(graph)     models/gnn.py:102-152   (type_GNN='SWEGNN')
 *   rollout_test(model,b)  training/train.py:67-95
 * and the package's Python host side (mswe-gnn_amd/models/gnn.py, training/train.py)
 * binds the entry points below through ctypes (mswe-gnn_amd/mswegnn/_lib.py); the binding
 * a maintainer would add on the reference side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types, no torch types; all float data is fp32, row-major.
 *   - host pointers are read only during msw_plan_create (graph + weights are copied to
 *     device memory the plan owns); device pointers passed to msw_forward / msw_rollout
 *     are owned by the caller and must stay valid until the stream has executed the work.
 *   - every function returns MSW_OK (0) or a negative MSW_ERR_* code and never aborts;
 *     msw_last_error() returns a thread-local message for the last failure.
 *   - a plan is bound to one device and is not re-entrant: one stream at a time.
 *   - msw_forward / msw_rollout enqueue asynchronously on `stream` (a hipStream_t, NULL =
 *     default stream) and never synchronise the host.
 */
#ifndef MSWEGNN_H
#define MSWEGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MSW_ABI_VERSION 1

#define MSW_OK 0
#define MSW_ERR_INVALID (-1)     /* bad argument / inconsistent graph or model description */
#define MSW_ERR_HIP (-2)         /* HIP runtime error (allocation, launch, ...)           */
#define MSW_ERR_UNSUPPORTED (-3) /* configuration outside what the engine implements      */

/* Activation codes: activation_functions(), models/models.py:149-169. */
enum msw_activation {
  MSW_ACT_NONE = 0,
  MSW_ACT_PRELU = 1, /* single learned slope (nn.PReLU() default num_parameters=1) */
  MSW_ACT_RELU = 2,
  MSW_ACT_LEAKYRELU = 3, /* slope 0.1 */
  MSW_ACT_ELU = 4,
  MSW_ACT_SWISH = 5, /* SiLU */
  MSW_ACT_SIGMOID = 6,
  MSW_ACT_TANH = 7
};

/* One nn.Linear followed by its activation (make_mlp, models/models.py:121-146:
 * the activation follows EVERY layer, including the last). */
typedef struct {
  int32_t in_features;
  int32_t out_features;
  const float* weight; /* host [out_features][in_features] */
  const float* bias;   /* host [out_features] or NULL (bias=False) */
  int32_t act;         /* enum msw_activation */
  float act_param;     /* PReLU slope */
} msw_linear;

#define MSW_MAX_MLP_LAYERS 4
typedef struct {
  int32_t n_layers;
  msw_linear layer[MSW_MAX_MLP_LAYERS];
} msw_mlp;

/* One SWEGNN layer (models/gnn.py:352-445). */
typedef struct {
  int32_t K;                  /* hops */
  int32_t normalize;          /* s_ij / ||s_ij||, NaN -> 0  (gnn.py:424-426) */
  int32_t with_filter_matrix; /* filter_matrix[0..K] (gnn.py:381-384) */
  int32_t with_gradient;      /* (out[col]-out[row]) * s  vs  s * out[row] (gnn.py:429-435) */
  int32_t upwind_mode;        /* clamp negative gradients (gnn.py:431-432) */
  int32_t edge_features;      /* width of edge_attr fed to this layer; 0 for intra_scale_gnn */
  msw_mlp edge_mlp;           /* input 4F + edge_features -> 2F -> ... -> F */
  const float* const* filter; /* K+1 host pointers to [F][F] (bias-free) or NULL */
} msw_swegnn;

/* Model description.  model_type 0 = MSGNN (models/gnn.py:154-350),
 * 1 = GNN with type_GNN='SWEGNN' (models/gnn.py:13-152). */
typedef struct {
  int32_t model_type;
  int32_t hid_features;      /* F: 16, or 32..64.  16 / 32 / 64 run at their own width; 33..63 run
                              * zero-padded to rows of 64 (msw_plan_stats.padded_features); every
                              * tensor here keeps the model's own F-based shapes */
  int32_t num_scales;        /* S (GNN: 1) */
  int32_t previous_t;        /* p, 1..8 (else MSW_ERR_UNSUPPORTED) */
  int32_t num_node_features; /* static + 2p */
  int32_t with_WL;           /* append DEM + h_t to the static input (gnn.py:288-291) */
  int32_t skip_connections;  /* MSGNN x_down skips (gnn.py:330-331) */
  int32_t learned_pooling;   /* must be 0 (no shipped config uses it) */
  int32_t gnn_act;           /* MSGNN: on x_up (gnn.py:335-336); GNN: after every layer */
  float gnn_act_param;
  /* residual: res_var = sum_tau residual_weights[tau][var] * x[:, dyn + 2 tau + var]
   * (models/models.py:50-77 folded to a [p][2] matrix by the host; NULL = none) */
  const float* residual_weights;
  int32_t edge_mlp;      /* edge encoder present (gnn.py:203-206) */
  msw_mlp edge_encoder;  /* raw edge features -> F */
  msw_mlp static_encoder;
  msw_mlp dynamic_encoder;
  msw_mlp decoder; /* F -> ... -> 2 */
  int32_t num_processors;        /* MSGNN: 2S-1 (down 0..S-2, coarsest, up); GNN: n_GNN_layers */
  const msw_swegnn* processors;
  int32_t num_unpool;            /* MSGNN: S-1 intra_scale_gnn; GNN: 0 */
  const msw_swegnn* unpool;
} msw_model_desc;

/* Graph description in the reference's layout:
 *   - nodes of graph g, scale s: [node_ptr[g*(S+1)+s], node_ptr[g*(S+1)+s+1])
 *     (a single Data: num_graphs=1; a Batch after update_batch_multiscale, train.py:31-65)
 *   - edge_index[0] = row (source j), edge_index[1] = col (target i); scale s edges are
 *     [edge_ptr[s], edge_ptr[s+1]) (scale-major)
 *   - intra_edge_index rows (coarse, fine), level l (coarse scale l+1, fine scale l) is
 *     [intra_edge_ptr[l], intra_edge_ptr[l+1]). */
typedef struct {
  int64_t num_nodes;
  int32_t num_scales;
  int32_t num_graphs;
  const int64_t* node_ptr; /* [num_graphs][num_scales+1] */
  int64_t num_edges;
  const int64_t* edge_index; /* [2][num_edges] */
  const float* edge_attr;    /* [num_edges][num_edge_features] */
  int32_t num_edge_features;
  const int64_t* edge_ptr; /* [num_scales+1] */
  int64_t num_intra_edges;
  const int64_t* intra_edge_index; /* [2][num_intra_edges] */
  const int64_t* intra_edge_ptr;   /* [num_scales] */
} msw_graph_desc;

typedef struct msw_plan msw_plan;

/* Statistics for tests / benchmarks. */
typedef struct {
  int64_t num_nodes;
  int64_t num_edges;
  int32_t num_scales;
  int32_t hid_features;      /* the model's F */
  int32_t padded_features;   /* row width of the plan's buffers and kernels: 16, 32 or 64 */
  int32_t kernels_per_step;  /* launches one forward enqueues */
  int64_t forward_calls;     /* forwards executed through the HIP path so far */
  int64_t rollout_steps;     /* rollout steps executed through the HIP path so far */
  int64_t device_bytes;      /* device memory owned by the plan */
  int32_t graph_captured;    /* a hipGraph of one rollout step is instantiated */
  int64_t rccl_calls;        /* ncclSend / ncclRecv calls this plan issued (eagerly, or recorded
                                into a captured rollout graph) */
  int64_t rccl_steps;        /* rollout steps whose halo exchanges ran over RCCL (eager or replayed) */
} msw_plan_stats;

/* Halo exchange of one rank of a single mesh split over several ranks (SURVEY §8 f2,
 * mswegnn/partition.py).  The graph given to msw_plan_create_part is the rank's LOCAL graph
 * (owned nodes + halo nodes, in-edges of owned nodes only).  An entry = one (scale, peer)
 * pair: the rows this rank receives from `peer` (its halo rows of that scale, local graph
 * numbering) and the rows it sends to `peer` (its owned rows the peer holds as halo, in the
 * peer's receive order).  Exchanged before every launch that gathers from other nodes:
 * U and out_0 before a layer's first hop, out_k before each further hop.  An entry whose peer
 * is the rank itself (equal receive and send counts) copies send row k to receive row k through
 * the transport -- RCCL send / recv to self in a one-rank communicator. */
typedef struct msw_exchange_desc {
  int32_t num_entries;
  const int32_t* peer;       /* [num_entries] peer rank */
  const int32_t* scale;      /* [num_entries] scale of the entry */
  const int64_t* recv_ptr;   /* [num_entries + 1] offsets into recv_rows */
  const int32_t* recv_rows;
  const int64_t* send_ptr;   /* [num_entries + 1] offsets into send_rows */
  const int32_t* send_rows;
} msw_exchange_desc;

/* Build CSR-by-destination per scale, pooling/unpooling maps, pack the weights for
 * the gfx950 kernels, allocate workspaces.  Host-synchronous; call once per graph. */
int msw_plan_create(const msw_graph_desc* graph, const msw_model_desc* model, int device,
                    msw_plan** out_plan);
int msw_plan_destroy(msw_plan* plan);

/* msw_plan_create for one rank of a partitioned mesh: `xch` describes its halo exchange
 * (hop pairs are not used: their halo is two rings deep).  The exchange itself runs either
 * over RCCL (msw_plan_set_comm, one process per GPU, inside msw_rollout; launched eagerly:
 * a partitioned plan is created with graph capture off, and msw_set_graph_capture(plan, 1) is
 * the only way to capture the RCCL exchanges too) or between plans of one process
 * (msw_group_rollout, validation on one GPU: the group's steps are captured as hipGraphs held
 * by plans[0] -- msw_set_group_graph(plans[0], 0) steps it eagerly). */
int msw_plan_create_part(const msw_graph_desc* graph, const msw_model_desc* model, int device,
                         const msw_exchange_desc* xch, int32_t rank, msw_plan** out_plan);

/* msw_plan_create with a base row order.  A plan keeps the caller's numbering at every boundary
 * (x, y, the rollout's out, node_bc, msw_debug_buffer) and lays each (graph, scale) range of
 * node_ptr out internally in graph order, moved only inside tiling.h's 64-row packing window, so
 * every row gather of the step inherits the caller's numbering.  row_order (HOST int64
 * [num_nodes], read during the call only) replaces the graph order: over every range [a, b) that
 * node_ptr names, row_order[a .. b) must be a permutation of a .. b-1, and the range's rows are
 * laid out in that order before the packing runs (on the in-degrees taken in that order).  No sum
 * changes its terms or their order, so the plan gives the bits of msw_plan_create's plan, in the
 * caller's numbering (msw_locality_order below builds such an order from coordinates).
 * row_order NULL: exactly msw_plan_create.
 * MSW_ERR_INVALID, naming the first offending position of row_order (ranges in node_ptr's order):
 * an entry outside its range (so an entry that crosses a scale or a graph), a repeated entry.
 * Partitioned plans (msw_plan_create_part) take no order. */
int msw_plan_create_ordered(const msw_graph_desc* graph, const msw_model_desc* model, int device,
                            const int64_t* row_order, msw_plan** out_plan);

/* The plan's internal row layout: perm[i] = graph row held by internal row i, -1 for a padding
 * row (scale starts are padded).  Writes min(capacity, npad) entries to perm (HOST) and the number
 * of internal rows to *npad; capacity = 0 (perm may be NULL) sizes the buffer.  Host only. */
int msw_plan_row_layout(const msw_plan* plan, int32_t* perm, int64_t capacity, int64_t* npad);

/* RCCL transport.  msw_comm_unique_id writes an ncclUniqueId (128 bytes) on the rank that
 * creates it; every rank then calls msw_plan_set_comm with the same bytes.  RCCL is bound
 * at run time from the process (the copy PyTorch loaded) or librccl.so.1. */
int msw_comm_unique_id(char* uid128);
int msw_plan_set_comm(msw_plan* plan, const char* uid128, int32_t nranks, int32_t rank);

/* All ranks' plans of one partitioned mesh in ONE process, stepped in lockstep with the
 * halo exchange done by device copies between the plans (no RCCL): validates the
 * decomposition on a single GPU.  Per-plan arrays: x0, bc, bc_tstride, node_bc, n_bc, out
 * as msw_rollout takes them. */
int msw_group_rollout(msw_plan* const* plans, int32_t num_plans, const float* const* x0,
                      const float* const* bc, const int32_t* bc_tstride,
                      const int32_t* const* node_bc, const int32_t* n_bc, int32_t type_bc,
                      int32_t T, float* const* out, void* stream);

/* One forward (MSGNN.forward / GNN.forward): x [N][num_node_features] -> y [N][2].
 * Does not modify x.  Equivalent to models/gnn.py:267-350 (MSGNN) or :102-152 (GNN).
 * With graph capture on (the default), the first call captures the forward schedule into a
 * hipGraph over plan-owned I/O slots; every call then enqueues copy x -> slot, one graph
 * launch, copy slot -> y (the reference's per-step rollout loop, train.py:87-95, calls this
 * once per step). */
int msw_forward(msw_plan* plan, const float* x, float* y, void* stream);

/* Autoregressive rollout (rollout_test, training/train.py:67-95 with
 * apply_boundary_condition / use_prediction, utils/dataset.py:486-529):
 *   for t in 0..T-1: x[node_bc, dyn + (type_bc-1) + 2 tau] = bc[b][tau][t]
 *                    pred = forward(x); x = shift(x, pred); out[:, :, t] = pred
 * x0 [N][nnf] (device, not modified), bc [n_bc][p][T_bc] device with T_bc >= T,
 * node_bc host int32 [n_bc] (node ids in the graph's numbering), out [N][2][T] device. */
int msw_rollout(msw_plan* plan, const float* x0, const float* bc, int32_t bc_time_stride,
                const int32_t* node_bc, int32_t n_bc, int32_t type_bc, int32_t T, float* out,
                void* stream);

/* Copy an internal per-node buffer ("x_s", "x_d", "x_down", "x_up") of the last forward
 * into dst (device, [N][F], graph numbering).  Debug / parity localisation only. */
int msw_debug_buffer(msw_plan* plan, const char* name, float* dst, void* stream);

/* Enable (1) / disable (0) graph capture of this plan's own rollout steps and msw_forward
 * (default 1, partitioned plans 0; 0 = every launch enqueued eagerly).  With a communicator
 * set, 1 captures the RCCL halo exchanges into the rollout graphs too. */
int msw_set_graph_capture(msw_plan* plan, int enable);
/* msw_group_rollout's own graphs (default 1): only the flag of the group's plans[0] is read,
 * and it is independent of msw_set_graph_capture. */
int msw_set_group_graph(msw_plan* plans0, int enable);

int msw_plan_get_stats(const msw_plan* plan, msw_plan_stats* stats);

/* The plan's launch schedule as text: one line per launch of a rollout step (rollout = 1)
 * or of msw_forward (rollout = 0), tab-separated key=value fields:
 *   kind     encode | edge_hop | edge_mlp | hop | pool | epi | decode | exchange
 *   variant  the kernel instantiation, a stable short name ("hop loop mid", "hop rows",
 *            "edge_coop4 pool", "encode loop stream", "pool rows loop", ...)
 *   nt scale prelu   F / 16, destination scale, compile-time PReLU path
 *   grid waves       workgroups launched (before XCD padding), waves per workgroup
 *   units per_wg     what the grid walks (edge tiles, row tiles, 64-row chunks or MLP chunks)
 *                    and how many of them a workgroup takes per round
 *   iters ragged     ceil(units / (grid * per_wg)): the most loop iterations any wave makes;
 *                    1 if the last round is partly empty
 *   lds              dynamic LDS bytes
 * Produced by the same code that chooses what the launchers launch.  Writes at most `cap`
 * bytes (NUL-terminated) to buf and the size needed, NUL included, to *needed; call with
 * cap = 0 (buf may be NULL) to size the buffer. */
int msw_plan_schedule(const msw_plan* plan, int32_t rollout, char* buf, int64_t cap, int64_t* needed);


/* Re-launch one kernel of the step `iters` times on `stream` (benchmark / roofline hook;
 * call after a forward or rollout: it reuses the plan's workspaces and overwrites scratch).
 *   kernel: 0 = middle hop (first processor on `scale`), 1 = fused edge MLP + hop 1
 *           (same processor), 2 = mean pooling + projection into `scale` (scale >= 1),
 *           3 = node encoders (+ projection of processor 0), 4 = unpooling layer into
 *           `scale` (scale < S-1) with its projection epilogue.
 * units_out (optional) receives {rows, edges} processed by ONE launch. */
int msw_bench_kernel(msw_plan* plan, int32_t kernel, int32_t scale, int32_t iters,
                     int64_t* units_out, void* stream);

/* On-device rollout evaluation (the reference's test-time metrics, finest scale only;
 * utils/miscellaneous.py:116-199, training/loss.py:8-35,120-169).  pred, real: device
 * [N][2][T] (graph numbering, as msw_rollout writes them); fine_ranges: host int64
 * [num_sims][2], the finest-scale row range of each simulation (node_ptr[g][0],
 * node_ptr[g][1]); thresholds: host float [n_thr] (n_thr <= 4) water-depth thresholds;
 * area: device float [N] cell areas by graph row (data.area), or NULL.
 * Outputs (device): sums written (fp64, workgroup partials added in a fixed order -- bit-
 * reproducible; stream-ordered scratch from hipMallocAsync), counts ZEROED by the caller
 * (exact integer atomics):
 *   sums   double [num_sims][T][10]: sum|dh|, sum|dv|, sum dh^2, sum dv^2, the same four
 *          over rows with dh != 0 or dv != 0 (mask_on_water), that row count, and the
 *          stored volume sum(area * h_pred) (0 when area is NULL);
 *   counts uint64 [num_sims][T][n_thr][4]: TP, TN, FP, FN of h_pred > thr vs h_real > thr.
 * A simulation with an empty range gets zero sums and its counts are left as they are.
 * Stream-ordered, no host synchronisation; needs no plan.  T = 0: no-op.  MSW_ERR_INVALID
 * (before any HIP call): NULL pred, real, fine_ranges or sums, NULL thresholds or counts with
 * n_thr > 0, n_thr outside 0..4, negative T or num_sims, a range with end < start, a negative
 * start, or an end past the kernel's int32 row indices. */
int msw_rollout_metrics(const float* pred, const float* real, int32_t T, const int64_t* fine_ranges,
                        int32_t num_sims, const float* thresholds, int32_t n_thr, const float* area,
                        double* sums, uint64_t* counts, void* stream);
/* The launch msw_rollout_metrics makes for one simulation of nrows finest rows over T steps (from
 * the code the launcher itself uses): workgroups along the rows (at most 512), chunks of 32 steps
 * (the grid is grid x time_chunks), rows a workgroup takes per round (256) and the rounds of its
 * grid-stride row loop, so that grid * rows_per_wg * iters >= nrows.  nrows = 0 or T = 0: grid,
 * time_chunks and iters are 0.  MSW_ERR_INVALID: negative nrows or T, a NULL output.  Host only. */
int msw_rollout_metrics_launch(int64_t nrows, int32_t T, int32_t* grid, int32_t* time_chunks,
                               int32_t* rows_per_wg, int32_t* iters);

/* On-device flood maps: a rollout reduced over time into per-cell maps, the sibling of
 * msw_rollout_metrics.  The reference builds them on the host after every rollout:
 * flood-arrival time WD_to_FAT (utils/miscellaneous.py:56-68, it counts wet steps), peak depth
 * and discharge (utils/visualization.py:592-598), velocity and Froude number get_velocity /
 * get_Froude (utils/miscellaneous.py:44-54). */
#define MSW_MAX_MAP_THRESHOLDS 4
typedef struct {            /* device pointers; NULL = this map is not produced            */
  float*   h_max;           /* [nrows]                                                      */
  int32_t* t_h_max;         /* [nrows] first global step attaining h_max                    */
  float*   q_max;           /* [nrows] max |pred[:,1,:]|                                    */
  int32_t* t_q_max;
  float*   vel_max;         /* [nrows] max_t get_velocity(|q|, h, vel_eps)                  */
  float*   froude_max;      /* [nrows] max_t get_Froude(vel, h)                             */
  int32_t* wet_steps;       /* [n_thr][nrows] number of steps with h > thr                  */
  int32_t* first_wet;       /* [n_thr][nrows] first / last global step with h > thr, or -1  */
  int32_t* last_wet;
} msw_flood_maps;

/* Reduce steps t_begin .. t_begin + t_count - 1 of rows row0 .. row0 + nrows - 1 of pred (device
 * [N][2][T], graph numbering, as msw_rollout writes it) into the maps (indexed by row - row0).
 * The global step of column t is t_offset + (t - t_begin).  Per (row, step), with
 * h = pred[n][0][t] and q = |pred[n][1][t]|:
 *   vel = h > vel_eps ? q / h : 0          fr = h > 0 ? vel / sqrtf(9.81f * h) : 0
 *   wet at threshold k iff h > thresholds[k]   (host float [n_thr], n_thr <= 4; strict)
 * first = 1: the arrays are overwritten and need no initialisation.  first = 0: they hold the
 * state of earlier calls and are continued -- a maximum moves only to a strictly larger value
 * (the earliest step keeps a tie), first_wet is kept once set, last_wet and wet_steps advance --
 * so a rollout fed piece by piece gives the maps of the whole.  The division and square root are
 * skipped when vel_max and froude_max are both NULL, the threshold work when n_thr = 0.  Inputs
 * are finite (the decoder's outputs are); NaN behaviour is unspecified.
 * Stream-ordered, no host synchronisation, no allocation; needs no plan.  t_count = 0 or
 * nrows = 0: no-op.  MSW_ERR_INVALID (before any HIP call): NULL pred or maps, NULL thresholds
 * with n_thr > 0, n_thr outside 0..4, a window outside [0, T], negative row0 / nrows. */
int msw_flood_maps_update(const float* pred, int32_t T, int32_t t_begin, int32_t t_count,
                          int32_t t_offset, int64_t row0, int64_t nrows,
                          const float* thresholds, int32_t n_thr, float vel_eps,
                          int32_t first, const msw_flood_maps* maps, void* stream);
/* The launch msw_flood_maps_update makes for that size (from the code the launcher itself uses):
 * workgroups, rows a workgroup takes per round, and the rounds of its row loop, so that
 * grid * rows_per_wg * iters >= nrows.  Windows longer than 1024 steps run as successive
 * launches of at most 1024 steps; the numbers are those of each. */
int msw_flood_maps_launch(int64_t nrows, int32_t t_count, int32_t* grid, int32_t* rows_per_wg,
                          int32_t* iters);

/* On-device zone series: a rollout reduced over space into per-(zone, step) series, the spatial
 * sibling of the flood maps.  A zone is a list of graph rows (a district, a river reach, one
 * simulation of a batch); a gauge is a zone of one row.  The reference has no counterpart beyond
 * the stored volume inside its mass-conservation metric (training/loss.py:120-169).
 *
 * A zone set is built once per mesh: zone z = rows zone_rows[zone_ptr[z] .. zone_ptr[z+1]) (HOST
 * arrays, zone_ptr [num_zones + 1] starting at 0; graph row ids in [0, num_rows), in any order; a
 * row may appear in several zones or twice in one -- it then counts twice; empty zones allowed).
 * The handle holds device copies of the lists, the launch's work list and the scratch of the
 * partial sums, so updates that share a handle must be ordered on one stream.  device = -1 makes
 * a host-only handle that answers msw_zone_series_launch and cannot be updated.
 * MSW_ERR_INVALID, before any HIP call and with nothing allocated: a row id outside
 * [0, num_rows), a zone_ptr that does not start at 0 or is not monotone, NULLs. */
typedef struct msw_zones msw_zones;
int msw_zones_create(const int64_t* zone_ptr, const int32_t* zone_rows, int64_t num_zones,
                     int64_t num_rows, int device, msw_zones** out);
int msw_zones_destroy(msw_zones* zones);

typedef struct {          /* device pointers, NULL = not produced; leading stride T_out            */
  double*  volume;        /* [Z][T_out]        sum (double)a * (double)h over the zone's rows       */
  double*  wet_area;      /* [n_thr][Z][T_out] sum (double)a over rows with h > thr_k (strict)      */
  int32_t* wet_cells;     /* [n_thr][Z][T_out] number of such rows                                  */
  float*   h_max;         /* [Z][T_out]        max h   (0 for an empty zone)                        */
  float*   q_max;         /* [Z][T_out]        max |pred[:,1,:]| (0 for an empty zone)              */
} msw_zone_series;

/* Steps t_begin .. t_begin + t_count - 1 of pred (device [N][2][T], graph numbering, N = num_rows
 * of the zone set) -> columns t_out0 .. t_out0 + t_count - 1 of the outputs; columns outside the
 * window are not touched, the window's are overwritten (no initialisation needed).
 * a = area[row] (device float [N]) or 1.0f when area is NULL.  thresholds: host float [n_thr],
 * n_thr <= MSW_MAX_MAP_THRESHOLDS.
 * wet_cells, h_max and q_max are exact.  volume and wet_area are fp64 sums of terms that are exact
 * in fp64, added in an order that the row list alone fixes: chunks of 256 consecutive list entries
 * summed in list order from 0, then -- for a zone of several chunks -- the chunk sums in chunk
 * order.  No atomics: the sums are the same bit for bit from call to call and however a rollout is
 * cut into windows or pieces.  Inputs are finite; NaN behaviour is unspecified.
 * Stream-ordered, no host synchronisation, no allocation.  t_count = 0 or no zones: no-op.
 * MSW_ERR_INVALID (before any HIP call): NULL zones, pred or out, NULL thresholds with n_thr > 0,
 * n_thr outside 0..4, a window outside [0, T], t_out0 < 0 or t_out0 + t_count > T_out. */
int msw_zone_series_update(const msw_zones* zones, const float* pred, int32_t T, int32_t t_begin,
                           int32_t t_count, const float* area, const float* thresholds, int32_t n_thr,
                           int32_t T_out, int32_t t_out0, const msw_zone_series* out, void* stream);
/* The launch msw_zone_series_update makes for that window (from the code the launcher itself
 * uses).  A unit is one chunk of a zone's list x one tile of 64 steps: workgroups, units a
 * workgroup takes per round of its loop (1: a workgroup is one wave) and the rounds, so that
 * grid * units_per_wg * iters >= units.  Windows longer than the handle's scratch holds (at most
 * 1024 steps) run as successive launches; the numbers are those of the first. */
int msw_zone_series_launch(const msw_zones* zones, int32_t t_count, int32_t* grid,
                           int32_t* units_per_wg, int32_t* iters);

/* On-device ensemble products: statistics ACROSS the members of an ensemble -- one mesh run with
 * M boundary hydrographs, breach locations or initial states -- the third sibling: the flood maps
 * reduce over time, the zone series over space, these over members.  The reference has no
 * counterpart.
 *
 * An ensemble is M members, 1 <= M <= MSW_MAX_ENSEMBLE_MEMBERS, of n cells each.  Member m occupies
 * rows member_row0[m] .. member_row0[m] + n - 1 of pred (device [N][2][T], graph numbering, as
 * msw_rollout writes it): cell i of member m is row member_row0[m] + i.  For a batch of M copies of
 * one mesh these are the finest-scale ranges of the batch (equal lengths, coarse rows in between).
 * member_row0 is a HOST int64 [M] array in any order; the kernel takes it by value in its
 * arguments.  A range may repeat and that member then counts twice.  Member order is the order of
 * that list: every tie-break and every sum below uses it.  Larger ensembles, and merging the
 * statistics of separately reduced groups, are out of scope. */
#define MSW_MAX_ENSEMBLE_MEMBERS 64
#define MSW_MAX_ENSEMBLE_RANKS 8

typedef struct {            /* device pointers, NULL = not produced; leading stride T_out           */
  int32_t* wet_members;     /* [n_thr][n][T_out] number of members with h_m > thr_k (strict)        */
  float*   h_mean;          /* [n][T_out] (float)(S / (double)M), S = fp64 sum of (double)h_m added
                               in member order from 0                                               */
  float*   h_min;           /* [n][T_out] smallest h_m over the members                             */
  float*   h_max;           /* [n][T_out] largest h_m over the members                              */
} msw_ensemble_steps_out;

/* Per-step statistics across members, the streaming pass: steps t_begin .. t_begin + t_count - 1
 * of cells 0 .. n - 1, with h_m = pred[member_row0[m] + i][0][t], -> columns t_out0 ..
 * t_out0 + t_count - 1 of the outputs; columns outside the window are not touched, the window's
 * are overwritten (no initialisation needed).  thresholds: host float [n_thr],
 * n_thr <= MSW_MAX_MAP_THRESHOLDS.
 * Every depth of the window is read once, the discharge half of a row never.  No atomics, no
 * scratch, no allocation: the results are the same bit for bit from call to call and however the
 * horizon is cut into windows.  Inputs are finite; NaN behaviour is unspecified.
 * Stream-ordered, no host synchronisation; needs no plan.  t_count = 0 or n = 0: no-op.
 * MSW_ERR_INVALID (before any HIP call): NULL pred, out or member_row0, NULL thresholds with
 * n_thr > 0, n_thr outside 0..4, M outside 1..64, a window outside [0, T], t_out0 < 0 or
 * t_out0 + t_count > T_out, negative n or a negative member_row0. */
int msw_ensemble_steps_update(const float* pred, int32_t T, int32_t t_begin, int32_t t_count,
                              const int64_t* member_row0, int32_t M, int64_t n,
                              const float* thresholds, int32_t n_thr, int32_t T_out, int32_t t_out0,
                              const msw_ensemble_steps_out* out, void* stream);
/* The launch msw_ensemble_steps_update makes for that size (from the code the launcher itself
 * uses): workgroups, cells a workgroup takes per round, and the rounds of its cell loop, so that
 * grid * cells_per_wg * iters >= n.  n = 0 or t_count = 0: grid and iters are 0.
 * MSW_ERR_INVALID: negative n or t_count, M outside 1..64, a NULL output.  Host only. */
int msw_ensemble_steps_launch(int64_t n, int32_t M, int32_t t_count, int32_t* grid,
                              int32_t* cells_per_wg, int32_t* iters);

typedef struct {                /* device pointers, NULL = not produced                             */
  int32_t* exceed_members;      /* [n_thr][n]   number of members with value_m > thr_k (strict)     */
  float*   mean;                /* [n]          as h_mean above, over values                        */
  float*   rank_values;         /* [n_ranks][n] the value whose rank is ranks[j]                    */
  int32_t* members_with_step;   /* [n]          number of members with steps_m >= 0                 */
  int32_t* rank_steps;          /* [n_ranks][n] the step whose rank is ranks[j], or -1              */
} msw_ensemble_maps_out;

/* Order statistics across members of per-member maps, one shot, no carry-over.  values: device
 * float [M][n] (e.g. each member's h_max) or NULL; steps: device int32 [M][n] (e.g. first_wet at
 * one threshold, -1 = never) or NULL; the outputs of a NULL input are not produced.  ranks: host
 * int32 [n_ranks], n_ranks <= MSW_MAX_ENSEMBLE_RANKS, each in 0..M-1, duplicates allowed.
 *   values  member m has rank #{m' : v_m' < v_m, or v_m' == v_m and m' < m}: a stable ascending
 *           sort by member order; rank 0 is the minimum, rank M - 1 the maximum.
 *   steps   the same order with -1 sorting after every step: rank_steps[j] is -1 when fewer than
 *           ranks[j] + 1 members have a step, else the first step by which at least ranks[j] + 1
 *           members have been wet.
 * No arithmetic touches the selected values: they are exact.  Inputs are finite; NaN behaviour is
 * unspecified.  Stream-ordered, no host synchronisation, no allocation.  n = 0: no-op.
 * MSW_ERR_INVALID (before any HIP call): NULL out, NULL thresholds with n_thr > 0, NULL ranks with
 * n_ranks > 0, n_thr outside 0..4, M outside 1..64, n_ranks outside 0..8, a rank outside 0..M-1,
 * negative n. */
int msw_ensemble_maps(const float* values, const int32_t* steps, int32_t M, int64_t n,
                      const float* thresholds, int32_t n_thr, const int32_t* ranks, int32_t n_ranks,
                      const msw_ensemble_maps_out* out, void* stream);

/* Ensemble scores: the members of an ensemble verified against a truth run, the probabilistic
 * sibling of msw_rollout_metrics.  Per cell i and step t, in fp64 on the converted float32 depths
 * h_m = pred[member_row0[m] + i][0][t] and y = truth[truth_row0 + i][0][t_truth0 + (t - t_begin)]:
 *   a = sum_m |h_m - y|     b = sum_{m<m'} |h_m - h_m'|     S = sum_m h_m (member order from 0)
 *   e = S - M y             v = M sum_m h_m^2 - S^2         (M^2 times the population variance)
 *   c_k = number of members with h_m > thr_k (strict, float32 against float32), o_k = y > thr_k.
 * b is taken as sum_m (2 rank_m - M + 1) h_m over the stable ascending order of the members (the
 * ranks of msw_ensemble_maps).  The kernel never divides by M or n: CRPS = sum a / (M n) -
 * sum b / (M^2 n), the ensemble mean's MAE = sum |e| / (M n) and RMSE = sqrt(sum e^2 / (M^2 n)),
 * the spread = sqrt(sum v / (M^2 n)); the Brier score and its decomposition follow from the table. */
typedef struct {            /* device pointers, NULL = not produced                                  */
  double*  sums;            /* [T_out][5] column t_out0 + (t - t_begin): the sums over the n cells of
                               a, b, |e|, e^2, v; overwritten                                         */
  int64_t* reliability;     /* [T_out][n_thr][M + 1][2]: per threshold and forecast count c = 0..M the
                               number of cells with c_k = c, and how many of those have o_k;
                               overwritten                                                            */
  double*  cell_crps;       /* [n] ACCUMULATED: per step cell_crps[i] += M a - b, one addition per step
                               in step order onto the carried value; the caller zeroes it.  Divided by
                               M^2 and the steps seen: the time-mean CRPS map                         */
} msw_ensemble_scores_out;

/* Steps t_begin .. t_begin + t_count - 1 of cells 0 .. n - 1 -> columns t_out0 .. of sums and
 * reliability (columns outside the window are not touched) and onto cell_crps.  truth: device
 * [*][2][T_truth], the same layout as pred; it may be pred itself (a control run that is not a
 * member).  member_row0, thresholds: host arrays, as for msw_ensemble_steps_update.
 * Order: the cells are cut into blocks whose length depends on n alone; a block is added in cell
 * order, the blocks in block order (a second small kernel over stream-ordered scratch), without
 * atomics -- so sums is the same bit for bit however the horizon is cut into windows, and so is
 * cell_crps.  Integers are exact.  A NaN member or truth depth makes the five terms of its cell
 * and step NaN (the step's sums, the cell's cell_crps from then on) and counts as "not above".
 * Every depth of the window is read once; rows outside the member ranges and the truth range and
 * the discharge half of every row are never read.  Stream-ordered, no host synchronisation; needs
 * no plan.  t_count = 0, n = 0 or no output asked for: no-op.
 * MSW_ERR_INVALID (before any HIP call): NULL pred, truth, out or member_row0, NULL thresholds with
 * n_thr > 0, n_thr outside 0..4, M outside 1..64, negative n, member_row0 or truth_row0, a window
 * outside [0, T], truth columns outside [0, T_truth], output columns outside [0, T_out]. */
int msw_ensemble_scores_update(const float* pred, int32_t T, int32_t t_begin, int32_t t_count,
                               const int64_t* member_row0, int32_t M, int64_t n,
                               const float* truth, int32_t T_truth, int32_t t_truth0, int64_t truth_row0,
                               const float* thresholds, int32_t n_thr, int32_t T_out, int32_t t_out0,
                               const msw_ensemble_scores_out* out, void* stream);
/* The launch msw_ensemble_scores_update makes for that size (from the code the launcher itself
 * uses): workgroups (= blocks of cells: a function of n alone), cells a workgroup takes per round
 * and the rounds of its cell loop per tile of steps, so that grid * cells_per_wg * iters >= n.
 * n = 0 or t_count = 0: grid and iters are 0.  MSW_ERR_INVALID: negative n or t_count, M outside
 * 1..64, a NULL output.  Host only. */
int msw_ensemble_scores_launch(int64_t n, int32_t M, int32_t t_count, int32_t* grid,
                               int32_t* cells_per_wg, int32_t* iters);

/* Raster products: per-cell maps and rollout frames resampled onto a regular grid, the last step
 * between a rollout on the device and a layer a GIS, a warning system or a web viewer takes.  The
 * reference resamples on the host with a plotting library (plot_faces, a PolyCollection); there is
 * no numerical counterpart.  Every output is an index decided by fp64 predicates evaluated in the
 * written order below, or a 32-bit word copied unchanged: all of it is exact.
 *
 * Geometry of ONE mesh scale: node_xy float64 [num_nodes][2], face_nodes int32 [num_faces][3]
 * (triangles; the signature admits nothing else), optional face_row int32 [num_faces]: the graph
 * row that holds face f's value (NULL: f; -1: the face has no value -- it still takes part in
 * the location and yields -1).  All three are HOST arrays.  The grid: pixel (i, j), element
 * j * width + i, has the centre px = x0 + (double)i * dx, py = y0 + (double)j * dy (one multiply,
 * one add, no fma); dx and dy may be negative (north-up rasters).
 *
 * Edge function of the directed edge (u -> v) at a pixel: p = whichever of u, v has the LOWER
 * vertex index, q = the other;
 *     E = (q.x - p.x) * (py - p.y) - (q.y - p.y) * (px - p.x)
 * in float64, every operation rounded on its own; E is negated when u was not the lower one.  Both
 * faces of a shared edge see the same magnitude with opposite signs: a pixel near a shared edge
 * cannot be rejected by both.
 * Face (a, b, c): area2 = (b.x - a.x) * (c.y - a.y) - (b.y - a.y) * (c.x - a.x).  area2 == 0 (or
 * NaN): the face contains nothing.  area2 > 0: it contains the pixel iff E(a->b), E(b->c), E(c->a)
 * are all >= 0; area2 < 0: iff all three are <= 0.  A pixel contained in several faces (on an
 * edge, at a vertex, in overlapping faces) takes the LOWEST face index.
 *     pixel_rows[j][i] = face_row[f] of that face, or -1 when no face contains the pixel.
 *
 * msw_raster_create copies the geometry, builds on the host a uniform bucket grid over the mesh
 * (face indices per bucket, ascending; a face is listed in every bucket its bounding box, widened
 * by a rounding margin, touches), uploads it, runs the locate kernel on `stream` and waits for
 * it: on return pixel_rows is complete and the handle may be used on any stream.  The handle owns
 * its device memory; calls that share a handle need no ordering among themselves (they only read).
 * MSW_ERR_INVALID, with nothing allocated: NULLs (face_row may be NULL), negative counts, a
 * non-finite coordinate or grid number, dx or dy zero, width or height < 1, width * height >
 * 2^31 - 1, a vertex index outside [0, num_nodes), a face_row below -1, device < 0.
 * MSW_ERR_UNSUPPORTED: more than 2^26 faces. */
typedef struct {
  double  x0, y0;         /* centre of pixel (0, 0)                                                 */
  double  dx, dy;         /* pixel pitch, != 0, either sign                                          */
  int32_t width, height;  /* >= 1, width * height <= 2^31 - 1                                        */
} msw_raster_grid;

typedef struct {
  int64_t buckets;            /* buckets of the host-built grid (buckets_x * buckets_y)             */
  int64_t list_entries;       /* face indices over all bucket lists                                 */
  int64_t longest_list;       /* faces in the longest bucket list                                   */
  int64_t device_bytes;       /* device memory the handle owns                                      */
  double  host_build_seconds; /* host time of the checks, the face records and the bucket grid      */
  double  locate_us;          /* device time of the locate kernel (events around it, at create)     */
  int32_t buckets_x, buckets_y;
} msw_raster_stats;

typedef struct msw_raster msw_raster;
int msw_raster_create(const double* node_xy, int64_t num_nodes, const int32_t* face_nodes,
                      const int32_t* face_row, int64_t num_faces, const msw_raster_grid* grid,
                      int device, void* stream, msw_raster** out);
int msw_raster_destroy(msw_raster* raster);
/* *pixel_rows = the handle's device array int32 [height][width]; it lives as long as the handle. */
int msw_raster_pixel_rows(const msw_raster* raster, const int32_t** pixel_rows);
int msw_raster_get_stats(const msw_raster* raster, msw_raster_stats* stats);

/* out[l][j][i] = the 32-bit word layers[l * layer_stride + row_offset + pixel_rows[j][i]], or the
 * word nodata_bits where pixel_rows is -1.  layers (device, float32 or int32 alike: words are
 * copied as bits, NaN payloads and -0.0 survive) holds num_rows words per layer that may be
 * addressed; out is device [num_layers][height][width].  row_offset lets one handle serve every
 * member of an ensemble batch and every simulation on the same mesh.  Stream-ordered, no host
 * synchronisation, no allocation.  num_layers = 0: no-op.
 * MSW_ERR_INVALID (before any HIP call): NULL raster, layers or out, negative num_layers,
 * layer_stride or num_rows, a face_row of the handle for which row_offset + face_row lies outside
 * [0, num_rows) (checked against the smallest and the largest face_row >= 0). */
int msw_raster_sample(const msw_raster* raster, const void* layers, int32_t num_layers,
                      int64_t layer_stride, int64_t row_offset, int64_t num_rows,
                      uint32_t nodata_bits, void* out, void* stream);
/* Frames of a rollout pred (device float32 [N][2][T], graph numbering):
 *     out[k][j][i] = pred[row_offset + pixel_rows[j][i]][var][t_begin + k],  k < t_count,
 * or nodata_bits; out is device, frame-major [t_count][height][width].  A row's steps are fetched
 * with 16-byte loads where pred, T and t_begin are multiples of 16 bytes / 4 steps.  Stream-ordered,
 * no host synchronisation, no allocation.  t_count = 0: no-op.
 * MSW_ERR_INVALID (before any HIP call): NULL raster, pred or out, var not 0 or 1, negative N or T,
 * a window outside [0, T], a face_row for which row_offset + face_row lies outside [0, N). */
int msw_raster_frames(const msw_raster* raster, const float* pred, int64_t N, int32_t T, int32_t var,
                      int32_t t_begin, int32_t t_count, int64_t row_offset, uint32_t nodata_bits,
                      void* out, void* stream);
/* The launch of the locate kernel for a width x height grid (from the code the launcher itself
 * uses): one-wave workgroups, each taking one 8 x 8 pixel block (pixels_per_wg = 64, blocks in
 * row-major order, ragged at the right and bottom rims) per round of its loop, so that
 * grid * iters >= ceil(width / 8) * ceil(height / 8).  msw_raster_sample and msw_raster_frames walk
 * rounds of 64 consecutive pixels under the same cap of 4096 workgroups.
 * MSW_ERR_INVALID: a NULL output, width or height < 1, too many pixels.  Host only. */
int msw_raster_launch(int32_t width, int32_t height, int32_t* grid, int32_t* pixels_per_wg,
                      int32_t* iters);

/* Zonal statistics: raster layers and frame stacks reduced onto the cells of one mesh scale, the
 * transpose of the raster products -- a DEM, a roughness layer, an observed depth raster or the
 * frames of a raster model become per-cell values and [N][2][T] rows.  Centres only, as above: a
 * pixel belongs to the face that pixel_rows names for it, whole.  The reference has no counterpart.
 *
 * msw_zonal_create builds on the device, from a raster handle, and owns
 *   face_ptr     int32 [num_faces + 1], pixels int32 [face_ptr[num_faces]]: the list of face f,
 *                pixels[face_ptr[f] .. face_ptr[f + 1]), holds exactly the pixel indices
 *                p = j * width + i with pixel_rows[p] == face_row[f], ascending; empty for a face
 *                with face_row -1 and for a zero-area face.  The lists together are a permutation
 *                of {p : pixel_rows[p] >= 0}.
 *   centre_pixel int32 [num_faces]: the pixel nearest to the face's centroid, in float64, every
 *                operation rounded on its own: cx = ((a.x + b.x) + c.x) / 3.0 (cy likewise),
 *                i = floor((cx - x0) / dx + 0.5), j = floor((cy - y0) / dy + 0.5); j * width + i
 *                when 0 <= i < width and 0 <= j < height, else -1.
 * The handle copies what it needs: it outlives the raster handle, and calls that share it need no
 * ordering among themselves (they only read).  Create runs on `stream` and waits for it.
 * MSW_ERR_INVALID: a NULL argument.  MSW_ERR_UNSUPPORTED: two faces with the same face_row >= 0
 * (the lists are keyed by face; such a mesh would count pixels twice).  A refusal leaves nothing
 * allocated. */
typedef struct {
  int64_t num_faces;
  int64_t listed_pixels;  /* face_ptr[num_faces]                                                   */
  int64_t longest_list;   /* pixels in the longest list                                            */
  int64_t empty_faces;    /* faces with face_row >= 0 and an empty list                            */
  int64_t wave_faces;     /* faces with more than 32 pixels: msw_zonal_reduce's second launch      */
  int64_t device_bytes;   /* device memory the handle owns                                         */
  double  build_us;       /* host clock around create: kernels, copies and the host prefix sum     */
} msw_zonal_stats;

typedef struct msw_zonal msw_zonal;
int msw_zonal_create(const msw_raster* raster, void* stream, msw_zonal** out);
int msw_zonal_destroy(msw_zonal* zonal);
/* The handle's device arrays; they live as long as the handle. */
int msw_zonal_lists(const msw_zonal* zonal, const int32_t** face_ptr, const int32_t** pixels,
                    const int32_t** centre_pixel);
int msw_zonal_get_stats(const msw_zonal* zonal, msw_zonal_stats* stats);

/* Per-cell statistics of layers (device float32 [num_layers][height][width], layer l at
 * layers + l * layer_stride).  Four outputs, each device [num_layers][out_stride] or NULL: mean
 * and vmin / vmax float32, count int32.  Face f with r = face_row[f] >= 0 writes element
 * l * out_stride + row_offset + r of every output given; every other element is left untouched,
 * so one call per scale fills one [N] array of a multiscale graph.  Per face and layer:
 *   a pixel whose value is NaN is skipped; count = the pixels not skipped;
 *   mean = (float)(S / (double)count), S the float64 sum of the remaining values started from
 *   +0.0 (a cell of -0.0 pixels has mean +0.0).  The order of the sum is a function of the list
 *   alone (not of the layer count, offsets, stream or repetition): a list of n <= 32 entries is
 *   summed front to back; a longer one as 64 partial sums, partial k over the entries k, k + 64,
 *   k + 128, ... front to back from +0.0, which are then combined pairwise: s[k] + s[k ^ 32], then
 *   ^ 16, ^ 8, ^ 4, ^ 2, ^ 1;
 *   vmin / vmax = one pixel's own word, copied as bits, the least / greatest by IEEE comparison
 *   with -0.0 below +0.0 (no dependence on order);
 *   count == 0: with fill_centre != 0 and centre_pixel[f] >= 0, mean, vmin and vmax take that
 *   pixel's word of the layer, copied as bits (a NaN included); otherwise nodata_bits.  count stays 0.
 * Stream-ordered, no host synchronisation, no allocation.  num_layers = 0: no-op.
 * MSW_ERR_INVALID (before any HIP call): NULL zonal or layers, all four outputs NULL, negative
 * num_layers, layer_stride, num_rows or out_stride, a face_row for which row_offset + face_row
 * lies outside [0, num_rows). */
int msw_zonal_reduce(const msw_zonal* zonal, const float* layers, int32_t num_layers,
                     int64_t layer_stride, int64_t row_offset, int64_t num_rows, int64_t out_stride,
                     int32_t fill_centre, uint32_t nodata_bits, float* mean, int32_t* count,
                     float* vmin, float* vmax, void* stream);
/* The inverse of msw_raster_frames: frames (device float32 [t_count][height][width], frame k at
 * frames + k * frame_stride) into a rollout array pred (device float32 [N][2][T]):
 *     pred[row_offset + face_row[f]][var][t_begin + k] = the mean msw_zonal_reduce gives for
 * frame k and face f, bit for bit (the same device function), fill_centre and nodata_bits
 * included.  Nothing else in pred is touched.  Stream-ordered, no host synchronisation, no
 * allocation.  t_count = 0: no-op.
 * MSW_ERR_INVALID (before any HIP call): NULL zonal, frames or pred, var not 0 or 1, negative N, T
 * or frame_stride, a window outside [0, T], a face_row for which row_offset + face_row lies
 * outside [0, N). */
int msw_zonal_frames(const msw_zonal* zonal, const float* frames, int64_t frame_stride, float* pred,
                     int64_t N, int32_t T, int32_t var, int32_t t_begin, int32_t t_count,
                     int64_t row_offset, int32_t fill_centre, uint32_t nodata_bits, void* stream);
/* The launch of the reduce kernel over num_faces faces (from the code the launcher itself uses):
 * one-wave workgroups, each taking faces_per_wg = 64 consecutive faces per round of its loop, so
 * that grid * 64 * iters >= num_faces; a lane reduces the list of its face when it holds at most
 * 32 pixels.  The wave_faces faces with longer lists go to a second launch, one face per wave and
 * round, of min(wave_faces, the same cap of 4096) workgroups; a launch with no face to take is not
 * made.  num_faces = 0: grid and iters are 0.
 * MSW_ERR_INVALID: a NULL output, num_faces negative.  Host only. */
int msw_zonal_launch(int64_t num_faces, int32_t* grid, int32_t* faces_per_wg, int32_t* iters);

/* Mesh graphs: the way INTO the engine from a plain triangulation -- arbitrary points located in
 * the triangles of one mesh scale, and the dual graph of one scale from its coordinates and vertex
 * lists alone.  mswegnn/meshgraph.py assembles both into a multiscale graph in the reference's
 * layout (database/graph_creation.py builds its graphs on the host with meshkernel, networkx and
 * one matplotlib Path.contains_points call per coarse face, O(N_coarse * N_fine)).  Every index is
 * decided by the fp64 predicates of "Raster products" or by vertex lists; every float64 output is
 * a stated sequence of IEEE operations, each rounded on its own (no fma).
 *
 * a) Point locator.  Geometry as for msw_raster_create (HOST arrays; face_row NULL: f; -1: the face
 * takes part and yields -1), the same face records, bucket grid and rounding margin, no pixel grid.
 *     rows[i] = face_row[f] of the LOWEST face f that contains (xy[i][0], xy[i][1]), else -1,
 * "contains" being exactly the rule of "Raster products": the edge functions taken from the lower
 * vertex index, E >= 0 (area2 > 0) or E <= 0 (area2 < 0) on all three edges, a face with area2 == 0
 * contains nothing.  A point outside the bucket grid (the faces' bounding boxes, each widened by
 * its margin) gets -1 without touching memory; so does a point with a NaN or an infinite
 * coordinate.  msw_locator_create is host-synchronous (the build and three uploads, no kernel);
 * msw_locate_points (xy device float64 [n][2], rows device int32 [n]) is stream-ordered, without
 * host synchronisation or allocation, and only reads the handle.  n = 0: no-op.
 * MSW_ERR_INVALID: as msw_raster_create for the geometry; NULL loc, xy or rows; negative n; xy not
 * 8-byte or rows not 4-byte aligned.  MSW_ERR_UNSUPPORTED: more than 2^26 faces. */
typedef struct {
  int64_t buckets;            /* buckets of the host-built grid (buckets_x * buckets_y)             */
  int64_t list_entries;       /* face indices over all bucket lists                                 */
  int64_t longest_list;       /* faces in the longest bucket list                                   */
  int64_t device_bytes;       /* device memory the handle owns                                      */
  double  host_build_seconds; /* host time of the checks, the face records and the bucket grid      */
  int32_t buckets_x, buckets_y;
} msw_locator_stats;

typedef struct msw_locator msw_locator;
int msw_locator_create(const double* node_xy, int64_t num_nodes, const int32_t* face_nodes,
                       const int32_t* face_row, int64_t num_faces, int device, msw_locator** out);
int msw_locator_destroy(msw_locator* loc);
int msw_locator_get_stats(const msw_locator* loc, msw_locator_stats* stats);
int msw_locate_points(const msw_locator* loc, const double* xy, int64_t n, int32_t* rows, void* stream);
/* The launch of the locate kernel for n points (from the code the launcher itself uses): one-wave
 * workgroups, each taking points_per_wg = 64 consecutive points per round of its loop, at most 4096
 * workgroups, so that grid * 64 * iters >= n.  n = 0: grid and iters are 0.
 * MSW_ERR_INVALID: a NULL output, n negative.  Host only. */
int msw_locate_launch(int64_t n, int32_t* grid, int32_t* points_per_wg, int32_t* iters);

/* b) Dual graph of one scale: graph nodes are faces, two faces are joined when they share an edge.
 * From node_xy float64 [num_nodes][2] and face_nodes int32 [num_faces][3] (HOST arrays; faces in
 * either orientation, vertices that no face uses allowed) msw_mesh_dual_create builds and owns, on
 * the device, with a = face_nodes[f][0], b = [1], c = [2]:
 *   centroid    float64 [num_faces][2]: ((a.x + b.x) + c.x) / 3.0, y likewise;
 *   area        float64 [num_faces]: 0.5 * fabs((b.x - a.x) * (c.y - a.y) - (c.x - a.x) * (b.y - a.y));
 *   adjacent    int32 [num_faces][3]: slot 0 is the edge (a, b), 1 (b, c), 2 (c, a); the other face
 *               that holds both vertices of the edge, -1 where there is none (a boundary edge);
 *   edge_index  int64 [2][num_edges]: every dual edge in both directions, sorted by (row, column):
 *               rows ascend, the columns of a row ascend (PyG to_undirected's coalesced order);
 *   edge_length float64 [num_edges]: dx = centroid[col].x - centroid[row].x, dy likewise,
 *               sqrt(dx * dx + dy * dy), the root rounded to nearest like the other operations (the
 *               kernel corrects the device's sqrt with one exact residual);
 *   boundary    int32 [num_boundary][2]: the (face, slot) pairs with adjacent == -1, face-major,
 *               slots ascending; num_edges + num_boundary = 3 * num_faces.
 * Create is host-synchronous: the host checks each face and builds a vertex -> incident-faces CSR
 * (faces ascending in every list), a kernel (lane = face) computes centroid, area, adjacent and the
 * number of neighbours by walking the star of each edge's lower vertex, the host takes the prefix
 * sum, a second kernel (lane = face) writes edge_index, edge_length and boundary.  No atomics: no
 * output bit depends on an order of execution.  Both kernels run on `stream`; create waits for it.
 * MSW_ERR_INVALID with a message "face F: ...": the checks run in this order and the message names
 * the lowest face that fails the first check that fails --
 *   faces one at a time: a vertex index outside [0, num_nodes), a repeated vertex, a non-finite
 *   coordinate, area2 zero or not finite;
 *   then a non-finite coordinate of a vertex that no face uses (no face is named);
 *   then, over the whole mesh: an edge shared by more than two faces, two faces that share more than
 *   one edge.
 * Also MSW_ERR_INVALID: NULLs, negative counts, device < 0.  MSW_ERR_UNSUPPORTED: more than 2^26
 * faces.  A refusal leaves nothing allocated.  num_faces = 0: every array is empty (NULL). */
typedef struct {
  int64_t num_faces, num_edges, num_boundary;
  int64_t longest_star;       /* faces round the vertex with the most                               */
  int64_t device_bytes;       /* device memory the handle owns                                      */
  double  host_build_seconds; /* host: the checks, the vertex CSR, the prefix sum                   */
  double  create_seconds;     /* host clock around all of create: host build, copies, both kernels  */
  double  faces_us, edges_us; /* device time of the two kernels (events around each)                */
} msw_mesh_dual_stats;

typedef struct msw_mesh_dual msw_mesh_dual;
int msw_mesh_dual_create(const double* node_xy, int64_t num_nodes, const int32_t* face_nodes,
                         int64_t num_faces, int device, void* stream, msw_mesh_dual** out);
int msw_mesh_dual_destroy(msw_mesh_dual* dual);
/* The handle's device arrays; they live as long as the handle. */
int msw_mesh_dual_arrays(const msw_mesh_dual* dual, const double** centroid, const double** area,
                         const int32_t** adjacent, const int64_t** edge_index, const double** edge_length,
                         int64_t* num_edges, const int32_t** boundary, int64_t* num_boundary);
int msw_mesh_dual_get_stats(const msw_mesh_dual* dual, msw_mesh_dual_stats* stats);
/* The launch of both dual-graph kernels over num_faces faces: one-wave workgroups, faces_per_wg =
 * 64 consecutive faces per round, at most 4096 workgroups, grid * 64 * iters >= num_faces.
 * num_faces = 0: grid and iters are 0.  MSW_ERR_INVALID: a NULL output, num_faces negative. */
int msw_mesh_dual_launch(int64_t num_faces, int32_t* grid, int32_t* faces_per_wg, int32_t* iters);

/* Locality order: a row order for msw_plan_create_ordered from per-row coordinates, rows sorted
 * along a Hilbert curve inside each segment (a (graph, scale) range).
 *
 * Keys.  With the segment's box (x0, y0, side): sc = 65536.0 / side, fx = (x - x0) * sc,
 *     ix = fx < 0 ? 0 : fx >= 65536 ? 65535 : (int)floor(fx),          fy, iy likewise,
 * each a separate IEEE float64 operation (nothing contracts), and the key is the 32-bit index of
 * cell (ix, iy) on the order-16 Hilbert curve:
 *     d = 0;  for (s = 32768; s > 0; s >>= 1) {
 *         rx = (ix & s) != 0;  ry = (iy & s) != 0;  d += s * s * ((3 * rx) ^ ry);
 *         if (!ry) { if (rx) { ix = 65535 - ix; iy = 65535 - iy; }  swap(ix, iy); } }
 * A row with a non-finite coordinate gets key 0xFFFFFFFF (it sorts last, with the curve's last cell).
 * Order.  Inside segment j, order[seg_ptr[j] + k] is the row of [seg_ptr[j], seg_ptr[j + 1]) with
 * the k-th smallest key, ties to the lower row: a stable sort, so no output bit depends on an order
 * of execution (LSD radix sort of (key, row) pairs, 8-bit digits, LDS counters, no global atomics;
 * the segment index is sorted last as further digits).
 *
 * msw_locality_order: xy device float64 [n][2], seg_ptr HOST int64 [num_segs + 1] tiling [0, n)
 * (empty segments allowed), boxes HOST float64 [num_segs][3] = (x0, y0, side), order device int32
 * [n].  Host-synchronous: allocates its scratch (12 bytes per row and the digit table), runs on
 * `stream`, waits for it and frees.  stats may be NULL.  n = 0: no-op.
 * msw_hilbert_keys: the key kernel alone with one box, keys device uint32 [n]; stream-ordered, no
 * allocation.  msw_locality_sort: the sort alone on given keys (device uint32 [n]); otherwise as
 * msw_locality_order.
 * MSW_ERR_INVALID (before any HIP call): NULLs, negative n, num_segs < 1, a seg_ptr that does not
 * tile [0, n), a box that is not finite, a side that is not finite and positive or so small that
 * 65536.0 / side is not finite, xy not 8-byte or keys / order not 4-byte aligned.  MSW_ERR_UNSUPPORTED: n > 2^26 (from the size alone). */
typedef struct {
  int64_t n, num_segs;
  int64_t scratch_bytes;      /* device memory allocated and freed by the call                      */
  int32_t passes;             /* radix passes: 4 over the key + those over the segment index        */
  int32_t grid;               /* workgroups of every launch of the sort                             */
  double  keys_us, sort_us;   /* device time of the key kernel and of all sort passes (events)      */
} msw_locality_stats;

int msw_locality_order(const double* xy, int64_t n, const int64_t* seg_ptr, int32_t num_segs,
                       const double* boxes, int32_t* order, int device, void* stream,
                       msw_locality_stats* stats);
int msw_hilbert_keys(const double* xy, int64_t n, double x0, double y0, double side, uint32_t* keys,
                     void* stream);
int msw_locality_sort(const uint32_t* keys, int64_t n, const int64_t* seg_ptr, int32_t num_segs,
                      int32_t* order, int device, void* stream, msw_locality_stats* stats);
/* The launch of the key kernel and of every pass of the sort over n rows (from the code the
 * launchers themselves use): 256-thread workgroups, items_per_wg = 256 consecutive rows per round,
 * at most 1024 workgroups, each taking `iters` consecutive rounds (the sort: one contiguous run),
 * grid * 256 * iters >= n.  n = 0: grid and iters are 0.
 * MSW_ERR_INVALID: a NULL output, n negative.  Host only. */
int msw_locality_launch(int64_t n, int32_t* grid, int32_t* items_per_wg, int32_t* iters);

/* ---- Training: autograd through one SWEGNN processor ------------------------
 * Replaces the autograd of SWEGNN.forward (models/gnn.py:387-445) the reference trains through
 * in training_step (training/train.py:125-145).  Stateless: every buffer is device memory the
 * caller owns (mswegnn/autograd.py allocates them as torch tensors).  Parameters are the
 * layer's own tensors: edge_mlp Linear weights [width[l+1]][width[l]] / biases, single-slope
 * PReLU parameters, filter_matrix[k].weight [F][F]. */
#define MSW_MAX_HOPS 8
typedef struct {
  int64_t num_nodes, num_edges;
  int32_t F;             /* dynamic_node_features = static = edge_output_size */
  int32_t edge_features; /* width of edge_attr (0 for intra_scale_gnn) */
  int32_t K;             /* hops, 1..MSW_MAX_HOPS */
  int32_t n_layers;      /* edge MLP depth, 1..MSW_MAX_MLP_LAYERS */
  int32_t width[MSW_MAX_MLP_LAYERS + 1]; /* width[0] = 4F + edge_features, width[n_layers] = F */
  int32_t act[MSW_MAX_MLP_LAYERS];       /* enum msw_activation after each layer */
  int32_t normalize, with_filter_matrix, with_gradient, upwind_mode;
  /* graph, device int32: row / col = edge_index[0] / [1]; CSR by destination (col) and by
   * source (row), edges of a node in reference (edge_index) order */
  const int32_t *row, *col;
  const int32_t *in_ptr, *in_edge;   /* [N + 1], [E] */
  const int32_t *out_ptr, *out_edge; /* [N + 1], [E] */
  const float* weight[MSW_MAX_MLP_LAYERS];
  const float* bias[MSW_MAX_MLP_LAYERS];  /* NULL = bias=False */
  const float* slope[MSW_MAX_MLP_LAYERS]; /* device scalar (PReLU) or NULL */
  const float* filter[MSW_MAX_HOPS + 1];  /* with_filter_matrix: K + 1 matrices */
} msw_swegnn_train_desc;

/* Gradient outputs (device; written, not accumulated).  d_x_d is required; any other NULL
 * pointer skips that gradient. */
typedef struct {
  float *d_x_s, *d_x_d, *d_edge_attr;
  float* d_weight[MSW_MAX_MLP_LAYERS];
  float* d_bias[MSW_MAX_MLP_LAYERS];
  float* d_slope[MSW_MAX_MLP_LAYERS];
  float* d_filter[MSW_MAX_HOPS + 1];
} msw_swegnn_grads;

/* Floats of the forward's saved state (kept until the backward) and of the backward's scratch. */
int msw_swegnn_train_workspace(const msw_swegnn_train_desc* desc, int64_t* saved_floats,
                               int64_t* scratch_floats);
/* out [N][F] = SWEGNN(x_s, x_d, edge_attr); `saved` receives the MLP inputs / pre-activations,
 * s_ij, ||h||, out_k, the aggregated messages and the activity flags of every hop. */
int msw_swegnn_train_forward(const msw_swegnn_train_desc* desc, const float* x_s, const float* x_d,
                             const float* edge_attr, float* saved, float* out, void* stream);
/* Gradients of all inputs and parameters given grad_out [N][F] and the forward's `saved`. */
int msw_swegnn_train_backward(const msw_swegnn_train_desc* desc, const float* x_s, const float* x_d,
                              const float* edge_attr, const float* saved, const float* grad_out,
                              const msw_swegnn_grads* grads, float* scratch, void* stream);

/* ---- Training: autograd through one make_mlp stack --------------------------
 * Replaces the autograd of a make_mlp Sequential (models/models.py:121-146: Linear + activation
 * after every layer, no dropout / layer norm) -- the model's edge / node encoders and node
 * decoder (models/gnn.py:204-215, 239-240) -- in training_step (training/train.py:125-145). */
typedef struct {
  int64_t rows;
  int32_t n_layers;                      /* 1..MSW_MAX_MLP_LAYERS */
  int32_t width[MSW_MAX_MLP_LAYERS + 1]; /* width[0] = input features, width[n_layers] = output */
  int32_t act[MSW_MAX_MLP_LAYERS];       /* enum msw_activation after each layer */
  const float* weight[MSW_MAX_MLP_LAYERS]; /* [width[l+1]][width[l]] */
  const float* bias[MSW_MAX_MLP_LAYERS];   /* NULL = bias=False */
  const float* slope[MSW_MAX_MLP_LAYERS];  /* device scalar (PReLU) or NULL */
} msw_mlp_train_desc;

/* Gradient outputs (device; written, not accumulated); NULL skips that gradient. */
typedef struct {
  float* d_x;
  float* d_weight[MSW_MAX_MLP_LAYERS];
  float* d_bias[MSW_MAX_MLP_LAYERS];
  float* d_slope[MSW_MAX_MLP_LAYERS];
} msw_mlp_grads;

int msw_mlp_train_workspace(const msw_mlp_train_desc* desc, int64_t* saved_floats, int64_t* scratch_floats);
/* out [rows][width[n_layers]] = MLP(x [rows][width[0]]); `saved` receives every layer's
 * pre-activation and the hidden layers' outputs. */
int msw_mlp_train_forward(const msw_mlp_train_desc* desc, const float* x, float* saved, float* out, void* stream);
/* Gradients of the input and the parameters given grad_out and the forward's `saved`. */
int msw_mlp_train_backward(const msw_mlp_train_desc* desc, const float* x, const float* saved,
                           const float* grad_out, const msw_mlp_grads* grads, float* scratch, void* stream);

/* ---- Training: autograd of the mean pooling ----------------------------------
 * Replaces MSGNN._pooling (models/gnn.py:242-257, learnable=False, reduce='mean') and its
 * autograd: pooling edge e maps fine[e] -> coarse[e] (intra_mesh_edge_index rows (coarse,
 * fine), gnn.py:310); cptr / cedge = CSR of the pooling edges by coarse node, fptr / fedge by
 * fine node ([N + 1], [E], edges in pooling-edge order).  out[c] = sum of x[fine] over c's
 * edges / max(#edges, 1), rows without children 0; deterministic (no atomics). */
int msw_pool_mean_forward(int64_t num_nodes, int32_t F, const int32_t* fine, const int32_t* cptr,
                          const int32_t* cedge, const float* x, float* out, void* stream);
int msw_pool_mean_backward(int64_t num_nodes, int32_t F, const int32_t* coarse, const int32_t* cptr,
                           const int32_t* fptr, const int32_t* fedge, const float* grad_out, float* grad_x,
                           void* stream);

/* ---- Training: the loss of training_step and its gradient ---------------------
 * Replaces loss_function (training/loss.py:76-169) and its autograd, which training_step calls
 * after each of its R curriculum rollout steps (training/train.py:125-145): the masked multiscale
 * RMSE / MAE over the finest scale of every graph, the velocity scaler, and the mass-conservation
 * term conservation * |conservation_loss| with get_inflow_volume (utils/dataset.py:577-591).
 * Stateless; every buffer is device memory the caller owns.  No atomics, no host synchronisation,
 * no allocation: results are the same bit for bit from call to call.
 *
 * The rows of the ranges, taken in ascending order, form one list of `total` rows.  Forward,
 * launch 1 (msw_train_loss_launch: `grid` workgroups of 256 threads, `iters` rounds): thread t of
 * workgroup b takes list entries (b + k * grid) * 256 + t for k = 0, 1, ... and adds, in fp64 from
 * +0.0 and in that order, per row i with d_h = (double)pred[i][0] - (double)real[i][0] and d_v
 * likewise from column 1:
 *     sel = !only_where_water || d_h != 0 || d_v != 0            (mask_on_water, loss.py:25-35)
 *     n += sel;  S_h += sel ? d_h * d_h : 0;  S_v += sel ? d_v * d_v : 0       (MAE: |d_h|, |d_v|)
 *     V += (double)area[i] * ((double)pred[i][0] - (double)input_h[i * stride])    (conservation != 0)
 * The 64 lanes of a wave are combined by a butterfly (xor 32, 16, ... 1), the four waves in wave
 * order, and the workgroup writes {n, S_h, S_v, V} to scratch[4 b ..].  Launch 2, one workgroup,
 * all in fp64 and in this order:
 *     n, S_h, S_v, V   = the workgroups' partials added in index order from +0.0
 *     corr   = sum over k = 0 .. n_bc - 1 in order of (double)area[r] * ((double)pred[r][0] -
 *              (double)input_h[r * stride]), r = node_bc[k]; entries outside [0, num_rows) are skipped
 *     inflow = (sum over k in order of (double)bc[k] * (double)edge_bc_length[k]) * seconds_per_step
 *     L_c    = sqrt(S_c / n)  (RMSE)   or   S_c / n  (MAE)                        c = h, v
 *     data   = (L_h + vs * L_v) / (1 + vs)                                  vs = velocity_scaler
 *     cons   = ((V - inflow) - corr) / 1e6 / num_graphs
 *     loss   = conservation != 0 ? data + conservation * |cons| : data
 *     coef_h = (1 / (1 + vs)) / (n * L_h),  coef_v = (vs / (1 + vs)) / (n * L_v)         (RMSE)
 *     coef_h = (1 / (1 + vs)) / n,          coef_v = (vs / (1 + vs)) / n                 (MAE)
 *     cc     = conservation * sgn(cons) / (1e6 * num_graphs)      sgn(x) = 1, -1 or x (0, NaN)
 * With conservation == 0: V = corr = inflow = cons = cc = 0.  *loss_out = (float)loss and
 *     record[12] = {n, S_h, S_v, V, corr, inflow, cons, loss, coef_h, coef_v, cc, data}.
 * Backward, g = (double)*grad_out, per row i of [0, num_rows):
 *     selected row of a range:  grad_pred[i][c] = (float)((g * coef_c) * d_c)               (RMSE)
 *                               grad_pred[i][c] = (float)((g * coef_c) * sgn(d_c))          (MAE)
 *     every other row: +0.0 in both columns (rows between the ranges included)
 *     conservation != 0, with m_i = (float)((g * cc) * (double)area[i]):
 *       range rows:   grad_pred[i][0] += m_i (an fp32 addition);   grad_input_h[i] = -m_i
 *       other rows:   grad_input_h[i] = +0.0
 *       then, one thread, for k = 0 .. n_bc - 1 in order, r = node_bc[k] in [0, num_rows):
 *                     grad_pred[r][0] -= m_r;                      grad_input_h[r] += m_r
 * (grad_input_h, [num_rows] floats with stride 1, is optional and written only when
 * conservation != 0.)  The IEEE results of these formulas are the semantics: n = 0 gives a NaN
 * loss and zero gradients, an RMSE column with S_c = 0 and n > 0 gives NaN gradients (0 * inf) on
 * the selected rows, a NaN or inf in a range row selects the row and gives a NaN loss. */
#define MSW_MAX_LOSS_RANGES 64
#define MSW_TRAIN_LOSS_RECORD 12 /* doubles in `record` */
enum msw_loss_type { MSW_LOSS_RMSE = 0, MSW_LOSS_MAE = 1 };
typedef struct {
  int64_t num_rows;                        /* N: rows of pred / real / area / input_h / the gradients */
  int32_t num_ranges;                      /* 1..MSW_MAX_LOSS_RANGES */
  int32_t type_loss;                       /* enum msw_loss_type */
  int64_t ranges[MSW_MAX_LOSS_RANGES][2];  /* host values: [start, end) of the finest scale of every
                                              graph (node_ptr[g][0], node_ptr[g][1]), or {0, N};
                                              ascending and disjoint, empty ranges allowed */
  int32_t only_where_water;
  int32_t num_graphs;                      /* divides cons (a Batch's num_graphs; 1 for one Data) */
  double velocity_scaler;
  double conservation;                     /* 0: no mass term, the pointers below are not read */
  double seconds_per_step;                 /* 60 * temporal_res (minutes) */
  const float* area;                       /* device [N] cell areas (data.area) */
  const float* input_h;                    /* device: water depth entering the step, row i at
                                              input_h[i * input_h_stride] (data.x[:, -2]) */
  int64_t input_h_stride;                  /* in elements */
  const int64_t* node_bc;                  /* device [n_bc] ghost-cell rows (data.node_BC) */
  const float* bc;                         /* device [n_bc] unit discharge of the step */
  const float* edge_bc_length;             /* device [n_bc] */
  int32_t n_bc;
} msw_train_loss_desc;

/* Doubles of the forward's scratch (4 per workgroup of launch 1, at least 4). */
int msw_train_loss_workspace(const msw_train_loss_desc* desc, int64_t* scratch_doubles);
/* pred, real: device [N][2] fp32.  loss_out: device float.  record_out: device double[12]. */
int msw_train_loss_forward(const msw_train_loss_desc* desc, const float* pred, const float* real,
                           double* scratch, float* loss_out, double* record_out, void* stream);
/* record: the forward's, on the same desc, pred and real.  grad_out: device float (the gradient of
 * the loss).  grad_pred: device [N][2], written.  grad_input_h: device [N] or NULL. */
int msw_train_loss_backward(const msw_train_loss_desc* desc, const float* pred, const float* real,
                            const double* record, const float* grad_out, float* grad_pred,
                            float* grad_input_h, void* stream);
/* Launch 1 of the forward for `total_rows` rows in all ranges together (from the code the launcher
 * itself uses): workgroups (at most 512), rows a workgroup takes per round (256) and the rounds of
 * its grid-stride loop, so that grid * rows_per_wg * iters >= total_rows; 0 rows: grid = iters = 0
 * (the forward then skips launch 1).  MSW_ERR_INVALID: negative total_rows, a NULL output.  Host only.
 * MSW_ERR_INVALID of the three functions above, before any HIP call: NULL desc or required pointer,
 * num_ranges outside 1..64, a range with end < start, a negative start, an end past num_rows (or
 * num_rows past the kernels' int32 row indices), ranges not ascending and disjoint, an unknown
 * type_loss, num_graphs < 1, and with conservation != 0: NULL area or input_h, negative n_bc, or
 * n_bc > 0 with a NULL node_bc, bc or edge_bc_length. */
int msw_train_loss_launch(int64_t total_rows, int32_t* grid, int32_t* rows_per_wg, int32_t* iters);

/* Diagnostics: route per-phase timestamps of wave 0 of workgroup 0 of every launch to the
 * device buffer `buf` (uint64[20]: {shader clock, 100 MHz clock} for phase marks 0..9).
 * Only builds compiled with -DMSW_TRACE record anything; NULL disables. */
int msw_set_trace(msw_plan* plan, uint64_t* buf);

/* sizeof() of a descriptor struct ("msw_linear", "msw_mlp", "msw_swegnn",
 * "msw_model_desc", "msw_graph_desc", "msw_plan_stats", ..., "msw_train_loss_desc"); -1 if
 * unknown.  Pure host code:
 * lets FFI bindings verify their struct layouts without a GPU. */
int64_t msw_struct_size(const char* name);
const char* msw_last_error(void);
int msw_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MSWEGNN_H */
