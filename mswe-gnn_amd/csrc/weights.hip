// Where an operand lies: the model's weights packed as MFMA operands into the plan's blob
// (pack_model), and the operands of each launch copied into a contiguous region the kernels
// stage in LDS (relocate).
//
// Reference semantics followed (sdat2/mSWE-GNN): SWEGNN.forward models/gnn.py:387-445.
#include <map>

#include "plan.h"

using namespace msw;

namespace {

// Pack W (original [out_dim][in_dim]) as the A operand of v_mfma_f32_16x16x4_f32,
// [tout][tin][lane][4]: lane l, k-step r of input tile ti for output tile to holds
// W[16 to + (l & 15)][16 ti + 4 (l >> 4) + r] (register layout: kernels_impl.h).
// in_map(k) / out_map(o): original column / row of packed input feature k / output
// feature o, or -1 for a zero pad.
template <class InMap, class OutMap>
int pack_operand(Blob& B, const float* W, int in_dim, int tout, int tin, InMap in_map,
                 OutMap out_map) {
  const int off = B.alloc((size_t)tout * tin * 64 * 4);
  float* A = B.h.data() + off;
  for (int to = 0; to < tout; ++to)
    for (int ti = 0; ti < tin; ++ti)
      for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 4; ++r) {
          const int o = out_map(16 * to + (lane & 15));
          const int k = in_map(16 * ti + 4 * (lane >> 4) + r);
          float v = 0.f;
          if (o >= 0 && k >= 0) v = W[(size_t)o * in_dim + k];
          A[(((size_t)to * tin + ti) * 64 + lane) * 4 + r] = v;
        }
  return off;
}

// Width embedding (hid_features 33..63 run zero-padded to Fp = 64): a dimension made of nb
// blocks of F model features is stored as nb blocks of Fp, each block's features in its first
// F columns.  Packed index k -> model index, or -1 for a pad column.  F == Fp: the identity
// on [0, nb F).
struct Embed {
  int F, Fp;
  int operator()(int k, int nb) const {
    const int b = k / Fp, c = k % Fp;
    return (b < nb && c < F) ? b * F + c : -1;
  }
};

// Every layer gets a bias vector (zeros for bias=False): the kernels add it unconditionally.
// out_map as pack_operand's.
template <class OutMap>
int pack_bias(Blob& B, const float* b, int tout, OutMap out_map) {
  const int off = B.alloc((size_t)16 * tout);
  if (b)
    for (int q = 0; q < 16 * tout; ++q) {
      const int o = out_map(q);
      if (o >= 0) B.h[off + q] = b[o];
    }
  return off;
}

// Pack a make_mlp stack (natural feature order in and out).  Hidden widths are one feature
// block (F, embedded into Fp); in_feat / out_feat: so are the stack's input / output
// (otherwise raw columns: the encoders' inputs, the decoder's two outputs).
int pack_mlp(Blob& B, const msw_mlp& m, MlpDev& d, Embed em, bool in_feat, bool out_feat) {
  if (m.n_layers < 1 || m.n_layers > kMaxLayers)
    return fail(MSW_ERR_UNSUPPORTED, "MLP depth must be 1.." + std::to_string(kMaxLayers));
  d.n = m.n_layers;
  for (int i = 0; i < m.n_layers; ++i) {
    const msw_linear& L = m.layer[i];
    if (!L.weight || L.in_features <= 0 || L.out_features <= 0)
      return fail(MSW_ERR_INVALID, "MLP layer without weight");
    if (L.act < 0 || L.act > 7) return fail(MSW_ERR_INVALID, "unknown activation code");
    const int din = L.in_features, dout = L.out_features;
    const bool fin = i > 0 || in_feat, fout = i + 1 < m.n_layers || out_feat;
    const int tin = cdiv(fin ? em.Fp : din, 16), tout = cdiv(fout ? em.Fp : dout, 16);
    auto inm = [&](int k) { return fin ? em(k, 1) : (k < din ? k : -1); };
    auto outm = [&](int o) { return fout ? em(o, 1) : (o < dout ? o : -1); };
    d.l[i].tin = tin;
    d.l[i].tout = tout;
    d.l[i].a_off = pack_operand(B, L.weight, din, tout, tin, inm, outm);
    d.l[i].b_off = pack_bias(B, L.bias, tout, outm);
    d.l[i].act = L.act;
    d.l[i].slope = L.act_param;
  }
  return MSW_OK;
}

// every activation of the MLP is a PReLU with slope <= 1, slope != 0: the compile-time PReLU
// kernels (kernels/k_base.h act_static<1>: max(x, slope x)); otherwise the run-time switch
int all_prelu(const msw_mlp& m) {
  for (int i = 0; i < m.n_layers; ++i) {
    const float s = m.layer[i].act_param;
    if (m.layer[i].act != MSW_ACT_PRELU || !(s <= 1.f && s != 0.f)) return 0;
  }
  return 1;
}

// SWEGNN layer -> packed Proc (gnn.py:352-445).
int build_proc(msw_plan* P, const msw_swegnn& g, int scale, bool intra, Proc& pr) {
  // F: the model's width (indexes its tensors); Fp = 16 NT: the engine's row width
  const int F = P->F, Fp = P->Fp, NT = P->NT;
  const Embed em{F, Fp};
  pr.scale = scale;
  pr.K = g.K;
  pr.normalize = g.normalize;
  pr.with_filter = g.with_filter_matrix;
  pr.with_gradient = g.with_gradient;
  pr.upwind = g.upwind_mode;
  if (g.K < 1) return fail(MSW_ERR_UNSUPPORTED, "SWEGNN with K < 1");
  const msw_mlp& m = g.edge_mlp;
  if (m.n_layers < 1 || m.n_layers > kMaxLayers) return fail(MSW_ERR_UNSUPPORTED, "edge MLP depth must be 1..4");
  const msw_linear& L1 = m.layer[0];
  const int ef = g.edge_features;
  if (L1.in_features != 4 * F + ef) return fail(MSW_ERR_INVALID, "edge MLP input width != 4F + edge_features");
  const int H1 = L1.out_features;
  if (H1 != (m.n_layers > 1 ? 2 * F : F)) return fail(MSW_ERR_UNSUPPORTED, "edge MLP hidden width must be 2F");
  for (int i = 1; i < m.n_layers; ++i)
    if (m.layer[i].in_features != 2 * F || m.layer[i].out_features != (i == m.n_layers - 1 ? F : 2 * F))
      return fail(MSW_ERR_UNSUPPORTED, "edge MLP layer widths must be 2F -> ... -> F");
  const int hb = H1 / F;  // feature blocks of the hidden width (2, or 1 for one-layer MLPs)
  pr.h1t = cdiv(hb * Fp, 16);
  P->h1t_max = std::max(P->h1t_max, pr.h1t);
  const int din = L1.in_features;
  const float* W1 = L1.weight;
  auto outm = [&](int o) { return em(o, hb); };
  // cat(x_s[row], x_s[col], x_d[row], x_d[col], e_ij) (gnn.py:414-420): U takes the row
  // (source) blocks, V the col (receiving) blocks; packed input = [x_s (Fp) | x_d (Fp)], W1's
  // columns are the model's (blocks of F)
  auto blk = [&](int k, int b_xs, int b_xd) {  // packed column -> W1 column (x_s / x_d block)
    const int q = em(k, 2);
    return q < 0 ? -1 : (q < F ? b_xs * F + q : b_xd * F + (q - F));
  };
  auto in_u = [&](int k) { return blk(k, 0, 2); };
  auto in_v = [&](int k) { return blk(k, 1, 3); };
  pr.a_u = pack_operand(P->blob, W1, din, pr.h1t, 2 * NT, in_u, outm);
  pr.a_v = pack_operand(P->blob, W1, din, pr.h1t, 2 * NT, in_v, outm);
  if (intra)  // fine rows enter with x_d = 0: V from the x_s block alone
    pr.a_vu = pack_operand(P->blob, W1, din, pr.h1t, NT, [&](int k) { return k < F ? F + k : -1; }, outm);
  pr.act1 = L1.act;
  pr.slope1 = L1.act_param;
  pr.b1_off = pack_bias(P->blob, L1.bias, pr.h1t, outm);
  auto idF = [&](int q) { return q < F ? q : -1; };
  if (g.with_filter_matrix) {
    if (intra) return fail(MSW_ERR_UNSUPPORTED, "intra-scale SWEGNN with filter matrix");
    if (!g.filter) return fail(MSW_ERR_INVALID, "with_filter_matrix but no filter weights");
    pr.a_o = pack_operand(P->blob, g.filter[0], F, NT, NT, idF, idF);
    for (int k = 1; k <= g.K; ++k) pr.filt.push_back(pack_operand(P->blob, g.filter[k], F, NT, NT, idF, idF));
  } else if (!intra) {
    // out = x_d.clone() (gnn.py:404): identity operand, exact (1*x + 0*y sums)
    std::vector<float> I((size_t)F * F, 0.f);
    for (int i = 0; i < F; ++i) I[(size_t)i * F + i] = 1.f;
    pr.a_o = pack_operand(P->blob, I.data(), F, NT, NT, idF, idF);
  }
  pr.rest.n = m.n_layers - 1;
  for (int i = 1; i < m.n_layers; ++i) {
    const msw_linear& L = m.layer[i];
    const int di = L.in_features, ob = L.out_features / F;  // 2F in; 2F or F out
    LayerDev& d = pr.rest.l[i - 1];
    d.tin = cdiv(2 * Fp, 16);
    d.tout = cdiv(ob * Fp, 16);
    auto om = [&](int o) { return em(o, ob); };
    d.a_off = pack_operand(P->blob, L.weight, di, d.tout, d.tin, [&](int k) { return em(k, 2); }, om);
    d.b_off = pack_bias(P->blob, L.bias, d.tout, om);
    d.act = L.act;
    d.slope = L.act_param;
  }
  pr.prelu = all_prelu(m);
  return MSW_OK;
}

}  // namespace

int msw::pack_model(msw_plan* P, const msw_model_desc* m, int ef_raw) {
  const int F = P->F;
  const Embed em{F, P->Fp};
  int rc;
  auto chain_ok = [&](const msw_mlp& mm, int last_out) {
    for (int i = 0; i < mm.n_layers; ++i) {
      const int want = (i == mm.n_layers - 1) ? last_out : F;
      if (mm.layer[i].out_features != want) return false;
      if (i > 0 && mm.layer[i].in_features != F) return false;
    }
    return true;
  };
  if (!chain_ok(m->static_encoder, F) || !chain_ok(m->dynamic_encoder, F) || !chain_ok(m->decoder, 2) ||
      (m->edge_mlp && !chain_ok(m->edge_encoder, F)) || m->decoder.layer[0].in_features != F)
    return fail(MSW_ERR_UNSUPPORTED, "encoder/decoder hidden widths must equal hid_features");
  if ((rc = pack_mlp(P->blob, m->static_encoder, P->stat, em, false, true))) return rc;
  if ((rc = pack_mlp(P->blob, m->dynamic_encoder, P->dynm, em, false, true))) return rc;
  if ((rc = pack_mlp(P->blob, m->decoder, P->dec, em, true, false))) return rc;
  if (m->static_encoder.layer[0].in_features != P->nstat_raw + P->with_wl)
    return fail(MSW_ERR_INVALID, "static encoder input width");
  if (m->dynamic_encoder.layer[0].in_features != P->dyn) return fail(MSW_ERR_INVALID, "dynamic encoder input width");
  if (m->residual_weights) {
    P->resw_off = P->blob.alloc(2 * P->p);
    for (int i = 0; i < 2 * P->p; ++i) P->blob.h[P->resw_off + i] = m->residual_weights[i];
  }
  if (m->edge_mlp) {
    if ((rc = pack_mlp(P->blob, m->edge_encoder, P->edge_enc, em, false, true))) return rc;
    if (m->edge_encoder.layer[0].in_features != ef_raw) return fail(MSW_ERR_INVALID, "edge encoder input width");
    if (ef_raw > 16) return fail(MSW_ERR_UNSUPPORTED, "more than 16 raw edge features");
  } else if (ef_raw > F) {
    return fail(MSW_ERR_UNSUPPORTED, "more raw edge features than F");
  }
  const int ef = m->edge_mlp ? F : ef_raw;
  P->procs.resize(m->num_processors);
  for (int j = 0; j < m->num_processors; ++j) {
    const int S = P->S;
    const int scale = P->model_type == 1 ? 0 : (j <= S - 1 ? j : 2 * S - 2 - j);
    if (m->processors[j].edge_features != ef) return fail(MSW_ERR_INVALID, "processor edge_features mismatch");
    if ((rc = build_proc(P, m->processors[j], scale, false, P->procs[j]))) return rc;
    P->procs[j].par = j & 1;
  }
  P->unpools.resize(P->model_type == 0 ? m->num_unpool : 0);
  for (size_t i = 0; i < P->unpools.size(); ++i) {
    if (m->unpool[i].edge_features != 0) return fail(MSW_ERR_INVALID, "intra-scale layer with edge features");
    if (m->unpool[i].K != 1) return fail(MSW_ERR_UNSUPPORTED, "intra-scale layer with K != 1");
    if (m->unpool[i].with_gradient) return fail(MSW_ERR_UNSUPPORTED, "intra-scale layer with gradient");
    if ((rc = build_proc(P, m->unpool[i], P->S - 2 - (int)i, true, P->unpools[i]))) return rc;
  }
  P->prelu = all_prelu(m->static_encoder) & all_prelu(m->dynamic_encoder) & all_prelu(m->decoder);
  return MSW_OK;
}

MlpDev msw::pack_edge_term(const msw_plan* P, Blob& tb, const msw_linear& L1, int feat_dim) {
  const int F = P->F, NT = P->NT;
  const Embed em{F, P->Fp};
  const int hb = L1.out_features / F;  // hidden feature blocks, as build_proc
  auto outm = [&](int o) { return em(o, hb); };
  MlpDev md{};  // one NT -> 2NT layer (zero padded)
  md.n = 1;
  md.l[0].tin = NT;
  md.l[0].tout = 2 * NT;
  md.l[0].a_off = pack_operand(tb, L1.weight, L1.in_features, 2 * NT, NT,
                               [&](int k) { return k < feat_dim ? 4 * F + k : -1; }, outm);
  md.l[0].b_off = pack_bias(tb, L1.bias, 2 * NT, outm);
  md.l[0].act = 0;
  return md;
}

// ---------------------------------------------------------------------------- weight regions
namespace {

// Copies the operands one launch reads into a contiguous blob region and rewrites the
// launch's offsets to LDS offsets (kernels stage the region per workgroup).
struct RegionBuilder {
  Blob& B;
  int base, shift;
  std::map<int, int> memo;
  RegionBuilder(Blob& b, int sh) : B(b), shift(sh) { base = B.alloc(0); }
  int put(int off, int len) {
    if (off < 0) return off;
    auto it = memo.find(off);
    if (it != memo.end()) return it->second;
    len = (len + 3) & ~3;
    std::vector<float> tmp(len, 0.f);
    for (int i = 0; i < len && off + i < (int)B.h.size(); ++i) tmp[i] = B.h[off + i];
    const int pos = (int)B.h.size();
    B.h.insert(B.h.end(), tmp.begin(), tmp.end());
    const int r = pos - base + shift;
    memo[off] = r;
    return r;
  }
  int pos() const { return (int)B.h.size() - base; }
  WReg done(int split = -1) const {
    const int len = (int)B.h.size() - base;
    return WReg{base, len, split < 0 ? len : split};
  }
};

struct Relocator {
  int NT, p;
  void layer(RegionBuilder& R, LayerDev& L) {
    L.a_off = R.put(L.a_off, L.tout * L.tin * 256);
    L.b_off = R.put(L.b_off, 16 * L.tout);
  }
  void mlp(RegionBuilder& R, MlpDev& m) {
    for (int i = 0; i < m.n; ++i) layer(R, m.l[i]);
  }
  void np(RegionBuilder& R, NpDesc& d) {
    d.a_u = R.put(d.a_u, d.h1t * 2 * NT * 256);
    d.a_v = R.put(d.a_v, d.h1t * 2 * NT * 256);
    d.a_o = R.put(d.a_o, NT * NT * 256);
  }
  void epi(RegionBuilder& R, Epilogue& e) {
    np(R, e.np);
    e.uu_a = R.put(e.uu_a, e.uu_h1t * 2 * NT * 256);
    if (e.dec.on) {
      mlp(R, e.dec.dec);
      e.dec.resw_off = R.put(e.dec.resw_off, 2 * p);
    }
  }
  // an edge launch's region of its MLP operands only (b1, layers 2..L)
  void mlp_region(Blob& B, EdgeHopArgs& a) {
    RegionBuilder R(B, 0);
    a.b1_off = R.put(a.b1_off, 16 * a.h1t);
    mlp(R, a.rest);
    a.reg = R.done();
    a.reg_nf = a.reg.len;
    a.filt_l = -1;
  }
};

// the LDS a staged region may take: 160 KB minus the F = 32 edge slab
constexpr int kMaxRegionFloats = (160 * 1024) / 4 - kWaves * kRowsPerWave * (3 * 32 + 4);

}  // namespace

// mlp_only (F = 64): only the edge hops' MLP operands get a region -- when it fits beside the
// edge slab, else the launch silently keeps its blob offsets; every other operand stays a
// blob offset.  Staged (F <= 32): every launch's region is checked against kMaxRegionFloats.
int msw::relocate(msw_plan* P, std::vector<Launch>& q, bool mlp_only) {
  Relocator rl{P->NT, P->p};
  for (Launch& L : q) {
    WReg* reg = nullptr;
    int tot = 0;
    if (mlp_only) {
      if (L.kind != L_EDGE_HOP && L.kind != L_EDGE_MLP) continue;
      EdgeHopArgs& a = L.eh;
      int len = 16 * a.h1t;
      for (int i = 0; i < a.rest.n; ++i) len += a.rest.l[i].tout * a.rest.l[i].tin * 256 + 16 * a.rest.l[i].tout;
      const int slab = kWaves * kRowsPerWave * (48 * P->NT + 4) * (int)sizeof(float);
      if ((len + 255) / 256 * 256 * (int)sizeof(float) + slab > 160 * 1024) continue;  // stays in the blob
      rl.mlp_region(P->blob, a);
      continue;
    }
    if (L.kind == L_ENCODE) {
      // one contiguous region per scale (one LDS-DMA copy per workgroup): the static
      // encoder first -- identical relative offsets in every scale's region -- then the
      // dynamic encoder + projection 0 (scale 0) and that scale's unpool V operand
      EncodeArgs& a = L.enc;
      const MlpDev stat0 = a.stat, dec0 = a.dec.dec;
      const int resw0 = a.dec.resw_off;
      a.reg = WReg{0, 0, 0};
      a.lds_floats = 0;
      for (int s = 0; s < a.S; ++s) {
        RegionBuilder Rs(P->blob, 0);
        MlpDev st = stat0;
        rl.mlp(Rs, st);
        a.stat = st;
        if (a.dec.on) {  // the decoder (rollout mode): same offsets in every scale's region
          MlpDev dm = dec0;
          rl.mlp(Rs, dm);
          a.dec.dec = dm;
          a.dec.resw_off = Rs.put(resw0, 2 * P->p);
        }
        if (s == 0) {
          rl.mlp(Rs, a.dynm);
          rl.np(Rs, a.np0);
        }
        a.vu_a[s] = Rs.put(a.vu_a[s], a.vu_h1t * P->NT * 256);
        a.sreg[s] = Rs.done();
        a.lds_floats = std::max(a.lds_floats, a.sreg[s].len);
      }
      tot = (a.lds_floats + 255) / 256 * 256;
    } else if (L.kind == L_EDGE_MLP) {
      rl.mlp_region(P->blob, L.eh);
      reg = &L.eh.reg;
    } else if (L.kind == L_EDGE_HOP) {
      EdgeHopArgs& a = L.eh;
      RegionBuilder R(P->blob, 0);
      a.b1_off = R.put(a.b1_off, 16 * a.h1t);
      rl.mlp(R, a.rest);
      if (a.pool.parent) {  // fused unpooling: its edge MLP, then the projection
        a.pool.b1_off = R.put(a.pool.b1_off, 16 * a.pool.h1t);
        rl.mlp(R, a.pool.rest);
      }
      if (a.pool.slots || a.pool.parent) rl.np(R, a.pool.np);  // fused (un)pooling: before the MLP
      const int split = R.pos();  // operands after this one stream in behind the MLP
      if (a.last) rl.epi(R, a.epi);
      // filt_a stays a blob offset (the one-tile-per-wave variant loads it into registers and
      // stages the region without it); the grid-stride variant reads this trailing copy
      a.reg_nf = R.pos();
      a.filt_l = R.put(a.filt_a, P->NT * P->NT * 256);
      a.reg = R.done(split);
      reg = &a.reg;
    } else if (L.kind == L_EXCHANGE || L.kind == L_DECODE) {
      continue;  // no LDS weight region (the forward decode reads its operands from the blob)
    } else if (L.kind == L_EPI) {
      EpiArgs& a = L.ep;
      RegionBuilder R(P->blob, 0);
      rl.epi(R, a.epi);
      a.reg = R.done();
      reg = &a.reg;
    } else if (L.kind == L_HOP) {
      HopArgs& a = L.hop;
      if (!a.last) continue;  // middle hops load their filter from the blob (k_hop<.., false>)
      RegionBuilder R(P->blob, 0);  // filt_a stays a blob offset (k_hop loads it into registers)
      rl.epi(R, a.epi);
      a.reg = R.done();
      reg = &a.reg;
    } else {
      PoolArgs& a = L.pool;
      RegionBuilder R(P->blob, 0);
      rl.np(R, a.np);
      a.reg = R.done();
      reg = &a.reg;
    }
    if (reg) tot = (reg->len + 255) / 256 * 256;  // LDS-DMA chunks
    if (tot > kMaxRegionFloats)
      return fail(MSW_ERR_UNSUPPORTED, "weights of one launch exceed the LDS budget (" + std::to_string(tot * 4) + " B)");
  }
  return MSW_OK;
}
