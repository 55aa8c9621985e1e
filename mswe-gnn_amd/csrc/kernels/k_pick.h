// gfx950 kernels: the one description of every kernel variant (variant_of: kernel, workgroup,
// dynamic-LDS rule and cap of a VariantKey, engine.h) and the choice of variant, grid and
// dynamic LDS of every launch kind (pick_*, engine.h Pick), which launch_pick launches and
// msw_plan_schedule (plan.hip) prints: one copy of the rules.
// Part of kernels_impl.h (included inside namespace msw, in this order); see its header
// comment for the register layout and conventions.
#pragma once

template <int NT>
constexpr size_t lds_bytes(int floats) {
  return kStaged<NT> ? (size_t)((floats + kChunk - 1) / kChunk * kChunk) * sizeof(float) : 0;
}

template <class A>
static inline int tile_grid(const A& a) {
  return tile_loop(a) ? a.max_blocks : cdiv(a.ntiles, kWaves);
}

// ---------------------------------------------------------------------------- variants
// dynamic LDS of a launch with a weight region of n floats: none, the region where the width
// stages its weights (lds_bytes), or the edge hop's MLP region at every width (eh_lds_bytes)
enum LdsRule { LDS_NONE, LDS_STAGED, LDS_EDGE_HOP };
struct Variant {
  const void* fn;  // the kernel, null where none exists
  int waves;       // per workgroup
  int lds;         // LdsRule
  int lds_cap;     // the dynamic LDS prepare_kernels allows the kernel past the 64 KB default, 0 = none
};
template <int NT>
static inline size_t variant_lds(const Variant& v, int floats) {
  return v.lds == LDS_EDGE_HOP ? eh_lds_bytes(floats) : v.lds == LDS_STAGED ? lds_bytes<NT>(floats) : 0;
}

// a run-time flag as a template argument: f(std::true_type) or f(std::false_type)
template <class F>
static inline Variant by_flag(int flag, F&& f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}

// Adding a variant: one entry here (and a flag in VariantKey if no existing one tells it
// apart); its pick and the plan's residency query then name it by key.
template <int NT>
static Variant variant_of(const VariantKey& k) {
  // gfx950 has 160 KB of LDS per CU: what the largest static slab (edge-MLP rows) of a
  // workgroup of `wv` waves leaves
  auto mx = [](int wv) { return 160 * 1024 - wv * kRowsPerWave * (16 * 2 * NT + 16 * NT + 4) * (int)sizeof(float); };
  auto act = [&](const void* prelu, const void* other) { return k.prelu ? prelu : other; };
  const Variant none{};
  switch (k.family) {
    case K_ENCODE: {
      if (k.dec && k.stream) return none;  // the decoding encoder does not stream
      const void* f =
          k.stream ? act((const void*)k_encode<NT, 1, false, true>, (const void*)k_encode<NT, -1, false, true>)
          : k.dec  ? act((const void*)k_encode<NT, 1, true>, (const void*)k_encode<NT, -1, true>)
                   : act((const void*)k_encode<NT, 1, false>, (const void*)k_encode<NT, -1, false>);
      return {f, kWaves, LDS_STAGED, mx(kWaves)};
    }
    case K_ENCODE_COOP:  // NT waves per row tile (F = 32: 2, F = 64: 4)
      if constexpr (NT >= 2) {
        const void* f =
            k.dec ? act((const void*)k_encode_coop<NT, 1, true, NT>, (const void*)k_encode_coop<NT, -1, true, NT>)
                  : act((const void*)k_encode_coop<NT, 1, false, NT>, (const void*)k_encode_coop<NT, -1, false, NT>);
        return {f, enc_coop_waves<NT>(), LDS_STAGED, mx(enc_coop_waves<NT>())};
      }
      return none;
    case K_EDGE_HOP:
      return by_flag(k.loop, [&](auto lp) {
        return by_flag(k.last, [&](auto ls) {
          constexpr bool L = decltype(lp)::value;
          constexpr int LS = decltype(ls)::value;
          return Variant{act((const void*)k_edge_hop<NT, 1, L, LS>, (const void*)k_edge_hop<NT, -1, L, LS>),
                         edge_waves<NT, L, LS>(), LDS_EDGE_HOP, mx(edge_waves<NT, L, LS>())};
        });
      });
    case K_EDGE_COOP: {  // waves per tile: 2 (F = 32), 4 or 2 (F = 64)
      if (k.waves != 2 && !(NT == 4 && k.waves == 4)) return none;
      const void* f = edge_coop_kernel<NT>(k.prelu, k.last, k.waves, k.fuse);
      return {f, kWaves, LDS_EDGE_HOP, f ? edge_coop_lds_cap<NT>(k.waves, k.fuse) : 0};
    }
    case K_EDGE_MLP:  // no slab
      return {act((const void*)k_edge_mlp<NT, 1>, (const void*)k_edge_mlp<NT, -1>), kMlpWaves, LDS_EDGE_HOP, 160 * 1024};
    case K_HOP:  // a middle hop has no activation and stages nothing
      return by_flag(k.loop, [&](auto lp) {
        constexpr bool L = decltype(lp)::value;
        const void* f = !k.last ? (const void*)k_hop<NT, 1, false, L>
                                : act((const void*)k_hop<NT, 1, true, L>, (const void*)k_hop<NT, -1, true, L>);
        return Variant{f, hop_waves<NT, L>(), LDS_STAGED, k.last ? mx(hop_waves<NT, L>()) : 0};
      });
    case K_HOP_ROWS: return {(const void*)k_hop_rows<NT>, kRowHopWaves, LDS_NONE, 0};
    case K_HOP_SPLIT:
      if constexpr (NT >= 2) return {(const void*)k_hop_split<NT>, kWaves, LDS_NONE, 0};
      return none;
    case K_HOP_COOP: return {hop_coop_kernel<NT>(k.prelu), kWaves, LDS_STAGED, mx(kWaves)};
    case K_HOP_DENSE:  // F <= 32; a middle hop has no activation
      if constexpr (NT <= 2) {
        const void* f = !k.last ? (const void*)k_hop_dense<NT, 1, false>
                                : act((const void*)k_hop_dense<NT, 1, true>, (const void*)k_hop_dense<NT, -1, true>);
        return {f, 1, LDS_NONE, 0};  // one wave (one row tile) per workgroup
      }
      return none;
    case K_POOL_ROWS:
      return by_flag(k.loop, [&](auto lp) {
        constexpr bool L = decltype(lp)::value;
        return Variant{(const void*)k_pool<NT, L>, waves_of<NT, L>(), LDS_STAGED, mx(waves_of<NT, L>())};
      });
    case K_POOL_EDGE:  // waves per tile: one, NT, or 2 NT (one tile per workgroup)
      if (k.waves <= 1) return {(const void*)k_pool_edge<NT>, kWaves, LDS_STAGED, mx(kWaves)};
      if constexpr (NT >= 2) {
        if (k.waves == NT) return {(const void*)k_pool_edge<NT, NT>, kWaves, LDS_STAGED, mx(kWaves)};
        if (k.waves == 2 * NT) return {(const void*)k_pool_edge<NT, 2 * NT, 2 * NT>, 2 * NT, LDS_STAGED, mx(2 * NT)};
      }
      return none;
    case K_EPI:
      return by_flag(k.loop, [&](auto lp) {
        constexpr bool L = decltype(lp)::value;
        return Variant{act((const void*)k_epi<NT, 1, L>, (const void*)k_epi<NT, -1, L>), waves_of<NT, L>(), LDS_STAGED,
                       mx(waves_of<NT, L>())};
      });
    case K_DECODE:
      return {act((const void*)k_decode_fwd<NT, 1>, (const void*)k_decode_fwd<NT, -1>), kWaves, LDS_NONE, 0};
  }
  return none;
}

// Every key: all flag combinations of all families.  variant_of gives no kernel for a
// combination that has none and the same kernel for keys that differ in a flag the family
// does not take, so a walk over the variants skips null and repeated kernels.
template <class F>
static inline void for_each_key(F&& f) {
  for (int family = 0; family < K_FAMILIES; ++family)
    for (int bits = 0; bits < 32; ++bits)
      for (int waves : {1, 2, 4, 8})
        for (int fuse = 0; fuse < 3; ++fuse)
          f(VariantKey{family, bits & 1, bits >> 1 & 1, bits >> 2 & 1, waves, fuse, bits >> 3 & 1, bits >> 4 & 1});
}

// ---------------------------------------------------------------------------- picks
static inline Pick pick_invalid() {
  Pick p{};
  p.err = (int)hipErrorInvalidValue;
  snprintf(p.name, sizeof(p.name), "invalid");
  return p;
}
// variant v on `grid` workgroups, with a weight region of `floats`
template <int NT>
static inline Pick pick_make(const Variant& v, const char* name, int grid, int pack, int floats, long units,
                             int per_wg) {
  if (!v.fn) return pick_invalid();
  Pick p{};
  p.fn = v.fn;
  snprintf(p.name, sizeof(p.name), "%s", name);
  p.grid = grid; p.waves = v.waves; p.pack = pack; p.lds = variant_lds<NT>(v, floats); p.units = units; p.per_wg = per_wg;
  return p;
}
// "family" + the flags set, in order
static inline const char* pick_name(char (&buf)[40], const char* family,
                                    std::initializer_list<std::pair<bool, const char*>> flags) {
  int n = snprintf(buf, sizeof(buf), "%s", family);
  for (const auto& f : flags)
    if (f.first && n < (int)sizeof(buf)) n += snprintf(buf + n, sizeof(buf) - n, " %s", f.second);
  return buf;
}

template <int NT>
Pick pick_encode(const EncodeArgs& a) {
  if (a.Npad <= 0) return Pick{};
  char nm[40];
  const bool dec = a.dec.on != 0;
  if constexpr (NT >= 2) {
    if (a.coop == NT) {
      const Variant v = variant_of<NT>({K_ENCODE_COOP, a.c.prelu, 0, 0, NT, 0, dec});
      const int g = v.waves / NT;  // row tiles per workgroup
      return pick_make<NT>(v, pick_name(nm, "encode coop", {{dec, "dec"}}), a.Npad / (g * kRowsPerWave), 0,
                           a.lds_floats, a.Npad / kRowsPerWave, g);
    }
  }
  const int n = a.Npad / kRowsPerBlock;  // 64-row chunks
  const int grid = a.max_blocks > 0 && n > a.max_blocks ? a.max_blocks : n;
  const bool stream = a.stream && !dec;
  return pick_make<NT>(variant_of<NT>({K_ENCODE, a.c.prelu, 0, 0, 0, 0, dec, stream}),
                       pick_name(nm, "encode", {{grid < n, "loop"}, {stream, "stream"}, {dec, "dec"}}), grid, 0,
                       a.lds_floats, n, 1);
}

template <int NT>
Pick pick_edge_mlp(const EdgeHopArgs& a) {
  if (a.nchunks <= 0) return Pick{};
  const int n = cdiv(a.nchunks, kMlpWaves);
  const int grid = a.max_blocks > 0 && n > a.max_blocks ? a.max_blocks : n;
  return pick_make<NT>(variant_of<NT>({K_EDGE_MLP, a.c.prelu}), "edge_mlp", grid, 0, a.reg.len, a.nchunks, kMlpWaves);
}

template <int NT>
Pick pick_edge_hop(const EdgeHopArgs& a) {
  if (a.ntiles <= 0) return Pick{};
  char nm[40];
  const bool last = a.last != 0;
  if (a.coop == 2 || a.coop == 4) {  // waves per tile; 4: F = 64, one tile per workgroup
    const int fuse = a.pool.slots ? 1 : a.pool.parent ? 2 : 0;
    return pick_make<NT>(variant_of<NT>({K_EDGE_COOP, a.c.prelu, a.last, 0, a.coop, fuse}),
                         pick_name(nm, a.coop == 4 ? "edge_coop4" : "edge_coop2",
                                   {{last, "last"}, {fuse == 1, "pool"}, {fuse == 2, "unpool"}, {a.wdirect != 0, "direct"}}),
                         a.coop == 4 ? a.ntiles : cdiv((long)a.ntiles * a.coop, kWaves), 1, a.wdirect ? 0 : a.reg_nf,
                         a.ntiles, kWaves / a.coop);
  }
  if (a.pool.slots || a.pool.parent) return pick_invalid();  // fused into k_edge_coop only
  const bool loop = tile_loop(a);
  const Variant v = variant_of<NT>({K_EDGE_HOP, a.c.prelu, a.last, loop});
  return pick_make<NT>(v, pick_name(nm, "edge_hop", {{loop, "loop"}, {last, "last"}, {!last, "first"}}), tile_grid(a),
                       !loop, loop ? a.reg.len : a.reg_nf, a.ntiles, v.waves);
}

template <int NT>
Pick pick_hop(const HopArgs& a) {
  if (a.ntiles <= 0) return Pick{};
  char nm[40];
  if (a.coop > 1 && a.last)  // waves per tile = NT (2 for F = 32, 4 for F = 64)
    return pick_make<NT>(variant_of<NT>({K_HOP_COOP, a.c.prelu, 1, 0, a.coop}), "hop coop",
                         cdiv((long)a.ntiles * a.coop, kWaves), 1, a.reg.len, a.ntiles, kWaves / a.coop);
  if (a.rows && !a.last) {  // row-layout middle hop (large meshes)
    const int nt = cdiv(a.nrows, kRowsPerWave);
    const int grid = a.max_blocks > 0 ? std::min(a.max_blocks, cdiv(nt, kRowHopWaves)) : cdiv(nt, kRowHopWaves);
    return pick_make<NT>(variant_of<NT>({K_HOP_ROWS}), "hop rows", grid, 0, 0, nt, kRowHopWaves);
  }
  if constexpr (NT >= 2) {
    if (a.split && !a.last)  // feature-split middle hop: two waves per tile
      return pick_make<NT>(variant_of<NT>({K_HOP_SPLIT}), "hop split", cdiv((long)a.ntiles * 2, kWaves), 1, 0,
                           a.ntiles, kWaves / 2);
  }
  const bool loop = tile_loop(a), last = a.last != 0;
  const Variant v = variant_of<NT>({K_HOP, a.c.prelu, last, loop});
  return pick_make<NT>(v, pick_name(nm, "hop", {{loop, "loop"}, {last, "last"}, {!last, "mid"}}), tile_grid(a), !loop,
                       last ? a.reg.len : 0, a.ntiles, v.waves);
}

// dense row-tile hop (latency-bound scales, Launch::dense): one row tile per one-wave workgroup, one round
template <int NT>
Pick pick_hop_dense(const HopArgs& a) {
  if (a.nrows <= 0) return Pick{};
  char nm[40];
  const int nt = cdiv(a.nrows, kRowsPerWave);
  return pick_make<NT>(variant_of<NT>({K_HOP_DENSE, a.c.prelu, a.last != 0}),
                       pick_name(nm, "hop dense", {{a.last != 0, "last"}}), nt, 1, 0, nt, 1);
}

template <int NT>
Pick pick_pool(const PoolArgs& a) {
  if (a.ntiles <= 0) return Pick{};
  if (!a.rows) {
    if constexpr (NT >= 2) {
      if (a.coop == 2 * NT)  // 2 NT waves per tile (one tile per workgroup)
        return pick_make<NT>(variant_of<NT>({K_POOL_EDGE, 0, 0, 0, 2 * NT}), "pool edge wide", a.ntiles, 1, a.reg.len,
                             a.ntiles, 1);
      if (a.coop == NT)  // waves per tile: 2 (F = 32), 4 (F = 64)
        return pick_make<NT>(variant_of<NT>({K_POOL_EDGE, 0, 0, 0, NT}), "pool edge coop",
                             cdiv((long)a.ntiles * NT, kWaves), 1, a.reg.len, a.ntiles, kWaves / NT);
    }
    return pick_make<NT>(variant_of<NT>({K_POOL_EDGE}), "pool edge", cdiv(a.ntiles, kWaves), 1, a.reg.len, a.ntiles,
                         kWaves);
  }
  const bool loop = tile_loop(a);
  const Variant v = variant_of<NT>({K_POOL_ROWS, 0, 0, loop});
  return pick_make<NT>(v, loop ? "pool rows loop" : "pool rows", tile_grid(a), !loop, a.reg.len, a.ntiles, v.waves);
}

template <int NT>
Pick pick_epi(const EpiArgs& a) {
  if (a.ntiles <= 0) return Pick{};
  const bool loop = tile_loop(a);
  const Variant v = variant_of<NT>({K_EPI, a.c.prelu, 1, loop});
  return pick_make<NT>(v, loop ? "epi loop" : "epi", tile_grid(a), !loop, a.reg.len, a.ntiles, v.waves);
}

template <int NT>
Pick pick_decode(const DecodeArgs& a) {
  if (a.Npad <= 0) return Pick{};
  const int n = cdiv(a.Npad, kRowsPerBlock);
  return pick_make<NT>(variant_of<NT>({K_DECODE, a.c.prelu}), "decode", n, 0, 0, n, 1);
}
