// gfx950 kernels: the choice of kernel variant, grid, workgroup and dynamic LDS of every
// launch kind (pick_*, engine.h Pick) and the launchers, which launch exactly what was picked.
// msw_plan_schedule (plan.hip) prints the same picks: one copy of the rules.
// Part of kernels_impl.h (included inside namespace msw, in this order); see its header
// comment for the register layout and conventions.
#pragma once

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

template <int NT>
constexpr size_t lds_bytes(int floats) {
  return kStaged<NT> ? (size_t)((floats + kChunk - 1) / kChunk * kChunk) * sizeof(float) : 0;
}

// XCD packing of a one-round grid of g workgroups (b: the launch's argument copy): the
// fewest XCDs (1, 2, 4 <= c.xcd_max) that hold one workgroup per CU, else all eight
template <class A>
static inline dim3 xcd_grid(A& b, long g) {
  b.c.xcd = 0;
  for (int k = 1; k <= b.c.xcd_max && k < kXcds; k *= 2)
    if (g <= (long)kCusPerXcd * k) {
      b.c.xcd = k;
      return dim3((unsigned)(cdiv(g, k) * kXcds));
    }
  return dim3((unsigned)g);
}

// one tile per wave while that grid is resident at once; grid-stride loop beyond that
template <class A>
static inline bool tile_loop(const A& a) {
  return a.fit_blocks > 0 && a.max_blocks > 0 && cdiv(a.ntiles, kWaves) > a.fit_blocks;
}
template <class A>
static inline int tile_grid(const A& a) {
  return tile_loop(a) ? a.max_blocks : cdiv(a.ntiles, kWaves);
}

template <int NT>
static const void* edge_hop_kernel(int prelu, bool loop, int last) {
  if (loop) {
    if (last) return prelu ? (const void*)k_edge_hop<NT, 1, true, 1> : (const void*)k_edge_hop<NT, -1, true, 1>;
    return prelu ? (const void*)k_edge_hop<NT, 1, true, 0> : (const void*)k_edge_hop<NT, -1, true, 0>;
  }
  if (last) return prelu ? (const void*)k_edge_hop<NT, 1, false, 1> : (const void*)k_edge_hop<NT, -1, false, 1>;
  return prelu ? (const void*)k_edge_hop<NT, 1, false, 0> : (const void*)k_edge_hop<NT, -1, false, 0>;
}

// ---------------------------------------------------------------------------- picks
static inline Pick pick_make(const void* fn, const char* name, int grid, int waves, int pack, size_t lds,
                             long units, int per_wg) {
  Pick p{};
  p.fn = fn;
  snprintf(p.name, sizeof(p.name), "%s", name);
  p.grid = grid; p.waves = waves; p.pack = pack; p.lds = lds; p.units = units; p.per_wg = per_wg;
  return p;
}
static inline Pick pick_invalid() {
  Pick p{};
  p.err = (int)hipErrorInvalidValue;
  snprintf(p.name, sizeof(p.name), "invalid");
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
  const size_t sh = lds_bytes<NT>(a.lds_floats);
  const bool dec = a.dec.on != 0, prelu = a.c.prelu != 0;
  if constexpr (NT >= 2) {
    if (a.coop == NT) {  // P = NT waves per row tile (F = 32: 2, F = 64: 4)
      constexpr int P = NT, WV = enc_coop_waves<NT>();
      const void* f = dec ? (prelu ? (const void*)k_encode_coop<NT, 1, true, P> : (const void*)k_encode_coop<NT, -1, true, P>)
                          : (prelu ? (const void*)k_encode_coop<NT, 1, false, P> : (const void*)k_encode_coop<NT, -1, false, P>);
      return pick_make(f, pick_name(nm, "encode coop", {{dec, "dec"}}), a.Npad / ((WV / P) * kRowsPerWave), WV, 0,
                       sh, a.Npad / kRowsPerWave, WV / P);
    }
  }
  const int n = a.Npad / kRowsPerBlock;  // 64-row chunks
  const int grid = a.max_blocks > 0 && n > a.max_blocks ? a.max_blocks : n;
  const bool stream = a.stream && !dec;
  const void* f = stream ? (prelu ? (const void*)k_encode<NT, 1, false, true> : (const void*)k_encode<NT, -1, false, true>)
                  : dec  ? (prelu ? (const void*)k_encode<NT, 1, true> : (const void*)k_encode<NT, -1, true>)
                         : (prelu ? (const void*)k_encode<NT, 1, false> : (const void*)k_encode<NT, -1, false>);
  return pick_make(f, pick_name(nm, "encode", {{grid < n, "loop"}, {stream, "stream"}, {dec, "dec"}}), grid, kWaves,
                   0, sh, n, 1);
}

template <int NT>
Pick pick_edge_mlp(const EdgeHopArgs& a) {
  if (a.nchunks <= 0) return Pick{};
  const int n = cdiv(a.nchunks, kMlpWaves);
  const int grid = a.max_blocks > 0 && n > a.max_blocks ? a.max_blocks : n;
  const void* f = a.c.prelu ? (const void*)k_edge_mlp<NT, 1> : (const void*)k_edge_mlp<NT, -1>;
  return pick_make(f, "edge_mlp", grid, kMlpWaves, 0, eh_lds_bytes(a.reg.len), a.nchunks, kMlpWaves);
}

template <int NT>
Pick pick_edge_hop(const EdgeHopArgs& a) {
  if (a.ntiles <= 0) return Pick{};
  char nm[40];
  const bool last = a.last != 0;
  if (a.coop == 2 || a.coop == 4) {  // waves per tile; 4: F = 64, one tile per workgroup
    const int fuse = a.pool.slots ? 1 : a.pool.parent ? 2 : 0;
    const void* f = edge_coop_kernel<NT>(a.c.prelu, a.last, a.coop, fuse);
    if (!f || (fuse && NT == 2 && a.coop != 2)) return pick_invalid();
    return pick_make(f, pick_name(nm, a.coop == 4 ? "edge_coop4" : "edge_coop2",
                                  {{last, "last"}, {fuse == 1, "pool"}, {fuse == 2, "unpool"}, {a.wdirect != 0, "direct"}}),
                     a.coop == 4 ? a.ntiles : cdiv((long)a.ntiles * a.coop, kWaves), kWaves, 1,
                     a.wdirect ? 0 : eh_lds_bytes(a.reg_nf), a.ntiles, kWaves / a.coop);
  }
  if (a.pool.slots || a.pool.parent) return pick_invalid();  // fused into k_edge_coop only
  const bool loop = tile_loop(a);
  const int wv = loop ? (a.last ? edge_waves<NT, true, 1>() : edge_waves<NT, true, 0>()) : kWaves;
  return pick_make(edge_hop_kernel<NT>(a.c.prelu, loop, a.last),
                   pick_name(nm, "edge_hop", {{loop, "loop"}, {last, "last"}, {!last, "first"}}), tile_grid(a), wv,
                   !loop, eh_lds_bytes(loop ? a.reg.len : a.reg_nf), a.ntiles, wv);
}

template <int NT>
Pick pick_hop(const HopArgs& a) {
  if (a.ntiles <= 0) return Pick{};
  char nm[40];
  if (a.coop > 1 && a.last) {  // waves per tile = NT (2 for F = 32, 4 for F = 64)
    const void* f = hop_coop_kernel<NT>(a.c.prelu);
    if (!f) return pick_invalid();
    return pick_make(f, "hop coop", cdiv((long)a.ntiles * a.coop, kWaves), kWaves, 1, lds_bytes<NT>(a.reg.len),
                     a.ntiles, kWaves / a.coop);
  }
  if (a.rows && !a.last) {  // row-layout middle hop (large meshes)
    const int nt = cdiv(a.nrows, kRowsPerWave);
    const int grid = a.max_blocks > 0 ? std::min(a.max_blocks, cdiv(nt, kRowHopWaves)) : cdiv(nt, kRowHopWaves);
    return pick_make((const void*)k_hop_rows<NT>, "hop rows", grid, kRowHopWaves, 0, 0, nt, kRowHopWaves);
  }
  if constexpr (NT >= 2) {
    if (a.split && !a.last)  // feature-split middle hop: two waves per tile
      return pick_make((const void*)k_hop_split<NT>, "hop split", cdiv((long)a.ntiles * 2, kWaves), kWaves, 1, 0,
                       a.ntiles, kWaves / 2);
  }
  const bool loop = tile_loop(a), last = a.last != 0;
  const int wv = loop ? hop_waves<NT, true>() : kWaves;
  const void* f;
  if (!last)
    f = loop ? (const void*)k_hop<NT, 1, false, true> : (const void*)k_hop<NT, 1, false, false>;
  else if (a.c.prelu)
    f = loop ? (const void*)k_hop<NT, 1, true, true> : (const void*)k_hop<NT, 1, true, false>;
  else
    f = loop ? (const void*)k_hop<NT, -1, true, true> : (const void*)k_hop<NT, -1, true, false>;
  return pick_make(f, pick_name(nm, "hop", {{loop, "loop"}, {last, "last"}, {!last, "mid"}}), tile_grid(a), wv, !loop,
                   last ? lds_bytes<NT>(a.reg.len) : 0, a.ntiles, wv);
}

template <int NT>
Pick pick_pool(const PoolArgs& a) {
  if (a.ntiles <= 0) return Pick{};
  const size_t sh = lds_bytes<NT>(a.reg.len);
  if (!a.rows) {
    if constexpr (NT >= 2) {
      if (a.coop == 2 * NT)  // 2 NT waves per tile (one tile per workgroup)
        return pick_make((const void*)k_pool_edge<NT, 2 * NT, 2 * NT>, "pool edge wide", a.ntiles, 2 * NT, 1, sh,
                         a.ntiles, 1);
      if (a.coop == NT)  // waves per tile: 2 (F = 32), 4 (F = 64)
        return pick_make((const void*)k_pool_edge<NT, NT>, "pool edge coop", cdiv((long)a.ntiles * NT, kWaves), kWaves,
                         1, sh, a.ntiles, kWaves / NT);
    }
    return pick_make((const void*)k_pool_edge<NT>, "pool edge", cdiv(a.ntiles, kWaves), kWaves, 1, sh, a.ntiles,
                     kWaves);
  }
  const bool loop = tile_loop(a);
  const int wv = loop ? waves_of<NT, true>() : kWaves;
  return pick_make(loop ? (const void*)k_pool<NT, true> : (const void*)k_pool<NT, false>,
                   loop ? "pool rows loop" : "pool rows", tile_grid(a), wv, !loop, sh, a.ntiles, wv);
}

template <int NT>
Pick pick_epi(const EpiArgs& a) {
  if (a.ntiles <= 0) return Pick{};
  const bool loop = tile_loop(a);
  const int wv = loop ? waves_of<NT, true>() : kWaves;
  const void* f = a.c.prelu ? (loop ? (const void*)k_epi<NT, 1, true> : (const void*)k_epi<NT, 1, false>)
                            : (loop ? (const void*)k_epi<NT, -1, true> : (const void*)k_epi<NT, -1, false>);
  return pick_make(f, loop ? "epi loop" : "epi", tile_grid(a), wv, !loop, lds_bytes<NT>(a.reg.len), a.ntiles, wv);
}

template <int NT>
Pick pick_decode(const DecodeArgs& a) {
  if (a.Npad <= 0) return Pick{};
  const int n = cdiv(a.Npad, kRowsPerBlock);
  return pick_make(a.c.prelu ? (const void*)k_decode_fwd<NT, 1> : (const void*)k_decode_fwd<NT, -1>, "decode", n,
                   kWaves, 0, 0, n, 1);
}

// ---------------------------------------------------------------------------- launchers
template <class A>
static inline hipError_t launch_pick(const Pick& p, const A& a, hipStream_t st) {
  if (p.err) return (hipError_t)p.err;
  if (!p.fn) return hipSuccess;  // nothing to do
  A b = a;
  const dim3 grid = p.pack ? xcd_grid(b, p.grid) : dim3((unsigned)p.grid);
  if (!p.pack) b.c.xcd = 0;
  void* args[] = {&b};
  return hipLaunchKernel(p.fn, grid, dim3(64 * p.waves), args, p.lds, st);
}
template <int NT>
hipError_t launch_encode(const EncodeArgs& a, hipStream_t st) { return launch_pick(pick_encode<NT>(a), a, st); }
template <int NT>
hipError_t launch_edge_mlp(const EdgeHopArgs& a, hipStream_t st) { return launch_pick(pick_edge_mlp<NT>(a), a, st); }
template <int NT>
hipError_t launch_edge_hop(const EdgeHopArgs& a, hipStream_t st) { return launch_pick(pick_edge_hop<NT>(a), a, st); }
template <int NT>
hipError_t launch_hop(const HopArgs& a, hipStream_t st) { return launch_pick(pick_hop<NT>(a), a, st); }
template <int NT>
hipError_t launch_pool(const PoolArgs& a, hipStream_t st) { return launch_pick(pick_pool<NT>(a), a, st); }
template <int NT>
hipError_t launch_epi(const EpiArgs& a, hipStream_t st) { return launch_pick(pick_epi<NT>(a), a, st); }
template <int NT>
hipError_t launch_decode(const DecodeArgs& a, hipStream_t st) { return launch_pick(pick_decode<NT>(a), a, st); }
