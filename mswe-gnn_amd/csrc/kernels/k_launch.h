// gfx950 kernels: kernel preparation, residency queries and per-F instantiation (the
// launchers are in k_pick.h).
// Part of kernels_impl.h (included inside namespace msw, in this order); see its header
// comment for the register layout and conventions.
#pragma once

// ---------------------------------------------------------------------------- preparation
// Allow the dynamic weight regions past the 64 KB default (gfx950: 160 KB per CU).
template <int NT>
hipError_t prepare_kernels() {
  // the largest static slab (edge-MLP rows) of a workgroup of `wv` waves
  auto mx = [](int wv) { return 160 * 1024 - wv * kRowsPerWave * (16 * 2 * NT + 16 * NT + 4) * (int)sizeof(float); };
  constexpr int WL = waves_of<NT, true>();
  const std::pair<const void*, int> fns[] = {
      {(const void*)k_encode<NT, 1, false>, kWaves}, {(const void*)k_encode<NT, -1, false>, kWaves},
      {(const void*)k_encode<NT, 1, true>, kWaves}, {(const void*)k_encode<NT, -1, true>, kWaves},
      {(const void*)k_encode<NT, 1, false, true>, kWaves}, {(const void*)k_encode<NT, -1, false, true>, kWaves},
      {(const void*)k_edge_hop<NT, 1, false, 0>, kWaves}, {(const void*)k_edge_hop<NT, -1, false, 0>, kWaves},
      {(const void*)k_edge_hop<NT, 1, false, 1>, kWaves}, {(const void*)k_edge_hop<NT, -1, false, 1>, kWaves},
      {(const void*)k_edge_hop<NT, 1, true, 0>, edge_waves<NT, true, 0>()},
      {(const void*)k_edge_hop<NT, -1, true, 0>, edge_waves<NT, true, 0>()},
      {(const void*)k_edge_hop<NT, 1, true, 1>, edge_waves<NT, true, 1>()},
      {(const void*)k_edge_hop<NT, -1, true, 1>, edge_waves<NT, true, 1>()},
      {(const void*)k_hop<NT, 1, true, false>, kWaves}, {(const void*)k_hop<NT, -1, true, false>, kWaves},
      {(const void*)k_hop<NT, 1, true, true>, hop_waves<NT, true>()},
      {(const void*)k_hop<NT, -1, true, true>, hop_waves<NT, true>()},
      {(const void*)k_pool<NT, false>, kWaves}, {(const void*)k_pool<NT, true>, WL},
      {(const void*)k_pool_edge<NT>, kWaves}, {(const void*)k_pool_edge<NT, NT >= 2 ? NT : 1>, kWaves},
      {(const void*)k_epi<NT, 1, false>, kWaves}, {(const void*)k_epi<NT, -1, false>, kWaves},
      {(const void*)k_epi<NT, 1, true>, WL}, {(const void*)k_epi<NT, -1, true>, WL}};
  for (const auto& f : fns) {
    hipError_t e = hipFuncSetAttribute(f.first, hipFuncAttributeMaxDynamicSharedMemorySize, mx(f.second));
    if (e != hipSuccess) return e;
  }
  for (const void* f : {(const void*)k_edge_mlp<NT, 1>, (const void*)k_edge_mlp<NT, -1>}) {  // no slab
    hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
  }
  if constexpr (NT >= 2) {  // wide pooling (one tile per workgroup)
    hipError_t e = hipFuncSetAttribute((const void*)k_pool_edge<NT, 2 * NT, 2 * NT>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, mx(2 * NT));
    if (e != hipSuccess) return e;
  }
  if constexpr (NT >= 2) {  // cooperative encoders
    for (const void* f : {(const void*)k_encode_coop<NT, 1, false, NT>, (const void*)k_encode_coop<NT, -1, false, NT>,
                          (const void*)k_encode_coop<NT, 1, true, NT>, (const void*)k_encode_coop<NT, -1, true, NT>}) {
      hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, mx(enc_coop_waves<NT>()));
      if (e != hipSuccess) return e;
    }
  }
  if constexpr (NT == 4) {  // F = 64 cooperative encoder on two waves per row tile
    for (const void* f : {(const void*)k_encode_coop<NT, 1, false, 2>, (const void*)k_encode_coop<NT, -1, false, 2>,
                          (const void*)k_encode_coop<NT, 1, true, 2>, (const void*)k_encode_coop<NT, -1, true, 2>}) {
      hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, mx(enc_coop_waves<NT>()));
      if (e != hipSuccess) return e;
    }
  }
  if constexpr (NT >= 2) {  // cooperative last hops (F = 32, 64)
    for (int prelu = 0; prelu < 2; ++prelu) {
      hipError_t e = hipFuncSetAttribute(hop_coop_kernel<NT>(prelu), hipFuncAttributeMaxDynamicSharedMemorySize, mx(kWaves));
      if (e != hipSuccess) return e;
    }
  }
  if constexpr (NT == 4) {  // F = 64 cooperative edge hops: a slab + exchange buffers per tile
    for (int pw = 2; pw <= 4; pw += 2) {
      for (int prelu = 0; prelu < 2; ++prelu)
        for (int last = 0; last < 2; ++last)
          for (int pool = 0; pool < 2; ++pool) {
            hipError_t e = hipFuncSetAttribute(edge_coop_kernel<NT>(prelu, last, pw, pool),
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               edge_coop_lds_cap<NT>(pw, pool));
            if (e != hipSuccess) return e;
          }
    }
  }
  if constexpr (NT == 2) {  // cooperative edge hops: 160 KB minus slabs and exchange buffers
    for (int prelu = 0; prelu < 2; ++prelu)
      for (int last = 0; last < 2; ++last)
        for (int pool = 0; pool < 3; ++pool) {
          hipError_t e = hipFuncSetAttribute(edge_coop_kernel<NT>(prelu, last, 0, pool),
                                             hipFuncAttributeMaxDynamicSharedMemorySize,
                                             edge_coop_lds_cap<NT>(2, pool));
          if (e != hipSuccess) return e;
        }
  }
  return hipSuccess;
}

template <int NT>
hipError_t launch_rowmlp(const RowMlpArgs& a, hipStream_t st) {
  if (a.R <= 0) return hipSuccess;
  if (a.mode == 1)
    hipLaunchKernelGGL((k_rowmlp<NT, 1>), dim3(cdiv(a.R, kRowsPerBlock)), dim3(kBlock), 0, st, a);
  else
    hipLaunchKernelGGL((k_rowmlp<NT, 0>), dim3(cdiv(a.R, kRowsPerBlock)), dim3(kBlock), 0, st, a);
  return hipGetLastError();
}

// Workgroups of one launch resident on the whole chip (grid cap of the grid-stride kernels).
template <int NT, bool LOOP>
static const void* kernel_of(int kind, int prelu, int last) {
  switch (kind) {
    case 0: return prelu ? (const void*)k_encode<NT, 1, false> : (const void*)k_encode<NT, -1, false>;
    case 1: return edge_hop_kernel<NT>(prelu, LOOP, last);
    case 2:
      return !last ? (const void*)k_hop<NT, 1, false, LOOP>
                   : (prelu ? (const void*)k_hop<NT, 1, true, LOOP> : (const void*)k_hop<NT, -1, true, LOOP>);
    case 3: return (const void*)k_pool<NT, LOOP>;
    case 5: return (const void*)k_pool_edge<NT>;
    case 13:
      if constexpr (NT >= 2) return (const void*)k_pool_edge<NT, 2 * NT, 2 * NT>;
      return nullptr;
    case 6: return prelu ? (const void*)k_epi<NT, 1, LOOP> : (const void*)k_epi<NT, -1, LOOP>;
    case 7: return edge_coop_kernel<NT>(prelu, last);
    case 16: return edge_coop_kernel<NT>(prelu, last, 0, 1);
    case 12: return edge_coop_kernel<NT>(prelu, last, 2);
    case 9: return hop_coop_kernel<NT>(prelu);
    case 10: return prelu ? (const void*)k_edge_mlp<NT, 1> : (const void*)k_edge_mlp<NT, -1>;
    case 14: return (const void*)k_hop_rows<NT>;
    default: return nullptr;
  }
}
template <int NT>
int resident_blocks(int kind, int prelu, int last, size_t dyn_bytes, int loop) {
  const void* f = loop ? kernel_of<NT, true>(kind, prelu, last) : kernel_of<NT, false>(kind, prelu, last);
  int per_cu = 0, dev = 0, cus = 0;
  if (!f) return 0;
  const size_t dyn = (kind == 1 || kind == 7 || kind == 10 || kind == 12) ? eh_lds_bytes((int)(dyn_bytes / 4))
                                                                          : lds_bytes<NT>((int)(dyn_bytes / 4));
  if (dyn > 160 * 1024) return 0;
  const int block = kind == 1 ? 64 * (loop ? (last ? edge_waves<NT, true, 1>() : edge_waves<NT, true, 0>()) : kWaves)
                    : kind == 10 ? 64 * kMlpWaves
                    : kind == 13 ? 64 * 2 * NT
                    : kind == 14 ? 64 * kRowHopWaves
                    : kind == 2 ? 64 * (loop ? hop_waves<NT, true>() : kWaves)
                    : 64 * (loop && (kind == 3 || kind == 6) ? waves_of<NT, true>() : kWaves);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, f, block, dyn) != hipSuccess)
    return 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return per_cu > 0 ? per_cu * cus : 0;
}

#define MSW_INSTANTIATE(NT)                                                       \
  template hipError_t prepare_kernels<NT>();                                      \
  template int resident_blocks<NT>(int, int, int, size_t, int);                   \
  template Pick pick_encode<NT>(const EncodeArgs&);                               \
  template Pick pick_edge_hop<NT>(const EdgeHopArgs&);                            \
  template Pick pick_edge_mlp<NT>(const EdgeHopArgs&);                            \
  template Pick pick_hop<NT>(const HopArgs&);                                     \
  template Pick pick_pool<NT>(const PoolArgs&);                                   \
  template Pick pick_epi<NT>(const EpiArgs&);                                     \
  template Pick pick_decode<NT>(const DecodeArgs&);                               \
  template hipError_t launch_encode<NT>(const EncodeArgs&, hipStream_t);          \
  template hipError_t launch_edge_hop<NT>(const EdgeHopArgs&, hipStream_t);       \
  template hipError_t launch_edge_mlp<NT>(const EdgeHopArgs&, hipStream_t);       \
  template hipError_t launch_hop<NT>(const HopArgs&, hipStream_t);                \
  template hipError_t launch_pool<NT>(const PoolArgs&, hipStream_t);              \
  template hipError_t launch_epi<NT>(const EpiArgs&, hipStream_t);                \
  template hipError_t launch_rowmlp<NT>(const RowMlpArgs&, hipStream_t);           \
  template hipError_t launch_decode<NT>(const DecodeArgs&, hipStream_t);
