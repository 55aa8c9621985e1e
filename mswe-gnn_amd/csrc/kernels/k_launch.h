// gfx950 kernels: kernel preparation, residency queries and per-F instantiation (the
// variants and picks are in k_pick.h, launch_pick in engine.h).
// Part of kernels_impl.h (included inside namespace msw, in this order); see its header
// comment for the register layout and conventions.
#pragma once

// ---------------------------------------------------------------------------- preparation
// Allow the dynamic weight regions past the 64 KB default (gfx950: 160 KB per CU).
template <int NT>
hipError_t prepare_kernels() {
  std::set<const void*> done;
  hipError_t e = hipSuccess;
  for_each_key([&](const VariantKey& k) {
    const Variant v = variant_of<NT>(k);
    if (e == hipSuccess && v.fn && v.lds_cap && done.insert(v.fn).second)
      e = hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, v.lds_cap);
  });
  return e;
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
template <int NT>
int resident_blocks(const VariantKey& k, int floats) {
  const Variant v = variant_of<NT>(k);
  int per_cu = 0, dev = 0, cus = 0;
  if (!v.fn) return 0;
  const size_t dyn = variant_lds<NT>(v, floats);
  if (dyn > 160 * 1024) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, v.fn, 64 * v.waves, dyn) != hipSuccess)
    return 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  return per_cu > 0 ? per_cu * cus : 0;
}

#define MSW_INSTANTIATE(NT)                                                       \
  template hipError_t prepare_kernels<NT>();                                      \
  template int resident_blocks<NT>(const VariantKey&, int);                       \
  template Pick pick_encode<NT>(const EncodeArgs&);                               \
  template Pick pick_edge_hop<NT>(const EdgeHopArgs&);                            \
  template Pick pick_edge_mlp<NT>(const EdgeHopArgs&);                            \
  template Pick pick_hop<NT>(const HopArgs&);                                     \
  template Pick pick_hop_dense<NT>(const HopArgs&);                               \
  template Pick pick_pool<NT>(const PoolArgs&);                                   \
  template Pick pick_epi<NT>(const EpiArgs&);                                     \
  template Pick pick_decode<NT>(const DecodeArgs&);                               \
  template hipError_t launch_rowmlp<NT>(const RowMlpArgs&, hipStream_t);
