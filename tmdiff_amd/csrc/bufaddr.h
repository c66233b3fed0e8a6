// Buffer-descriptor addressing and LDS-DMA: a tensor region (one sample's channel tile, one chunk of input channels) behind a
// descriptor, a lane's address one 32-bit byte offset -- the base and size live in scalar registers, and there is no 64-bit
// address arithmetic per lane.  An offset at or beyond the descriptor's size -- kOutside -- makes a load return zero and a store
// vanish in the hardware's bounds check.  So a ragged tile runs the code of a full one: no store under a divergent branch
// (around which the compiler spills live accumulators: conv3d_wf.hip's epilogue, profiles/r04_wf_experiments.txt), and the zero
// padding of a convolution costs a select of the offset, not a second source pointer.
#pragma once
#include <hip/hip_runtime.h>

namespace tmdiff {
namespace buf {

constexpr unsigned kOutside = 0xFFFFFFF0u;

#if defined(__HIP_DEVICE_COMPILE__)   // the builtins exist in the device pass only
using rsrc = __amdgpu_buffer_rsrc_t;
__device__ __forceinline__ rsrc make(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, bytes, 0x00020000);
}
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
// one dword per lane from base + voff + soff (soff wave-uniform)
__device__ __forceinline__ float load(rsrc r, unsigned voff, unsigned soff) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ float4 load4(rsrc r, unsigned voff) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, 0, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
__device__ __forceinline__ float2 load2(rsrc r, unsigned voff) {
  const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, 0, 0);
  return make_float2(__uint_as_float(v.x), __uint_as_float(v.y));
}
__device__ __forceinline__ void store(rsrc r, unsigned voff, float t) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(t), r, voff, 0, 0);
}
__device__ __forceinline__ void store4(rsrc r, unsigned voff, float4 t) {
  const u32x4 v = {__float_as_uint(t.x), __float_as_uint(t.y), __float_as_uint(t.z), __float_as_uint(t.w)};
  __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, 0, 0);
}
__device__ __forceinline__ void store4(rsrc r, unsigned voff, uint4 t) {
  const u32x4 v = {t.x, t.y, t.z, t.w};
  __builtin_amdgcn_raw_buffer_store_b128(v, r, voff, 0, 0);
}
__device__ __forceinline__ void store2(rsrc r, unsigned voff, float2 t) {
  const u32x2 v = {__float_as_uint(t.x), __float_as_uint(t.y)};
  __builtin_amdgcn_raw_buffer_store_b64(v, r, voff, 0, 0);
}
// LDS-DMA: 16 bytes per lane from base + voff + soff (soff wave-uniform) to dst + 16 * lane (dst wave-uniform)
__device__ __forceinline__ void dma_b128(rsrc r, unsigned voff, unsigned soff, float* dst) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, dst, 16, voff, soff, 0, 0);
}
#else
struct rsrc {};
__device__ __forceinline__ rsrc make(const void*, unsigned) { return {}; }
__device__ __forceinline__ float load(rsrc, unsigned, unsigned) { return 0.f; }
__device__ __forceinline__ float4 load4(rsrc, unsigned) { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float2 load2(rsrc, unsigned) { return make_float2(0.f, 0.f); }
__device__ __forceinline__ void store(rsrc, unsigned, float) {}
__device__ __forceinline__ void store4(rsrc, unsigned, float4) {}
__device__ __forceinline__ void store4(rsrc, unsigned, uint4) {}
__device__ __forceinline__ void store2(rsrc, unsigned, float2) {}
__device__ __forceinline__ void dma_b128(rsrc, unsigned, unsigned, float*) {}
#endif
// base + add where the base is inside (kOutside + anything would wrap around into the descriptor)
__device__ __forceinline__ unsigned at(unsigned base, unsigned add) { return base >= kOutside ? kOutside : base + add; }

// LDS-DMA by pointer (global_load_lds): 4 / 16 bytes per lane from src (per lane) to dst + 4 / 16 * lane (dst wave-uniform)
__device__ __forceinline__ void dma_b32(const float* src, float* dst) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_global_load_lds(src, dst, 4, 0, 0);
#endif
}
__device__ __forceinline__ void dma_b128(const float* src, float* dst) {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
#endif
}

}  // namespace buf
}  // namespace tmdiff
