// Small device helpers shared by the fp32 loss kernels (ge2e_fused_f32.hip, the fused-split body, the team kernels,
// ge2e_tiled.hip): float4 arithmetic, buffer-resource loads / stores, the fast norm bookkeeping, the split-fp16 image write.
#pragma once
#include "ge2e_common.hpp"
#include "ge2e_split_gemm.hpp"

namespace ge2e {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned OOB = 0x7FFFFF00u;  // lane offset that is out of range of every buffer here

__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
    return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w;
}
__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 scale4(const float4& a, float s) {
    return make_float4(a.x * s, a.y * s, a.z * s, a.w * s);
}

// All global traffic of these kernels goes through buffer resources: one SGPR descriptor + a 32-bit lane offset, and a
// lane offset of OOB reads 0 / drops the store with no predication branch.
// AUX = cache-policy bits of buffer instructions on gfx950: 1 = sc0, 2 = nt (streaming), 16 = sc1
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
template <int AUX = 0>
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, AUX));
}
__device__ __forceinline__ float bload1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
// NOTE the offset of a 16-byte store goes entirely into the VGPR (soffset = immediate 0).  With a
// REGISTER soffset LLVM assumes the "VMEM store > 64 bit, then VALU write of its data VGPRs" hazard does
// not exist and lets the very next instruction overwrite the store's data registers; on gfx950 with two
// waves per SIMD that clobbered ~5 % of launches (4 rows x 64 columns at a time, always the younger
// wave of a SIMD).  With an immediate soffset the hazard recognizer inserts the wait state itself.
// Two forms: the whole offset in `voff`, or a lane part + a uniform part that are added into the VGPR here.
template <int AUX = 0>
__device__ __forceinline__ void bstore4(__amdgpu_buffer_rsrc_t r, unsigned voff, const float4& v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, 0, AUX);
}
template <int AUX = 0>
__device__ __forceinline__ void bstore4(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff, const float4& v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff + soff, 0, AUX);
}

// unit_stats with the common case (norm above the cosine eps) on v_rsq_f32 + one Newton step
// instead of sqrt and two IEEE divisions; the clamped case keeps the exact slow path.
__device__ __forceinline__ void unit_stats_fast(float sq, float eps_cos, float& rn, float& kappa) {
    if (sq > eps_cos * eps_cos && sq < 1e30f) {
        float r = __builtin_amdgcn_rsqf(sq);
        r = r * (1.5f - 0.5f * sq * r * r);
        rn = r;
        kappa = 1.0f;
    } else {
        unit_stats(sq, eps_cos, rn, kappa);
    }
}

// write 4 scaled values as fp16 hi / lo at the same (row, col) of two images
__device__ __forceinline__ void put_split4(_Float16* hi_img, _Float16* lo_img, int off, const float4& x) {
    h4 hi, lo;
    split4(x, hi, lo);
    *reinterpret_cast<h4*>(hi_img + off) = hi;
    *reinterpret_cast<h4*>(lo_img + off) = lo;
}

}  // namespace ge2e
