// ge_wave.h -- what the wave-per-row kernels share: a lane's vector of a row, the raw buffer accesses and the wave reduction.
// k_adagrad_runs (glove.hip) and k_strata_fp32 (strata_fp32.hip) use the same lane shape, the same accesses and the same
// reduction tree, which tests/kernel_model.py restates (lane_dot, wave_sum).
#pragma once
#include "ge_common.h"

namespace ge {

template <int VW> struct Vec;
template <> struct Vec<4> { using T = float4; };
template <> struct Vec<2> { using T = float2; };
template <> struct Vec<1> { using T = float; };

template <int VW> __device__ __forceinline__ float &comp(typename Vec<VW>::T &v, int c);
template <> __device__ __forceinline__ float &comp<4>(float4 &v, int c) { return (&v.x)[c]; }
template <> __device__ __forceinline__ float &comp<2>(float2 &v, int c) { return (&v.x)[c]; }
template <> __device__ __forceinline__ float &comp<1>(float &v, int) { return v; }

typedef int   ge_i4 __attribute__((ext_vector_type(4)));
typedef int   ge_i2 __attribute__((ext_vector_type(2)));

constexpr int AUX_PLAIN = 0;
constexpr int AUX_SC1 = 16;     // agent-coherent: bypasses the CU's L1, sees memory-side atomics

template <int VW, int AUX>
__device__ __forceinline__ typename Vec<VW>::T buf_load(__amdgpu_buffer_rsrc_t rs, int off) {
    typename Vec<VW>::T r;
    if constexpr (VW == 4) { ge_i4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, AUX); __builtin_memcpy(&r, &v, 16); }
    else if constexpr (VW == 2) { ge_i2 v = __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, AUX); __builtin_memcpy(&r, &v, 8); }
    else { int v = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, AUX); __builtin_memcpy(&r, &v, 4); }
    return r;
}
template <int VW>
__device__ __forceinline__ void buf_store(typename Vec<VW>::T val, __amdgpu_buffer_rsrc_t rs, int off) {
    if constexpr (VW == 4) { ge_i4 v; __builtin_memcpy(&v, &val, 16); __builtin_amdgcn_raw_buffer_store_b128(v, rs, off, 0, AUX_SC1); }
    else if constexpr (VW == 2) { ge_i2 v; __builtin_memcpy(&v, &val, 8); __builtin_amdgcn_raw_buffer_store_b64(v, rs, off, 0, AUX_SC1); }
    else { int v; __builtin_memcpy(&v, &val, 4); __builtin_amdgcn_raw_buffer_store_b32(v, rs, off, 0, AUX_SC1); }
}
__device__ __forceinline__ float buf_load_f32(__amdgpu_buffer_rsrc_t rs, int off, bool coherent) {
    int v = coherent ? __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, AUX_SC1)
                     : __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, AUX_PLAIN);
    return __builtin_bit_cast(float, v);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ int rfl(int v) { return __builtin_amdgcn_readfirstlane(v); }
// Sum over the 64 lanes, result in every lane.  Four DPP adds reduce each row of 16 lanes
// (quad swaps, half-row mirror, row mirror), then the four row sums are read through SGPRs.
__device__ __forceinline__ float dpp_add(float v, int ctrl_sel) {
    const int iv = __builtin_bit_cast(int, v);
    int r;
    switch (ctrl_sel) {
        case 0:  r = __builtin_amdgcn_update_dpp(0, iv, 0xB1, 0xF, 0xF, false); break;    // quad_perm [1,0,3,2]
        case 1:  r = __builtin_amdgcn_update_dpp(0, iv, 0x4E, 0xF, 0xF, false); break;    // quad_perm [2,3,0,1]
        case 2:  r = __builtin_amdgcn_update_dpp(0, iv, 0x141, 0xF, 0xF, false); break;   // row_half_mirror
        default: r = __builtin_amdgcn_update_dpp(0, iv, 0x140, 0xF, 0xF, false); break;   // row_mirror
    }
    return v + __builtin_bit_cast(float, r);
}
__device__ __forceinline__ float wave_sum(float v) {
    v = dpp_add(v, 0); v = dpp_add(v, 1); v = dpp_add(v, 2); v = dpp_add(v, 3);
    const int iv = __builtin_bit_cast(int, v);
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(iv, 48));
    return (r0 + r1) + (r2 + r3);
}

}  // namespace ge
