// mesh_common.h - what the translation units of libgadapt_mesh.so share: the error string behind gadapt_mesh_last_error()
// and the wave reductions on DPP (mmpde5_kernels.hip, ma_kernels.hip, ma_strided_kernels.hip, ma_m2n_slow_kernels.hip,
// ma_table_kernels.hip).
#ifndef GADAPT_MESH_COMMON_H
#define GADAPT_MESH_COMMON_H

#include <hip/hip_runtime.h>
#include <stdio.h>

namespace gadapt_mesh_shared {

inline thread_local char g_err[256] = "";

inline int mesh_fail(int code, const char* msg) {
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}

template <int CTRL>
__device__ inline float dpp_move(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}

// Sum over the 64 lanes, the same bits in every lane: a butterfly inside each row of 16 (quad_perm [1,0,3,2], [2,3,0,1],
// row_half_mirror, row_mirror: each lane adds its partner's value, and a + b == b + a), then the four rows in a fixed order.
__device__ inline float wave_sum(float v) {
    v = v + dpp_move<0xB1>(v);
    v = v + dpp_move<0x4E>(v);
    v = v + dpp_move<0x141>(v);
    v = v + dpp_move<0x140>(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return (r0 + r1) + (r2 + r3);
}

// The same butterfly with max / min (the Monge-Ampere kernels): only lane 0's value is used, and every lane reads it back from LDS.
__device__ inline float wave_max(float v) {
    v = fmaxf(v, dpp_move<0xB1>(v));
    v = fmaxf(v, dpp_move<0x4E>(v));
    v = fmaxf(v, dpp_move<0x141>(v));
    v = fmaxf(v, dpp_move<0x140>(v));
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}

__device__ inline float wave_min(float v) { return -wave_max(-v); }

}  // namespace gadapt_mesh_shared

#endif
