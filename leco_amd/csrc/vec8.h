// 16-byte vectors of 8 bf16 <-> 8 floats, and the launch grid of the kernels that stride over them: shared by the HBM-bound
// translation units.  Include after <leco_prims.h>.
#pragma once
#include <stdint.h>

namespace leco {
__device__ __forceinline__ void unpack8(const u32x4& v, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = bf2f((bf16_t)(v[i] & 0xffffu));
        f[2 * i + 1] = bf2f((bf16_t)(v[i] >> 16));
    }
}
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = pack_bf2(f[2 * i], f[2 * i + 1]);
    return v;
}

// 256-thread workgroups of a grid-stride kernel over n_items work items
inline int grid_for(int64_t n_items) {
    int64_t g = (n_items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}
}  // namespace leco
