// Double-precision sums over a 256-thread workgroup in a FIXED order: what the reductions that must be bitwise reproducible
// (Prodigy's two sums in elementwise.hip, the gradient norm in grad_clip.hip) are built from.  Include after <leco_prims.h>.
#pragma once

namespace leco {
__device__ __forceinline__ double shfl_xor_f64(double v, int mask) {      // the two halves travel as bit patterns
    const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
    const float lo = shfl_xor(__builtin_bit_cast(float, (unsigned)(u & 0xffffffffull)), mask);
    const float hi = shfl_xor(__builtin_bit_cast(float, (unsigned)(u >> 32)), mask);
    return __builtin_bit_cast(double, ((unsigned long long)__builtin_bit_cast(unsigned, hi) << 32) |
                                          (unsigned long long)__builtin_bit_cast(unsigned, lo));
}
// sums of a and b over the 256 threads of the block, in a fixed order (xor butterfly in each wave, then the four wave totals);
// the result is valid in thread 0.  `red` is free again after the next __syncthreads().
__device__ __forceinline__ void block_sum_f64(double& a, double& b, double (&red)[2][4]) {
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) {
        a += shfl_xor_f64(a, mk);
        b += shfl_xor_f64(b, mk);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = a;
        red[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}
}  // namespace leco
