// The GEMM epilogue on registers (leco_gemm_args: + bias[n] + rowbias[sample][n] + residual, activation, fp32 and / or
// bf16 store) for 4 consecutive columns of one output row.  Device only; include after <leco_prims.h>.  The two split-K
// finishing kernels (gemm.hip) call it; gemm_kernel and conv_patch_kernel still spell the same sequence out, 8 columns
// wide, inside their staged item loops ("GEMM epilogue": calling a shared form there cost
// registers and 0.2 % of the step).
#pragma once
#include "act.h"

namespace leco {

// v[4] = columns n .. n + 3 of output row m (fp32 sums); rr = the residual's two words for them (read only where
// p.residual is set).  Stores what p asks for and returns the bf16 words as stored (zeros without a bf16 output): the
// statistics are taken from them.
__device__ __forceinline__ u32x2 epi_apply4(const leco_gemm_args& p, int m, int n, float (&v)[4], const u32x2 rr) {
    if (p.bias) {
        const f32x4 b = *(const f32x4*)(p.bias + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += b[r];
    }
    if (p.rowbias) {
        const f32x4 b = *(const f32x4*)(p.rowbias + (int64_t)(m / p.rows_per_group) * p.ld_rowbias + n);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] += b[r];
    }
    if (p.residual) {
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            v[2 * r] += bf2f((bf16_t)(rr[r] & 0xffffu));
            v[2 * r + 1] += bf2f((bf16_t)(rr[r] >> 16));
        }
    }
    apply_act(v, p.act);
    if (p.c_f32) {
        const f32x4 of = {v[0], v[1], v[2], v[3]};
        *(f32x4*)(p.c_f32 + (int64_t)m * p.ldc32 + n) = of;
    }
    u32x2 o = {0u, 0u};
    if (p.c) {
        o = u32x2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
        *(u32x2*)((bf16_t*)p.c + (int64_t)m * p.ldc + n) = o;
    }
    return o;
}

}  // namespace leco
