// Pointwise activations of the GEMM epilogues (leco_gemm_args.act), shared by every kernel that applies one.  Include
// after <leco_prims.h>.
#pragma once
#include "leco_hip.h"

namespace leco {
// gelu(x) = x Phi(x) (the erf form diffusers' GEGLU and OpenCLIP's MLP use, F.gelu) with erf by Abramowitz-Stegun 7.1.26
// (|err| <= 1.5e-7, far below the bf16 rounding of the result): one v_rcp + one v_exp instead of libm's branchy erff, which
// made the fused GEGLU epilogue cost MORE than the K loop it follows (tools/ablate_gemm.py --plain: 48 of 86 us on the
// level-0 tile).  x < 0 uses q = 1 - erf directly: no cancellation in the tail.
__device__ __forceinline__ float gelu_fast(float x) {
    const float z = fabsf(x) * 0.7071067811865476f;
    const float t = fast_rcp(1.f + 0.3275911f * z);
    const float poly = t * (0.254829592f + t * (-0.284496736f + t * (1.421413741f + t * (-1.453152027f + t * 1.061405429f))));
    const float hq = 0.5f * x * poly * fast_exp2(-z * z * 1.4426950408889634f);   // 0.5 x (1 - erf(|x| / sqrt 2))
    return x >= 0.f ? x - hq : hq;
}
// quick-GELU (CLIP-L's MLP, transformers' QuickGELUActivation): x sigmoid(1.702 x)
__device__ __forceinline__ float quick_gelu(float x) { return x / (1.f + __expf(-1.702f * x)); }

// the pointwise members of the act enum (LECO_ACT_GEGLU pairs two columns: the GEMM epilogue handles it itself)
template <int N>
__device__ __forceinline__ void apply_act(float (&v)[N], int act) {
    if (act == LECO_ACT_SILU) {
#pragma unroll
        for (int r = 0; r < N; ++r) v[r] = v[r] / (1.f + __expf(-v[r]));
    } else if (act == LECO_ACT_QUICK_GELU) {
#pragma unroll
        for (int r = 0; r < N; ++r) v[r] = quick_gelu(v[r]);
    } else if (act == LECO_ACT_GELU) {
#pragma unroll
        for (int r = 0; r < N; ++r) v[r] = gelu_fast(v[r]);
    }
}
}  // namespace leco
