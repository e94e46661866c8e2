// Controls on the flat fp32 LoRA gradient slab between the backward and the optimizer: the global L2 norm with clipping
// through the optimizers' own device-side grad_scale, and the accumulation of micro-steps.  The slab is fp32 in the bf16
// and the fp32 compute modes alike: both entry points serve both.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <leco_prims.h>
#include <math.h>

#include "common.h"
#include "reduce_f64.h"
#include "vec8.h"

namespace leco {
namespace {

// ---- leco_grad_clip: norm = |grad_scale g|, hyper[3] *= min(1, max_norm / (norm + 1e-6)) -------------------------------
// The reduction of prodigy_moments_kernel (elementwise.hip): a fixed grid, each block leaves its partials (the double sum
// of squares, the integer count of non-finite elements) in scratch of this kernel's own and draws a ticket; the block that
// draws the last one adds the partials in a FIXED order (thread t takes blocks t, t + 256, ...), so the result is bitwise
// reproducible and data-parallel replicas, which see the same all-reduced slab, derive the same coef.  Every thread reads
// hyper[3] before its block's sum, i.e. before the block draws its ticket: when the last block rewrites it, nobody reads
// it any more.  The scratch is per device: launches must be stream-ordered (they are: one per optimizer step).
constexpr int CLIP_BLOCKS = 8192;                      // grid_for's cap
__device__ double g_clip_part[CLIP_BLOCKS];
__device__ unsigned g_clip_bad[CLIP_BLOCKS];
__device__ unsigned g_clip_ticket = 0;

__global__ __launch_bounds__(256) void grad_clip_kernel(const float* g, int64_t n, float* hyper, float max_norm,
                                                         float* stats) {
    __shared__ double red[2][4];
    __shared__ bool last;
    const double gs = (double)hyper[3];
    double sum = 0.0, bad = 0.0;                       // (the count rides the pair reduction: small integers are exact)
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const float x = g[e];
        const double v = (double)x * gs;
        sum += v * v;
        if ((__builtin_bit_cast(unsigned, x) & 0x7f800000u) == 0x7f800000u) bad += 1.0;      // inf or NaN
    }
    block_sum_f64(sum, bad, red);
    if (threadIdx.x == 0) {
        g_clip_part[blockIdx.x] = sum;
        g_clip_bad[blockIdx.x] = (unsigned)bad;
        __threadfence();                                               // partials visible device-wide before the ticket
        last = atomicAdd(&g_clip_ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;                                                 // (block-uniform)
    __threadfence();
    double ts = 0.0, tb = 0.0;
    for (unsigned b = threadIdx.x; b < gridDim.x; b += 256) {
        ts += ((volatile double*)g_clip_part)[b];
        tb += (double)((volatile unsigned*)g_clip_bad)[b];
    }
    __syncthreads();                                                   // thread 0 is done with `red`
    block_sum_f64(ts, tb, red);
    if (threadIdx.x == 0) {           // every block has read hyper[3] before it drew its ticket: it may change now
        const double norm = sqrt(ts);
        double coef = 1.0;
        if (max_norm > 0.f && tb == 0.0) coef = fmin(1.0, (double)max_norm / (norm + 1e-6));
        stats[0] = (float)norm;
        stats[1] = (float)coef;
        stats[2] = (float)tb;
        stats[3] = 0.f;
        if (coef < 1.0) hyper[3] = (float)(gs * coef);
        g_clip_ticket = 0;                                             // re-armed for the next (stream-ordered) launch
    }
}

// ---- leco_grad_accumulate: acc = first ? g : acc + g -------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_accumulate_kernel(float* acc, const float* g, int64_t n, int first) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256)
        acc[e] = first ? g[e] : acc[e] + g[e];
}

}  // namespace
}  // namespace leco

using namespace leco;
#define LECO_STREAM ((hipStream_t)stream)

extern "C" int leco_grad_clip(const float* g, int64_t n, float* hyper, float max_norm, float* stats, leco_stream_t stream) {
    if (!g || !hyper || !stats || n <= 0) return fail(-EINVAL, "leco_grad_clip: null operand or n=%lld <= 0", (long long)n);
    if (!(max_norm >= 0.f)) return fail(-EINVAL, "leco_grad_clip: max_norm=%g must be >= 0 (0: measure only)", (double)max_norm);
    const int grid = grid_for(n);                 // <= CLIP_BLOCKS: one partial per block; a function of n alone
    hipLaunchKernelGGL(grad_clip_kernel, dim3(grid), dim3(256), 0, LECO_STREAM, g, n, hyper, max_norm, stats);
    return check_launch("leco_grad_clip");
}

extern "C" int leco_grad_accumulate(float* acc, const float* g, int64_t n, int32_t first, leco_stream_t stream) {
    if (!acc || !g || n <= 0) return fail(-EINVAL, "leco_grad_accumulate: null operand or n=%lld <= 0", (long long)n);
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(grid_for(n)), dim3(256), 0, LECO_STREAM, acc, g, n, (int)first);
    return check_launch("leco_grad_accumulate");
}
