// Max-norm regularisation of the LoRA weights on the flat fp32 slab (train.scale_weight_norms): per module the Frobenius
// norm of its effective update scale * up * down, the decision against the bound, the in-place pull-back of both matrices
// (slab and bf16 shadow) and the cross-module statistics, in ONE launch.  The slab is fp32 in the bf16 and the fp32 compute
// modes alike.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <leco_prims.h>
#include <math.h>

#include "common.h"
#include "reduce_f64.h"

namespace leco {
namespace {

// ---- leco_lora_max_norm ---------------------------------------------------------------------------------------------
// One 256-thread workgroup per module.  With D = lora_down [r][K] and U = lora_up [N][r]:
//     |U D|_F^2 = sum_ij (U^T U)_ij (D D^T)_ij
// so U D is never formed: the two r x r Gram matrices are walked in TILE x TILE tiles of (i, j) pairs (upper triangle,
// off-diagonal entries weighted 2).  The rows i and j of D (columns of U) of a tile pass through LDS in chunks of CHUNK
// elements; every Gram entry belongs to ONE thread group of S threads (S = 256 / T^2 with T = 4, 8 or 16 chosen from r, so
// that rank 4 still uses the whole workgroup), thread s of the group adding the products of elements s, s + S, ... of every
// chunk in order, in double (an fp32 x fp32 product is exact in double); the S partials are then added in the order 0 .. S-1
// and the per-pair products G_U G_D by the fixed-order block sum.  Nothing depends on timing: two launches on the same slab
// are bit-equal, and data-parallel replicas, which hold the same slab, take the same decisions without communicating.
// Every thread of the workgroup ends with the same norm and derives the same factor; the workgroup then scales its own
// module.  Cross-module statistics: the ticket scheme of grad_clip_kernel -- each workgroup leaves its module's norm after
// scaling and its flags in scratch of this kernel's own, and the one that draws the last ticket adds them in a FIXED order
// (thread t takes modules t, t + 256, ...) and re-arms the ticket.  The scratch is per device: launches must be
// stream-ordered (they are: one per optimizer step).
constexpr int NORM_MAX_MODULES = 8192;
constexpr int TILE = 16, CHUNK = 128, LDT = CHUNK + 1;     // (+1: the 16 rows of a tile fall into different LDS banks)
__device__ double g_norm_part[NORM_MAX_MODULES];
__device__ unsigned g_norm_flag[NORM_MAX_MODULES];          // bit 0: scaled, bit 1: norm not finite
__device__ unsigned g_norm_ticket = 0;

__device__ __forceinline__ bool finite_f64(double v) {
    return (__builtin_bit_cast(unsigned long long, v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// This thread's share of sum_c X(i, c) X(j, c) for its pair (i0 + pi, j0 + pj): X(i, c) = base[i * rs + c * cs], c < len.
// Rows past r are staged as zeros.  Block-uniform control flow (the barriers are met by all 256 threads).
__device__ __forceinline__ double gram_share(const float* base, int64_t rs, int64_t cs, int len, int r, int i0, int j0, int T,
                                             int S, int pi, int pj, int s, bool active, float* ti, float* tj) {
    double acc = 0.0;
    for (int c0 = 0; c0 < len; c0 += CHUNK) {
        const int cl = min(CHUNK, len - c0);
        __syncthreads();                                               // the previous chunk has been consumed
        for (int idx = threadIdx.x; idx < T * cl; idx += 256) {
            int row, col;                                              // consecutive threads walk consecutive addresses
            if (cs == 1) { row = idx / cl; col = idx - row * cl; } else { col = idx / T; row = idx - col * T; }
            const int64_t at = (int64_t)(c0 + col) * cs;
            ti[row * LDT + col] = i0 + row < r ? base[(int64_t)(i0 + row) * rs + at] : 0.f;
            tj[row * LDT + col] = j0 + row < r ? base[(int64_t)(j0 + row) * rs + at] : 0.f;
        }
        __syncthreads();
        if (active)
            for (int c = s; c < cl; c += S) acc += (double)ti[pi * LDT + c] * (double)tj[pj * LDT + c];
    }
    return acc;
}

__global__ __launch_bounds__(256) void lora_max_norm_kernel(float* slab, bf16_t* shadow, int64_t n_slab,
                                                             const leco_lora_norm_module* table, int M, float max_norm,
                                                             float* norms, float* factors, float* stats) {
    __shared__ float ti[TILE * LDT], tj[TILE * LDT];
    __shared__ double part_u[256], part_d[256];
    __shared__ double red[2][4];
    __shared__ bool last;
    const int m = blockIdx.x, tid = threadIdx.x;
    const leco_lora_norm_module mod = table[m];
    const int r = mod.r, K = mod.k, N = mod.n;
    // a table row that does not lie inside the slab is never followed: it is reported like a non-finite norm
    const bool inside = r > 0 && K > 0 && N > 0 && mod.down_off >= 0 && mod.up_off >= 0 &&
                        mod.down_off + (int64_t)r * K <= n_slab && mod.up_off + (int64_t)N * r <= n_slab;
    double sum2 = 0.0, unused = 0.0;
    if (inside) {                                                      // (block-uniform)
        const float* D = slab + mod.down_off;
        const float* U = slab + mod.up_off;
        const int T = r <= 4 ? 4 : (r <= 8 ? 8 : 16), S = 256 / (T * T);
        const int p = tid % (T * T), s = tid / (T * T), pi = p / T, pj = p % T;
        for (int i0 = 0; i0 < r; i0 += T)
            for (int j0 = i0; j0 < r; j0 += T) {
                const int i = i0 + pi, j = j0 + pj;
                const bool active = i < r && j < r && i <= j;
                const double gd = gram_share(D, K, 1, K, r, i0, j0, T, S, pi, pj, s, active, ti, tj);    // (D D^T)_ij
                const double gu = gram_share(U, 1, r, N, r, i0, j0, T, S, pi, pj, s, active, ti, tj);    // (U^T U)_ij
                __syncthreads();                                       // part_* of the previous tile have been read
                part_d[tid] = gd;
                part_u[tid] = gu;
                __syncthreads();
                if (active && s == 0) {
                    double fd = 0.0, fu = 0.0;
                    for (int q = 0; q < S; ++q) {
                        fd += part_d[p + q * T * T];
                        fu += part_u[p + q * T * T];
                    }
                    sum2 += (i < j ? 2.0 : 1.0) * (fu * fd);
                }
            }
        __syncthreads();
    }
    block_sum_f64(sum2, unused, red);                                  // every thread holds the same total afterwards
    const double qnan = __builtin_bit_cast(double, 0x7ff8000000000000ull);
    const double norm = inside ? (double)mod.scale * sqrt(sum2) : qnan;
    const bool finite = finite_f64(norm);
    const bool scaled = finite && max_norm > 0.f && norm > (double)max_norm;
    const double ratio = scaled ? (double)max_norm / norm : 1.0;
    const float f = scaled ? (float)sqrt(ratio) : 1.f;
    if (scaled) {                                                      // (block-uniform) both matrices, slab and shadow
        const int64_t nd = (int64_t)r * K, nu = (int64_t)N * r;
        for (int64_t e = tid; e < nd; e += 256) {
            const float v = slab[mod.down_off + e] * f;
            slab[mod.down_off + e] = v;
            shadow[mod.down_off + e] = f2bf(v);
        }
        for (int64_t e = tid; e < nu; e += 256) {
            const float v = slab[mod.up_off + e] * f;
            slab[mod.up_off + e] = v;
            shadow[mod.up_off + e] = f2bf(v);
        }
    }
    if (tid == 0) {
        norms[m] = (float)norm;
        factors[m] = f;
        g_norm_part[m] = finite ? norm * ratio : 0.0;
        g_norm_flag[m] = (scaled ? 1u : 0u) | (finite ? 0u : 2u);
        __threadfence();                                               // visible device-wide before the ticket
        last = atomicAdd(&g_norm_ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;                                                 // (block-uniform)
    __threadfence();
    double tot = 0.0, top = 0.0, n_scaled = 0.0, n_bad = 0.0;          // (small integer counts are exact in double)
    for (int b = tid; b < M; b += 256) {
        const unsigned fl = ((volatile unsigned*)g_norm_flag)[b];
        const double v = ((volatile double*)g_norm_part)[b];
        if (fl & 2u) {
            n_bad += 1.0;
        } else {
            tot += v;
            top = fmax(top, v);
        }
        if (fl & 1u) n_scaled += 1.0;
    }
    __syncthreads();                                                   // `red` is free again
    block_sum_f64(tot, n_scaled, red);
    __syncthreads();
    block_sum_f64(n_bad, unused, red);
    __syncthreads();
#pragma unroll
    for (int mk = 32; mk >= 1; mk >>= 1) top = fmax(top, shfl_xor_f64(top, mk));
    if ((tid & 63) == 0) red[0][tid >> 6] = top;
    __syncthreads();
    if (tid == 0) {
        top = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
        const double n_finite = (double)M - n_bad;
        stats[0] = (float)n_scaled;
        stats[1] = (float)(n_finite > 0.0 ? tot / n_finite : 0.0);
        stats[2] = (float)top;
        stats[3] = (float)n_bad;
        g_norm_ticket = 0;                                             // re-armed for the next (stream-ordered) launch
    }
}

}  // namespace
}  // namespace leco

using namespace leco;
#define LECO_STREAM ((hipStream_t)stream)

extern "C" int leco_lora_max_norm(float* slab, void* shadow, int64_t n, const leco_lora_norm_module* table, int32_t M,
                                  float max_norm, float* norms, float* factors, float* stats, leco_stream_t stream) {
    if (!slab || !shadow || !table || !norms || !factors || !stats || n <= 0)
        return fail(-EINVAL, "leco_lora_max_norm: null operand or n=%lld <= 0", (long long)n);
    if (M <= 0 || M > NORM_MAX_MODULES)
        return fail(-EINVAL, "leco_lora_max_norm: M=%d modules, must be 1 .. %d", (int)M, NORM_MAX_MODULES);
    if (!(max_norm >= 0.f)) return fail(-EINVAL, "leco_lora_max_norm: max_norm=%g must be >= 0 (0: measure only)", (double)max_norm);
    hipLaunchKernelGGL(lora_max_norm_kernel, dim3(M), dim3(256), 0, LECO_STREAM, slab, (bf16_t*)shadow, n, table, (int)M,
                       max_norm, norms, factors, stats);
    return check_launch("leco_lora_max_norm");
}
