// Cross-attention token heatmaps (leco_amd/attn_maps.py, `Engine.plan(attn_maps=M)`):
//   * leco_xattn_token_maps: maps[b][m][i] += step_w / heads * sum_h sum_j tok_w[m][j] softmax_j(scale <q_bhi, k_bhj>), from
//     the Q and K operands of a cross-attention -- the probabilities the attention kernels never write anywhere;
//   * leco_attn_maps_merge: the layer maps of one UNet pass -> one heat map per (sample, word) at picture size, a weighted sum
//     of bilinear resamplings (torch's align_corners=False rule);
//   * leco_heat_overlay: a heat map blended over a uint8 picture through a 256-entry colour table.
//
// Token maps on gfx950.  A workgroup (4 waves) owns 64 query rows of one sample, a wave 16 of them, for ALL heads: the heads
// are a loop inside the workgroup, so every (b, m, i) has one owner, the sum over heads is formed in registers in a fixed
// order and nothing is atomic.  Per head the <= 128 keys of that head (skv x d bf16, at most 128 x 160 = 40 KB) are staged
// in LDS, rows padded by 16 bytes (the fragment reads are ds_read_b128: consecutive rows start 4 banks apart plus the row
// length); key rows past skv and the columns that pad d to a multiple of 32 are zeros that are SELECTED, never loaded.
// S^T = K Q^T runs on v_mfma_f32_16x16x32_bf16 (A = 16 keys, B = the wave's 16 query rows): lane l then holds, for query row
// l & 15, the scores of keys 16 f + 4 (l >> 4) + r of every 16-key tile f, i.e. a whole softmax row lives in the four lanes
// that share l & 15: 32 fp32 registers, one rows4_max and one rows4_sum per head.  All keys of a row are in that one tile, so
// the maximum and the sum are the exact ones (no running rescale).  Everything behind the MFMA accumulators is fp32: the
// probabilities are never rounded to bf16.  The token weights sit in LDS as fp32 [8][128], zero past skv / n_maps.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <leco_prims.h>
#include <math.h>

#include "common.h"

namespace leco {
namespace {

constexpr int TM_MAX_KEYS = 128, TM_MAX_MAPS = 8;

struct TokenMapArgs {
    const bf16_t* q;
    int64_t ldq, bsq;
    const bf16_t* k;
    int64_t ldk, bsk;
    const float* tok_w;
    int n_maps;
    const float* step_w;
    float* maps;
    int heads, sq, skv;
    float scale;
};

template <int D>
__global__ __launch_bounds__(256) void xattn_token_maps_kernel(TokenMapArgs p) {
    constexpr int DK = (D + 31) / 32 * 32, NKS = DK / 32, NDC = D / 8;
    constexpr int KROW = DK + 8;                                   // padded K row (elements)
    __shared__ __attribute__((aligned(16))) bf16_t sK[TM_MAX_KEYS * KROW];
    __shared__ __attribute__((aligned(16))) float sW[TM_MAX_MAPS * TM_MAX_KEYS];

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const int b = (int)blockIdx.y;
    const int qrow = (int)blockIdx.x * 64 + wave * 16 + fr;
    const bool row_ok = qrow < p.sq;
    const int nt = (p.skv + 15) >> 4;                              // 16-key tiles that hold a key
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    for (int e = tid; e < TM_MAX_MAPS * TM_MAX_KEYS; e += 256) {
        const int m = e / TM_MAX_KEYS, j = e - m * TM_MAX_KEYS;
        sW[e] = (m < p.n_maps && j < p.skv) ? p.tok_w[(int64_t)m * p.skv + j] : 0.f;
    }
    if constexpr (DK / 8 > NDC) {      // the columns [D, DK) of every key row: zeros, written once (the staging covers [0, D))
        constexpr int PADC = DK / 8 - NDC;
        for (int e = tid; e < TM_MAX_KEYS * PADC; e += 256) {
            const int key = e / PADC, ch = NDC + e % PADC;
            *(u32x4*)(sK + key * KROW + ch * 8) = zero4;
        }
    }

    const bf16_t* qb = p.q + (int64_t)b * p.bsq;
    const bf16_t* kb = p.k + (int64_t)b * p.bsk;
    float acc[TM_MAX_MAPS];
#pragma unroll
    for (int m = 0; m < TM_MAX_MAPS; ++m) acc[m] = 0.f;
    const float log2e = 1.4426950408889634f;

    for (int h = 0; h < p.heads; ++h) {
        __syncthreads();               // the previous head's fragment reads are done (first head: orders nothing that matters)
        for (int e = tid; e < nt * 16 * NDC; e += 256) {
            const int key = e / NDC, ch = e - key * NDC;
            const u32x4 v = key < p.skv ? *(const u32x4*)(kb + (int64_t)key * p.ldk + h * D + ch * 8) : zero4;
            *(u32x4*)(sK + key * KROW + ch * 8) = v;
        }
        // Q fragments of this head (MFMA B operand: column = query row, k = head dim); rows past sq are not read
        bf16x8 qf[NKS];
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int ch = ks * 4 + fg;
            const u32x4 t = (row_ok && ch < NDC) ? *(const u32x4*)(qb + (int64_t)qrow * p.ldq + h * D + ch * 8) : zero4;
            qf[ks] = __builtin_bit_cast(bf16x8, t);
        }
        __syncthreads();

        // S^T = K Q^T: lane holds s[f][r] = <q_fr, k_(16 f + 4 fg + r)>; tiles past the last key are never formed
        f32x4 s[TM_MAX_KEYS / 16];
        float mx = -INFINITY;
#pragma unroll
        for (int f = 0; f < TM_MAX_KEYS / 16; ++f) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
            if (f < nt) {
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    const bf16x8 kf = *(const bf16x8*)(sK + (16 * f + fr) * KROW + (ks * 4 + fg) * 8);
                    a = mfma16(kf, qf[ks], a);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = 16 * f + 4 * fg + r;
                a[r] = key < p.skv ? a[r] * p.scale : -INFINITY;        // masked by selection
                mx = fmaxf(mx, a[r]);
            }
            s[f] = a;
        }
        mx = rows4_max(mx);                                            // skv >= 1: finite
        float rs = 0.f;
        float part[TM_MAX_MAPS];
#pragma unroll
        for (int m = 0; m < TM_MAX_MAPS; ++m) part[m] = 0.f;
#pragma unroll
        for (int f = 0; f < TM_MAX_KEYS / 16; ++f) {
            if (f < nt) {
                f32x4 e;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = 16 * f + 4 * fg + r;
                    e[r] = key < p.skv ? fast_exp2((s[f][r] - mx) * log2e) : 0.f;
                }
                rs += (e[0] + e[1]) + (e[2] + e[3]);
#pragma unroll
                for (int m = 0; m < TM_MAX_MAPS; ++m) {
                    if (m < p.n_maps) {
                        const f32x4 w = *(const f32x4*)(sW + m * TM_MAX_KEYS + 16 * f + 4 * fg);
                        part[m] = fmaf(w[0], e[0], part[m]);
                        part[m] = fmaf(w[1], e[1], part[m]);
                        part[m] = fmaf(w[2], e[2], part[m]);
                        part[m] = fmaf(w[3], e[3], part[m]);
                    }
                }
            }
        }
        const float inv = 1.0f / rows4_sum(rs);                        // >= 1: the row maximum contributes exp2(0)
#pragma unroll
        for (int m = 0; m < TM_MAX_MAPS; ++m) acc[m] = fmaf(part[m], inv, acc[m]);
    }

    // the four lanes of a query row hold a quarter of its keys each; lane group fg stores maps fg and fg + 4
    const float wgt = p.step_w[0] / (float)p.heads;
#pragma unroll
    for (int m = 0; m < TM_MAX_MAPS; ++m) {
        const float v = rows4_sum(acc[m]);
        if (row_ok && m < p.n_maps && (m & 3) == fg) {
            float* o = p.maps + ((int64_t)b * p.n_maps + m) * p.sq + qrow;
            *o = fmaf(wgt, v, *o);
        }
    }
}

struct MergeLayer {       // == leco_attn_map_layer
    const float* map;
    int32_t h, w;
    float weight;
};

// torch's area_pixel_compute_source_index (align_corners = False, not cubic): src = max(scale (dst + 0.5) - 0.5, 0)
__device__ __forceinline__ void bilinear_tap(int dst, int in, float scale, int& i0, int& i1, float& l0, float& l1) {
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    i0 = (int)src;
    i0 = i0 < in - 1 ? i0 : in - 1;
    i1 = i0 < in - 1 ? i0 + 1 : i0;
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

__global__ __launch_bounds__(256) void attn_maps_merge_kernel(const MergeLayer* layers, int n_layers, float* heat, int planes, int ht,
                                                              int wt) {
    const int64_t total = (int64_t)planes * ht * wt;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int x = (int)(e % wt);
        const int64_t t = e / wt;
        const int y = (int)(t % ht), pl = (int)(t / ht);
        float sum = 0.f;
        for (int l = 0; l < n_layers; ++l) {
            const MergeLayer L = layers[l];
            int y0, y1, x0, x1;
            float ly0, ly1, lx0, lx1;
            bilinear_tap(y, L.h, (float)L.h / (float)ht, y0, y1, ly0, ly1);
            bilinear_tap(x, L.w, (float)L.w / (float)wt, x0, x1, lx0, lx1);
            const float* src = L.map + (int64_t)pl * L.h * L.w;
            const float v = ly0 * (lx0 * src[y0 * L.w + x0] + lx1 * src[y0 * L.w + x1])
                          + ly1 * (lx0 * src[y1 * L.w + x0] + lx1 * src[y1 * L.w + x1]);
            sum = fmaf(L.weight, v, sum);
        }
        heat[e] = sum;
    }
}

__global__ __launch_bounds__(256) void heat_overlay_kernel(const float* heat, const float* rmax, const unsigned char* pic,
                                                           const unsigned char* lut, unsigned char* out, int batch, int n_maps,
                                                           int map_index, int hw, float alpha) {
    const int64_t total = (int64_t)batch * hw;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int b = (int)(e / hw);
        const int64_t px = e - (int64_t)b * hw;
        const int pl = b * n_maps + map_index;
        const float v = fminf(fmaxf(heat[(int64_t)pl * hw + px] * rmax[pl], 0.f), 1.f);     // (a NaN becomes 0)
        const int idx = (int)(v * 255.f + 0.5f);
        const float av = alpha * v;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float mix = (float)pic[e * 3 + c] * (1.f - av) + (float)lut[idx * 3 + c] * av;
            out[e * 3 + c] = (unsigned char)floorf(fminf(fmaxf(mix, 0.f), 255.f) + 0.5f);
        }
    }
}
}  // namespace
}  // namespace leco

using namespace leco;

extern "C" int leco_xattn_token_maps(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk, int64_t bsk,
                                     const float* tok_w, int32_t n_maps, const float* step_w, float* maps, int32_t batch,
                                     int32_t heads, int32_t sq, int32_t skv, int32_t head_dim, float scale, leco_stream_t stream) {
    if (!q || !k || !tok_w || !step_w || !maps)
        return fail(-EINVAL, "xattn_token_maps: null operand (%s)",
                    !q ? "q" : (!k ? "k" : (!tok_w ? "tok_w" : (!step_w ? "step_w" : "maps"))));
    if (batch <= 0 || heads <= 0 || sq <= 0) return fail(-EINVAL, "xattn_token_maps: empty problem batch=%d heads=%d sq=%d", batch, heads, sq);
    if (n_maps < 1 || n_maps > TM_MAX_MAPS) return fail(-EINVAL, "xattn_token_maps: n_maps=%d must be in 1..%d", n_maps, TM_MAX_MAPS);
    if (skv < 1 || skv > TM_MAX_KEYS) return fail(-EINVAL, "xattn_token_maps: skv=%d must be in 1..%d (one key tile per row)", skv, TM_MAX_KEYS);
    if (head_dim != 32 && head_dim != 40 && head_dim != 64 && head_dim != 80 && head_dim != 160)
        return fail(-EINVAL, "xattn_token_maps: unsupported head_dim %d (32, 40, 64, 80, 160)", head_dim);
    const int64_t c = (int64_t)heads * head_dim;
    if (ldq % 8 || ldk % 8 || bsq % 8 || bsk % 8 || ldq < c || ldk < c || ((uintptr_t)q & 15) || ((uintptr_t)k & 15))
        return fail(-EINVAL, "xattn_token_maps: q / k must be 16-byte aligned with strides that are multiples of 8 and at least "
                             "heads * head_dim = %lld (ldq=%lld ldk=%lld)", (long long)c, (long long)ldq, (long long)ldk);
    if (batch > 65535) return fail(-EINVAL, "xattn_token_maps: batch=%d exceeds the grid", batch);
    TokenMapArgs a{(const bf16_t*)q, ldq, bsq, (const bf16_t*)k, ldk, bsk, tok_w, n_maps, step_w, maps, heads, sq, skv, scale};
    const dim3 grid((unsigned)cdiv(sq, 64), (unsigned)batch), block(256);
    hipStream_t s = (hipStream_t)stream;
    switch (head_dim) {
        case 32: hipLaunchKernelGGL(xattn_token_maps_kernel<32>, grid, block, 0, s, a); break;
        case 40: hipLaunchKernelGGL(xattn_token_maps_kernel<40>, grid, block, 0, s, a); break;
        case 64: hipLaunchKernelGGL(xattn_token_maps_kernel<64>, grid, block, 0, s, a); break;
        case 80: hipLaunchKernelGGL(xattn_token_maps_kernel<80>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(xattn_token_maps_kernel<160>, grid, block, 0, s, a); break;
    }
    return check_launch("leco_xattn_token_maps");
}

extern "C" int leco_attn_maps_merge(const leco_attn_map_layer* layers, int32_t n_layers, float* heat, int32_t planes, int32_t ht,
                                    int32_t wt, leco_stream_t stream) {
    static_assert(sizeof(MergeLayer) == sizeof(leco_attn_map_layer), "layer table layout");
    if (!layers || !heat) return fail(-EINVAL, "attn_maps_merge: null operand (%s)", !layers ? "layers" : "heat");
    if (n_layers <= 0 || planes <= 0 || ht <= 0 || wt <= 0)
        return fail(-EINVAL, "attn_maps_merge: empty problem layers=%d planes=%d ht=%d wt=%d", n_layers, planes, ht, wt);
    const int64_t total = (int64_t)planes * ht * wt;
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(attn_maps_merge_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const MergeLayer*)layers, n_layers,
                       heat, planes, ht, wt);
    return check_launch("leco_attn_maps_merge");
}

extern "C" int leco_heat_overlay(const float* heat, const float* rmax, const void* pic, const void* lut, void* out, int32_t batch,
                                 int32_t n_maps, int32_t map_index, int32_t ht, int32_t wt, float alpha, leco_stream_t stream) {
    if (!heat || !rmax || !pic || !lut || !out)
        return fail(-EINVAL, "heat_overlay: null operand (%s)", !heat ? "heat" : (!rmax ? "rmax" : (!pic ? "pic" : (!lut ? "lut" : "out"))));
    if (batch <= 0 || n_maps <= 0 || ht <= 0 || wt <= 0) return fail(-EINVAL, "heat_overlay: empty problem batch=%d n_maps=%d ht=%d wt=%d", batch, n_maps, ht, wt);
    if (map_index < 0 || map_index >= n_maps) return fail(-EINVAL, "heat_overlay: map_index=%d outside 0..%d", map_index, n_maps - 1);
    if (!(alpha >= 0.f && alpha <= 1.f)) return fail(-EINVAL, "heat_overlay: alpha=%g must be in [0, 1]", (double)alpha);
    if ((int64_t)ht * wt > 0x7fffffff) return fail(-EINVAL, "heat_overlay: picture of %d x %d exceeds 2^31 pixels", ht, wt);
    const int64_t total = (int64_t)batch * ht * wt;
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(heat_overlay_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, heat, rmax, (const unsigned char*)pic,
                       (const unsigned char*)lut, (unsigned char*)out, batch, n_maps, map_index, ht * wt, alpha);
    return check_launch("leco_heat_overlay");
}
