// Kernels of the CLIP image tower and the CLIP score that the rest of the kernel set lacks (leco_amd/clip_vision.py):
//   * leco_clip_preprocess: uint8 NHWC pixels -> the bf16 patch rows the patch-embedding GEMM reads, in one pass: PIL's
//     antialiased bicubic resize of the shortest edge, centre crop, 1/255, mean / std, patch flattening, K padding;
//   * leco_vit_embed: class token + patch embeddings + position embeddings -> the token rows of the encoder;
//   * leco_cosine_scores: cosines of image embeddings against text embeddings.
//
// Preprocessing on gfx950.  One workgroup owns one patch = one output row (p * p pixels x 3 channels + the zero padding up
// to a multiple of 64 columns); one work-item computes one output pixel, its three channels at once (the three bytes of a
// source pixel are adjacent).  The filter is separable and is applied in PIL's order: along each source row of the pixel's
// vertical window first (column taps), that sum clamped to [0, 255] as PIL's 8-bit intermediate picture is, then the row
// taps over those sums, clamped again.  Everything between the source bytes and the one bf16 rounding is fp32; PIL's two
// roundings to whole 8-bit levels are NOT made.  Only the rows and columns that survive the crop have table entries, so
// nothing outside the crop is computed.  The source windows overlap heavily between neighbouring pixels of a patch and
// stay in L1 / L2; at 512^2 -> 224^2 a pixel reads 11 x 11 taps, the whole picture 18 M bytes from cache: this is not the
// expensive part of a ViT forward.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <leco_prims.h>
#include <math.h>

#include "common.h"

namespace leco {
namespace {

struct PrepArgs {
    const unsigned char* img;      // [B][h][w][3]
    int h, w;
    const int32_t* row_tab;        // [S][2]: first source row, tap count
    const float* row_w;            // [S][row_taps]
    int row_taps;
    const int32_t* col_tab;        // [S][2]
    const float* col_w;            // [S][col_taps]
    int col_taps;
    const float* mean_std;         // mean[3], std[3]
    int p, g, kp;                  // patch size, patches per side, padded row length
    bf16_t* out;                   // [B * g * g][ldo]
    int64_t ldo;
};

__device__ __forceinline__ float clamp255(float v) { return fminf(fmaxf(v, 0.f), 255.f); }

__global__ __launch_bounds__(256) void clip_preprocess_kernel(PrepArgs a) {
    const int tid = (int)threadIdx.x;
    const int P = a.g * a.g, pp = a.p * a.p;
    const int row = (int)blockIdx.x;               // b * P + py * g + px
    const int b = row / P, t = row - b * P;
    const int py = t / a.g, px = t - py * a.g;
    bf16_t* orow = a.out + (int64_t)row * a.ldo;
    const unsigned char* src = a.img + (int64_t)b * a.h * a.w * 3;

    for (int e = tid; e < pp; e += 256) {
        const int i = e / a.p, j = e - i * a.p;
        const int oy = py * a.p + i, ox = px * a.p + j;
        // the tables are built and checked by the caller; the clamps keep every read inside the picture whatever they say
        int ys = a.row_tab[2 * oy], ny = a.row_tab[2 * oy + 1];
        int xs = a.col_tab[2 * ox], nx = a.col_tab[2 * ox + 1];
        ys = ys < 0 ? 0 : (ys > a.h - 1 ? a.h - 1 : ys);
        xs = xs < 0 ? 0 : (xs > a.w - 1 ? a.w - 1 : xs);
        ny = ny < a.row_taps ? ny : a.row_taps;
        ny = ny < a.h - ys ? ny : a.h - ys;
        nx = nx < a.col_taps ? nx : a.col_taps;
        nx = nx < a.w - xs ? nx : a.w - xs;
        const float* wy = a.row_w + (int64_t)oy * a.row_taps;
        const float* wx = a.col_w + (int64_t)ox * a.col_taps;
        float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;
        for (int ty = 0; ty < ny; ++ty) {
            const unsigned char* r = src + ((int64_t)(ys + ty) * a.w + xs) * 3;
            float h0 = 0.f, h1 = 0.f, h2 = 0.f;
            for (int tx = 0; tx < nx; ++tx) {
                const float w = wx[tx];
                h0 = fmaf(w, (float)r[3 * tx], h0);
                h1 = fmaf(w, (float)r[3 * tx + 1], h1);
                h2 = fmaf(w, (float)r[3 * tx + 2], h2);
            }
            const float v = wy[ty];
            acc0 = fmaf(v, clamp255(h0), acc0);
            acc1 = fmaf(v, clamp255(h1), acc1);
            acc2 = fmaf(v, clamp255(h2), acc2);
        }
        const float inv255 = 1.f / 255.f;
        orow[e] = f2bf((clamp255(acc0) * inv255 - a.mean_std[0]) / a.mean_std[3]);
        orow[pp + e] = f2bf((clamp255(acc1) * inv255 - a.mean_std[1]) / a.mean_std[4]);
        orow[2 * pp + e] = f2bf((clamp255(acc2) * inv255 - a.mean_std[2]) / a.mean_std[5]);
    }
    for (int c = 3 * pp + tid; c < a.kp; c += 256) orow[c] = (bf16_t)0;
}

// one work-item = 8 columns of one token row: 16-byte loads, fp32 sum, one 16-byte store
__global__ __launch_bounds__(256) void vit_embed_kernel(const bf16_t* patches, int64_t ldp, const bf16_t* cls, const bf16_t* pos,
                                                        int64_t ldpos, bf16_t* out, int64_t ldo, int batch, int tokens, int c8) {
    const int64_t total = (int64_t)batch * (tokens + 1) * c8;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / c8;
        const int ch = (int)(e - r * c8);
        const int b = (int)(r / (tokens + 1)), t = (int)(r - (int64_t)b * (tokens + 1));
        const bf16_t* s = t == 0 ? cls : patches + ((int64_t)b * tokens + (t - 1)) * ldp;
        u32x4 x = *(const u32x4*)(s + ch * 8);
        const u32x4 q = *(const u32x4*)(pos + (int64_t)t * ldpos + ch * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float lo = bf2f((bf16_t)(x[j] & 0xffffu)) + bf2f((bf16_t)(q[j] & 0xffffu));
            const float hi = bf2f((bf16_t)(x[j] >> 16)) + bf2f((bf16_t)(q[j] >> 16));
            x[j] = pack_bf2(lo, hi);
        }
        *(u32x4*)(out + r * ldo + ch * 8) = x;
    }
}

// one wave = one (image, text) pair: 16-byte loads, three fp32 sums, one wave reduction each
__global__ __launch_bounds__(256) void cosine_scores_kernel(const bf16_t* x, int64_t ldx, const bf16_t* y, int64_t ldy, float* out,
                                                            int64_t ldo, int nb, int nt, int d8, float scale) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int64_t pair = (int64_t)blockIdx.x * 4 + wave;
    if (pair < (int64_t)nb * nt) {          // wave-uniform
        const int b = (int)(pair / nt), t = (int)(pair - (int64_t)b * nt);
        const bf16_t* xr = x + (int64_t)b * ldx;
        const bf16_t* yr = y + (int64_t)t * ldy;
        float xy = 0.f, xx = 0.f, yy = 0.f;
        for (int ch = lane; ch < d8; ch += 64) {
            const u32x4 u = *(const u32x4*)(xr + ch * 8);
            const u32x4 v = *(const u32x4*)(yr + ch * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float u0 = bf2f((bf16_t)(u[j] & 0xffffu)), u1 = bf2f((bf16_t)(u[j] >> 16));
                const float v0 = bf2f((bf16_t)(v[j] & 0xffffu)), v1 = bf2f((bf16_t)(v[j] >> 16));
                xy = fmaf(u0, v0, xy); xy = fmaf(u1, v1, xy);
                xx = fmaf(u0, u0, xx); xx = fmaf(u1, u1, xx);
                yy = fmaf(v0, v0, yy); yy = fmaf(v1, v1, yy);
            }
        }
        xy = wave_sum(xy);
        xx = wave_sum(xx);
        yy = wave_sum(yy);
        if (lane == 0) out[(int64_t)b * ldo + t] = scale * (xy / (fmaxf(sqrtf(xx), 1e-12f) * fmaxf(sqrtf(yy), 1e-12f)));
    }
}
}  // namespace
}  // namespace leco

using namespace leco;

extern "C" int leco_clip_preprocess(const void* img, int32_t batch, int32_t h, int32_t w, const int32_t* row_tab,
                                    const float* row_w, int32_t row_taps, const int32_t* col_tab, const float* col_w,
                                    int32_t col_taps, const float* mean_std, int32_t image_size, int32_t patch_size, void* out,
                                    int64_t ldo, leco_stream_t stream) {
    if (!img || !row_tab || !row_w || !col_tab || !col_w || !mean_std || !out)
        return fail(-EINVAL, "clip_preprocess: null operand (%s)",
                    !img ? "img" : (!out ? "out" : (!mean_std ? "mean_std" : (!row_tab || !row_w ? "row table" : "column table"))));
    if (batch <= 0 || h <= 0 || w <= 0) return fail(-EINVAL, "clip_preprocess: empty problem batch=%d h=%d w=%d", batch, h, w);
    if (image_size <= 0 || patch_size <= 0 || image_size % patch_size)
        return fail(-EINVAL, "clip_preprocess: image_size=%d must be a positive multiple of patch_size=%d", image_size, patch_size);
    if (patch_size > 1024) return fail(-EINVAL, "clip_preprocess: patch_size=%d exceeds 1024", patch_size);
    if (row_taps <= 0 || col_taps <= 0) return fail(-EINVAL, "clip_preprocess: row_taps=%d / col_taps=%d must be positive", row_taps, col_taps);
    const int g = image_size / patch_size;
    const int kp = (3 * patch_size * patch_size + 63) / 64 * 64;
    if (ldo % 8 || ldo < kp) return fail(-EINVAL, "clip_preprocess: ldo=%lld must be a multiple of 8 and at least %d", (long long)ldo, kp);
    const int64_t rows = (int64_t)batch * g * g;
    if (rows > 0x7fffffff) return fail(-EINVAL, "clip_preprocess: batch=%d x %d patches exceed the grid", batch, g * g);
    PrepArgs a{(const unsigned char*)img, h, w, row_tab, row_w, row_taps, col_tab, col_w, col_taps, mean_std, patch_size, g, kp,
               (bf16_t*)out, ldo};
    hipLaunchKernelGGL(clip_preprocess_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("leco_clip_preprocess");
}

extern "C" int leco_vit_embed(const void* patches, int64_t ldp, const void* cls, const void* pos, int64_t ldpos, void* out,
                              int64_t ldo, int32_t batch, int32_t tokens, int32_t c, leco_stream_t stream) {
    if (!patches || !cls || !pos || !out)
        return fail(-EINVAL, "vit_embed: null operand (%s)", !patches ? "patches" : (!cls ? "cls" : (!pos ? "pos" : "out")));
    if (batch <= 0 || tokens <= 0 || c <= 0) return fail(-EINVAL, "vit_embed: empty problem batch=%d tokens=%d c=%d", batch, tokens, c);
    if (c % 8 || ldp % 8 || ldpos % 8 || ldo % 8 || ldp < c || ldpos < c || ldo < c)
        return fail(-EINVAL, "vit_embed: c=%d and the row strides must be multiples of 8, the strides at least c", c);
    const int64_t total = (int64_t)batch * (tokens + 1) * (c / 8);
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(vit_embed_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)patches, ldp,
                       (const bf16_t*)cls, (const bf16_t*)pos, ldpos, (bf16_t*)out, ldo, batch, tokens, c / 8);
    return check_launch("leco_vit_embed");
}

extern "C" int leco_cosine_scores(const void* x, int64_t ldx, const void* y, int64_t ldy, float* out, int64_t ldo, int32_t nb,
                                  int32_t nt, int32_t d, float scale, leco_stream_t stream) {
    if (!x || !y || !out) return fail(-EINVAL, "cosine_scores: null operand (%s)", !x ? "x" : (!y ? "y" : "out"));
    if (nb <= 0 || nt <= 0 || d <= 0) return fail(-EINVAL, "cosine_scores: empty problem b=%d t=%d d=%d", nb, nt, d);
    if (d % 8 || ldx % 8 || ldy % 8 || ldx < d || ldy < d)
        return fail(-EINVAL, "cosine_scores: d=%d and the row strides must be multiples of 8, the strides at least d", d);
    if (ldo < nt) return fail(-EINVAL, "cosine_scores: ldo=%lld is less than t=%d", (long long)ldo, nt);
    const int64_t pairs = (int64_t)nb * nt;
    if ((pairs + 3) / 4 > 0x7fffffff) return fail(-EINVAL, "cosine_scores: b=%d x t=%d exceed the grid", nb, nt);
    hipLaunchKernelGGL(cosine_scores_kernel, dim3((unsigned)((pairs + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       ldx, (const bf16_t*)y, ldy, out, ldo, nb, nt, d / 8, scale);
    return check_launch("leco_cosine_scores");
}
