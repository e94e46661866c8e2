// The edge convolutions: the 3x3 (pad 1) convolutions at the ends of the UNet and the VAE, too thin to be GEMM-shaped
// (Cin <= 8 or Cout <= 8), and the 1x1 post_quant_conv in front of the decoder.
//   conv_in         NCHW bf16 latents (Cin <= 8) -> channels-last bf16              (UNet, VAE decoder)
//   conv_in_rgb     fp32 NCHW / uint8 NHWC image (3 channels) -> channels-last bf16 (VAE encoder)
//   conv_out        channels-last bf16 -> 4 channels, fp32 NCHW, and its dgrad       (UNet)
//   conv_out_rgb    channels-last bf16 -> 3 channels, fp32 NCHW and / or uint8 NHWC  (VAE decoder)
//   conv_out_moments  channels-last bf16 -> 8 channels + quant_conv + the Gaussian sample (VAE encoder)
//   latent_affine   post_quant_conv with 1 / scaling_factor folded in                (VAE decoder)
// The scalar conv_in / conv_out kernels re-read their weights once per output element (conv_in: 72 16-byte loads per 8
// outputs; conv_out: the whole 23 KB weight set per pixel) and cost 28 us each per UNet pass -- as much as a level-0 3x3
// convolution with 80x the work; they remain for the widths the matrix-core forms do not take.  Both are tiny GEMMs:
//   conv_in : [pixels][Cin * 9 (<= 64)] x [Cin * 9][Cout]   -- weights stationary in REGISTERS (fp32 split into bf16 hi + lo:
//             the result keeps the fp32-weight accuracy of the scalar kernel), a wave owns up to 5 fragments of 16 output
//             channels, the activation fragment is gathered from the NCHW input;
//   conv_out: [pixels][9 C] x [9 C][Cout <= 8 (one 16-row fragment, rows >= Cout zero)] -- K split over the 4 waves of a
//             workgroup, activation and weight fragments straight from global / L2, partial sums meet in LDS
//             (conv_out_sums: ONE loop for the three exits, which differ in what they do with a pixel's Cout sums).
// mfma16(W, X, acc): lane (fr, fg) receives rows n = 4 fg + r of column (pixel) fr.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <leco_prims.h>

#include "common.h"
#include "vec8.h"

namespace leco {
namespace {

// pix -> image b, row py, column px of a [B][H][W] pixel index.  The host keeps B * H * W below 2^30 on every path that
// comes here, so the divisions are 32-bit: a 64-bit one is ~200 instructions.
__device__ __forceinline__ void pixel_coords(int pix, int H, int W, int& b, int& py, int& px) {
    const unsigned row = (unsigned)pix / (unsigned)W;
    px = (int)((unsigned)pix - row * (unsigned)W);
    b = (int)(row / (unsigned)H);
    py = (int)(row - (unsigned)b * (unsigned)H);
}

// two fp32 weights as bf16 pairs {hi, lo}: hi = their roundings, lo = the roundings of what hi lost
__device__ __forceinline__ u32x2 split_hi_lo(float a, float b) {
    const unsigned hi = pack_bf2(a, b);
    return u32x2{hi, pack_bf2(a - bf2f((bf16_t)(hi & 0xffffu)), b - bf2f((bf16_t)(hi >> 16)))};
}

// ---- conv_in: 3x3 pad 1, Cin (<=8) -> Cout, NCHW bf16 in, channels-last bf16 out -------------------
// weights fp32 [Cin][3][3][Cout] (Cout contiguous: 8 adjacent outputs = two float4 loads), bias fp32.
__global__ __launch_bounds__(256) void conv_in_kernel(const bf16_t* x, const float* w, const float* bias,
                                                       bf16_t* y, int B, int H, int W, int Cin, int Cout) {
    const int nv = Cout / 8;
    const int64_t total = (int64_t)B * H * W * nv;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t pix = e / nv;
        const int co = (int)(e - pix * nv) * 8;
        const int px = (int)(pix % W), py = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
        float acc[8];
        {
            f32x4 b0 = *(const f32x4*)(bias + co), b1 = *(const f32x4*)(bias + co + 4);
            acc[0] = b0[0]; acc[1] = b0[1]; acc[2] = b0[2]; acc[3] = b0[3];
            acc[4] = b1[0]; acc[5] = b1[1]; acc[6] = b1[2]; acc[7] = b1[3];
        }
        for (int c = 0; c < Cin; ++c)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int iy = py + tap / 3 - 1, ix = px + tap % 3 - 1;
                if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
                const float xv = bf2f(x[((int64_t)(b * Cin + c) * H + iy) * W + ix]);
                const float* wr = w + (int64_t)(c * 9 + tap) * Cout + co;
                f32x4 w0 = *(const f32x4*)wr, w1 = *(const f32x4*)(wr + 4);
                acc[0] += xv * w0[0]; acc[1] += xv * w0[1]; acc[2] += xv * w0[2]; acc[3] += xv * w0[3];
                acc[4] += xv * w1[0]; acc[5] += xv * w1[1]; acc[6] += xv * w1[2]; acc[7] += xv * w1[3];
            }
        *(u32x4*)(y + pix * Cout + co) = pack8(acc);
    }
}

// ---- conv_out: 3x3 pad 1, C -> Cout (4), channels-last bf16 in, NCHW fp32 out ------------------------
// one wave per output pixel; weights bf16 [Cout][3][3][C]; lanes split C in vectors of 8.
template <int COUT>
__global__ __launch_bounds__(256) void conv_out_kernel(const bf16_t* x, const bf16_t* w, const float* bias,
                                                        float* y, int B, int H, int W, int C) {
    const int lane = lane_id();
    const int64_t pix = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t npix = (int64_t)B * H * W;
    const bool live = pix < npix;
    const int64_t pp = live ? pix : 0;
    const int px = (int)(pp % W), py = (int)((pp / W) % H), b = (int)(pp / ((int64_t)W * H));
    const int nv = C / 8;
    float acc[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) acc[o] = 0.f;
    for (int tap = 0; tap < 9; ++tap) {
        const int iy = py + tap / 3 - 1, ix = px + tap % 3 - 1;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;  // wave-uniform
        const bf16_t* xr = x + ((int64_t)(b * H + iy) * W + ix) * C;
        for (int v = lane; v < nv; v += 64) {
            float xv[8], wv[8];
            unpack8(*(const u32x4*)(xr + v * 8), xv);
#pragma unroll
            for (int o = 0; o < COUT; ++o) {
                unpack8(*(const u32x4*)(w + ((int64_t)(o * 9 + tap)) * C + v * 8), wv);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[o] += xv[i] * wv[i];
            }
        }
    }
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) acc[o] += shfl_xor(acc[o], m);
    }
    if (live && lane == 0) {
#pragma unroll
        for (int o = 0; o < COUT; ++o) y[((int64_t)(b * COUT + o) * H + py) * W + px] = acc[o] + bias[o];
    }
}

// ---- conv_in on the matrix cores ------------------------------------------------------------------------------------
constexpr int CIN_FPW = 5;     // output fragments per wave (Cout <= 4 * 5 * 16)
__global__ __launch_bounds__(256) void conv_in_mfma_kernel(const bf16_t* x, const float* w, const float* bias, bf16_t* y, int B,
                                                            int H, int W, int Cin, int Cout, int groups_per_block) {
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6), fr = lane & 15, fg = lane >> 4;
    const int nf = Cout / 16, fpw = (nf + 3) / 4, f0 = wave * fpw, f1 = min(nf, f0 + fpw);
    const int K = Cin * 9;
    if (f0 >= f1) return;
    // weight fragments: k = 32 ks + 8 fg + i, row n = 16 f + fr
    bf16x8 whi[CIN_FPW][2], wlo[CIN_FPW][2];
    f32x4 bia[CIN_FPW];
#pragma unroll
    for (int q = 0; q < CIN_FPW; ++q) {
        const int f = f0 + q;
        const bool live = f < f1;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 hi = {0u, 0u, 0u, 0u}, lo = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                const int k = 32 * ks + 8 * fg + i;
                const float a = (live && k < K) ? w[(int64_t)k * Cout + 16 * f + fr] : 0.f;
                const float b = (live && k + 1 < K) ? w[(int64_t)(k + 1) * Cout + 16 * f + fr] : 0.f;
                const u32x2 s = split_hi_lo(a, b);
                hi[i >> 1] = s[0];
                lo[i >> 1] = s[1];
            }
            whi[q][ks] = __builtin_bit_cast(bf16x8, hi);
            wlo[q][ks] = __builtin_bit_cast(bf16x8, lo);
        }
        bia[q] = live ? *(const f32x4*)(bias + 16 * f + 4 * fg) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int npix = B * H * W;
    for (int g = 0; g < groups_per_block; ++g) {
        const int pix = ((int)blockIdx.x * groups_per_block + g) * 16 + fr;
        if (((int)blockIdx.x * groups_per_block + g) * 16 >= npix) break;
        const bool pv = pix < npix;
        int b, py, px;
        pixel_coords(pv ? pix : 0, H, W, b, py, px);
        bf16x8 xf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 t = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int k = 32 * ks + 8 * fg + i;
                const int c = k / 9, tap = k - 9 * c;
                const int iy = py + tap / 3 - 1, ix = px + tap % 3 - 1;
                unsigned v = 0u;
                if (pv && k < K && iy >= 0 && iy < H && ix >= 0 && ix < W) v = x[((int64_t)(b * Cin + c) * H + iy) * W + ix];
                t[i >> 1] |= v << ((i & 1) * 16);
            }
            xf[ks] = __builtin_bit_cast(bf16x8, t);
        }
#pragma unroll
        for (int q = 0; q < CIN_FPW; ++q) {
            const int f = f0 + q;
            if (f >= f1) break;
            f32x4 acc = bia[q];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                acc = mfma16(whi[q][ks], xf[ks], acc);
                acc = mfma16(wlo[q][ks], xf[ks], acc);
            }
            if (pv) {
                const u32x2 o = {pack_bf2(acc[0], acc[1]), pack_bf2(acc[2], acc[3])};
                *(u32x2*)(y + (int64_t)pix * Cout + 16 * f + 4 * fg) = o;
            }
        }
    }
}

// ---- conv_out on the matrix cores: the loop of the three exits --------------------------------------------------------
// 16 pixels per workgroup (blockIdx.x), weights bf16 [COUT][3][3][C], C % 32 == 0.  Returns true in the one lane per pixel
// (lane fr of wave 0, pixel inside the image) that goes on to the exit's epilogue, with pix / b / py / px of its pixel and
// v[n] = bias[n] + the sum of output row n.  Row 4 h + r of pixel fr is element r of lane 16 h + fr, and the partial sums
// a0..a3 of the four waves are added as (a0 + a1) + (a2 + a3) + bias[n]: the exits are bit-equal row for row.
template <int COUT>
__device__ __forceinline__ bool conv_out_sums(const bf16_t* x, const bf16_t* w, const float* bias, int B, int H, int W, int C,
                                              int& pix, int& b, int& py, int& px, float (&v)[COUT]) {
    __shared__ f32x4 red[4][64];
    const int lane = lane_id(), wave = uniform((int)(threadIdx.x >> 6)), fr = lane & 15, fg = lane >> 4;
    pix = (int)blockIdx.x * 16 + fr;
    const bool pv = pix < B * H * W;
    pixel_coords(pv ? pix : 0, H, W, b, py, px);
    const int nkc = C / 32;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const u32x4 z = {0u, 0u, 0u, 0u};
    // k-steps are handed out in UNITS of (channel block, kernel row): the three horizontal taps of a unit read the same
    // cache lines, and the three kernel rows of a channel block are in flight on the workgroup's waves together -- the input
    // is fetched from L2 ~once instead of once per tap (9x: 94 MB per launch at level 0, the bound of the first version)
    constexpr int UU = 4;                                  // units (x 3 taps) in flight per wave
    const int nunits = 3 * nkc;
    for (int u0 = wave; u0 < nunits; u0 += 4 * UU) {
        u32x4 xv[UU][3], wv[UU][3];
#pragma unroll
        for (int uu = 0; uu < UU; ++uu) {
            const int unit = u0 + 4 * uu;
            const int cb = unit / 3, ky = unit - 3 * cb;
            const int iy = py + ky - 1;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = px + kx - 1;
                const bool ok = unit < nunits && pv && iy >= 0 && iy < H && ix >= 0 && ix < W;
                xv[uu][kx] = ok ? *(const u32x4*)(x + ((int64_t)(b * H + iy) * W + ix) * C + cb * 32 + fg * 8) : z;
                wv[uu][kx] = (unit < nunits && fr < COUT) ? *(const u32x4*)(w + (int64_t)(fr * 9 + ky * 3 + kx) * C + cb * 32 + fg * 8) : z;
            }
        }
#pragma unroll
        for (int uu = 0; uu < UU; ++uu)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
                acc = mfma16(__builtin_bit_cast(bf16x8, wv[uu][kx]), __builtin_bit_cast(bf16x8, xv[uu][kx]), acc);
    }
    red[wave][lane] = acc;
    __syncthreads();
    if (wave != 0 || fg != 0 || !pv) return false;
#pragma unroll
    for (int h = 0; 4 * h < COUT; ++h) {
        const f32x4 a0 = red[0][16 * h + fr], a1 = red[1][16 * h + fr], a2 = red[2][16 * h + fr], a3 = red[3][16 * h + fr];
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * h + r < COUT) v[4 * h + r] = (a0[r] + a1[r]) + (a2[r] + a3[r]) + bias[4 * h + r];
    }
    return true;
}

// ---- UNet conv_out: fp32 NCHW ------------------------------------------------------------------------------------------
template <int COUT>
__global__ __launch_bounds__(256) void conv_out_mfma_kernel(const bf16_t* x, const bf16_t* w, const float* bias, float* y, int B,
                                                             int H, int W, int C) {
    int pix, b, py, px;
    float v[COUT];
    if (!conv_out_sums<COUT>(x, w, bias, B, H, W, C, pix, b, py, px, v)) return;
#pragma unroll
    for (int n = 0; n < COUT; ++n) y[((int64_t)(b * COUT + n) * H + py) * W + px] = v[n];
}

// ---- VAE decoder entry: post_quant_conv (a 1x1 convolution on the latents) with the 1 / scaling_factor of `decode` folded in:
// y[b][o][p] = bias[o] + sum_c w[o][c] * (in_scale * x[b][c][p]); fp32 NCHW in, bf16 NCHW out (what conv_in reads).
__global__ __launch_bounds__(256) void latent_affine_kernel(const float* x, const float* w, const float* bias, bf16_t* y, int B,
                                                             int HW, int Cin, int Cout, float in_scale) {
    const int64_t total = (int64_t)B * Cout * HW;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t bo = e / HW;
        const int p = (int)(e - bo * HW), o = (int)(bo % Cout), b = (int)(bo / Cout);
        float acc = bias ? bias[o] : 0.f;
        for (int c = 0; c < Cin; ++c) acc += w[o * Cin + c] * (in_scale * x[((int64_t)b * Cin + c) * HW + p]);
        y[e] = f2bf(acc);
    }
}

// ---- VAE decoder conv_out: C -> 3 (RGB) with the image epilogue -------------------------------------------------------
// Outputs, either or both: y fp32 NCHW (batch, 3, h, w) -- the pre-rounding result -- and img uint8 NHWC (batch, h, w, 3) =
// floor(clamp(y / 2 + 0.5, 0, 1) * 255 + 0.5): the denormalisation of the sampling scripts followed by the rounding of an
// 8-bit image writer.
__global__ __launch_bounds__(256) void conv_out_rgb_kernel(const bf16_t* x, const bf16_t* w, const float* bias, float* y,
                                                            unsigned char* img, int B, int H, int W, int C) {
    constexpr int COUT = 3;
    int pix, b, py, px;
    float v[COUT];
    if (!conv_out_sums<COUT>(x, w, bias, B, H, W, C, pix, b, py, px, v)) return;
#pragma unroll
    for (int n = 0; n < COUT; ++n) {
        if (y) y[((int64_t)(b * COUT + n) * H + py) * W + px] = v[n];
        if (img) img[(int64_t)pix * COUT + n] = (unsigned char)floorf(fminf(fmaxf(v[n] * 0.5f + 0.5f, 0.f), 1.f) * 255.f + 0.5f);
    }
}

// ---- VAE encoder conv_in: 3x3 pad 1 from a 3-channel image to channels-last bf16 [batch*h*w][Cout] ------------------------
// The image is fp32 NCHW in [-1, 1] (x) or 8-bit NHWC (img, meaning p / 127.5 - 1).  A [pixels][27] x [27][Cout] GEMM whose
// K fits ONE 32-wide MFMA k-step; the launch writes Cout * 2 bytes per pixel against 3..12 read (67 MB vs 0.8 MB at 512^2), so
// it is laid out for its stores: a wave owns 16 consecutive pixels and every output channel of them -- one contiguous
// 16 * Cout * 2 byte span -- and the weight-row order of a fragment PAIR is permuted (row 4 fg + r of fragment j is channel
// 32 P + 8 fg + 4 j + r) so that a lane ends up with 8 consecutive channels of its pixel: one 16-byte store, the 4 lanes fg of
// a pixel a full 64-byte segment.  Weights stay in registers, fp32 split into bf16 hi + lo (as conv_in_mfma_kernel); the
// image value is split the same way (hi*hi + lo*hi + hi*lo: ~2^-17 relative before the single bf16 rounding).  An 8-bit pixel
// p means the fp32 number (float)p / 127.5f - 1.f -- what `img.float() / 127.5 - 1` gives -- looked up, already split, in a
// 256-entry LDS table, so the two inputs describing one image give the same bits; a padding tap is 0 in that normalised space.
constexpr int RGB_PAIRS = 4;       // 32-channel pairs per pass: blockIdx.y walks Cout in steps of 128
__global__ __launch_bounds__(256) void conv_in_rgb_kernel(const float* x, const unsigned char* img, const float* w,
                                                           const float* bias, bf16_t* y, int B, int H, int W, int Cout,
                                                           int groups_per_wave) {
    constexpr int K = 27;
    __shared__ unsigned lut[256];                // 8-bit path: bf16 hi | lo << 16 of (float)p / 127.5f - 1.f
    if (img) {                                   // (block-uniform)
        const float v = (float)(int)threadIdx.x / 127.5f - 1.f;
        const bf16_t h = f2bf(v);
        lut[threadIdx.x] = (unsigned)h | ((unsigned)f2bf(v - bf2f(h)) << 16);
        __syncthreads();
    }
    const int lane = lane_id(), wave = uniform((int)(threadIdx.x >> 6)), fr = lane & 15, fg = lane >> 4;
    const int p0 = (int)blockIdx.y * RGB_PAIRS;
    const int np = min(RGB_PAIRS, Cout / 32 - p0);
    bf16x8 whi[RGB_PAIRS][2], wlo[RGB_PAIRS][2];
    float bia[RGB_PAIRS][8];
#pragma unroll
    for (int q = 0; q < RGB_PAIRS; ++q) {
        const bool live = q < np;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = 32 * (p0 + q) + 8 * (fr >> 2) + 4 * j + (fr & 3);       // the channel this lane's A row carries
            u32x4 hi = {0u, 0u, 0u, 0u}, lo = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                const int k = 8 * fg + i;
                const float a = (live && k < K) ? w[(int64_t)n * K + k] : 0.f;
                const float b = (live && k + 1 < K) ? w[(int64_t)n * K + k + 1] : 0.f;
                const u32x2 s = split_hi_lo(a, b);
                hi[i >> 1] = s[0];
                lo[i >> 1] = s[1];
            }
            whi[q][j] = __builtin_bit_cast(bf16x8, hi);
            wlo[q][j] = __builtin_bit_cast(bf16x8, lo);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) bia[q][e] = live ? bias[32 * (p0 + q) + 8 * fg + e] : 0.f;
    }
    const int npix = B * H * W;
    for (int g = 0; g < groups_per_wave; ++g) {
        const int group = ((int)blockIdx.x * 4 + wave) * groups_per_wave + g;      // wave-uniform
        if ((int64_t)group * 16 >= npix) break;
        const int pix = group * 16 + fr;
        const bool pv = pix < npix;
        int b, py, px;
        pixel_coords(pv ? pix : 0, H, W, b, py, px);
        u32x4 th = {0u, 0u, 0u, 0u}, tl = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = 8 * fg + i;
            const int c = k / 9, tap = k - 9 * c;
            const int iy = py + tap / 3 - 1, ix = px + tap % 3 - 1;
            unsigned hl = 0u;                    // hi | lo << 16
            if (pv && k < K && iy >= 0 && iy < H && ix >= 0 && ix < W) {
                if (img) {
                    hl = lut[img[((int64_t)(b * H + iy) * W + ix) * 3 + c]];
                } else {
                    const float v = x[((int64_t)(b * 3 + c) * H + iy) * W + ix];
                    const bf16_t h = f2bf(v);
                    hl = (unsigned)h | ((unsigned)f2bf(v - bf2f(h)) << 16);
                }
            }
            th[i >> 1] |= (hl & 0xffffu) << ((i & 1) * 16);
            tl[i >> 1] |= (hl >> 16) << ((i & 1) * 16);
        }
        const bf16x8 xh = __builtin_bit_cast(bf16x8, th), xl = __builtin_bit_cast(bf16x8, tl);
#pragma unroll
        for (int q = 0; q < RGB_PAIRS; ++q) {
            if (q >= np) break;
            float o[8];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                acc = mfma16(wlo[q][j], xh, acc);
                acc = mfma16(whi[q][j], xl, acc);
                acc = mfma16(whi[q][j], xh, acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) o[4 * j + r] = acc[r] + bia[q][4 * j + r];
            }
            if (pv) *(u32x4*)(y + (int64_t)pix * Cout + 32 * (p0 + q) + 8 * fg) = pack8(o);
        }
    }
}

// ---- VAE encoder exit: conv_out (C -> 8) + quant_conv (8 x 8, fp32) + the diagonal-Gaussian sample ---------------------
// One lane per pixel applies quant_conv to the 8 fp32 sums (never folded into the bf16 weights) and writes, either or both:
// moments fp32 NCHW (batch, 8, h, w) = [mean | logvar], and latents fp32 NCHW (batch, 4, h, w) =
// scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise); noise = NULL: scale * mean (the mode).
__global__ __launch_bounds__(256) void conv_out_moments_kernel(const bf16_t* x, const bf16_t* w, const float* bias, const float* qw,
                                                                const float* qb, const float* noise, float* moments,
                                                                float* latents, float scale, int B, int H, int W, int C) {
    constexpr int COUT = 8;
    int pix, b, py, px;
    float v[COUT], m[COUT];
    if (!conv_out_sums<COUT>(x, w, bias, B, H, W, C, pix, b, py, px, v)) return;
#pragma unroll
    for (int o = 0; o < COUT; ++o) {
        float s = qb[o];
#pragma unroll
        for (int i = 0; i < COUT; ++i) s += qw[o * COUT + i] * v[i];
        m[o] = s;
        if (moments) moments[((int64_t)(b * COUT + o) * H + py) * W + px] = s;
    }
    if (latents) {
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const int64_t at = ((int64_t)(b * 4 + ch) * H + py) * W + px;
            float val = m[ch];
            if (noise) val += expf(0.5f * fminf(fmaxf(m[4 + ch], -30.f), 20.f)) * noise[at];
            latents[at] = scale * val;
        }
    }
}

// dgrad of conv_out: dx[pix][c] = sum_{tap,o} dy[b][o][pix - off(tap)] * w[o][tap][c]
template <int COUT>
__global__ __launch_bounds__(256) void conv_out_bwd_kernel(const float* dy, const bf16_t* w, bf16_t* dx, int B,
                                                            int H, int W, int C) {
    const int nv = C / 8;
    const int64_t total = (int64_t)B * H * W * nv;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t pix = e / nv;
        const int c = (int)(e - pix * nv) * 8;
        const int px = (int)(pix % W), py = (int)((pix / W) % H), b = (int)(pix / ((int64_t)W * H));
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int tap = 0; tap < 9; ++tap) {
            // output pixel (oy, ox) used input (py, px) through tap iff oy + kh - 1 = py
            const int oy = py - (tap / 3 - 1), ox = px - (tap % 3 - 1);
            if (oy < 0 || oy >= H || ox < 0 || ox >= W) continue;
#pragma unroll
            for (int o = 0; o < COUT; ++o) {
                const float d = dy[((int64_t)(b * COUT + o) * H + oy) * W + ox];
                float wv[8];
                unpack8(*(const u32x4*)(w + ((int64_t)(o * 9 + tap)) * C + c), wv);
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[i] += d * wv[i];
            }
        }
        *(u32x4*)(dx + pix * C + c) = pack8(acc);
    }
}
}  // namespace
}  // namespace leco

using namespace leco;
#define LECO_STREAM ((hipStream_t)stream)

extern "C" int leco_conv_in(const void* x, const float* w, const float* bias, void* y, int32_t batch, int32_t h,
                            int32_t wd, int32_t cin, int32_t cout, leco_stream_t stream) {
    if (cout % 8) return fail(-EINVAL, "conv_in: Cout=%d %% 8 != 0", cout);
    if (cout % 16 == 0 && cout <= 64 * CIN_FPW && cin * 9 <= 64 && (int64_t)batch * h * wd < (1ll << 30)) {
        const int64_t groups = ((int64_t)batch * h * wd + 15) / 16;
        const int gpb = groups >= 2048 ? 4 : (groups >= 512 ? 2 : 1);       // >= 256 workgroups where the problem has them
        hipLaunchKernelGGL(conv_in_mfma_kernel, dim3((unsigned)((groups + gpb - 1) / gpb)), dim3(256), 0, LECO_STREAM,
                           (const bf16_t*)x, w, bias, (bf16_t*)y, batch, h, wd, cin, cout, gpb);
        return check_launch("leco_conv_in");
    }
    hipLaunchKernelGGL(conv_in_kernel, dim3(grid_for((int64_t)batch * h * wd * cout / 8)), dim3(256), 0, LECO_STREAM,
                       (const bf16_t*)x, w, bias, (bf16_t*)y, batch, h, wd, cin, cout);
    return check_launch("leco_conv_in");
}
extern "C" int leco_conv_out(const void* x, const void* w, const float* bias, float* y, int32_t batch, int32_t h,
                             int32_t wd, int32_t c, int32_t cout, leco_stream_t stream) {
    if (cout != 4 || c % 8) return fail(-EINVAL, "conv_out: needs Cout=4 (got %d), C %% 8 == 0", cout);
    const int64_t npix = (int64_t)batch * h * wd;
    if (c % 32 == 0 && npix < (1ll << 30)) {
        hipLaunchKernelGGL((conv_out_mfma_kernel<4>), dim3((unsigned)((npix + 15) / 16)), dim3(256), 0, LECO_STREAM,
                           (const bf16_t*)x, (const bf16_t*)w, bias, y, batch, h, wd, c);
        return check_launch("leco_conv_out");
    }
    hipLaunchKernelGGL((conv_out_kernel<4>), dim3((unsigned)((npix + 3) / 4)), dim3(256), 0, LECO_STREAM,
                       (const bf16_t*)x, (const bf16_t*)w, bias, y, batch, h, wd, c);
    return check_launch("leco_conv_out");
}
extern "C" int leco_latent_affine(const float* x, const float* w, const float* bias, void* y, int32_t batch, int32_t hw,
                                  int32_t cin, int32_t cout, float in_scale, leco_stream_t stream) {
    if (batch <= 0 || hw <= 0 || cin <= 0 || cout <= 0) return fail(-EINVAL, "latent_affine: empty problem");
    hipLaunchKernelGGL(latent_affine_kernel, dim3(grid_for((int64_t)batch * cout * hw)), dim3(256), 0, LECO_STREAM, x, w, bias,
                       (bf16_t*)y, batch, hw, cin, cout, in_scale);
    return check_launch("leco_latent_affine");
}
extern "C" int leco_conv_out_rgb(const void* x, const void* w, const float* bias, float* y, void* img, int32_t batch, int32_t h,
                                 int32_t wd, int32_t c, leco_stream_t stream) {
    if (c % 32) return fail(-EINVAL, "conv_out_rgb: C=%d %% 32 != 0", c);
    if (!y && !img) return fail(-EINVAL, "conv_out_rgb: neither y nor img given");
    const int64_t npix = (int64_t)batch * h * wd;
    if (batch <= 0 || h <= 0 || wd <= 0 || npix >= (1ll << 30)) return fail(-EINVAL, "conv_out_rgb: batch * h * w out of range");
    hipLaunchKernelGGL(conv_out_rgb_kernel, dim3((unsigned)((npix + 15) / 16)), dim3(256), 0, LECO_STREAM,
                       (const bf16_t*)x, (const bf16_t*)w, bias, y, (unsigned char*)img, batch, h, wd, c);
    return check_launch("leco_conv_out_rgb");
}
extern "C" int leco_conv_in_rgb(const float* x, const void* img, const float* w, const float* bias, void* y, int32_t batch,
                                int32_t h, int32_t wd, int32_t cout, leco_stream_t stream) {
    if (!x && !img) return fail(-EINVAL, "conv_in_rgb: neither x (fp32 NCHW) nor img (uint8 NHWC) given");
    if (x && img) return fail(-EINVAL, "conv_in_rgb: both x and img given; the image comes from exactly one of them");
    if (!w || !bias || !y) return fail(-EINVAL, "conv_in_rgb: null weight / bias / output");
    if (cout <= 0 || cout % 32) return fail(-EINVAL, "conv_in_rgb: Cout=%d %% 32 != 0", cout);
    const int64_t npix = (int64_t)batch * h * wd;
    if (batch <= 0 || h <= 0 || wd <= 0 || npix >= (1ll << 30)) return fail(-EINVAL, "conv_in_rgb: batch * h * w out of range");
    const int64_t groups = (npix + 15) / 16;
    const int gpw = groups >= 16384 ? 4 : (groups >= 4096 ? 2 : 1);       // >= 1024 workgroups where the image has them
    hipLaunchKernelGGL(conv_in_rgb_kernel, dim3((unsigned)((groups + 4 * gpw - 1) / (4 * gpw)), (unsigned)((cout + 127) / 128)),
                       dim3(256), 0, LECO_STREAM, x, (const unsigned char*)img, w, bias, (bf16_t*)y, batch, h, wd, cout, gpw);
    return check_launch("leco_conv_in_rgb");
}
extern "C" int leco_conv_out_moments(const void* x, const void* w, const float* bias, const float* qw, const float* qb,
                                     const float* noise, float* moments, float* latents, float scale, int32_t batch, int32_t h,
                                     int32_t wd, int32_t c, leco_stream_t stream) {
    if (c <= 0 || c % 32) return fail(-EINVAL, "conv_out_moments: C=%d %% 32 != 0", c);
    if (!moments && !latents) return fail(-EINVAL, "conv_out_moments: neither moments nor latents given");
    if (!x || !w || !bias || !qw || !qb) return fail(-EINVAL, "conv_out_moments: null input / weight / bias / quant_conv operand");
    const int64_t npix = (int64_t)batch * h * wd;
    if (batch <= 0 || h <= 0 || wd <= 0 || npix >= (1ll << 30)) return fail(-EINVAL, "conv_out_moments: batch * h * w out of range");
    hipLaunchKernelGGL(conv_out_moments_kernel, dim3((unsigned)((npix + 15) / 16)), dim3(256), 0, LECO_STREAM, (const bf16_t*)x,
                       (const bf16_t*)w, bias, qw, qb, noise, moments, latents, scale, batch, h, wd, c);
    return check_launch("leco_conv_out_moments");
}
extern "C" int leco_conv_out_bwd(const float* dy, const void* w, void* dx, int32_t batch, int32_t h, int32_t wd,
                                 int32_t c, int32_t cout, leco_stream_t stream) {
    if (cout != 4 || c % 8) return fail(-EINVAL, "conv_out_bwd: needs Cout=4, C %% 8 == 0");
    hipLaunchKernelGGL((conv_out_bwd_kernel<4>), dim3(grid_for((int64_t)batch * h * wd * c / 8)), dim3(256), 0,
                       LECO_STREAM, dy, (const bf16_t*)w, (bf16_t*)dx, batch, h, wd, c);
    return check_launch("leco_conv_out_bwd");
}
