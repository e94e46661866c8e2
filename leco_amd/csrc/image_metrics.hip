// Picture against picture on the device (leco_amd/image_metrics.py, `--image_diff`): leco_image_compare gives, per picture of
// a uint8 NHWC batch and a reference picture, the mean SSIM (Wang et al. 2004: per channel, 11 x 11 Gaussian window, biased
// moments, valid region only), the exact sum of squared differences and, optionally, the change map 1 - ssim.
//
// Tiling on gfx950.  A workgroup (256 threads) owns a 32 x 16 tile of the valid region, i.e. the pixels whose windows start
// at rows 16 ty .. 16 ty + 15 and columns 32 tx .. 32 tx + 31 of the picture.  The 26 x 42 patch those windows cover (the tile
// plus its 5-pixel halo on every side) is staged ONCE for both pictures and all three channels as centred levels
// (level - 128, which fits int8) in rows of 44 bytes: 2 x 3 x 26 x 44 = 6,864 B.  Per channel a row pass then forms, for
// every patch row and tile column, the five horizontal moments (a, r, a a, r r, a r) into LDS planes of doubles
// [5][26][32] = 33,280 B -- a thread takes one patch row and four adjacent columns, reads its 14 + 14 levels as four dwords
// per picture and writes 32 contiguous bytes per plane -- and a column pass, in which a thread owns one column and two
// adjacent rows of the tile, reads 12 consecutive doubles per plane (consecutive lanes = consecutive 8-byte words: no bank
// conflict) and evaluates the SSIM of its two pixels.  40,208 B of LDS per workgroup with the reduction scratch: three
// workgroups (12 waves) per CU.
//
// Arithmetic.  The levels and their products are integers; the window is symmetric, so the two levels that share a tap are
// added first (exactly, in int32) and every moment is 6 products per pass.  Both passes and the SSIM formula run in fp64:
// against a float64 statement with float64 taps the only error left is the rounding of the fp32 taps themselves and the one
// rounding of the change map to fp32 ("Image metrics").  The variances are formed from the centred moments (they
// do not depend on the centre), the means get their 128 back for the luminance term.  What is stored is d = (den - num) / den
// with num = (2 ma mr + C1)(2 sar + C2), den = (ma^2 + mr^2 + C1)(saa + srr + C2), formed without contraction: for a == ref
// the three second moments are the same operations on the same integers, num == den bit for bit, d == 0 and the mean SSIM,
// 1 - sum d / count, is exactly 1.
//
// Ownership.  Every change-map element and every picture byte's share of the SSE has one owner: tile (tx, ty) owns the picture
// pixels of its patch that lie in columns [32 tx, 32 tx + 32) -- up to the picture's edge for the last tile of a row -- and
// rows likewise; it adds their squared differences (as integers held in doubles) and writes the zeros of the 5-pixel border
// among them.  Each workgroup leaves its two partial sums in the workspace; a finishing launch adds the partials of a
// picture in a fixed order.  No atomics.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <leco_prims.h>
#include <math.h>

#include "common.h"
#include "reduce_f64.h"

namespace leco {
namespace {

constexpr int IC_WIN = 11, IC_HALO = 5;
constexpr int IC_TW = 32, IC_TH = 16;                                  // tile of the valid region
constexpr int IC_PH = IC_TH + IC_WIN - 1, IC_PW = IC_TW + IC_WIN - 1;  // 26 x 42 patch
constexpr int IC_PROW = 44;                                            // bytes per staged patch row (dword reads of 16 levels)
constexpr double IC_C1 = (0.01 * 255.0) * (0.01 * 255.0), IC_C2 = (0.03 * 255.0) * (0.03 * 255.0);

struct CompareArgs {
    const unsigned char* a;
    const unsigned char* ref;
    int64_t ref_stride;
    int h, w;
    const float* taps;
    float* change;
    double* part;                  // [batch][tiles][2]: sum of 1 - ssim over the tile's valid pixels, SSE of the owned pixels
};

// d = 1 - ssim of one channel from the centred moments; see the head of the file for why it is (den - num) / den
__device__ __forceinline__ double ssim_deficit(double ma, double mr, double eaa, double err, double ear) {
#pragma clang fp contract(off)
    const double saa = eaa - ma * ma, srr = err - mr * mr, sar = ear - ma * mr;
    const double la = ma + 128.0, lr = mr + 128.0;
    const double maa = la * la, mrr = lr * lr, mar = la * lr;
    const double den = ((maa + mrr) + IC_C1) * ((saa + srr) + IC_C2);
    const double num = (2.0 * mar + IC_C1) * (2.0 * sar + IC_C2);
    return (den - num) / den;
}

__global__ __launch_bounds__(256) void image_compare_kernel(CompareArgs p) {
    __shared__ __attribute__((aligned(16))) signed char sPatch[2][3][IC_PH][IC_PROW];
    __shared__ __attribute__((aligned(16))) double sPlane[5][IC_PH][IC_TW];
    __shared__ double red[2][4];

    const int tid = (int)threadIdx.x;
    const int b = (int)blockIdx.z;
    const int x0 = (int)blockIdx.x * IC_TW, y0 = (int)blockIdx.y * IC_TH;      // picture coordinates of the patch
    const bool last_x = blockIdx.x == gridDim.x - 1, last_y = blockIdx.y == gridDim.y - 1;
    const int64_t pic = (int64_t)p.h * p.w * 3;
    const unsigned char* pa = p.a + (int64_t)b * pic;
    const unsigned char* pr = p.ref + (int64_t)b * p.ref_stride;

    double w[6];                                                               // the window is symmetric: taps 0..5
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = (double)p.taps[k];

    // ---- stage the patch of both pictures (centred, zeros outside the picture), the SSE and the border of the change map ----
    double sse = 0.0;
    for (int e = tid; e < IC_PH * IC_PROW * 3; e += 256) {
        const int py = e / (IC_PROW * 3), i = e - py * (IC_PROW * 3);
        const int px = i / 3, c = i - px * 3;
        const int Y = y0 + py, X = x0 + px;
        const bool in = px < IC_PW && Y < p.h && X < p.w;
        int va = 0, vr = 0;
        if (in) {
            const int64_t at = ((int64_t)Y * p.w + X) * 3 + c;
            va = (int)pa[at] - 128;
            vr = (int)pr[at] - 128;
            if ((px < IC_TW || last_x) && (py < IC_TH || last_y)) {             // this tile owns the pixel
                const int d = va - vr;
                sse += (double)(d * d);
                if (c == 0 && p.change && (Y < IC_HALO || Y >= p.h - IC_HALO || X < IC_HALO || X >= p.w - IC_HALO))
                    p.change[((int64_t)b * p.h + Y) * p.w + X] = 0.f;
            }
        }
        sPatch[0][c][py][px] = (signed char)va;
        sPatch[1][c][py][px] = (signed char)vr;
    }
    __syncthreads();

    const int rrow = tid >> 3, rcol = (tid & 7) * 4;                           // row pass: patch row, first of four columns
    const int cx = tid & 31, cy = (tid >> 5) * 2;                              // column pass: tile column, first of two rows
    double def0 = 0.0, def1 = 0.0;                                             // sum over the channels of 1 - ssim

    for (int c = 0; c < 3; ++c) {
        if (rrow < IC_PH) {
            int la[16], lr[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const unsigned ua = *(const unsigned*)&sPatch[0][c][rrow][rcol + 4 * q];
                const unsigned ur = *(const unsigned*)&sPatch[1][c][rrow][rcol + 4 * q];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    la[4 * q + t] = (int)(signed char)(ua >> (8 * t));
                    lr[4 * q + t] = (int)(signed char)(ur >> (8 * t));
                }
            }
            double o[5][4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ac = la[j + 5], rc = lr[j + 5];
                double m0 = w[5] * (double)ac, m1 = w[5] * (double)rc, m2 = w[5] * (double)(ac * ac), m3 = w[5] * (double)(rc * rc),
                       m4 = w[5] * (double)(ac * rc);
#pragma unroll
                for (int k = 0; k < 5; ++k) {
                    const int a0 = la[j + k], a1 = la[j + 10 - k], r0 = lr[j + k], r1 = lr[j + 10 - k];
                    m0 = fma(w[k], (double)(a0 + a1), m0);
                    m1 = fma(w[k], (double)(r0 + r1), m1);
                    m2 = fma(w[k], (double)(a0 * a0 + a1 * a1), m2);
                    m3 = fma(w[k], (double)(r0 * r0 + r1 * r1), m3);
                    m4 = fma(w[k], (double)(a0 * r0 + a1 * r1), m4);
                }
                o[0][j] = m0, o[1][j] = m1, o[2][j] = m2, o[3][j] = m3, o[4][j] = m4;
            }
#pragma unroll
            for (int q = 0; q < 5; ++q)
#pragma unroll
                for (int j = 0; j < 4; ++j) sPlane[q][rrow][rcol + j] = o[q][j];
        }
        __syncthreads();

        double m[5][2];
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            double v[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) v[k] = sPlane[q][cy + k][cx];
            double s0 = w[5] * v[5], s1 = w[5] * v[6];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                s0 = fma(w[k], v[k] + v[10 - k], s0);
                s1 = fma(w[k], v[k + 1] + v[11 - k], s1);
            }
            m[q][0] = s0, m[q][1] = s1;
        }
        def0 += ssim_deficit(m[0][0], m[1][0], m[2][0], m[3][0], m[4][0]);
        def1 += ssim_deficit(m[0][1], m[1][1], m[2][1], m[3][1], m[4][1]);
        __syncthreads();                                                       // the planes are free for the next channel
    }

    // ---- the two pixels of this thread: the change map and the tile's sum ----
    const int X = x0 + cx, Y = y0 + cy;                                        // window origin = valid-region coordinates
    const bool xin = X < p.w - (IC_WIN - 1);
    const bool in0 = xin && Y < p.h - (IC_WIN - 1), in1 = xin && Y + 1 < p.h - (IC_WIN - 1);
    const double d0 = def0 / 3.0, d1 = def1 / 3.0;
    if (p.change) {
        float* o = p.change + ((int64_t)b * p.h + Y + IC_HALO) * p.w + X + IC_HALO;
        if (in0) o[0] = (float)d0;
        if (in1) o[p.w] = (float)d1;
    }
    double dsum = (in0 ? d0 : 0.0) + (in1 ? d1 : 0.0);
    block_sum_f64(dsum, sse, red);
    if (tid == 0) {
        const int64_t tile = ((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        p.part[2 * tile] = dsum;
        p.part[2 * tile + 1] = sse;
    }
}

// stats[b] = (1 - sum of the tiles' deficits / valid pixels, sum of the tiles' SSE): thread t adds tiles t, t + 256, ...
__global__ __launch_bounds__(256) void image_compare_finish_kernel(const double* part, int tiles, double valid, double* stats) {
    __shared__ double red[2][4];
    const int b = (int)blockIdx.x;
    double ds = 0.0, se = 0.0;
    for (int t = (int)threadIdx.x; t < tiles; t += 256) {
        ds += part[2 * ((int64_t)b * tiles + t)];
        se += part[2 * ((int64_t)b * tiles + t) + 1];
    }
    block_sum_f64(ds, se, red);
    if (threadIdx.x == 0) {
        stats[2 * b] = 1.0 - ds / valid;
        stats[2 * b + 1] = se;
    }
}

inline int64_t compare_tiles(int h, int w) { return (int64_t)cdiv(h - (IC_WIN - 1), IC_TH) * cdiv(w - (IC_WIN - 1), IC_TW); }

}  // namespace
}  // namespace leco

using namespace leco;

extern "C" int64_t leco_image_compare_workspace(int32_t batch, int32_t h, int32_t w) {
    if (batch < 1 || h < IC_WIN || w < IC_WIN) return 0;
    return (int64_t)batch * compare_tiles(h, w) * 2 * (int64_t)sizeof(double);
}

extern "C" int leco_image_compare(const void* a, const void* ref, int64_t ref_stride, int32_t batch, int32_t h, int32_t w,
                                  const float* taps, float* change_map, double* stats, void* workspace, int64_t workspace_bytes,
                                  leco_stream_t stream) {
    if (!a || !ref || !taps || !stats || !workspace)
        return fail(-EINVAL, "image_compare: null operand (%s)",
                    !a ? "a" : (!ref ? "ref" : (!taps ? "taps" : (!stats ? "stats" : "workspace"))));
    if (batch < 1 || batch > 65535) return fail(-EINVAL, "image_compare: batch=%d must be in 1..65535", batch);
    if (h < IC_WIN || w < IC_WIN)
        return fail(-EINVAL, "image_compare: picture of %d x %d (h=%d w=%d) is smaller than the %d x %d window", h, w, h, w, IC_WIN, IC_WIN);
    const int64_t pic = (int64_t)h * w * 3;
    if (ref_stride != 0 && ref_stride != pic)
        return fail(-EINVAL, "image_compare: ref_stride=%lld must be 0 (one baseline) or h * w * 3 = %lld (pairwise)",
                    (long long)ref_stride, (long long)pic);
    const int gx = cdiv(w - (IC_WIN - 1), IC_TW), gy = cdiv(h - (IC_WIN - 1), IC_TH);
    if (gy > 65535 || (int64_t)gx * gy > 0x7fffffff) return fail(-EINVAL, "image_compare: picture of %d x %d exceeds the grid", h, w);
    const int64_t need = leco_image_compare_workspace(batch, h, w);
    if (workspace_bytes < need || ((uintptr_t)workspace & 7))
        return fail(-EINVAL, "image_compare: workspace of %lld bytes at %p, %lld bytes aligned to 8 are needed (workspace_bytes=%lld)",
                    (long long)workspace_bytes, workspace, (long long)need, (long long)workspace_bytes);
    CompareArgs p{(const unsigned char*)a, (const unsigned char*)ref, ref_stride, h, w, taps, change_map, (double*)workspace};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(image_compare_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)batch), dim3(256), 0, s, p);
    const int rc = check_launch("leco_image_compare");
    if (rc) return rc;
    hipLaunchKernelGGL(image_compare_finish_kernel, dim3((unsigned)batch), dim3(256), 0, s, (const double*)workspace, gx * gy,
                       (double)(h - (IC_WIN - 1)) * (double)(w - (IC_WIN - 1)), stats);
    return check_launch("leco_image_compare");
}
