// Kernels of the CLIP text encoder that the UNet's kernel set lacks (leco_amd/clip.py):
//   * leco_attention_causal_fwd: O = softmax(Q K^T * scale + causal) V per (batch, head), head dim 64, up to 128 tokens;
//   * leco_embed_rows: row gather (+ periodic add) -- token + position embedding, and the EOS-row gather of the pooled output.
//
// Causal attention on gfx950 (wave64, v_mfma_f32_16x16x32_bf16).  The problem is tiny and latency-bound: two SD1.5 prompts
// are 24 (batch, head) pairs of 77 x 77 scores on 256 CUs.  So the query rows are split over workgroups too:
//   * grid = (ceil(S / 16), heads, batch); one workgroup = ONE wave = 16 query rows [q0, q0 + 16).  S = 77, 12 heads, 2 prompts:
//     120 single-wave workgroups, each with at most two 64-key tiles of work;
//   * the workgroup stages into LDS only the keys / values [0, min(q0 + 16, S)): what lies above its last row is never
//     read, and the key loop ends with the tile that holds the diagonal (tiles above it are skipped, not masked); rows of
//     the last staged tile past that bound are zero-filled so that the PV product meets finite values;
//   * inside the tile on the diagonal every score with key > query row is set to -inf before the softmax (earlier tiles
//     lie wholly below the diagonal: no compare);
//   * arithmetic and lane mapping are those of attn_fwd_kernel (attention.hip): both products swapped (S^T = K Q^T,
//     O^T = V^T P^T) so a lane owns one query row, online softmax in fp32 on exp2 with scale * log2(e) folded in, P stays
//     in registers as bf16, V is read with the hardware transpose read.
// LDS: 128 keys x (72 + 80) bf16 = 38 KB static; K rows padded by 16 bytes (conflict-free ds_read_b128), V row stride an odd
// multiple of 32 bytes (the transpose reads of a half wave cover the banks once).
#include <errno.h>
#include <hip/hip_runtime.h>
#include <leco_prims.h>
#include <math.h>

#include "common.h"

namespace leco {
namespace {

constexpr int CA_D = 64;                       // head dim
constexpr int CA_SMAX = LECO_CAUSAL_ATTN_MAX_S;
constexpr int CA_KT = 64;                      // keys per tile
constexpr int CA_QR = 16;                      // query rows per workgroup
constexpr int CA_KROW = CA_D + 8;              // padded K row (elements)
constexpr int CA_VROW = 80;                    // V row stride (elements): 160 bytes = 5 x 32
static_assert(CA_SMAX % CA_KT == 0, "the LDS image holds whole key tiles");

struct CausalArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v;
    int64_t ldq, ldk, ldv, bsq, bsk, bsv;
    bf16_t* o; int64_t ldo, bso;
    int s;
    float scale_log2;          // scale * log2(e)
};

__global__ __launch_bounds__(64) void attn_causal_kernel(CausalArgs p) {
    constexpr int NKS = CA_D / 32, NFD = CA_D / 16, NDC = CA_D / 8;
    __shared__ __attribute__((aligned(16))) bf16_t sK[CA_SMAX * CA_KROW];
    __shared__ __attribute__((aligned(16))) bf16_t sV[CA_SMAX * CA_VROW];

    const int lane = (int)threadIdx.x & 63;
    const int fr = lane & 15, fg = lane >> 4;
    const int q0 = (int)blockIdx.x * CA_QR, h = (int)blockIdx.y, b = (int)blockIdx.z;
    const int kv_end = q0 + CA_QR < p.s ? q0 + CA_QR : p.s;              // keys this workgroup can see
    const int kv_pad = (kv_end + CA_KT - 1) / CA_KT * CA_KT;              // ... rounded up to whole tiles (<= CA_SMAX)

    const bf16_t* qb = p.q + (int64_t)b * p.bsq + (int64_t)h * CA_D;
    const bf16_t* kb = p.k + (int64_t)b * p.bsk + (int64_t)h * CA_D;
    const bf16_t* vb = p.v + (int64_t)b * p.bsv + (int64_t)h * CA_D;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // stage K / V rows [0, kv_pad): chunk e -> (key = e / 8, 16-byte slot e % 8); four chunks per operand in flight per lane
    for (int e0 = lane; e0 < kv_pad * NDC; e0 += 4 * 64) {
        u32x4 kr[4], vr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = e0 + 64 * i, key = e / NDC, ch = e - key * NDC;
            const bool ok = key < kv_end;
            kr[i] = ok ? *(const u32x4*)(kb + (int64_t)key * p.ldk + ch * 8) : zero4;
            vr[i] = ok ? *(const u32x4*)(vb + (int64_t)key * p.ldv + ch * 8) : zero4;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = e0 + 64 * i, key = e / NDC, ch = e - key * NDC;
            if (key < kv_pad) {
                *(u32x4*)(sK + key * CA_KROW + ch * 8) = kr[i];
                *(u32x4*)(sV + key * CA_VROW + ch * 8) = vr[i];
            }
        }
    }

    // Q fragments (MFMA B operand: col = query row, k = head dim); rows past the sequence are zero and never stored
    const int qrow = q0 + fr;
    bf16x8 qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const u32x4 t = qrow < p.s ? *(const u32x4*)(qb + (int64_t)qrow * p.ldq + (ks * 4 + fg) * 8) : zero4;
        qf[ks] = __builtin_bit_cast(bf16x8, t);
    }
    // the mask bound of this lane's row; a row past the sequence is masked like the last one (its first key stays visible,
    // so its softmax stays finite)
    const int qmask = qrow < p.s ? qrow : p.s - 1;

    f32x4 acc_o[NFD];
#pragma unroll
    for (int fd = 0; fd < NFD; ++fd) acc_o[fd] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    __syncthreads();

    for (int kv0 = 0; kv0 < kv_end; kv0 += CA_KT) {
        const bf16_t* tK = sK + kv0 * CA_KROW;
        const bf16_t* tV = sV + kv0 * CA_VROW;
        // S^T = K Q^T : lane holds S[q = fr][key = kv0 + 16 f + 4 fg + r]
        f32x4 acc_s[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const bf16x8 kf = *(const bf16x8*)(tK + (16 * f + fr) * CA_KROW + (ks * 4 + fg) * 8);
                a = mfma16(kf, qf[ks], a);
            }
            acc_s[f] = a;
        }
        // only the tile that reaches past the first query row of the block holds masked elements (wave-uniform)
        const bool diag = kv0 + CA_KT > q0;
        float mx = -INFINITY;
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (diag) {
                    const int key = kv0 + 16 * f + 4 * fg + r;
                    acc_s[f][r] = key <= qmask ? acc_s[f][r] : -INFINITY;
                }
                mx = fmaxf(mx, acc_s[f][r]);
            }
        mx = rows4_max(mx);      // (every row sees key kv0 <= q0 of each tile it visits: mx is finite)
        const float m_new = fmaxf(m_run, mx * p.scale_log2);     // scale > 0: max and scale commute
        const float alpha = fast_exp2(m_run - m_new);
        m_run = m_new;
        float rs = 0.f;
        u32x4 pw[2];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const float e0 = fast_exp2(fmaf(acc_s[f][0], p.scale_log2, -m_new));
            const float e1 = fast_exp2(fmaf(acc_s[f][1], p.scale_log2, -m_new));
            const float e2 = fast_exp2(fmaf(acc_s[f][2], p.scale_log2, -m_new));
            const float e3 = fast_exp2(fmaf(acc_s[f][3], p.scale_log2, -m_new));
            rs += (e0 + e1) + (e2 + e3);
            pw[f >> 1][(f & 1) * 2] = pack_bf2(e0, e1);
            pw[f >> 1][(f & 1) * 2 + 1] = pack_bf2(e2, e3);
        }
        l_run = l_run * alpha + rs;
        // O^T += V^T P^T.  V^T fragment (MFMA A operand: row = d, k = permuted key): MFMA k index 8 fg + t <-> tile key
        // 16 (2 s + (t >> 2)) + 4 fg + (t & 3), matching the P^T registers.
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) {
            acc_o[fd][0] *= alpha; acc_o[fd][1] *= alpha; acc_o[fd][2] *= alpha; acc_o[fd][3] *= alpha;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16_t* blk = tV + (16 * (2 * s) + 4 * fg + (fr >> 2)) * CA_VROW + 16 * fd + 4 * (fr & 3);
                const u32x2 lo = lds_read_tr16(blk);
                const u32x2 hi = lds_read_tr16(blk + 16 * CA_VROW);
                const u32x4 t = {lo[0], lo[1], hi[0], hi[1]};
                acc_o[fd] = mfma16(__builtin_bit_cast(bf16x8, t), __builtin_bit_cast(bf16x8, pw[s]), acc_o[fd]);
            }
        }
    }

    const float inv = 1.f / rows4_sum(l_run);
    if (qrow < p.s) {
        bf16_t* ob = p.o + (int64_t)b * p.bso + (int64_t)h * CA_D + (int64_t)qrow * p.ldo;
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) {
            const f32x4 o = acc_o[fd];
            const u32x2 w = {pack_bf2(o[0] * inv, o[1] * inv), pack_bf2(o[2] * inv, o[3] * inv)};
            *(u32x2*)(ob + 16 * fd + 4 * fg) = w;
        }
    }
}

// one thread = 8 columns of one output row: 16-byte loads and one 16-byte store
__global__ __launch_bounds__(256) void embed_rows_kernel(const bf16_t* table, int64_t ldt, int rows, const int32_t* idx,
                                                         const bf16_t* pos, int64_t ldp, int period, bf16_t* out, int64_t ldo,
                                                         int n, int c8) {
    const int64_t total = (int64_t)n * c8;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int i = (int)(e / c8), ch = (int)(e - (int64_t)i * c8);
        int r = idx[i];
        r = r < 0 ? 0 : (r >= rows ? rows - 1 : r);       // validated by the caller; never read outside the table
        u32x4 t = *(const u32x4*)(table + (int64_t)r * ldt + ch * 8);
        if (pos) {
            const u32x4 q = *(const u32x4*)(pos + (int64_t)(i % period) * ldp + ch * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float lo = bf2f((bf16_t)(t[j] & 0xffffu)) + bf2f((bf16_t)(q[j] & 0xffffu));
                const float hi = bf2f((bf16_t)(t[j] >> 16)) + bf2f((bf16_t)(q[j] >> 16));
                t[j] = pack_bf2(lo, hi);
            }
        }
        *(u32x4*)(out + (int64_t)i * ldo + ch * 8) = t;
    }
}
}  // namespace
}  // namespace leco

using namespace leco;

extern "C" int leco_attention_causal_fwd(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk, int64_t bsk,
                                         const void* v, int64_t ldv, int64_t bsv, void* o, int64_t ldo, int64_t bso,
                                         int32_t batch, int32_t heads, int32_t s, int32_t head_dim, float scale,
                                         leco_stream_t stream) {
    if (!q || !k || !v || !o)
        return fail(-EINVAL, "causal attention: null operand (%s)", !q ? "q" : (!k ? "k" : (!v ? "v" : "o")));
    if (batch <= 0 || heads <= 0) return fail(-EINVAL, "causal attention: empty problem batch=%d heads=%d", batch, heads);
    if (head_dim != CA_D) return fail(-EINVAL, "causal attention: unsupported head_dim %d (64)", head_dim);
    if (s < 1 || s > CA_SMAX) return fail(-EINVAL, "causal attention: s=%d outside [1, %d]", s, CA_SMAX);
    if (batch > 65535 || heads > 65535) return fail(-EINVAL, "causal attention: batch=%d / heads=%d exceed the grid", batch, heads);
    if ((ldq | ldk | ldv | ldo | bsq | bsk | bsv | bso) % 8)
        return fail(-EINVAL, "causal attention: strides (ldq .. bso) must be multiples of 8 elements");
    if (!(scale > 0.f)) return fail(-EINVAL, "causal attention: scale must be positive");
    CausalArgs a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ldq, ldk, ldv, bsq, bsk, bsv, (bf16_t*)o, ldo, bso, s,
                 scale * 1.4426950408889634f};
    hipLaunchKernelGGL(attn_causal_kernel, dim3(cdiv(s, CA_QR), heads, batch), dim3(64), 0, (hipStream_t)stream, a);
    return check_launch("leco_attention_causal_fwd");
}

extern "C" int leco_embed_rows(const void* table, int64_t ldt, int32_t rows, const int32_t* idx, const void* pos, int64_t ldp,
                               int32_t period, void* out, int64_t ldo, int32_t n, int32_t c, leco_stream_t stream) {
    if (!table || !idx || !out) return fail(-EINVAL, "embed_rows: null operand (%s)", !table ? "table" : (!idx ? "idx" : "out"));
    if (n <= 0 || c <= 0 || rows <= 0) return fail(-EINVAL, "embed_rows: empty problem n=%d c=%d rows=%d", n, c, rows);
    if (c % 8 || ldt % 8 || ldo % 8 || (pos && ldp % 8)) return fail(-EINVAL, "embed_rows: c=%d and the row strides must be multiples of 8", c);
    if (pos && period <= 0) return fail(-EINVAL, "embed_rows: pos needs period > 0 (got %d)", period);
    const int64_t total = (int64_t)n * (c / 8);
    const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(embed_rows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)table, ldt, rows, idx,
                       (const bf16_t*)pos, ldp, period > 0 ? period : 1, (bf16_t*)out, ldo, n, c / 8);
    return check_launch("leco_embed_rows");
}
