// Flash-style attention forward for the UNet's self- and cross-attention:
//   O = softmax(Q K^T * scale) V  per (batch, head), never materialising the score matrix.
// Head dims 32/40/64/80/160 (SD1.x: 40/80/160, SD2.x/SDXL: 64), key counts 77 .. 9216; forward only: 128 / 512 (the VAE
// decoder's single wide head, attn_fwd_wide_kernel below).
//
// gfx950 mapping (wave64, v_mfma_f32_16x16x32_bf16):
//   * one workgroup = 4 waves = QF*64 query rows of one (b, head); K/V stream through LDS in
//     64-key tiles shared by the 4 waves (K row-major with a 16-byte row pad => conflict-free
//     ds_read_b128; V transposed on the way in so the PV operand is two ds_read_b64);
//   * both products are issued "swapped" -- S^T = K Q^T and O^T = V^T P^T -- so that every
//     lane owns ONE query row (col = lane & 15): the online-softmax state (running max, sum)
//     is one scalar per lane, the row max needs only two xor-shuffles (lanes l, l^16, l^32,
//     l^48 hold the same row), and P never leaves registers: with the key order of a tile
//     permuted consistently on the V side, the S^T accumulator registers ARE the P^T operand;
//   * exp2 with scale*log2(e) folded in; fp32 running statistics; bf16 P for the PV MFMA;
//   * epilogue: lane holds 4 consecutive d of its row => 8-byte stores; LSE saved for backward.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <leco_prims.h>
#include <math.h>
#include <stdlib.h>
#include <type_traits>

#include "common.h"

namespace leco {
namespace {

struct AttnArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v;
    int64_t ldq, ldk, ldv;     // token strides (elements)
    int64_t bsq, bsk, bsv;     // batch strides (elements)
    bf16_t* o; int64_t ldo, bso;
    float* lse;                // [B][H][Sq] natural-log sum-exp of the scaled scores
    int heads, sq, skv;
    float scale_log2;          // scale * log2(e)
    int xcd_remap;             // 1: walk the (tile, head, sample) grid XCD-contiguously (attn_ids)
};

constexpr int KT = 64;  // keys per tile

// Workgroup -> (tile along the sequence, head, sample).  The hardware places linear workgroup id L on XCD L % 8 (private
// 4 MB L2 each).  With the plain (x = tile, y = head, z = sample) decoding the tiles of one (sample, head) are spread over
// all eight XCDs, so every XCD pulls the K and V of EVERY head through its own L2: 8 x the fill traffic (335 MB instead of
// 42 MB per level-0 self-attention launch at UNet batch 4).  Round 6: each XCD gets a contiguous run of (sample, head)
// pairs with all of their tiles -- the K / V of its 4 heads (2.6 MB) stay in its L2.  LECO_ATTN_XCD=0: the plain decoding.
__device__ __forceinline__ void attn_ids(int remap, int& xi, int& h, int& b) {
    const int nx = (int)gridDim.x, H = (int)gridDim.y, items = nx * H * (int)gridDim.z;
    int item = (int)blockIdx.x + nx * ((int)blockIdx.y + H * (int)blockIdx.z);
    if (remap && (items & 7) == 0) item = (item & 7) * (items >> 3) + (item >> 3);
    const int hb = item / nx;
    xi = item - hb * nx;
    b = hb / H;
    h = hb - b * H;
}
inline int attn_xcd_default() {
    static const int v = [] { const char* e = getenv("LECO_ATTN_XCD"); return e ? atoi(e) : 1; }();
    return v;
}

// Tuning aid (tools/ablate_attn.py): 1 = no exp2, 2 = no K/V staging, 3 = no PV MFMA, 4 = no QK MFMA.
#ifndef LECO_ATTN_ABLATE
#define LECO_ATTN_ABLATE 0
#endif
// occupancy floor (waves per SIMD) of the d <= 40 forward kernels: 4 caps the kernel at 128 VGPRs (it needs 132 without
// the cap); tools/ablate_attn.py occN times the alternatives
#ifndef LECO_ATTN_OCC40
#define LECO_ATTN_OCC40 4
#endif
#ifndef LECO_ATTN_OCC64    // d = 64 (SD2.x / SDXL): 3 caps the kernel at 168 VGPRs (182 without); d = 80 would spill at 3
#define LECO_ATTN_OCC64 3
#endif
// MASKED: the key count is not a multiple of the 64-key tile (cross-attention, 77 keys): every tile applies the key
// bound.  Self-attention (4096 / 1024 / 256 keys) runs the instantiation without a single compare or select.
// The softmax is VALU-bound here (per 64-key x 32-query wave tile: 28 MFMAs = 448 cycles, but 34 quarter-rate v_exp +
// ~190 other VALU instructions), so every instruction that is not needed is removed:
//   * the scale rides in the fma in front of exp2: e = exp2(s * scale - m); the row max is taken on the raw scores and
//     scaled once (scale > 0);
//   * ONES (head dims whose padded width has a spare column, d = 40 -> 48): the spare V column holds 1.0, so the PV
//     MFMA accumulates the softmax row sum l = sum P next to O -- no VALU adds, and l is rescaled with O for free.
template <int D, int QF, bool MASKED>
__global__ __launch_bounds__(256) LECO_MIN_WAVES_PER_SIMD(D <= 40 ? LECO_ATTN_OCC40 : (D == 64 ? LECO_ATTN_OCC64 : (D <= 80 ? 2 : 1))) void attn_fwd_kernel(AttnArgs p) {
    constexpr int DK = (D + 31) / 32 * 32, DV = (D + 15) / 16 * 16;
    constexpr bool ONES = DV > D;
    constexpr int NKS = DK / 32, NFD = DV / 16, NDC = D / 8;
    constexpr int KROW = DK + 8;   // padded K row (elements)
    // V stays ROW-major in LDS ([key][d], staged with the same 16-byte stores as K); the PV operand
    // (8 consecutive keys of one channel per lane) is gathered by the hardware transpose read
    // ds_read_b64_tr_b16.  Row stride = an odd multiple of 32 bytes, so the eight 32-byte row segments a
    // 32-lane half reads land on disjoint banks.
    constexpr int VRB0 = (DV * 2 + 31) / 32 * 32, VRB = ((VRB0 / 32) % 2) ? VRB0 : VRB0 + 32;
    constexpr int VROW = VRB / 2;  // V row stride (elements)
    constexpr int BUF = KT * KROW + KT * VROW;
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * BUF];   // two K|V tile buffers: one barrier per tile

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    int bx, h, b;
    attn_ids(p.xcd_remap, bx, h, b);
    const int q0 = bx * (64 * QF) + wave * (16 * QF);

    const bf16_t* qb = p.q + (int64_t)b * p.bsq + (int64_t)h * D;
    const bf16_t* kb = p.k + (int64_t)b * p.bsk + (int64_t)h * D;
    const bf16_t* vb = p.v + (int64_t)b * p.bsv + (int64_t)h * D;

    // Q fragments (MFMA B operand: col = query row, k = head-dim)
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    bf16x8 qf[QF][NKS];
#pragma unroll
    for (int u = 0; u < QF; ++u) {
        const int qrow = q0 + u * 16 + fr;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int ch = ks * 4 + fg;
            u32x4 t = (qrow < p.sq && ch < NDC) ? *(const u32x4*)(qb + (int64_t)qrow * p.ldq + ch * 8) : zero4;
            qf[u][ks] = __builtin_bit_cast(bf16x8, t);
        }
    }

    f32x4 acc_o[QF][NFD];
    float m_run[QF], l_run[QF];
#pragma unroll
    for (int u = 0; u < QF; ++u) {
        m_run[u] = -INFINITY;
        l_run[u] = 0.f;
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) acc_o[u][fd] = f32x4{0.f, 0.f, 0.f, 0.f};
    }

    // K/V tiles are register-staged one tile ahead: the global loads of tile t+1 are issued before the
    // MFMAs of tile t and written into the OTHER LDS buffer after them (latency hidden behind compute, one
    // barrier per tile).  K and V chunks: thread e -> (key = e / NDC, ch = e % NDC): coalesced rows, one
    // 16-byte LDS store each.
    constexpr int NLD = (KT * NDC + 255) / 256;   // 16-byte chunks per thread per operand
    u32x4 kreg[NLD], vreg[NLD];
    auto fetch = [&](int kv0) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + 256 * i;
            const int key = e / NDC, ch = e - key * NDC;
            const bool ok = e < KT * NDC && kv0 + key < p.skv;
            kreg[i] = ok ? *(const u32x4*)(kb + (int64_t)(kv0 + key) * p.ldk + ch * 8) : zero4;
            vreg[i] = ok ? *(const u32x4*)(vb + (int64_t)(kv0 + key) * p.ldv + ch * 8) : zero4;
        }
    };
    auto stash = [&](int buf) {   // staged registers -> LDS buffer `buf`
        bf16_t* dK = smem + buf * BUF;
        bf16_t* dV = dK + KT * KROW;
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int e = tid + 256 * i;
            if (e < KT * NDC && LECO_ATTN_ABLATE != 2) {
                const int key = e / NDC, ch = e - key * NDC;
                *(u32x4*)(dK + key * KROW + ch * 8) = kreg[i];
                *(u32x4*)(dV + key * VROW + ch * 8) = vreg[i];
            }
        }
    };
    // zero the K columns [D, DK) and V columns [D, DV) of both buffers once (the staged chunks cover [0, D))
    if constexpr (DK / 8 > NDC) {
        constexpr int PADC = DK / 8 - NDC;   // zero chunks per key
        for (int e = tid; e < 2 * KT * PADC; e += 256) {
            const int buf = e / (KT * PADC), r = e - buf * (KT * PADC);
            const int key = r / PADC, ch = NDC + r % PADC;
            *(u32x4*)(smem + buf * BUF + key * KROW + ch * 8) = zero4;
        }
    }
    if (DV > D) {   // V columns [D, DV): column D = 1.0 (the row-sum column), the rest 0
        const u32x4 one_then_zero = {0x00003f80u, 0u, 0u, 0u};
        for (int e = tid; e < 2 * KT; e += 256) {
            const int buf = e / KT, key = e - buf * KT;
            *(u32x4*)(smem + buf * BUF + KT * KROW + key * VROW + NDC * 8) = one_then_zero;
        }
    }
    fetch(0);
    stash(0);
    __syncthreads();
    for (int kv0 = 0, tile = 0; kv0 < p.skv; kv0 += KT, ++tile) {
        const bf16_t* sK = smem + (tile & 1) * BUF;
        const bf16_t* sV = sK + KT * KROW;
        const bool more = kv0 + KT < p.skv;
        if (more && LECO_ATTN_ABLATE != 2) fetch(kv0 + KT);

        // S^T = K Q^T : lane holds S[q = fr][key = kv0 + 16 f + 4 fg + r]
        f32x4 acc_s[QF][4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            bf16x8 kf[NKS];
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks)
                kf[ks] = *(const bf16x8*)(sK + (16 * f + fr) * KROW + (ks * 4 + fg) * 8);
#pragma unroll
            for (int u = 0; u < QF; ++u) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) {
                    if (LECO_ATTN_ABLATE != 4) a = mfma16(kf[ks], qf[u][ks], a);
                    else a[0] += __uint_as_float((unsigned)(kf[ks][0] ^ qf[u][ks][0]));
                }
                acc_s[u][f] = a;
            }
        }

        // online softmax per owned query row on the RAW scores; P^T operand built in registers
        u32x4 pw[QF][2];
        float alpha[QF];
#pragma unroll
        for (int u = 0; u < QF; ++u) {
            float mx = -INFINITY;
#pragma unroll
            for (int f = 0; f < 4; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (MASKED) {
                        const int key = kv0 + 16 * f + 4 * fg + r;
                        acc_s[u][f][r] = key < p.skv ? acc_s[u][f][r] : -INFINITY;
                    }
                    mx = fmaxf(mx, acc_s[u][f][r]);
                }
            mx = rows4_max(mx);
            const float m_new = fmaxf(m_run[u], mx * p.scale_log2);     // scale > 0: max and scale commute
            alpha[u] = fast_exp2(m_run[u] - m_new);
            m_run[u] = m_new;
            float rs = 0.f;
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                float e0, e1, e2, e3;
                if (LECO_ATTN_ABLATE != 1) {
                    e0 = fast_exp2(fmaf(acc_s[u][f][0], p.scale_log2, -m_new));
                    e1 = fast_exp2(fmaf(acc_s[u][f][1], p.scale_log2, -m_new));
                    e2 = fast_exp2(fmaf(acc_s[u][f][2], p.scale_log2, -m_new));
                    e3 = fast_exp2(fmaf(acc_s[u][f][3], p.scale_log2, -m_new));
                } else {
                    e0 = acc_s[u][f][0] - m_new; e1 = acc_s[u][f][1] - m_new;
                    e2 = acc_s[u][f][2] - m_new; e3 = acc_s[u][f][3] - m_new;
                }
                if (!ONES) rs += (e0 + e1) + (e2 + e3);
                pw[u][f >> 1][(f & 1) * 2] = pack_bf2(e0, e1);
                pw[u][f >> 1][(f & 1) * 2 + 1] = pack_bf2(e2, e3);
            }
            if (!ONES) l_run[u] = l_run[u] * alpha[u] + rs;
        }

        // O^T += V^T P^T.  V^T fragment (MFMA A operand: row = d, k = permuted key): MFMA k index
        // 8*fg + t  <->  tile key 16*(2s + (t>>2)) + 4*fg + (t&3), matching the P^T registers.
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) {
#pragma unroll
            for (int u = 0; u < QF; ++u) {
                acc_o[u][fd][0] *= alpha[u]; acc_o[u][fd][1] *= alpha[u];
                acc_o[u][fd][2] *= alpha[u]; acc_o[u][fd][3] *= alpha[u];
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                // 16-lane group fg gathers the [4 keys][16 d] blocks of keys 16 (2s + h) + 4 fg .. + 3: lane i
                // of the group addresses row i / 4, columns 4 (i % 4) .. + 3 and receives column i (4 keys)
                const bf16_t* blk = sV + (16 * (2 * s) + 4 * fg + (fr >> 2)) * VROW + 16 * fd + 4 * (fr & 3);
                const u32x2 lo = lds_read_tr16(blk);
                const u32x2 hi = lds_read_tr16(blk + 16 * VROW);
                u32x4 t = {lo[0], lo[1], hi[0], hi[1]};
                const bf16x8 vf = __builtin_bit_cast(bf16x8, t);
#pragma unroll
                for (int u = 0; u < QF; ++u) {
                    if (LECO_ATTN_ABLATE != 3) acc_o[u][fd] = mfma16(vf, __builtin_bit_cast(bf16x8, pw[u][s]), acc_o[u][fd]);
                    else acc_o[u][fd][0] += __uint_as_float((unsigned)vf[0] ^ pw[u][s][0]);
                }
            }
        }
        if (more) stash((tile + 1) & 1);
        __syncthreads();
    }

    bf16_t* ob = p.o + (int64_t)b * p.bso + (int64_t)h * D;
#pragma unroll
    for (int u = 0; u < QF; ++u) {
        float l;
        if (ONES) {   // column D of O^T: fragment D / 16, lanes fg = (D % 16) / 4, element D % 4
            l = shfl(acc_o[u][D / 16][D % 4], fr + 16 * ((D % 16) / 4));
        } else {
            l = l_run[u];
            l = rows4_sum(l);
        }
        const float inv = 1.f / l;
        const int qrow = q0 + u * 16 + fr;
        if (qrow < p.sq) {
#pragma unroll
            for (int fd = 0; fd < NFD; ++fd) {
                const int d = 16 * fd + 4 * fg;
                if (d < D) {
                    f32x4 o = acc_o[u][fd];
                    u32x2 w = {pack_bf2(o[0] * inv, o[1] * inv), pack_bf2(o[2] * inv, o[3] * inv)};
                    *(u32x2*)(ob + (int64_t)qrow * p.ldo + d) = w;
                }
            }
            if (fg == 0 && p.lse)
                p.lse[((int64_t)b * p.heads + h) * p.sq + qrow] = (m_run[u] + log2f(l)) * 0.6931471805599453f;
        }
    }
}


// ------------------------------------------------------------------------------------------
// Self-attention forward with the K / V tiles brought in by LDS-DMA (round 4).  Same mapping and arithmetic as
// attn_fwd_kernel<D, QF, false> (swapped products, one query row per lane, P in registers); what changes is the staging:
// tools/ablate_attn.py measured the register-staged path (4 global loads + 4 ds_write_b128 per thread and tile, written
// in the shadow of the PV MFMAs, one tile ahead) at 40 of 174 us on the level-0 problem.  Here
//   * a tile is KS + VS wave-wide `buffer_load ... lds` pieces (KS / VS = 16-byte slots per K / V row), three per wave, into
//     a 3-deep ring: the DMA of tile t + 2 is issued right behind the barrier that opens tile t, so a landing has two
//     tiles of compute to hide under and the barrier never waits for memory;
//   * the LDS image of a DMA is lane-linear, so the rows are DENSE: K row = KS slots (KS odd: the 16 rows of a fragment
//     read start in 16 different bank groups), V row = VS slots (VS / 2 odd: the transpose reads of a half wave cover the
//     64 banks once); slots past the head dim are out-of-range lanes of the descriptor (zeros, no traffic; the ring is
//     also zeroed once);
//   * K fragment reads beyond the head dim (d = 40: k-step 1, lane groups 1..3) re-read the row's last slot: Q is zero
//     there, the product does not depend on it;
//   * the softmax row sum comes from one extra MFMA per P operand against an all-ones fragment (the ones COLUMN of the
//     register-staged kernel cannot be DMA'd);
//   * every LDS read is inline asm (ds_read_b128 / ds_read_b64_tr_b16 with immediate offsets): with LDS-DMA in flight the
//     compiler would otherwise drain vmcnt in front of each of them.
// Requirements (else the register-staged kernel runs): skv % 64 == 0, sq % (64 QF) == 0; built for d = 40 / 64 / 80.
template <int D, int NBUF>
struct AttnDmaCfg {
    static constexpr int NDC = D / 8, KS = NDC | 1;
    static constexpr int DV = (D + 15) / 16 * 16, VS0 = DV / 8, VS = ((VS0 / 2) % 2) ? VS0 : VS0 + 2;
    static constexpr int KB = KT * KS * 16, VB = KT * VS * 16, TILE = KB + VB;
    static constexpr int NP = KS + VS, PPW = (NP + 3) / 4;
    static constexpr int OFF_DUMP = NBUF * TILE, LDS_BYTES = OFF_DUMP + 1024;
};
// completes all but the n youngest LDS operations; n is a compile-time constant after unrolling (lgkmcnt holds 0..15)
__device__ __forceinline__ void lds_wait_n(int n) {
    switch (n < 15 ? n : 15) {
        case 0: lds_wait<0>(); break;
        case 1: lds_wait<1>(); break;
        case 2: lds_wait<2>(); break;
        case 3: lds_wait<3>(); break;
        case 4: lds_wait<4>(); break;
        case 5: lds_wait<5>(); break;
        case 6: lds_wait<6>(); break;
        case 7: lds_wait<7>(); break;
        case 8: lds_wait<8>(); break;
        case 9: lds_wait<9>(); break;
        case 10: lds_wait<10>(); break;
        case 11: lds_wait<11>(); break;
        case 12: lds_wait<12>(); break;
        case 13: lds_wait<13>(); break;
        case 14: lds_wait<14>(); break;
        default: lds_wait<15>(); break;
    }
}
// NBUF: depth of the K / V ring (3 where the LDS budget of the occupancy target allows: d = 40 at 4 workgroups per CU, d = 80
// at 2; d = 64 runs 3 workgroups per CU on a 2-deep ring)
template <int D, int QF, int NBUF>
__global__ __launch_bounds__(256) LECO_MIN_WAVES_PER_SIMD(D <= 40 ? LECO_ATTN_OCC40 : (D == 64 ? LECO_ATTN_OCC64 : 2)) void attn_fwd_dma_kernel(AttnArgs p) {
    using Cf = AttnDmaCfg<D, NBUF>;
    constexpr int DK = (D + 31) / 32 * 32, DV = Cf::DV;
    constexpr int NKS = DK / 32, NFD = DV / 16, NDC = Cf::NDC, KS = Cf::KS, VS = Cf::VS, PPW = Cf::PPW;
    constexpr int KB = Cf::KB, TILE = Cf::TILE;
    static_assert(NFD <= 10 && NKS <= 5, "fragment dispatch tables");
    unsigned char* lds = dyn_lds();

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const int fr = lane & 15, fg = lane >> 4;
    int bx, h, b;
    attn_ids(p.xcd_remap, bx, h, b);
    const int q0 = bx * (64 * QF) + wave * (16 * QF);
    const bf16_t* qb = p.q + (int64_t)b * p.bsq + (int64_t)h * D;
    const bf16_t* kb = p.k + (int64_t)b * p.bsk + (int64_t)h * D;
    const bf16_t* vb = p.v + (int64_t)b * p.bsv + (int64_t)h * D;

    // zero the ring once (slots no DMA lane ever fills must not hold NaN patterns), then the Q fragments
    for (int e = tid; e < Cf::LDS_BYTES / 16; e += 256) *(u32x4*)(lds + e * 16) = u32x4{0u, 0u, 0u, 0u};
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    bf16x8 qf[QF][NKS];
#pragma unroll
    for (int u = 0; u < QF; ++u) {
        const int qrow = q0 + u * 16 + fr;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const int ch = ks * 4 + fg;
            u32x4 t = ch < NDC ? *(const u32x4*)(qb + (int64_t)qrow * p.ldq + ch * 8) : zero4;
            qf[u][ks] = __builtin_bit_cast(bf16x8, t);
        }
    }
    __syncthreads();

    // ---- DMA pieces of this wave: piece j = wave * PPW + i; j < KS: K slots 64 j .. 64 j + 63, then the V pieces, then
    // (to keep the per-wave count uniform) dummies that read nothing and land in a dump area
    const buf_rsrc rk = make_rsrc(kb, (unsigned)((((int64_t)p.skv - 1) * p.ldk + D) * 2));
    const buf_rsrc rv = make_rsrc(vb, (unsigned)((((int64_t)p.skv - 1) * p.ldv + D) * 2));
    unsigned voff[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        const int j = wave * PPW + i;
        if (j < KS) {
            const int sl = j * 64 + lane, key = sl / KS, c = sl - key * KS;
            voff[i] = c < NDC ? (unsigned)key * (unsigned)p.ldk * 2u + (unsigned)c * 16u : DMA_OOB;
        } else if (j < KS + VS) {
            const int sl = (j - KS) * 64 + lane, key = sl / VS, c = sl - key * VS;
            voff[i] = c < NDC ? (unsigned)key * (unsigned)p.ldv * 2u + (unsigned)c * 16u : DMA_OOB;
        } else {
            voff[i] = DMA_OOB;
        }
    }
    const int ntiles = p.skv / KT;
    auto issue = [&](int tile, int buf) {
        const unsigned dead = tile < ntiles ? 0u : DMA_OOB;
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            const int j = wave * PPW + i;
            const bool isk = j < KS, isv = !isk && j < KS + VS;
            const unsigned soff = (unsigned)tile * (unsigned)KT * (unsigned)(isk ? p.ldk : p.ldv) * 2u;
            unsigned char* dst = isk ? lds + buf * TILE + j * 1024 : (isv ? lds + buf * TILE + KB + (j - KS) * 1024 : lds + Cf::OFF_DUMP);
            glds16_buf(isk ? rk : rv, voff[i] | dead, tile < ntiles ? soff : 0u, dst);
        }
    };

    f32x4 acc_o[QF][NFD], acc_l[QF];
    float m_run[QF];
#pragma unroll
    for (int u = 0; u < QF; ++u) {
        m_run[u] = -INFINITY;
        acc_l[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) acc_o[u][fd] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const u32x4 ones4 = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
    const bf16x8 ones = __builtin_bit_cast(bf16x8, ones4);

    // lane parts of the fragment addresses (bytes inside a tile buffer)
    unsigned ka[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) ka[ks] = (unsigned)(fr * KS * 16 + (ks * 4 + fg < NDC ? ks * 4 + fg : NDC - 1) * 16);
    const unsigned va = (unsigned)(KB + ((4 * fg + (fr >> 2)) * VS * 16) + 8 * (fr & 3));

    // fragment reads with compile-time displacements (f / fd are constants after unrolling; the switch folds)
    auto read_k = [&](unsigned base, int f, bf16x8 (&dst)[NKS]) {
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const unsigned a = base + ka[ks];
            switch (f) {
                case 0: dst[ks] = lds_read16_at<0 * 16 * KS * 16>(a); break;
                case 1: dst[ks] = lds_read16_at<1 * 16 * KS * 16>(a); break;
                case 2: dst[ks] = lds_read16_at<2 * 16 * KS * 16>(a); break;
                default: dst[ks] = lds_read16_at<3 * 16 * KS * 16>(a); break;
            }
        }
    };
    auto read_v4 = [&](unsigned vbase, auto fd_c, u32x2 (&dst)[4]) {
        constexpr int F = decltype(fd_c)::value;
        dst[0] = lds_read_tr16_at<(0 * 16) * VS * 16 + 32 * F>(vbase);
        dst[1] = lds_read_tr16_at<(1 * 16) * VS * 16 + 32 * F>(vbase);
        dst[2] = lds_read_tr16_at<(2 * 16) * VS * 16 + 32 * F>(vbase);
        dst[3] = lds_read_tr16_at<(3 * 16) * VS * 16 + 32 * F>(vbase);
    };
    auto read_v = [&](unsigned vbase, int fd, u32x2 (&dst)[4]) {
        switch (fd) {
            case 0: read_v4(vbase, std::integral_constant<int, 0>{}, dst); break;
            case 1: read_v4(vbase, std::integral_constant<int, (1 < NFD ? 1 : 0)>{}, dst); break;
            case 2: read_v4(vbase, std::integral_constant<int, (2 < NFD ? 2 : 0)>{}, dst); break;
            case 3: read_v4(vbase, std::integral_constant<int, (3 < NFD ? 3 : 0)>{}, dst); break;
            case 4: read_v4(vbase, std::integral_constant<int, (4 < NFD ? 4 : 0)>{}, dst); break;
            case 5: read_v4(vbase, std::integral_constant<int, (5 < NFD ? 5 : 0)>{}, dst); break;
            case 6: read_v4(vbase, std::integral_constant<int, (6 < NFD ? 6 : 0)>{}, dst); break;
            case 7: read_v4(vbase, std::integral_constant<int, (7 < NFD ? 7 : 0)>{}, dst); break;
            case 8: read_v4(vbase, std::integral_constant<int, (8 < NFD ? 8 : 0)>{}, dst); break;
            default: read_v4(vbase, std::integral_constant<int, (9 < NFD ? 9 : 0)>{}, dst); break;
        }
    };

#pragma unroll
    for (int t = 0; t < NBUF - 1; ++t) issue(t, t);
    int cur = 0;
    for (int tile = 0; tile < ntiles; ++tile) {
        wait_vmcnt<(NBUF - 2) * PPW>();   // this wave's pieces of `tile` have landed (those of the next NBUF - 2 tiles may be in flight)
        barrier_keep_dma();               // ... every wave's; and every wave is done with tile - 1, whose buffer is refilled now
        issue(tile + NBUF - 1, cur == 0 ? NBUF - 1 : cur - 1);
        const unsigned base = lds_addr(lds) + (unsigned)(cur * TILE);

        // S^T = K Q^T : lane holds S[q = fr][key = 16 f + 4 fg + r].  Fragment reads run two key fragments ahead.
        f32x4 acc_s[QF][4];
        bf16x8 kf[4][NKS];
        read_k(base, 0, kf[0]);
        read_k(base, 1, kf[1]);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            lds_wait_n(f < 3 ? NKS : 0);
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) lds_tie(kf[f][ks]);
#pragma unroll
            for (int u = 0; u < QF; ++u) {
                f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < NKS; ++ks) a = mfma16(kf[f][ks], qf[u][ks], a);
                acc_s[u][f] = a;
            }
            if (f + 2 < 4) read_k(base, f + 2, kf[f + 2]);
        }
        // the first two V^T fragments travel while the softmax runs
        const unsigned vbase = base + va;
        u32x2 vt[NFD][4];
        read_v(vbase, 0, vt[0]);
        if (NFD > 1) read_v(vbase, 1, vt[NFD > 1 ? 1 : 0]);

        // online softmax per owned query row on the RAW scores; P^T operand built in registers.  DEFERRED maximum: the
        // reference point m of a row only has to keep exp2(s - m) in range, it need not be the maximum -- while no row of
        // the wave outgrew its m by more than 2^8 the old m stays (P <= 256: exact in the fp32 / bf16 exponent range, the
        // softmax is invariant to m), and the alpha exponentials and the rescale of O and l are skipped.  On the first
        // tile m = -inf forces the update.
        u32x4 pw[QF][2];
        float m_new[QF];
        bool grow = false;
#pragma unroll
        for (int u = 0; u < QF; ++u) {
            float mx = -INFINITY;
#pragma unroll
            for (int f = 0; f < 4; ++f)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, acc_s[u][f][r]);
            mx = rows4_max(mx);
            m_new[u] = fmaxf(m_run[u], mx * p.scale_log2);
            grow |= !(m_new[u] - m_run[u] <= 8.f);
        }
        if (wave_any(grow)) {
#pragma unroll
            for (int u = 0; u < QF; ++u) {
                const float alpha = fast_exp2(m_run[u] - m_new[u]);
                m_run[u] = m_new[u];
                acc_l[u][0] *= alpha;
#pragma unroll
                for (int fd = 0; fd < NFD; ++fd) {
                    acc_o[u][fd][0] *= alpha; acc_o[u][fd][1] *= alpha;
                    acc_o[u][fd][2] *= alpha; acc_o[u][fd][3] *= alpha;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < QF; ++u) {
            const f32x2 sc2 = {p.scale_log2, p.scale_log2}, nm2 = {-m_run[u], -m_run[u]};
#pragma unroll
            for (int f = 0; f < 4; ++f) {
                const f32x2 t01 = pk_fma(f32x2{acc_s[u][f][0], acc_s[u][f][1]}, sc2, nm2);
                const f32x2 t23 = pk_fma(f32x2{acc_s[u][f][2], acc_s[u][f][3]}, sc2, nm2);
                pw[u][f >> 1][(f & 1) * 2] = pack_bf2(fast_exp2(t01[0]), fast_exp2(t01[1]));
                pw[u][f >> 1][(f & 1) * 2 + 1] = pack_bf2(fast_exp2(t23[0]), fast_exp2(t23[1]));
            }
        }

        // O^T += V^T P^T (transpose reads: 16-lane group fg gathers keys 16 (2 s + hh) + 4 fg .. + 3 of columns 16 fd ..),
        // l += 1^T P^T
#pragma unroll
        for (int u = 0; u < QF; ++u) {
            acc_l[u] = mfma16(ones, __builtin_bit_cast(bf16x8, pw[u][0]), acc_l[u]);
            acc_l[u] = mfma16(ones, __builtin_bit_cast(bf16x8, pw[u][1]), acc_l[u]);
        }
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) {
            lds_wait_n(fd + 1 < NFD ? 4 : 0);
#pragma unroll
            for (int q = 0; q < 4; ++q) lds_tie2(vt[fd][q]);
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const u32x4 t = {vt[fd][2 * s2][0], vt[fd][2 * s2][1], vt[fd][2 * s2 + 1][0], vt[fd][2 * s2 + 1][1]};
                const bf16x8 vf = __builtin_bit_cast(bf16x8, t);
#pragma unroll
                for (int u = 0; u < QF; ++u) acc_o[u][fd] = mfma16(vf, __builtin_bit_cast(bf16x8, pw[u][s2]), acc_o[u][fd]);
            }
            if (fd + 2 < NFD) read_v(vbase, fd + 2, vt[fd + 2 < NFD ? fd + 2 : 0]);
        }
        cur = cur == NBUF - 1 ? 0 : cur + 1;
    }
    wait_vmcnt<0>();                  // the out-of-range pieces issued past the last tile

    bf16_t* ob = p.o + (int64_t)b * p.bso + (int64_t)h * D;
#pragma unroll
    for (int u = 0; u < QF; ++u) {
        const float l = acc_l[u][0];
        const float inv = 1.f / l;
        const int qrow = q0 + u * 16 + fr;
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) {
            const int d = 16 * fd + 4 * fg;
            if (d < D) {
                f32x4 o = acc_o[u][fd];
                u32x2 w = {pack_bf2(o[0] * inv, o[1] * inv), pack_bf2(o[2] * inv, o[3] * inv)};
                *(u32x2*)(ob + (int64_t)qrow * p.ldo + d) = w;
            }
        }
        if (fg == 0 && p.lse)
            p.lse[((int64_t)b * p.heads + h) * p.sq + qrow] = (m_run[u] + log2f(l)) * 0.6931471805599453f;
    }
}
template <int D, int QF, int NBUF>
void launch_fwd_dma(const AttnArgs& a, int batch, hipStream_t s) {
    using Cf = AttnDmaCfg<D, NBUF>;
    static bool attr_set[64] = {};
    int dev_id = 0;
    (void)hipGetDevice(&dev_id);
    if (Cf::LDS_BYTES > 64 * 1024 && (dev_id < 0 || dev_id >= 64 || !attr_set[dev_id])) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_dma_kernel<D, QF, NBUF>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, Cf::LDS_BYTES);
        if (dev_id >= 0 && dev_id < 64) attr_set[dev_id] = true;
    }
    hipLaunchKernelGGL((attn_fwd_dma_kernel<D, QF, NBUF>), dim3(a.sq / (64 * QF), a.heads, batch), dim3(256), Cf::LDS_BYTES, s, a);
}

// ------------------------------------------------------------------------------------------
// Backward (once per optimizer step, for the LoRA-on "target" pass only).  P is recomputed
// from the saved LSE; no atomics, deterministic:
//   attn_delta : delta[q] = sum_d dO[q][d] O[q][d]
//   attn_bwd_dq : same shape as the forward (a wave owns 16 query rows, K/V stream through
//                 LDS): S^T = K Q^T, dP^T = V dO^T, dS = P (dP - delta), dQ^T += K^T dS^T.
//   attn_bwd_dkv: a wave owns 16 keys (K, V fragments live in registers), Q/dO stream through
//                 LDS in 32-row tiles, both row-major (for S = Q K^T, dP = dO V^T) and
//                 transposed (for dV^T += dO^T P, dK^T += Q^T dS).
// The register-resident P / dS accumulators are re-used directly as the second MFMA operand
// through the same key (resp. query) permutation trick as the forward.
// ------------------------------------------------------------------------------------------
struct AttnBwdArgs {
    const bf16_t* q; const bf16_t* k; const bf16_t* v; const bf16_t* o; const bf16_t* d_o;
    int64_t ldq, ldk, ldv, ldo, lddo;
    int64_t bsq, bsk, bsv, bso, bsdo;
    const float* lse; float* delta;
    bf16_t* dq; bf16_t* dk; bf16_t* dv;
    int64_t lddq, lddk, lddv, bsdq, bsdk, bsdv;
    int heads, sq, skv;
    float scale, scale_log2;
    int xcd_remap;
};

template <int D>
__global__ __launch_bounds__(256) void attn_delta_kernel(AttnBwdArgs p, int batch) {
    const int64_t total = (int64_t)batch * p.heads * p.sq;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int qi = (int)(e % p.sq);
        const int h = (int)((e / p.sq) % p.heads), b = (int)(e / ((int64_t)p.sq * p.heads));
        const bf16_t* orow = p.o + (int64_t)b * p.bso + (int64_t)qi * p.ldo + h * D;
        const bf16_t* drow = p.d_o + (int64_t)b * p.bsdo + (int64_t)qi * p.lddo + h * D;
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < D / 8; ++c) {
            u32x4 a = *(const u32x4*)(orow + c * 8), d = *(const u32x4*)(drow + c * 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                acc += bf2f((bf16_t)(a[i] & 0xffffu)) * bf2f((bf16_t)(d[i] & 0xffffu));
                acc += bf2f((bf16_t)(a[i] >> 16)) * bf2f((bf16_t)(d[i] >> 16));
            }
        }
        p.delta[e] = acc;
    }
}

template <int D>
__global__ __launch_bounds__(256) LECO_MIN_WAVES_PER_SIMD(2) void attn_bwd_dq_kernel(AttnBwdArgs p) {
    constexpr int DK = (D + 31) / 32 * 32, DV = (D + 15) / 16 * 16;
    constexpr int NKS = DK / 32, NFD = DV / 16, NDC = D / 8;
    constexpr int KROW = DK + 8, VROW = KT + 8;
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * KT * KROW + DV * VROW];
    bf16_t* sK = smem;
    bf16_t* sV = smem + KT * KROW;
    bf16_t* sKt = smem + 2 * KT * KROW;

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    int bx, h, b;
    attn_ids(p.xcd_remap, bx, h, b);
    const int q0 = bx * 64 + wave * 16;
    const int qrow = q0 + fr;
    const bool qok = qrow < p.sq;

    const bf16_t* kb = p.k + (int64_t)b * p.bsk + (int64_t)h * D;
    const bf16_t* vb = p.v + (int64_t)b * p.bsv + (int64_t)h * D;
    for (int e = tid; e < DV * VROW; e += 256) sKt[e] = 0;

    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    bf16x8 qf[NKS], dof[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int ch = ks * 4 + fg;
        const bool ok = qok && ch < NDC;
        u32x4 t = ok ? *(const u32x4*)(p.q + (int64_t)b * p.bsq + (int64_t)qrow * p.ldq + h * D + ch * 8) : zero4;
        u32x4 u = ok ? *(const u32x4*)(p.d_o + (int64_t)b * p.bsdo + (int64_t)qrow * p.lddo + h * D + ch * 8) : zero4;
        qf[ks] = __builtin_bit_cast(bf16x8, t);
        dof[ks] = __builtin_bit_cast(bf16x8, u);
    }
    const int64_t stat = ((int64_t)b * p.heads + h) * p.sq + (qok ? qrow : 0);
    const float lse2 = p.lse[stat] * 1.4426950408889634f;
    const float dlt = p.delta[stat];

    f32x4 acc[NFD];
#pragma unroll
    for (int fd = 0; fd < NFD; ++fd) acc[fd] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int kv0 = 0; kv0 < p.skv; kv0 += KT) {
        __syncthreads();
        for (int e = tid; e < KT * (DK / 8); e += 256) {
            const int key = e / (DK / 8), ch = e - key * (DK / 8);
            const bool ok = kv0 + key < p.skv && ch < NDC;
            u32x4 tk = ok ? *(const u32x4*)(kb + (int64_t)(kv0 + key) * p.ldk + ch * 8) : zero4;
            u32x4 tv = ok ? *(const u32x4*)(vb + (int64_t)(kv0 + key) * p.ldv + ch * 8) : zero4;
            *(u32x4*)(sK + key * KROW + ch * 8) = tk;
            *(u32x4*)(sV + key * KROW + ch * 8) = tv;
            if (ch < NDC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sKt[(ch * 8 + 2 * i) * VROW + key] = (bf16_t)(tk[i] & 0xffffu);
                    sKt[(ch * 8 + 2 * i + 1) * VROW + key] = (bf16_t)(tk[i] >> 16);
                }
            }
        }
        __syncthreads();

        u32x4 pw[2];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const bf16x8 kf = *(const bf16x8*)(sK + (16 * f + fr) * KROW + (ks * 4 + fg) * 8);
                const bf16x8 vf = *(const bf16x8*)(sV + (16 * f + fr) * KROW + (ks * 4 + fg) * 8);
                s = mfma16(kf, qf[ks], s);
                dp = mfma16(vf, dof[ks], dp);
            }
            float ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kv0 + 16 * f + 4 * fg + r;
                const float pr = key < p.skv ? fast_exp2(s[r] * p.scale_log2 - lse2) : 0.f;
                ds[r] = pr * (dp[r] - dlt);
            }
            pw[f >> 1][(f & 1) * 2] = pack_bf2(ds[0], ds[1]);
            pw[f >> 1][(f & 1) * 2 + 1] = pack_bf2(ds[2], ds[3]);
        }
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16_t* row = sKt + (16 * fd + fr) * VROW + 4 * fg;
                u32x2 lo = *(const u32x2*)(row + 16 * (2 * s2));
                u32x2 hi = *(const u32x2*)(row + 16 * (2 * s2 + 1));
                u32x4 t = {lo[0], lo[1], hi[0], hi[1]};
                acc[fd] = mfma16(__builtin_bit_cast(bf16x8, t), __builtin_bit_cast(bf16x8, pw[s2]), acc[fd]);
            }
    }
    if (qok) {
        bf16_t* dst = p.dq + (int64_t)b * p.bsdq + (int64_t)qrow * p.lddq + h * D;
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) {
            const int d = 16 * fd + 4 * fg;
            if (d < D) {
                u32x2 w = {pack_bf2(acc[fd][0] * p.scale, acc[fd][1] * p.scale),
                           pack_bf2(acc[fd][2] * p.scale, acc[fd][3] * p.scale)};
                *(u32x2*)(dst + d) = w;
            }
        }
    }
}

constexpr int QT = 32;  // query rows per tile in the dK/dV kernel

template <int D>
__global__ __launch_bounds__(256) LECO_MIN_WAVES_PER_SIMD(2) void attn_bwd_dkv_kernel(AttnBwdArgs p) {
    constexpr int DK = (D + 31) / 32 * 32, DV = (D + 15) / 16 * 16;
    constexpr int NKS = DK / 32, NFD = DV / 16, NDC = D / 8;
    constexpr int KROW = DK + 8, TROW = QT + 8;
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * QT * KROW + 2 * DV * TROW];
    __shared__ __attribute__((aligned(16))) float sstat[2 * QT];
    bf16_t* sQ = smem;
    bf16_t* sDO = smem + QT * KROW;
    bf16_t* sQt = smem + 2 * QT * KROW;
    bf16_t* sDOt = sQt + DV * TROW;

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    int bx, h, b;
    attn_ids(p.xcd_remap, bx, h, b);
    const int key = bx * 64 + wave * 16 + fr;
    const bool kok = key < p.skv;

    for (int e = tid; e < 2 * DV * TROW; e += 256) sQt[e] = 0;

    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    bf16x8 kf[NKS], vf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        const int ch = ks * 4 + fg;
        const bool ok = kok && ch < NDC;
        u32x4 t = ok ? *(const u32x4*)(p.k + (int64_t)b * p.bsk + (int64_t)key * p.ldk + h * D + ch * 8) : zero4;
        u32x4 u = ok ? *(const u32x4*)(p.v + (int64_t)b * p.bsv + (int64_t)key * p.ldv + h * D + ch * 8) : zero4;
        kf[ks] = __builtin_bit_cast(bf16x8, t);
        vf[ks] = __builtin_bit_cast(bf16x8, u);
    }
    f32x4 acc_dk[NFD], acc_dv[NFD];
#pragma unroll
    for (int fd = 0; fd < NFD; ++fd) {
        acc_dk[fd] = f32x4{0.f, 0.f, 0.f, 0.f};
        acc_dv[fd] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const bf16_t* qb = p.q + (int64_t)b * p.bsq + (int64_t)h * D;
    const bf16_t* dob = p.d_o + (int64_t)b * p.bsdo + (int64_t)h * D;
    const int64_t stat0 = ((int64_t)b * p.heads + h) * p.sq;

    for (int q0 = 0; q0 < p.sq; q0 += QT) {
        __syncthreads();
        for (int e = tid; e < QT * (DK / 8); e += 256) {
            const int qi = e / (DK / 8), ch = e - qi * (DK / 8);
            const bool ok = q0 + qi < p.sq && ch < NDC;
            u32x4 tq = ok ? *(const u32x4*)(qb + (int64_t)(q0 + qi) * p.ldq + ch * 8) : zero4;
            u32x4 td = ok ? *(const u32x4*)(dob + (int64_t)(q0 + qi) * p.lddo + ch * 8) : zero4;
            *(u32x4*)(sQ + qi * KROW + ch * 8) = tq;
            *(u32x4*)(sDO + qi * KROW + ch * 8) = td;
            if (ch < NDC) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sQt[(ch * 8 + 2 * i) * TROW + qi] = (bf16_t)(tq[i] & 0xffffu);
                    sQt[(ch * 8 + 2 * i + 1) * TROW + qi] = (bf16_t)(tq[i] >> 16);
                    sDOt[(ch * 8 + 2 * i) * TROW + qi] = (bf16_t)(td[i] & 0xffffu);
                    sDOt[(ch * 8 + 2 * i + 1) * TROW + qi] = (bf16_t)(td[i] >> 16);
                }
            }
        }
        if (tid < QT) {
            const bool ok = q0 + tid < p.sq;
            sstat[tid] = ok ? p.lse[stat0 + q0 + tid] * 1.4426950408889634f : 0.f;
            sstat[QT + tid] = ok ? p.delta[stat0 + q0 + tid] : 0.f;
        }
        __syncthreads();

        // S[q][key], dP[q][key]: lane holds q = q0 + 16 f + 4 fg + r for its key (= fr)
        u32x4 pp, pds;
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            f32x4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const bf16x8 aq = *(const bf16x8*)(sQ + (16 * f + fr) * KROW + (ks * 4 + fg) * 8);
                const bf16x8 ad = *(const bf16x8*)(sDO + (16 * f + fr) * KROW + (ks * 4 + fg) * 8);
                s = mfma16(aq, kf[ks], s);
                dp = mfma16(ad, vf[ks], dp);
            }
            const f32x4 l4 = *(const f32x4*)(sstat + 16 * f + 4 * fg);
            const f32x4 d4 = *(const f32x4*)(sstat + QT + 16 * f + 4 * fg);
            float pr[4], ds[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool ok = q0 + 16 * f + 4 * fg + r < p.sq;
                pr[r] = ok ? fast_exp2(s[r] * p.scale_log2 - l4[r]) : 0.f;
                ds[r] = pr[r] * (dp[r] - d4[r]);
            }
            pp[2 * f] = pack_bf2(pr[0], pr[1]);
            pp[2 * f + 1] = pack_bf2(pr[2], pr[3]);
            pds[2 * f] = pack_bf2(ds[0], ds[1]);
            pds[2 * f + 1] = pack_bf2(ds[2], ds[3]);
        }
        // dV^T += dO^T P ; dK^T += Q^T dS   (MFMA k index 8 fg + t <-> tile row 16 (t>>2) + 4 fg + (t&3))
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) {
            const bf16_t* rq = sQt + (16 * fd + fr) * TROW + 4 * fg;
            const bf16_t* rd = sDOt + (16 * fd + fr) * TROW + 4 * fg;
            u32x2 qlo = *(const u32x2*)(rq), qhi = *(const u32x2*)(rq + 16);
            u32x2 dlo = *(const u32x2*)(rd), dhi = *(const u32x2*)(rd + 16);
            u32x4 tq = {qlo[0], qlo[1], qhi[0], qhi[1]};
            u32x4 td = {dlo[0], dlo[1], dhi[0], dhi[1]};
            acc_dv[fd] = mfma16(__builtin_bit_cast(bf16x8, td), __builtin_bit_cast(bf16x8, pp), acc_dv[fd]);
            acc_dk[fd] = mfma16(__builtin_bit_cast(bf16x8, tq), __builtin_bit_cast(bf16x8, pds), acc_dk[fd]);
        }
    }
    if (kok) {
        bf16_t* dkd = p.dk + (int64_t)b * p.bsdk + (int64_t)key * p.lddk + h * D;
        bf16_t* dvd = p.dv + (int64_t)b * p.bsdv + (int64_t)key * p.lddv + h * D;
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) {
            const int d = 16 * fd + 4 * fg;
            if (d < D) {
                u32x2 wk = {pack_bf2(acc_dk[fd][0] * p.scale, acc_dk[fd][1] * p.scale),
                            pack_bf2(acc_dk[fd][2] * p.scale, acc_dk[fd][3] * p.scale)};
                u32x2 wv = {pack_bf2(acc_dv[fd][0], acc_dv[fd][1]), pack_bf2(acc_dv[fd][2], acc_dv[fd][3])};
                *(u32x2*)(dkd + d) = wk;
                *(u32x2*)(dvd + d) = wv;
            }
        }
    }
}

template <int D>
int launch_bwd(const AttnBwdArgs& a, int batch, hipStream_t s) {
    const int64_t rows = (int64_t)batch * a.heads * a.sq;
    hipLaunchKernelGGL((attn_delta_kernel<D>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, a, batch);
    hipLaunchKernelGGL((attn_bwd_dq_kernel<D>), dim3(cdiv(a.sq, 64), a.heads, batch), dim3(256), 0, s, a);
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<D>), dim3(cdiv(a.skv, 64), a.heads, batch), dim3(256), 0, s, a);
    return check_launch("leco_attention_bwd");
}

// ------------------------------------------------------------------------------------------
// Wide-head forward (the VAE decoder's mid-block attention: ONE head as wide as the channel count, d = 512; d = 128 for the
// tiny synthetic decoder).  Forward only, flash-style: O(S d) memory at any S.  A wave cannot hold 16 query rows x d of O
// next to a d-wide Q fragment (d = 512: 64 + 512 registers), so the two products are split differently over the 4 waves of
// a workgroup (64 query rows):
//   phase A  wave w owns the query stripe 16 w .. 16 w + 15 over the FULL d (Q fragment in registers, d / 8 VGPRs): S^T = K Q^T
//            against the 64-key K tile in LDS, online softmax per lane-owned row exactly as in attn_fwd_kernel; the bf16 P^T
//            operand registers and the row's rescale factor alpha go to LDS;
//   phase B  wave w owns the COLUMN slice d / 4 * w .. of O for all 64 query rows (fp32, 64 x d / 4: d / 4 VGPRs): it reads the
//            four stripes' P^T operands back lane-for-lane (the layout a lane wrote is the layout a lane needs) and
//            O^T += V^T P^T against the V tile in LDS through the transpose read.
// LDS: K tile 64 x (d + 8), V tile 64 x (d + 16), P 8 KB: 140 KB at d = 512 -- one workgroup per CU, single-buffered (three
// barriers per tile).  The kernel runs once per decode.
template <int D>
struct AttnWideCfg {
    static constexpr int DW = D / 4, NKS = D / 32, NFD = DW / 16, NDC = D / 8;
    static constexpr int KROW = D + 8;
    static constexpr int VRB0 = D * 2, VRB = ((VRB0 / 32) % 2) ? VRB0 : VRB0 + 32, VROW = VRB / 2;
    static constexpr int OFF_V = KT * KROW * 2, OFF_P = OFF_V + KT * VROW * 2, OFF_A = OFF_P + 8 * 64 * 16;
    static constexpr int LDS_BYTES = OFF_A + 64 * 4;
    static_assert(D % 64 == 0 && (KT * NDC) % 256 == 0, "wide attention: d must be a multiple of 64");
    static_assert(LDS_BYTES <= 160 * 1024, "wide attention: tiles exceed the 160 KB LDS");
};

template <int D>
__global__ __launch_bounds__(256) LECO_MIN_WAVES_PER_SIMD(1) void attn_fwd_wide_kernel(AttnArgs p) {
    using Cf = AttnWideCfg<D>;
    constexpr int DW = Cf::DW, NKS = Cf::NKS, NFD = Cf::NFD, NDC = Cf::NDC, KROW = Cf::KROW, VROW = Cf::VROW;
    unsigned char* lds = dyn_lds();
    bf16_t* sK = (bf16_t*)lds;
    bf16_t* sV = (bf16_t*)(lds + Cf::OFF_V);
    u32x4* sP = (u32x4*)(lds + Cf::OFF_P);     // [stripe 4][s 2][lane 64]: the P^T operand registers of each stripe's wave
    float* sA = (float*)(lds + Cf::OFF_A);     // [64 query rows]: alpha of the tile (after the last tile: the row sum l)

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    int bx, h, b;
    attn_ids(p.xcd_remap, bx, h, b);
    const int q0 = bx * 64;
    const bf16_t* qb = p.q + (int64_t)b * p.bsq + (int64_t)h * D;
    const bf16_t* kb = p.k + (int64_t)b * p.bsk + (int64_t)h * D;
    const bf16_t* vb = p.v + (int64_t)b * p.bsv + (int64_t)h * D;

    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    bf16x8 qf[NKS];
    {
        const int qrow = q0 + wave * 16 + fr;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            u32x4 t = qrow < p.sq ? *(const u32x4*)(qb + (int64_t)qrow * p.ldq + (ks * 4 + fg) * 8) : zero4;
            qf[ks] = __builtin_bit_cast(bf16x8, t);
        }
    }
    f32x4 acc_o[4][NFD];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) acc_o[u][fd] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;

    for (int kv0 = 0; kv0 < p.skv; kv0 += KT) {
        // stage the K and V tiles (rows past skv: zeros); thread e -> (key = e / NDC, 16-byte chunk e % NDC)
#pragma unroll 4
        for (int e = tid; e < KT * NDC; e += 256) {
            const int key = e / NDC, ch = e - key * NDC;
            const bool ok = kv0 + key < p.skv;
            const u32x4 tk = ok ? *(const u32x4*)(kb + (int64_t)(kv0 + key) * p.ldk + ch * 8) : zero4;
            const u32x4 tv = ok ? *(const u32x4*)(vb + (int64_t)(kv0 + key) * p.ldv + ch * 8) : zero4;
            *(u32x4*)(sK + key * KROW + ch * 8) = tk;
            *(u32x4*)(sV + key * VROW + ch * 8) = tv;
        }
        __syncthreads();

        // ---- phase A: S^T = K Q^T for this wave's stripe: lane holds S[q = fr][key = kv0 + 16 f + 4 fg + r]
        f32x4 acc_s[4];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const bf16x8 kf = *(const bf16x8*)(sK + (16 * f + fr) * KROW + (ks * 4 + fg) * 8);
                a = mfma16(kf, qf[ks], a);
            }
            acc_s[f] = a;
        }
        float mx = -INFINITY;
#pragma unroll
        for (int f = 0; f < 4; ++f)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = kv0 + 16 * f + 4 * fg + r;
                acc_s[f][r] = key < p.skv ? acc_s[f][r] : -INFINITY;
                mx = fmaxf(mx, acc_s[f][r]);
            }
        mx = rows4_max(mx);
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
        sP[(wave * 2 + 0) * 64 + lane] = pw[0];
        sP[(wave * 2 + 1) * 64 + lane] = pw[1];
        if (fg == 0) sA[wave * 16 + fr] = alpha;
        __syncthreads();

        // ---- phase B: O^T[d slice of this wave][all 64 rows] += V^T P^T (key order of the P^T registers: MFMA k index
        // 8 fg + t <-> tile key 16 (2 s + (t >> 2)) + 4 fg + (t & 3), matched by the transpose reads as in attn_fwd_kernel)
        float al[4];
        bf16x8 pf[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            al[u] = sA[16 * u + fr];
            pf[u][0] = __builtin_bit_cast(bf16x8, sP[(u * 2 + 0) * 64 + lane]);
            pf[u][1] = __builtin_bit_cast(bf16x8, sP[(u * 2 + 1) * 64 + lane]);
        }
#pragma unroll
        for (int fd = 0; fd < NFD; ++fd) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                acc_o[u][fd][0] *= al[u]; acc_o[u][fd][1] *= al[u];
                acc_o[u][fd][2] *= al[u]; acc_o[u][fd][3] *= al[u];
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const bf16_t* blk = sV + (16 * (2 * s) + 4 * fg + (fr >> 2)) * VROW + wave * DW + 16 * fd + 4 * (fr & 3);
                const u32x2 lo = lds_read_tr16(blk);
                const u32x2 hi = lds_read_tr16(blk + 16 * VROW);
                const u32x4 t = {lo[0], lo[1], hi[0], hi[1]};
                const bf16x8 vf = __builtin_bit_cast(bf16x8, t);
#pragma unroll
                for (int u = 0; u < 4; ++u) acc_o[u][fd] = mfma16(vf, pf[u][s], acc_o[u][fd]);
            }
        }
        __syncthreads();      // every wave is done with K, V, P and alpha of this tile
    }

    // row sums of the four stripes -> LDS; each wave normalises and stores its column slice of all 64 rows
    {
        const float l = rows4_sum(l_run);
        const int qrow = q0 + wave * 16 + fr;
        if (fg == 0) {
            sA[wave * 16 + fr] = l;
            if (p.lse && qrow < p.sq) p.lse[((int64_t)b * p.heads + h) * p.sq + qrow] = (m_run + log2f(l)) * 0.6931471805599453f;
        }
    }
    __syncthreads();
    bf16_t* ob = p.o + (int64_t)b * p.bso + (int64_t)h * D + wave * DW;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float inv = 1.f / sA[16 * u + fr];
        const int qrow = q0 + 16 * u + fr;
        if (qrow < p.sq) {
#pragma unroll
            for (int fd = 0; fd < NFD; ++fd) {
                const f32x4 o = acc_o[u][fd];
                const u32x2 w = {pack_bf2(o[0] * inv, o[1] * inv), pack_bf2(o[2] * inv, o[3] * inv)};
                *(u32x2*)(ob + (int64_t)qrow * p.ldo + 16 * fd + 4 * fg) = w;
            }
        }
    }
}
template <int D>
int launch_fwd_wide(const AttnArgs& a, int batch, hipStream_t s) {
    using Cf = AttnWideCfg<D>;
    static bool attr_set[64] = {};
    int dev_id = 0;
    (void)hipGetDevice(&dev_id);
    if (Cf::LDS_BYTES > 64 * 1024 && (dev_id < 0 || dev_id >= 64 || !attr_set[dev_id])) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_wide_kernel<D>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, Cf::LDS_BYTES);
        if (dev_id >= 0 && dev_id < 64) attr_set[dev_id] = true;
    }
    hipLaunchKernelGGL((attn_fwd_wide_kernel<D>), dim3(cdiv(a.sq, 64), a.heads, batch), dim3(256), Cf::LDS_BYTES, s, a);
    return check_launch("leco_attention_fwd");
}

template <int D>
int launch_fwd(const AttnArgs& a, int batch, hipStream_t s) {
    static const int force_qf = [] {   // tuning override: LECO_ATTN_QF = 1 | 2 (query fragments per wave)
        const char* e = getenv("LECO_ATTN_QF");
        return e ? atoi(e) : 0;
    }();
    // two query fragments per wave halve the K/V traffic per query but also the workgroup count: worth it once
    // there are still >= 4 workgroups per CU (measured: 4x8x4096^2x40 218 vs 238 us, 4x8x1024^2x80 35.8 vs 31.8 us)
    const long wgs2 = (long)cdiv(a.sq, 128) * a.heads * batch;
    const bool masked = a.skv % KT != 0;
    // self-attention at d = 40 / 64 / 80 with enough workgroups to fill the chip: the LDS-DMA staged kernel (LECO_ATTN_DMA=0:
    // off; =2: also for small grids -- the kernel tests)
    const char* dma_env = getenv("LECO_ATTN_DMA");             // (read per launch: launches are recorded into graphs once)
    const int use_dma = dma_env ? atoi(dma_env) : 1;
    if constexpr (D == 40 || D == 64 || D == 80) {
        constexpr int NBUF = D == 64 ? 2 : 3;
        const long wgs1 = (long)cdiv(a.sq, 64) * a.heads * batch;
        const bool fits = ((int64_t)a.skv * a.ldk * 2 < (1ll << 31)) && ((int64_t)a.skv * a.ldv * 2 < (1ll << 31));
        if (use_dma && !masked && fits) {
            if (a.sq % 128 == 0 && (wgs2 >= 512 || (use_dma == 2 && force_qf != 1)) && force_qf != 1) {
                launch_fwd_dma<D, 2, NBUF>(a, batch, s);
                return check_launch("leco_attention_fwd");
            }
            if (a.sq % 64 == 0 && (wgs1 >= 512 || use_dma == 2) && force_qf != 2) {
                launch_fwd_dma<D, 1, NBUF>(a, batch, s);
                return check_launch("leco_attention_fwd");
            }
        }
    }
    if (force_qf ? force_qf == 2 : wgs2 >= 1024) {
        const dim3 grid(cdiv(a.sq, 128), a.heads, batch);
        if (masked) hipLaunchKernelGGL((attn_fwd_kernel<D, 2, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((attn_fwd_kernel<D, 2, false>), grid, dim3(256), 0, s, a);
    } else {
        const dim3 grid(cdiv(a.sq, 64), a.heads, batch);
        if (masked) hipLaunchKernelGGL((attn_fwd_kernel<D, 1, true>), grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL((attn_fwd_kernel<D, 1, false>), grid, dim3(256), 0, s, a);
    }
    return check_launch("leco_attention_fwd");
}
}  // namespace
}  // namespace leco

using namespace leco;

extern "C" int leco_attention_fwd(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk,
                                  int64_t bsk, const void* v, int64_t ldv, int64_t bsv, void* o,
                                  int64_t ldo, int64_t bso, float* lse, int32_t batch, int32_t heads,
                                  int32_t sq, int32_t skv, int32_t head_dim, float scale,
                                  leco_stream_t stream) {
    if (batch <= 0 || heads <= 0 || sq <= 0 || skv <= 0) return fail(-EINVAL, "attention: empty problem");
    if ((ldq | ldk | ldv | ldo | bsq | bsk | bsv | bso) % 8) return fail(-EINVAL, "attention: strides must be multiples of 8 elements");
    AttnArgs a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, ldq, ldk, ldv, bsq, bsk, bsv,
               (bf16_t*)o, ldo, bso, lse, heads, sq, skv, scale * 1.4426950408889634f, attn_xcd_default()};
    hipStream_t s = (hipStream_t)stream;
    switch (head_dim) {
        case 32: return launch_fwd<32>(a, batch, s);
        case 40: return launch_fwd<40>(a, batch, s);
        case 64: return launch_fwd<64>(a, batch, s);
        case 80: return launch_fwd<80>(a, batch, s);
        case 160: return launch_fwd<160>(a, batch, s);
        case 128: return launch_fwd_wide<128>(a, batch, s);      // single wide head (VAE mid-block): forward only, lse optional
        case 512: return launch_fwd_wide<512>(a, batch, s);
        default: return fail(-EINVAL, "attention: unsupported head_dim %d (32/40/64/80/160, forward only: 128/512)", head_dim);
    }
}

extern "C" int leco_attention_bwd(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk,
                                  int64_t bsk, const void* v, int64_t ldv, int64_t bsv, const void* o,
                                  int64_t ldo, int64_t bso, const void* d_o, int64_t lddo, int64_t bsdo,
                                  const float* lse, float* delta, void* dq, int64_t lddq, int64_t bsdq,
                                  void* dk, int64_t lddk, int64_t bsdk, void* dv, int64_t lddv,
                                  int64_t bsdv, int32_t batch, int32_t heads, int32_t sq, int32_t skv,
                                  int32_t head_dim, float scale, leco_stream_t stream) {
    if (batch <= 0 || heads <= 0 || sq <= 0 || skv <= 0) return fail(-EINVAL, "attention_bwd: empty problem");
    if ((ldq | ldk | ldv | ldo | lddo | lddq | lddk | lddv | bsq | bsk | bsv | bso | bsdo | bsdq | bsdk | bsdv) % 4)
        return fail(-EINVAL, "attention_bwd: strides must be multiples of 4 elements");
    AttnBwdArgs a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)o, (const bf16_t*)d_o,
                  ldq, ldk, ldv, ldo, lddo, bsq, bsk, bsv, bso, bsdo, lse, delta,
                  (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, lddq, lddk, lddv, bsdq, bsdk, bsdv,
                  heads, sq, skv, scale, scale * 1.4426950408889634f, attn_xcd_default()};
    hipStream_t s = (hipStream_t)stream;
    switch (head_dim) {
        case 32: return launch_bwd<32>(a, batch, s);
        case 40: return launch_bwd<40>(a, batch, s);
        case 64: return launch_bwd<64>(a, batch, s);
        case 80: return launch_bwd<80>(a, batch, s);
        case 160: return launch_bwd<160>(a, batch, s);
        default: return fail(-EINVAL, "attention_bwd: unsupported head_dim %d", head_dim);
    }
}
