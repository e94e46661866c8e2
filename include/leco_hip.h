/* libleco_hip.so -- C ABI of the MI355X (gfx950) LECO training hot path.
 *
 * The reference (p1atdev/LECO) has no FFI: its per-step arithmetic is
 * diffusers' UNet2DConditionModel.forward / autograd / DDIMScheduler.step /
 * torch.optim.AdamW called from train_util.py:142-193 and train_lora.py:141-290.
 * Each entry point below names the reference call it replaces.  Conventions:
 *   - all pointers are DEVICE pointers owned by the caller (PyTorch allocations);
 *   - activations are bf16, channels-last ([B][H][W][C] == [B*H*W tokens][C]);
 *   - every function only ENQUEUES work on `stream` (a hipStream_t) and never
 *     synchronises, so a sequence of calls can be captured into a hipGraph;
 *   - return 0 on success, a negative errno-style code on bad arguments or a
 *     failed launch; leco_last_error() gives the message (thread-local).
 * No torch types cross this boundary.
 */
#ifndef LECO_HIP_H
#define LECO_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* leco_stream_t; /* hipStream_t */

int leco_version(void);
const char* leco_last_error(void);

/* ------------------------------------------------------------------------
 * Fused GEMM / implicit-GEMM 3x3 convolution, bf16 MFMA with fp32 accumulation, with the
 * rank-r LoRA product folded into the same accumulator as one extra K tile
 * ("K-extension": A_ext = x*A^T, W_ext = scale*B):
 *   C[m][n] = act( sum_k A[m][k] W[n][k] + sum_j A_ext[m][j] W_ext[n][j]
 *                  + bias[n] + rowbias[m/rows_per_group][n] + residual[m][n] )
 * Replaces: every nn.Linear / nn.Conv2d forward inside diffusers' UNet (call site
 * train_util.py:156-160) including the LoRA branch lora.py:102-106 (org_forward(x) +
 * lora_up(lora_down(x))*multiplier*scale) and -- with pre-transposed weights -- their
 * autograd dgrad (train_lora.py:279).
 * ---------------------------------------------------------------------- */
enum {
    LECO_A_PLAIN = 0,      /* A is [M][K] row-major (optionally split over two sources) */
    LECO_A_CONV3_S1 = 1,   /* 3x3 pad 1 stride 1 on NHWC input, K = 9*Cin, k = tap*Cin + c */
    LECO_A_CONV3_S2 = 2,   /* 3x3 pad 1 stride 2 (Downsample2D) */
    LECO_A_CONV3_UP2 = 3,  /* 3x3 pad 1 on the nearest-2x upsampled input (Upsample2D) */
    LECO_A_CONV3_TR2 = 4,  /* transposed stride-2 gather: dgrad of LECO_A_CONV3_S2 */
    /* 3x3 stride 2 with padding on the bottom / right only (diffusers Downsample2D(padding=0): F.pad(x, (0,1,0,1)) then a
     * pad-0 conv, the VAE encoder's downsample): tap (kh, kw) of output (y, x) reads input (2y + kh, 2x + kw), zero past
     * the last row / column.  h_in, w_in even, h_out = h_in / 2, w_out = w_in / 2, else -EINVAL.  leco_gemm (every tile of the
     * implicit-GEMM kernel, split-K, column statistics) only: leco_f32_gemm, leco_lora_wgrad_conv and the patch-staged
     * convolution refuse it by name. */
    LECO_A_CONV3_S2_PAD01 = 5
};
/* LECO_ACT_GEGLU (leco_gemm only): the GEMM is the GEGLU input projection (diffusers GEGLU.proj, N = 2F) with its
 * weight / bias / w_ext ROWS interleaved in blocks of 64 -- row 128 j + r holds value row 64 j + r (r < 64) or gate
 * row F + 64 j + (r - 64) (r >= 64) -- so one 128-column tile owns a value block and its gate block: the epilogue
 * writes value * gelu(gate) (erf form) as bf16 [M][F] (row stride ldc) and the [M][2F] intermediate never
 * exists.  Needs n % 128 == 0, c != NULL, no residual / rowbias / c_f32, no split-K.
 * LECO_ACT_QUICK_GELU: z sigmoid(1.702 z) (CLIP-L's MLP, transformers' QuickGELUActivation); LECO_ACT_GELU: z Phi(z), the
 * erf form (OpenCLIP-H / bigG's MLP; the same gelu the GEGLU epilogue applies to its gate).  Both are pointwise like
 * LECO_ACT_SILU -- C = act(acc + bias + rowbias + residual) -- on every tile id of leco_gemm / leco_gemm_tile /
 * leco_gemm_ex, conv gathers included; under split-K the finishing kernel applies them.  leco_f32_gemm rejects them
 * (-EINVAL); leco_xgemm and the stripe chains carry no act argument.  Any other value of act is -EINVAL. */
enum { LECO_ACT_NONE = 0, LECO_ACT_SILU = 1, LECO_ACT_GEGLU = 2, LECO_ACT_QUICK_GELU = 3, LECO_ACT_GELU = 4 };

typedef struct leco_gemm_args {
    const void* a0;       /* bf16 */
    const void* a1;       /* bf16, second channel/K source (skip-connection concat) or NULL */
    int64_t lda0, lda1;   /* plain: row strides (elements); conv: per-pixel channel strides */
    int32_t k_split;      /* plain: columns [0,k_split) come from a0; conv: channels [0,k_split) */
    int32_t a_mode;
    int32_t batch, h_out, w_out, h_in, w_in; /* conv modes only */
    const void* w;        /* bf16 [N][K], K contiguous; conv: [N][3][3][Cin] */
    int64_t ldw;
    int32_t m, n, k;      /* k % 64 == 0 (conv: Cin % 64 == 0), n % 8 == 0 */
    const void* a_ext;    /* bf16 [M][ext_k] (row stride ld_aext) or NULL */
    int64_t ld_aext;
    const void* w_ext;    /* bf16 [N][ext_k] (row stride ld_wext) */
    int64_t ld_wext;
    int32_t ext_k;        /* 0, 32 or 64 */
    const float* bias;        /* fp32 [N] or NULL */
    const float* rowbias;     /* fp32 [M/rows_per_group][N] or NULL (time-embedding add) */
    int32_t rows_per_group;
    int64_t ld_rowbias;       /* row stride of rowbias (elements) */
    const void* residual;     /* bf16 [M][N] (row stride ldr) or NULL */
    int64_t ldr;
    int32_t act;
    void* c;                  /* bf16 out, row stride ldc (or NULL) */
    int64_t ldc;
    float* c_f32;             /* optional fp32 copy of the pre-rounding result, row stride ldc32 */
    int64_t ldc32;
    /* Fused LoRA down-projection (plain A only; exclusive with a_ext): t_w = stacked lora_down rows, bf16
     * [32][K] (rows >= groups*r zero), row stride ld_tw; t_rows = 16 or 32 = how many of them are non-zero
     * (rounded up to 16).  The kernel forms T = A t_w^T during its own K sweep, rounds it to bf16 and uses it
     * as the A side of the K-extension against w_ext (ext_k must be 32).  t_out (optional, bf16 [M][32], row
     * stride ld_tout) receives T for the backward (lora_up wgrad); it is REQUIRED scratch when the launch
     * heuristic may split K (then T is computed by a separate skinny GEMM into t_out). */
    const void* t_w;
    int64_t ld_tw;
    int32_t t_rows;
    void* t_out;
    int64_t ld_tout;
    /* GroupNorm statistics emitted by the PRODUCER of a tensor (diffusers' GroupNorm re-reads the whole tensor for them;
     * `north_star`: conv2d / GroupNorm fused): col_stats != NULL accumulates {sum, sum of squares} of the bf16-ROUNDED
     * values this call stores to c, per sample and per ATOM of stats_atom adjacent output columns -- fp32
     * [m / stats_rows][n / stats_atom][2], fp32 atomics (a global fp32 atomic costs ~12 ns at its memory channel: one per
     * atom and tile, not one per column), into a buffer the caller has zeroed.  stats_rows = rows (pixels) per sample;
     * stats_atom divides every GroupNorm group the tensor will be part of (SD: 320 / 32 = 10 channels).
     * leco_groupnorm_apply_stats consumes them.  Needs a bf16 output; not with LECO_ACT_GEGLU. */
    float* col_stats;
    int32_t stats_rows;
    int32_t stats_atom;
} leco_gemm_args;

int leco_gemm(const leco_gemm_args* args, leco_stream_t stream);

/* Re-pack every LoRA site (1..3 LoRA modules sharing an input: fused q|k|v) from the bf16
 * shadow of the trainable slab into the four MFMA operand images the hot path consumes:
 *   dn_s [R16][K]  = stacked lora_down rows (zero rows up to R16)          fwd: T = x dn_s^T
 *   up_p [N][Rp]   = scale * lora_up, block-diagonal over groups            fwd K-extension
 *   up_t [R16][N]  = lora_up^T, block-diagonal                              bwd: U = dy up_t^T
 *   dn_p [K][Rp]   = scale * lora_down^T                                    bwd K-extension
 * R = groups*r, R16 = roundup(R,16), Rp = roundup(R,32) unless `rp` overrides it; group g owns output columns
 * [g*N/groups, (g+1)*N/groups).  down[g] is [r][K], up[g] is [N/groups][r] (lora.py:65-66).
 * `sites` is a DEVICE array of descriptors; one launch covers all of them. */
typedef struct leco_lora_site {
    const void* down[3]; /* bf16 */
    const void* up[3];   /* bf16 */
    int32_t groups, r, k, n;
    float scale;         /* multiplier * alpha / r  (lora.py:87,105) */
    int32_t taps;        /* 0/1: Linear or 1x1 conv; 9: 3x3 conv LoRA (k = 9*Cin, lora_down is [r][Cin][3][3]):
                            Rp = 64, dn_s[j][tap*Cin+c], dn_p[c][tap][j] = scale*down[j][c][8-tap] (dgrad operand) */
    void* dn_s;
    void* up_p;
    void* up_t;
    void* dn_p;
    void* up_pg;         /* optional: a second copy of up_p with the LECO_ACT_GEGLU row interleave (or NULL) */
    int32_t rp;          /* 0: Rp = roundup(R, 32) (64 for conv sites); else the column count of up_p / dn_p (a multiple
                            of 64 for R > 64: ranks whose stacked columns need several 64-wide K-extension steps) */
} leco_lora_site;

int leco_lora_pack(const leco_lora_site* sites, int32_t nsites, leco_stream_t stream);
/* Per-sample LoRA strength (the forward-only "sweep" plans): the low-rank image T = x down^T of a site, bf16
 * [rows][cols] with row stride ld (elements), is scaled in place,
 *     T[m][c] = bf16(float(T[m][c]) * strengths[m / rows_per_sample]),
 * strengths = fp32 [rows / rows_per_sample] in DEVICE memory, read when the kernel runs (a captured graph picks up new
 * values at replay).  cols and ld are multiples of 8 (the sites' Rp: 32 or a multiple of 64), T is 16-byte aligned,
 * rows is a multiple of rows_per_sample; columns cols..ld are not touched. */
int leco_lora_rowscale(void* t, int64_t ld, int32_t rows, int32_t cols, int32_t rows_per_sample, const float* strengths,
                       leco_stream_t stream);
/* The same for a STACK of LoRA files that sit side by side in the rank dimension (LoRAStack): every file has a strength of
 * its own per sample,
 *     T[m][c] = bf16(float(T[m][c]) * strengths[m / rows_per_sample][col_file[c % period]]),
 * strengths = fp32 [rows / rows_per_sample][files] and col_file = int32 [period] (entries < files), both in DEVICE memory and
 * read when the kernel runs.  period = the per-module stacked rank (a fused q|k|v site holds three modules of `period`
 * columns in one T); it need not be a multiple of 8 and the files' column blocks need not start on one.  1 <= files <= 8,
 * period >= 1; cols, ld, T and rows as for leco_lora_rowscale. */
int leco_lora_rowscale_stack(void* t, int64_t ld, int32_t rows, int32_t cols, int32_t rows_per_sample, const float* strengths,
                             int32_t files, const int32_t* col_file, int32_t period, leco_stream_t stream);


/* G[j*g_sj + c*g_sc] += scale * sum_m P[m][p_off+j] * Q[m][q_off+c], j<r, c<cols (LoRA weight
 * gradients into the flat gradient slab).  P, Q bf16.  Replaces autograd's wgrad of lora_down / lora_up
 * (train_lora.py:279).  part == NULL: the 128-row slabs of M accumulate with fp32 atomics (fast, summation order
 * varies run to run).  part != NULL (DETERMINISTIC mode): every slab writes its contribution to the caller's fp32
 * scratch (ceil(m/128) * r * cols floats <= part_bytes) and a second launch adds them in slab order: bitwise
 * reproducible gradients. */
int leco_lora_wgrad(const void* p, int64_t ldp, const void* q, int64_t ldq, float* g,
                    int64_t g_sj, int64_t g_sc, int32_t m, int32_t r, int32_t cols, float scale,
                    float* part, int64_t part_bytes, leco_stream_t stream);

/* All LoRA weight gradients of a backward in ONE launch (atomic accumulation, like leco_lora_wgrad with part == NULL):
 * `problems` is a DEVICE array; problem i owns the blocks [block_start, block_start + blocks_x * ceil(m / 128)) with
 * blocks_x = ceil(cols / 256); total_blocks = their sum; max_rank = largest r in the table (<= 16).  a_mode
 * LECO_A_PLAIN: a leco_lora_wgrad problem; LECO_A_CONV3_S1/S2/UP2: a leco_lora_wgrad_conv problem (tap kh, kw). */
typedef struct leco_wgrad_problem {
    const void* p; int64_t ldp;
    const void* q; int64_t ldq;
    float* g; int64_t g_sj, g_sc;
    int32_t m, r, cols;
    float scale;
    int32_t a_mode, h_out, w_out, h_in, w_in, kh, kw;
    int32_t block_start, blocks_x;
} leco_wgrad_problem;
int leco_lora_wgrad_grouped(const leco_wgrad_problem* problems, int32_t nproblems, int32_t total_blocks,
                            int32_t max_rank, leco_stream_t stream);

/* same as leco_gemm with an explicit tile choice: 0 heuristic, 1 = 128x128 (wave shape by grid size), 2 = 128x160,
 * 3 = 64x64, 4 = 256x128, 5 = 128x128 as 4-wave workgroups (two per CU), 6 = 128x128 as one 8-wave workgroup per CU,
 * 11 = 128x64 (7..10: the patch-staged 3x3 convolution kernels, conv_patch.hip)
 * (tests / the launch-shape tuner leco_amd/tune.py). */
int leco_gemm_tile(const leco_gemm_args* args, int tile, leco_stream_t stream);
/* full form: additionally split_k (0 = heuristic, 1 = none, n = that many K slices) with a
 * caller-owned fp32 workspace for the partial slabs (split_k * m * n * 4 bytes; a too small
 * workspace only reduces the split).  Deep-K / small-M problems (the 8x8 and 16x16 UNet levels)
 * need this to fill 256 CUs. */
int leco_gemm_ex(const leco_gemm_args* args, int tile, int split_k, void* workspace,
                 int64_t workspace_bytes, leco_stream_t stream);
/* dry run of leco_gemm_ex: writes the kernel instantiation(s) that call would launch -- "gemm_kernel<BM, BN, CONV, NS,
 * NWM, TF> grid=.. split=.." as rocprofv3 names them, " ; "-separated when a call expands to two GEMMs -- into out.
 * Nothing is launched.  Measurement tooling (bench.py attributes plan launches to profile rows with it). */
int leco_gemm_describe(const leco_gemm_args* args, int tile, int split_k, void* workspace,
                       int64_t workspace_bytes, char* out, int32_t out_len);

/* same with Q gathered like the A operand of a 3x3 conv (one call per tap; a_mode LECO_A_CONV3_S1/S2/UP2):
 * the wgrad of a conv lora_down (c3lier, lora.py:72-81).  m = batch*h_out*w_out output rows. */
int leco_lora_wgrad_conv(const void* p, int64_t ldp, const void* q, int64_t ldq, float* g, int64_t g_sj,
                         int64_t g_sc, int32_t m, int32_t r, int32_t cols, float scale, int32_t a_mode,
                         int32_t h_out, int32_t w_out, int32_t h_in, int32_t w_in, int32_t kh, int32_t kw,
                         float* part, int64_t part_bytes, leco_stream_t stream);
/* out[b][c] = sum of the rows_per_group rows of sample b of x[.][c] (fp32): gradient of the per-sample
 * time-embedding bias added by ResnetBlock2D (needed only when time_emb_proj carries a LoRA). */
int leco_rowgroup_sum(const void* x, int64_t ldx, float* out, int64_t ldo, int32_t groups,
                      int32_t rows_per_group, int32_t cols, leco_stream_t stream);

/* ------------------------------------------------------------------------
 * Normalisation (diffusers GroupNorm(32) in ResnetBlock2D / Transformer2DModel / conv_norm_out,
 * LayerNorm in BasicTransformerBlock; call site train_util.py:156-160; dgrads train_lora.py:279).
 * x may be the channel concat [x0 | x1] (x1 == NULL: single source).  stats / bstats are
 * fp32 [batch][groups][2] scratch ({sum, sumsq} resp. {sum dxhat, sum dxhat*xhat}); the
 * forward stats must be kept for the backward.  act: LECO_ACT_NONE / LECO_ACT_SILU (any other value: -EINVAL).
 * ---------------------------------------------------------------------- */
#define LECO_GN_STATS_FLOATS(batch, groups) ((int64_t)(batch) * (groups) * 2 * 257)
int leco_groupnorm_fwd(const void* x0, int64_t ld0, const void* x1, int64_t ld1, int32_t c0,
                       const float* gamma, const float* beta, int32_t batch, int32_t hw, int32_t c,
                       int32_t groups, float eps, int32_t act, float* stats, void* y, int64_t ldy,
                       leco_stream_t stream);
int leco_groupnorm_bwd(const void* x0, int64_t ld0, const void* x1, int64_t ld1, int32_t c0,
                       const void* dy, int64_t lddy, const float* gamma, const float* beta,
                       const float* stats, int32_t batch, int32_t hw, int32_t c, int32_t groups,
                       float eps, int32_t act, float* bstats, void* dx, int64_t lddx,
                       leco_stream_t stream);
/* 1 if leco_groupnorm_fwd handles this shape in one launch, 0 if it takes three (statistics, finish, apply) */
int leco_groupnorm_single_launch(int32_t batch, int32_t hw, int32_t c, int32_t groups);
/* GroupNorm forward from per-(sample, channel) {sum, sumsq} statistics that the producers of x0 / x1 left behind
 * (leco_gemm_args.col_stats, or leco_colstats for tensors whose producer has no such epilogue): ONE pass over x, no
 * reduction over pixels.  cstats0: fp32 [batch][(c0 or c) / atom][2] for x0's channels, cstats1: [batch][(c - c0) / atom][2]
 * for x1's; atom divides c0 and c / groups.  Also writes stats[b][g] = {sum, sumsq} per group, which leco_groupnorm_bwd
 * expects. */
int leco_groupnorm_apply_stats(const void* x0, int64_t ld0, const void* x1, int64_t ld1, int32_t c0, const float* cstats0,
                               const float* cstats1, int32_t atom, const float* gamma, const float* beta, int32_t batch,
                               int32_t hw, int32_t c, int32_t groups, float eps, int32_t act, float* stats, void* y,
                               int64_t ldy, leco_stream_t stream);
/* col_stats[b][ch / atom] += {sum, sumsq} over the hw rows of sample b of a bf16 [batch * hw][c] tensor (row stride ld) */
int leco_colstats(const void* x, int64_t ld, float* col_stats, int32_t atom, int32_t batch, int32_t hw, int32_t c,
                  leco_stream_t stream);
int leco_layernorm_fwd(const void* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                       int32_t m, int32_t c, void* y, int64_t ldy, float* mean, float* rstd,
                       leco_stream_t stream);
/* dx = LayerNorm dgrad (+ dres if not NULL: the residual-branch gradient) */
int leco_layernorm_bwd(const void* x, int64_t ldx, const void* dy, int64_t lddy, const float* gamma,
                       const float* mean, const float* rstd, const void* dres, int64_t ldres,
                       int32_t m, int32_t c, void* dx, int64_t lddx, leco_stream_t stream);

/* ------------------------------------------------------------------------
 * Attention core softmax(Q K^T * scale) V per (batch, head); replaces diffusers' Attention
 * processor / xformers memory_efficient_attention (train_lora.py:68).  q/k/v/o are bf16 with
 * token stride ld* and batch stride bs* (elements); head h occupies columns [h*d, (h+1)*d).
 * lse: fp32 [batch][heads][sq] (log-sum-exp of the scaled scores), needed by the backward.
 * head_dim in {32, 40, 64, 80, 160}; leco_attention_fwd alone also takes 128 and 512 (one wide head: the VAE decoder's
 * mid-block attention), where lse may be NULL.  No score matrix exists in global memory at any sq / skv.
 * ---------------------------------------------------------------------- */
int leco_attention_fwd(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk,
                       int64_t bsk, const void* v, int64_t ldv, int64_t bsv, void* o, int64_t ldo,
                       int64_t bso, float* lse, int32_t batch, int32_t heads, int32_t sq,
                       int32_t skv, int32_t head_dim, float scale, leco_stream_t stream);
/* dQ, dK, dV from dO (flash backward, recomputing P from lse).  delta: fp32 [batch][heads][sq]
 * scratch.  No atomics: dQ and dK/dV are produced by two deterministic kernels. */
int leco_attention_bwd(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk,
                       int64_t bsk, const void* v, int64_t ldv, int64_t bsv, const void* o,
                       int64_t ldo, int64_t bso, const void* d_o, int64_t lddo, int64_t bsdo,
                       const float* lse, float* delta, void* dq, int64_t lddq,
                       int64_t bsdq, void* dk, int64_t lddk, int64_t bsdk, void* dv, int64_t lddv,
                       int64_t bsdv, int32_t batch, int32_t heads, int32_t sq, int32_t skv,
                       int32_t head_dim, float scale, leco_stream_t stream);

/* Causal self-attention core softmax(Q K^T * scale + causal) V per (batch, head): key j contributes to query i only for
 * j <= i.  Replaces the attention of transformers' CLIPTextModel layers (text_encoder(...) in train_util.py:32-62).  Same
 * operand convention as leco_attention_fwd (bf16, token stride ld*, batch stride bs*, head h in columns [h*d, (h+1)*d);
 * q | k | v may be column views of one fused [B][S][3C] buffer); one sequence length s for queries and keys,
 * 1 <= s <= LECO_CAUSAL_ATTN_MAX_S, head_dim == 64.  bf16 MFMA, fp32 accumulation and softmax; no score matrix in global
 * memory; a workgroup owns 16 query rows and stages only the keys up to its last row: key tiles above the diagonal are
 * never read, the tile on the diagonal is masked per element. */
#define LECO_CAUSAL_ATTN_MAX_S 128
int leco_attention_causal_fwd(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk, int64_t bsk,
                              const void* v, int64_t ldv, int64_t bsv, void* o, int64_t ldo, int64_t bso, int32_t batch,
                              int32_t heads, int32_t s, int32_t head_dim, float scale, leco_stream_t stream);

/* ------------------------------------------------------------------------
 * Elementwise / small kernels.
 * ---------------------------------------------------------------------- */
/* Row gather (+ periodic add): out[i][:] = table[idx[i]][:] (+ pos[i % period][:]), i < n; table / pos / out bf16 with row
 * strides ldt / ldp / ldo (multiples of 8), c % 8 == 0, the sum formed in fp32 and rounded once.  idx: DEVICE int32 [n],
 * every entry in [0, rows) (the caller validates; the kernel clamps, it never reads outside the table).  With pos it is
 * CLIPTextEmbeddings (token_embedding(ids) + position_embedding, period = sequence length); with pos == NULL it gathers
 * the EOS row of each sample for the pooled output (last_hidden_state[arange(B), eos_pos]). */
int leco_embed_rows(const void* table, int64_t ldt, int32_t rows, const int32_t* idx, const void* pos, int64_t ldp,
                    int32_t period, void* out, int64_t ldo, int32_t n, int32_t c, leco_stream_t stream);

/* ------------------------------------------------------------------------
 * CLIP image tower and CLIP score (leco_amd/clip_vision.py; csrc/vision.hip).
 * ---------------------------------------------------------------------- */
/* transformers' CLIPImageProcessor + the patch flattening in one pass: img uint8 NHWC [batch][h][w][3] (any h, w >= 1) ->
 * out bf16 [batch * P][ldo], P = (image_size / patch_size)^2, row b * P + py * (image_size / patch_size) + px = patch
 * (py, px) of picture b; column c * p * p + i * p + j = channel c, pixel (i, j) of the patch (the flattening of
 * patch_embedding.weight[out][3][p][p]); columns [3 p p, Kp) with Kp = 3 p p rounded up to a multiple of 64 are written as
 * zeros (leco_gemm needs k % 64 == 0); ldo >= Kp, ldo % 8 == 0.
 * The picture is resized so that its shortest edge is image_size with PIL's antialiased bicubic filter, centre-cropped to
 * image_size x image_size, scaled by 1/255 and normalised, value = (level / 255 - mean[c]) / std[c].  The filter is
 * separable; the caller passes it as two DEVICE tap tables that hold only the output rows / columns that survive the crop:
 *   row_tab int32 [image_size][2] = (first source row, tap count <= row_taps), row_w fp32 [image_size][row_taps],
 *   col_tab / col_w / col_taps likewise for the columns (`clip_vision.resize_taps`: PIL's precompute_coeffs rule).
 * Per output pixel: the column taps along every source row of its window (that sum clamped to [0, 255], PIL's 8-bit
 * intermediate picture saturates), then the row taps over those sums (clamped to [0, 255] again).  All arithmetic from the
 * source bytes to the one final bf16 rounding is fp32: PIL's two roundings to whole levels are not made.  A table entry
 * that points outside the picture is clamped into it, never followed.  mean_std: DEVICE fp32 [6] = mean[3], std[3]. */
int leco_clip_preprocess(const void* img, int32_t batch, int32_t h, int32_t w, const int32_t* row_tab, const float* row_w,
                         int32_t row_taps, const int32_t* col_tab, const float* col_w, int32_t col_taps,
                         const float* mean_std, int32_t image_size, int32_t patch_size, void* out, int64_t ldo,
                         leco_stream_t stream);
/* CLIPVisionEmbeddings after the patch GEMM: out[b][0][:] = cls[:] + pos[0][:], out[b][1 + t][:] = patches[b][t][:] +
 * pos[1 + t][:]; patches bf16 [batch * tokens][ldp], cls bf16 [c], pos bf16 [tokens + 1][ldpos], out bf16
 * [batch * (tokens + 1)][ldo].  c % 8 == 0, strides multiples of 8; the sum is formed in fp32 and rounded once. */
int leco_vit_embed(const void* patches, int64_t ldp, const void* cls, const void* pos, int64_t ldpos, void* out, int64_t ldo,
                   int32_t batch, int32_t tokens, int32_t c, leco_stream_t stream);
/* out[b][t] = scale * <x_b, y_t> / (max(|x_b|, 1e-12) * max(|y_t|, 1e-12)): x bf16 [nb][ldx], y bf16 [nt][ldy], out fp32
 * [nb][ldo]; d % 8 == 0, ldx / ldy multiples of 8; the three sums in fp32, one wave per pair.  scale = 1: the cosines (the
 * CLIP score); scale = exp(logit_scale): transformers' logits_per_image.  An all-zero row gives 0. */
int leco_cosine_scores(const void* x, int64_t ldx, const void* y, int64_t ldy, float* out, int64_t ldo, int32_t nb, int32_t nt,
                       int32_t d, float scale, leco_stream_t stream);

/* ------------------------------------------------------------------------
 * Cross-attention token heatmaps (leco_amd/attn_maps.py, `Engine.plan(attn_maps=M)`; csrc/attn_maps.hip).
 * ---------------------------------------------------------------------- */
/* DAAM-style token maps from the Q and K operands of one cross-attention:
 *   maps[b][m][i] += step_w[0] / heads * sum_h sum_j tok_w[m][j] * softmax_j(scale * <q_bhi, k_bhj>)
 * q, k: bf16 in the operand convention of leco_attention_fwd (token stride ld*, batch stride bs*, head h in columns
 * [h*d, (h+1)*d)), 16-byte aligned, strides multiples of 8; k may be a column view of the [B*skv][k|v] buffer `attn2.kv`
 * writes.  tok_w: DEVICE fp32 [n_maps][skv], 1 <= n_maps <= 8 (a word of several tokens = a row with several ones).
 * step_w: DEVICE fp32 [1], read when the launch RUNS (a captured graph weights or mutes a step without a new capture).
 * maps: fp32 [batch][n_maps][sq], accumulated in place.  The kernel forms its own row maximum and row sum (all skv <= 128
 * keys of a row are one tile; no lse buffer is read); Q K^T on the bf16 MFMAs with fp32 accumulation, everything from the
 * scores to the store in fp32 (no P is rounded to bf16).  Every (b, m, i) has exactly one owner and the heads are summed in a
 * fixed order: no atomics, two runs give equal bits.  Key columns past skv are masked by selection (whatever lies behind
 * the last key row, a NaN included, never reaches the output); rows past sq are neither read nor written.
 * head_dim in {40, 64, 80, 160} (the cross-attention widths of SD1.x / SD2.x / SDXL) or 32 (the synthetic tiny models),
 * 1 <= skv <= 128, any sq >= 1; anything else is -EINVAL with leco_last_error set, and nothing is launched. */
int leco_xattn_token_maps(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk, int64_t bsk,
                          const float* tok_w, int32_t n_maps, const float* step_w, float* maps, int32_t batch,
                          int32_t heads, int32_t sq, int32_t skv, int32_t head_dim, float scale, leco_stream_t stream);
/* heat[p][y][x] = sum_l weight_l * bilinear(map_l[p] -> ht x wt)(y, x), p < planes (= samples x words): `layers` is a DEVICE
 * table of n_layers entries, map_l fp32 [planes][h_l][w_l], any h_l, w_l, ht, wt >= 1.  The bilinear rule is
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False): source index max((in / out) (dst + 0.5) - 0.5, 0),
 * the upper tap clamped to the last row / column; fp32 throughout, layers added in table order. */
typedef struct leco_attn_map_layer {
    const float* map;
    int32_t h, w;
    float weight;
} leco_attn_map_layer;
int leco_attn_maps_merge(const leco_attn_map_layer* layers, int32_t n_layers, float* heat, int32_t planes, int32_t ht,
                         int32_t wt, leco_stream_t stream);
/* Heat map `map_index` of every sample blended over its picture: heat fp32 [batch][n_maps][ht][wt], rmax DEVICE fp32
 * [batch * n_maps] (the reciprocal of the value that maps to full heat, per map), pic / out uint8 [batch][ht][wt][3], lut
 * DEVICE uint8 [256][3] (the colour table), 0 <= alpha <= 1.  Per pixel, in fp32:
 *   v = min(max(heat * rmax, 0), 1)  (a NaN gives 0),  c = lut[floor(255 v + 0.5)],
 *   out = floor(pic * (1 - alpha v) + c * (alpha v) + 0.5)     -- round half up, the sum clamped to [0, 255] first. */
int leco_heat_overlay(const float* heat, const float* rmax, const void* pic, const void* lut, void* out, int32_t batch,
                      int32_t n_maps, int32_t map_index, int32_t ht, int32_t wt, float alpha, leco_stream_t stream);

/* ------------------------------------------------------------------------
 * Picture against picture: SSIM, squared error, change map (leco_amd/image_metrics.py; csrc/image_metrics.hip).
 * ---------------------------------------------------------------------- */
/* a: uint8 NHWC [batch][h][w][3]; ref: the same layout, picture b read at ref + b * ref_stride BYTES: ref_stride = 0 compares
 * every picture with ONE baseline, ref_stride = h * w * 3 compares pairwise.  taps: DEVICE fp32 [11], the normalised
 * Gaussian window (sigma = 1.5) computed on the host in float64 and rounded once (`image_metrics.gaussian_taps`); the window
 * is symmetric and taps[0..5] are what is read; no exp is evaluated on the device.
 * SSIM is Wang et al. 2004: per channel, the 11 x 11 separable window, biased moments, C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2,
 *   ssim = (2 ma mr + C1)(2 sar + C2) / ((ma^2 + mr^2 + C1)(saa + srr + C2)),
 * a pixel's value = the mean over the three channels, defined on the valid region only: the (h - 10) x (w - 10) pixels whose
 * whole window lies inside the picture.
 *   stats: DEVICE double [batch][2]; stats[b][0] = the mean SSIM over the valid region, stats[b][1] = the sum over ALL pixels
 *     and channels of (a - ref)^2, an exact integer (PSNR and MSE are the host's to derive);
 *   change_map (may be NULL): fp32 [batch][h][w] = 1 - ssim at the window's centre on the valid region, exactly 0 on the
 *     5-pixel border.  It is not clamped: rounding can leave a value a few 1e-7 below 0.
 * The moments are formed from centred levels (level - 128) in fp64; against a float64 statement with float64 taps an SSIM
 * value differs by at most 5e-4 (the rounding of the taps to fp32; DESIGN.md, "Image metrics").  a == ref gives a mean SSIM of
 * exactly 1.0 and a change map of exactly 0.  Every output element has one owner, the per-picture sums are added from
 * per-workgroup partials in a fixed order by a second launch: no atomics, two runs give equal bits.
 * workspace: DEVICE scratch of at least leco_image_compare_workspace(batch, h, w) bytes, 8-byte aligned; no state is kept in
 * it between calls.  h < 11, w < 11, batch < 1 (or > 65535), a ref_stride that is neither 0 nor h * w * 3, or a workspace
 * that is too small: -EINVAL with leco_last_error set, and nothing is launched. */
int leco_image_compare(const void* a, const void* ref, int64_t ref_stride, int32_t batch, int32_t h, int32_t w,
                       const float* taps, float* change_map, double* stats, void* workspace, int64_t workspace_bytes,
                       leco_stream_t stream);
/* bytes of workspace leco_image_compare needs (0 for arguments it refuses) */
int64_t leco_image_compare_workspace(int32_t batch, int32_t h, int32_t w);

/* GEGLU (diffusers FeedForward ff.net.0): y[m][f] = u[m][f] * gelu_erf(u[m][F+f]) */
int leco_geglu_fwd(const void* u, int64_t ldu, void* y, int64_t ldy, int32_t m, int32_t f,
                   leco_stream_t stream);
int leco_geglu_bwd(const void* u, int64_t ldu, const void* dy, int64_t lddy, void* du, int64_t lddu,
                   int32_t m, int32_t f, leco_stream_t stream);
/* out = a + b (+ c) on row-strided bf16 matrices (gradient fan-in at residual/skip joins) */
int leco_add(const void* a, int64_t lda, const void* b, int64_t ldb, const void* c, int64_t ldc,
             void* out, int64_t ldo, int32_t m, int32_t cols, leco_stream_t stream);
/* dgrad of F.interpolate(scale=2, nearest) (Upsample2D): dx = 2x2 block sums of dy */
int leco_upsample2x_bwd(const void* dy, void* dx, int32_t batch, int32_t h, int32_t w, int32_t c,
                        leco_stream_t stream);
/* UNet conv_in: NCHW bf16 (batch,cin,h,w) -> channels-last bf16; w fp32 [cin][3][3][cout] */
int leco_conv_in(const void* x, const float* w, const float* bias, void* y, int32_t batch, int32_t h,
                 int32_t wd, int32_t cin, int32_t cout, leco_stream_t stream);
/* UNet conv_out: channels-last bf16 -> NCHW fp32 (batch,4,h,w); w bf16 [4][3][3][c]; and its dgrad */
int leco_conv_out(const void* x, const void* w, const float* bias, float* y, int32_t batch, int32_t h,
                  int32_t wd, int32_t c, int32_t cout, leco_stream_t stream);
int leco_conv_out_bwd(const float* dy, const void* w, void* dx, int32_t batch, int32_t h, int32_t wd,
                      int32_t c, int32_t cout, leco_stream_t stream);
/* VAE decoder entry (post_quant_conv of `decode`, with the division by the scaling factor folded in): a 1x1 convolution on
 * the latents, y[b][o][p] = bias[o] + sum_c w[o][c] * (in_scale * x[b][c][p]); x fp32 NCHW (batch,cin,hw), w fp32 [cout][cin],
 * y bf16 NCHW (batch,cout,hw) -- the input layout of leco_conv_in. */
int leco_latent_affine(const float* x, const float* w, const float* bias, void* y, int32_t batch, int32_t hw, int32_t cin,
                       int32_t cout, float in_scale, leco_stream_t stream);
/* VAE decoder conv_out with the image epilogue: channels-last bf16 [batch*h*w][c] -> 3x3 pad 1, 3 outputs (RGB); w bf16
 * [3][3][3][c], bias fp32 [3], c % 32 == 0.  Writes either or both (the other NULL) of y: fp32 NCHW (batch,3,h,w), the
 * pre-rounding result, and img: uint8 NHWC (batch,h,w,3) = floor(clamp(y / 2 + 0.5, 0, 1) * 255 + 0.5). */
int leco_conv_out_rgb(const void* x, const void* w, const float* bias, float* y, void* img, int32_t batch, int32_t h,
                      int32_t wd, int32_t c, leco_stream_t stream);
/* VAE encoder conv_in: 3x3 pad 1 from a 3-channel image to channels-last bf16 [batch*h*w][cout], cout % 32 == 0.  The image
 * comes from exactly one of x: fp32 NCHW (batch,3,h,w), values in [-1, 1], and img: uint8 NHWC (batch,h,w,3), meaning the
 * fp32 number (float)p / 127.5f - 1.f, so that img and x = img / 127.5 - 1 give the same bits (the other NULL; both or
 * neither: -EINVAL).  w fp32 [cout][3][3][3] (the Conv2d layout: channel, kh, kw), bias
 * fp32 [cout].  fp32 accuracy before the single bf16 rounding of the output; padding taps are exactly 0 in the normalised
 * space. */
int leco_conv_in_rgb(const float* x, const void* img, const float* w, const float* bias, void* y, int32_t batch, int32_t h,
                     int32_t wd, int32_t cout, leco_stream_t stream);
/* VAE encoder exit: channels-last bf16 [batch*h*w][c] (c % 32 == 0) -> 3x3 pad 1 conv to 8 channels (w bf16 [8][3][3][c], bias
 * fp32 [8]) -> quant_conv as an fp32 8x8 matrix qw [out][in] + bias qb [8] on the fp32 accumulators.  Writes either or both
 * (not neither) of moments: fp32 NCHW (batch,8,h,w) = [mean | logvar], and latents: fp32 NCHW (batch,4,h,w) =
 * scale * (mean + exp(0.5 * clamp(logvar, -30, 20)) * noise), noise fp32 NCHW (batch,4,h,w); noise == NULL gives the mode,
 * scale * mean. */
int leco_conv_out_moments(const void* x, const void* w, const float* bias, const float* qw, const float* qb, const float* noise,
                          float* moments, float* latents, float scale, int32_t batch, int32_t h, int32_t wd, int32_t c,
                          leco_stream_t stream);
/* diffusers Timesteps(flip_sin_to_cos=True, freq_shift=0): out[i] = [cos | sin](t_i * f), bf16
 * [n][dim]; t_i = t_table[*idx + i*t_stride] (idx may be NULL => 0): the timestep is read on
 * the device so a captured graph can be replayed for every denoising step. */
int leco_timestep_embedding(const float* t_table, const int32_t* idx, int32_t t_stride, int32_t n,
                            int32_t dim, void* out, leco_stream_t stream);
int leco_advance(int32_t* counter, leco_stream_t stream);
/* predict_noise's guidance combine (train_util.py:163-166) fused with DDIMScheduler.step
 * (train_util.py:190): eps = u + g (c - u); x <- coef[step][0] x + coef[step][1] eps; also writes
 * the next UNet input cat([x]*2) as bf16 (train_util.py:151). */
int leco_cfg_ddim_step(const float* pred, float* x, void* x2, const float* coef, const int32_t* step,
                       float guidance, int64_t half_n, leco_stream_t stream);

/* Same role for the other schedulers the reference accepts (ddpm / lms / euler_a, model_util.py:247-274), all linear
 * in (sample, model output, fresh noise, previous derivatives).  coef: fp32 [steps][LECO_SCHED_ROW] rows
 * {c_x, c_e, c_n, c_h1, c_h2, c_h3, s_in, d_x, d_e, -, -, -}:
 *   x' = c_x x + c_e out + c_n noise + sum_j c_hj h_j        (out = CFG-combined raw prediction, or 0 if pred == NULL)
 *   d  = d_x x + d_e out, history h1 <- d, h2 <- h1, h3 <- h2  (hist: fp32 [n_hist][half_n], n_hist = 0..3)
 *   x2 = bf16(s_in x') twice = next UNet input (scale_model_input of the NEXT step, train_util.py:153).
 * noise (fp32 [half_n]) may be NULL for deterministic schedulers. */
#define LECO_SCHED_ROW 12
int leco_cfg_sched_step(const float* pred, float* x, void* x2, const float* coef, const int32_t* step,
                        float guidance, int64_t half_n, const float* noise, float* hist, int32_t n_hist,
                        leco_stream_t stream);
/* PromptEmbedsPair.loss (prompt_util.py:107-148) with MSELoss(mean) on device in fp32, plus
 * d loss / d (raw target-pass UNet output) (train_lora.py:279 first autograd step). */
int leco_esd_loss(const float* tgt, const float* pos, const float* neu, const float* unc, float g_pred,
                  float g_loss, float sign, int64_t half_n, float* loss, float* dpred,
                  leco_stream_t stream);
/* The same objective on CONDITIONAL-ONLY predictions (fp32 [half_n] each): at guidance_scale = 1 -- what the reference
 * passes for the three frozen passes and the target pass, train_lora.py:202-256 -- predict_noise's u + 1 (c - u)
 * (train_util.py:163-166) is c, so FusedStep's de-duplicated step never evaluates the unconditional halves.  pos_c / neu_c /
 * unc_c may alias (identical prompts are evaluated once).  dpred_c (may be NULL): d loss / d tgt_c. */
int leco_esd_loss_cond(const float* tgt_c, const float* pos_c, const float* neu_c, const float* unc_c, float g_loss,
                       float sign, int64_t half_n, float* loss, float* dpred_c, leco_stream_t stream);
/* torch.optim.AdamW step on the flat fp32 LoRA slab + refresh of its bf16 shadow
 * (train_lora.py:280).  hyper (device): {lr, 1-beta1^t, 1-beta2^t, grad_scale}. */
int leco_adamw(float* p, const float* g, float* m, float* v, void* shadow, const float* hyper,
               float beta1, float beta2, float eps, float wd, int64_t n, leco_stream_t stream);

/* Lion (`lion_pytorch.Lion`, selected by train.optimizer = "lion", train_util.py:362-365): p *= 1 - lr wd;
 * p -= lr sign(beta1 m + (1-beta1) g); m = beta2 m + (1-beta2) g.  Same hyper block ({lr, -, -, grad_scale}) and
 * bf16 shadow refresh as leco_adamw. */
int leco_lion(float* p, const float* g, float* m, void* shadow, const float* hyper, float beta1, float beta2,
              float wd, int64_t n, leco_stream_t stream);
/* Prodigy (Mishchenko & Defazio 2023, as released in prodigyopt 1.0; selected by train.optimizer = "prodigy",
 * train_util.py:366-370): Adam whose step size d lr is ESTIMATED -- d grows from d0 by the ratio of two sums over ALL
 * parameters, so `lr` stays at 1.  The reference's prepare_optimizer_params() is one param group: one pass over the flat
 * slab is the published algorithm.  g = grad_scale * grad (+ weight_decay p when not decoupled),
 *   bc   = bias correction ? sqrt(1 - beta2^(k+1)) / (1 - beta1^(k+1)) : 1,   dlr = d lr bc   (d BEFORE this step)
 *   lr > 0:  num = beta3 d_numerator + (d/d0) dlr sum g (p0 - p)
 *            exp_avg = beta1 exp_avg + d (1-beta1) g,  exp_avg_sq = beta2 exp_avg_sq + d^2 (1-beta2) g^2
 *            s = beta3 s + (d/d0) (safeguard warmup ? d : dlr) g,  den = sum |s|        (lr <= 0: den = 0)
 *   den == 0: p, d, k stay (d_numerator keeps the decayed value).  Otherwise, for lr > 0: d_hat = d_coef num / den,
 *            d = max(d, d_hat) while d is still d0, d_max = max(d_max, d_hat), d = min(d_max, d growth_rate); then
 *   p *= 1 - weight_decay dlr (decoupled),  p -= dlr exp_avg / (sqrt(exp_avg_sq) + d eps)   (NEW d, this step's dlr),  k += 1.
 * Two launches, no host round trip: the first updates exp_avg / exp_avg_sq / s and reduces the two sums (per-block
 * partials added in a fixed order by the last block to finish: bitwise reproducible, so data-parallel replicas derive the
 * same d) and updates *state; the second applies the update and refreshes the bf16 shadow.  The scalars are doubles:
 * d_numerator is an exponentially weighted sum over thousands of steps of terms that start near d0 = 1e-6 (the package
 * holds it as a Python float).  Start a run from {d0, d0, d0, 0, 0, d0, 0, 0}.  s, p0 (fp32 [n], caller-owned like the
 * moments): s starts at 0, p0 holds the parameters at the first Prodigy step.  hyper (device): {lr, -, -, grad_scale}.
 * beta3: the package's default is sqrt(beta2).  growth_rate may be +inf.  Launches on one device must be stream-ordered. */
typedef struct leco_prodigy_state {
    double d, d0, d_max, d_numerator, d_denom, d_hat, dlr, k;
} leco_prodigy_state;
enum { LECO_PRODIGY_DECOUPLE = 1, LECO_PRODIGY_BIAS_CORRECTION = 2, LECO_PRODIGY_SAFEGUARD_WARMUP = 4 };
int leco_prodigy(float* p, const float* g, float* exp_avg, float* exp_avg_sq, float* s, const float* p0, void* shadow,
                 const float* hyper, leco_prodigy_state* state, double beta1, double beta2, double beta3, double eps,
                 double weight_decay, double d_coef, double growth_rate, int32_t flags, int64_t n, leco_stream_t stream);
/* Global L2 norm of grad_scale * g over the flat gradient slab, and clipping through the optimizer's own grad_scale: runs
 * between the upload of `hyper` and leco_adamw / leco_lion / leco_prodigy, which read hyper[3] -- they need no change.
 * hyper: the optimizers' device block {lr, bc1, bc2, grad_scale}.
 * stats (device fp32[4]): {norm, coef, number of non-finite elements (inf or NaN bit patterns of g), 0}.
 *   norm = sqrt(sum_e ((double)g[e] * (double)hyper[3])^2), accumulated in double
 *   coef = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1     (torch.nn.utils.clip_grad_norm_'s arithmetic, in double;
 *          max_norm = 0: measure only; 1 as well when a non-finite element was seen: nothing is scaled then)
 *   hyper[3] <- (float)((double)hyper[3] * coef)   -- NOT written when coef == 1 or when a non-finite element was seen
 * One pass over g, one launch, no host round trip.  Per-block double partials added in a fixed order by the last block to
 * finish (the reduction of leco_prodigy): bitwise reproducible, so data-parallel replicas derive the same coef.  The
 * scratch is per device: launches on one device must be stream-ordered.  -EINVAL: a null operand, n <= 0, max_norm
 * negative or NaN. */
int leco_grad_clip(const float* g, int64_t n, float* hyper, float max_norm, float* stats, leco_stream_t stream);
/* acc = first ? g : acc + g  (fp32, elementwise; acc is not read when first != 0).  One launch per micro-step of a
 * gradient-accumulation group. */
int leco_grad_accumulate(float* acc, const float* g, int64_t n, int32_t first, leco_stream_t stream);
/* One LoRA module of the slab, for leco_lora_max_norm: lora_down = slab[down_off ..] as [r][k] (k = in_features, or
 * in * kh * kw of a convolution), lora_up = slab[up_off ..] as [n][r], both row-major; r is the module's own rank (after
 * the clamp of a narrow convolution), scale = alpha / r.  Offsets are in elements and need no alignment. */
typedef struct leco_lora_norm_module {
    int64_t down_off, up_off;
    int32_t r, k, n;
    float scale;
} leco_lora_norm_module;
/* Max-norm regularisation of the LoRA weights (train.scale_weight_norms), after the optimizer step, in one launch.
 * table: M modules, in DEVICE memory; slab / shadow: the fp32 master slab of n elements and its bf16 shadow.  Per module m
 *   norm_m  = scale_m * |up_m down_m|_F   from the two r x r Gram matrices, |U D|_F^2 = sum_ij (U^T U)_ij (D D^T)_ij,
 *             accumulated in double from the fp32 slab; the multiplier is not part of it
 *   ratio_m = norm_m <= max_norm ? 1 : max_norm / norm_m          (max_norm = 0: measure only, every ratio is 1)
 *   f_m     = (float)sqrt(ratio_m), the square root in double; where ratio_m < 1 every element of lora_down and lora_up is
 *             multiplied by f_m in fp32 in place and its shadow element rewritten with the optimizers' rounding (f2bf).
 *             Modules with ratio_m = 1 are not written at all.
 * A module whose norm is not finite (or whose table row does not lie inside the n elements) is left alone and counted.
 * Outputs (device fp32): norms[M] before scaling, factors[M] = f_m (exactly 1 where nothing was scaled), stats[4] =
 * {modules scaled, mean and maximum of norm_m * ratio_m over the modules with a finite norm, modules with a non-finite norm}.
 * One workgroup per module; fixed summation orders and no floating-point atomics: bitwise reproducible.  The scratch of
 * the statistics is per device: launches on one device must be stream-ordered.  -EINVAL: a null operand, n <= 0, M <= 0
 * or M > 8192, max_norm negative or NaN. */
int leco_lora_max_norm(float* slab, void* shadow, int64_t n, const leco_lora_norm_module* table, int32_t M, float max_norm,
                       float* norms, float* factors, float* stats, leco_stream_t stream);
int leco_cast_f32_bf16(const float* x, void* y, int64_t n, leco_stream_t stream);
int leco_memset(void* p, int32_t value, int64_t bytes, leco_stream_t stream);
/* dst = `reps` copies of the `bytes` (multiple of 16) at src, back to back: batch broadcast of a tensor that is identical for
 * several samples (the two halves of predict_noise's cat([latents] * 2), train_util.py:151, before the first use of the
 * prompt embeddings) */
int leco_repeat(const void* src, void* dst, int64_t bytes, int32_t reps, leco_stream_t stream);
/* Step glue of the reference loop body as two launches (the tensors the reference moves with framework ops between its
 * UNet calls, train_lora.py:175-199):
 *   leco_step_begin: x2 = cat([scale x] * 2) in the activation dtype (bf16, or fp32 when x2_is_f32) -- the first UNet input
 *     of `diffusion` (train_util.py:151-153,172-193; scale = scale_model_input of the first step, 1 for DDIM) -- and
 *     *t_idx = 0 (the denoising pass counter; may be NULL).
 *   leco_step_mid: after the k denoising passes the last UNet input IS cat([denoised] * 2); it becomes the input of the
 *     LoRA-on target pass (dst_a, may be NULL) and, `reps_b` times back to back, of the batched LoRA-off passes (dst_b)
 *     (train_lora.py:202-256); `current_timestep` (train_lora.py:195-199) is stored into both plans' timestep tables
 *     (t_slot_*: the slot's address) and both step indices are pointed at that slot.  bytes: multiple of 16. */
int leco_step_begin(const float* x, void* x2, int32_t x2_is_f32, float scale, int64_t half_n, int32_t* t_idx,
                    leco_stream_t stream);
int leco_step_mid(const void* src, void* dst_a, void* dst_b, int64_t bytes, int32_t reps_b, float t_cur,
                  float* t_slot_a, float* t_slot_b, int32_t* t_idx_a, int32_t* t_idx_b, int32_t slot,
                  leco_stream_t stream);

/* ------------------------------------------------------------------------
 * Row-stripe fused transformer-block kernels (csrc/stripe.hip): forward-only, bf16, C = 320 (the 64^2 level of SD1.x /
 * SD2.x: head dim 40 or 64).  One workgroup owns 64 token rows for a whole chain of Linear / LayerNorm / cross-attention /
 * GEGLU operations of diffusers' BasicTransformerBlock + Transformer2DModel (call site train_util.py:156-160; LoRA term
 * lora.py:102-106): the residual stream stays in registers (fp32), the activation operand of every GEMM in LDS, the block's
 * weights stream once through registers in MFMA operand layout.  Replaces 14 of the per-op launches above per transformer block in the LoRA-on denoising passes
 * (train_util.py:172-193) and the batched LoRA-off predictions (train_lora.py:202-237); the differentiated pass keeps the
 * per-op kernels (it must save every intermediate).
 * ---------------------------------------------------------------------- */
typedef struct leco_xlin {     /* one Linear of a stripe chain: y = x W^T + bias (+ (x down^T) (scale up)^T) */
    const void* w;             /* bf16 [N][K], K contiguous */
    int64_t ldw;
    const float* bias;         /* fp32 [N] or NULL */
    const void* dn;            /* stacked lora_down rows, bf16 [t_rows][K] (leco_lora_site.dn_s); NULL = LoRA off */
    int64_t ld_dn;
    const void* up;            /* scale * lora_up, bf16 [N][32] (leco_lora_site.up_p; columns >= groups*r zero) */
    int64_t ld_up;
    int32_t t_rows;            /* 16 or 32: stacked rank rounded up to 16 */
    int32_t packed;            /* 1: w is stored in MFMA fragment order instead of row-major (frozen weights, re-laid once):
                                  element (n, k) at ((n / 16 * (K / 32) + k / 32) * 64 + (k % 32 / 8) * 16 + n % 16) * 8 + k % 8,
                                  i.e. the 16 rows x 32 columns a wave loads per k-step are ONE contiguous 1 KB block (8 whole
                                  cache lines per load instead of 16 half lines); needs ldw == K */
} leco_xlin;

/* A-stationary GEMM for the short-K / small-M Linears of the transformer blocks (csrc/xgemm.hip; forward-only plans):
 *   c = a lin.w^T (+ (a lin.dn^T)(lin.up)^T) + lin.bias (+ residual)
 * -- attn{1,2}.to_q / to_out.0, the fused q|k|v projection, Transformer2DModel.proj_in / proj_out below the 64^2 level
 * (diffusers' BasicTransformerBlock / Transformer2DModel via train_util.py:156-160; LoRA term lora.py:102-106).  The
 * workgroup's BM x K activation tile is staged in LDS once, lin.w streams global -> VGPR in MFMA fragment order
 * (lin.packed must be 1, lin.ldw == k), the LoRA down-projection rides along in the same K sweep.
 * Shapes: n % 128 == 0, k in {320, 640, 1280} (leco_xgemm_supported); BM = leco_xgemm_rows(k) rows per workgroup. */
typedef struct leco_xgemm_args {
    int32_t m, n, k;
    const void* a;             /* bf16 [m][k], row stride lda (multiple of 8) */
    int64_t lda;
    leco_xlin lin;
    const void* residual;      /* bf16 [m][n] or NULL, row stride ldr (multiple of 4) */
    int64_t ldr;
    void* c;                   /* bf16 [m][n], row stride ldc (multiple of 4) */
    int64_t ldc;
} leco_xgemm_args;
int leco_xgemm_supported(int32_t m, int32_t n, int32_t k);
int leco_xgemm_rows(int32_t k);
int leco_xgemm(const leco_xgemm_args* a, leco_stream_t stream);

/* 1 if the stripe kernels cover this shape (else the caller keeps the per-op launches) */
int leco_xblock_supported(int32_t c, int32_t heads, int32_t skv, int32_t rows_per_sample);

/* K / V of the cross-attention for the stripe kernels, once per step: kv = output of the fused to_k|to_v projection,
 * bf16 [batch * skv][2 C] (row stride ld_kv).  kp: bf16 [batch][heads][80][64] (zero padded); vt: bf16
 * [batch][heads][roundup(head_dim, 16)][96], V^T with the key order permuted to the MFMA operand order (+ a row of ones
 * when head_dim % 16 != 0: the softmax row sum then comes out of the PV product). */
#define LECO_XATTN_KP_ELEMS(batch, heads) ((int64_t)(batch) * (heads) * 80 * 64)
#define LECO_XATTN_VT_ELEMS(batch, heads, head_dim) ((int64_t)(batch) * (heads) * (((head_dim) + 15) / 16 * 16) * 96)
int leco_xattn_prep(const void* kv, int64_t ld_kv, void* kp, void* vt, int32_t batch, int32_t heads, int32_t skv,
                    int32_t head_dim, leco_stream_t stream);

/* Everything of a BasicTransformerBlock after its self-attention core, + Transformer2DModel.proj_out:
 *   h1 = to_out1(attn) + h_in;  q2 = to_q2(LN2(h1));  a2 = softmax(q2 K^T scale) V;  h2 = to_out2(a2) + h1;
 *   h3 = ff2(GEGLU(ff1(LN3(h2)))) + h2;  out = proj_out.w ? proj_out(h3) + res : h3.
 * ff1 carries the LECO_ACT_GEGLU row interleave (weights, bias and up: blocks of 64 value rows followed by their 64 gate
 * rows).  col_stats (optional): {sum, sumsq} of the stored bf16 values per sample and atom of stats_atom (even) columns,
 * like leco_gemm_args.col_stats. */
typedef struct leco_xblock_tail_args {
    int32_t m, c, heads, skv, rows_per_sample;
    int32_t src_rows;                    /* 0: attn / h_in / res have m rows.  Else (a multiple of 64 dividing m): they have
                                            src_rows rows and row r reads row r % src_rows -- samples that are identical up to
                                            the first use of the prompt (classifier-free-guidance duplicates) are computed once */
    const void* attn; int64_t ld_attn;   /* self-attention output, bf16 [m][c] */
    const void* h_in; int64_t ld_h;      /* residual stream entering the block, bf16 [m][c] */
    leco_xlin to_out1, to_q2, to_out2, ff1, ff2, proj_out;
    const float* ln2_g; const float* ln2_b; const float* ln3_g; const float* ln3_b;
    float ln_eps;
    const void* kp; const void* vt;      /* leco_xattn_prep */
    float attn_scale;                    /* head_dim^-0.5 */
    const void* res; int64_t ld_res;     /* proj_out residual (the Transformer2DModel input), bf16 [m][c] */
    void* out; int64_t ld_out;           /* bf16 [m][c] */
    float* col_stats; int32_t stats_atom;
} leco_xblock_tail_args;
int leco_xblock_tail(const leco_xblock_tail_args* args, leco_stream_t stream);

/* Everything of a Transformer2DModel BEFORE the self-attention core of its first BasicTransformerBlock:
 *   n = GroupNorm(x) from the statistics the producer of x left (gn_cstats: fp32 [batch][c / stats_atom][2] {sum, sumsq},
 *       leco_gemm_args.col_stats; NULL: x is already normalised);  h_out = proj_in(n);  qkv_out = to_q|to_k|to_v(LN1(h_out)).
 * qkv is the fused [3 c][c] projection (its stacked lora_down rows are shared by the three 320-column sweeps). */
typedef struct leco_xblock_head_args {
    int32_t m, c, rows_per_sample;
    const void* x; int64_t ld_x;                 /* bf16 [m][c] */
    const float* gn_cstats; int32_t stats_atom; int32_t groups;
    const float* gn_g; const float* gn_b; float gn_eps;
    leco_xlin proj_in, qkv;
    const float* ln1_g; const float* ln1_b; float ln_eps;
    void* h_out; int64_t ld_hout;                /* bf16 [m][c]: the residual stream entering the block */
    void* qkv_out; int64_t ld_qkv;               /* bf16 [m][3 c] */
} leco_xblock_head_args;
int leco_xblock_head(const leco_xblock_head_args* args, leco_stream_t stream);

/* ------------------------------------------------------------------------
 * hipGraph capture of a whole UNet pass (the reference issues ~10^4 eager kernel launches
 * per pass from Python; here a pass is one graph launch).
 * ---------------------------------------------------------------------- */
typedef void* leco_graph_t;
int leco_graph_begin_capture(leco_stream_t stream);
int leco_graph_end_capture(leco_stream_t stream, leco_graph_t* out);
int leco_graph_launch(leco_graph_t graph, leco_stream_t stream);
int leco_graph_destroy(leco_graph_t graph);

/* ---- fp32 compute mode (`train.precision: float32`, config_util.py:75-83; csrc/f32.hip) --------------------------------
 * One twin per entry point above that touches activations: SAME argument list and meaning, but every tensor the bf16
 * entry point takes as bf16 (activations, packed weights, LoRA operand images) is fp32 here, strides still in elements.
 * Contractions run on the exact-fp32 MFMA (v_mfma_f32_16x16x4_f32); a whole SD1.5 UNet pass agrees with the fp32
 * reference to 3.7e-6.  Written for exactness, not speed. */
int leco_f32_gemm(const leco_gemm_args* args, leco_stream_t stream);
int leco_f32_attention_fwd(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk,
                       int64_t bsk, const void* v, int64_t ldv, int64_t bsv, void* o, int64_t ldo,
                       int64_t bso, float* lse, int32_t batch, int32_t heads, int32_t sq,
                       int32_t skv, int32_t head_dim, float scale, leco_stream_t stream);
int leco_f32_attention_bwd(const void* q, int64_t ldq, int64_t bsq, const void* k, int64_t ldk,
                       int64_t bsk, const void* v, int64_t ldv, int64_t bsv, const void* o,
                       int64_t ldo, int64_t bso, const void* d_o, int64_t lddo, int64_t bsdo,
                       const float* lse, float* delta, void* dq, int64_t lddq,
                       int64_t bsdq, void* dk, int64_t lddk, int64_t bsdk, void* dv, int64_t lddv,
                       int64_t bsdv, int32_t batch, int32_t heads, int32_t sq, int32_t skv,
                       int32_t head_dim, float scale, leco_stream_t stream);
int leco_f32_groupnorm_fwd(const void* x0, int64_t ld0, const void* x1, int64_t ld1, int32_t c0,
                       const float* gamma, const float* beta, int32_t batch, int32_t hw, int32_t c,
                       int32_t groups, float eps, int32_t act, float* stats, void* y, int64_t ldy,
                       leco_stream_t stream);
int leco_f32_groupnorm_bwd(const void* x0, int64_t ld0, const void* x1, int64_t ld1, int32_t c0,
                       const void* dy, int64_t lddy, const float* gamma, const float* beta,
                       const float* stats, int32_t batch, int32_t hw, int32_t c, int32_t groups,
                       float eps, int32_t act, float* bstats, void* dx, int64_t lddx,
                       leco_stream_t stream);
int leco_f32_layernorm_fwd(const void* x, int64_t ldx, const float* gamma, const float* beta, float eps,
                       int32_t m, int32_t c, void* y, int64_t ldy, float* mean, float* rstd,
                       leco_stream_t stream);
int leco_f32_layernorm_bwd(const void* x, int64_t ldx, const void* dy, int64_t lddy, const float* gamma,
                       const float* mean, const float* rstd, const void* dres, int64_t ldres,
                       int32_t m, int32_t c, void* dx, int64_t lddx, leco_stream_t stream);
int leco_f32_geglu_fwd(const void* u, int64_t ldu, void* y, int64_t ldy, int32_t m, int32_t f,
                   leco_stream_t stream);
int leco_f32_geglu_bwd(const void* u, int64_t ldu, const void* dy, int64_t lddy, void* du, int64_t lddu,
                   int32_t m, int32_t f, leco_stream_t stream);
int leco_f32_add(const void* a, int64_t lda, const void* b, int64_t ldb, const void* c, int64_t ldc,
             void* out, int64_t ldo, int32_t m, int32_t cols, leco_stream_t stream);
int leco_f32_upsample2x_bwd(const void* dy, void* dx, int32_t batch, int32_t h, int32_t w, int32_t c,
                        leco_stream_t stream);
int leco_f32_conv_in(const void* x, const float* w, const float* bias, void* y, int32_t batch, int32_t h,
                 int32_t wd, int32_t cin, int32_t cout, leco_stream_t stream);
int leco_f32_conv_out(const void* x, const void* w, const float* bias, float* y, int32_t batch, int32_t h,
                  int32_t wd, int32_t c, int32_t cout, leco_stream_t stream);
int leco_f32_conv_out_bwd(const float* dy, const void* w, void* dx, int32_t batch, int32_t h, int32_t wd,
                      int32_t c, int32_t cout, leco_stream_t stream);
int leco_f32_timestep_embedding(const float* t_table, const int32_t* idx, int32_t t_stride, int32_t n,
                            int32_t dim, void* out, leco_stream_t stream);
int leco_f32_cfg_ddim_step(const float* pred, float* x, void* x2, const float* coef, const int32_t* step,
                       float guidance, int64_t half_n, leco_stream_t stream);
int leco_f32_cfg_sched_step(const float* pred, float* x, void* x2, const float* coef, const int32_t* step,
                        float guidance, int64_t half_n, const float* noise, float* hist, int32_t n_hist,
                        leco_stream_t stream);
int leco_f32_cast_f32_bf16(const float* x, void* y, int64_t n, leco_stream_t stream);
int leco_f32_rowgroup_sum(const void* x, int64_t ldx, float* out, int64_t ldo, int32_t groups,
                      int32_t rows_per_group, int32_t cols, leco_stream_t stream);
int leco_f32_lora_pack(const leco_lora_site* sites, int32_t nsites, leco_stream_t stream);
int leco_f32_lora_wgrad(const void* p, int64_t ldp, const void* q, int64_t ldq, float* g,
                    int64_t g_sj, int64_t g_sc, int32_t m, int32_t r, int32_t cols, float scale,
                    float* part, int64_t part_bytes, leco_stream_t stream);
int leco_f32_lora_wgrad_conv(const void* p, int64_t ldp, const void* q, int64_t ldq, float* g, int64_t g_sj,
                         int64_t g_sc, int32_t m, int32_t r, int32_t cols, float scale, int32_t a_mode,
                         int32_t h_out, int32_t w_out, int32_t h_in, int32_t w_in, int32_t kh, int32_t kw,
                         float* part, int64_t part_bytes, leco_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LECO_HIP_H */
