/* libvlp_hip.so -- C ABI of the MI355X (gfx950) hot path of LuoweiZhou/VLP.
 *
 * The reference has no FFI/plugin layer: its seam is the Python class API of
 * pytorch_pretrained_bert/modeling.py + optimization*.py, underneath which apex / cuBLAS / torch
 * CUDA kernels run.  This header is the boundary a maintainer would bind (ctypes stub in
 * INTEGRATION.md) to replace those third-party kernels.  Each entry point cites the reference call
 * site(s) it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain C linkage, POD argument structs, raw DEVICE pointers, no torch types;
 *   - all floating tensors are IEEE fp16 ("half") unless a field says f32; accumulation is fp32;
 *   - the caller owns every buffer (the library never allocates or frees device memory); scratch is
 *     passed in and sized by the matching *_workspace_bytes() query;
 *   - `stream` is a hipStream_t; launches are asynchronous, no entry point synchronises the device;
 *   - re-entrant and thread-safe (backward runs on autograd worker threads);
 *   - return value: VLP_OK (0) or a negative vlp_status; vlp_last_error_string() returns the
 *     thread-local message of the last failure.  Nothing throws or aborts across the ABI.
 *   - dropout masks are a pure function of (seed, rng_stream, element index), so backward entry
 *     points regenerate them from the same triple instead of reading a stored mask.
 */
#ifndef VLP_HIP_H
#define VLP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VLP_ABI_VERSION 5      /* 5 (round 6): + vlp_dec_gemm, vlp_dec_reduce_ln, vlp_argmax_rows2 (no existing struct changed) */
/* + vlp_mlm_loss_ls_fwd / vlp_mlm_loss_ls_bwd with their own argument structs: purely additive (no existing struct or entry point
 * changed), so a binding written against version 5 keeps working and the version number stays 5. */
/* + vlp_scst_layout, vlp_embed_bwd_pos, vlp_token_logprob_fwd / vlp_token_logprob_bwd (self-critical sequence training), each with its own
 * argument struct: purely additive as well. */
/* + vlp_bce_sparse_loss_fwd / vlp_bce_sparse_loss_bwd, vlp_vqa_answer_rows (VQA 2.0 on real data: answer targets as (index, score) pairs):
 * purely additive as well. */
/* + vlp_cider_d / vlp_cider_d_workspace_bytes (the SCST reward on the device): purely additive as well. */
/* + vlp_cider_d_df / vlp_cider_d_df_workspace_bytes (the same reward with document frequencies from a resident table): purely additive as
 * well. */
/* + vlp_cider_d_multi / vlp_cider_d_multi_df with their workspace functions (2..16 hypotheses per group, leave-one-out reward) and
 * vlp_sample_rows_rep (several draws per logits row, seed in device memory): they take the existing structs; purely additive as well. */
/* + vlp_bleu4 (sentence BLEU-4 of the SCST hypotheses, mixed with the CIDEr-D scores, with the baseline) and its argument struct: purely
 * additive as well. */
/* + vlp_caption_eval / vlp_caption_eval_workspace_bytes (caption metrics of word strings: CIDEr-D, the BLEU integers, LCS for ROUGE-L) and
 * its argument struct: purely additive as well. */
/* + vlp_cider_d_consensus / vlp_cider_d_consensus_workspace_bytes (the K samples of an image scored against each other, the pick) and its
 * argument struct: purely additive as well. */
/* + vlp_live_rows_build, vlp_gemm_nt_rows, vlp_gemm_tn_grouped_rows, vlp_layernorm_bwd_rows (listed-row backward of the last encoder layer):
 * they take the existing argument structs plus the row list as separate arguments, so no struct grew: purely additive as well. */
/* + vlp_beam_select_groups (diverse beam search: the selection step with the beams in groups): it takes vlp_beam_select_args as it is plus two
 * scalars; purely additive as well. */
/* + vlp_logsoftmax_topk_want, vlp_beam_select_constrained (constrained beam search): the existing arguments plus separate ones, no struct grew;
 * purely additive as well. */
/* + vlp_kept_rows_build, vlp_gemm_tn_grouped_mapped (the dense step's grouped wgrad over a device map of the kept rows): they take
 * vlp_gemm_tn_args as it is plus the map and its device count; purely additive as well. */
/* + vlp_token_score (log-probability, entropy, rank and arg-max of a given token per logits row: scoring given captions) and its argument
 * struct: purely additive as well. */

typedef enum {
    VLP_OK = 0,
    VLP_ERR_BAD_ARG = -1,     /* shape / alignment / null pointer / unsupported configuration */
    VLP_ERR_HIP = -2,         /* a HIP runtime call or kernel launch failed */
    VLP_ERR_WORKSPACE = -3    /* workspace too small */
} vlp_status;

enum { VLP_ACT_NONE = 0, VLP_ACT_GELU = 1, VLP_ACT_RELU = 2, VLP_ACT_TANH = 3,
       VLP_ACT_GELU_SAVE_GRAD = 4 /* y = gelu(z), and `preact` receives gelu'(z) instead of z (z = fp16-rounded pre-activation) */ };
enum { VLP_MUL_NONE = 0, VLP_MUL_GELU_GRAD = 1, VLP_MUL_RELU_MASK = 2, VLP_MUL_PLAIN = 3 /* y *= mul_src (a stored derivative) */ };

int vlp_version(void);
const char* vlp_last_error_string(void);
/* 1 when the library was compiled with -DVLP_LAB_BUILD (tools/build_variant_lib.sh): the investigation variants of vlp_gemm_nt (phased
 * kernels, k32 ring, further wave-pipelined configurations), the two-kernel / exchange-tile attention backward and the stream-K grouped
 * wgrad are then present; the product library (0) launches its selected kernels and the fallback rings only. */
int vlp_lab_build(void);
/* Test hook: owner lookups of device pointers by the calling thread and how many of them asked the driver (the entry guard caches the
 * owner per allocation). */
void vlp_debug_device_lookup_stats(unsigned long long* lookups, unsigned long long* driver_queries);

/* ------------------------------------------------------------------------------------------------
 * Y[M,N] = epilogue( alpha * X[M,K] . W[N,K]^T )                      (fp16 in/out, fp32 accumulate)
 * epilogue order:  + bias[n] -> (store preact) -> act -> * mul(mul_src) -> dropout -> + residual
 * Replaces every nn.Linear forward on the path (modeling.py:270-272, 314, 341 + gelu :62-67, 354,
 * 415, 432, 481, 1003-1005, 1016, 1027-1029) with its bias/activation/dropout/residual glue
 * (:315-316, :355-356), and -- called with a transposed weight shadow as W -- the dgrad GEMMs of
 * autograd's LinearBackward, with gelu'/relu' fused through mul_mode.
 * Requirements: K % 64 == 0; ld* % 8 == 0; ldy (ldr, ldp, ldm) >= roundup8(N); 16-byte aligned bases.
 * Columns in [N, roundup8(N)) of Y / preact are written as 0.
 */
typedef struct {
    const void* X; int64_t ldx;          /* [M,K] */
    const void* W; int64_t ldw;          /* [N,K] */
    void* Y; int64_t ldy;                /* [M,N] */
    const void* bias;                    /* [N] or NULL */
    const void* residual; int64_t ldr;   /* [M,N] or NULL */
    void* preact; int64_t ldp;           /* [M,N] or NULL: value after bias, before act (fp16) */
    const void* mul_src; int64_t ldm;    /* [M,N] operand of mul_mode or NULL */
    int32_t M, N, K;
    int32_t act;                         /* VLP_ACT_* */
    int32_t mul_mode;                    /* VLP_MUL_*: GELU_GRAD multiplies by gelu'(mul_src), RELU_MASK by (mul_src > 0), PLAIN by mul_src */
    float alpha;
    float dropout_p; uint64_t seed; uint32_t rng_stream;
    int32_t variant;                     /* tile shape / staging of the launch; every variant computes the same bits (ascending-k fp32 chains:
                                            profiles/r04_nt_variant_identity.json).  Product library:
                                              value       tile      staging                                   used for
                                              0           128x128   register-staged, 2 stages                 default / tiny problems
                                              1, 2        128x128   LDS-DMA double buffer / single buffer     M <= 1024 (decoder, heads)
                                              3, 4        256x128   LDS-DMA double / single buffer            A/B
                                              5           256x256   LDS-DMA double buffer (16 waves)          A/B
                                              17, 19      128x128 / 256x128  4- / 3-stage LDS-DMA ring        skinny M / N <= 1024 fallback
                                              21          256x256   2-stage ring, one raw barrier per k tile  wide outputs (N > 1024)
                                              64+1, 64+5  256x256 / 256x128  wave-pipelined (gemm_nt_wp.hip)  N <= 1024: 64 + 5
                                              256         256x128   persistent k stream (gemm_nt_ps.hip)      QKV forward
                                            + 8 on any value = XCD-aware tile (run) order: the table uses 27 = 19 + 8, 29 = 21 + 8, 77, 264.
                                            A wave-pipelined / persistent variant whose epilogue or shape is not carried (erf / tanh epilogues;
                                            N % 128, K <= 512, 32-bit offsets) runs on the rings 27 / 29 instead: vlp_gemm_nt_resolved_variant().
                                            Investigation variants (6 / 7 phased, 53 k32 ring, other wave-pipelined configurations) exist in
                                            -DVLP_LAB_BUILD libraries only (vlp_lab_build()); the product library maps them to 27 / 29. */
    const int32_t* row_map;              /* ABI 4: [M] or NULL.  Padding-free (packed) runs: the dropout element of output (m, n) is
                                            (row_map[m], n) -- the row's LOGICAL index b*L + l -- so a packed run draws the masks of the
                                            dense run bit for bit.  NULL: row m itself. */
} vlp_gemm_nt_args;
int vlp_gemm_nt(const vlp_gemm_nt_args* a, void* stream);
/* The variant the calling thread's last vlp_gemm_nt launched after its fallbacks (a wave-pipelined variant without the requested
 * epilogue, or with operands beyond 32-bit offsets, and a persistent variant outside its epilogues / shapes, run on the rings 27 / 29);
 * -1 before the first call. */
int vlp_gemm_nt_resolved_variant(void);
/* Listed-row launches (the backward of the last encoder layer of a masked-LM step: only the masked rows carry gradient).  `live` is a device
 * int32 list of row indices, ascending and without duplicates, padded with -1 (vlp_live_rows_build): entry m >= 0 names the row of the big
 * [rows, *] buffers that compact row m stands for; a pad entry contributes nothing and its output row is not written. */
enum { VLP_ROWS_X = 1,    /* vlp_gemm_nt_rows: X row m is read at live[m];  vlp_gemm_tn_grouped_rows: A row m is read at live[m];
                             vlp_layernorm_bwd_rows: dy row m is read at live[m] */
       VLP_ROWS_MUL = 2,  /* mul_src row m is read at live[m] */
       VLP_ROWS_RES = 4,  /* residual row m is read at live[m] */
       VLP_ROWS_Y = 8     /* vlp_gemm_nt_rows: Y row m is written at live[m];  vlp_layernorm_bwd_rows: dx row m is written at live[m] */ };
/* live[0..n) = the distinct rows base(b) + clamp(pos[b, j]) of pos [B, P] (base / clamp as in vlp_gather_rows) in ascending order, the rest
 * of live[0..B*P) = -1; *count = n.  One workgroup; B*P <= 12288. */
int vlp_live_rows_build(const int64_t* pos, int32_t B, int32_t P, int32_t L, const int32_t* row_off, int32_t* live, int32_t* count, void* stream);
/* vlp_gemm_nt over the listed rows: a->M = entries of `live`; the operands named by `flags` (VLP_ROWS_*) are addressed at row live[m], the
 * others at row m.  Epilogues: bias, VLP_MUL_PLAIN / VLP_MUL_RELU_MASK, dropout (drawn at the logical row: a->row_map[live[m]], or live[m]),
 * residual.  One workgroup walks the whole K of its 128x128 tile in ascending order (the ring variant 17 of vlp_gemm_nt; no split-K), so a
 * listed output row has the bits that variant gives the same row in an unlisted launch. */
int vlp_gemm_nt_rows(const vlp_gemm_nt_args* a, const int32_t* live, int32_t flags, void* stream);
/* Split-K form for skinny problems (incremental decoding, M = 128..640 rows: only N/128 output tiles): the k range is cut into `splits`
 * slices computed by separate workgroups into an fp32 workspace of vlp_gemm_nt_splitk_workspace_bytes(M, N, splits) bytes; a second
 * kernel sums the slices in a fixed order (deterministic) and applies the same fused epilogue.  `variant` is ignored. */
int64_t vlp_gemm_nt_splitk_workspace_bytes(int32_t M, int32_t N, int32_t splits);
int vlp_gemm_nt_splitk(const vlp_gemm_nt_args* a, int32_t splits, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * dW[N,K] (+)= A[M,N]^T . B[M,K]          (wgrad: A = dY, B = layer input; contraction over rows M)
 * Replaces autograd's weight-gradient GEMMs for every nn.Linear above.
 * beta = 0 overwrites C, beta = 1 accumulates into it (gradient accumulation,
 * run_img2txt_dist.py:566-576).  Requirements: N % 8 == 0 is NOT required (rows n >= N are skipped)
 * but lda >= roundup8(N); K % 8 == 0; ld* % 8 == 0; 16-byte aligned bases.
 * workspace: vlp_gemm_tn_workspace_bytes(M,N,K) bytes of scratch (fp32 split-M partial slabs).
 */
typedef struct {
    const void* A; int64_t lda;          /* [M,N] */
    const void* B; int64_t ldb;          /* [M,K] */
    void* C; int64_t ldc;                /* [N,K] */
    int32_t M, N, K;
    int32_t beta;                        /* 0 or 1 */
    void* workspace; int64_t workspace_bytes;
    int32_t variant;                     /* 0 = ds_read_u16 fragment gathers, 1 = ds_read_b64_tr_b16 (register-staged), 2 = ds_read_b64_tr_b16 +
                                            LDS-DMA staging with a transpose-read swizzle, 128x128 tile; 3 / 4 = the same with
                                            256x128 / 128x256 (n x k) tiles (5 = 256x256 was removed in round 2: rejected); +8 = XCD-aware tile order,
                                            +16 = split-major tile order (with +8: one XCD per row range) */
    int32_t splits;                      /* 0 = choose automatically */
    void* bias_out;                      /* optional [N] fp16: (+)= column sums of A, i.e. the bias gradient of the same
                                            Linear, fused into the k-tile-0 workgroups (replaces a separate vlp_colsum) */
} vlp_gemm_tn_args;
int64_t vlp_gemm_tn_workspace_bytes(int32_t M, int32_t N, int32_t K);
int vlp_gemm_tn(const vlp_gemm_tn_args* a, void* stream);
/* Several weight gradients in ONE launch (1..8 problems; the four Linears of a BertLayer: modeling.py:270-272, 314, 341, 354).
 * Every 128x128 output tile of every problem is one workgroup that walks that problem's WHOLE contraction: no split-M slabs, no
 * reduce launches (`splits`, `variant` of the entries are ignored); `beta` and `bias_out` as in vlp_gemm_tn.
 * Stream-K form (VLP_TN_GROUP_MODE=5): with list[0].workspace / workspace_bytes >= vlp_gemm_tn_grouped_workspace_bytes(tiles) (tiles =
 * sum over the problems of ceil(N/128) * ceil(K/128); must be a multiple of 6, one M for all problems) the tiles are taken six at a
 * time and their contraction is dealt to seven workgroups in equal runs: every tile is cut once, its two fp32 partial chains meet
 * through the workspace (flags reset by a hipMemsetAsync ahead of the launch); without a workspace the launch runs in the plain form. */
int vlp_gemm_tn_grouped(const vlp_gemm_tn_args* list, int32_t count, void* stream);
int64_t vlp_gemm_tn_grouped_workspace_bytes(int32_t tiles);
/* The same launch with a row list per problem: live[i] (host array of `count` device pointers; NULL = problem i as in vlp_gemm_tn_grouped)
 * lists the contraction rows of problem i, M = entries of the list.  B row m is read at live[i][m]; A row m at live[i][m] when flags[i]
 * has VLP_ROWS_X, else at row m (compact dY).  Pad entries (-1) add nothing.  Rows are summed in list order. */
int vlp_gemm_tn_grouped_rows(const vlp_gemm_tn_args* list, const int32_t* const* live, const int32_t* flags, int32_t count, void* stream);
/* The same launch contracting over a device row map shared by all `n` problems (one M for all of them): the contraction is
 * sum over j < M' of A[map[j], :]^T . B[map[j], :] with M' = *count read on the device (clamped to [0, M]; map has M int32 entries, each
 * clamped to [0, M - 1]: a bad map gives wrong numbers, never a fault).  Rows the map does not name are never read.  Grid and tiles are those
 * of vlp_gemm_tn_grouped; a workgroup walks ceil(M' / 64) stages; with the identity map and M' = M the bits are those of
 * vlp_gemm_tn_grouped.  M' = 0 gives zeros at beta = 0 and leaves C at beta = 1.  Nothing on the host depends on M'. */
int vlp_gemm_tn_grouped_mapped(const vlp_gemm_tn_args* list, const int32_t* map, const int32_t* count, int32_t n, void* stream);
/* The map of the dense training step's kept rows: sample b keeps positions 0 .. n_b - 1 with n_b = 1 + the last key column any query of
 * the sample attends (maskb: the packed mask [B, L, Lp] of vlp_mask_pack / vlp_mask_build, byte 1 = attended) or lens_in[b] (exactly one of
 * maskb / lens_in is given), at least Nv + 2, at least max_j clamp(pos[b, j], 0, L - 1) + 1 (pos [B, P] or NULL), at most L.  Writes
 * lens[B] = n_b, map[0 .. M') = the dense rows b * L + l of the kept positions in ascending order (map[M' .. B * L) = B * L - 1) and
 * *count = M'.  B <= 8192. */
int vlp_kept_rows_build(const uint8_t* maskb, const int32_t* lens_in, const int64_t* pos, int32_t B, int32_t P, int32_t L, int32_t Lp,
                        int32_t Nv, int32_t* lens, int32_t* map, int32_t* count, void* stream);

/* out[n] (+)= sum_m A[m,n]  -- bias gradients (autograd SumBackward of the broadcast bias add). */
typedef struct {
    const void* A; int64_t lda; int32_t M, N;
    void* out;                           /* [N] fp16 */
    int32_t beta;
    void* workspace; int64_t workspace_bytes;   /* vlp_colsum_workspace_bytes(M,N) */
} vlp_colsum_args;
int64_t vlp_colsum_workspace_bytes(int32_t M, int32_t N);
int vlp_colsum(const vlp_colsum_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused masked-softmax attention.  qkv is the packed projection [B, L, 3*H] (q | k | v, head h at
 * column h*64 of each third); mask is the byte mask [B, L, Lp] produced by vlp_mask_pack
 * (1 = attend, 0 = masked -> additive -10000 exactly like modeling.py:807-833, 2 = padding); Lp = roundup32(L).
 * Forward replaces modeling.py:279-302 (transpose_for_scores, QK^T/sqrt(d), +mask, softmax, dropout,
 * PV, permute+contiguous); backward replaces the autograd of those ops.  head_dim must be 64,
 * L <= 256.  lse [B, heads, L] f32 is the per-row log-sum-exp saved for backward.
 */
typedef struct {
    const void* qkv; int64_t ld_qkv;     /* [B*L, 3H] */
    const uint8_t* mask;                 /* [B, L, Lp] */
    void* ctx; int64_t ld_ctx;           /* [B*L, H] out */
    float* lse;                          /* [B, heads, L] out */
    int32_t B, L, heads;
    float scale;                         /* 1/sqrt(head_dim) */
    float dropout_p; uint64_t seed; uint32_t rng_stream;
    const int32_t* row_off;              /* ABI 4: [B+1] or NULL.  Padding-free layout: sample b owns rows [row_off[b], row_off[b+1]) of
                                            qkv / ctx (its first n_b = row_off[b+1] - row_off[b] <= L positions; the dropped positions
                                            must be inert: attended by no kept query -- vlp_amd.engine derives n_b from the mask).  mask,
                                            lse and the dropout element (b, head, q, key) stay LOGICAL ([B, L, ..]).  NULL: row b*L + l. */
} vlp_attn_fwd_args;
int vlp_attn_fwd(const vlp_attn_fwd_args* a, void* stream);

/* Inference form of the same kernel for incremental decoding (modeling.py:1189-1253 with BertSelfAttention's history path
 * :273-277): Lq new query rows per sequence attend to Lk cached + new key/value rows that live in a separate K/V cache
 * (a TRUE K/V cache: the reference re-projects K and V over the whole history every step).  Row (b, i) of q is at
 * q + (b*q_rows_per_batch + i)*ld_q (+ 64*head); rows of k / v likewise with kv_rows_per_batch and ld_kv.
 * mask: bytes [B, Lq, roundup32(Lk)] as produced by vlp_mask_pack on the [B, Lq, Lk] slice of the attention mask.
 * ctx [B*Lq, heads*64].  No dropout, no statistics. */
typedef struct {
    const void* q; int64_t ld_q; int64_t q_rows_per_batch;
    const void* k; const void* v; int64_t ld_kv; int64_t kv_rows_per_batch;
    const uint8_t* mask;
    void* ctx; int64_t ld_ctx;
    int32_t B, Lq, Lk, heads;
    float scale;
    /* beam search: key/value rows [0, n_prefix) of sequence b are read from a cache SHARED by the `beams` sequences of one sample
     * (row b / beams of k_prefix / v_prefix, kv-style [*, prefix_rows_per_batch, ld_kv] layout), rows >= n_prefix from k / v.
     * The prefix (regions + [SEP]) is identical for all beams (select_beam_items only permutes generated positions), so it is
     * stored and streamed once per sample.  n_prefix = 0: everything comes from k / v. */
    const void* k_prefix; const void* v_prefix;
    int64_t prefix_rows_per_batch;
    int32_t n_prefix, beams;
} vlp_attn_decode_args;
int vlp_attn_decode(const vlp_attn_decode_args* a, void* stream);

typedef struct {
    const void* qkv; int64_t ld_qkv;
    const uint8_t* mask;
    const uint8_t* mask_t;               /* [B, Lp, Lp] key-major copy of the byte mask (vlp_mask_pack's second output) */
    const void* ctx; int64_t ld_ctx;     /* forward output */
    const void* dctx; int64_t ld_dctx;   /* [B*L, H] gradient of ctx */
    const float* lse;
    void* dqkv; int64_t ld_dqkv;         /* [B*L, 3H] out: dq | dk | dv */
    float* delta;                        /* [B, heads, L] f32 scratch */
    int32_t B, L, heads;
    float scale;
    float dropout_p; uint64_t seed; uint32_t rng_stream;
    const int32_t* row_off;              /* ABI 4: packed rows of qkv / ctx / dctx / dqkv, see vlp_attn_fwd_args; delta, lse, masks stay logical */
} vlp_attn_bwd_args;
int vlp_attn_bwd(const vlp_attn_bwd_args* a, void* stream);

/* int64 [B,L,L] 0/1 (seq2seq_loader.py:292-304) -> uint8 [B,L,Lp]: 1 attend, 0 masked, 2 for the padding
 * columns >= L (excluded from the softmax). */
/* out_t (optional, [B,Lp,Lp]): the key-major copy used by vlp_attn_bwd -- row `key` holds the flags of all queries, 2 wherever key >= L
 * or q >= L.  ABI 3: inside a row the byte of query q = 16 t + 4 g + e sits at g * (Lp / 4) + 4 t + e (the order in which a lane of the
 * backward kernel consumes them: its words are consecutive); treat the buffer as opaque, produced here and by vlp_mask_build only. */
int vlp_mask_pack(const int64_t* mask, uint8_t* out, uint8_t* out_t, int32_t B, int32_t L, int32_t Lp, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm, TF style (eps inside sqrt, biased variance, fp32 statistics): modeling.py:174-192 /
 * apex FusedLayerNorm.  y = dropout( gamma * (x - mean) * rstd + beta ).  H % 8 == 0, H <= 4096.
 */
typedef struct {
    const void* x; int64_t ldx;          /* [M,H] */
    const void* gamma; const void* beta; /* [H] */
    void* y; int64_t ldy;                /* [M,H] */
    float* mean; float* rstd;            /* [M] out (may be NULL for inference) */
    int32_t M, H; float eps;
    float dropout_p; uint64_t seed; uint32_t rng_stream;
    const int32_t* row_map;              /* ABI 4: [M] or NULL: dropout element of (m, c) is (row_map[m], c): packed rows, see vlp_gemm_nt_args */
} vlp_layernorm_fwd_args;
int vlp_layernorm_fwd(const vlp_layernorm_fwd_args* a, void* stream);

/* dx = LN'(x)·(drop(dy)); dgamma/dbeta (+)= column sums.  If dy_drop_p > 0 the incoming dy is first
 * multiplied by the forward's output-dropout mask.  If out_drop_p > 0 a second output
 * dx_drop = dx * mask(out_seed, out_stream) is written (the gradient that flows into the dropout
 * that FED the pre-LN sum: modeling.py:315-316, 355-356).
 */
typedef struct {
    const void* dy; int64_t lddy;
    const void* x; int64_t ldx;
    const void* gamma;
    const float* mean; const float* rstd;
    void* dx; int64_t lddx;
    void* dx_drop; int64_t lddxd;        /* optional */
    void* dgamma; void* dbeta;           /* [H] fp16 */
    int32_t M, H; int32_t beta;          /* beta: accumulate into dgamma/dbeta */
    float dy_drop_p; uint64_t dy_seed; uint32_t dy_stream;
    float out_drop_p; uint64_t out_seed; uint32_t out_stream;
    void* workspace; int64_t workspace_bytes;   /* vlp_layernorm_bwd_workspace_bytes(H) */
    int32_t defer_reduce;                /* 1: leave the per-block dgamma/dbeta partials in `workspace` and do NOT touch dgamma/dbeta;
                                            the caller reduces many LayerNorms at once with vlp_layernorm_bwd_reduce_batched */
    const int32_t* row_map;              /* ABI 4: [M] or NULL: both dropout masks are drawn at (row_map[m], c) (packed rows) */
} vlp_layernorm_bwd_args;
int64_t vlp_layernorm_bwd_workspace_bytes(int32_t H);
int vlp_layernorm_bwd(const vlp_layernorm_bwd_args* a, void* stream);
/* vlp_layernorm_bwd over the listed rows: a->M = entries of `live`; x / mean / rstd are read at row live[m], dy at live[m] with VLP_ROWS_X
 * (else at row m), dx is written at row live[m] with VLP_ROWS_Y (else at row m), dx_drop at row m; both dropout masks are drawn at the
 * logical row (a->row_map[live[m]], or live[m]).  The launch leaves as many partial rows in the workspace as vlp_layernorm_bwd with
 * M = part_M does (exact zeros in those that saw no row), so a deferred vlp_layernorm_bwd_reduce_batched over M = part_M stays complete. */
int vlp_layernorm_bwd_rows(const vlp_layernorm_bwd_args* a, const int32_t* live, int32_t flags, int32_t part_M, void* stream);
/* Second stage of `count` deferred vlp_layernorm_bwd calls in ONE launch (the 25 LayerNorms of a 12-layer step otherwise cost 25
 * tiny reduce launches): slot i of `parts` (stride = vlp_layernorm_bwd_workspace_bytes(H) / 4 floats) holds the partials of
 * LayerNorm i (all with the same M, H); dst[2*i] / dst[2*i+1] (device array of pointers) are its dgamma / dbeta ([H] fp16). */
int vlp_layernorm_bwd_reduce_batched(const float* parts, const void* const* dst, int32_t count, int32_t M, int32_t H, int32_t beta, void* stream);

/* ------------------------------------------------------------------------------------------------
 * mask_image_regions / vis_pretext_loss (modeling.py:1049-1056, 1113-1131; loader: seq2seq_loader.py:267-269, 303-304).
 * vlp_region_mask_build: vis_masked_pos [B, Pm] (int64, values 1..Nv) -> out [B*Nv] bytes, 1 on the masked region rows.
 * vlp_pretext_fwd: per sample b, with r_i = vis_masked_pos[b,i] - 1:  A_i = vispe_h[b, r_i] + pooled[b]  (rounded to fp16 like the
 *   reference's in-place add :1124),  V_j = vis_h[b, r_j],  sim = A . V^T ([Pm, Pm], rounded to fp16 like the half matmul :1126),
 *   probs = softmax(sim) rows (fp32, kept for backward),  sample_loss[b] = -mean_i log probs[i,i];  loss[0] = mean_b sample_loss[b]
 *   (:1127-1131; summed in a fixed order: bitwise reproducible).  Pm <= 64.
 * vlp_pretext_bwd: gscale[0] = upstream gradient of the pretext loss (x loss scale).  dsim = gscale / (B Pm) (probs - I);
 *   dA = dsim . V, dV = dsim^T . A.  Writes ONLY the masked rows of d_vis_h / d_vispe_h (through ReLU + dropout exactly as
 *   vlp_embed_bwd does for the other rows: y > 0 mask and the dropout multiplier of element (region row, col) of streams
 *   vis_stream / vispe_stream), and d_pooled_pre[b] = (sum_i dA_i) * (1 - pooled[b]^2) (backward of the pooler's tanh, :416).
 * Precondition of vlp_pretext_fwd / vlp_pretext_bwd: the Pm positions of a row of vis_masked_pos are DISTINCT and within 1..Nv, as the
 *   loader draws them without replacement (seq2seq_loader.py:267-269).  The loss takes the diagonal of `probs` as the target and
 *   vlp_pretext_bwd writes one row of d_vis_h / d_vispe_h per position: with a duplicate two work items store the same row and the
 *   diagonal is no longer the target, so duplicates are outside the contract and are not diagnosed.  A position outside 1..Nv is clamped
 *   to the nearest region by the two pretext kernels and ignored by vlp_region_mask_build (which is indifferent to duplicates).
 */
int vlp_region_mask_build(const int64_t* vis_masked_pos, int32_t B, int32_t Pm, int32_t Nv, uint8_t* out, void* stream);
typedef struct {
    const void* vis_h; const void* vispe_h;                 /* f16 [B*Nv, H] (post ReLU + dropout) */
    const void* pooled;                                     /* f16 [B, H] */
    const int64_t* vis_masked_pos;                          /* [B, Pm] */
    float* probs;                                           /* f32 [B, Pm, Pm] out */
    float* sample_loss;                                     /* f32 [B] out */
    float* loss;                                            /* f32 [1] out */
    int32_t B, Nv, Pm, H;
} vlp_pretext_fwd_args;
int vlp_pretext_fwd(const vlp_pretext_fwd_args* a, void* stream);
typedef struct {
    const void* vis_h; const void* vispe_h; const void* pooled;
    const int64_t* vis_masked_pos;
    const float* probs;                                     /* from vlp_pretext_fwd */
    const float* gscale;                                    /* device f32 [1] */
    void* d_vis_h; void* d_vispe_h;                         /* f16 [B*Nv, H]: masked rows written */
    void* d_pooled_pre;                                     /* f16 [B, H] out */
    int32_t B, Nv, Pm, H;
    float drop_p; uint64_t seed; uint32_t vis_stream; uint32_t vispe_stream;
} vlp_pretext_bwd_args;
int vlp_pretext_bwd(const vlp_pretext_bwd_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Embedding splice (modeling.py:217-236): pre[b,l,:] = word(l) + pos(l) + type[seg[b,l]] where for
 * l in [1, Nv] word(l) = vis_h[b,l-1] and pos(l) = vispe_h[b,l-1] (projected region features / box
 * encodings), else word = word_emb[input_ids[b,l]], pos = pos_emb[l].  (LayerNorm + dropout :239-240
 * are done by vlp_layernorm_fwd on `pre`.)
 */
typedef struct {
    const int64_t* input_ids; const int64_t* segment_ids;   /* [B,L] */
    const void* word_emb; const void* pos_emb; const void* type_emb;   /* [V,H] [P,H] [T,H] */
    const void* vis_h; const void* vispe_h;                 /* [B*Nv, H] */
    void* pre;                                              /* [B*L, H] out */
    int32_t B, L, Nv, H, vocab, type_vocab;
    const int64_t* position_ids;                            /* [B,L] or NULL (= 0..L-1); incremental decoding passes them (:856-865) */
    int32_t max_pos;                                        /* rows of pos_emb */
    const uint8_t* region_mask;                             /* ABI 3: [B*Nv] or NULL; 1 = this region row enters as zeros (word and position
                                                               stream; mask_image_regions, modeling.py:1049-1056), vlp_region_mask_build */
    const int32_t* row_map; int32_t rows;                   /* ABI 4: packed output: `pre` has `rows` rows, row p holds logical row row_map[p] = b*L + l
                                                               (input_ids / segment_ids / position_ids stay [B,L]).  NULL: rows = B*L, p = b*L + l */
} vlp_embed_fwd_args;
int vlp_embed_fwd(const vlp_embed_fwd_args* a, void* stream);

/* Backward of the splice: adds dpre into d_word_emb rows (no atomics: one owner per token id sums its rows in a fixed order in fp32, so
 * the result is bitwise reproducible), d_pos_emb, d_type_emb, and writes the region-row gradients.
 * d_vis_h = dpre * relu'(vis_h) * dropmask(vis), d_vispe_h = dpre * relu'(vispe_h) * dropmask(vispe) (backward of ReLU+Dropout,
 * modeling.py:1006-1007, 1017-1018).  acc32 is f32 scratch of vlp_embed_bwd_workspace_floats(B, L, Nv, H) floats; type_vocab <= 8; H <= 2048.
 */
int64_t vlp_embed_bwd_workspace_floats(int32_t B, int32_t L, int32_t Nv, int32_t H);
typedef struct {
    const void* dpre;                                       /* [B*L, H] */
    const int64_t* input_ids; const int64_t* segment_ids;
    const void* vis_h; const void* vispe_h;                 /* forward outputs (post ReLU+dropout) */
    void* d_word_emb; void* d_pos_emb; void* d_type_emb;    /* accumulated into (+=) */
    void* d_vis_h; void* d_vispe_h;                         /* [B*Nv, H] out */
    float* acc32;
    int32_t B, L, Nv, H, vocab, type_vocab;
    float drop_p; uint64_t seed; uint32_t vis_stream; uint32_t vispe_stream;
    const uint8_t* region_mask;                             /* ABI 3: [B*Nv] or NULL; rows with 1 got no signal from the encoder: their d_vis_h /
                                                               d_vispe_h rows are NOT written here (vlp_pretext_bwd owns them) */
    int32_t parts;                                          /* ABI 4: 0 = everything; 1 = region rows only (d_vis_h / d_vispe_h: what the region-
                                                               projection dgrad chain waits for); 2 = the three embedding tables only.  The two
                                                               halves read dpre and write disjoint outputs: a caller may run them on two streams. */
} vlp_embed_bwd_args;
int vlp_embed_bwd(const vlp_embed_bwd_args* a, void* stream);
/* vlp_embed_bwd with explicit position ids (the SCST scoring pass, whose slots carry the logical positions of the incremental decoder's rows,
 * modeling.py:856-865, 1210-1222): the dpre row (b, l) of a token position adds into d_pos_emb[position_ids[b, l]] (clamped to [0, max_pos)
 * like vlp_embed_fwd); everything else is vlp_embed_bwd on `base`.  Deterministic like it: every table row sums its rows in (b, l) order in
 * fp32, no atomics; position_ids = 0..L-1 gives vlp_embed_bwd's bits.  max_pos = rows of d_pos_emb. */
typedef struct {
    vlp_embed_bwd_args base;
    const int64_t* position_ids;                            /* [B, L] */
    int32_t max_pos;
} vlp_embed_bwd_pos_args;
int vlp_embed_bwd_pos(const vlp_embed_bwd_pos_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------
 * small data-movement helpers
 */
/* dst[r, 0:cols_dst] = (beta ? dst : 0) + cast_f16(src[r, 0:cols_src]) ; columns >= cols_src are 0.
 * src_f32 != 0 reads fp32 input (features arrive as fp32 then .half(): run_img2txt_dist.py:466-468). */
int vlp_copy2d(const void* src, int64_t lds, int32_t src_f32, void* dst, int64_t ldd, int32_t rows,
               int32_t cols_src, int32_t cols_dst, int32_t beta, void* stream);
/* dst[c, r] = src[r, c] for r < rows, c < cols; dst columns in [rows, rows_pad) of the rows c < cols are written as 0
 * (weight shadows W^T for the dgrad GEMMs; zero padding keeps K % 64 == 0); columns in [rows_pad, ldd) are not written
 * (rows_pad >= rows, ldd >= rows_pad). */
int vlp_transpose(const void* src, int64_t lds, void* dst, int64_t ldd, int32_t rows, int32_t cols,
                  int32_t rows_pad, void* stream);
/* Batched form: n independent transposes in one launch.  descs / tile_start live in DEVICE memory; tile_start[i] is the
 * index of matrix i's first 64x64 tile in the concatenated list (tiles = ceil(rows_pad/64) * ceil(cols/64) per matrix),
 * total_tiles their sum.  Requirements per matrix: lds, ldd multiples of 8, 16-byte aligned bases. */
typedef struct {
    const void* src; void* dst;
    int64_t lds, ldd;
    int32_t rows, cols, rows_pad, reserved;
} vlp_transpose_desc;
int vlp_transpose_batched(const vlp_transpose_desc* descs_dev, const int32_t* tile_start_dev, int32_t n, int32_t total_tiles, void* stream);
/* out[i,:] = src[base(i / P) + pos[i], :]   (gather_seq_out_by_pos, modeling.py:1068-1069); base(b) = b * L, or row_off[b] when
 * row_off ([B+1], ABI 4) is given (packed rows; pos must then lie inside sample b's kept rows: clamped to them) */
int vlp_gather_rows(const void* src, int64_t lds, const int64_t* pos, void* out, int64_t ldo,
                    int32_t B, int32_t P, int32_t L, int32_t H, const int32_t* row_off, void* stream);
/* dst[base(i / P) + pos[i], :] += src[i, :]   (backward of the gather; fp16 packed atomics) */
int vlp_scatter_add_rows(const void* src, int64_t lds, const int64_t* pos, void* dst, int64_t ldd,
                         int32_t B, int32_t P, int32_t L, int32_t H, const int32_t* row_off, void* stream);
/* Padding-free (packed) row layout, ABI 4.  row_off [B+1] (int32, device): sample b keeps its first n_b = row_off[b+1] - row_off[b]
 * positions and owns the packed rows [row_off[b], row_off[b+1]).
 *   vlp_rowmap_build: row_map[row_off[b] + l] = b*L + l for l < n_b  (the logical index of every packed row);
 *   vlp_rows_unpack: dst[row_map[p], 0:H] = src[p, 0:H] for p < rows (dst rows that no packed row maps to are NOT touched: clear dst first);
 *   vlp_rows_pack:   dst[p, 0:H] = src[row_map[p], 0:H]. */
int vlp_rowmap_build(const int32_t* row_off, int32_t B, int32_t L, int32_t* row_map, void* stream);
int vlp_rows_unpack(const void* src, int64_t lds, const int32_t* row_map, int32_t rows, void* dst, int64_t ldd, int32_t H, void* stream);
int vlp_rows_pack(const void* src, int64_t lds, const int32_t* row_map, int32_t rows, void* dst, int64_t ldd, int32_t H, void* stream);
/* Incremental decoding helpers (modeling.py:1189-1253):
 *   vlp_mask_pack_rect: [B, Lq, Lk] slice of the int64 attention mask (element strides given) -> bytes [B, Lq, roundup32(Lk)];
 *   vlp_kv_append: cache[b, start + i, 0:2H] = qkv_new[b*T + i, H:3H]  (K | V of the new tokens into the K/V cache [B, Lcap, 2H]);
 *   vlp_argmax_rows: ids[r*ids_stride] = argmax_v logits[r, v] (first maximum), vals[r*vals_stride] = max  (greedy token choice :1228). */
int vlp_mask_pack_rect(const int64_t* mask, int64_t batch_stride, int64_t row_stride, uint8_t* out, int32_t B, int32_t Lq, int32_t Lk,
                       int32_t Lkp, void* stream);
int vlp_kv_append(const void* qkv_new, int64_t ld, void* cache, int32_t Lcap, int32_t B, int32_t T, int32_t start, int32_t H, void* stream);
int vlp_argmax_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, int64_t* ids, int64_t ids_stride, float* vals, int64_t vals_stride,
                    void* stream);
/* Token-step kernels of the incremental decoder (round 6; csrc/decode.hip).  One token step of BertForSeq2SeqDecoder.forward
 * (modeling.py:1189-1253) runs BertLayer (:360-372) on M = sequences x T rows (T = 1-2 new positions): launch- and latency-bound, so a
 * Linear is ONE load burst per workgroup instead of a k loop, and the split-K reduce IS the LayerNorm launch.
 *   vlp_dec_gemm: Y[M, N] = act(X[M, K] . W[N, K]^T + bias)   (the Linears of :270-272, :314, :341, :354 on the new rows), M any, N any,
 *       K % (64 * splits) == 0, K / splits <= 768.
 *       splits == 1, slab == NULL: fp16 result.  If kv_cache != NULL, output columns >= kv_col0 (the K | V part of a packed QKV projection,
 *       kv_col0 % 32 == 0) are written to kv_cache[(m / kv_T) * kv_Lcap + kv_start + m % kv_T][n - kv_col0] (row pitch kv_ld) instead of Y:
 *       the K/V append of vlp_kv_append fused into the projection (a TRUE K/V cache in place of the hidden-state history of :273-277, 386-394).
 *       splits > 1 (or slab != NULL): raw fp32 partial sums of k slice s to slab[s][m][n] (pitch ldslab, ldslab % 8 == 0); bias / act / Y unused.
 *   vlp_dec_reduce_ln: Y[m, :] = LayerNorm( fp16( sum_s slab[s][m, :] + bias + residual[m, :] ) ) * gamma + beta  (:315-316, :355-356: dense
 *       output + bias, dropout p = 0, residual add, BertLayerNorm :188-192 with fp32 statistics); slabs summed in index order (deterministic).
 *       H in {256, 512, 768, 1024}. */
typedef struct {
    const void* X; int64_t ldx;          /* f16 [M, K] */
    const void* W; int64_t ldw;          /* f16 [N, K] */
    const void* bias;                    /* f16 [N] or NULL (splits == 1 only) */
    void* Y; int64_t ldy;                /* f16 [M, N] (splits == 1) */
    float* slab; int64_t ldslab;         /* f32 [splits][M][ldslab] (split form) or NULL */
    void* kv_cache; int64_t kv_ld;       /* f16 [sequences][kv_Lcap][kv_ld] or NULL */
    int32_t kv_col0, kv_Lcap, kv_T, kv_start;
    int32_t M, N, K, splits;
    int32_t act;                         /* VLP_ACT_NONE | VLP_ACT_GELU (splits == 1 only) */
    const void* residual; int64_t ldr;   /* f16 [M, N] or NULL (splits == 1): Y = act(X W^T + bias + residual), one rounding (modeling.py:315-316) */
    /* LayerNorm prologue (splits == 1, K <= 768): X holds PRE-LayerNorm rows; the kernel computes X' = LayerNorm(X) * gamma + beta (fp32 statistics,
     * one rounding, modeling.py:188-192) in LDS and multiplies X'.  ln_out (optional): X' [M, K] is also written there (the next residual). */
    const void* ln_gamma; const void* ln_beta; float ln_eps;
    void* ln_out; int64_t ld_ln_out;
} vlp_dec_gemm_args;
int vlp_dec_gemm(const vlp_dec_gemm_args* a, void* stream);
typedef struct {
    const float* slab; int64_t ldslab; int32_t splits;
    const void* bias;                    /* f16 [H] or NULL */
    const void* residual; int64_t ldr;   /* f16 [M, H] or NULL */
    const void* gamma; const void* beta; /* f16 [H] */
    float eps;
    void* Y; int64_t ldy;                /* f16 [M, H] */
    int32_t M, H;
} vlp_dec_reduce_ln_args;
int vlp_dec_reduce_ln(const vlp_dec_reduce_ln_args* a, void* stream);
/* vlp_argmax_rows2: vlp_argmax_rows with the index written to TWO destinations (the output column and the next step's input token,
 * :1228, 1248-1250; ids_b may be NULL) by one launch: 1024 threads per row, 16-byte loads (ld % 8 == 0, logits 16-byte aligned). */
int vlp_argmax_rows2(const void* logits, int64_t ld, int32_t rows, int32_t V, int64_t* ids_a, int64_t ids_a_stride, int64_t* ids_b, int64_t ids_b_stride,
                     float* vals, int64_t vals_stride, void* stream);
/* On-device input preparation (replaces per-sample CPU work of vlp/seq2seq_loader.py):
 *   vlp_mask_build: the packed attention masks (format of vlp_mask_pack, incl. the optional key-major copy) straight from the per-sample
 *       lengths, seq2seq_loader.py:292-301:  second_st = len(tokens_a)+2, second_end = len(tokens_a)+len(tokens_b)+3;
 *       s2s: attend(q,k) = k < st || (st <= q < en && st <= k <= q);  bi: attend(q,k) = k < en.  No int64 [B,L,L] tensor is shipped or read.
 *   vlp_vis_pe_prep: raw boxes [B,Nv,6] (x1,y1,x2,y2,-,confidence) + class probabilities [B*Nv, ld_cls] (f16 as stored on disk, or f32)
 *       -> the 6+n_cls encoding of seq2seq_loader.py:338-351 (corners / largest corner of the image, clamped relative area, layer norm of the 6
 *       box numbers and of the class probabilities, eps inside the sqrt) in f16, zero padded to pad_to columns = the K-padded operand of the
 *       vis_pe_embed GEMM (modeling.py:1016). */
/* ABI 3: region_mask ([B*Nv] bytes from vlp_region_mask_build, or NULL) additionally blocks the key columns 1..Nv of masked regions
 * for every query (mask_image_regions, seq2seq_loader.py:303-304). */
int vlp_mask_build(const int32_t* second_st, const int32_t* second_end, const int32_t* is_s2s, uint8_t* out, uint8_t* out_t, int32_t B, int32_t L,
                   int32_t Lp, const uint8_t* region_mask, int32_t Nv, void* stream);
typedef struct {
    const float* bbox;       /* [B, Nv, 6] f32 */
    const void* cls;         /* [B*Nv, ld_cls] f16 or f32 */
    int64_t ld_cls;
    void* out;               /* [B*Nv, ld_out] f16 */
    int64_t ld_out;
    int32_t B, Nv, n_cls, pad_to, cls_is_f32;
    float eps;               /* 1e-5 (F.layer_norm default) */
} vlp_vis_pe_prep_args;
int vlp_vis_pe_prep(const vlp_vis_pe_prep_args* a, void* stream);
/* sample_mode == 'sample' (modeling.py:1229-1235): ids[r*ids_stride] ~ Categorical(softmax(logits[r, :V])) drawn by the Gumbel-max trick
 * on the library's counter-based hash (seed, rng_stream, row, column) -- torch.multinomial's stream cannot be reproduced, the
 * distribution is the same; logp[r*logp_stride] = log_softmax(logits[r])[ids[r]]. */
int vlp_sample_rows(const void* logits, int64_t ld, int32_t rows, int32_t V, uint64_t seed, uint32_t rng_stream, int64_t* ids,
                    int64_t ids_stride, float* logp, int64_t logp_stride, void* stream);
/* vlp_sample_rows with `rep` draws per logits row and the seed in device memory: draw r (of `rows`) reads logits row r / rep, its RNG row key
 * is r (the rep draws of a logits row differ), the seed is *seed_cell + seed_add with seed_cell an 8-byte aligned device address read with a
 * plain load -- so a launch whose seed changes from call to call has call-invariant arguments and can be replayed from a captured graph.
 * ids2 (optional, NULL = none) receives the same id at ids2[r*ids2_stride].  With rep == 1, the same effective seed and rng_stream, ids and
 * logp equal vlp_sample_rows' bit for bit (one shared kernel body). */
int vlp_sample_rows_rep(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t rep, const uint64_t* seed_cell, uint64_t seed_add,
                        uint32_t rng_stream, int64_t* ids, int64_t ids_stride, int64_t* ids2, int64_t ids2_stride, float* logp, int64_t logp_stride,
                        void* stream);
/* vlp_sample_rows_rep's draw from a tempered and truncated distribution.  With l_v the fp16 logit of column v < V:
 *   z_v = l_v / temperature;
 *   top-k (0 < top_k < V): S_k = {v : l_v >= tau_k}, tau_k the top_k-th largest logit counted with multiplicity -- ties at the threshold are all
 *     kept; otherwise S_k is every column;
 *   top-p (top_p < 1): with q_v = softmax(z) over S_k, tau_p is the largest fp16 value t whose columns {v in S_k : l_v >= t} carry a mass
 *     >= top_p, and S = {v in S_k : l_v >= tau_p}; otherwise S = S_k;
 *   ids[r*ids_stride] = argmax over S of z_v + g_v with vlp_sample_rows_rep's Gumbel values (same row key r, same hash), and
 *   logp[r*logp_stride] = log of the id's probability under softmax(z) over S, the distribution drawn from.
 * S is a value threshold and always holds the row's maximum; -inf logits are never drawn.  rows, rep, seed_cell, seed_add, rng_stream, ids2
 * and the strides are vlp_sample_rows_rep's (call-invariant arguments: the launch can be captured); with temperature = 1, top_k = 0 and
 * top_p = 1 the ids are vlp_sample_rows_rep's.  cutoff (optional, NULL = none): cutoff[r] = the smallest kept logit (the row minimum when
 * nothing is filtered); kept (optional): kept[r] = |S|.  Repeated launches return the same bits in all four outputs.
 * VLP_ERR_BAD_ARG, nothing launched: temperature <= 0 or not finite, top_k < 0, top_p <= 0, top_p > 1, rep < 1, or top_p < 1 with V > 2^22
 * (the probability mass of a row is summed in 64-bit integers of 2^-40 of the largest column's). */
int vlp_sample_rows_filtered(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t rep, const uint64_t* seed_cell, uint64_t seed_add,
                             uint32_t rng_stream, float temperature, int32_t top_k, float top_p, int64_t* ids, int64_t ids_stride, int64_t* ids2,
                             int64_t ids2_stride, float* logp, int64_t logp_stride, float* cutoff, int32_t* kept, void* stream);
/* SCST scoring layout: the teacher-forced sequence whose training forward reproduces, for every sampled position, the hidden states of the
 * incremental decoder (replaces differentiating the decoder itself, modeling.py:1210-1251 under autograd in run_img2txt_dist.py:506-507).
 * With T sampled tokens y_0..y_{T-1} the scoring sequence has L' = in_len + 2T - 1 <= 256 slots:
 *   [prefix 0..in_len-1 | y_0..y_{T-2} at logical positions in_len..in_len+T-2 | [MASK]_0..[MASK]_{T-1} at logical positions in_len..in_len+T-1];
 * ids / token types / position ids are read at each slot's logical position ([MASK] slots get mask_word_id), masked_pos[b, t] = slot of
 * [MASK]_t.  With am = mask[b] ([L, L]): a prefix / real slot at logical p keeps am[p, p'] for prefix / real slots p' <= max(p, in_len - 1)
 * and am[p, q] for the [MASK] slot at logical q = max(p + 1, in_len); [MASK] at logical q keeps am[q, p'] for prefix / real slots p' <= q - 1
 * and am[q, q] for itself; every other entry is 0.  Outputs int64: out_ids / out_segment_ids / out_position_ids [B, L'], out_mask
 * [B, L', L'] (pack it with vlp_mask_pack), masked_pos [B, T].  Inputs: prefix_ids [B, in_len], sample_ids [B, T], segment_ids /
 * position_ids [B, L], mask [B, L, L] (all contiguous int64), in_len + T <= L. */
typedef struct {
    const int64_t* prefix_ids; const int64_t* sample_ids;
    const int64_t* segment_ids; const int64_t* position_ids; const int64_t* mask;
    int64_t* out_ids; int64_t* out_segment_ids; int64_t* out_position_ids; int64_t* out_mask; int64_t* masked_pos;
    int32_t B, L, in_len, T;
    int64_t mask_word_id;
} vlp_scst_layout_args;
int vlp_scst_layout(const vlp_scst_layout_args* a, void* stream);
/* Beam search (modeling.py:1255-1494):
 *   vlp_logsoftmax_topk: per row log_softmax over V (fp32 from fp16 logits), -10000 added on forbidden words (uint8 [rows, V], may be
 *       NULL; :1298-1299), the eos column forced to -10000 while the minimum length is not reached (:1300-1301), then the K best
 *       (value descending, index ascending on ties; :1302) -> out_scores / out_ids [rows, K];
 *   vlp_beam_select: per sample the K best of the K*K continuations  kk + last_eos * -10000 + last_total  (:1308-1316), their back
 *       pointers, ids and eos flags; src_rows[b*K+k] = the cache row the beam continues (b in the first step, b*K+ptr later);
 *       next_ids receives the chosen ids with the given element stride (the decoder's next input column);
 *   vlp_kv_gather: dst[r, pos, :] = src[idx[r], pos, :] for pos in [lo, hi) -- first_expand / select_beam_items (:1325-1349) applied
 *       to the K/V caches instead of the reference's hidden-state history. */
int vlp_logsoftmax_topk(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t K, const uint8_t* forbid, int32_t eos_id,
                        int32_t block_eos, float* out_scores, int64_t* out_ids, void* stream);
typedef struct {
    const float* kk_scores;   /* [rows, K]  rows = B (first) or B*K */
    const int64_t* kk_ids;    /* [rows, K] */
    const float* last_total;  /* [B, K] cumulative scores of the previous frame (NULL when first) */
    const float* last_eos;    /* [B, K] 1.0 where the previous frame's word was eos (NULL when first) */
    float* out_scores;        /* [B, K] */
    int64_t* out_ids;         /* [B, K] */
    int64_t* out_ptrs;        /* [B, K] */
    float* out_eos;           /* [B, K] */
    int64_t* src_rows;        /* [B*K] */
    int64_t* next_ids;        /* B*K elements, stride next_ids_stride */
    int64_t next_ids_stride;
    int32_t B, K, first;
    int64_t eos_id;
} vlp_beam_select_args;
int vlp_beam_select(const vlp_beam_select_args* a, void* stream);
/* Diverse (group) beam search (Vijayakumar et al. 2016; not in the reference): vlp_beam_select with the K beams of a sample split into
 * `groups` = G groups of Kg = K / G, extended one after another inside the step.  Per sample b, for g = 0 .. G-1:
 *   candidates: the continuations of the group's own rows r in [g*Kg, (g+1)*Kg), index i = r*K + j, v0 = vlp_beam_select's value
 *       kk + last_eos * -10000 + last_total (same expression and order); in the first step every group sees the single row (i = j, v0 = kk);
 *   key = v0 - fl32(penalty * c), c = the number of picks of the groups < g of this step and sample whose word id is the candidate's (eos and
 *       the picks of ended parents count); the product is rounded to fp32 before the subtraction; a NaN key orders as -inf;
 *   Kg successive picks, each the maximum among the candidates after the previous pick in the (key descending, i ascending) order;
 *   pick n of group g goes to slot b*K + g*Kg + n of the six outputs, which have vlp_beam_select's meaning; out_scores holds v0, the
 *       unpenalised cumulative log-probability (the penalty steers the selection only).
 * Back pointers stay inside their group (out_ptrs / Kg == slot / Kg).  groups = 1 gives vlp_beam_select's bits for any penalty when no v0 is NaN
 * (vlp_beam_select has no NaN rule: it never picks a NaN candidate).  The per-row
 * top-K lists suffice: a word outside a row's top K has K words above it, at most K - Kg of them penalised.
 * One launch (one wave per sample, the earlier groups' picks and the group's keys in LDS), no synchronisation, capturable; equal inputs give
 * bit-equal outputs.  VLP_ERR_BAD_ARG before any launch: a null operand, B <= 0, K outside 1..64, groups < 1, K % groups != 0, a penalty that
 * is NaN, negative or infinite, first == 0 without last_total / last_eos. */
int vlp_beam_select_groups(const vlp_beam_select_args* a, int32_t groups, float penalty, void* stream);
/* Constrained beam search (Anderson et al. 2017, Post & Vilar 2018; not in the reference): captions that must mention given phrases.
 *   vlp_logsoftmax_topk_want: vlp_logsoftmax_topk (forbid, or neither) / vlp_logsoftmax_topk_list (cand_ids, cand_ld, cand_cnt) -- the two
 *       forms exclude each other -- on the same kernel bodies, dispatch and lse, so out_scores / out_ids are theirs bit for bit; in addition
 *       want_val[r, c] (f32 [rows, C]) = the value that kernel body computes for word want_ids[r, c] (int32 [rows, C], 1 <= C <= 8):
 *       (float)x[w] - lse, + -10000 when forbidden by mask or list, -10000 when it is the blocked eos; -inf for an id of -1 (or outside
 *       [0, V)).  A wanted word that is in the row's list carries the list's bits.  A few gathers behind the lse, no second walk.
 *   vlp_beam_select_constrained: the selection step.  cons_ids int32 [B, C, Lc] / cons_len int32 [B, C] (0: unused) are the phrases of every
 *       sample; a beam's state is one int32 (bits 0-7 met mask, 8-11 phrase in progress + 1, 16-23 tokens of it matched); prev_state
 *       [B, K] (NULL in the first step).  Row r of a sample offers K + C candidates, index i = r*(K+C) + j: its top-K list (j < K) and its
 *       wanted words want_ids / want_val [rows, C] (absent: -1, a list id of the row, an earlier wanted id of the row).  v0 is
 *       vlp_beam_select's value; an eos of a live parent that leaves a phrase unmet gets + -10000 and is dead, as every candidate of an
 *       ended parent is; with `last` != 0 (the search's last step, which ends every hypothesis) every candidate of a live parent that leaves
 *       a phrase unmet is treated so, whatever its word.  K picks walk the banks (bank = matched tokens, met phrases included) from
 *       Tb = sum of cons_len downwards, wrapping, skipping banks without a live candidate, each the best (v0 descending, i ascending, NaN as -inf) live candidate of its bank; dead
 *       candidates follow when no live one is left.  The six outputs of vlp_beam_select keep their meaning; out_state int32 [B, K] and
 *       want_next int32 [B*K, C] (the next step's want_ids: per phrase its next token, -1 when met / unused / the beam has ended) are
 *       added.  With every cons_len == 0 the picks are vlp_beam_select's whenever live candidates outrank dead ones (any search).  The rule
 *       in full, as a numpy specification: vlp_amd/constrained.py.
 *       One launch (one wave per sample, <= 64 * 72 candidates in LDS), no synchronisation, capturable; equal inputs give equal bits.
 *       VLP_ERR_BAD_ARG before any launch: a null operand, B <= 0, K outside 1..64, C outside 1..8, Lc outside 1..8, first == 0 without
 *       last_total / last_eos / prev_state. */
int vlp_logsoftmax_topk_want(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t K, const uint8_t* forbid, const int32_t* cand_ids,
                             int64_t cand_ld, const int32_t* cand_cnt, int32_t eos_id, int32_t block_eos, const int32_t* want_ids, int32_t C,
                             float* out_scores, int64_t* out_ids, float* want_val, void* stream);
int vlp_beam_select_constrained(const vlp_beam_select_args* a, const int32_t* want_ids, const float* want_val, const int32_t* prev_state,
                                const int32_t* cons_ids, const int32_t* cons_len, int32_t C, int32_t Lc, int32_t last, int32_t* out_state,
                                int32_t* want_next, void* stream);
/* Duplicate n-gram blocking on the device (get_dup_ngram_candidates, modeling.py:1391-1406), for a search that never leaves the GPU:
 *   vlp_ngram_candidates: wids / ptrs are the frames [frames, B, K] that vlp_beam_select writes (int64, contiguous).  Row r = b*K + k:
 *       the hypothesis that ends in beam k of frame s is rebuilt by following ptrs back from frame s (length s + 1 <= 256); the words that
 *       would complete a repeated n-gram (n = ngram_size >= 2) go to cand_ids[r * cand_ld + 0 .. cand_cnt[r]): every distinct
 *       seq[i + n - 1] with seq[i .. i + n - 2] equal to the last n - 1 words, except words of the ignore list; the count is 0 when
 *       s + 1 < n or when one of the last n - 1 words is in the ignore list (ignore_ids: n_ignore int64 on the device, NULL when 0).
 *       cand_ld >= s + 1; nothing beyond the first cand_cnt[r] entries of a row is written.  K <= 64.
 *   vlp_logsoftmax_topk_list: vlp_logsoftmax_topk with the forbidden words of row r given as that list instead of a dense mask (cand_ld <=
 *       1024; a count is clamped to cand_ld); same ids, scores equal bit for bit to the dense form with the mask scattered from the lists. */
int vlp_ngram_candidates(const int64_t* wids, const int64_t* ptrs, int32_t B, int32_t K, int32_t s, int32_t ngram_size, const int64_t* ignore_ids,
                         int32_t n_ignore, int32_t* cand_ids, int64_t cand_ld, int32_t* cand_cnt, void* stream);
int vlp_logsoftmax_topk_list(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t K, const int32_t* cand_ids, int64_t cand_ld,
                             const int32_t* cand_cnt, int32_t eos_id, int32_t block_eos, float* out_scores, int64_t* out_ids, void* stream);
int vlp_kv_gather(const void* src, int64_t src_rows_per_batch, void* dst, int64_t dst_rows_per_batch, const int64_t* idx, int32_t R, int32_t lo,
                  int32_t hi, int32_t row_elems, void* stream);
/* The N best hypotheses of a finished search, ranked and back-tracked on the device (:1446-1474 applied to every rank):
 *   tot (f32) / wids / ptrs (int64): the frames [F, B, K] that vlp_beam_select wrote, contiguous.  Per sample b: last = the first frame whose K
 *       words are all eos_id, else F - 1; candidate (f, k) exists when f <= last and (wids[f,b,k] == eos_id or f == last); its value is
 *       (double)tot[f,b,k] + length_penalty * (f + 1) in fp64 (product rounded, then the sum); candidates are ordered by value descending, then
 *       by f*K + k ascending.  Rank n of sample b goes to row n*B + b (sample-major):
 *       seq [N*B, T] int64   the words along the back pointers from (f, k), zero padded (a pointer outside [0, K) counts as 0);
 *       score [N*B] f32      tot[f,b,k];      value [N*B] f64   the ranking value;      len [N*B] int32   f + 1;
 *       ok [N*B] uint8       1 when the value is finite and no position before the last one is eos_id (0: the continuation of a hypothesis
 *                            that had ended, which the search keeps at -10000).
 *       A rank whose value is not finite gets an all-zero row, len 0 and ok 0 (the reference's [0]).
 *   1 <= N <= K <= 64, 1 <= F <= 256, T >= F, B > 0; anything else is VLP_ERR_BAD_ARG before the launch.  One launch, no synchronisation. */
int vlp_beam_nbest(const float* tot, const int64_t* wids, const int64_t* ptrs, int32_t F, int32_t B, int32_t K, int64_t eos_id, double length_penalty,
                   int32_t N, int32_t T, int64_t* seq, float* score, double* value, int32_t* len, uint8_t* ok, void* stream);
/* VQA fusion (modeling.py:1044,1138): out[b,:] = h[b,0,:] * h[b,Nv+1,:]; backward adds into dh rows.  row_off ([B+1] or NULL, ABI 4):
 * packed rows, sample b starts at row row_off[b] instead of b*L. */
int vlp_vqa_mul_fwd(const void* h, void* out, int32_t B, int32_t L, int32_t Nv, int32_t H, const int32_t* row_off, void* stream);
int vlp_vqa_mul_bwd(const void* h, const void* dout, void* dh, int32_t B, int32_t L, int32_t Nv, int32_t H, const int32_t* row_off, void* stream);
/* dz = dy * dropmask * (y > 0): backward of Linear->ReLU->Dropout given the layer OUTPUT y */
int vlp_relu_dropout_bwd(const void* dy, const void* y, void* dz, int64_t n, int64_t ncols, float drop_p,
                         uint64_t seed, uint32_t rng_stream, void* stream);

/* dz = dy * gelu'(z)   (backward of the head transform's gelu, modeling.py:433; n % 8 == 0) */
int vlp_gelu_bwd(const void* dy, const void* z, void* dz, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Losses
 * Masked-LM loss (modeling.py:1083-1111): per-row CE in fp32 over V logits, * masked_weights,
 * per-sample sum, keep the int(B*(1-ratio)) smallest samples, / (sum of kept weights + 1e-5), sum.
 * vlp_mlm_loss_fwd writes loss[0] (f32), per-row lse [B*P] and the per-row gradient coefficient
 * coef[B*P] = keep * weight / denominator; vlp_mlm_loss_bwd writes
 * dlogits[r, v] = grad_scale * coef[r] * (softmax(logits[r])[v] - [v == label[r]]) for v < V and 0 for
 * V <= v < ld_dlogits.
 * drop_worst_ratio is a float field (ABI) while the reference computes int(B * (1 - ratio)) with the caller's double, and the
 * widened float is not that double (1 - 0.2f is 1.2e-8 short of 0.8: B = 40 would keep 31, Python keeps 32).  The launcher (both
 * vlp_mlm_loss_fwd and vlp_mlm_loss_ls_fwd, csrc/keep_count.h) therefore recovers the caller's double before the double
 * arithmetic: the double nearest to the float's shortest round-tripping decimal when that has at most 6 significant digits
 * (0.2f -> 0.2), else the simplest fraction p / q inside the float's rounding interval (0.33333334f -> 1.0 / 3); then double
 * difference, double product, truncation, as Python does.  A caller who passes such a Python float r gets Python's count.
 */
typedef struct {
    const void* logits; int64_t ld_logits;    /* [B*P, V] fp16 */
    const int64_t* labels;                    /* [B*P] */
    const int64_t* weights;                   /* [B*P] masked_weights */
    float* loss;                              /* [1] out */
    float* lse; float* coef;                  /* [B*P] out */
    float* row_loss;                          /* [B*P] scratch */
    int32_t B, P, V;
    float drop_worst_ratio;
} vlp_mlm_loss_fwd_args;
int vlp_mlm_loss_fwd(const vlp_mlm_loss_fwd_args* a, void* stream);
typedef struct {
    const void* logits; int64_t ld_logits;
    const int64_t* labels;
    const float* lse; const float* coef;
    const float* grad_scale;                  /* [1] device scalar (upstream gradient x loss scale) */
    void* dlogits; int64_t ld_dlogits;        /* [B*P, ld] fp16 out */
    int32_t rows, V;
} vlp_mlm_loss_bwd_args;
int vlp_mlm_loss_bwd(const vlp_mlm_loss_bwd_args* a, void* stream);

/* Label-smoothed masked-LM loss (loss.py LabelSmoothingLoss, used at modeling.py:995-999, 1104-1106 when
 * config.label_smoothing is set): per row the KL divergence sum_w q[w] * (log q[w] - log_softmax(logits[r])[w])
 * in fp32 (0 log 0 = 0) with q[w] = smooth for w != ignore_index, q[label] = confidence, and q == 0 on a row
 * whose label is ignore_index; then the same masking / drop-worst / normalisation as vlp_mlm_loss_fwd.
 * smooth, confidence, q_sum = (V-2) * smooth + confidence and q_log_q = sum_w q[w] log q[w] of a row (the
 * label-independent term of the KL) are the values of the caller's smoothed one-hot buffer in ITS dtype: an fp16
 * model rounds smooth / confidence, and the reference rounds every q log q term to fp16 (xlogy on the fp16
 * target), so q_log_q = (V-2) * half(s log s) + half(c log c) there.  Requires V > 2, 0 <= ignore_index < V.
 * vlp_mlm_loss_ls_bwd writes dlogits[r, v] = grad_scale * coef[r] * (softmax(logits[r])[v] * q_sum - q[v])
 * for v < V, 0 for V <= v < ld_dlogits, and 0 on every column of a row whose label is ignore_index.
 * Labels are clamped to [0, V) like the plain CE entry points.  drop_worst_ratio: the launcher recovers the caller's double from the
 * float field exactly as vlp_mlm_loss_fwd does (one shared helper), so the kept-sample count is Python's int(B * (1 - r)). */
typedef struct {
    const void* logits; int64_t ld_logits;    /* [B*P, V] fp16 */
    const int64_t* labels;                    /* [B*P] */
    const int64_t* weights;                   /* [B*P] masked_weights */
    float* loss;                              /* [1] out */
    float* lse; float* coef;                  /* [B*P] out */
    float* row_loss;                          /* [B*P] scratch */
    int32_t B, P, V;
    float drop_worst_ratio;
    float smooth, confidence, q_sum, q_log_q;
    int32_t ignore_index;
} vlp_mlm_loss_ls_fwd_args;
int vlp_mlm_loss_ls_fwd(const vlp_mlm_loss_ls_fwd_args* a, void* stream);
typedef struct {
    const void* logits; int64_t ld_logits;
    const int64_t* labels;
    const float* lse; const float* coef;      /* written by vlp_mlm_loss_ls_fwd */
    const float* grad_scale;                  /* [1] device scalar (upstream gradient x loss scale) */
    void* dlogits; int64_t ld_dlogits;        /* [B*P, ld] fp16 out */
    int32_t rows, V;
    float smooth, confidence, q_sum;
    int32_t ignore_index;
} vlp_mlm_loss_ls_bwd_args;
int vlp_mlm_loss_ls_bwd(const vlp_mlm_loss_ls_bwd_args* a, void* stream);

/* Log-probability of one chosen token per row (SCST, the sampled caption's log-probs: modeling.py:1232-1235, without the fp16 rounding of
 * the reference's log_softmax): fwd logp[r] = logits[r, ids[r]] - lse[r] with lse[r] = logsumexp(logits[r, :V]), both fp32 from the fp16
 * logits (the arithmetic of vlp_mlm_loss_fwd); bwd dlogits[r, v] = g[r] * ([v == ids[r]] - exp(logits[r, v] - lse[r])) for v < V and 0 for
 * V <= v < ld_dlogits.  g: device [rows] fp32 upstream gradient (carries the loss scale; either sign).  ids are clamped to [0, V). */
typedef struct {
    const void* logits; int64_t ld_logits;    /* [rows, V] fp16 */
    const int64_t* ids;                       /* [rows] */
    float* logp; float* lse;                  /* [rows] out */
    int32_t rows, V;
} vlp_token_logprob_fwd_args;
int vlp_token_logprob_fwd(const vlp_token_logprob_fwd_args* a, void* stream);
typedef struct {
    const void* logits; int64_t ld_logits;
    const int64_t* ids;
    const float* lse;                         /* written by vlp_token_logprob_fwd */
    const float* g;                           /* [rows] device upstream gradient */
    void* dlogits; int64_t ld_dlogits;        /* [rows, ld] fp16 out */
    int32_t rows, V;
} vlp_token_logprob_bwd_args;
int vlp_token_logprob_bwd(const vlp_token_logprob_bwd_args* a, void* stream);

/* The SCST policy pi_T = softmax(logits / T) of one chosen token per row, and its entropy (--scst_temperature, --scst_entropy_weight).  For
 * one row, l_v the fp16 logit of column v < V as fp32 (columns >= V do not exist), T = temperature, finite and > 0:
 *   z_v = l_v / T;  lse = log sum_v exp(z_v);  q_v = exp(z_v - lse);  logp = z_id - lse  (id clamped to [0, V));
 *   H = -sum_v q_v log q_v, with 0 log 0 = 0: a column with q_v = 0 (a -inf logit included) adds nothing.
 * fwd writes lse (that of z), logp and, when `entropy` is not NULL, H; computed as H = log S - A / S with d = (l_v - l_max) / T,
 * S = sum e^d, A = sum e^d d (subtracted before divided, so a small T does not overflow).
 * bwd takes the per-row upstream gradients g[r] = dL/dlogp_r and h[r] = dL/dH_r (optional; either sign, both carry the loss scale):
 *   dlogits[r, v] = (1/T) (g[r] ([v == id] - q_v) - h[r] q_v (log q_v + H_r))  for v < V, 0 for V <= v < ld_dlogits;
 * a column with q_v = 0 gets exactly 0 from the entropy term.  `entropy` (the forward's) is read only with h and required then.
 * T = 1 without entropy / h gives vlp_token_logprob_fwd / _bwd's bits.  VLP_ERR_BAD_ARG before any launch: a temperature that is not finite
 * or <= 0 (or subnormal: its reciprocal overflows), a null required operand, the layout / alignment rules of vlp_token_logprob_*, h without entropy. */
typedef struct {
    const void* logits; int64_t ld_logits;    /* [rows, V] fp16 */
    const int64_t* ids;                       /* [rows] */
    float* logp; float* lse;                  /* [rows] out */
    float* entropy;                           /* [rows] out, or NULL */
    int32_t rows, V;
    float temperature;
} vlp_token_policy_fwd_args;
int vlp_token_policy_fwd(const vlp_token_policy_fwd_args* a, void* stream);
typedef struct {
    const void* logits; int64_t ld_logits;
    const int64_t* ids;
    const float* lse;                         /* written by vlp_token_policy_fwd with the same temperature */
    const float* entropy;                     /* written by vlp_token_policy_fwd; NULL without h */
    const float* g;                           /* [rows] device upstream gradient of logp */
    const float* h;                           /* [rows] device upstream gradient of the entropy, or NULL */
    void* dlogits; int64_t ld_dlogits;        /* [rows, ld] fp16 out */
    int32_t rows, V;
    float temperature;
} vlp_token_policy_bwd_args;
int vlp_token_policy_bwd(const vlp_token_policy_bwd_args* a, void* stream);

/* Scoring a given token per row (Engine.score_captions: log-likelihood, token accuracy and entropy of given captions).  For one row with
 * id = ids[r] >= 0 (clamped to V - 1 from above), l_v the fp16 logit of column v < V as fp32 (columns >= V are never read):
 *   lse = log sum_v exp(l_v);  logp = l_id - lse;  entropy = -sum_v q_v log q_v with q_v = exp(l_v - lse) and 0 log 0 = 0 -- on a 16-byte
 *     aligned row with ld_logits % 8 == 0 bit for bit what vlp_token_policy_fwd writes at temperature 1 with entropy (the same expressions,
 *     the same summation order); any other row is walked column by column, in another summation order;
 *   rank = #{v : l_v > l_id} + #{v < id : l_v == l_id}: the token's place, from 0, when the columns are sorted by falling logit with
 *     equal logits in rising column order.  Comparisons of the fp16 values, exact;
 *   top_id / top_logit: the row's largest logit and its column, the SMALLEST column on ties (vlp_argmax_rows's first maximum).
 * The two tie rules agree: rank == 0 exactly when top_id == id.  A row without a column above -inf has top_id 0.
 * A row with ids[r] < 0 is not counted and not read: logp = lse = entropy = top_logit = 0, rank = top_id = -1.
 * One launch, one workgroup per row, the two passes of vlp_token_logprob_fwd.  VLP_ERR_BAD_ARG before the launch: a null operand, rows or
 * V < 1, V > 2^24, ld_logits < V. */
typedef struct {
    const void* logits; int64_t ld_logits;    /* [rows, V] fp16 */
    const int64_t* ids;                       /* [rows]; < 0: the row is not counted */
    float* logp; float* lse; float* entropy;  /* [rows] out */
    int32_t* rank;                            /* [rows] out */
    int64_t* top_id; float* top_logit;        /* [rows] out */
    int32_t rows, V;
} vlp_token_score_args;
int vlp_token_score(const vlp_token_score_args* a, void* stream);

/* CIDEr-D of id strings (SCST, the reward the reference computes on the host: scst_utils.py:36-63 with pycocoevalcap's Cider(df='corpus')).
 * The specification is vlp_amd/scst.py CiderD.compute_score on the strings array_to_str makes:
 *   - a string is the ids of a row up to AND INCLUDING the first 0, or all T ids without one; nothing behind the first 0 is read as text.
 *     Ids are vocabulary indices, 0 <= id < 2^31;
 *   - hypothesis row i (of mult*G) is scored against the references of group i % G; group g has R reference rows of which the first
 *     ref_count[g] (clamped to 1..R; NULL = R) are valid, the others are never read as text;
 *   - n-grams of order 1..4 are counted exactly (token comparison, no hashing).  df(g) = mult * the number of groups whose valid references
 *     hold g; ref_len = log(mult*G); weight = tf * (ref_len - log(max(1, df))), also for a hypothesis n-gram that no reference holds; one
 *     L2 norm per order; a string's length is its number of bigram occurrences;
 *   - per reference and order sum_g min(h_g, r_g) * r_g, divided by the two norms when both are non-zero, times
 *     exp(-(len_h - len_r)^2 / (2 sigma^2)); scores[i] = 10 * the mean over the orders, averaged over the group's valid references;
 *   - reward (optional, mult == 2: rows [0, G) the samples, [G, 2G) the greedy captions) [g] = scores[g] - scores[G + g], one fp32
 *     subtraction of the two stored scores.
 * fp32 with the accurate logf / expf / sqrtf, every sum in a fixed order, no atomics: equal inputs give bit-equal outputs.  Two launches
 * (counting, scoring), no host involvement, capturable.  Nothing is written outside scores[0, mult*G), reward[0, G) and the workspace.
 * Accepted: 1 <= T <= 64, 1 <= R <= 8, 1 <= G <= 1024, mult 1 or 2, hyp_ld / ref_ld >= T, ref_group_stride >= (R-1) * ref_ld + T (strides in
 * elements), sigma > 0, a 16-byte aligned workspace of vlp_cider_d_workspace_bytes() bytes (0 for a refused shape).  Anything else -- a
 * workspace that is too small included -- returns VLP_ERR_BAD_ARG before anything is launched. */
typedef struct {
    const int64_t* hyp; int64_t hyp_ld;                        /* [mult*G, T]; row i is scored against group i % G */
    const int64_t* ref; int64_t ref_group_stride, ref_ld;      /* [G, R, T] */
    const int32_t* ref_count;                                  /* [G], 1..R references of each group are valid; NULL = all R */
    int32_t G, R, T, mult;                                     /* mult = hypotheses per group (SCST: 2 = sample, greedy) */
    float sigma;                                               /* 6.0 */
    float* scores;                                             /* [mult*G] out */
    float* reward;                                             /* optional [G] out: scores[g] - scores[G+g]; needs mult == 2 */
    void* workspace; int64_t workspace_bytes;
} vlp_cider_d_args;
int64_t vlp_cider_d_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult);
int vlp_cider_d(const vlp_cider_d_args* a, void* stream);

/* vlp_cider_d with the document frequencies of a resident table (vlp_amd/scst.py DocFreq: df over a whole training set, one document per
 * image) instead of the call's own references.  The specification is CiderD(df=<DocFreq>).compute_score; everything of vlp_cider_d that is
 * not restated here holds as it stands (strings, groups, ref_count, norms, bigram length, clipped products, zero-norm rule, Gaussian
 * penalty, mean over orders and references, x 10, reward, accepted shapes and strides, two capturable launches, fixed summation order, no
 * atomics, bit-equal repeats, nothing written outside scores, reward and the workspace):
 *   - the key of an n-gram t0..t(k-1), k <= 4, is ((t0+1) << 48) | ((t1+1) << 32) | ((t2+1) << 16) | (t3+1), absent positions contributing
 *     0; df_keys [df_n] holds the keys of the table strictly ascending AS UNSIGNED 64-bit integers, df_vals [df_n] their df (>= 1);
 *   - df(g) = df_vals[i] where df_keys[i] is g's key, 0 when the table has no such key.  A token < 0 or >= 65535 inside a string makes
 *     every n-gram that contains it a miss (df 0): no key is formed from such a token, so it cannot alias another n-gram;
 *   - idf = logf((float)n_docs) - logf(fmaxf(1.f, (float)df)), in that order; weight = tf * idf, also for a miss (tf * logf(n_docs));
 *   - there is no `mult` factor anywhere: mult only says how many hypotheses a group has (in vlp_cider_d it doubles df because the
 *     reference sets are listed twice);
 *   - the lookup is a lower-bound binary search over df_keys with unsigned 64-bit comparison, at most ceil(log2(df_n + 1)) probes, one
 *     lane per (position, order) so that the probes of a string overlap.  The table is read only through vector loads; nothing is ever
 *     written to it.
 * Accepted beyond vlp_cider_d's conditions on `s`: df_n >= 0 (an empty table is legal and makes every df 0; the two arrays are then not
 * read), 1 <= n_docs <= 2^24 (so that (float)n_docs is exact), df_keys non-null and 8-byte aligned and df_vals non-null and 4-byte aligned
 * when df_n > 0, s.workspace of vlp_cider_d_df_workspace_bytes() bytes (0 for a refused shape; larger than vlp_cider_d's: idf is kept as a
 * full-width fp32 per hypothesis position and order, table df reaches 2^24).  Anything else returns VLP_ERR_BAD_ARG before a launch. */
typedef struct {
    vlp_cider_d_args s;                                        /* strings, shapes, outputs and workspace, as for vlp_cider_d */
    const uint64_t* df_keys;                                   /* [df_n] strictly ascending (unsigned) */
    const int32_t* df_vals;                                    /* [df_n] 1 <= df <= n_docs */
    int64_t df_n;
    int64_t n_docs;                                            /* documents the table was counted over */
} vlp_cider_d_df_args;
int64_t vlp_cider_d_df_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult);
int vlp_cider_d_df(const vlp_cider_d_df_args* a, void* stream);

/* The two entries above for K = mult samples per image, 2 <= mult <= 16, with a leave-one-out baseline (self-critical training with several
 * samples per image).  Same argument structs, same row layout (hypothesis row i belongs to group i % G), same kernels (the scoring block
 * has 64 * mult threads), every other shape limit unchanged.  Scores are what the specifications above give for that mult: without a table
 * df(g) = mult * the number of groups that hold g and ref_len = log(mult*G); with a table there is no mult factor.
 *   - reward (optional) is [mult*G] in the row order of hyp: reward[k*G + g] = s[k*G + g] - (sum over j != k of s[j*G + g]) / (mult - 1),
 *     the sum over the stored fp32 scores in ascending j starting from 0, then one divide and one subtract: a fixed order, bit-equal
 *     repeats.  With mult == 2 reward[g] equals the two entries' above bit for bit and reward[G + g] == -reward[g].
 * Nothing is written outside scores[0, mult*G), reward[0, mult*G) and the workspace; no atomics; two capturable launches.  The workspace
 * sizes are the functions below (0 for a refused shape, mult == 1 included); vlp_cider_d / vlp_cider_d_df keep refusing mult > 2. */
int64_t vlp_cider_d_multi_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult);
int vlp_cider_d_multi(const vlp_cider_d_args* a, void* stream);
int64_t vlp_cider_d_multi_df_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult);
int vlp_cider_d_multi_df(const vlp_cider_d_df_args* a, void* stream);

/* Consensus selection among the K samples of an image (minimum-Bayes-risk decoding under CIDEr-D): every sample is scored against the
 * image's other K - 1 samples as its references, and the sample with the largest score is picked.  No references are needed.  hyp is int64
 * [K*G, T] in sample-major order: row k*G + g is sample k of image g.  Strings, the table (key packing, ids outside 0..65534 form no key, an
 * empty table is legal, unsigned lower-bound search, read only) and idf = logf((float)n_docs) - logf(fmaxf(1.f, (float)df)) are
 * vlp_cider_d_df's: a string is a row's ids up to AND INCLUDING the first 0, or all T ids without one; nothing behind the first 0 is read.
 *   - utility [K*G] f32: utility[k*G + g] is what CiderD(df=<DocFreq>).compute_score gives for sample k of image g with the image's samples
 *     j != k as its references, in ascending j.  The arithmetic and its order are vlp_cider_d_df's: per reference and order the clipped
 *     product, divided by the two norms when both are non-zero, times the Gaussian penalty on the bigram-count lengths, accumulated per
 *     order over the references, then (acc0 + acc1 + acc2 + acc3) / 4 / (K - 1) * 10;
 *   - pick [G] int32: the lowest k whose stored fp32 utility[k*G + g] is the largest of image g;
 *   - pair [G, K, K] f32, optional (NULL: not written): pair[g][k][j] is the same score of sample k with sample j as its only reference
 *     (divisor 1); the diagonal is written as 0.  Not symmetric: the clipping uses the reference's weight.  utility and pick are the same
 *     bits with and without pair.
 * Two launches (cider_count_kernel over the K*G rows alone; one scoring block per image with 64 * K threads, the K rows staged once in LDS
 * and serving both roles), no host involvement, capturable; no atomics, every sum in a fixed order: equal inputs give bit-equal outputs.
 * Nothing is written outside utility[0, K*G), pick[0, G), pair[0, G*K*K) and the workspace.
 * Accepted: 1 <= T <= 64, 2 <= K <= 16, 1 <= G <= 1024, hyp_ld >= T, sigma > 0, non-null hyp / utility / pick, vlp_cider_d_df's table
 * conditions, a 16-byte aligned workspace of vlp_cider_d_consensus_workspace_bytes() bytes (0 for a refused shape).  Anything else returns
 * VLP_ERR_BAD_ARG before a launch. */
typedef struct {
    const int64_t* hyp; int64_t hyp_ld;                        /* [K*G, T]; row k*G + g is sample k of image g */
    int32_t G, K, T;
    float sigma;                                               /* 6.0 */
    const uint64_t* df_keys;                                   /* [df_n] strictly ascending (unsigned) */
    const int32_t* df_vals;                                    /* [df_n] 1 <= df <= n_docs */
    int64_t df_n;
    int64_t n_docs;
    float* utility;                                            /* [K*G] out */
    int32_t* pick;                                             /* [G] out */
    float* pair;                                               /* optional [G, K, K] out */
    void* workspace; int64_t workspace_bytes;
} vlp_cider_d_consensus_args;
int64_t vlp_cider_d_consensus_workspace_bytes(int32_t G, int32_t K, int32_t T);
int vlp_cider_d_consensus(const vlp_cider_d_consensus_args* a, void* stream);

/* Sentence BLEU-4 of id strings, the weighted mix with the CIDEr-D scores of a preceding vlp_cider_d* launch and the baseline of the mixed
 * scores (SCST with the reward cider_weight * CIDEr-D + bleu_weight * BLEU-4).  The specification is vlp_amd/scst.py Bleu.compute_score
 * (coco-caption's per-sentence BLEU with option='closest') on the strings array_to_str makes.  Strings, groups and ref_count are
 * vlp_cider_d's: a string is a row's ids up to AND INCLUDING the first 0 (all T without one), hypothesis row i belongs to group i % G, the
 * first ref_count[g] (clamped to 1..R, NULL = R) reference rows of a group are valid; nothing behind a row's first 0 and no invalid
 * reference row is read as text.  n-grams are compared token by token, never hashed.  Per hypothesis h:
 *   - len_h = its number of tokens; reflen = the valid reference length closest to len_h, the shorter on a tie;
 *   - correct_k (k = 1..4) = sum over the distinct k-grams g of h of min(count_h(g), max over the valid references of count_r(g)), exact
 *     integers; guess_k = max(0, len_h - k + 1);
 *   - fp32: p_0 = 1, p_k = p_(k-1) * ((correct_k + 1e-15f) / (guess_k + 1e-9f)); bleu4 = powf(p_4, 0.25f), times
 *     expf((len_h - reflen) / len_h) when len_h < reflen (the brevity penalty exp(1 - reflen / len_h));
 *   - stats (optional) [i][0..6) = correct_1..4, len_h, reflen: the integers the score is made of;
 *   - mixed (optional) [i] = w_base * base[i] + w_bleu * bleu4[i] -- two fp32 multiplications and one fp32 addition, never contracted into
 *     an fma -- or w_bleu * bleu4[i] when base is NULL.  mixed may be the same array as base (element i is read before it is written, by
 *     the thread that writes it);
 *   - reward (optional, needs mixed) over the stored mixed values m, with the formulas and summation order of the vlp_cider_d entries:
 *     VLP_BLEU_REWARD_PAIR (mult == 2): reward [G], [g] = m[g] - m[G + g];  VLP_BLEU_REWARD_LOO (mult >= 2): reward [mult*G],
 *     [k*G + g] = m[k*G + g] - (sum over j != k of m[j*G + g], ascending j from 0) / (mult - 1).
 * One launch (one block per group, one wave per hypothesis, one lane per position), no workspace, no host involvement, capturable; the
 * accurate logf / expf / powf, every sum in a fixed order, no atomics: equal inputs give bit-equal outputs.  Nothing is written outside
 * bleu4[0, mult*G), stats[0, 6*mult*G), mixed[0, mult*G) and reward.
 * Accepted: 1 <= T <= 64, 1 <= R <= 8, 1 <= G <= 1024, 1 <= mult <= 16, non-null hyp / ref / bleu4, hyp_ld / ref_ld >= T, ref_group_stride
 * >= (R-1) * ref_ld + T, reward only with mixed and a mode that fits mult.  Anything else returns VLP_ERR_BAD_ARG before a launch. */
enum { VLP_BLEU_REWARD_PAIR = 0, VLP_BLEU_REWARD_LOO = 1 };
typedef struct {
    const int64_t* hyp; int64_t hyp_ld;                        /* [mult*G, T]; row i is scored against group i % G */
    const int64_t* ref; int64_t ref_group_stride, ref_ld;      /* [G, R, T] */
    const int32_t* ref_count;                                  /* [G] or NULL = all R */
    int32_t G, R, T, mult;
    float* bleu4;                                              /* [mult*G] out */
    int32_t* stats;                                            /* optional [mult*G, 6] out */
    const float* base;                                         /* optional [mult*G]: the CIDEr-D scores */
    float w_base, w_bleu;
    float* mixed;                                              /* optional [mult*G] out */
    float* reward;                                             /* optional out, [G] (pair) or [mult*G] (leave-one-out); needs mixed */
    int32_t reward_mode;                                       /* VLP_BLEU_REWARD_* */
} vlp_bleu4_args;
int vlp_bleu4(const vlp_bleu4_args* a, void* stream);

/* Caption metrics of id strings (evaluation, not a reward): per group g -- one image -- the CIDEr-D score of its one hypothesis against a
 * resident document-frequency table, the six integers corpus BLEU-1..4 is made of, and per reference the longest common subsequence
 * ROUGE-L is made of.  The specifications are vlp_amd/scst.py CiderD(df=<DocFreq>).compute_score and Bleu.sentence_stats and
 * vlp_amd/caption_metrics.py lcs_len.  Operands, strides, ref_count and the table are vlp_cider_d_df's (d.s.mult must be 1, d.s.reward NULL;
 * d.s.scores is the cider output), with ONE difference in how a row is read:
 *   - a string is a WORD STRING: the ids of a row BEFORE its first 0, or all T ids without one.  The 0 is padding and never a token, an
 *     empty string is legal, nothing from the first 0 on is read as text, and no invalid reference row is read at all.
 * Outputs:
 *   - d.s.scores [G] f32: vlp_cider_d_df's arithmetic on the word strings (same operations, same order).  An empty string has no n-grams,
 *     zero norms and length 0;
 *   - bleu_stats [G, 6] int32 = correct_1..4, len_h, reflen: vlp_bleu4's stats on the word strings (reflen = the valid reference length
 *     closest to len_h, the shorter on a tie; an empty valid reference has length 0);
 *   - lcs [G, R, 2] int32 = (length of the longest common subsequence of the hypothesis and reference r, len_r), (0, 0) for an invalid
 *     reference row.
 * Three launches (counting, scoring, LCS), no host involvement, capturable; no atomics, every sum in a fixed order: equal inputs give
 * bit-equal outputs.  Nothing is written outside the three outputs and the workspace.
 * Accepted: what vlp_cider_d_df accepts with mult == 1 (1 <= T <= 64, 1 <= R <= 8, 1 <= G <= 1024, the strides, sigma > 0, the table
 * conditions), non-null bleu_stats and lcs, a 16-byte aligned workspace of vlp_caption_eval_workspace_bytes() bytes (0 for a refused
 * shape).  Anything else returns VLP_ERR_BAD_ARG before a launch. */
typedef struct {
    vlp_cider_d_df_args d;                                     /* strings, shapes, cider output, workspace and table */
    int32_t* bleu_stats;                                       /* [G, 6] out */
    int32_t* lcs;                                              /* [G, R, 2] out */
} vlp_caption_eval_args;
int64_t vlp_caption_eval_workspace_bytes(int32_t G, int32_t R, int32_t T);
int vlp_caption_eval(const vlp_caption_eval_args* a, void* stream);

/* VQA loss (modeling.py:1030,1140): BCEWithLogits(mean) * num_answers. fwd -> loss[0] (loss must hold
 * 257 floats: loss[1..257) is scratch);
 * bwd -> dlogits = grad_scale * (sigmoid(x) - y) / B, zero for columns >= N. */
int vlp_bce_loss_fwd(const void* logits, int64_t ld, const void* labels_f32, int64_t ldl, int32_t B, int32_t N,
                     float* loss, void* stream);
int vlp_bce_loss_bwd(const void* logits, int64_t ld, const void* labels_f32, int64_t ldl, int32_t B, int32_t N,
                     const float* grad_scale, void* dlogits, int64_t ldd, void* stream);
/* The same two with the target given as what a VQA question has -- at most S <= 16 (answer index, score) pairs per row -- instead of a dense
 * f32 [B, N] array:  y[b, n] = ans_score[b, s] where ans_idx[b, s] == n, else 0.  ans_idx i32 [B, S] / ans_score f32 [B, S], contiguous;
 * ans_idx == -1 marks an empty slot; the caller guarantees that the indices of a row are distinct and every index is -1 or in [0, N)
 * (seq2seq_loader.py:355 builds the dense vector from such pairs).  The kernels are the dense kernels instantiated with another source of y
 * (the pairs of the rows a block works on sit in LDS): same element order, same expression, same summation order, so loss[0] and dlogits equal
 * the dense entry points' on the densified target bit for bit.  No atomics. */
int vlp_bce_sparse_loss_fwd(const void* logits, int64_t ld, const int32_t* ans_idx, const float* ans_score, int32_t S, int32_t B, int32_t N,
                            float* loss, void* stream);
int vlp_bce_sparse_loss_bwd(const void* logits, int64_t ld, const int32_t* ans_idx, const float* ans_score, int32_t S, int32_t B, int32_t N,
                            const float* grad_scale, void* dlogits, int64_t ldd, void* stream);
/* VQA answer choice (modeling.py:1046 `argmax(pred[:, 1:]) + 1`, eval_vqa2.py): per row of logits f16 [rows, ld] the FIRST maximum over
 * columns [first_col, N): out_ids[r] = its absolute column, out_vals[r] = the maximum.  Columns < first_col and >= N (row padding) are never
 * chosen.  With ans_idx / ans_score (as above) given, out_scores[r] = the score row r lists for out_ids[r], 0 if it lists none (the soft
 * accuracy of the prediction); with ans_idx == NULL out_scores is not touched (it may be NULL).  One launch, no fp32 copy of the logits. */
int vlp_vqa_answer_rows(const void* logits, int64_t ld, int32_t rows, int32_t N, int32_t first_col, const int32_t* ans_idx,
                        const float* ans_score, int32_t S, int64_t* out_ids, float* out_vals, float* out_scores, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimizers
 * vlp_sumsq: out[0] = sum(g^2) in f32, out[1] = 1.0 if any element is inf/nan else 0 (the overflow
 * check + grad norm of apex FP16_Optimizer._compute_grad_norm).  partial = f32 scratch [2048].
 */
int vlp_sumsq(const void* g_f16, int64_t n, float* out2, float* partial, void* stream);
/* ABI 3: the same over another range, ADDED to out2 (sum += , flag = max): the sharded optimizer step (vlp_amd/distributed.py ShardPlan)
 * sums over the chunks a rank owns; launches of one stream run in order, so the total is reproducible. */
int vlp_sumsq_acc(const void* g_f16, int64_t n, float* out2, float* partial, void* stream);

/* apex fused_adam_cuda.adam as called by FusedAdam.step (run_img2txt_dist.py:411-420):
 *   g = g16 / (*combined_scale); m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 *   denom = eps_inside_sqrt ? sqrt(v + eps) : sqrt(v) + eps;
 *   p32 -= step_size * (m / denom + decay * p32); p16 = half(p32)
 * hyper points to 3 device floats {combined_scale, step_size, skip}; when skip != 0 (overflow) the
 * kernel leaves all state untouched -- so the loss-scale logic never forces a host sync.
 */
typedef struct {
    float* p32; float* m; float* v;      /* master weights and moments [n] */
    const void* g16;                     /* [n] fp16 gradients (still multiplied by the loss scale) */
    void* p16;                           /* [n] fp16 model weights out */
    int64_t n;
    float b1, b2, eps, decay;
    int32_t eps_inside_sqrt;
    const float* hyper;                  /* device {combined_scale, step_size, skip} */
} vlp_fused_adam_args;
int vlp_fused_adam(const vlp_fused_adam_args* a, void* stream);
/* device-side scalar logic of FP16_Optimizer.step + FusedAdam.step for one param group:
 *   scale = scale_state[0]; norm = sqrt(sumsq[0]); overflow = max(sumsq[1], any_overflow[0]);
 *   clip = (norm/scale + 1e-6)/max_grad_norm; combined = scale * max(clip, 1); hyper = {combined, step_size, overflow} */
int vlp_adam_hyper(const float* sumsq2, const float* any_overflow, const float* scale_state, float max_grad_norm,
                   float step_size, float* hyper3, void* stream);
/* apex FP16_Optimizer._update_scale on the device, so the loss scale never forces a host sync.
 * scale_state (8 device floats) = {cur_scale, cur_iter, last_overflow_iter, scale_factor, scale_window, dynamic,
 * skipped_steps, reserved}: on overflow cur_scale = max(cur_scale / factor, 1), last_overflow_iter = cur_iter; otherwise
 * cur_scale *= factor whenever (cur_iter - last_overflow_iter) % window == 0; then cur_iter += 1. */
int vlp_loss_scale_update(float* scale_state, const float* overflow, void* stream);

/* BertAdam (optimization.py:112-182) over a flat fp32 master buffer made of `ntensors` tensors:
 * per-tensor L2 clip to max_grad_norm (:146-147), no bias correction, decoupled decay, lr already
 * scheduled by the host (warmup_linear :45-48).  seg_off[ntensors+1] (int64, device) are the tensor
 * boundaries inside the flat buffers.  g may be fp16 or fp32.
 * norms: f32 scratch of vlp_bert_adam_norms_floats(n, ntensors) floats (ABI 2; it was [ntensors] in ABI 1): [0, ntensors) receive the
 * per-tensor squared gradient norms, the rest holds one partial sum per (4096-element chunk, tensor) pair, which a second kernel adds
 * up in a fixed order -- no atomics: the clip factors, hence the update, are bitwise reproducible.
 */
int64_t vlp_bert_adam_norms_floats(int64_t n, int32_t ntensors);
typedef struct {
    float* p32; float* m; float* v;
    const void* g; int32_t g_is_f32;
    void* p16;                           /* optional fp16 copy out (NULL for pure-fp32 use) */
    const int64_t* seg_off; int32_t ntensors; int64_t n;
    float* norms; int64_t norms_floats;  /* ABI 3: size of `norms` in floats, checked against vlp_bert_adam_norms_floats() */
    float lr, b1, b2, eps, decay, max_grad_norm;
    float grad_scale;                    /* gradients are divided by this (loss scale), 1 for fp32 */
    const int32_t* active;               /* [ntensors] device flags or NULL: tensors with 0 are skipped entirely
                                            (the reference skips parameters whose .grad is None, optimization.py:125-126) */
} vlp_bert_adam_args;
int vlp_bert_adam(const vlp_bert_adam_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VLP_HIP_H */
