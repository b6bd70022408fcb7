// CIDEr-D of id strings on the device (vlp_cider_d, include/vlp_hip.h): the reward of self-critical sequence training without the host.
// The specification is vlp_amd/scst.py CiderD.compute_score on the strings array_to_str makes; this file restates it with exact integer
// counting and fp32 arithmetic in a fixed order (no atomics: equal inputs give bit-equal outputs).
//
// An n-gram is never hashed: two n-grams are equal when their tokens are.  For a query position p and a reference position q the MATCH
// LENGTH m(p, q) = the number of leading equal tokens of the two suffixes, capped at 4 and cut at either string's end, answers all four
// orders at once -- the k-gram at p equals the k-gram at q exactly when m >= k.  Strings are staged as int32 with a sentinel past their
// end (the query's is -1, a reference's -2, so two ends never match) and three sentinel columns behind every row: the inner loop is one
// LDS read and a few compares per (p, q), with no bounds test.
//
//   cider_count_kernel   (reward_common.h, shared with caption_eval.hip) one block per string (the mult*G hypotheses, then the G*R references).
//                        A worker = P consecutive lanes (P = the power of two >= T), one lane per position of the block's string; the 256 / P
//                        workers share the groups of a tile of references staged in LDS.  Per position and order: the number of groups whose
//                        valid references hold the n-gram (-> df), its multiplicity in its own string (tf) and whether it is the first
//                        occurrence there.  From them the string's four L2 norms; a hypothesis also keeps (df, tf, first) per position.
//   cider_score_kernel   one block per group, one wave per hypothesis, one lane per position: tf of the hypothesis' n-grams in each
//                        valid reference of its group, the clipped dot products, norms, length penalty, mean; then the reward.
//
// Every scoring kernel of this file and of caption_eval.hip is a composition of reward_common.h's pieces: cd_load_hyp (the hypothesis in
// registers), cd_stage_refs / cd_stage_wave_row (the references in LDS), cd_load_weights (what the counting pass left), cd_count_row (the
// walk over one reference), then cd_cider_terms (CIDEr-D) and / or cd_count_own, cd_bleu_update, cd_bleu_correct (BLEU), and cd_baseline (the
// reward).  Each loop exists once, so two entries given the same strings agree bit for bit (tests/test_88_ngram_family_gpu.py).
//
// vlp_cider_d_multi / vlp_cider_d_multi_df are the same two kernels with 2..16 hypotheses per group (64 * mult threads in the scoring block) and
// the leave-one-out reward: every hypothesis against the mean of the group's other scores.
//
// vlp_cider_d_consensus scores the K samples of an image against each other (consensus selection): the counting kernel with TABLE = true over
// the sample rows alone, and a scoring kernel whose references are the block's own rows.
//
// vlp_bleu4 (at the end of this file): sentence BLEU-4 of the hypotheses, its weighted mix with the CIDEr-D scores and the reward of the mixed
// scores, in one launch of the scoring kernel's shape.
//
// vlp_cider_d_df takes df from a resident table (sorted uint64 keys, int32 df; vlp_amd/scst.py DocFreq) instead of the call's references.
// Both kernels are the ones above with TABLE = true: the counting pass drops its loop over the groups -- every (position, order) of the
// block's string gets a lane of its own that packs the n-gram's key and looks it up (cd_key_df: a lower-bound binary search of dependent
// global loads: 256 independent searches per block overlap) -- and hands the scoring pass idf as a full-width fp32 next to the packed
// (tf, first), since table df does not fit cd_pack's 11 bits.
// END = 1 in this file: the 0 is a token.
#include "reward_common.h"

// TABLE: idf of each hypothesis position and order comes from idf_in (the counting pass wrote it), not from the packed group count.
// LOO: reward [mult*G] = each score minus the mean of the group's other scores, else reward [G] = scores[g] - scores[G + g] (mult == 2).
template <bool TABLE>
__global__ __launch_bounds__(64 * CD_MAX_MULT) void cider_score_kernel(vlp_cider_d_args a, const int* info, const float* norms, const float* idf_in, int loo) {
    extern __shared__ __attribute__((aligned(16))) int cd_refs[];      // [R][T + CD_PAD]
    __shared__ int ref_len_s[8];
    __shared__ float sc[CD_MAX_MULT];
    const int T = a.T, R = a.R, G = a.G, ldr = T + CD_PAD, SH = a.mult * G;
    const int g = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = w * G + g;
    cd_stage_refs(a, g * R, R, cd_refs, ref_len_s, 64, blockDim.x);
    int tok, av[4];
    const int len = cd_load_hyp<1>(a.hyp + (int64_t)h * a.hyp_ld, T, lane, tok, av);
    __syncthreads();

    float idf[4], hv[4], nh[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
    int tf[4], first[4], t[4];
    cd_load_weights<TABLE>(info, idf_in, norms, h, T, lane, a.mult, SH, idf, tf, hv, first, nh);
    const int nr = cd_ref_count(a.ref_count, g, R);
    const float two_sigma2 = 2.f * a.sigma * a.sigma;
    for (int r = 0; r < nr; ++r) {
        cd_count_row(av, cd_refs + r * ldr, T, t);
        cd_cider_terms(t, idf, hv, first, nh, norms + ((int64_t)SH + (int64_t)g * R + r) * 4, len, ref_len_s[r], two_sigma2, acc, nullptr);
    }
    const float score = (acc[0] + acc[1] + acc[2] + acc[3]) / 4.f / (float)nr * 10.f;
    if (lane == 0) {
        a.scores[h] = score;
        sc[w] = score;
    }
    if (a.reward) cd_baseline(sc, a.mult, G, g, loo, a.reward);
}

extern "C" int64_t vlp_cider_d_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult) {
    return cd_shape_ok(G, R, T, mult) ? cd_workspace_bytes(G, R, T, mult, false) : 0;
}
extern "C" int64_t vlp_cider_d_multi_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult) {
    return cd_shape_ok(G, R, T, mult, true) ? cd_workspace_bytes(G, R, T, mult, false) : 0;
}
// workspace: int32 info[mult*G][4][T] (tf, first), f32 idf[mult*G][4][T], then f32 norms[mult*G + G*R][4]
extern "C" int64_t vlp_cider_d_df_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult) {
    return cd_shape_ok(G, R, T, mult) ? cd_workspace_bytes(G, R, T, mult, true) : 0;
}
extern "C" int64_t vlp_cider_d_multi_df_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult) {
    return cd_shape_ok(G, R, T, mult, true) ? cd_workspace_bytes(G, R, T, mult, true) : 0;
}

// the two launches of the four vlp_cider_d* entries: df from the table of `d`, or (d NULL) from the call's own references.  `who` names the
// entry in messages; the arguments were checked by the caller
static int cd_run(const vlp_cider_d_args* a, const vlp_cider_d_df_args* d, void* stream, bool multi, const char* who) {
    VLP_ENTER(a->ref, who);
    const int SH = a->mult * a->G, SR = a->G * a->R, ldr = a->T + CD_PAD;
    const cd_workspace ws = cd_carve(a->workspace, a->G, a->T, a->mult, d != nullptr);
    if (d) {
        cd_launch_count_table<1>(*a, SH + SR, ws, cd_table_of(d), stream);
    } else {
        int P = 1;                                                     // the power of two >= T
        while (P < a->T) P <<= 1;
        int tile_groups = CD_TILE_INTS / (a->R * ldr);                 // >= 15 at the largest accepted R, T
        if (tile_groups > a->G) tile_groups = a->G;
        hipLaunchKernelGGL((cider_count_kernel<false, 1>), dim3(SH + SR), dim3(CD_THREADS), (size_t)tile_groups * a->R * ldr * sizeof(int), (hipStream_t)stream,
                           *a, P, tile_groups, ws.info, ws.norms, cd_table{}, (float*)nullptr);
    }
    VLP_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(d ? cider_score_kernel<true> : cider_score_kernel<false>, dim3(a->G), dim3(64 * a->mult), (size_t)a->R * ldr * sizeof(int),
                       (hipStream_t)stream, *a, (const int*)ws.info, (const float*)ws.norms, (const float*)ws.idf, multi ? 1 : 0);
    VLP_CHECK_LAUNCH(who);
    return VLP_OK;
}

extern "C" int vlp_cider_d(const vlp_cider_d_args* a, void* stream) {
    VLP_CHECK_ARG(a, "vlp_cider_d: null args");
    const int64_t need = vlp_cider_d_workspace_bytes(a->G, a->R, a->T, a->mult);
    CD_CHECK_ARGS(a, "vlp_cider_d", need, false);
    return cd_run(a, nullptr, stream, false, "vlp_cider_d");
}

extern "C" int vlp_cider_d_multi(const vlp_cider_d_args* a, void* stream) {
    VLP_CHECK_ARG(a, "vlp_cider_d_multi: null args");
    const int64_t need = vlp_cider_d_multi_workspace_bytes(a->G, a->R, a->T, a->mult);
    CD_CHECK_ARGS(a, "vlp_cider_d_multi", need, true);
    return cd_run(a, nullptr, stream, true, "vlp_cider_d_multi");
}

extern "C" int vlp_cider_d_df(const vlp_cider_d_df_args* d, void* stream) {
    VLP_CHECK_ARG(d, "vlp_cider_d_df: null args");
    const vlp_cider_d_args* a = &d->s;
    const int64_t need = vlp_cider_d_df_workspace_bytes(a->G, a->R, a->T, a->mult);
    CD_CHECK_ARGS(a, "vlp_cider_d_df", need, false);
    CD_CHECK_TABLE(d, "vlp_cider_d_df");
    return cd_run(a, d, stream, false, "vlp_cider_d_df");
}

extern "C" int vlp_cider_d_multi_df(const vlp_cider_d_df_args* d, void* stream) {
    VLP_CHECK_ARG(d, "vlp_cider_d_multi_df: null args");
    const vlp_cider_d_args* a = &d->s;
    const int64_t need = vlp_cider_d_multi_df_workspace_bytes(a->G, a->R, a->T, a->mult);
    CD_CHECK_ARGS(a, "vlp_cider_d_multi_df", need, true);
    CD_CHECK_TABLE(d, "vlp_cider_d_multi_df");
    return cd_run(a, d, stream, true, "vlp_cider_d_multi_df");
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// vlp_cider_d_consensus: the K samples of an image scored against each other (consensus selection: keep the sample that agrees most with the
// others).  The counting pass is cider_count_kernel<true, 1> over the K*G sample rows alone -- a sample's norms in the reference role are its
// own --; the scoring block below composes the pieces cider_score_kernel<true> is made of, with the references taken from the block's own rows:
// one block per image, one wave per sample, one lane per position.  Every wave stages its row once in LDS with the reference's sentinel and
// keeps it in registers with the hypothesis' sentinel (the two ends stay distinct: two string ends never match), then walks the other K - 1
// rows in ascending j.
// ------------------------------------------------------------------------------------------------------------------------------------------
static inline bool cd_consensus_shape_ok(int32_t G, int32_t K, int32_t T) {
    return T >= 1 && T <= 64 && K >= 2 && K <= CD_MAX_MULT && G >= 1 && G <= 1024;
}

__global__ __launch_bounds__(64 * CD_MAX_MULT) void consensus_score_kernel(vlp_cider_d_consensus_args a, const int* info, const float* norms, const float* idf_in) {
    __shared__ int rows[CD_MAX_MULT][64 + CD_PAD];                     // the image's samples with a reference's sentinel
    __shared__ int len_s[CD_MAX_MULT];
    __shared__ float util[CD_MAX_MULT];
    const int T = a.T, G = a.G, K = a.K;
    const int g = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = w * G + g;
    int tok, av[4];
    const int len = cd_load_hyp<1>(a.hyp + (int64_t)h * a.hyp_ld, T, lane, tok, av);
    cd_stage_wave_row(rows[w], tok, len, lane);
    if (lane == 0) len_s[w] = len;
    __syncthreads();

    float idf[4], hv[4], nh[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
    int tf[4], first[4], t[4];
    cd_load_weights<true>(info, idf_in, norms, h, T, lane, 1, 1, idf, tf, hv, first, nh);
    const float two_sigma2 = 2.f * a.sigma * a.sigma;
    for (int j = 0; j < K; ++j) {
        if (j == w) continue;                                          // (wave-uniform)
        float one[4];                                                  // this reference alone
        cd_count_row(av, rows[j], T, t);
        cd_cider_terms(t, idf, hv, first, nh, norms + ((int64_t)j * G + g) * 4, len, len_s[j], two_sigma2, acc, one);
        const float single = (one[0] + one[1] + one[2] + one[3]) / 4.f * 10.f;
        if (a.pair && lane == 0) a.pair[((int64_t)g * K + w) * K + j] = single;
    }
    const float score = (acc[0] + acc[1] + acc[2] + acc[3]) / 4.f / (float)(K - 1) * 10.f;
    if (lane == 0) {
        a.utility[h] = score;
        util[w] = score;
        if (a.pair) a.pair[((int64_t)g * K + w) * K + w] = 0.f;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                            // the lowest k with the largest stored utility
        int best = 0;
        for (int k = 1; k < K; ++k)
            if (util[k] > util[best]) best = k;
        a.pick[g] = best;
    }
}

// workspace: cider_count_kernel<true, 1>'s for K*G hypotheses and no reference: int32 info[K*G][4][T], f32 idf[K*G][4][T], f32 norms[K*G][4]
extern "C" int64_t vlp_cider_d_consensus_workspace_bytes(int32_t G, int32_t K, int32_t T) {
    if (!cd_consensus_shape_ok(G, K, T)) return 0;
    const int64_t bytes = 4 * (2 * cd_info_ints(G, T, K) + 4 * (int64_t)K * G);
    return (bytes + 255) / 256 * 256;
}

extern "C" int vlp_cider_d_consensus(const vlp_cider_d_consensus_args* c, void* stream) {
    VLP_CHECK_ARG(c, "vlp_cider_d_consensus: null args");
    VLP_CHECK_ARG(cd_consensus_shape_ok(c->G, c->K, c->T), "vlp_cider_d_consensus: needs 1 <= T <= 64, 2 <= K <= 16, 1 <= G <= 1024 (G %d, K %d, T %d)", c->G,
                  c->K, c->T);
    VLP_CHECK_ARG(c->hyp && c->utility && c->pick && c->workspace, "vlp_cider_d_consensus: null operand");
    VLP_CHECK_ARG(c->hyp_ld >= c->T, "vlp_cider_d_consensus: hyp_ld shorter than the rows");
    CD_CHECK_SIGMA(c, "vlp_cider_d_consensus");
    const int64_t need = vlp_cider_d_consensus_workspace_bytes(c->G, c->K, c->T);
    CD_CHECK_WORKSPACE(c, "vlp_cider_d_consensus", need);
    CD_CHECK_TABLE(c, "vlp_cider_d_consensus");
    VLP_ENTER(c->hyp, "vlp_cider_d_consensus");
    vlp_cider_d_args a = {};                                           // the counting pass sees K*G hypotheses and no reference block
    a.hyp = c->hyp; a.hyp_ld = c->hyp_ld;
    a.G = c->G; a.R = 1; a.T = c->T; a.mult = c->K;
    const cd_workspace ws = cd_carve(c->workspace, c->G, c->T, c->K, true);
    cd_launch_count_table<1>(a, c->K * c->G, ws, cd_table_of(c), stream);
    VLP_CHECK_LAUNCH("vlp_cider_d_consensus");
    hipLaunchKernelGGL(consensus_score_kernel, dim3(c->G), dim3(64 * c->K), 0, (hipStream_t)stream, *c, (const int*)ws.info, (const float*)ws.norms,
                       (const float*)ws.idf);
    VLP_CHECK_LAUNCH("vlp_cider_d_consensus");
    return VLP_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// vlp_bleu4: sentence BLEU-4 of the hypotheses (vlp_amd/scst.py Bleu), mixed with the CIDEr-D scores of a preceding launch, and the baseline
// of the mixed scores.  One block per group, one wave per hypothesis, one lane per position, the group's valid references staged in LDS as
// above.  Per position and order a lane holds the n-gram's multiplicity in its own string (tf), whether it is the first occurrence there,
// and the maximum over the references of its count: the first occurrence of every distinct n-gram contributes min(tf, max count), an integer
// wave sum gives correct_k.  Lane 0 turns the six integers into the score in fp32.
// ------------------------------------------------------------------------------------------------------------------------------------------
struct bleu_out {
    float* bleu4;
    int32_t* stats;
    const float* base;
    float w_base, w_bleu;
    float* mixed;
    float* reward;
    int loo;
};

// wa * a + wb * b as two fp32 multiplications and one fp32 addition.  The library is built with -ffp-contract=fast, which fuses across
// statements and disregards pragmas (and __fmul_rn is a plain product here), so each product passes through an empty asm statement: the
// compiler cannot look through it, and what reaches the addition is the rounded product.
DEVFN float mix_unfused(float wa, float a, float wb, float b) {
    float x = wa * a, y = wb * b;
    asm volatile("" : "+v"(x), "+v"(y));
    return x + y;
}

__global__ __launch_bounds__(64 * CD_MAX_MULT) void bleu4_kernel(vlp_cider_d_args a, bleu_out o) {
    extern __shared__ __attribute__((aligned(16))) int cd_refs[];      // [R][T + CD_PAD]
    __shared__ int ref_len_s[8];
    __shared__ int hrow[CD_MAX_MULT][64 + CD_PAD];                     // each wave's own string with a reference's sentinel
    __shared__ float sc[CD_MAX_MULT];
    const int T = a.T, R = a.R, G = a.G, ldr = T + CD_PAD;
    const int g = blockIdx.x, w = threadIdx.x >> 6, lane = threadIdx.x & 63, h = w * G + g;
    cd_stage_refs(a, g * R, R, cd_refs, ref_len_s, 64, blockDim.x);
    int tok, av[4];
    const int len = cd_load_hyp<1>(a.hyp + (int64_t)h * a.hyp_ld, T, lane, tok, av);
    cd_stage_wave_row(hrow[w], tok, len, lane);
    __syncthreads();

    int tf[4], first[4], t[4], best[4] = {0, 0, 0, 0}, correct[4];
    cd_count_own(av, hrow[w], T, lane, tf, first);
    const int nr = cd_ref_count(a.ref_count, g, R);
    int reflen = 0, refdist = 1 << 30;
    for (int r = 0; r < nr; ++r) {
        cd_count_row(av, cd_refs + r * ldr, T, t);
        cd_bleu_update(t, ref_len_s[r], len, best, reflen, refdist);
    }
    cd_bleu_correct(tf, first, best, correct);

    if (lane == 0) {
        float p = 1.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) p = p * (((float)correct[k] + 1e-15f) / ((float)max(0, len - k) + 1e-9f));
        float b = powf(p, 0.25f);
        if (len < reflen) b *= expf((float)(len - reflen) / (float)len);       // exp(1 - reflen / len_h)
        o.bleu4[h] = b;
        if (o.stats) cd_bleu_stats(o.stats + (int64_t)h * 6, correct, len, reflen);
        if (o.mixed) {
            const float m = o.base ? mix_unfused(o.w_base, o.base[h], o.w_bleu, b) : o.w_bleu * b;
            o.mixed[h] = m;
            sc[w] = m;
        }
    }
    if (o.reward) cd_baseline(sc, a.mult, G, g, o.loo, o.reward);      // (the entry checked that mixed is there)
}

extern "C" int vlp_bleu4(const vlp_bleu4_args* b, void* stream) {
    VLP_CHECK_ARG(b, "vlp_bleu4: null args");
    VLP_CHECK_ARG(b->T >= 1 && b->T <= 64 && b->R >= 1 && b->R <= 8 && b->G >= 1 && b->G <= 1024 && b->mult >= 1 && b->mult <= CD_MAX_MULT,
                  "vlp_bleu4: needs 1 <= T <= 64, 1 <= R <= 8, 1 <= G <= 1024, 1 <= mult <= 16 (G %d, R %d, T %d, mult %d)", b->G, b->R, b->T, b->mult);
    VLP_CHECK_ARG(b->hyp && b->ref && b->bleu4, "vlp_bleu4: null operand");
    CD_CHECK_STRIDES(b, "vlp_bleu4");
    if (b->reward) {
        VLP_CHECK_ARG(b->mixed, "vlp_bleu4: the reward is computed from the mixed scores: reward without mixed");
        VLP_CHECK_ARG(b->reward_mode == VLP_BLEU_REWARD_PAIR || b->reward_mode == VLP_BLEU_REWARD_LOO, "vlp_bleu4: unknown reward_mode %d", b->reward_mode);
        VLP_CHECK_ARG(b->reward_mode != VLP_BLEU_REWARD_PAIR || b->mult == 2, "vlp_bleu4: reward = mixed[g] - mixed[G + g] needs mult == 2 (mult %d)", b->mult);
        VLP_CHECK_ARG(b->reward_mode != VLP_BLEU_REWARD_LOO || b->mult >= 2, "vlp_bleu4: the leave-one-out reward needs mult >= 2 (mult %d)", b->mult);
    }
    VLP_ENTER(b->ref, "vlp_bleu4");
    vlp_cider_d_args a = {};
    a.hyp = b->hyp; a.hyp_ld = b->hyp_ld;
    a.ref = b->ref; a.ref_group_stride = b->ref_group_stride; a.ref_ld = b->ref_ld;
    a.ref_count = b->ref_count;
    a.G = b->G; a.R = b->R; a.T = b->T; a.mult = b->mult;
    const bleu_out o = {b->bleu4, b->stats, b->base, b->w_base, b->w_bleu, b->mixed, b->reward, b->reward_mode == VLP_BLEU_REWARD_LOO ? 1 : 0};
    hipLaunchKernelGGL(bleu4_kernel, dim3(b->G), dim3(64 * b->mult), (size_t)b->R * (b->T + CD_PAD) * sizeof(int), (hipStream_t)stream, a, o);
    VLP_CHECK_LAUNCH("vlp_bleu4");
    return VLP_OK;
}
