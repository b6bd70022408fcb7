// Caption metrics on the device (vlp_caption_eval, include/vlp_hip.h): per image the CIDEr-D score against a resident document-frequency table,
// the six integers corpus BLEU-1..4 is made of, and per reference the longest common subsequence ROUGE-L is made of.  The specifications are
// vlp_amd/scst.py CiderD(df=<DocFreq>) and Bleu.sentence_stats and vlp_amd/caption_metrics.py Rouge, all on WORD STRINGS: the ids of a row
// before its first 0 (the 0 is padding, never a token; an empty string is legal).  The reward kernels of reward.hip read a row up to and
// including that 0; both files are composed of reward_common.h's pieces, instantiated here with END = 0.
//
//   counting pass     cider_count_kernel<true, 0> (reward_common.h: the kernel vlp_cider_d_df launches as <true, 1>) with one hypothesis per
//                     group: one block per string (the G hypotheses, then the G*R references), one lane per (position, order) looks the
//                     n-gram up in the table; wave 0 then counts multiplicity and first occurrence inside the string and writes the four L2
//                     norms, and for a hypothesis (tf, first) and idf per position and order.
//   ce_score_kernel   one wave per group, one lane per hypothesis position: cd_count_row counts the n-grams that start there in every valid
//                     reference once, and the counts feed both cd_cider_terms (cider_score_kernel<true>'s arithmetic: clipped products,
//                     norms, Gaussian penalty; then the mean, x 10) and cd_bleu_update / cd_bleu_correct (bleu4_kernel's integers:
//                     correct_1..4, len_h, closest reflen).
//   ce_lcs_kernel     one wave per (hypothesis, reference) pair, lane q holding reference token q.  For hypothesis token j the ballot
//                     M = (ref_q == h_j, q < len_r) is the match mask of the whole reference; the wave-uniform 64-bit recurrence
//                     V = ~0;  u = V & M;  V = (V + u) | (V & ~M)  (the carry out of bit 63 dropped) keeps a 0 bit per step of the LCS
//                     row, so lcs = popcount(~V & mask(len_r)) after the last token: at most 64 ballots and scalar arithmetic per pair,
//                     no LDS, no divergence.  The quadratic DP of caption_metrics.lcs_len is the specification.
// fp32 with the accurate logf / expf / sqrtf, every sum in a fixed order, no atomics: equal inputs give bit-equal outputs.
#include "reward_common.h"

__global__ __launch_bounds__(64) void ce_score_kernel(vlp_cider_d_args a, const int* info, const float* idf_in, const float* norms, int32_t* stats) {
    __shared__ int cd_refs[8 * (64 + CD_PAD)];                         // [R][T + CD_PAD]
    __shared__ int ref_len_s[8];
    const int T = a.T, R = a.R, G = a.G, ldr = T + CD_PAD;
    const int g = blockIdx.x, lane = threadIdx.x;
    cd_stage_refs<0>(a, g * R, R, cd_refs, ref_len_s, 64, 64);
    int tok, av[4];
    const int len = cd_load_hyp<0>(a.hyp + (int64_t)g * a.hyp_ld, T, lane, tok, av);
    __syncthreads();

    float idf[4], hv[4], nh[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
    int tf[4], first[4], t[4], best[4] = {0, 0, 0, 0}, correct[4];
    cd_load_weights<true>(info, idf_in, norms, g, T, lane, 1, 1, idf, tf, hv, first, nh);
    const int nr = cd_ref_count(a.ref_count, g, R);
    const float two_sigma2 = 2.f * a.sigma * a.sigma;
    int reflen = 0, refdist = 1 << 30;
    for (int r = 0; r < nr; ++r) {
        cd_count_row(av, cd_refs + r * ldr, T, t);
        cd_cider_terms(t, idf, hv, first, nh, norms + ((int64_t)G + (int64_t)g * R + r) * 4, len, ref_len_s[r], two_sigma2, acc, nullptr);
        cd_bleu_update(t, ref_len_s[r], len, best, reflen, refdist);
    }
    const float score = (acc[0] + acc[1] + acc[2] + acc[3]) / 4.f / (float)nr * 10.f;
    cd_bleu_correct(tf, first, best, correct);
    if (lane == 0) {
        a.scores[g] = score;
        cd_bleu_stats(stats + (int64_t)g * 6, correct, len, reflen);
    }
}

#define CE_LCS_WAVES 4
__global__ __launch_bounds__(64 * CE_LCS_WAVES) void ce_lcs_kernel(vlp_cider_d_args a, int32_t* out) {
    const int T = a.T, R = a.R;
    const int lane = threadIdx.x & 63, pair = blockIdx.x * CE_LCS_WAVES + (threadIdx.x >> 6);
    if (pair >= a.G * R) return;                                       // wave-uniform
    const int g = pair / R, r = pair - g * R;
    const bool valid = r < cd_ref_count(a.ref_count, g, R);            // an invalid reference row is never read
    const int h = lane < T ? (int)a.hyp[(int64_t)g * a.hyp_ld + lane] : 0;
    const int len_h = cd_len_of<0>(__ballot(lane < T && h == 0), T);
    const int t = (valid && lane < T) ? (int)a.ref[(int64_t)g * a.ref_group_stride + (int64_t)r * a.ref_ld + lane] : 0;
    const int len_r = valid ? cd_len_of<0>(__ballot(lane < T && t == 0), T) : 0;
    unsigned long long V = ~0ull;
    for (int j = 0; j < len_h; ++j) {
        const int hj = __shfl(h, j, 64);
        const unsigned long long M = __ballot(lane < len_r && t == hj);
        const unsigned long long u = V & M;
        V = (V + u) | (V & ~M);
    }
    const unsigned long long mask = len_r >= 64 ? ~0ull : (1ull << len_r) - 1ull;
    if (lane == 0) {
        out[(int64_t)pair * 2] = __popcll(~V & mask);
        out[(int64_t)pair * 2 + 1] = len_r;
    }
}

extern "C" int64_t vlp_caption_eval_workspace_bytes(int32_t G, int32_t R, int32_t T) {
    return cd_shape_ok(G, R, T, 1) ? cd_workspace_bytes(G, R, T, 1, true) : 0;
}

extern "C" int vlp_caption_eval(const vlp_caption_eval_args* e, void* stream) {
    VLP_CHECK_ARG(e, "vlp_caption_eval: null args");
    const vlp_cider_d_df_args* d = &e->d;
    const vlp_cider_d_args* a = &d->s;
    VLP_CHECK_ARG(a->mult == 1 && !a->reward, "vlp_caption_eval: one hypothesis per group and no reward (mult %d)", a->mult);
    const int64_t need = vlp_caption_eval_workspace_bytes(a->G, a->R, a->T);
    CD_CHECK_ARGS(a, "vlp_caption_eval", need, false);
    CD_CHECK_TABLE(d, "vlp_caption_eval");
    VLP_CHECK_ARG(e->bleu_stats && e->lcs, "vlp_caption_eval: null bleu_stats or lcs");
    VLP_ENTER(a->ref, "vlp_caption_eval");
    const int G = a->G, SR = a->G * a->R;
    const cd_workspace ws = cd_carve(a->workspace, G, a->T, 1, true);  // the layout of vlp_cider_d_df's workspace with mult = 1
    cd_launch_count_table<0>(*a, G + SR, ws, cd_table_of(d), stream);
    VLP_CHECK_LAUNCH("vlp_caption_eval");
    hipLaunchKernelGGL(ce_score_kernel, dim3(G), dim3(64), 0, (hipStream_t)stream, *a, (const int*)ws.info, (const float*)ws.idf, (const float*)ws.norms,
                       e->bleu_stats);
    VLP_CHECK_LAUNCH("vlp_caption_eval");
    hipLaunchKernelGGL(ce_lcs_kernel, dim3(cdiv(SR, CE_LCS_WAVES)), dim3(64 * CE_LCS_WAVES), 0, (hipStream_t)stream, *a, e->lcs);
    VLP_CHECK_LAUNCH("vlp_caption_eval");
    return VLP_OK;
}
