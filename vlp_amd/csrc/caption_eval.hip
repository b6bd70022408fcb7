// Caption metrics on the device (vlp_caption_eval, include/vlp_hip.h): per image the CIDEr-D score against a resident document-frequency table,
// the six integers corpus BLEU-1..4 is made of, and per reference the longest common subsequence ROUGE-L is made of.  The specifications are
// vlp_amd/scst.py CiderD(df=<DocFreq>) and Bleu.sentence_stats and vlp_amd/caption_metrics.py Rouge, all on WORD STRINGS: the ids of a row
// before its first 0 (the 0 is padding, never a token; an empty string is legal).  The reward kernels of reward.hip read a row up to and
// including that 0; the staging and matching helpers of both files are reward_common.h's, instantiated here with END = 0.
//
//   ce_count_kernel   cider_count_kernel<true> of reward.hip for word strings and one hypothesis per group: one block per string (the G
//                     hypotheses, then the G*R references), one lane per (position, order) looks the n-gram up in the table; wave 0 then
//                     counts multiplicity and first occurrence inside the string and writes the four L2 norms, and for a hypothesis
//                     (tf, first) and idf per position and order.
//   ce_score_kernel   one wave per group, one lane per hypothesis position: the count of the n-grams that start there in every valid
//                     reference.  The counts feed both cider_score_kernel<true>'s arithmetic (clipped products, norms, Gaussian penalty,
//                     mean, x 10: the same operations in the same order) and bleu4_kernel's integers (correct_1..4, len_h, closest reflen).
//   ce_lcs_kernel     one wave per (hypothesis, reference) pair, lane q holding reference token q.  For hypothesis token j the ballot
//                     M = (ref_q == h_j, q < len_r) is the match mask of the whole reference; the wave-uniform 64-bit recurrence
//                     V = ~0;  u = V & M;  V = (V + u) | (V & ~M)  (the carry out of bit 63 dropped) keeps a 0 bit per step of the LCS
//                     row, so lcs = popcount(~V & mask(len_r)) after the last token: at most 64 ballots and scalar arithmetic per pair,
//                     no LDS, no divergence.  The quadratic DP of caption_metrics.lcs_len is the specification.
// fp32 with the accurate logf / expf / sqrtf, every sum in a fixed order, no atomics: equal inputs give bit-equal outputs.
#include "reward_common.h"

__global__ __launch_bounds__(CD_THREADS) void ce_count_kernel(vlp_cider_d_args a, int* info, float* idf_out, float* norms, cd_table tab) {
    __shared__ int qrow[64 + CD_PAD], srow[64 + CD_PAD];               // the block's string with the query's / a reference's sentinel
    __shared__ int cnt[4][64];
    const int T = a.T, R = a.R, G = a.G;
    const int s = blockIdx.x, tid = threadIdx.x, k = tid >> 6, q = tid & 63;
    const bool is_hyp = s < G;
    const int64_t* src;
    if (is_hyp) {
        src = a.hyp + (int64_t)s * a.hyp_ld;
    } else {
        const int row = s - G, g = row / R, r = row - g * R;
        if (r >= cd_ref_count(a.ref_count, g, R)) return;              // not a reference of its group: nobody reads its norms (block-uniform)
        src = a.ref + (int64_t)g * a.ref_group_stride + (int64_t)r * a.ref_ld;
    }
    if (tid < 64) {                                                    // wave 0: the block's own string
        const int tok = tid < T ? (int)src[tid] : CD_HYP_END;
        const int len = cd_len_of<0>(__ballot(tid < T && tok == 0), T);
        if (tid < T) {
            qrow[tid] = tid < len ? tok : CD_HYP_END;
            srow[tid] = tid < len ? tok : CD_REF_END;
        }
        if (tid < CD_PAD) {
            qrow[T + tid] = CD_HYP_END;
            srow[T + tid] = CD_REF_END;
        }
    }
    __syncthreads();
    // lane (order k, position q): the table df of the k+1-gram that starts there.  A sentinel (the string ends inside the n-gram) or an id
    // outside [0, 65535) forms no key: df 0
    int df = 0;
    if (q < T) {
        uint64_t key = 0;
        bool ok = true;
        for (int j = 0; j <= k; ++j) {
            const int t = qrow[q + j];
            ok = ok && t >= 0 && t < 65535;
            key |= (uint64_t)(((unsigned)t + 1u) & 0xffffu) << (48 - 16 * j);   // (used only when every id is in range)
        }
        if (ok) df = cd_table_df(tab, key);
    }
    cnt[k][q] = df;
    __syncthreads();
    if (tid >= 64) return;

    // wave 0, lane = position: multiplicity and first occurrence inside the own string, then weights and norms
    int tf[4] = {0, 0, 0, 0}, first[4] = {1, 1, 1, 1};
    if (tid < T) {
        const int a0 = qrow[tid], a1 = qrow[tid + 1], a2 = qrow[tid + 2], a3 = qrow[tid + 3];
        int b0 = srow[0], b1 = srow[1], b2 = srow[2];
        for (int p = 0; p < T; ++p) {
            const int b3 = srow[p + 3];
            const int m = cd_match(a0, a1, a2, a3, b0, b1, b2, b3);
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                tf[o] += m > o;
                first[o] &= !(m > o && p < tid);
            }
            b0 = b1; b1 = b2; b2 = b3;
        }
    }
    const float ref_len = logf(tab.n_docs);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const float idf = ref_len - logf(fmaxf(1.f, (float)(tid < T ? cnt[o][tid] : 0)));
        float v = 0.f;
        if (tid < T && tf[o] > 0 && first[o]) v = (float)tf[o] * idf;
        const float n2 = wave_sum(v * v);
        if (tid == 0) norms[(int64_t)s * 4 + o] = sqrtf(n2);
        if (is_hyp && tid < T) {
            info[((int64_t)s * 4 + o) * T + tid] = cd_pack(0, tf[o], tf[o] > 0 && first[o]);
            idf_out[((int64_t)s * 4 + o) * T + tid] = idf;
        }
    }
}

__global__ __launch_bounds__(64) void ce_score_kernel(vlp_cider_d_args a, const int* info, const float* idf_in, const float* norms, int32_t* stats) {
    __shared__ int cd_refs[8 * (64 + CD_PAD)];                         // [R][T + CD_PAD]
    __shared__ int ref_len_s[8];
    const int T = a.T, R = a.R, G = a.G, ldr = T + CD_PAD;
    const int g = blockIdx.x, lane = threadIdx.x;
    cd_stage_refs<0>(a, g * R, R, cd_refs, ref_len_s, 64, 64);

    const int tok = lane < T ? (int)a.hyp[(int64_t)g * a.hyp_ld + lane] : CD_HYP_END;
    const int len = cd_len_of<0>(__ballot(lane < T && tok == 0), T);
    int av[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = __shfl(tok, (lane + j) & 63, 64);
        av[j] = lane + j < len ? t : CD_HYP_END;
    }
    __syncthreads();

    float idf[4], hv[4], nh[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
    int tf[4], best[4] = {0, 0, 0, 0};
    bool first[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int pk = lane < T ? info[((int64_t)g * 4 + k) * T + lane] : 0;
        idf[k] = lane < T ? idf_in[((int64_t)g * 4 + k) * T + lane] : 0.f;
        tf[k] = (pk >> 11) & 127;
        hv[k] = (float)tf[k] * idf[k];
        first[k] = (pk >> 18) & 1;
        nh[k] = norms[(int64_t)g * 4 + k];
    }
    const int nr = cd_ref_count(a.ref_count, g, R);
    const float two_sigma2 = 2.f * a.sigma * a.sigma;
    int reflen = 0, refdist = 1 << 30;
    for (int r = 0; r < nr; ++r) {
        const int* row = cd_refs + r * ldr;
        int t[4] = {0, 0, 0, 0};
        int b0 = row[0], b1 = row[1], b2 = row[2];
        for (int q = 0; q < T; ++q) {
            const int b3 = row[q + 3];
            const int m = cd_match(av[0], av[1], av[2], av[3], b0, b1, b2, b3);
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] += m > k;
            b0 = b1; b1 = b2; b2 = b3;
        }
        // CIDEr-D: the clipped products of this reference
        const int lr = ref_len_s[r];
        const float delta = (float)(max(len - 1, 0) - max(lr - 1, 0));
        const float penalty = expf(-(delta * delta) / two_sigma2);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float rv = (float)t[k] * idf[k];
            float val = wave_sum(first[k] ? fminf(hv[k], rv) * rv : 0.f);
            const float nrk = norms[((int64_t)G + (int64_t)g * R + r) * 4 + k];
            if (nh[k] != 0.f && nrk != 0.f) val /= nh[k] * nrk;
            acc[k] += val * penalty;
        }
        // BLEU: the largest count over the references; the closest reference length, the shorter on a tie
#pragma unroll
        for (int k = 0; k < 4; ++k) best[k] = max(best[k], t[k]);
        const int d = abs(lr - len);
        if (d < refdist || (d == refdist && lr < reflen)) { refdist = d; reflen = lr; }
    }
    const float score = (acc[0] + acc[1] + acc[2] + acc[3]) / 4.f / (float)nr * 10.f;
    int correct[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) correct[k] = wave_sum_int(first[k] ? min(tf[k], best[k]) : 0);
    if (lane == 0) {
        a.scores[g] = score;
        int32_t* st = stats + (int64_t)g * 6;
        st[0] = correct[0]; st[1] = correct[1]; st[2] = correct[2]; st[3] = correct[3]; st[4] = len; st[5] = reflen;
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
    int* info = (int*)a->workspace;                                    // the layout of vlp_cider_d_df's workspace with mult = 1
    float* idf = (float*)(info + cd_info_ints(G, a->T, 1));
    float* norms = idf + cd_info_ints(G, a->T, 1);
    const cd_table tab = {d->df_keys, d->df_vals, d->df_n, (float)d->n_docs};
    hipLaunchKernelGGL(ce_count_kernel, dim3(G + SR), dim3(CD_THREADS), 0, (hipStream_t)stream, *a, info, idf, norms, tab);
    VLP_CHECK_LAUNCH("vlp_caption_eval");
    hipLaunchKernelGGL(ce_score_kernel, dim3(G), dim3(64), 0, (hipStream_t)stream, *a, (const int*)info, (const float*)idf, (const float*)norms, e->bleu_stats);
    VLP_CHECK_LAUNCH("vlp_caption_eval");
    hipLaunchKernelGGL(ce_lcs_kernel, dim3(cdiv(SR, CE_LCS_WAVES)), dim3(64 * CE_LCS_WAVES), 0, (hipStream_t)stream, *a, e->lcs);
    VLP_CHECK_LAUNCH("vlp_caption_eval");
    return VLP_OK;
}
