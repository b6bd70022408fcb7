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
//   cider_count_kernel   one block per string (the mult*G hypotheses, then the G*R references).  A worker = P consecutive lanes (P = the power
//                        of two >= T), one lane per position of the block's string; the 256 / P workers share the groups of a tile of
//                        references staged in LDS.  Per position and order: the number of groups whose valid references hold the
//                        n-gram (-> df), its multiplicity in its own string (tf) and whether it is the first occurrence there.  From
//                        them the string's four L2 norms; a hypothesis also keeps (df, tf, first) per position for the second pass.
//   cider_score_kernel   one block per group, one wave per hypothesis, one lane per position: tf of the hypothesis' n-grams in each
//                        valid reference of its group, the clipped dot products, norms, length penalty, mean; then the reward.
//
// vlp_cider_d_multi / vlp_cider_d_multi_df are the same two kernels with 2..16 hypotheses per group (64 * mult threads in the scoring block) and
// the leave-one-out reward: every hypothesis against the mean of the group's other scores.
//
// vlp_cider_d_consensus scores the K samples of an image against each other (consensus selection): the counting kernel with TABLE = true over
// the sample rows alone, and a scoring kernel of its own whose references are the block's own rows.
//
// vlp_bleu4 (at the end of this file) is a third kernel of the scoring kernel's shape: sentence BLEU-4 of the hypotheses, its weighted mix with the
// CIDEr-D scores and the reward of the mixed scores, in one launch.
//
// vlp_cider_d_df takes df from a resident table (sorted uint64 keys, int32 df; vlp_amd/scst.py DocFreq) instead of the call's references.
// Both kernels are the ones above with TABLE = true: the counting pass drops its loop over the groups -- every (position, order) of the
// block's string gets a lane of its own that packs the n-gram's key and looks it up (a lower-bound binary search of dependent global loads:
// 256 independent searches per block overlap) -- and hands the scoring pass idf as a full-width fp32 next to the packed (tf, first), since
// table df does not fit cd_pack's 11 bits.
// Staging, cd_match, the table lookup and the operand checks are in reward_common.h, shared with caption_eval.hip (END = 1 here: the 0 is a token).
#include "reward_common.h"

// TABLE: df from `tab` (one lane per position and order: P is 64; tile_groups is unused, no dynamic LDS) and idf_out [mult*G][4][T] written
// for the hypotheses; otherwise df from the call's own references as described above (tab and idf_out unused).
template <bool TABLE>
__global__ __launch_bounds__(CD_THREADS) void cider_count_kernel(vlp_cider_d_args a, int P, int tile_groups, int* info, float* norms, cd_table tab,
                                                                 float* idf_out) {
    extern __shared__ __attribute__((aligned(16))) int cd_tile[];      // [tile_groups][R][T + CD_PAD]
    __shared__ int qrow[64 + CD_PAD], srow[64 + CD_PAD];               // the block's string with the query's / a reference's sentinel
    __shared__ int cnt[4][CD_THREADS];
    const int T = a.T, R = a.R, G = a.G, ldr = T + CD_PAD, SH = a.mult * G;
    const int s = blockIdx.x, tid = threadIdx.x;
    const int W = CD_THREADS / P, worker = tid / P, p = tid % P;
    const bool is_hyp = s < SH;
    const int64_t* src;
    if (is_hyp) {
        src = a.hyp + (int64_t)s * a.hyp_ld;
    } else {
        const int row = s - SH, g = row / R, r = row - g * R;
        if (r >= cd_ref_count(a.ref_count, g, R)) return;              // not a reference of its group: nobody reads its norms (block-uniform)
        src = a.ref + (int64_t)g * a.ref_group_stride + (int64_t)r * a.ref_ld;
    }
    if (tid < 64) {                                                    // wave 0: the block's own string
        const int tok = tid < T ? (int)src[tid] : CD_HYP_END;
        unsigned long long m = __ballot(tid < T && tok == 0);
        const int len = m ? (int)__builtin_ctzll(m) + 1 : T;
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
    int a0 = CD_HYP_END, a1 = CD_HYP_END, a2 = CD_HYP_END, a3 = CD_HYP_END;
    if (p < T) { a0 = qrow[p]; a1 = qrow[p + 1]; a2 = qrow[p + 2]; a3 = qrow[p + 3]; }

    if constexpr (TABLE) {
        // lane (order k = tid / 64, position tid % 64): the table df of the k+1-gram that starts there.  A sentinel (the string ends inside
        // the n-gram) or an id outside [0, 65535) forms no key: df 0
        const int k = worker, q = p;                                   // P is 64 here
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
    } else {
    // groups whose valid references hold the k-gram at p
    int c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    for (int g0 = 0; g0 < G; g0 += tile_groups) {
        const int ng = min(tile_groups, G - g0);
        __syncthreads();                                               // the previous tile has been read
        cd_stage_refs(a, g0 * R, ng * R, cd_tile, nullptr, P, CD_THREADS);
        __syncthreads();
        for (int gl = worker; gl < ng; gl += W) {
            const int nr = cd_ref_count(a.ref_count, g0 + gl, R);
            int best = 0;
            for (int r = 0; r < nr; ++r) {
                const int* row = cd_tile + (gl * R + r) * ldr;
                int b0 = row[0], b1 = row[1], b2 = row[2];
                for (int q = 0; q < T; ++q) {
                    const int b3 = row[q + 3];
                    best = max(best, cd_match(a0, a1, a2, a3, b0, b1, b2, b3));
                    b0 = b1; b1 = b2; b2 = b3;
                }
            }
            c1 += best >= 1; c2 += best >= 2; c3 += best >= 3; c4 += best >= 4;
        }
    }
    cnt[0][tid] = c1; cnt[1][tid] = c2; cnt[2][tid] = c3; cnt[3][tid] = c4;
    __syncthreads();
    }
    if (tid >= 64) return;

    // wave 0, lane = position: multiplicity and first occurrence inside the own string, then weights and norms
    int tf[4] = {0, 0, 0, 0}, first[4] = {1, 1, 1, 1}, groups[4] = {0, 0, 0, 0};
    if (tid < T) {
        int b0 = srow[0], b1 = srow[1], b2 = srow[2];
        for (int q = 0; q < T; ++q) {
            const int b3 = srow[q + 3];
            const int m = cd_match(a0, a1, a2, a3, b0, b1, b2, b3);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tf[k] += m > k;
                first[k] &= !(m > k && q < tid);
            }
            b0 = b1; b1 = b2; b2 = b3;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if constexpr (TABLE) groups[k] = cnt[k][tid];              // the table's df itself
            else
                for (int w = 0; w < W; ++w) groups[k] += cnt[k][w * P + tid];
        }
    }
    const float ref_len = logf(TABLE ? tab.n_docs : (float)SH);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float idf = ref_len - logf(fmaxf(1.f, (float)(TABLE ? groups[k] : a.mult * groups[k])));
        float v = 0.f;
        if (tid < T && tf[k] > 0 && first[k]) v = (float)tf[k] * idf;
        const float n2 = wave_sum(v * v);
        if (tid == 0) norms[(int64_t)s * 4 + k] = sqrtf(n2);
        if (is_hyp && tid < T) {
            info[((int64_t)s * 4 + k) * T + tid] = cd_pack(TABLE ? 0 : groups[k], tf[k], tf[k] > 0 && first[k]);
            if constexpr (TABLE) idf_out[((int64_t)s * 4 + k) * T + tid] = idf;
        }
    }
}

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

    const int tok = lane < T ? (int)a.hyp[(int64_t)h * a.hyp_ld + lane] : CD_HYP_END;
    const unsigned long long zm = __ballot(lane < T && tok == 0);
    const int len = zm ? (int)__builtin_ctzll(zm) + 1 : T;
    int av[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = __shfl(tok, (lane + j) & 63, 64);
        av[j] = lane + j < len ? t : CD_HYP_END;
    }
    __syncthreads();

    const float ref_len = logf((float)SH);                             // (unused with TABLE)
    float idf[4], hv[4], nh[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
    bool first[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int pk = lane < T ? info[((int64_t)h * 4 + k) * T + lane] : 0;
        if constexpr (TABLE) idf[k] = lane < T ? idf_in[((int64_t)h * 4 + k) * T + lane] : 0.f;
        else idf[k] = ref_len - logf(fmaxf(1.f, (float)(a.mult * (pk & 2047))));
        hv[k] = (float)((pk >> 11) & 127) * idf[k];
        first[k] = (pk >> 18) & 1;
        nh[k] = norms[(int64_t)h * 4 + k];
    }
    const int nr = cd_ref_count(a.ref_count, g, R);
    const float two_sigma2 = 2.f * a.sigma * a.sigma;
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
        const float delta = (float)(max(len - 1, 0) - max(ref_len_s[r] - 1, 0));
        const float penalty = expf(-(delta * delta) / two_sigma2);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float rv = (float)t[k] * idf[k];
            float val = wave_sum(first[k] ? fminf(hv[k], rv) * rv : 0.f);
            const float nrk = norms[((int64_t)SH + (int64_t)g * R + r) * 4 + k];
            if (nh[k] != 0.f && nrk != 0.f) val /= nh[k] * nrk;
            acc[k] += val * penalty;
        }
    }
    const float score = (acc[0] + acc[1] + acc[2] + acc[3]) / 4.f / (float)nr * 10.f;
    if (lane == 0) {
        a.scores[h] = score;
        sc[w] = score;
    }
    if (a.reward) {
        __syncthreads();
        if (loo) {                                                     // lane k: hypothesis k of the group against the others, ascending j
            const int k = threadIdx.x;
            if (k < a.mult) {
                float others = 0.f;
                for (int j = 0; j < a.mult; ++j)
                    if (j != k) others += sc[j];
                a.reward[(int64_t)k * G + g] = sc[k] - others / (float)(a.mult - 1);
            }
        } else if (threadIdx.x == 0) {                                 // mult == 2 (checked by the entry): sample - greedy
            a.reward[g] = sc[0] - sc[1];
        }
    }
}

static int cd_pow2_at_least(int T) {
    int P = 1;
    while (P < T) P <<= 1;
    return P;
}

extern "C" int64_t vlp_cider_d_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult) {
    return cd_shape_ok(G, R, T, mult) ? cd_workspace_bytes(G, R, T, mult, false) : 0;
}
extern "C" int64_t vlp_cider_d_multi_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult) {
    return cd_shape_ok(G, R, T, mult, true) ? cd_workspace_bytes(G, R, T, mult, false) : 0;
}

// the two launches of vlp_cider_d and vlp_cider_d_multi (`who` names the entry in messages; args checked by the caller)
static int cd_run(const vlp_cider_d_args* a, void* stream, bool multi, const char* who) {
    VLP_ENTER(a->ref, who);
    const int SH = a->mult * a->G, SR = a->G * a->R, ldr = a->T + CD_PAD;
    const int P = cd_pow2_at_least(a->T);
    int tile_groups = CD_TILE_INTS / (a->R * ldr);                     // >= 15 at the largest accepted R, T
    if (tile_groups > a->G) tile_groups = a->G;
    int* info = (int*)a->workspace;
    float* norms = (float*)(info + cd_info_ints(a->G, a->T, a->mult));
    hipLaunchKernelGGL(cider_count_kernel<false>, dim3(SH + SR), dim3(CD_THREADS), (size_t)tile_groups * a->R * ldr * sizeof(int), (hipStream_t)stream, *a, P,
                       tile_groups, info, norms, cd_table{}, (float*)nullptr);
    VLP_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(cider_score_kernel<false>, dim3(a->G), dim3(64 * a->mult), (size_t)a->R * ldr * sizeof(int), (hipStream_t)stream, *a, (const int*)info,
                       (const float*)norms, (const float*)nullptr, multi ? 1 : 0);
    VLP_CHECK_LAUNCH(who);
    return VLP_OK;
}

extern "C" int vlp_cider_d(const vlp_cider_d_args* a, void* stream) {
    VLP_CHECK_ARG(a, "vlp_cider_d: null args");
    const int64_t need = vlp_cider_d_workspace_bytes(a->G, a->R, a->T, a->mult);
    CD_CHECK_ARGS(a, "vlp_cider_d", need, false);
    return cd_run(a, stream, false, "vlp_cider_d");
}

extern "C" int vlp_cider_d_multi(const vlp_cider_d_args* a, void* stream) {
    VLP_CHECK_ARG(a, "vlp_cider_d_multi: null args");
    const int64_t need = vlp_cider_d_multi_workspace_bytes(a->G, a->R, a->T, a->mult);
    CD_CHECK_ARGS(a, "vlp_cider_d_multi", need, true);
    return cd_run(a, stream, true, "vlp_cider_d_multi");
}

// workspace: int32 info[mult*G][4][T] (tf, first), f32 idf[mult*G][4][T], then f32 norms[mult*G + G*R][4]
extern "C" int64_t vlp_cider_d_df_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult) {
    return cd_shape_ok(G, R, T, mult) ? cd_workspace_bytes(G, R, T, mult, true) : 0;
}
extern "C" int64_t vlp_cider_d_multi_df_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult) {
    return cd_shape_ok(G, R, T, mult, true) ? cd_workspace_bytes(G, R, T, mult, true) : 0;
}

static int cd_run_df(const vlp_cider_d_df_args* d, void* stream, bool multi, const char* who) {
    const vlp_cider_d_args* a = &d->s;
    VLP_ENTER(a->ref, who);
    const int SH = a->mult * a->G, SR = a->G * a->R, ldr = a->T + CD_PAD;
    int* info = (int*)a->workspace;
    float* idf = (float*)(info + cd_info_ints(a->G, a->T, a->mult));
    float* norms = idf + cd_info_ints(a->G, a->T, a->mult);
    const cd_table tab = {d->df_keys, d->df_vals, d->df_n, (float)d->n_docs};
    hipLaunchKernelGGL(cider_count_kernel<true>, dim3(SH + SR), dim3(CD_THREADS), 0, (hipStream_t)stream, *a, 64, 0, info, norms, tab, idf);
    VLP_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(cider_score_kernel<true>, dim3(a->G), dim3(64 * a->mult), (size_t)a->R * ldr * sizeof(int), (hipStream_t)stream, *a, (const int*)info,
                       (const float*)norms, (const float*)idf, multi ? 1 : 0);
    VLP_CHECK_LAUNCH(who);
    return VLP_OK;
}

extern "C" int vlp_cider_d_df(const vlp_cider_d_df_args* d, void* stream) {
    VLP_CHECK_ARG(d, "vlp_cider_d_df: null args");
    const vlp_cider_d_args* a = &d->s;
    const int64_t need = vlp_cider_d_df_workspace_bytes(a->G, a->R, a->T, a->mult);
    CD_CHECK_ARGS(a, "vlp_cider_d_df", need, false);
    CD_CHECK_TABLE(d, "vlp_cider_d_df");
    return cd_run_df(d, stream, false, "vlp_cider_d_df");
}

extern "C" int vlp_cider_d_multi_df(const vlp_cider_d_df_args* d, void* stream) {
    VLP_CHECK_ARG(d, "vlp_cider_d_multi_df: null args");
    const vlp_cider_d_args* a = &d->s;
    const int64_t need = vlp_cider_d_multi_df_workspace_bytes(a->G, a->R, a->T, a->mult);
    CD_CHECK_ARGS(a, "vlp_cider_d_multi_df", need, true);
    CD_CHECK_TABLE(d, "vlp_cider_d_multi_df");
    return cd_run_df(d, stream, true, "vlp_cider_d_multi_df");
}

// ------------------------------------------------------------------------------------------------------------------------------------------
// vlp_cider_d_consensus: the K samples of an image scored against each other (consensus selection: keep the sample that agrees most with the
// others).  The counting pass is cider_count_kernel<true> over the K*G sample rows alone -- a sample's norms in the reference role are its own
// --; the scoring block below is cider_score_kernel<true>'s with the references taken from the block's own rows: one block per image, one
// wave per sample, one lane per position.  Every wave stages its row once in LDS with the reference's sentinel and keeps it in registers with
// the hypothesis' sentinel (the two ends stay distinct: two string ends never match), then walks the other K - 1 rows in ascending j.
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

    const int tok = lane < T ? (int)a.hyp[(int64_t)h * a.hyp_ld + lane] : CD_HYP_END;
    const unsigned long long zm = __ballot(lane < T && tok == 0);
    const int len = zm ? (int)__builtin_ctzll(zm) + 1 : T;
    int av[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = __shfl(tok, (lane + j) & 63, 64);
        av[j] = lane + j < len ? t : CD_HYP_END;
    }
    rows[w][lane] = lane < len ? tok : CD_REF_END;
    if (lane < CD_PAD) rows[w][64 + lane] = CD_REF_END;
    if (lane == 0) len_s[w] = len;
    __syncthreads();

    float idf[4], hv[4], nh[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
    bool first[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int pk = lane < T ? info[((int64_t)h * 4 + k) * T + lane] : 0;
        idf[k] = lane < T ? idf_in[((int64_t)h * 4 + k) * T + lane] : 0.f;
        hv[k] = (float)((pk >> 11) & 127) * idf[k];
        first[k] = (pk >> 18) & 1;
        nh[k] = norms[(int64_t)h * 4 + k];
    }
    const float two_sigma2 = 2.f * a.sigma * a.sigma;
    for (int j = 0; j < K; ++j) {
        if (j == w) continue;                                          // (wave-uniform)
        const int* row = rows[j];
        int t[4] = {0, 0, 0, 0};
        int b0 = row[0], b1 = row[1], b2 = row[2];
        for (int q = 0; q < T; ++q) {
            const int b3 = row[q + 3];
            const int m = cd_match(av[0], av[1], av[2], av[3], b0, b1, b2, b3);
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] += m > k;
            b0 = b1; b1 = b2; b2 = b3;
        }
        const float delta = (float)(max(len - 1, 0) - max(len_s[j] - 1, 0));
        const float penalty = expf(-(delta * delta) / two_sigma2);
        float one[4];                                                  // this reference alone
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float rv = (float)t[k] * idf[k];
            float val = wave_sum(first[k] ? fminf(hv[k], rv) * rv : 0.f);
            const float nrk = norms[((int64_t)j * G + g) * 4 + k];
            if (nh[k] != 0.f && nrk != 0.f) val /= nh[k] * nrk;
            one[k] = val * penalty;
            acc[k] += val * penalty;
        }
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

// workspace: cider_count_kernel<true>'s for K*G hypotheses and no reference: int32 info[K*G][4][T], f32 idf[K*G][4][T], f32 norms[K*G][4]
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
    VLP_CHECK_ARG(c->sigma > 0.f, "vlp_cider_d_consensus: sigma must be positive");
    const int64_t need = vlp_cider_d_consensus_workspace_bytes(c->G, c->K, c->T);
    VLP_CHECK_ARG(c->workspace_bytes >= need && (uintptr_t)c->workspace % 16 == 0, "vlp_cider_d_consensus: workspace of %lld bytes, needs %lld (16-byte aligned)",
                  (long long)c->workspace_bytes, (long long)need);
    CD_CHECK_TABLE(c, "vlp_cider_d_consensus");
    VLP_ENTER(c->hyp, "vlp_cider_d_consensus");
    vlp_cider_d_args a = {};                                           // the counting pass sees K*G hypotheses and no reference block
    a.hyp = c->hyp; a.hyp_ld = c->hyp_ld;
    a.G = c->G; a.R = 1; a.T = c->T; a.mult = c->K;
    const int SH = c->K * c->G;
    int* info = (int*)c->workspace;
    float* idf = (float*)(info + cd_info_ints(c->G, c->T, c->K));
    float* norms = idf + cd_info_ints(c->G, c->T, c->K);
    const cd_table tab = {c->df_keys, c->df_vals, c->df_n, (float)c->n_docs};
    hipLaunchKernelGGL(cider_count_kernel<true>, dim3(SH), dim3(CD_THREADS), 0, (hipStream_t)stream, a, 64, 0, info, norms, tab, idf);
    VLP_CHECK_LAUNCH("vlp_cider_d_consensus");
    hipLaunchKernelGGL(consensus_score_kernel, dim3(c->G), dim3(64 * c->K), 0, (hipStream_t)stream, *c, (const int*)info, (const float*)norms, (const float*)idf);
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

    const int tok = lane < T ? (int)a.hyp[(int64_t)h * a.hyp_ld + lane] : CD_HYP_END;
    const unsigned long long zm = __ballot(lane < T && tok == 0);
    const int len = zm ? (int)__builtin_ctzll(zm) + 1 : T;
    int av[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = __shfl(tok, (lane + j) & 63, 64);
        av[j] = lane + j < len ? t : CD_HYP_END;
    }
    hrow[w][lane] = lane < len ? tok : CD_REF_END;
    if (lane < CD_PAD) hrow[w][64 + lane] = CD_REF_END;
    __syncthreads();

    // multiplicity and first occurrence of the k-gram at this lane inside the own string
    int tf[4] = {0, 0, 0, 0}, first[4] = {1, 1, 1, 1}, best[4] = {0, 0, 0, 0};
    {
        const int* row = hrow[w];
        int b0 = row[0], b1 = row[1], b2 = row[2];
        for (int q = 0; q < T; ++q) {
            const int b3 = row[q + 3];
            const int m = cd_match(av[0], av[1], av[2], av[3], b0, b1, b2, b3);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                tf[k] += m > k;
                first[k] &= !(m > k && q < lane);
            }
            b0 = b1; b1 = b2; b2 = b3;
        }
    }
    // its count in every valid reference: the maximum; the closest reference length, the shorter on a tie
    const int nr = cd_ref_count(a.ref_count, g, R);
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
#pragma unroll
        for (int k = 0; k < 4; ++k) best[k] = max(best[k], t[k]);
        const int lr = ref_len_s[r], d = abs(lr - len);
        if (d < refdist || (d == refdist && lr < reflen)) { refdist = d; reflen = lr; }
    }
    int correct[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) correct[k] = wave_sum_int((tf[k] > 0 && first[k]) ? min(tf[k], best[k]) : 0);

    if (lane == 0) {
        float p = 1.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) p = p * (((float)correct[k] + 1e-15f) / ((float)max(0, len - k) + 1e-9f));
        float b = powf(p, 0.25f);
        if (len < reflen) b *= expf((float)(len - reflen) / (float)len);       // exp(1 - reflen / len_h)
        o.bleu4[h] = b;
        if (o.stats) {
            int32_t* st = o.stats + (int64_t)h * 6;
            st[0] = correct[0]; st[1] = correct[1]; st[2] = correct[2]; st[3] = correct[3]; st[4] = len; st[5] = reflen;
        }
        if (o.mixed) {
            const float m = o.base ? mix_unfused(o.w_base, o.base[h], o.w_bleu, b) : o.w_bleu * b;
            o.mixed[h] = m;
            sc[w] = m;
        }
    }
    if (o.reward) {                                                    // (the entry checked that mixed is there)
        __syncthreads();
        if (o.loo) {                                                   // thread k: hypothesis k of the group against the others, ascending j
            const int k = threadIdx.x;
            if (k < a.mult) {
                float others = 0.f;
                for (int j = 0; j < a.mult; ++j)
                    if (j != k) others += sc[j];
                o.reward[(int64_t)k * G + g] = sc[k] - others / (float)(a.mult - 1);
            }
        } else if (threadIdx.x == 0) {                                 // mult == 2 (checked by the entry)
            o.reward[g] = sc[0] - sc[1];
        }
    }
}

extern "C" int vlp_bleu4(const vlp_bleu4_args* b, void* stream) {
    VLP_CHECK_ARG(b, "vlp_bleu4: null args");
    VLP_CHECK_ARG(b->T >= 1 && b->T <= 64 && b->R >= 1 && b->R <= 8 && b->G >= 1 && b->G <= 1024 && b->mult >= 1 && b->mult <= CD_MAX_MULT,
                  "vlp_bleu4: needs 1 <= T <= 64, 1 <= R <= 8, 1 <= G <= 1024, 1 <= mult <= 16 (G %d, R %d, T %d, mult %d)", b->G, b->R, b->T, b->mult);
    VLP_CHECK_ARG(b->hyp && b->ref && b->bleu4, "vlp_bleu4: null operand");
    VLP_CHECK_ARG(b->hyp_ld >= b->T && b->ref_ld >= b->T && b->ref_group_stride >= (int64_t)(b->R - 1) * b->ref_ld + b->T,
                  "vlp_bleu4: strides shorter than the rows");
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
