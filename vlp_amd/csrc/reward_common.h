// The pieces the n-gram scoring kernels of reward.hip (SCST reward: CIDEr-D, consensus, BLEU-4) and caption_eval.hip (caption metrics) are
// composed of, each written once: loading and staging id strings in sentinel form, the match length of two n-gram positions and the two walks
// built on it, the document-frequency table lookup, the CIDEr-D terms of one reference, the BLEU bookkeeping, the baseline of a group's scores,
// and the counting kernel both files launch.  State passes through plain arrays of four (one element per n-gram order).
//
// The two files read a padded row differently, and the difference is a template argument, never a run-time branch:
//   END = 1   the reward's string: the ids up to AND INCLUDING the first 0 (array_to_str's: [SEP] and the 0 are tokens);
//   END = 0   a word string: the ids BEFORE the first 0 -- the 0 is padding, an empty string is legal.
// Either way a row without a 0 is all its T ids.
#pragma once
#include "common.h"

#define CD_THREADS 256
#define CD_PAD 3                 // sentinel columns behind every staged row
#define CD_HYP_END (-1)
#define CD_REF_END (-2)
#define CD_TILE_INTS 8192        // LDS budget of one reference tile (32 KiB)

// (df groups, tf, first occurrence) of one (position, order): groups <= 1024, tf <= 64
DEVFN int cd_pack(int groups, int tf, int first) { return groups | (tf << 11) | (first << 18); }

DEVFN int cd_match(int a0, int a1, int a2, int a3, int b0, int b1, int b2, int b3) {
    return a0 == b0 ? (a1 == b1 ? (a2 == b2 ? (a3 == b3 ? 4 : 3) : 2) : 1) : 0;
}

// The string length of a row from the ballot of its zeros (bit p = id p is 0, only bits below T set): see END above.
template <int END = 1>
DEVFN int cd_len_of(unsigned long long zeros, int T) {
    return zeros ? (int)__builtin_ctzll(zeros) + END : T;
}

// The P lanes of a segment hold one row (lane p its id p, p < T): the row's string length.
template <int END = 1>
DEVFN int cd_row_len(bool is_zero, int seg, int P, int T) {
    unsigned long long m = __ballot(is_zero);
    m >>= seg * P;                                   // seg * P <= 63
    if (P < 64) m &= (1ull << P) - 1ull;
    return cd_len_of<END>(m, T);
}

// df of one n-gram in the table: lower bound of `key` in keys[0, n) (ascending as unsigned), at most ceil(log2(n + 1)) probes -- the key at
// the final bound is the last one probed there, so the equality test costs no further probe.  Plain per-lane vector loads; read only.
struct cd_table {
    const uint64_t* keys;
    const int32_t* vals;
    int64_t n;
    float n_docs;                                    // exact: n_docs <= 2^24
};

DEVFN int cd_table_df(const cd_table& t, uint64_t key) {
    int64_t lo = 0, hi = t.n;
    uint64_t at_hi = 0;                              // keys[hi] once hi < n (key 0 never occurs)
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);   // lo <= mid < hi <= n
        const uint64_t v = t.keys[mid];
        if (v < key) lo = mid + 1;
        else { hi = mid; at_hi = v; }
    }
    return at_hi == key ? t.vals[hi] : 0;
}

DEVFN int cd_ref_count(const int32_t* ref_count, int g, int R) {
    if (!ref_count) return R;
    const int c = ref_count[g];
    return c < 1 ? 1 : (c > R ? R : c);
}

// Stage `rows` reference rows, starting at reference row row0 of the whole [G*R] list, into dst[rows][T + CD_PAD] (sentinel form).  Every
// lane of the block calls this (the ballot needs whole waves); a row past its group's ref_count is all sentinels.  len_out (or NULL) gets
// each row's length, 0 for an invalid row.
template <int END = 1>
DEVFN void cd_stage_refs(const vlp_cider_d_args& a, int row0, int rows, int* dst, int* len_out, int P, int nthreads) {
    const int T = a.T, R = a.R, ldr = T + CD_PAD;
    const int W = nthreads / P, worker = threadIdx.x / P, p = threadIdx.x % P, seg = (threadIdx.x & 63) / P;
    for (int i0 = 0; i0 < rows; i0 += W) {
        const int i = i0 + worker;
        const bool live = i < rows && p < T;
        int tok = CD_REF_END;
        bool valid = false;
        if (i < rows) {
            const int row = row0 + i, g = row / R, r = row - g * R;
            valid = r < cd_ref_count(a.ref_count, g, R);
            if (live && valid) tok = (int)a.ref[(int64_t)g * a.ref_group_stride + (int64_t)r * a.ref_ld + p];
        }
        const int len = cd_row_len<END>(live && valid && tok == 0, seg, P, T);
        if (live) dst[i * ldr + p] = (valid && p < len) ? tok : CD_REF_END;
        if (i < rows && p < CD_PAD) dst[i * ldr + T + p] = CD_REF_END;
        if (len_out && i < rows && p == 0) len_out[i] = valid ? len : 0;
    }
}

DEVFN int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- a string in a wave: lane p holds id p -------------------------------------------------------------------------------------------------
// Lane p < T reads id p of `row` into tok (CD_HYP_END on the other lanes); returns the row's string length.  Whole waves call this.
template <int END>
DEVFN int cd_load_row(const int64_t* row, int T, int lane, int& tok) {
    tok = lane < T ? (int)row[lane] : CD_HYP_END;
    return cd_len_of<END>(__ballot(lane < T && tok == 0), T);
}

// A hypothesis in registers: cd_load_row, and av[j] = id lane + j of the string, the query's sentinel from the string's end on.
template <int END>
DEVFN int cd_load_hyp(const int64_t* row, int T, int lane, int& tok, int av[4]) {
    const int len = cd_load_row<END>(row, T, lane, tok);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int t = __shfl(tok, (lane + j) & 63, 64);
        av[j] = lane + j < len ? t : CD_HYP_END;
    }
    return len;
}

// The wave's own string (cd_load_hyp's tok and len) as a reference row dst[64 + CD_PAD] in LDS: a reference's sentinel from its end on.
DEVFN void cd_stage_wave_row(int* dst, int tok, int len, int lane) {
    dst[lane] = lane < len ? tok : CD_REF_END;
    if (lane < CD_PAD) dst[64 + lane] = CD_REF_END;
}

// Wave 0 of a counting block stages the block's string twice, [T + CD_PAD] each: qrow with the query's sentinel, srow with a reference's.
template <int END>
DEVFN void cd_stage_own(const int64_t* src, int T, int* qrow, int* srow) {
    const int lane = threadIdx.x;
    int tok;
    const int len = cd_load_row<END>(src, T, lane, tok);
    if (lane < T) {
        qrow[lane] = lane < len ? tok : CD_HYP_END;
        srow[lane] = lane < len ? tok : CD_REF_END;
    }
    if (lane < CD_PAD) {
        qrow[T + lane] = CD_HYP_END;
        srow[T + lane] = CD_REF_END;
    }
}

// ---- the walks: the n-grams that start at a lane's position (av) against every position of one staged row -----------------------------------
// Both count in locals and copy out at the end: with the loop counting in the caller's arrays hipcc unrolled it 16-fold and kept the
// partial sums in ~80 more VGPRs (126 instead of 47: occupancy 4 instead of 8 in every scoring kernel).
// t[k] = the number of positions of row[T + CD_PAD] whose k+1-gram equals the lane's
DEVFN void cd_count_row(const int av[4], const int* row, int T, int t[4]) {
    const int a0 = av[0], a1 = av[1], a2 = av[2], a3 = av[3];
    int c[4] = {0, 0, 0, 0};
    int b0 = row[0], b1 = row[1], b2 = row[2];
    for (int q = 0; q < T; ++q) {
        const int b3 = row[q + 3];
        const int m = cd_match(a0, a1, a2, a3, b0, b1, b2, b3);
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] += m > k;
        b0 = b1; b1 = b2; b2 = b3;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = c[k];
}

// The same walk over the lane's own string (with a reference's sentinel): tf[k] = the k+1-gram's multiplicity there, first[k] = no position
// before `lane` holds it.
DEVFN void cd_count_own(const int av[4], const int* row, int T, int lane, int tf[4], int first[4]) {
    const int a0 = av[0], a1 = av[1], a2 = av[2], a3 = av[3];
    int c[4] = {0, 0, 0, 0}, f[4] = {1, 1, 1, 1};
    int b0 = row[0], b1 = row[1], b2 = row[2];
    for (int q = 0; q < T; ++q) {
        const int b3 = row[q + 3];
        const int m = cd_match(a0, a1, a2, a3, b0, b1, b2, b3);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[k] += m > k;
            f[k] &= !(m > k && q < lane);
        }
        b0 = b1; b1 = b2; b2 = b3;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { tf[k] = c[k]; first[k] = f[k]; }
}

// The table df of the k+1-gram that starts at position q of qrow (query's sentinel).  A sentinel (the string ends inside the n-gram) or an id
// outside [0, 65535) forms no key: df 0
DEVFN int cd_key_df(const int* qrow, int q, int k, const cd_table& tab) {
    uint64_t key = 0;
    bool ok = true;
    for (int j = 0; j <= k; ++j) {
        const int t = qrow[q + j];
        ok = ok && t >= 0 && t < 65535;
        key |= (uint64_t)(((unsigned)t + 1u) & 0xffffu) << (48 - 16 * j);   // (used only when every id is in range)
    }
    return ok ? cd_table_df(tab, key) : 0;
}

// ---- CIDEr-D ------------------------------------------------------------------------------------------------------------------------------
// What the counting pass left for hypothesis h, at this lane's position and per order: idf (TABLE: read from idf_in; else from the packed
// group count, SH = mult * G strings), tf, hv = tf * idf, first (the first occurrence of an n-gram the string holds), and the norms nh.
template <bool TABLE>
DEVFN void cd_load_weights(const int* info, const float* idf_in, const float* norms, int h, int T, int lane, int mult, int SH, float idf[4], int tf[4],
                           float hv[4], int first[4], float nh[4]) {
    const float ref_len = logf((float)SH);                             // (unused with TABLE)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int pk = lane < T ? info[((int64_t)h * 4 + k) * T + lane] : 0;
        if constexpr (TABLE) idf[k] = lane < T ? idf_in[((int64_t)h * 4 + k) * T + lane] : 0.f;
        else idf[k] = ref_len - logf(fmaxf(1.f, (float)(mult * (pk & 2047))));
        tf[k] = (pk >> 11) & 127;
        hv[k] = (float)tf[k] * idf[k];
        first[k] = (pk >> 18) & 1;
        nh[k] = norms[(int64_t)h * 4 + k];
    }
}

// The terms of one reference (its counts t, its four norms nr, its length): Gaussian length penalty, per order the clipped product summed over
// the wave and divided by the two norms, accumulated into acc; `one` (or NULL) gets this reference's terms alone.
DEVFN void cd_cider_terms(const int t[4], const float idf[4], const float hv[4], const int first[4], const float nh[4], const float* nr, int len,
                          int len_ref, float two_sigma2, float acc[4], float* one) {
    const float delta = (float)(max(len - 1, 0) - max(len_ref - 1, 0));
    const float penalty = expf(-(delta * delta) / two_sigma2);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float rv = (float)t[k] * idf[k];
        float val = wave_sum(first[k] ? fminf(hv[k], rv) * rv : 0.f);
        const float nrk = nr[k];
        if (nh[k] != 0.f && nrk != 0.f) val /= nh[k] * nrk;
        if (one) one[k] = val * penalty;
        acc[k] += val * penalty;
    }
}

// ---- BLEU ---------------------------------------------------------------------------------------------------------------------------------
// One more reference (counts t, length lr) for a hypothesis of length len: the largest count per order; the closest reference length, the
// shorter on a tie (reflen 0, refdist 1 << 30 before the first)
DEVFN void cd_bleu_update(const int t[4], int lr, int len, int best[4], int& reflen, int& refdist) {
#pragma unroll
    for (int k = 0; k < 4; ++k) best[k] = max(best[k], t[k]);
    const int d = abs(lr - len);
    if (d < refdist || (d == refdist && lr < reflen)) { refdist = d; reflen = lr; }
}

// correct_k: the first occurrence of every distinct n-gram contributes min(tf, best), summed over the wave
DEVFN void cd_bleu_correct(const int tf[4], const int first[4], const int best[4], int correct[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) correct[k] = wave_sum_int((tf[k] > 0 && first[k]) ? min(tf[k], best[k]) : 0);
}

DEVFN void cd_bleu_stats(int32_t* st, const int correct[4], int len, int reflen) {
    st[0] = correct[0]; st[1] = correct[1]; st[2] = correct[2]; st[3] = correct[3]; st[4] = len; st[5] = reflen;
}

// ---- the baseline of a group's scores sc[mult] (LDS, written by the waves' lanes 0); the whole block calls this -------------------------------
// loo: reward [mult*G], each score minus the mean of the group's others, summed in ascending j; else reward [G] = sc[0] - sc[1] (mult == 2,
// checked by the entry: sample - greedy)
DEVFN void cd_baseline(const float* sc, int mult, int G, int g, int loo, float* reward) {
    __syncthreads();
    if (loo) {
        const int k = threadIdx.x;
        if (k < mult) {
            float others = 0.f;
            for (int j = 0; j < mult; ++j)
                if (j != k) others += sc[j];
            reward[(int64_t)k * G + g] = sc[k] - others / (float)(mult - 1);
        }
    } else if (threadIdx.x == 0) {
        reward[g] = sc[0] - sc[1];
    }
}

// ---- the counting kernel ------------------------------------------------------------------------------------------------------------------
// One block per string (the mult*G hypotheses, then the G*R references).  Per position and order: df, the n-gram's multiplicity in its own
// string (tf) and whether it is the first occurrence there; from them the string's four L2 norms, and for a hypothesis (df, tf, first) per
// position for the scoring pass.
// TABLE: df from `tab` -- lane (order tid / 64, position tid % 64) packs the n-gram's key and looks it up; P is 64, tile_groups is unused, no
// dynamic LDS -- and idf_out [mult*G][4][T] is written for the hypotheses, since table df does not fit cd_pack's 11 bits.  Otherwise df = the
// groups whose valid references hold the n-gram: a worker = P consecutive lanes (P = the power of two >= T), one lane per position of the block's
// string; the 256 / P workers share the groups of a tile of references staged in LDS (tab and idf_out unused).
template <bool TABLE, int END>
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
    if (tid < 64) cd_stage_own<END>(src, T, qrow, srow);
    __syncthreads();
    int av[4] = {CD_HYP_END, CD_HYP_END, CD_HYP_END, CD_HYP_END};
    if (p < T) { av[0] = qrow[p]; av[1] = qrow[p + 1]; av[2] = qrow[p + 2]; av[3] = qrow[p + 3]; }

    if constexpr (TABLE) {
        cnt[worker][p] = p < T ? cd_key_df(qrow, p, worker, tab) : 0;  // P is 64 here: order `worker`, position p
        __syncthreads();
    } else {
        // groups whose valid references hold the k-gram at p: the best match over a group's rows
        int c[4] = {0, 0, 0, 0};
        for (int g0 = 0; g0 < G; g0 += tile_groups) {
            const int ng = min(tile_groups, G - g0);
            __syncthreads();                                           // the previous tile has been read
            cd_stage_refs<END>(a, g0 * R, ng * R, cd_tile, nullptr, P, CD_THREADS);
            __syncthreads();
            for (int gl = worker; gl < ng; gl += W) {
                const int nr = cd_ref_count(a.ref_count, g0 + gl, R);
                int best = 0;
                for (int r = 0; r < nr; ++r) {
                    const int* row = cd_tile + (gl * R + r) * ldr;
                    int b0 = row[0], b1 = row[1], b2 = row[2];
                    for (int q = 0; q < T; ++q) {
                        const int b3 = row[q + 3];
                        best = max(best, cd_match(av[0], av[1], av[2], av[3], b0, b1, b2, b3));
                        b0 = b1; b1 = b2; b2 = b3;
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) c[k] += best > k;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k][tid] = c[k];
        __syncthreads();
    }
    if (tid >= 64) return;

    // wave 0, lane = position: multiplicity and first occurrence inside the own string, then weights and norms
    int tf[4] = {0, 0, 0, 0}, first[4] = {1, 1, 1, 1}, groups[4] = {0, 0, 0, 0};
    if (tid < T) {
        cd_count_own(av, srow, T, tid, tf, first);
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

// ---- host side: shapes, workspace layout and the operand checks the entry points share --------------------------------------------------
#define CD_MAX_MULT 16

// multi: the vlp_cider_d_multi* entries (2..CD_MAX_MULT hypotheses per group), else vlp_cider_d / vlp_cider_d_df (1 or 2)
static inline bool cd_shape_ok(int32_t G, int32_t R, int32_t T, int32_t mult, bool multi = false) {
    return T >= 1 && T <= 64 && R >= 1 && R <= 8 && G >= 1 && G <= 1024 && (multi ? (mult >= 2 && mult <= CD_MAX_MULT) : (mult == 1 || mult == 2));
}
// workspace: int32 info[mult*G][4][T] (df groups, tf, first per hypothesis position and order), then f32 norms[mult*G + G*R][4]; with a table
// f32 idf[mult*G][4][T] between the two
static inline int64_t cd_info_ints(int32_t G, int32_t T, int32_t mult) { return (int64_t)mult * G * 4 * T; }

static inline int64_t cd_workspace_bytes(int32_t G, int32_t R, int32_t T, int32_t mult, bool table) {
    const int64_t bytes = 4 * ((table ? 2 : 1) * cd_info_ints(G, T, mult) + 4 * ((int64_t)mult * G + (int64_t)G * R));
    return (bytes + 255) / 256 * 256;
}

// the workspace carved: info, idf (NULL without a table), norms
struct cd_workspace {
    int* info;
    float* idf;
    float* norms;
};
static inline cd_workspace cd_carve(void* workspace, int32_t G, int32_t T, int32_t mult, bool table) {
    int* info = (int*)workspace;
    const int64_t n = cd_info_ints(G, T, mult);
    return {info, table ? (float*)(info + n) : nullptr, (float*)(info + (table ? 2 : 1) * n)};
}

// the table of an argument struct that carries (df_keys, df_vals, df_n, n_docs)
template <class D>
static inline cd_table cd_table_of(const D* d) { return {d->df_keys, d->df_vals, d->df_n, (float)d->n_docs}; }

// The counting launch with a table, over the first `strings` strings of `a` (its mult*G hypotheses, then its G*R references), into the
// carved workspace.  The caller checks the launch.
template <int END>
static inline void cd_launch_count_table(const vlp_cider_d_args& a, int strings, const cd_workspace& ws, const cd_table& tab, void* stream) {
    hipLaunchKernelGGL((cider_count_kernel<true, END>), dim3(strings), dim3(CD_THREADS), 0, (hipStream_t)stream, a, 64, 0, ws.info, ws.norms, tab, ws.idf);
}

// The checks of an argument struct `a` (any that has the fields named), one condition each; `who` names the entry in the message.
#define CD_CHECK_STRIDES(a, who)                                                                                                                 \
    VLP_CHECK_ARG((a)->hyp_ld >= (a)->T && (a)->ref_ld >= (a)->T && (a)->ref_group_stride >= (int64_t)((a)->R - 1) * (a)->ref_ld + (a)->T,       \
                  who ": strides shorter than the rows")
#define CD_CHECK_SIGMA(a, who) VLP_CHECK_ARG((a)->sigma > 0.f, who ": sigma must be positive")
#define CD_CHECK_WORKSPACE(a, who, need)                                                                                                         \
    VLP_CHECK_ARG((a)->workspace_bytes >= (need) && (uintptr_t)(a)->workspace % 16 == 0, who ": workspace of %lld bytes, needs %lld (16-byte aligned)", \
                  (long long)(a)->workspace_bytes, (long long)(need))

// `need` is the entry's own workspace size, `multi` as in cd_shape_ok
#define CD_CHECK_ARGS(a, who, need, multi)                                                                                                       \
    VLP_CHECK_ARG(cd_shape_ok((a)->G, (a)->R, (a)->T, (a)->mult, multi), who ": needs 1 <= T <= 64, 1 <= R <= 8, 1 <= G <= 1024, mult %s (G %d, R %d, T %d, mult %d)", \
                  (multi) ? "in 2..16" : "1 or 2", (a)->G, (a)->R, (a)->T, (a)->mult);                                                          \
    VLP_CHECK_ARG((a)->hyp && (a)->ref && (a)->scores && (a)->workspace, who ": null operand");                                                  \
    VLP_CHECK_ARG((multi) || !(a)->reward || (a)->mult == 2, who ": reward = scores[g] - scores[G + g] needs mult == 2");                        \
    CD_CHECK_STRIDES(a, who);                                                                                                                    \
    CD_CHECK_SIGMA(a, who);                                                                                                                      \
    CD_CHECK_WORKSPACE(a, who, need)

#define CD_CHECK_TABLE(d, who)                                                                                                                   \
    VLP_CHECK_ARG((d)->df_n >= 0 && (d)->n_docs >= 1 && (d)->n_docs <= (1 << 24), who ": needs df_n >= 0 and 1 <= n_docs <= 2^24 (df_n %lld, n_docs %lld)", \
                  (long long)(d)->df_n, (long long)(d)->n_docs);                                                                                 \
    VLP_CHECK_ARG((d)->df_n == 0 || ((d)->df_keys && (d)->df_vals && (uintptr_t)(d)->df_keys % 8 == 0 && (uintptr_t)(d)->df_vals % 4 == 0),      \
                  who ": a table of %lld keys needs non-null df_keys (8-byte aligned) and df_vals (4-byte aligned)", (long long)(d)->df_n)
