// Device helpers shared by the n-gram scoring kernels of reward.hip (SCST reward: CIDEr-D, BLEU-4) and caption_eval.hip (caption metrics):
// staging of id strings in sentinel form, the match length of two n-gram positions, the document-frequency table lookup.
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

// `need` is the entry's own workspace size, `multi` as in cd_shape_ok
#define CD_CHECK_ARGS(a, who, need, multi)                                                                                                       \
    VLP_CHECK_ARG(cd_shape_ok((a)->G, (a)->R, (a)->T, (a)->mult, multi), who ": needs 1 <= T <= 64, 1 <= R <= 8, 1 <= G <= 1024, mult %s (G %d, R %d, T %d, mult %d)", \
                  (multi) ? "in 2..16" : "1 or 2", (a)->G, (a)->R, (a)->T, (a)->mult);                                                          \
    VLP_CHECK_ARG((a)->hyp && (a)->ref && (a)->scores && (a)->workspace, who ": null operand");                                                  \
    VLP_CHECK_ARG((multi) || !(a)->reward || (a)->mult == 2, who ": reward = scores[g] - scores[G + g] needs mult == 2");                        \
    VLP_CHECK_ARG((a)->hyp_ld >= (a)->T && (a)->ref_ld >= (a)->T && (a)->ref_group_stride >= (int64_t)((a)->R - 1) * (a)->ref_ld + (a)->T,       \
                  who ": strides shorter than the rows");                                                                                        \
    VLP_CHECK_ARG((a)->sigma > 0.f, who ": sigma must be positive");                                                                             \
    VLP_CHECK_ARG((a)->workspace_bytes >= (need) && (uintptr_t)(a)->workspace % 16 == 0, who ": workspace of %lld bytes, needs %lld (16-byte aligned)", \
                  (long long)(a)->workspace_bytes, (long long)(need))

#define CD_CHECK_TABLE(d, who)                                                                                                                   \
    VLP_CHECK_ARG((d)->df_n >= 0 && (d)->n_docs >= 1 && (d)->n_docs <= (1 << 24), who ": needs df_n >= 0 and 1 <= n_docs <= 2^24 (df_n %lld, n_docs %lld)", \
                  (long long)(d)->df_n, (long long)(d)->n_docs);                                                                                 \
    VLP_CHECK_ARG((d)->df_n == 0 || ((d)->df_keys && (d)->df_vals && (uintptr_t)(d)->df_keys % 8 == 0 && (uintptr_t)(d)->df_vals % 4 == 0),      \
                  who ": a table of %lld keys needs non-null df_keys (8-byte aligned) and df_vals (4-byte aligned)", (long long)(d)->df_n)
