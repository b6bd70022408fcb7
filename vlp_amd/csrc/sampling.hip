// Temperature / top-k / top-p sampling of vocabulary rows (include/vlp_hip.h: vlp_sample_rows_filtered).
//
// The kept set of a row is a pure value threshold, S = {v : l_v >= cutoff}, and an fp16 logit has 65 536 values: both thresholds are found
// by a radix select on the 16-bit order-preserving key of the logit (two 256-bin histogram rounds, high byte then low byte), counts for
// top-k and probability mass for top-p.  Nothing is sorted.  Passes over the row (each skipped when its control is off):
//   A  row maximum and minimum, count histogram of the high key byte                       (histogram: top-k only)
//   B  count histogram of the low key byte inside the selected high byte   -> tau_k        (top-k only)
//   C  mass histogram of the high key byte over l >= tau_k                                 (top-p only)
//   D  mass histogram of the low key byte inside the selected high byte    -> tau_p        (top-p only)
//   E  sample_row_body's second loop (sum of exp, Gumbel arg-max on the same hash) over l >= cutoff, plus |S|
// Every result is independent of the order in which threads run: counts and masses are integers (mass = exp(z - z_max) in units of 2^-40,
// accumulated in 64 bits), added with LDS atomics; the bins are scanned with a fixed 256-thread suffix scan; the sum of exp behind logp
// goes through block_reduce_sum.  A repeated launch returns the same bits.
#include "vocab_row.h"

#include <cmath>

struct SampleFilterArgs {
    const f16* logits;
    int64_t ld;
    int V, rep;
    const uint64_t* seed_cell;
    uint64_t seed_add;
    uint32_t rng_stream;
    float T;
    int top_k;                // 0: top-k off (the launcher has folded top_k >= V into 0)
    float top_p;              // 1: top-p off
    int64_t* ids; int64_t ids_stride;
    int64_t* ids2; int64_t ids2_stride;
    float* logp; int64_t logp_stride;
    float* cutoff;
    int32_t* kept;
};

// 16-bit key of an fp16 value: a < b as numbers <=> key(a) < key(b) as integers (-0 takes +0's key: they are one value)
DEVFN uint32_t f16_key(float f) {
    uint32_t b = __builtin_bit_cast(uint16_t, (f16)f);       // (f came from an fp16: the conversion back is exact)
    if (b == 0x8000u) b = 0u;
    return (b & 0x8000u) ? (~b & 0xffffu) : (b | 0x8000u);
}
DEVFN float key_value(uint32_t k) {
    const uint16_t b = (uint16_t)((k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xffffu));
    return (float)__builtin_bit_cast(f16, b);
}

// probability mass as an integer: exp(z - z_max) <= 1 in units of 2^-40.  A float above 2^-16 converts exactly, a smaller one loses less than 2^-40
// of the row maximum's mass; V <= 2^22 columns sum to less than 2^63.
#define VLP_FILTER_MAX_TOP_P_COLS (1 << 22)
DEVFN unsigned long long mass_units(float e) { return (unsigned long long)(e * 1099511627776.0f); }

// h[t] <- h[t] + h[t + 1] + ... + h[255] for the 256 threads of the block (h complete and visible on entry, visible again on return)
template <typename N>
DEVFN void suffix_scan256(N* h) {
    const int tid = threadIdx.x;
    N v = h[tid];
#pragma unroll
    for (int o = 1; o < 256; o <<= 1) {
        const N a = tid + o < 256 ? h[tid + o] : (N)0;
        __syncthreads();
        v += a;
        h[tid] = v;
        __syncthreads();
    }
}
// the largest bin t whose suffix sum reaches `target` (1 <= target <= h[0]); *rem = what bin t itself has to supply.  Every thread returns the bin.
template <typename N>
DEVFN int pick_bin256(const N* h, N target, int* sel, N* rem) {
    const int tid = threadIdx.x;
    const N above = tid < 255 ? h[tid + 1] : (N)0;
    if (h[tid] >= target && above < target) { *sel = tid; *rem = target - above; }
    __syncthreads();
    return *sel;
}

template <bool VEC>
__global__ __launch_bounds__(256) void sample_rows_filtered_kernel(SampleFilterArgs a) {
    __shared__ uint32_t hc[256];
    __shared__ unsigned long long hm[256];
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ float red[4];
    __shared__ int sel;
    __shared__ uint32_t rem_c;
    __shared__ unsigned long long rem_m;
    __shared__ int n_kept;
    const int tid = threadIdx.x;
    const int row = blockIdx.x;
    const int V = a.V;
    const f16* x = a.logits + (int64_t)(row / a.rep) * a.ld;
    const float T = a.T;
    const bool use_k = a.top_k > 0, use_p = a.top_p < 1.f;

    hc[tid] = 0u;
    if (tid == 0) { sel = 0; rem_c = 1u; rem_m = 1ull; n_kept = 0; }
    __syncthreads();
    // A
    float mx = -INFINITY, mn = INFINITY;
    if (use_k) {
        row_visit<256, VEC>(x, 0, V, [&](float f, int) {
            mx = fmaxf(mx, f);
            atomicAdd(&hc[f16_key(f) >> 8], 1u);
        });
    } else {
        row_visit<256, VEC>(x, 0, V, [&](float f, int) {
            mx = fmaxf(mx, f);
            mn = fminf(mn, f);
        });
    }
    mx = block_reduce_max<256>(mx, red);
    uint32_t tk_key = 0u, cut_key;
    if (use_k) {
        suffix_scan256(hc);
        const uint32_t hb = (uint32_t)pick_bin256(hc, (uint32_t)a.top_k, &sel, &rem_c);
        const uint32_t need = rem_c;
        __syncthreads();
        hc[tid] = 0u;
        __syncthreads();
        // B
        row_visit<256, VEC>(x, 0, V, [&](float f, int) {
            const uint32_t k = f16_key(f);
            if ((k >> 8) == hb) atomicAdd(&hc[k & 255u], 1u);
        });
        __syncthreads();
        suffix_scan256(hc);
        tk_key = hb << 8 | (uint32_t)pick_bin256(hc, need, &sel, &rem_c);
        cut_key = tk_key;
    } else {
        mn = -block_reduce_max<256>(-mn, red);
        cut_key = f16_key(mn);
    }
    const float inv_T = 1.f / T;              // exp((l - l_max) / T): the difference of two fp16 values is exact, and with T = 1 so is the product
    if (use_p) {
        hm[tid] = 0ull;
        __syncthreads();
        // C
        row_visit<256, VEC>(x, 0, V, [&](float f, int) {
            const uint32_t k = f16_key(f);
            if (k >= tk_key) atomicAdd(&hm[k >> 8], mass_units(__expf((f - mx) * inv_T)));
        });
        __syncthreads();
        suffix_scan256(hm);
        const unsigned long long total = hm[0];            // >= 2^40: the row maximum is in S_k
        unsigned long long target = (unsigned long long)ceil((double)a.top_p * (double)total);
        target = target < 1ull ? 1ull : (target > total ? total : target);
        const uint32_t hb = (uint32_t)pick_bin256(hm, target, &sel, &rem_m);
        const unsigned long long need = rem_m;
        __syncthreads();
        hm[tid] = 0ull;
        __syncthreads();
        // D
        row_visit<256, VEC>(x, 0, V, [&](float f, int) {
            const uint32_t k = f16_key(f);
            if ((k >> 8) == hb && k >= tk_key) atomicAdd(&hm[k & 255u], mass_units(__expf((f - mx) * inv_T)));
        });
        __syncthreads();
        suffix_scan256(hm);
        cut_key = hb << 8 | (uint32_t)pick_bin256(hm, need, &sel, &rem_m);
    }
    const float cut = key_value(cut_key);
    // E: sample_row_body's second loop over l >= cut (row key, u and gum are that body's)
    uint64_t seed = *a.seed_cell + a.seed_add;
    seed = seed * 0x9E3779B97F4A7C15ull + (uint64_t)a.rng_stream * 0xD1B54A32D192ED03ull + 0x632BE59BD9B4E019ull;
    DropCtx rng;
    rng.k0 = (uint32_t)seed;
    rng.k1 = (uint32_t)(seed >> 32) | 1u;
    rng.thresh = 0u;
    rng.scale = 1.f;
    const uint32_t rkey = drop_rowkey(rng, (uint64_t)row);
    float sum = 0.f, best = -INFINITY;
    int bi = 0x7fffffff, cnt = 0;
    row_visit<256, VEC>(x, 0, V, [&](float f, int v) {
        if (f >= cut) {
            const float z = f / T;
            ++cnt;
            sum += __expf((f - mx) * inv_T);
            const uint32_t h = mix32(rkey + (uint32_t)v * 0x9E3779B9u);
            const float u = ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f);      // (0, 1)
            const float gum = -__logf(-__logf(u));
            const float val = z + gum;
            if (val > best) { best = val; bi = v; }
        }
    });
    if (cnt) atomicAdd(&n_kept, cnt);
    sum = block_reduce_sum<256>(sum, red);
    argmax_block256(best, bi, sv, si);
    if (tid == 0) {
        const int id = si[0] < V ? si[0] : 0;              // (nothing drawable, a row of -inf or NaN: column 0, never an address past the row)
        a.ids[row * a.ids_stride] = id;
        if (a.ids2) a.ids2[row * a.ids2_stride] = id;
        a.logp[row * a.logp_stride] = ((float)x[id] - mx) / T - __logf(sum);
        if (a.cutoff) a.cutoff[row] = cut;
        if (a.kept) a.kept[row] = n_kept;
    }
}

extern "C" int vlp_sample_rows_filtered(const void* logits, int64_t ld, int32_t rows, int32_t V, int32_t rep, const uint64_t* seed_cell, uint64_t seed_add,
                                        uint32_t rng_stream, float temperature, int32_t top_k, float top_p, int64_t* ids, int64_t ids_stride, int64_t* ids2,
                                        int64_t ids2_stride, float* logp, int64_t logp_stride, float* cutoff, int32_t* kept, void* stream) {
    VLP_CHECK_ARG(logits && ids && logp && seed_cell && (uintptr_t)seed_cell % 8 == 0 && rows > 0 && V > 0 && ld >= V && rep >= 1,
                  "vlp_sample_rows_filtered: bad args");
    VLP_CHECK_ARG(std::isfinite(temperature) && temperature > 0.f, "vlp_sample_rows_filtered: temperature must be finite and > 0 (got %g)", (double)temperature);
    VLP_CHECK_ARG(top_k >= 0, "vlp_sample_rows_filtered: top_k must be >= 0 (got %d)", (int)top_k);
    VLP_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "vlp_sample_rows_filtered: top_p must be in (0, 1] (got %g)", (double)top_p);
    VLP_CHECK_ARG(top_p == 1.f || V <= VLP_FILTER_MAX_TOP_P_COLS, "vlp_sample_rows_filtered: top_p < 1 takes rows of at most %d columns (got %d)",
                  VLP_FILTER_MAX_TOP_P_COLS, (int)V);
    VLP_ENTER(logits, "vlp_sample_rows_filtered");
    SampleFilterArgs a;
    a.logits = (const f16*)logits; a.ld = ld; a.V = V; a.rep = rep;
    a.seed_cell = seed_cell; a.seed_add = seed_add; a.rng_stream = rng_stream;
    a.T = temperature; a.top_k = top_k < V ? top_k : 0; a.top_p = top_p;
    a.ids = ids; a.ids_stride = ids_stride; a.ids2 = ids2; a.ids2_stride = ids2_stride; a.logp = logp; a.logp_stride = logp_stride;
    a.cutoff = cutoff; a.kept = kept;
    if ((uintptr_t)logits % 16 == 0 && ld % 8 == 0)
        hipLaunchKernelGGL(sample_rows_filtered_kernel<true>, dim3(rows), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(sample_rows_filtered_kernel<false>, dim3(rows), dim3(256), 0, (hipStream_t)stream, a);
    VLP_CHECK_LAUNCH("vlp_sample_rows_filtered");
    return VLP_OK;
}
