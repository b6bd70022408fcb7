// Loss kernels of the VLP hot path for gfx950.
//   masked-LM: CrossEntropyLoss(reduction='none') in fp32 over the tied-decoder logits, masked_weights,
//              per-sample sum, drop-worst top-k, normalisation (modeling.py:1083-1111);
//              with label smoothing the per-row KL of loss.py LabelSmoothingLoss instead of the CE (modeling.py:1104-1106);
//   VQA:       BCEWithLogitsLoss(mean) * num_answers (modeling.py:1030, 1140).
#include "keep_count.h"
#include "vocab_row.h"

#define CE_THREADS 256

// ---------------------------------------------------------------------------------------------
// Vocabulary-row losses.  Forward: one block per row, a max pass and a sum-exp pass give lse[row] = m + log S; a policy says whether
// A = sum (z - m) is accumulated as well (SUM_D) and what the row's second output is; TEMPERED scales z - m by the policy's 1 / T (the row is
// that of z / T, lse included) and SUM_ED accumulates A = sum e^d d, the entropy's sum.  Backward: grid (chunks of the row, rows), every
// 8-column chunk of [0, ldd) is written -- the policy's per-element expression below V, zeros in the pad columns [V, ldd) and on a row the
// policy zeroes.  Labels are clamped to [0, V).
// ---------------------------------------------------------------------------------------------
template <typename Policy>
__global__ __launch_bounds__(CE_THREADS) void row_lse_kernel(const f16* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                             float* __restrict__ lse, float* __restrict__ out, int V, Policy p) {
    __shared__ float sh[8];
    const int row = blockIdx.x;
    const f16* x = logits + (int64_t)row * ld;
    float mx = -INFINITY;
    row_visit<CE_THREADS, true>(x, 0, V, [&](float z, int) { mx = fmaxf(mx, z); });
    mx = block_reduce_max<CE_THREADS>(mx, sh);
    float s = 0.f, a = 0.f;
    row_visit<CE_THREADS, true>(x, 0, V, [&](float z, int) {
        float d = z - mx;
        if constexpr (Policy::TEMPERED) d = d * p.inv_T;    // subtract, then scale: d <= 0 whatever T is
        const float e = __expf(d);
        s += e;
        if constexpr (Policy::SUM_D) a += d;
        if constexpr (Policy::SUM_ED) a += d == -INFINITY ? 0.f : e * d;      // a -inf logit: 0 log 0 = 0, never 0 * inf
    });
    s = block_reduce_sum<CE_THREADS>(s, sh);
    if constexpr (Policy::SUM_D || Policy::SUM_ED) a = block_reduce_sum<CE_THREADS>(a, sh);
    if (threadIdx.x == 0) {
        const float ls = __logf(s);
        int64_t lab = labels[row];
        lab = lab < 0 ? 0 : (lab >= V ? V - 1 : lab);
        if constexpr (Policy::TEMPERED) mx = mx / p.T;      // max of z / T
        if constexpr (Policy::SUM_ED) a = a / s;            // sum q_v d_v: the entropy is log S - A / S
        lse[row] = mx + ls;
        out[row] = p.row_out(x, lab, V, mx, ls, a);
    }
}
// rc / rc_scale: the operands of the policy's row constant.  They are kernel arguments, not policy members, and rc_scale sits behind V: in the
// other forms tried the compiler loaded the label, waited, and only then loaded the row constant and lse -- a second scalar round trip per block,
// +0.9 us on the 30 us launch of vlp_token_logprob_bwd (profiles/vocab_row_refactor_ab.txt).
template <typename Policy>
__global__ __launch_bounds__(CE_THREADS) void dlogits_row_kernel(const f16* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                                 const float* __restrict__ lse, const float* __restrict__ rc,
                                                                 f16* __restrict__ dl, int64_t ldd, int V, const float* __restrict__ rc_scale, Policy p) {
    const int row = blockIdx.y;
    const f16* x = logits + (int64_t)row * ld;
    f16* d = dl + (int64_t)row * ldd;
    const auto c = p.row_const(rc, rc_scale, row);          // a float, or the policy's struct of per-row values
    const float l = lse[row];
    int64_t lab = labels[row];
    lab = lab < 0 ? 0 : (lab >= V ? V - 1 : lab);
    const int n8 = (int)(ldd >> 3);
    if (p.zero_row(lab)) {
        f16x8 z;
#pragma unroll
        for (int e = 0; e < 8; ++e) z[e] = (f16)0.f;
        for (int ch = blockIdx.x * CE_THREADS + threadIdx.x; ch < n8; ch += gridDim.x * CE_THREADS) st8(d + ch * 8, z);
        return;
    }
    for (int ch = blockIdx.x * CE_THREADS + threadIdx.x; ch < n8; ch += gridDim.x * CE_THREADS) {
        const int v0 = ch * 8;
        f16x8 o;
        if (v0 + 8 <= V) {
            f16x8 t = ld8(x + v0);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (f16)p.elem(c, (float)t[e], l, v0 + e, lab);
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int v = v0 + e;
                o[e] = v < V ? (f16)p.elem(c, (float)x[v], l, v, lab) : (f16)0.f;
            }
        }
        st8(d + v0, o);
    }
}
// the layout and alignment checks and the launch geometry of the two templates, for all entry points
template <typename Policy>
static int row_lse_launch(const char* who, const char* layout_msg, const void* logits, int64_t ld, const int64_t* labels, float* lse, float* out, int rows,
                          int V, Policy p, hipStream_t s) {
    VLP_CHECK_ARG(ld % 8 == 0 && ld >= V && (uintptr_t)logits % 16 == 0, "%s", layout_msg);
    hipLaunchKernelGGL(row_lse_kernel<Policy>, dim3(rows), dim3(CE_THREADS), 0, s, (const f16*)logits, ld, labels, lse, out, V, p);
    VLP_CHECK_LAUNCH(who);
    return VLP_OK;
}
template <typename Policy>
static int dlogits_row_launch(const char* who, int min_V, const void* logits, int64_t ld, const int64_t* labels, const float* lse, const float* rc,
                              const float* rc_scale, void* dlogits, int64_t ldd, int rows, int V, Policy p, void* stream) {
    VLP_CHECK_ARG(rows > 0 && V >= min_V && ld % 8 == 0 && ld >= V && ldd % 8 == 0 && ldd >= V, "%s: layout", who);
    VLP_CHECK_ARG(((uintptr_t)logits | (uintptr_t)dlogits) % 16 == 0, "%s: alignment", who);
    int bx = cdiv(ldd / 8, CE_THREADS);
    if (bx > 16) bx = 16;
    hipLaunchKernelGGL(dlogits_row_kernel<Policy>, dim3(bx, rows), dim3(CE_THREADS), 0, (hipStream_t)stream, (const f16*)logits, ld, labels, lse, rc,
                       (f16*)dlogits, ldd, V, rc_scale, p);
    VLP_CHECK_LAUNCH(who);
    return VLP_OK;
}

// cross entropy: row_loss[row] = lse - logit[label];  d row_loss / d z[w] = p[w] - [w == label], times coef[row] * grad_scale
struct CeRow {
    static constexpr bool SUM_D = false, TEMPERED = false, SUM_ED = false;
    DEVFN float row_out(const f16* x, int64_t lab, int, float mx, float ls, float) const { return (mx + ls) - (float)x[lab]; }
};
struct CeGrad {
    DEVFN bool zero_row(int64_t) const { return false; }
    DEVFN float row_const(const float* coef, const float* gscale, int row) const { return coef[row] * gscale[0]; }
    DEVFN float elem(float c, float z, float l, int v, int64_t lab) const { return c * (__expf(z - l) - (v == lab ? 1.f : 0.f)); }
};

// single block: masking, per-sample sums, drop-worst selection by rank, normalisation (modeling.py:1083-1093)
__global__ __launch_bounds__(1024) void mlm_finish_kernel(const float* __restrict__ row_loss, const int64_t* __restrict__ weights,
                                                          float* __restrict__ loss, float* __restrict__ coef, int B, int P, int keep_n) {
    extern __shared__ float shm[];
    float* ssum = shm;          // [B] per-sample masked loss
    float* wsum = shm + B;      // [B] per-sample weight sum
    float* keep = shm + 2 * B;  // [B]
    __shared__ float red[16];
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        float s = 0.f, w = 0.f;
        for (int p = 0; p < P; ++p) {
            const float wt = (float)weights[b * P + p];
            s += row_loss[b * P + p] * wt;
            w += wt;
        }
        ssum[b] = s;
        wsum[b] = w;
    }
    __syncthreads();
    float den_part = 0.f, loss_part = 0.f;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        // rank among samples (smallest first, ties broken by index) == torch.topk(largest=False) membership
        int rank = 0;
        const float sb = ssum[b];
        for (int j = 0; j < B; ++j) rank += (ssum[j] < sb || (ssum[j] == sb && j < b)) ? 1 : 0;
        const float k = rank < keep_n ? 1.f : 0.f;
        keep[b] = k;
        den_part += k * wsum[b];
        loss_part += k * sb;
    }
    const float den = block_reduce_sum<1024>(den_part, red) + 1e-5f;
    const float tot = block_reduce_sum<1024>(loss_part, red);
    if (threadIdx.x == 0) loss[0] = tot / den;
    __syncthreads();
    for (int i = threadIdx.x; i < B * P; i += blockDim.x) coef[i] = keep[i / P] * (float)weights[i] / den;
}

extern "C" int vlp_mlm_loss_fwd(const vlp_mlm_loss_fwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->logits && a->labels && a->weights && a->loss && a->lse && a->coef && a->row_loss, "vlp_mlm_loss_fwd: null operand");
    VLP_ENTER(a->logits, "vlp_mlm_loss_fwd");
    VLP_CHECK_ARG(a->B > 0 && a->P > 0 && a->V > 0 && a->B <= 4096, "vlp_mlm_loss_fwd: bad shape (B <= 4096)");
    VLP_CHECK_ARG(a->drop_worst_ratio >= 0.f && a->drop_worst_ratio < 1.f, "vlp_mlm_loss_fwd: drop_worst_ratio");
    hipStream_t s = (hipStream_t)stream;
    const int rc = row_lse_launch("vlp_mlm_loss_fwd(ce)", "vlp_mlm_loss_fwd: logits layout", a->logits, a->ld_logits, a->labels, a->lse, a->row_loss,
                                  a->B * a->P, a->V, CeRow{}, s);
    if (rc != VLP_OK) return rc;
    const int keep_n = vlp_drop_worst_keep_count(a->B, a->drop_worst_ratio);
    hipLaunchKernelGGL(mlm_finish_kernel, dim3(1), dim3(1024), 3 * a->B * sizeof(float), s, a->row_loss, a->weights, a->loss, a->coef, a->B, a->P, keep_n);
    VLP_CHECK_LAUNCH("vlp_mlm_loss_fwd(finish)");
    return VLP_OK;
}
extern "C" int vlp_mlm_loss_bwd(const vlp_mlm_loss_bwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->logits && a->labels && a->lse && a->coef && a->grad_scale && a->dlogits, "vlp_mlm_loss_bwd: null operand");
    VLP_ENTER(a->logits, "vlp_mlm_loss_bwd");
    return dlogits_row_launch("vlp_mlm_loss_bwd", 1, a->logits, a->ld_logits, a->labels, a->lse, a->coef, a->grad_scale, a->dlogits, a->ld_dlogits, a->rows,
                              a->V, CeGrad{}, stream);
}

// ---------------------------------------------------------------------------------------------
// Label-smoothed masked-LM loss (loss.py LabelSmoothingLoss, modeling.py:995-999, 1104-1106):
//   q[w] = smooth for w != ignore, q[label] = confidence, q == 0 on a row whose label is `ignore`;
//   row_loss = sum_w q[w] (log q[w] - logp[w])        (0 log 0 = 0)
// With m = max, S = sum exp(z - m), A = sum_{w != ignore} (z_w - m) and logp_w = z_w - m - log S:
//   sum_w q log q    = (V-2) s log s + c log c   (q_log_q: a constant of the buffer, passed in as the caller rounds it)
//   sum_w q logp     = s (A - (V-1) log S - logp_t) + c logp_t
// so the two passes of row_lse_kernel give the row's KL without a third one.
// ---------------------------------------------------------------------------------------------
struct CeLsRow {
    static constexpr bool SUM_D = true, TEMPERED = false, SUM_ED = false;
    float smooth, confidence, q_log_q; int ignore;
    DEVFN float row_out(const f16* x, int64_t lab, int V, float mx, float ls, float a) const {
        float r = 0.f;
        if (lab != ignore) {
            a -= (float)x[ignore] - mx;                                   // A runs over w != ignore
            const float lpt = (float)x[lab] - mx - ls;                    // logp[label]
            const float sum_lp = a - (float)(V - 1) * ls;                 // sum_{w != ignore} logp[w]
            r = q_log_q - smooth * (sum_lp - lpt) - confidence * lpt;
        }
        return r;
    }
};
// d row_loss / d z[w] = p[w] * sum(q) - q[w]; zero on a row whose label is `ignore`
struct CeLsGrad {
    float smooth, confidence, q_sum; int ignore;
    DEVFN bool zero_row(int64_t lab) const { return lab == ignore; }
    DEVFN float row_const(const float* coef, const float* gscale, int row) const { return coef[row] * gscale[0]; }
    DEVFN float elem(float c, float z, float l, int v, int64_t lab) const {
        const float q = v == lab ? confidence : (v == ignore ? 0.f : smooth);
        return c * (__expf(z - l) * q_sum - q);
    }
};

extern "C" int vlp_mlm_loss_ls_fwd(const vlp_mlm_loss_ls_fwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->logits && a->labels && a->weights && a->loss && a->lse && a->coef && a->row_loss, "vlp_mlm_loss_ls_fwd: null operand");
    VLP_ENTER(a->logits, "vlp_mlm_loss_ls_fwd");
    VLP_CHECK_ARG(a->B > 0 && a->P > 0 && a->V > 2 && a->B <= 4096, "vlp_mlm_loss_ls_fwd: bad shape (B <= 4096, V > 2)");
    VLP_CHECK_ARG(a->drop_worst_ratio >= 0.f && a->drop_worst_ratio < 1.f, "vlp_mlm_loss_ls_fwd: drop_worst_ratio");
    VLP_CHECK_ARG(a->smooth >= 0.f && a->confidence >= 0.f && a->q_sum > 0.f && a->ignore_index >= 0 && a->ignore_index < a->V,
                  "vlp_mlm_loss_ls_fwd: smoothing parameters");
    hipStream_t s = (hipStream_t)stream;
    const int rc = row_lse_launch("vlp_mlm_loss_ls_fwd(row)", "vlp_mlm_loss_ls_fwd: logits layout", a->logits, a->ld_logits, a->labels, a->lse, a->row_loss,
                                  a->B * a->P, a->V, CeLsRow{a->smooth, a->confidence, a->q_log_q, a->ignore_index}, s);
    if (rc != VLP_OK) return rc;
    const int keep_n = vlp_drop_worst_keep_count(a->B, a->drop_worst_ratio);
    hipLaunchKernelGGL(mlm_finish_kernel, dim3(1), dim3(1024), 3 * a->B * sizeof(float), s, a->row_loss, a->weights, a->loss, a->coef, a->B, a->P, keep_n);
    VLP_CHECK_LAUNCH("vlp_mlm_loss_ls_fwd(finish)");
    return VLP_OK;
}
extern "C" int vlp_mlm_loss_ls_bwd(const vlp_mlm_loss_ls_bwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->logits && a->labels && a->lse && a->coef && a->grad_scale && a->dlogits, "vlp_mlm_loss_ls_bwd: null operand");
    VLP_ENTER(a->logits, "vlp_mlm_loss_ls_bwd");
    VLP_CHECK_ARG(a->smooth >= 0.f && a->confidence >= 0.f && a->q_sum > 0.f && a->ignore_index >= 0 && a->ignore_index < a->V,
                  "vlp_mlm_loss_ls_bwd: smoothing parameters");
    return dlogits_row_launch("vlp_mlm_loss_ls_bwd", 3, a->logits, a->ld_logits, a->labels, a->lse, a->coef, a->grad_scale, a->dlogits, a->ld_dlogits,
                              a->rows, a->V, CeLsGrad{a->smooth, a->confidence, a->q_sum, a->ignore_index}, stream);
}

// ---------------------------------------------------------------------------------------------
// Log-probability of one chosen token per row (SCST: the sampled caption's log-probs, modeling.py:1229-1235):
//   logp[r] = logit[r, id[r]] - lse_r;  backward dlogits[r, v] = g[r] * ([v == id[r]] - exp(logit[r, v] - lse_r)).
// g is a per-row upstream gradient of either sign (it carries the loss scale).
// ---------------------------------------------------------------------------------------------
struct TokenLogpRow {
    static constexpr bool SUM_D = false, TEMPERED = false, SUM_ED = false;
    DEVFN float row_out(const f16* x, int64_t id, int, float mx, float ls, float) const { return (float)x[id] - (mx + ls); }
};
struct TokenLogpGrad {
    DEVFN bool zero_row(int64_t) const { return false; }
    DEVFN float row_const(const float* g, const float*, int row) const { return g[row]; }
    DEVFN float elem(float c, float z, float l, int v, int64_t id) const { return c * ((v == id ? 1.f : 0.f) - __expf(z - l)); }
};

extern "C" int vlp_token_logprob_fwd(const vlp_token_logprob_fwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->logits && a->ids && a->logp && a->lse, "vlp_token_logprob_fwd: null operand");
    VLP_ENTER(a->logits, "vlp_token_logprob_fwd");
    VLP_CHECK_ARG(a->rows > 0 && a->V > 0, "vlp_token_logprob_fwd: layout");
    return row_lse_launch("vlp_token_logprob_fwd", "vlp_token_logprob_fwd: layout", a->logits, a->ld_logits, a->ids, a->lse, a->logp, a->rows, a->V,
                          TokenLogpRow{}, (hipStream_t)stream);
}
extern "C" int vlp_token_logprob_bwd(const vlp_token_logprob_bwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->logits && a->ids && a->lse && a->g && a->dlogits, "vlp_token_logprob_bwd: null operand");
    VLP_ENTER(a->logits, "vlp_token_logprob_bwd");
    return dlogits_row_launch("vlp_token_logprob_bwd", 1, a->logits, a->ld_logits, a->ids, a->lse, a->g, nullptr, a->dlogits, a->ld_dlogits, a->rows, a->V,
                              TokenLogpGrad{}, stream);
}

// ---------------------------------------------------------------------------------------------
// The SCST policy pi_T = softmax(logits / T) of one chosen token per row, with its entropy (include/vlp_hip.h vlp_token_policy_fwd):
//   z = l / T, lse = logsumexp(z), q = exp(z - lse), logp = z_id - lse, H = -sum q log q = log S - A / S with d = (l - max) / T,
//   S = sum e^d, A = sum e^d d (row_lse_kernel's second pass);
//   dlogits[v] = (g / T) ([v == id] - q_v) - (h / T) q_v (log q_v + H), the entropy term skipped where q_v == 0.
// Elements and upstream gradients are scaled by 1 / T (one rounding, the host's); the forward's two per-row values are divided by T.  T == 1
// without entropy / h computes TokenLogpRow's / TokenLogpGrad's expressions: 1 * d, 1 * z - l, 1 * g and x / 1 are exact.
// ---------------------------------------------------------------------------------------------
template <bool ENT>
struct TokenPolicyRow {
    static constexpr bool SUM_D = false, TEMPERED = true, SUM_ED = ENT;
    float T, inv_T; float* entropy;
    // mx: the max of z; a: sum q_v d_v.  One block per row (row_lse_kernel): the row is blockIdx.x
    DEVFN float row_out(const f16* x, int64_t id, int, float mx, float ls, float a) const {
        if constexpr (ENT) entropy[blockIdx.x] = ls - a;
        return (float)x[id] / T - (mx + ls);
    }
};
struct TokenPolicyRc { float c, ch, H; };          // g / T, h / T (as products with 1 / T) and the row's entropy
template <bool ENT>
struct TokenPolicyGrad {
    float inv_T; const float* h; const float* entropy;
    DEVFN bool zero_row(int64_t) const { return false; }
    DEVFN auto row_const(const float* g, const float*, int row) const {
        // products, not quotients: a thread of this grid handles one or two chunks, and a division ahead of them showed in the launch's time
        if constexpr (ENT) return TokenPolicyRc{g[row] * inv_T, h[row] * inv_T, entropy[row]};
        else return g[row] * inv_T;
    }
    DEVFN float elem(float c, float z, float l, int v, int64_t id) const { return c * ((v == id ? 1.f : 0.f) - __expf(z * inv_T - l)); }
    DEVFN float elem(const TokenPolicyRc& r, float z, float l, int v, int64_t id) const {
        const float lq = z * inv_T - l, q = __expf(lq);
        const float gt = r.c * ((v == id ? 1.f : 0.f) - q);
        return q > 0.f ? gt - r.ch * (q * (lq + r.H)) : gt;              // q == 0 (a -inf logit, or underflow): no 0 * inf
    }
};

// finite and > 0 (false for a NaN); a subnormal T, whose reciprocal is inf, is refused with them
static bool policy_temperature_ok(float T) { return T >= 1.17549435e-38f && T <= 3.402823466e+38f; }

extern "C" int vlp_token_policy_fwd(const vlp_token_policy_fwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->logits && a->ids && a->logp && a->lse, "vlp_token_policy_fwd: null operand");
    VLP_ENTER(a->logits, "vlp_token_policy_fwd");
    VLP_CHECK_ARG(a->rows > 0 && a->V > 0, "vlp_token_policy_fwd: layout");
    VLP_CHECK_ARG(policy_temperature_ok(a->temperature), "vlp_token_policy_fwd: temperature must be finite and > 0");
    if (a->entropy)
        return row_lse_launch("vlp_token_policy_fwd", "vlp_token_policy_fwd: layout", a->logits, a->ld_logits, a->ids, a->lse, a->logp, a->rows, a->V,
                              TokenPolicyRow<true>{a->temperature, 1.f / a->temperature, a->entropy}, (hipStream_t)stream);
    return row_lse_launch("vlp_token_policy_fwd", "vlp_token_policy_fwd: layout", a->logits, a->ld_logits, a->ids, a->lse, a->logp, a->rows, a->V,
                          TokenPolicyRow<false>{a->temperature, 1.f / a->temperature, nullptr}, (hipStream_t)stream);
}
extern "C" int vlp_token_policy_bwd(const vlp_token_policy_bwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->logits && a->ids && a->lse && a->g && a->dlogits, "vlp_token_policy_bwd: null operand");
    VLP_ENTER(a->logits, "vlp_token_policy_bwd");
    VLP_CHECK_ARG(policy_temperature_ok(a->temperature), "vlp_token_policy_bwd: temperature must be finite and > 0");
    VLP_CHECK_ARG(!a->h || a->entropy, "vlp_token_policy_bwd: h needs the entropy the forward saved");
    const float T = a->temperature;
    if (a->h)
        return dlogits_row_launch("vlp_token_policy_bwd", 1, a->logits, a->ld_logits, a->ids, a->lse, a->g, nullptr, a->dlogits, a->ld_dlogits, a->rows,
                                  a->V, TokenPolicyGrad<true>{1.f / T, a->h, a->entropy}, stream);
    return dlogits_row_launch("vlp_token_policy_bwd", 1, a->logits, a->ld_logits, a->ids, a->lse, a->g, nullptr, a->dlogits, a->ld_dlogits, a->rows,
                              a->V, TokenPolicyGrad<false>{1.f / T, nullptr, nullptr}, stream);
}

// ---------------------------------------------------------------------------------------------
// Scoring a given token per row (include/vlp_hip.h vlp_token_score): what vlp_token_policy_fwd writes at T = 1 with entropy -- the same
// expressions in the same order, without the products and quotients by T = 1 (exact there), so logp / lse / entropy are its bits on a
// 16-byte aligned row -- plus the token's rank and the row's arg-max, which ride on the max pass: the token's own logit is read first, every
// thread counts the columns that beat it (exact comparisons of fp16 values) and keeps its first maximum.  The counts are reduced as floats:
// a count is <= V <= 2^24, so every partial sum is an exact integer.  A row with id < 0 is not read.
// VEC = false walks a row that is not 16-byte aligned column by column (another thread <-> column assignment: another summation order).
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(CE_THREADS) void token_score_kernel(const f16* __restrict__ logits, int64_t ld, const int64_t* __restrict__ ids,
                                                                 float* __restrict__ logp, float* __restrict__ lse, float* __restrict__ entropy,
                                                                 int32_t* __restrict__ rank, int64_t* __restrict__ top_id,
                                                                 float* __restrict__ top_logit, int V) {
    __shared__ float sh[8];
    __shared__ float sv[CE_THREADS];
    __shared__ int si[CE_THREADS];
    const int row = blockIdx.x;
    int64_t id64 = ids[row];
    if (id64 < 0) {                                         // block-uniform: an uncounted position costs one launch slot and six stores
        if (threadIdx.x == 0) {
            logp[row] = 0.f; lse[row] = 0.f; entropy[row] = 0.f;
            rank[row] = -1; top_id[row] = -1; top_logit[row] = 0.f;
        }
        return;
    }
    const int id = (int)(id64 >= V ? V - 1 : id64);
    const f16* x = logits + (int64_t)row * ld;
    const float lid = (float)x[id];
    float mx = -INFINITY;
    int bi = 0x7fffffff, cnt = 0;
    row_visit<CE_THREADS, VEC>(x, 0, V, [&](float z, int v) {
        bi = z > mx ? v : bi;                               // ascending columns within a thread: `>` keeps the first
        mx = fmaxf(mx, z);
        cnt += (z > lid || (z == lid && v < id)) ? 1 : 0;
    });
    const float best = mx;                                  // this thread's maximum, at column bi
    mx = block_reduce_max<CE_THREADS>(mx, sh);
    float s = 0.f, a = 0.f;
    row_visit<CE_THREADS, VEC>(x, 0, V, [&](float z, int) {
        const float d = z - mx;
        const float e = __expf(d);
        s += e;
        a += d == -INFINITY ? 0.f : e * d;                  // a -inf logit: 0 log 0 = 0, never 0 * inf
    });
    s = block_reduce_sum<CE_THREADS>(s, sh);
    a = block_reduce_sum<CE_THREADS>(a, sh);
    const float above = block_reduce_sum<CE_THREADS>((float)cnt, sh);
    argmax_block256(best, bi, sv, si);
    if (threadIdx.x == 0) {
        const float ls = __logf(s);
        a = a / s;                                          // sum q_v d_v: the entropy is log S - A / S
        lse[row] = mx + ls;
        entropy[row] = ls - a;
        logp[row] = lid - (mx + ls);
        rank[row] = (int32_t)above;
        top_id[row] = si[0] == 0x7fffffff ? 0 : si[0];      // no column above -inf (all -inf / NaN): column 0, as a first-maximum scan says
        top_logit[row] = sv[0];
    }
}

extern "C" int vlp_token_score(const vlp_token_score_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->logits && a->ids && a->logp && a->lse && a->entropy && a->rank && a->top_id && a->top_logit, "vlp_token_score: null operand");
    VLP_ENTER(a->logits, "vlp_token_score");
    VLP_CHECK_ARG(a->rows > 0 && a->V > 0 && a->V <= (1 << 24) && a->ld_logits >= a->V && (uintptr_t)a->logits % 2 == 0, "vlp_token_score: layout");
    const bool vec = a->ld_logits % 8 == 0 && (uintptr_t)a->logits % 16 == 0;
    hipLaunchKernelGGL(vec ? token_score_kernel<true> : token_score_kernel<false>, dim3(a->rows), dim3(CE_THREADS), 0, (hipStream_t)stream,
                       (const f16*)a->logits, a->ld_logits, a->ids, a->logp, a->lse, a->entropy, a->rank, a->top_id, a->top_logit, a->V);
    VLP_CHECK_LAUNCH("vlp_token_score");
    return VLP_OK;
}

// ---------------------------------------------------------------------------------------------
// BCE with logits.  loss = sum_{b,n} [max(x,0) - x*y + log(1 + exp(-|x|))] / (B*N) * N
// ---------------------------------------------------------------------------------------------
// Where y comes from is a template parameter (as the forbidden words of the top-k kernels are): SPARSE = false reads the dense f32 [B, ldl]
// target, SPARSE = true reads the row's S (answer index, score) pairs -- y is the score of the pair whose index is the column, 0 when no
// pair lists it (idx -1 = empty slot; the indices of a row are distinct, so at most one pair hits).  The pairs of the rows a block's current
// 256-element tile touches sit in LDS.  Element -> thread assignment, the per-element expression and the summation order do not depend on
// SPARSE, so both forms give the same bits for the same y.
struct BceAnswers { const int32_t* idx; const float* score; int S; };
// rows a tile of 256 consecutive elements of a [B, W] array can touch
static inline int bce_tile_rows(int B, int64_t W) {
    const int64_t r = 255 / W + 2;
    return (int)(r < B ? r : B);
}
// the pairs of rows [b0, b0 + nr) -> LDS (contiguous in memory); visible to the block after its next __syncthreads()
DEVFN void bce_pairs_load(const BceAnswers& sa, int64_t b0, int nr, int32_t* l_idx, float* l_sc) {
    const int n = nr * sa.S;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        l_idx[j] = sa.idx[b0 * sa.S + j];
        l_sc[j] = sa.score[b0 * sa.S + j];
    }
}
DEVFN float bce_pairs_y(const int32_t* l_idx, const float* l_sc, int S, int r, int n) {
    float yv = 0.f;
    for (int s = 0; s < S; ++s) yv = l_idx[r * S + s] == n ? l_sc[r * S + s] : yv;
    return yv;
}
template <bool SPARSE>
__global__ __launch_bounds__(256) void bce_fwd_kernel(const f16* x, int64_t ld, const float* y, int64_t ldl, BceAnswers sa, int tile_rows, int B, int N,
                                                      float* part) {
    __shared__ float sh[8];
    extern __shared__ __attribute__((aligned(16))) char bce_smem[];
    int32_t* l_idx = (int32_t*)bce_smem;
    float* l_sc = (float*)(bce_smem + (size_t)tile_rows * sa.S * sizeof(int32_t));
    float s = 0.f;
    const int64_t total = (int64_t)B * N;
    // block-uniform trip count (the tile's pairs are loaded between two barriers); thread t still walks base + t in ascending order
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        int64_t b0 = 0;
        if constexpr (SPARSE) {
            b0 = base / N;
            const int64_t last = (base + blockDim.x - 1 < total ? base + blockDim.x - 1 : total - 1) / N;
            __syncthreads();                                 // the previous tile's readers are done
            bce_pairs_load(sa, b0, (int)(last - b0) + 1, l_idx, l_sc);
            __syncthreads();
        }
        if (i < total) {
            const int64_t b = i / N;
            const int n = (int)(i % N);
            const float xv = (float)x[b * ld + n];
            float yv;
            if constexpr (SPARSE) yv = bce_pairs_y(l_idx, l_sc, sa.S, (int)(b - b0), n);
            else yv = y[b * ldl + n];
            s += fmaxf(xv, 0.f) - xv * yv + log1pf(__expf(-fabsf(xv)));
        }
    }
    s = block_reduce_sum<256>(s, sh);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}
__global__ void bce_finish_kernel(const float* part, int n, float inv, float* loss) {
    __shared__ float sh[8];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += part[i];
    s = block_reduce_sum<256>(s, sh);
    if (threadIdx.x == 0) loss[0] = s * inv;
}
template <bool SPARSE>
static int bce_fwd_launch(const char* who, const void* logits, int64_t ld, const float* labels, int64_t ldl, BceAnswers sa, int32_t B, int32_t N, float* loss,
                          void* stream) {
    // loss[1..257) is used as scratch: the caller passes a buffer of >= 257 floats
    hipStream_t s = (hipStream_t)stream;
    const int tile_rows = SPARSE ? bce_tile_rows(B, N) : 0;
    const size_t lds = (size_t)tile_rows * sa.S * (sizeof(int32_t) + sizeof(float));
    hipLaunchKernelGGL(bce_fwd_kernel<SPARSE>, dim3(256), dim3(256), lds, s, (const f16*)logits, ld, labels, ldl, sa, tile_rows, B, N, loss + 1);
    VLP_CHECK_LAUNCH(who);
    hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(256), 0, s, loss + 1, 256, 1.f / (float)B, loss);
    VLP_CHECK_LAUNCH(who);
    return VLP_OK;
}
extern "C" int vlp_bce_loss_fwd(const void* logits, int64_t ld, const void* labels, int64_t ldl, int32_t B, int32_t N, float* loss, void* stream) {
    VLP_CHECK_ARG(logits && labels && loss && B > 0 && N > 0 && ld >= N && ldl >= N, "vlp_bce_loss_fwd: bad args");
    VLP_ENTER(logits, "vlp_bce_loss_fwd");
    return bce_fwd_launch<false>("vlp_bce_loss_fwd", logits, ld, (const float*)labels, ldl, BceAnswers{nullptr, nullptr, 0}, B, N, loss, stream);
}
#define BCE_SPARSE_MAX_S 16
extern "C" int vlp_bce_sparse_loss_fwd(const void* logits, int64_t ld, const int32_t* ans_idx, const float* ans_score, int32_t S, int32_t B, int32_t N,
                                       float* loss, void* stream) {
    VLP_CHECK_ARG(logits && ans_idx && ans_score && loss && B > 0 && N > 0 && ld >= N && S > 0 && S <= BCE_SPARSE_MAX_S, "vlp_bce_sparse_loss_fwd: bad args");
    VLP_ENTER(logits, "vlp_bce_sparse_loss_fwd");
    return bce_fwd_launch<true>("vlp_bce_sparse_loss_fwd", logits, ld, nullptr, 0, BceAnswers{ans_idx, ans_score, S}, B, N, loss, stream);
}
template <bool SPARSE>
__global__ __launch_bounds__(256) void bce_bwd_kernel(const f16* x, int64_t ld, const float* y, int64_t ldl, BceAnswers sa, int tile_rows, int B, int N,
                                                      const float* gscale, f16* d, int64_t ldd) {
    extern __shared__ __attribute__((aligned(16))) char bce_smem[];
    int32_t* l_idx = (int32_t*)bce_smem;
    float* l_sc = (float*)(bce_smem + (size_t)tile_rows * sa.S * sizeof(int32_t));
    const float c = gscale[0] / (float)B;
    const int64_t total = (int64_t)B * ldd;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < total; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        int64_t b0 = 0;
        if constexpr (SPARSE) {
            b0 = base / ldd;
            const int64_t last = (base + blockDim.x - 1 < total ? base + blockDim.x - 1 : total - 1) / ldd;
            __syncthreads();
            bce_pairs_load(sa, b0, (int)(last - b0) + 1, l_idx, l_sc);
            __syncthreads();
        }
        if (i < total) {
            const int64_t b = i / ldd;
            const int n = (int)(i % ldd);
            float v = 0.f;
            if (n < N) {
                const float xv = (float)x[b * ld + n];
                float yv;
                if constexpr (SPARSE) yv = bce_pairs_y(l_idx, l_sc, sa.S, (int)(b - b0), n);
                else yv = y[b * ldl + n];
                v = c * (1.f / (1.f + __expf(-xv)) - yv);
            }
            d[i] = (f16)v;
        }
    }
}
template <bool SPARSE>
static int bce_bwd_launch(const char* who, const void* logits, int64_t ld, const float* labels, int64_t ldl, BceAnswers sa, int32_t B, int32_t N,
                          const float* grad_scale, void* dlogits, int64_t ldd, void* stream) {
    const int64_t total = (int64_t)B * ldd;
    int blocks = (int)((total + 255) / 256);
    if (blocks > 2048) blocks = 2048;
    const int tile_rows = SPARSE ? bce_tile_rows(B, ldd) : 0;
    const size_t lds = (size_t)tile_rows * sa.S * (sizeof(int32_t) + sizeof(float));
    hipLaunchKernelGGL(bce_bwd_kernel<SPARSE>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, (const f16*)logits, ld, labels, ldl, sa, tile_rows, B, N,
                       grad_scale, (f16*)dlogits, ldd);
    VLP_CHECK_LAUNCH(who);
    return VLP_OK;
}
extern "C" int vlp_bce_loss_bwd(const void* logits, int64_t ld, const void* labels, int64_t ldl, int32_t B, int32_t N, const float* grad_scale,
                                void* dlogits, int64_t ldd, void* stream) {
    VLP_CHECK_ARG(logits && labels && grad_scale && dlogits && B > 0 && N > 0 && ld >= N && ldl >= N && ldd >= N, "vlp_bce_loss_bwd: bad args");
    VLP_ENTER(logits, "vlp_bce_loss_bwd");
    return bce_bwd_launch<false>("vlp_bce_loss_bwd", logits, ld, (const float*)labels, ldl, BceAnswers{nullptr, nullptr, 0}, B, N, grad_scale, dlogits, ldd,
                                 stream);
}
extern "C" int vlp_bce_sparse_loss_bwd(const void* logits, int64_t ld, const int32_t* ans_idx, const float* ans_score, int32_t S, int32_t B, int32_t N,
                                       const float* grad_scale, void* dlogits, int64_t ldd, void* stream) {
    VLP_CHECK_ARG(logits && ans_idx && ans_score && grad_scale && dlogits && B > 0 && N > 0 && ld >= N && ldd >= N && S > 0 && S <= BCE_SPARSE_MAX_S,
                  "vlp_bce_sparse_loss_bwd: bad args");
    VLP_ENTER(logits, "vlp_bce_sparse_loss_bwd");
    return bce_bwd_launch<true>("vlp_bce_sparse_loss_bwd", logits, ld, nullptr, 0, BceAnswers{ans_idx, ans_score, S}, B, N, grad_scale, dlogits, ldd, stream);
}
