// LayerNorm forward / backward and column sums (bias gradients) for gfx950.  HBM-bound kernels:
// 16-byte vector loads, one wave per row, fp32 statistics, two-pass variance from registers.
//
// Replaces BertLayerNorm = apex FusedLayerNorm / the python fallback (modeling.py:174-192; used at
// :214,239 embeddings, :310,316 attention output, :350,356 FFN output, :429,434 head transform) and
// the dropout that follows the embedding LayerNorm (:240); backward replaces their autograd plus the
// SumBackward of every broadcast bias add.
#include "common.h"
#include <climits>
#include <cstdlib>

#define LN_THREADS 256
#define LN_WAVES 4

// What the two forward kernels share: the row's dropout key (dropout element = (row, col); packed rows: the LOGICAL row) and the output
// element from the row's statistics, the affine pair and the dropout multiplier m (1 when dropout is off).
DEVFN uint32_t ln_fwd_rowkey(const DropCtx& drop, const int32_t* __restrict__ row_map, int row) {
    return drop.thresh ? drop_rowkey(drop, row_map ? (uint64_t)(uint32_t)row_map[row] : (uint64_t)row) : 0u;
}
DEVFN f16 ln_fwd_out(float v, float mu, float rs, f16 gamma, f16 beta, float m) { return (f16)(((float)gamma * ((v - mu) * rs) + (float)beta) * m); }

template <int NP>   // per-lane pieces of 4 halfs (piece k = columns 256k + 4*lane .. +3): H <= 256*NP; at H = 768 every lane holds 12 columns
__global__ __launch_bounds__(LN_THREADS) void layernorm_fwd_kernel(
    const f16* __restrict__ x, int64_t ldx, const f16* __restrict__ gamma, const f16* __restrict__ beta,
    f16* __restrict__ y, int64_t ldy, float* __restrict__ mean, float* __restrict__ rstd, int M, int H, float eps, DropCtx drop, const int32_t* __restrict__ row_map) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * LN_WAVES;
    const float invH = 1.f / (float)H;
    for (int row = wave; row < M; row += nwaves) {
        const f16* xr = x + (int64_t)row * ldx;
        float v[NP][4];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int c = 256 * k + 4 * lane;
            if (c < H) {
                f16x4 t = ld4(xr + c);
#pragma unroll
                for (int e = 0; e < 4; ++e) { v[k][e] = (float)t[e]; s += v[k][e]; }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[k][e] = 0.f;
            }
        }
        const float mu = wave_sum(s) * invH;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k)
            if (256 * k + 4 * lane < H) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = v[k][e] - mu; q += d * d; }
            }
        const float var = wave_sum(q) * invH;
        const float rs = 1.f / sqrtf(var + eps);
        if (lane == 0) {
            if (mean) mean[row] = mu;
            if (rstd) rstd[row] = rs;
        }
        f16* yr = y + (int64_t)row * ldy;
        const uint32_t rkey = ln_fwd_rowkey(drop, row_map, row);
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int c = 256 * k + 4 * lane;
            if (c < H) {
                f16x4 gv = ld4(gamma + c), bv = ld4(beta + c), o;
                float m4[4] = {1.f, 1.f, 1.f, 1.f};
                if (drop.thresh) drop_mult4(drop, rkey, (uint32_t)c, m4);
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = ln_fwd_out(v[k][e], mu, rs, gv[e], bv[e], m4[e]);
                st4_out<VLP_SS_LN>(yr + c, o);
            }
        }
    }
}

// Half-wave form for H % 256 == 0 (H = 768, 1024, 2048: every LayerNorm of the model): lanes 0-31 own one row, lanes 32-63 the next, a
// lane holds NC 16-byte chunks (chunk k = columns 256 k + 8 (lane & 31) .. +7).  16-byte loads, twice the bytes in flight per wave, and
// M / 2 waves (5 344 at M = 10 688) fit the chip in ONE round -- the one-row-per-wave grid needs 1.3 rounds of 8 192 resident waves.
template <int NC>
__global__ __launch_bounds__(LN_THREADS, NC <= 3 ? 6 : 4) void layernorm_fwd_hw_kernel(      // NC = 3: <= 80 VGPRs -> 6 144 resident waves >= the 5 344 of M = 10 688
    const f16* __restrict__ x, int64_t ldx, const f16* __restrict__ gamma, const f16* __restrict__ beta,
    f16* __restrict__ y, int64_t ldy, float* __restrict__ mean, float* __restrict__ rstd, int M, int H, float eps, DropCtx drop, const int32_t* __restrict__ row_map) {
    const int lane = threadIdx.x & 63, hl = lane & 31;
    const int wave = blockIdx.x * LN_WAVES + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * LN_WAVES;
    const float invH = 1.f / (float)H;
    for (int pair = wave; 2 * pair < M; pair += nwaves) {
        const int row = 2 * pair + (lane >> 5);
        const bool live = row < M;
        const f16* xr = x + (int64_t)(live ? row : M - 1) * ldx;
        f16x8 t[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) t[k] = ld8(xr + 256 * k + 8 * hl);
        float v[NC][8];
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) { v[k][e] = (float)t[k][e]; s += v[k][e]; }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);          // within the 32-lane half
        const float mu = s * invH;
        float q = 0.f;
#pragma unroll
        for (int k = 0; k < NC; ++k)
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[k][e] - mu; q += d * d; }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
        const float rs = 1.f / sqrtf(q * invH + eps);
        if (hl == 0 && live) {
            if (mean) mean[row] = mu;
            if (rstd) rstd[row] = rs;
        }
        if (!live) continue;
        f16* yr = y + (int64_t)row * ldy;
        const uint32_t rkey = ln_fwd_rowkey(drop, row_map, row);
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int c = 256 * k + 8 * hl;
            const f16x8 gv = ld8(gamma + c), bv = ld8(beta + c);
            float m8[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
            if (drop.thresh) drop_mult8(drop, rkey, (uint32_t)c, m8);
            f16x8 o;
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = ln_fwd_out(v[k][e], mu, rs, gv[e], bv[e], m8[e]);
            st8_out<VLP_SS_LN>(yr + c, o);
        }
    }
}

// (Round 4, measured and not kept: a software-pipelined form -- several pairs per wave, the next pair's row requested before the current one
// is reduced and stored, so that reads and writes of different iterations overlap -- is SLOWER at every grid size: 12.4 us at one pair per
// wave (7 spilled registers at the 80-register budget of 6 waves per SIMD), 13.0 / 13.5 / 15.4 / 17.1 us at 2 / 3 / 4 / 5.2 pairs per wave,
// profiles/r04_layernorm_lab.txt.  One pair per wave with every wave resident at once stays the forward.)
// The block caps are read once; the per-call decision is a local (the entry points may be driven from several host threads)
static int env_blocks(const char* name, int dflt, int most) {
    const char* e = getenv(name);
    const int v = e ? atoi(e) : dflt;
    return v < 1 || v > most ? dflt : v;
}

// one row per wave up to this many blocks (VLP_LN_BLOCKS overrides for A/B runs)
static int ln_fwd_blocks(int M) {
    static const int cap = env_blocks("VLP_LN_BLOCKS", 4096, INT_MAX);
    const int blocks = cdiv(M, LN_WAVES);
    return blocks > cap ? cap : blocks;
}

extern "C" int vlp_layernorm_fwd(const vlp_layernorm_fwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->x && a->gamma && a->beta && a->y, "vlp_layernorm_fwd: null operand");
    VLP_ENTER(a->x, "vlp_layernorm_fwd");
    VLP_CHECK_ARG(a->M > 0 && a->H > 0 && a->H % 8 == 0 && a->H <= 4096, "vlp_layernorm_fwd: H=%d must be a multiple of 8 and <= 4096", a->H);
    VLP_CHECK_ARG(a->ldx % 8 == 0 && a->ldy % 8 == 0 && a->ldx >= a->H && a->ldy >= a->H, "vlp_layernorm_fwd: leading dims");
    VLP_CHECK_ARG(((uintptr_t)a->x | (uintptr_t)a->y | (uintptr_t)a->gamma | (uintptr_t)a->beta) % 16 == 0, "vlp_layernorm_fwd: alignment");
    DropCtx d = make_drop(a->dropout_p, a->seed, a->rng_stream);
    const int blocks = ln_fwd_blocks(a->M), hblocks = ln_fwd_blocks((a->M + 1) / 2);
    hipStream_t s = (hipStream_t)stream;
#define LAUNCH_LN_FWD(KERNEL_, BLOCKS_)                                                                                        \
    hipLaunchKernelGGL(KERNEL_, dim3(BLOCKS_), dim3(LN_THREADS), 0, s, (const f16*)a->x, a->ldx, (const f16*)a->gamma,        \
                       (const f16*)a->beta, (f16*)a->y, a->ldy, a->mean, a->rstd, a->M, a->H, a->eps, d, a->row_map)
    switch (a->H) {                     // the H with a half-wave instantiation; every other H: one row per wave
        case 256: LAUNCH_LN_FWD(layernorm_fwd_hw_kernel<1>, hblocks); break;
        case 512: LAUNCH_LN_FWD(layernorm_fwd_hw_kernel<2>, hblocks); break;
        case 768: LAUNCH_LN_FWD(layernorm_fwd_hw_kernel<3>, hblocks); break;
        case 1024: LAUNCH_LN_FWD(layernorm_fwd_hw_kernel<4>, hblocks); break;
        case 1536: LAUNCH_LN_FWD(layernorm_fwd_hw_kernel<6>, hblocks); break;
        case 2048: LAUNCH_LN_FWD(layernorm_fwd_hw_kernel<8>, hblocks); break;
        default:
            if (a->H <= 768) LAUNCH_LN_FWD(layernorm_fwd_kernel<3>, blocks);
            else if (a->H <= 1024) LAUNCH_LN_FWD(layernorm_fwd_kernel<4>, blocks);
            else if (a->H <= 2048) LAUNCH_LN_FWD(layernorm_fwd_kernel<8>, blocks);
            else LAUNCH_LN_FWD(layernorm_fwd_kernel<16>, blocks);
    }
#undef LAUNCH_LN_FWD
    VLP_CHECK_LAUNCH("vlp_layernorm_fwd");
    return VLP_OK;
}

// ---------------------------------------------------------------------------------------------
// backward.  Each wave walks rows (grid-stride) keeping per-column partial sums of dgamma / dbeta in
// registers; partials [nblocks][2][H] go to the workspace and a second kernel reduces them.
// A lane owns NP pieces of 4 columns (piece k = columns 256k + 4*lane .. +3, 8-byte loads): at H = 768 every lane is busy with 12
// columns and the kernel needs ~100 VGPRs, so two 8-wave blocks fit a CU.  (The earlier 8-column chunks left half the lanes idle
// in the second chunk at H = 768 and took 142 VGPRs -- one block per CU, 2 waves per SIMD, one row of prefetch each: 3.4 TB/s.)
// Round 3 tried the half-wave form of the forward here (two rows per wave, 16-byte loads, 48 column sums per lane, values recomputed in
// the second pass): 168 VGPRs + spills, 3 waves per SIMD, no next-row prefetch -- 20.9 us against 14.5 us for this kernel (tools/ln_lab.py).
// A third row in flight (prefetch two rows ahead, 128 VGPRs): 17.4 us -- a wave only sees 2.6 rows, the extra requests just queue up front.
// ---------------------------------------------------------------------------------------------
#define LNB_WAVES 8      // block geometry of the backward kernel
#define LNB_THREADS (64 * LNB_WAVES)
#define LNB_BLOCKS (4096 / LNB_WAVES)

// block-level reduction of the 8 waves' column sums through LDS, one partial row [2H] per block.  sums(k, 0 / 1) = the lane's dgamma / dbeta
// sums of piece k as a value: handed over as references to the kernel's arrays they pass a generic pointer, and the H = 768 kernels
// allocate up to 10 more VGPRs.
template <int NP, bool EXACT, typename Sums>
DEVFN void lnb_block_partials(Sums sums, float* __restrict__ part, int H) {
    extern __shared__ float lnb_sh[];      // [LNB_WAVES][2H]
    const int lane = threadIdx.x & 63;
    float* sg = lnb_sh + (threadIdx.x >> 6) * 2 * H;
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int c = 256 * k + 4 * lane;
        if (EXACT || c < H) {
            *reinterpret_cast<f32x4*>(sg + c) = sums(k, 0);
            *reinterpret_cast<f32x4*>(sg + H + c) = sums(k, 1);
        }
    }
    __syncthreads();
    float* dst = part + (int64_t)blockIdx.x * 2 * H;
    for (int i = threadIdx.x; i < 2 * H; i += LNB_THREADS) {
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < LNB_WAVES; ++w) t += lnb_sh[w * 2 * H + i];
        dst[i] = t;
    }
}

// EXACT: H == 256 NP at compile time (every LayerNorm of the model: 768), no column predicates; otherwise H <= 256 NP and a lane skips the
// pieces at c >= H.  HAS_DXD: the dropped twin dx_drop = dx * mask(out_drop) is written too; HAS_MAP: packed rows, the dropout masks are
// those of the logical row row_map[row].
// Round 6: a loop body the compiler can count.  In the rounds 2 - 5 kernel the next row's loads sat under row-dependent (row + nwaves < M,
// row_map != 0, dxd != 0) branches as well as the lane-dependent (c < H) one, so hipcc's waitcnt pass could not know how many requests are in
// flight at the join and put `s_waitcnt vmcnt(0)` in front of the current row's arithmetic (seen in the ISA: three of them per iteration): the
// "prefetch" was waited for in the iteration that issued it -- one row in flight per wave, not two.  Here every iteration issues exactly the
// same loads (the next row is clamped to M - 1 instead of skipped; the optional operands are template switches), so with EXACT the waits are
// counted and a wave really keeps two rows of HBM traffic in flight.
// LIST (vlp_layernorm_bwd_rows): M entries of `live`; entry m names the row of x / mean / rstd (and, by `lflags`, of dy and dx), < 0 is a pad
// that is skipped.  The row arithmetic is the one of the unlisted kernel: a listed row gets the bits an unlisted launch gives it.
template <int NP, bool EXACT, bool HAS_DXD, bool HAS_MAP, bool LIST = false>
__global__ __launch_bounds__(LNB_THREADS, NP <= 3 ? 4 : (NP == 4 ? 3 : 2)) void layernorm_bwd_kernel(
    const f16* __restrict__ dy, int64_t lddy, const f16* __restrict__ x, int64_t ldx, const f16* __restrict__ gamma,
    const float* __restrict__ mean, const float* __restrict__ rstd, f16* __restrict__ dx, int64_t lddx,
    f16* __restrict__ dxd, int64_t lddxd, float* __restrict__ part, int M, int H_, DropCtx dyd, DropCtx outd, const int32_t* __restrict__ row_map,
    const int32_t* __restrict__ live = nullptr, int lflags = 0) {
    const int H = EXACT ? 256 * NP : H_;
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * LNB_WAVES + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * LNB_WAVES;
    const float invH = 1.f / (float)H;
    float g[NP][4], dg[NP][4], db[NP][4];
#pragma unroll
    for (int k = 0; k < NP; ++k) {
        const int c = 256 * k + 4 * lane;
        f16x4 gv = (f16x4){0, 0, 0, 0};
        if (EXACT || c < H) gv = ld4(gamma + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) { g[k][e] = (float)gv[e]; dg[k][e] = 0.f; db[k][e] = 0.f; }
    }
    // software pipeline: the raw vectors (statistics, logical row) of the NEXT row are requested before the current row is
    // reduced, so two rows of HBM traffic are in flight per wave
    f16x4 xc[NP], dc[NP], xn[NP], dn[NP];
    float mu_c, rs_c, mu_n, rs_n;
    int map_c = 0, map_n = 0;
    int lr_c = 0, lr_n = 0;                // LIST: live[row] of the current / next row
    auto fetch = [&](int row, f16x4 (&X)[NP], f16x4 (&D)[NP], float& m_, float& r_, int& mp_, int& lr_) {
        if constexpr (LIST) {
            lr_ = live[row];
            const int src = max(lr_, 0);       // (a pad entry fetches row 0 and is skipped below)
#pragma unroll
            for (int k = 0; k < NP; ++k) {
                const int c = 256 * k + 4 * lane;
                if (EXACT || c < H) {
                    X[k] = ld4(x + (int64_t)src * ldx + c);
                    D[k] = ld4(dy + (int64_t)((lflags & VLP_ROWS_X) ? src : row) * lddy + c);
                }
            }
            m_ = mean[src];
            r_ = rstd[src];
            if constexpr (HAS_MAP) mp_ = row_map[src];
            return;
        }
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int c = 256 * k + 4 * lane;
            if (EXACT || c < H) {
                X[k] = ld4(x + (int64_t)row * ldx + c);
                D[k] = ld4(dy + (int64_t)row * lddy + c);
            }
        }
        m_ = mean[row];
        r_ = rstd[row];
        if constexpr (HAS_MAP) mp_ = row_map[row];
    };
    // one row: the current registers (xc, dc, statistics) -> dx (+ twin) and the lane's column sums
    auto row_body = [&](int row) {
        const float mu = mu_c, rs = rs_c;
        const int orow = (LIST && (lflags & VLP_ROWS_Y)) ? lr_c : row;
        const uint64_t drow = HAS_MAP ? (uint64_t)(uint32_t)map_c : (uint64_t)(LIST ? lr_c : row);
        const uint32_t rk_dy = dyd.thresh ? drop_rowkey(dyd, drow) : 0u;
        const uint32_t rk_out = outd.thresh ? drop_rowkey(outd, drow) : 0u;
        float xh[NP][4], d[NP][4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int c = 256 * k + 4 * lane;
            if (EXACT || c < H) {
                float m4[4] = {1.f, 1.f, 1.f, 1.f};
                if (dyd.thresh) drop_mult4(dyd, rk_dy, (uint32_t)c, m4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dd = (float)dc[k][e] * m4[e];
                    xh[k][e] = ((float)xc[k][e] - mu) * rs;
                    dg[k][e] += dd * xh[k][e];
                    db[k][e] += dd;
                    d[k][e] = dd * g[k][e];
                    s1 += d[k][e];
                    s2 += d[k][e] * xh[k][e];
                }
            } else {       // (defined values in the pieces a lane skips: left undefined they cost the column-predicated kernels registers, NP = 8 spills)
#pragma unroll
                for (int e = 0; e < 4; ++e) { xh[k][e] = 0.f; d[k][e] = 0.f; }
            }
        }
        s1 = wave_sum(s1) * invH;
        s2 = wave_sum(s2) * invH;
#pragma unroll
        for (int k = 0; k < NP; ++k) {
            const int c = 256 * k + 4 * lane;
            if (EXACT || c < H) {
                f16x4 o, od;
                float m4[4] = {1.f, 1.f, 1.f, 1.f};
                if (HAS_DXD) drop_mult4(outd, rk_out, (uint32_t)c, m4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = rs * (d[k][e] - s1 - xh[k][e] * s2);
                    o[e] = (f16)t;
                    od[e] = (f16)(t * m4[e]);
                }
                st4_out<VLP_SS_LN>(dx + (int64_t)orow * lddx + c, o);
                if (HAS_DXD) st4_out<VLP_SS_LN>(dxd + (int64_t)row * lddxd + c, od);
            }
        }
    };
    if constexpr (LIST) {
        // The listed row live[m] is taken by the wave that walks it in the unlisted launch of the same grid (row % nwaves), in ascending row
        // order (the list is ascending): the lane's column sums, the block partials and so dgamma / dbeta get the unlisted launch's bits --
        // there the rows in between add exact zeros.  Every wave scans the list 64 entries at a time; pads (-1) match nobody.
        for (int base = 0; base < M; base += 64) {
            const int e = base + lane;
            const int lv = e < M ? live[e] : -1;
            unsigned long long mask = __ballot(lv >= 0 && (lv % nwaves) == wave);
            while (mask) {
                const int bit = __ffsll(mask) - 1;
                mask &= mask - 1;
                fetch(base + bit, xc, dc, mu_c, rs_c, map_c, lr_c);
                row_body(base + bit);
            }
        }
    } else {
        if (wave >= M) {                       // (no rows: only the zero partials below)
            mu_c = rs_c = 0.f;
        } else {
            fetch(wave, xc, dc, mu_c, rs_c, map_c, lr_c);
        }
        for (int row = wave; row < M; row += nwaves) {
            fetch(min(row + nwaves, M - 1), xn, dn, mu_n, rs_n, map_n, lr_n);        // ALWAYS (the tail re-reads row M - 1): a countable loop body
            row_body(row);
#pragma unroll
            for (int k = 0; k < NP; ++k) { xc[k] = xn[k]; dc[k] = dn[k]; }
            mu_c = mu_n;
            rs_c = rs_n;
            map_c = map_n;
            lr_c = lr_n;
        }
    }
    lnb_block_partials<NP, EXACT>([&](int k, int b) { return b ? (f32x4){db[k][0], db[k][1], db[k][2], db[k][3]} : (f32x4){dg[k][0], dg[k][1], dg[k][2], dg[k][3]}; },
                                  part, H);
}

// Second stage of the backward and of colsum: dst(i) (+)= sum of column i over the nparts partial rows of width W.  Block = 64 columns x 16
// partial-groups; a group adds its rows p = pg, pg + 16, .. in ascending order, then the 16 LDS words are added in ascending order:
// every caller has this summation order (test_layernorm_bwd_deferred_batched_reduce compares two of them bit for bit).
template <typename DstOf>
DEVFN void reduce_partial_rows(const float* __restrict__ part, int nparts, int W, int beta, DstOf dst_of) {
    __shared__ float sh[16][64];
    const int cl = threadIdx.x & 63, pg = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + cl;
    float s = 0.f;
    if (i < W)
        for (int p = pg; p < nparts; p += 16) s += part[(int64_t)p * W + i];
    sh[pg][cl] = s;
    __syncthreads();
    if (pg == 0 && i < W) {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += sh[k][cl];
        f16* dst = dst_of(i);
        *dst = (f16)(beta ? (float)*dst + t : t);
    }
}

// out[0..H) = dgamma, out[H..2H) = dbeta from part[nparts][2H]
__global__ __launch_bounds__(1024) void ln_bwd_reduce_kernel(const float* __restrict__ part, int nparts, int H, f16* dgamma, f16* dbeta, int beta) {
    reduce_partial_rows(part, nparts, 2 * H, beta, [&](int i) { return i < H ? dgamma + i : dbeta + (i - H); });
}

// blockIdx.y = LayerNorm index: ln_bwd_reduce_kernel on slot y
__global__ __launch_bounds__(1024) void ln_bwd_reduce_batched_kernel(const float* __restrict__ parts, int64_t slot_stride, f16* const* __restrict__ dst,
                                                                     int nparts, int H, int beta) {
    reduce_partial_rows(parts + (int64_t)blockIdx.y * slot_stride, nparts, 2 * H, beta,
                        [&](int i) { return i < H ? dst[2 * blockIdx.y] + i : dst[2 * blockIdx.y + 1] + (i - H); });
}

// row-walking blocks of a backward launch (= partial rows in the workspace); VLP_LNB_BLOCKS lowers it for A/B runs
static int lnb_blocks(int M) {
    static const int cap = env_blocks("VLP_LNB_BLOCKS", LNB_BLOCKS, LNB_BLOCKS);
    const int blocks = cdiv(M, LNB_WAVES);
    if (blocks <= cap) return blocks;
    // every wave the SAME number of rows: with the cap alone a wave walks M / (cap * 8) = 2.6 rows at M = 10 688 -- 61 % of the waves do
    // three, the rest two, and the kernel ends when the three-row waves do.  R = ceil(rows per wave) rows for (almost) all of them:
    // 446 blocks instead of 512 at M = 10 688: 14.8 -> 14.1 us plain, 18.4 -> 17.3 us with the dropped twin (profiles/r04_layernorm_lab.txt)
    const int R = cdiv(M, cap * LNB_WAVES);
    return cdiv(M, R * LNB_WAVES);
}

extern "C" int64_t vlp_layernorm_bwd_workspace_bytes(int32_t H) {
    return (int64_t)LNB_BLOCKS * 2 * H * (int64_t)sizeof(float);
}

template <int NP, bool EXACT, bool HAS_DXD, bool HAS_MAP, bool LIST = false>
static void launch_ln_bwd(const vlp_layernorm_bwd_args* a, int blocks, const DropCtx& dyd, const DropCtx& outd, hipStream_t s, const int32_t* live = nullptr,
                          int lflags = 0) {
    const auto kernel = layernorm_bwd_kernel<NP, EXACT, HAS_DXD, HAS_MAP, LIST>;
    VLP_ONCE_PER_DEVICE((void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LNB_WAVES * 2 * 256 * NP * 4));
    const size_t lnb_smem = (size_t)LNB_WAVES * 2 * a->H * sizeof(float);   // <= 128 KiB at H = 2048
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(LNB_THREADS), lnb_smem, s, (const f16*)a->dy, a->lddy, (const f16*)a->x, a->ldx, (const f16*)a->gamma,
                       a->mean, a->rstd, (f16*)a->dx, a->lddx, (f16*)a->dx_drop, a->lddxd, (float*)a->workspace, a->M, a->H, dyd, outd, a->row_map, live, lflags);
}
template <int NP, bool EXACT, bool LIST = false>
static void launch_ln_bwd(const vlp_layernorm_bwd_args* a, int blocks, const DropCtx& dyd, const DropCtx& outd, hipStream_t s, const int32_t* live = nullptr,
                          int lflags = 0) {
    const bool hd = a->dx_drop != nullptr, hm = a->row_map != nullptr && (dyd.thresh || outd.thresh);
    if (hd && hm) launch_ln_bwd<NP, EXACT, true, true, LIST>(a, blocks, dyd, outd, s, live, lflags);
    else if (hd) launch_ln_bwd<NP, EXACT, true, false, LIST>(a, blocks, dyd, outd, s, live, lflags);
    else if (hm) launch_ln_bwd<NP, EXACT, false, true, LIST>(a, blocks, dyd, outd, s, live, lflags);
    else launch_ln_bwd<NP, EXACT, false, false, LIST>(a, blocks, dyd, outd, s, live, lflags);
}

static int ln_bwd_launch(const vlp_layernorm_bwd_args* a, const int32_t* live, int lflags, int part_M, void* stream) {
    VLP_CHECK_ARG(a->M > 0 && a->H > 0 && a->H % 8 == 0 && a->H <= 2048, "vlp_layernorm_bwd: H=%d must be a multiple of 8 and <= 2048", a->H);
    VLP_CHECK_ARG(a->lddy % 8 == 0 && a->ldx % 8 == 0 && a->lddx % 8 == 0, "vlp_layernorm_bwd: leading dims");
    VLP_CHECK_ARG(((uintptr_t)a->dy | (uintptr_t)a->x | (uintptr_t)a->dx | (uintptr_t)a->gamma) % 16 == 0, "vlp_layernorm_bwd: alignment");
    if (a->dx_drop) VLP_CHECK_ARG(a->lddxd % 8 == 0 && (uintptr_t)a->dx_drop % 16 == 0 && a->out_drop_p > 0.f, "vlp_layernorm_bwd: dx_drop needs out_drop_p > 0");
    const int64_t need = vlp_layernorm_bwd_workspace_bytes(a->H);
    if (!a->workspace || a->workspace_bytes < need) return vlp_set_error(VLP_ERR_WORKSPACE, "vlp_layernorm_bwd: workspace %lld < %lld", (long long)a->workspace_bytes, (long long)need);
    const DropCtx dyd = make_drop(a->dy_drop_p, a->dy_seed, a->dy_stream);
    const DropCtx outd = make_drop(a->out_drop_p, a->out_seed, a->out_stream);
    // listed rows: the grid of the unlisted launch over part_M rows, so that every partial row the deferred reduce reads is written (zeros
    // where a block saw no row) and every listed row is summed by the wave, and in the order, of that launch
    const int blocks = lnb_blocks(live ? part_M : a->M);
    hipStream_t s = (hipStream_t)stream;
    if (live) {
        if (a->H == 768) launch_ln_bwd<3, true, true>(a, blocks, dyd, outd, s, live, lflags);
        else if (a->H <= 768) launch_ln_bwd<3, false, true>(a, blocks, dyd, outd, s, live, lflags);
        else if (a->H <= 1024) launch_ln_bwd<4, false, true>(a, blocks, dyd, outd, s, live, lflags);
        else launch_ln_bwd<8, false, true>(a, blocks, dyd, outd, s, live, lflags);
    }
    else if (a->H == 768) launch_ln_bwd<3, true>(a, blocks, dyd, outd, s);
    else if (a->H <= 768) launch_ln_bwd<3, false>(a, blocks, dyd, outd, s);
    else if (a->H <= 1024) launch_ln_bwd<4, false>(a, blocks, dyd, outd, s);
    else launch_ln_bwd<8, false>(a, blocks, dyd, outd, s);
    VLP_CHECK_LAUNCH("vlp_layernorm_bwd");
    if (a->defer_reduce) return VLP_OK;
    hipLaunchKernelGGL(ln_bwd_reduce_kernel, dim3(cdiv(2 * a->H, 64)), dim3(1024), 0, s, (const float*)a->workspace, blocks, a->H, (f16*)a->dgamma,
                       (f16*)a->dbeta, a->beta);
    VLP_CHECK_LAUNCH("vlp_layernorm_bwd_reduce");
    return VLP_OK;
}

extern "C" int vlp_layernorm_bwd(const vlp_layernorm_bwd_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->dy && a->x && a->gamma && a->mean && a->rstd && a->dx && a->dgamma && a->dbeta, "vlp_layernorm_bwd: null operand");
    VLP_ENTER(a->dy, "vlp_layernorm_bwd");
    return ln_bwd_launch(a, nullptr, 0, 0, stream);
}

extern "C" int vlp_layernorm_bwd_rows(const vlp_layernorm_bwd_args* a, const int32_t* live, int32_t flags, int32_t part_M, void* stream) {
    VLP_CHECK_ARG(a && a->dy && a->x && a->gamma && a->mean && a->rstd && a->dx && a->dgamma && a->dbeta && live, "vlp_layernorm_bwd_rows: null operand");
    VLP_ENTER(a->dy, "vlp_layernorm_bwd_rows");
    VLP_CHECK_ARG((flags & ~(VLP_ROWS_X | VLP_ROWS_Y)) == 0 && part_M > 0, "vlp_layernorm_bwd_rows: bad flags %d / part_M %d", flags, part_M);
    return ln_bwd_launch(a, live, flags, part_M, stream);
}

extern "C" int vlp_layernorm_bwd_reduce_batched(const float* parts, const void* const* dst, int32_t count, int32_t M, int32_t H, int32_t beta, void* stream) {
    VLP_CHECK_ARG(parts && dst && count > 0 && count <= 65535 && M > 0 && H > 0 && H % 8 == 0 && H <= 2048, "vlp_layernorm_bwd_reduce_batched: bad args");
    VLP_ENTER(parts, "vlp_layernorm_bwd_reduce_batched");
    VLP_CHECK_ARG(beta == 0 || beta == 1, "vlp_layernorm_bwd_reduce_batched: beta must be 0 or 1");
    const int blocks = lnb_blocks(M);
    hipLaunchKernelGGL(ln_bwd_reduce_batched_kernel, dim3(cdiv(2 * H, 64), count), dim3(1024), 0, (hipStream_t)stream, parts,
                       (int64_t)LNB_BLOCKS * 2 * H, (f16* const*)dst, blocks, H, beta);
    VLP_CHECK_LAUNCH("vlp_layernorm_bwd_reduce_batched");
    return VLP_OK;
}

// ---------------------------------------------------------------------------------------------
// column sums: out[n] (+)= sum_m A[m,n].  grid (col blocks of 256, row splits); partials -> reduce.
// ---------------------------------------------------------------------------------------------
#define CS_SPLITS 64

__global__ __launch_bounds__(256) void colsum_kernel(const f16* __restrict__ A, int64_t lda, int M, int N, float* __restrict__ part) {
    __shared__ float red[8][256];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 column-chunks x 8 row lanes
    const int c0 = blockIdx.x * 256 + tx * 8;
    const int rows_per = (M + gridDim.y - 1) / gridDim.y;
    const int r0 = blockIdx.y * rows_per, r1 = min(M, r0 + rows_per);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (c0 < N) {
        for (int r = r0 + ty; r < r1; r += 8) {
            f16x8 v = ld8(A + (int64_t)r * lda + c0);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[ty][tx * 8 + e] = acc[e];
    __syncthreads();
    const int c = threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int y = 0; y < 8; ++y) s += red[y][c];
    const int col = blockIdx.x * 256 + c;
    if (col < N) part[(int64_t)blockIdx.y * N + col] = s;
}
__global__ __launch_bounds__(1024) void colsum_reduce_kernel(const float* __restrict__ part, int nparts, int N, f16* out, int beta) {
    reduce_partial_rows(part, nparts, N, beta, [&](int i) { return out + i; });
}

extern "C" int64_t vlp_colsum_workspace_bytes(int32_t M, int32_t N) {
    (void)M;
    return (int64_t)CS_SPLITS * N * (int64_t)sizeof(float);
}
extern "C" int vlp_colsum(const vlp_colsum_args* a, void* stream) {
    VLP_CHECK_ARG(a && a->A && a->out && a->M > 0 && a->N > 0, "vlp_colsum: bad args");
    VLP_ENTER(a->A, "vlp_colsum");
    VLP_CHECK_ARG(a->lda % 8 == 0 && a->lda >= (a->N + 7) / 8 * 8 && (uintptr_t)a->A % 16 == 0, "vlp_colsum: layout (lda must cover roundup8(N))");
    int splits = a->M >= CS_SPLITS * 8 ? CS_SPLITS : (a->M + 7) / 8;
    if (splits < 1) splits = 1;
    const int64_t need = (int64_t)splits * a->N * (int64_t)sizeof(float);
    if (!a->workspace || a->workspace_bytes < need) return vlp_set_error(VLP_ERR_WORKSPACE, "vlp_colsum: workspace %lld < %lld", (long long)a->workspace_bytes, (long long)need);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(colsum_kernel, dim3(cdiv(a->N, 256), splits), dim3(256), 0, s, (const f16*)a->A, a->lda, a->M, a->N, (float*)a->workspace);
    VLP_CHECK_LAUNCH("vlp_colsum");
    hipLaunchKernelGGL(colsum_reduce_kernel, dim3(cdiv(a->N, 64)), dim3(1024), 0, s, (const float*)a->workspace, splits, a->N, (f16*)a->out, a->beta);
    VLP_CHECK_LAUNCH("vlp_colsum_reduce");
    return VLP_OK;
}
