// Building blocks of the kernels that walk one fp16 logits row of the vocabulary (loss.hip, elementwise.hip, decode.hip): the strided row
// pass, the block reductions and the block arg-max.  Summation orders are part of the callers' results: do not swap one reduction for another.
#pragma once
#include "common.h"

// f(float value, int column) for this thread's elements of columns [first, V) of the row x, in ascending column order.
//   VEC  (16-byte aligned row, first == 0): the 8-element chunks tid, tid + NT, ..., elements 0..7 in order, then the scalar tail from (V >> 3) * 8 + tid;
//   !VEC: columns first + tid, + NT, ...
template <int NT, bool VEC, typename F>
DEVFN void row_visit(const f16* x, int first, int V, F f) {
    if constexpr (VEC) {
        const int nv = V >> 3;
        for (int c = threadIdx.x; c < nv; c += NT) {
            const f16x8 t = ld8(x + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) f((float)t[e], c * 8 + e);
        }
        for (int v = nv * 8 + threadIdx.x; v < V; v += NT) f((float)x[v], v);
    } else {
        for (int v = first + threadIdx.x; v < V; v += NT) f((float)x[v], v);
    }
}

// block of NT threads: wave butterfly first, then waves 0..NT/64-1 serially; sh holds one float per wave and may be reused right after the call.
// (NT is a template parameter: read from blockDim it is a scalar load in the middle of the kernel, a microsecond on a one-row block's critical path.)
template <int NT>
DEVFN float block_reduce_sum(float v, float* sh) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    float r = 0.f;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) r += sh[i];
    return r;
}
template <int NT>
DEVFN float block_reduce_max(float v, float* sh) {
    v = wave_max(v);
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    float r = -INFINITY;
#pragma unroll
    for (int i = 0; i < NT / 64; ++i) r = fmaxf(r, sh[i]);
    return r;
}

// (value, index) candidates: largest value wins, smallest index on ties
DEVFN void argmax_better(float& bv, int& bi, float f, int j) {
    if (f > bv || (f == bv && j < bi)) { bv = f; bi = j; }
}
// block arg-max of 256 candidates; the result is in sv[0] / si[0] for every thread
DEVFN void argmax_block256(float best, int bi, float* sv, int* si) {
    sv[threadIdx.x] = best;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) argmax_better(sv[threadIdx.x], si[threadIdx.x], sv[threadIdx.x + o], si[threadIdx.x + o]);
        __syncthreads();
    }
}
// block arg-max of 1024 candidates: wave butterfly, then the 16 wave results serially; every thread returns with the result in best / bi.
// sv / si [16] must not be written again (by the next call either) before a barrier.
DEVFN void argmax_block1024(float& best, int& bi, float* sv, int* si) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_better(best, bi, __shfl_xor(best, o, 64), __shfl_xor(bi, o, 64));
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    best = sv[0];
    bi = si[0];
#pragma unroll
    for (int j = 1; j < 16; ++j) argmax_better(best, bi, sv[j], si[j]);
}
// this thread's first maximum over its elements of columns [first, V) (ascending columns within a thread: `>` keeps the first); bi = 0x7fffffff: none
template <int NT, bool VEC>
DEVFN void row_first_max(const f16* x, int first, int V, float& best, int& bi) {
    best = -INFINITY;
    bi = 0x7fffffff;
    row_visit<NT, VEC>(x, first, V, [&](float f, int v) {
        if (f > best) { best = f; bi = v; }
    });
}
