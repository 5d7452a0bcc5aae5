// What evaluate.hip and evaluate_expr.hip share: the block reduction, and the valence / arousal body of the per-batch append as
// ONE text, so that m3t_eval_append and m3t_eval_append_mtl give the same bits in `rows` and `part` (same thread-to-frame
// mapping, same fp64 sums, same reduction tree).
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ double block_sum_f64(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// Clip n of a 256-thread workgroup.  rows[n][q][t], q = v_pred, a_pred (, v_gt, a_gt); a frame t >= len is written as 0 and
// its inputs are never loaded.  part[n][k][0..7) = n, sum p, sum g, sum p^2, sum g^2, sum p g, sum (p - g)^2 over the valid
// frames (t < len, |v_gt| <= 1 and |a_gt| <= 1: a NaN label fails the comparison), k = valence, arousal.  Every thread of the
// workgroup calls it (it synchronises when labels are given).
__device__ __forceinline__ void eval_append_va(const float* __restrict__ y, long n, int T, int C, int len,
                                               const float* __restrict__ lv, const float* __restrict__ la,
                                               float* __restrict__ rows, double* __restrict__ part, double* red) {
    const int Q = lv ? 4 : 2;
    const float* yn = y + n * (long)T * C + (C - 2);
    float* rn = rows + n * (long)Q * T;
    double m[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) m[k] = 0.0;
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const bool in = t < len;
        const float pv = in ? yn[(long)t * C] : 0.f, pa = in ? yn[(long)t * C + 1] : 0.f;
        rn[t] = pv;
        rn[T + t] = pa;
        if (lv) {
            const float gv = in ? lv[n * T + t] : 0.f, ga = in ? la[n * T + t] : 0.f;
            rn[2 * T + t] = gv;
            rn[3 * T + t] = ga;
            if (in && fabsf(gv) <= 1.f && fabsf(ga) <= 1.f) {
                const double p0 = pv, g0 = gv, p1 = pa, g1 = ga;
                m[0] += 1.0;
                m[1] += p0; m[2] += g0; m[3] += p0 * p0; m[4] += g0 * g0; m[5] += p0 * g0; m[6] += (p0 - g0) * (p0 - g0);
                m[7] += p1; m[8] += g1; m[9] += p1 * p1; m[10] += g1 * g1; m[11] += p1 * g1; m[12] += (p1 - g1) * (p1 - g1);
            }
        }
    }
    if (!lv) return;
#pragma unroll
    for (int k = 0; k < 13; ++k) m[k] = block_sum_f64(m[k], red);
    if (threadIdx.x == 0) {
        double* pn = part + n * 14;
        pn[0] = m[0];
        pn[7] = m[0];
#pragma unroll
        for (int k = 1; k < 7; ++k) { pn[k] = m[k]; pn[7 + k] = m[6 + k]; }
    }
}

__device__ __forceinline__ int eval_clip_len(long long ln, int T) { return ln < 0 ? 0 : (ln > T ? T : (int)ln); }

}  // namespace
