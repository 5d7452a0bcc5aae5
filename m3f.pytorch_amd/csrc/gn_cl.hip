// GroupNorm on the channels-last chain of the 3-D VGG-M stems (norm_layer='gn').  Reference: models/backbone.py:63-103,165-271 -- Conv3d ->
// GroupNorm(32, C) -> ReLU (-> MaxPool3d((1, 2, 2))).  Rows x [N][R][C] with R = T H W rows per clip; semantics of F.group_norm on [N, C, T, H, W]:
// one mean and one biased variance per (clip, group) over (C / G) R values, no running statistics, train == eval.
//   * statistics: float4 sweeps with a thread's channel quad fixed (as bncl_partial_kernel), fp64 sums per (clip, chunk, channel) -- a chunk
//     never crosses a clip; a final kernel folds the chunks, then the group's channels, in a fixed order.  No atomics on floats: a rerun is
//     bit-identical.  One launch covers all clips (the clip is the grid's y).
//   * a thread's float4 may straddle two groups (C = 64, G = 32: two channels per group): mean / rstd are looked up per ELEMENT
//   * apply / dx raise the magnitude slot of what they write (m3t_amax_out); the dx pass also leaves the column sums of dx -- under GroupNorm
//     the bias gradient of the convolution in front is not zero by construction
//   * GroupNorm + ReLU + k x k / stride k pooling as ONE operator (k = 2, 3): relu(gn(x)) at full resolution is neither written nor read
#include "common.h"

namespace {

constexpr int GN_TH = 256;

// the per-element map, shared by the plain and the fused kernels: the same bits in both
__device__ __forceinline__ float gn_map(float x, float mu, float w, float b, int relu) {
    const float r = fmaf(x - mu, w, b);
    return relu ? m3t_relu(r) : r;
}
// dx = rstd (gamma g - s1 / M - xhat s2 / M); w = gamma rstd, k1 = s1 / M, k2 = s2 / M
__device__ __forceinline__ float gn_dx(float g, float x, float mu, float is, float w, float k1, float k2) {
    return fmaf(w, g, -is * fmaf((x - mu) * is, k2, k1));
}
// the ReLU's gradient mask as torch's threshold_backward: 0 where y <= 0, dy elsewhere
__device__ __forceinline__ float gn_mask(float dy, float y) { return (y <= 0.f) ? 0.f : dy; }

struct GNStat { float mu[4], is[4]; };
__device__ __forceinline__ GNStat gn_load_stats(const float* __restrict__ mean, const float* __restrict__ rstd, int n, int G, int cpg, int q) {
    GNStat s;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int g = (4 * q + e) / cpg;
        s.mu[e] = mean[(size_t)n * G + g];
        s.is[e] = rstd[(size_t)n * G + g];
    }
    return s;
}

// ---- statistics: partial[clip][chunk][2][C] doubles.  MODE 0: sum x, sum x^2 (both in fp64: a mean that is large against the spread must not
// cost the variance its digits);  MODE 1 (backward): sum g, sum g xhat with g = dy (masked by y if relu)
template <int MODE>
__global__ __launch_bounds__(GN_TH) void gncl_partial_kernel(const float* __restrict__ a, const float* __restrict__ x, const float* __restrict__ y,
                                                             const float* __restrict__ mean, const float* __restrict__ rstd, size_t R, int C, int G,
                                                             size_t rows_per_chunk, int relu, double* __restrict__ partial) {
    extern __shared__ double red[];                         // [2][groups][C]
    const int c4n = C >> 2, groups = GN_TH / c4n;
    const int q = threadIdx.x % c4n, g = threadIdx.x / c4n;
    const int n = blockIdx.y;
    const size_t clip = (size_t)n * R * C;
    const size_t r0 = (size_t)blockIdx.x * rows_per_chunk;
    const size_t r1 = r0 + rows_per_chunk < R ? r0 + rows_per_chunk : R;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, t[4] = {0.0, 0.0, 0.0, 0.0};
    GNStat st;
#pragma unroll
    for (int e = 0; e < 4; ++e) { st.mu[e] = 0.f; st.is[e] = 0.f; }
    if (MODE == 1) st = gn_load_stats(mean, rstd, n, G, C / G, q);
    if (g < groups) {
        for (size_t rb = r0 + g; rb < r1; rb += (size_t)4 * groups) {      // four rows in flight per thread
            float4 av[4], xv4[4], yv4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const size_t r = rb + (size_t)u * groups;
                const bool in = r < r1;
                const size_t o = clip + (in ? r : rb) * C + 4 * q;
                av[u] = *reinterpret_cast<const float4*>(a + o);
                if (!in) av[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (MODE == 1) {
                    xv4[u] = *reinterpret_cast<const float4*>(x + o);
                    if (relu) yv4[u] = *reinterpret_cast<const float4*>(y + o);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                float ve[4] = {av[u].x, av[u].y, av[u].z, av[u].w};
                if (MODE == 0) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) { const double d = (double)ve[e]; s[e] += d; t[e] = fma(d, d, t[e]); }
                } else {
                    const float xe[4] = {xv4[u].x, xv4[u].y, xv4[u].z, xv4[u].w};
                    if (relu) {
                        const float ye[4] = {yv4[u].x, yv4[u].y, yv4[u].z, yv4[u].w};
#pragma unroll
                        for (int e = 0; e < 4; ++e) ve[e] = gn_mask(ve[e], ye[e]);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) { s[e] += (double)ve[e]; t[e] += (double)(ve[e] * ((xe[e] - st.mu[e]) * st.is[e])); }
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { red[(size_t)g * C + 4 * q + e] = s[e]; red[(size_t)(groups + g) * C + 4 * q + e] = t[e]; }
    }
    __syncthreads();
    const size_t pb = ((size_t)n * gridDim.x + blockIdx.x) * 2;
    for (int c = threadIdx.x; c < C; c += GN_TH) {
        double a0 = 0.0, b0 = 0.0;
        for (int k = 0; k < groups; ++k) { a0 += red[(size_t)k * C + c]; b0 += red[(size_t)(groups + k) * C + c]; }      // fixed order
        partial[(pb + 0) * C + c] = a0;
        partial[(pb + 1) * C + c] = b0;
    }
}

// Fold a clip's chunks for the CB channels [c0, c0 + CB) of this block into ch[2][CB]: 64 channels at a time, the chunks in four interleaved
// phases combined in phase order (a fixed order).  CB is a multiple of 64 or the whole C (< 64).
__device__ __forceinline__ void gncl_fold_chunks(const double* __restrict__ partial, int n, int cpc, int C, int c0, int CB,
                                                 double (&red)[2][4][64], double (&ch)[2][1024]) {
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6;
    for (int cb = 0; cb < CB; cb += 64) {
        const int c = c0 + cb + cl;
        double a = 0.0, b = 0.0;
        if (cb + cl < CB && c < C) {
            double a4[4] = {0.0, 0.0, 0.0, 0.0}, b4[4] = {0.0, 0.0, 0.0, 0.0};
            const double* p = partial + (size_t)n * cpc * 2 * C + c;
            int k = ph;
            for (; k + 12 < cpc; k += 16) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    a4[u] += p[((size_t)(k + 4 * u) * 2 + 0) * C];
                    b4[u] += p[((size_t)(k + 4 * u) * 2 + 1) * C];
                }
            }
            for (; k < cpc; k += 4) { a4[0] += p[((size_t)k * 2 + 0) * C]; b4[0] += p[((size_t)k * 2 + 1) * C]; }
            a = (a4[0] + a4[1]) + (a4[2] + a4[3]); b = (b4[0] + b4[1]) + (b4[2] + b4[3]);
        }
        red[0][ph][cl] = a; red[1][ph][cl] = b;
        __syncthreads();
        if (ph == 0 && cb + cl < CB) {
            ch[0][cb + cl] = red[0][0][cl] + red[0][1][cl] + red[0][2][cl] + red[0][3][cl];
            ch[1][cb + cl] = red[1][0][cl] + red[1][1][cl] + red[1][2][cl] + red[1][3][cl];
        }
        __syncthreads();
    }
}

// grid (C / CB, N): mean and rstd = 1 / sqrt(max(var, 0) + eps) of the groups inside the block's channels
__global__ __launch_bounds__(GN_TH) void gncl_stats_final_kernel(const double* __restrict__ partial, int cpc, double M, int C, int G, int CB, float eps,
                                                                 float* __restrict__ mean, float* __restrict__ rstd) {
    __shared__ double red[2][4][64];
    __shared__ double ch[2][1024];
    const int n = blockIdx.y, c0 = blockIdx.x * CB, cpg = C / G;
    gncl_fold_chunks(partial, n, cpc, C, c0, CB, red, ch);
    for (int t = threadIdx.x; t < CB / cpg; t += GN_TH) {
        double s = 0.0, ss = 0.0;
        for (int j = 0; j < cpg; ++j) { s += ch[0][t * cpg + j]; ss += ch[1][t * cpg + j]; }      // the group's channels in order
        const double mu = s / M;
        double var = ss / M - mu * mu;
        if (var < 0.0) var = 0.0;                          // (a NaN stays a NaN)
        const int g = c0 / cpg + t;
        mean[(size_t)n * G + g] = (float)mu;
        rstd[(size_t)n * G + g] = (float)(1.0 / sqrt(var + (double)eps));
    }
}

// grid (C / CB, N): chansum[n][2][C] = the clip's sums of g and g xhat per channel; sums[n][2][G] = s1 / M, s2 / M with s1 = sum gamma_c g,
// s2 = sum gamma_c g xhat over the group
__global__ __launch_bounds__(GN_TH) void gncl_bwd_final_kernel(const double* __restrict__ partial, int cpc, double M, int C, int G, int CB,
                                                               const float* __restrict__ gamma, double* __restrict__ chansum,
                                                               float* __restrict__ sums) {
    __shared__ double red[2][4][64];
    __shared__ double ch[2][1024];
    const int n = blockIdx.y, c0 = blockIdx.x * CB, cpg = C / G;
    gncl_fold_chunks(partial, n, cpc, C, c0, CB, red, ch);
    for (int c = threadIdx.x; c < CB; c += GN_TH) {
        chansum[((size_t)n * 2 + 0) * C + c0 + c] = ch[0][c];
        chansum[((size_t)n * 2 + 1) * C + c0 + c] = ch[1][c];
    }
    for (int t = threadIdx.x; t < CB / cpg; t += GN_TH) {
        double s1 = 0.0, s2 = 0.0;
        for (int j = 0; j < cpg; ++j) {
            const double w = gamma ? (double)gamma[c0 + t * cpg + j] : 1.0;
            s1 += w * ch[0][t * cpg + j]; s2 += w * ch[1][t * cpg + j];
        }
        const int g = c0 / cpg + t;
        sums[((size_t)n * 2 + 0) * G + g] = (float)(s1 / M);
        sums[((size_t)n * 2 + 1) * G + g] = (float)(s2 / M);
    }
}

// dgamma_c = sum_n sum g xhat, dbeta_c = sum_n sum g: the clips in order
__global__ __launch_bounds__(GN_TH) void gncl_dparam_kernel(const double* __restrict__ chansum, int N, int C, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta) {
    const int c = blockIdx.x * GN_TH + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, t = 0.0;
    for (int n = 0; n < N; ++n) { s += chansum[((size_t)n * 2 + 0) * C + c]; t += chansum[((size_t)n * 2 + 1) * C + c]; }
    if (dbeta) dbeta[c] = (float)s;
    if (dgamma) dgamma[c] = (float)t;
}

// the dx pass's column sums: a thread's four channels are fixed, its sums run in fp64; block partial [C] in thread order
__device__ __forceinline__ void gncl_block_colsum(const double (&cs)[4], double* csum, int C, double* __restrict__ colpart_row) {
    const int c4n = C >> 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) csum[threadIdx.x * 4 + e] = cs[e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += GN_TH) {
        double t = 0.0;
        for (int th = c >> 2; th < GN_TH; th += c4n) t += csum[th * 4 + (c & 3)];      // (a block starts at quad 0: C / 4 divides 256)
        colpart_row[c] = t;
    }
    __syncthreads();
}

// out[c] = sum over the blocks' partials, in block order
__global__ __launch_bounds__(256) void gncl_colsum_final_kernel(const double* __restrict__ colpart, int nblocks, int C, float* __restrict__ out) {
    __shared__ double red[4][64];
    const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
    double t = 0.0;
    if (c < C) {
        double t4[4] = {0.0, 0.0, 0.0, 0.0};
        int k = ph;
        for (; k + 12 < nblocks; k += 16) {
#pragma unroll
            for (int u = 0; u < 4; ++u) t4[u] += colpart[(size_t)(k + 4 * u) * C + c];
        }
        for (; k < nblocks; k += 4) t4[0] += colpart[(size_t)k * C + c];
        t = (t4[0] + t4[1]) + (t4[2] + t4[3]);
    }
    red[ph][cl] = t;
    __syncthreads();
    if (ph == 0 && c < C) out[c] = (float)(red[0][cl] + red[1][cl] + red[2][cl] + red[3][cl]);
}

// apply (+ReLU) / dx.  grid (blocks per clip, N); total4 = R C / 4 per clip; the stride (blocks x 256) is a multiple of C / 4
template <int MODE>
__global__ __launch_bounds__(GN_TH) void gncl_map_kernel(const float* __restrict__ a, const float* __restrict__ x, const float* __restrict__ y,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ sums, float* __restrict__ out, size_t total4, int C, int G,
                                                         int relu, unsigned long long* __restrict__ slot, double* __restrict__ colpart) {
    __shared__ float red4[4];
    __shared__ double csum[GN_TH * 4];
    const int c4n = C >> 2, cpg = C / G, n = blockIdx.y;
    const size_t i0 = (size_t)blockIdx.x * GN_TH + threadIdx.x;
    const int q = (int)(i0 % (size_t)c4n);
    const size_t base = (size_t)n * total4;
    const GNStat st = gn_load_stats(mean, rstd, n, G, cpg, q);
    float w[4], b[4], k1[4], k2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e, g = c / cpg;
        w[e] = (gamma ? gamma[c] : 1.f) * st.is[e];
        b[e] = (MODE == 0 && beta) ? beta[c] : 0.f;
        k1[e] = MODE == 1 ? sums[((size_t)n * 2 + 0) * G + g] : 0.f;
        k2[e] = MODE == 1 ? sums[((size_t)n * 2 + 1) * G + g] : 0.f;
    }
    float mx = 0.f;
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = i0; i < total4; i += (size_t)gridDim.x * GN_TH) {
        const float4 v = reinterpret_cast<const float4*>(a)[base + i];
        const float ve[4] = {v.x, v.y, v.z, v.w};
        float o[4];
        if (MODE == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = gn_map(ve[e], st.mu[e], w[e], b[e], relu);
        } else {
            const float4 xv = reinterpret_cast<const float4*>(x)[base + i];
            const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
            float ye[4] = {1.f, 1.f, 1.f, 1.f};
            if (relu) { const float4 yv = reinterpret_cast<const float4*>(y)[base + i]; ye[0] = yv.x; ye[1] = yv.y; ye[2] = yv.z; ye[3] = yv.w; }
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = gn_dx(relu ? gn_mask(ve[e], ye[e]) : ve[e], xe[e], st.mu[e], st.is[e], w[e], k1[e], k2[e]);
        }
        reinterpret_cast<float4*>(out)[base + i] = make_float4(o[0], o[1], o[2], o[3]);
        if (slot) mx = fmaxf(fmaxf(mx, fmaxf(m3t_fin_abs(o[0]), m3t_fin_abs(o[1]))), fmaxf(m3t_fin_abs(o[2]), m3t_fin_abs(o[3])));
        if (MODE == 1 && colpart) { cs[0] += (double)o[0]; cs[1] += (double)o[1]; cs[2] += (double)o[2]; cs[3] += (double)o[3]; }
    }
    if (MODE == 1 && colpart) gncl_block_colsum(cs, csum, C, colpart + ((size_t)n * gridDim.x + blockIdx.x) * C);
    if (slot) m3t_block_raise_slot(slot, mx, red4);         // (uniform: every thread of the block gets here)
}

// ---- GroupNorm + ReLU + max pooling (k x k, stride k, no padding) as one operator over a clip's T frames [T][H][W][C]
struct GNPool { int T, H, W, Ho, Wo, He, We, C, G; };      // He x We = ceil(H / k) x ceil(W / k): edge positions no window covers (odd H, W)

template <int K>
__global__ __launch_bounds__(GN_TH) void gnpool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd, float* __restrict__ yp,
                                                           unsigned char* __restrict__ win, size_t total4, GNPool g,
                                                           unsigned long long* __restrict__ slot) {
    __shared__ float red4[4];
    const int c4n = g.C >> 2, n = blockIdx.y;
    const size_t i0 = (size_t)blockIdx.x * GN_TH + threadIdx.x;
    const int q = (int)(i0 % (size_t)c4n);
    const GNStat st = gn_load_stats(mean, rstd, n, g.G, g.C / g.G, q);
    float w[4], b[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e;
        w[e] = (gamma ? gamma[c] : 1.f) * st.is[e];
        b[e] = beta ? beta[c] : 0.f;
    }
    const size_t p0 = (size_t)n * g.T, obase = (size_t)n * total4;
    float mx = 0.f;
    for (size_t i = i0; i < total4; i += (size_t)gridDim.x * GN_TH) {
        size_t r = i / (size_t)c4n;
        const int wo = (int)(r % (size_t)g.Wo); r /= (size_t)g.Wo;
        const int ho = (int)(r % (size_t)g.Ho);
        const size_t p = p0 + r / (size_t)g.Ho;
        float4 v[K * K];
#pragma unroll
        for (int dh = 0; dh < K; ++dh)
#pragma unroll
            for (int dw = 0; dw < K; ++dw)
                v[dh * K + dw] = *reinterpret_cast<const float4*>(x + ((p * g.H + (size_t)(ho * K + dh)) * g.W + (size_t)(wo * K + dw)) * (size_t)g.C + 4 * q);
        float best[4];
        int bi[4] = {0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < K * K; ++t) {
            const float ve[4] = {v[t].x, v[t].y, v[t].z, v[t].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = gn_map(ve[e], st.mu[e], w[e], b[e], 1);         // (NaN stays NaN; the pooling lets it win)
                if (t == 0 || m3t_nan_gt(y, best[e])) { best[e] = y; bi[e] = t; }
            }
        }
        reinterpret_cast<float4*>(yp)[obase + i] = make_float4(best[0], best[1], best[2], best[3]);
        reinterpret_cast<uchar4*>(win)[obase + i] = make_uchar4((unsigned char)bi[0], (unsigned char)bi[1], (unsigned char)bi[2], (unsigned char)bi[3]);
        if (slot) mx = fmaxf(fmaxf(mx, fmaxf(m3t_fin_abs(best[0]), m3t_fin_abs(best[1]))), fmaxf(m3t_fin_abs(best[2]), m3t_fin_abs(best[3])));
    }
    if (slot) m3t_block_raise_slot(slot, mx, red4);
}

// backward sums over a clip's pooled windows: partial[clip][chunk][2][C] = sum g, sum g xhat with g = dP masked by P, taken at the window's winner
template <int K>
__global__ __launch_bounds__(GN_TH) void gnpool_bwd_partial_kernel(const float* __restrict__ dyp, const float* __restrict__ x, const float* __restrict__ yp,
                                                                   const unsigned char* __restrict__ win, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd, size_t nwin, GNPool g, size_t win_per_chunk,
                                                                   double* __restrict__ partial) {
    extern __shared__ double red[];
    const int C = g.C, c4n = C >> 2, groups = GN_TH / c4n, n = blockIdx.y;
    const int q = threadIdx.x % c4n, gi = threadIdx.x / c4n;
    const size_t r0 = (size_t)blockIdx.x * win_per_chunk;
    const size_t r1 = r0 + win_per_chunk < nwin ? r0 + win_per_chunk : nwin;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, t[4] = {0.0, 0.0, 0.0, 0.0};
    const GNStat st = gn_load_stats(mean, rstd, n, g.G, C / g.G, q);
    const size_t p0 = (size_t)n * g.T;
    if (gi < groups) {
        for (size_t r = r0 + gi; r < r1; r += groups) {
            size_t rr = r;
            const int wo = (int)(rr % (size_t)g.Wo); rr /= (size_t)g.Wo;
            const int ho = (int)(rr % (size_t)g.Ho);
            const size_t p = p0 + rr / (size_t)g.Ho;
            const size_t o = ((size_t)n * nwin + r) * (size_t)c4n + q;
            const float4 d = reinterpret_cast<const float4*>(dyp)[o];
            const float4 pv = reinterpret_cast<const float4*>(yp)[o];
            const uchar4 wb = reinterpret_cast<const uchar4*>(win)[o];
            const float de[4] = {d.x, d.y, d.z, d.w}, pe[4] = {pv.x, pv.y, pv.z, pv.w};
            const int we[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gq = gn_mask(de[e], pe[e]);
                const int wi = we[e] < K * K ? we[e] : 0;                      // (a byte this library did not write must not index outside the window)
                const int dh = wi / K, dw = wi - dh * K;
                const float xv = x[((p * g.H + (size_t)(ho * K + dh)) * g.W + (size_t)(wo * K + dw)) * (size_t)C + 4 * q + e];
                s[e] += (double)gq;
                t[e] += (double)(gq * ((xv - st.mu[e]) * st.is[e]));
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { red[(size_t)gi * C + 4 * q + e] = s[e]; red[(size_t)(groups + gi) * C + 4 * q + e] = t[e]; }
    }
    __syncthreads();
    const size_t pb = ((size_t)n * gridDim.x + blockIdx.x) * 2;
    for (int c = threadIdx.x; c < C; c += GN_TH) {
        double a0 = 0.0, b0 = 0.0;
        for (int k = 0; k < groups; ++k) { a0 += red[(size_t)k * C + c]; b0 += red[(size_t)(groups + k) * C + c]; }
        partial[(pb + 0) * C + c] = a0;
        partial[(pb + 1) * C + c] = b0;
    }
}

// dx at full resolution: a thread = one (extended) window x four channels; positions outside the pooled grid (odd H / W) have g = 0
template <int K>
__global__ __launch_bounds__(GN_TH) void gnpool_bwd_dx_kernel(const float* __restrict__ dyp, const float* __restrict__ x, const float* __restrict__ yp,
                                                              const unsigned char* __restrict__ win, const float* __restrict__ gamma,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ sums, float* __restrict__ dx, size_t total4, GNPool g,
                                                              unsigned long long* __restrict__ slot, double* __restrict__ colpart) {
    __shared__ float red4[4];
    __shared__ double csum[GN_TH * 4];
    const int C = g.C, c4n = C >> 2, cpg = C / g.G, n = blockIdx.y;
    const size_t i0 = (size_t)blockIdx.x * GN_TH + threadIdx.x;
    const int q = (int)(i0 % (size_t)c4n);
    const GNStat st = gn_load_stats(mean, rstd, n, g.G, cpg, q);
    float w[4], k1[4], k2[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int c = 4 * q + e, gr = c / cpg;
        w[e] = (gamma ? gamma[c] : 1.f) * st.is[e];
        k1[e] = sums[((size_t)n * 2 + 0) * g.G + gr];
        k2[e] = sums[((size_t)n * 2 + 1) * g.G + gr];
    }
    const size_t p0 = (size_t)n * g.T;
    float mx = 0.f;
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = i0; i < total4; i += (size_t)gridDim.x * GN_TH) {
        size_t r = i / (size_t)c4n;
        const int we_ = (int)(r % (size_t)g.We); r /= (size_t)g.We;
        const int he = (int)(r % (size_t)g.He);
        const size_t p = p0 + r / (size_t)g.He;
        const bool pooled = he < g.Ho && we_ < g.Wo;
        float de[4] = {0.f, 0.f, 0.f, 0.f};
        int wi[4] = {-1, -1, -1, -1};
        if (pooled) {
            const size_t o = ((p * g.Ho + he) * g.Wo + we_) * (size_t)c4n + q;
            const float4 d = reinterpret_cast<const float4*>(dyp)[o];
            const float4 pv = reinterpret_cast<const float4*>(yp)[o];
            const uchar4 wb = reinterpret_cast<const uchar4*>(win)[o];
            de[0] = gn_mask(d.x, pv.x); de[1] = gn_mask(d.y, pv.y); de[2] = gn_mask(d.z, pv.z); de[3] = gn_mask(d.w, pv.w);
            wi[0] = wb.x; wi[1] = wb.y; wi[2] = wb.z; wi[3] = wb.w;
        }
#pragma unroll
        for (int dh = 0; dh < K; ++dh) {
            const int h = he * K + dh;
            if (h >= g.H) continue;
#pragma unroll
            for (int dw = 0; dw < K; ++dw) {
                const int ww = we_ * K + dw;
                if (ww >= g.W) continue;
                const size_t xo = ((p * g.H + h) * g.W + ww) * (size_t)C + 4 * q;
                const float4 xv = *reinterpret_cast<const float4*>(x + xo);
                const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e] = gn_dx((wi[e] == dh * K + dw) ? de[e] : 0.f, xe[e], st.mu[e], st.is[e], w[e], k1[e], k2[e]);
                *reinterpret_cast<float4*>(dx + xo) = make_float4(o[0], o[1], o[2], o[3]);
                if (slot) mx = fmaxf(fmaxf(mx, fmaxf(m3t_fin_abs(o[0]), m3t_fin_abs(o[1]))), fmaxf(m3t_fin_abs(o[2]), m3t_fin_abs(o[3])));
                if (colpart) { cs[0] += (double)o[0]; cs[1] += (double)o[1]; cs[2] += (double)o[2]; cs[3] += (double)o[3]; }
            }
        }
    }
    if (colpart) gncl_block_colsum(cs, csum, C, colpart + ((size_t)n * gridDim.x + blockIdx.x) * C);
    if (slot) m3t_block_raise_slot(slot, mx, red4);
}

// chunks / blocks per clip: about 256 rows a chunk and 16 float4 a thread, at most ~1024 chunks and ~2048 blocks over all clips
static int gn_chunks_per_clip(int N, size_t rows) {
    const size_t c = (rows + 255) / 256, cap = N >= 1024 ? 1 : (size_t)(1024 / N);
    return (int)(c < 1 ? 1 : (c > cap ? cap : c));
}
static int gn_blocks_per_clip(int N, size_t total4) {
    const size_t b = (total4 + (size_t)GN_TH * 16 - 1) / ((size_t)GN_TH * 16), cap = N >= 2048 ? 1 : (size_t)(2048 / N);
    return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
static int gn_cb(int C, int G) { const int cpg = C / G; return C < 64 ? C : (cpg > 64 ? cpg : 64); }      // channels per final block: whole groups

static bool gncl_shape_ok(int N, size_t R, int C, int G) {
    return C > 0 && C % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0 && G > 0 && C % G == 0 && N >= 1 && N <= 65535 && R >= 1;
}
static bool al16(const void* p) { return p && ((uintptr_t)p % 16) == 0; }

// workspace: fp64 chunk partials [N][chunks][2][C] | chansum [N][2][C] fp64 | sums [N][2][G <= C] | the dx pass's block partials [N][blocks][C] fp64
struct GNWs { double* partial; double* chansum; float* sums; double* colpart; size_t bytes; };
static GNWs gn_ws(void* ws, int N, size_t R, int C) {
    GNWs w;
    const size_t n_part = (size_t)N * gn_chunks_per_clip(N, R) * 2 * C, n_ch = (size_t)N * 2 * C;
    const size_t n_sums = ((size_t)N * 2 * C + 1) / 2 * 2;                   // (floats; even: what follows stays 8-B aligned)
    const size_t n_col = (size_t)N * gn_blocks_per_clip(N, R * (size_t)(C / 4)) * C;
    w.partial = reinterpret_cast<double*>(ws);
    w.chansum = w.partial + n_part;
    w.sums = reinterpret_cast<float*>(w.chansum + n_ch);
    w.colpart = reinterpret_cast<double*>(w.sums + n_sums);
    w.bytes = (n_part + n_ch + n_col) * sizeof(double) + n_sums * sizeof(float);
    return w;
}

static int gn_stats(const float* x, int N, size_t R, int C, int G, float eps, float* save_mean, float* save_rstd, const GNWs& w, hipStream_t s) {
    const int cpc = gn_chunks_per_clip(N, R), groups = GN_TH / (C / 4), CB = gn_cb(C, G);
    const size_t rpc = (R + cpc - 1) / cpc;
    gncl_partial_kernel<0><<<dim3(cpc, N), GN_TH, (size_t)2 * groups * C * sizeof(double), s>>>(x, nullptr, nullptr, nullptr, nullptr, R, C, G, rpc, 0,
                                                                                               w.partial);
    M3T_LAUNCH_CHECK();
    gncl_stats_final_kernel<<<dim3(C / CB, N), GN_TH, 0, s>>>(w.partial, cpc, (double)(C / G) * (double)R, C, G, CB, eps, save_mean, save_rstd);
    M3T_LAUNCH_CHECK();
    return 0;
}

static int gn_bwd_tail(int N, int C, float* dgamma, float* dbeta, float* dx_colsum, int nblk, const GNWs& w, hipStream_t s) {
    if (dgamma || dbeta) {
        gncl_dparam_kernel<<<cdiv(C, GN_TH), GN_TH, 0, s>>>(w.chansum, N, C, dgamma, dbeta);
        M3T_LAUNCH_CHECK();
    }
    if (dx_colsum) {
        gncl_colsum_final_kernel<<<cdiv(C, 64), 256, 0, s>>>(w.colpart, nblk, C, dx_colsum);
        M3T_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

extern "C" size_t m3t_gn_cl_ws_bytes(int N, size_t R, int C) {
    if (N < 1 || N > 65535 || R < 1 || C < 4 || C % 4 != 0) return 0;
    return gn_ws(nullptr, N, R, C).bytes;
}

extern "C" int m3t_gn_cl_fwd(const float* x, int N, size_t R, int C, int G, const float* gamma, const float* beta, float eps, int relu, float* y,
                             float* save_mean, float* save_rstd, float* ws, size_t ws_bytes, void* stream) {
    unsigned long long* slot = m3t_take_amax_out();
    if (!gncl_shape_ok(N, R, C, G) || !al16(x) || !al16(y) || !save_mean || !save_rstd) return M3T_EINVAL;
    const GNWs w = gn_ws(ws, N, R, C);
    if (!ws || ws_bytes < w.bytes || ((uintptr_t)ws % 8) != 0) return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int rc = gn_stats(x, N, R, C, G, eps, save_mean, save_rstd, w, s);
    if (rc) return rc;
    const size_t total4 = R * (size_t)(C / 4);
    gncl_map_kernel<0><<<dim3(gn_blocks_per_clip(N, total4), N), GN_TH, 0, s>>>(x, nullptr, nullptr, gamma, beta, save_mean, save_rstd, nullptr, y, total4,
                                                                                C, G, relu, slot, nullptr);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_gn_cl_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* save_mean, const float* save_rstd,
                             int N, size_t R, int C, int G, int relu, float* dx, float* dgamma, float* dbeta, float* dx_colsum, float* ws,
                             size_t ws_bytes, void* stream) {
    unsigned long long* slot = m3t_take_amax_out();
    if (!gncl_shape_ok(N, R, C, G) || !al16(dy) || !al16(x) || !al16(dx) || !save_mean || !save_rstd) return M3T_EINVAL;
    if (relu && !al16(y)) return M3T_EINVAL;
    const GNWs w = gn_ws(ws, N, R, C);
    if (!ws || ws_bytes < w.bytes || ((uintptr_t)ws % 8) != 0) return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int cpc = gn_chunks_per_clip(N, R), groups = GN_TH / (C / 4), CB = gn_cb(C, G);
    const size_t rpc = (R + cpc - 1) / cpc;
    gncl_partial_kernel<1><<<dim3(cpc, N), GN_TH, (size_t)2 * groups * C * sizeof(double), s>>>(dy, x, y, save_mean, save_rstd, R, C, G, rpc, relu,
                                                                                               w.partial);
    M3T_LAUNCH_CHECK();
    gncl_bwd_final_kernel<<<dim3(C / CB, N), GN_TH, 0, s>>>(w.partial, cpc, (double)(C / G) * (double)R, C, G, CB, gamma, w.chansum, w.sums);
    M3T_LAUNCH_CHECK();
    const size_t total4 = R * (size_t)(C / 4);
    const int bpc = gn_blocks_per_clip(N, total4);
    gncl_map_kernel<1><<<dim3(bpc, N), GN_TH, 0, s>>>(dy, x, y, gamma, nullptr, save_mean, save_rstd, w.sums, dx, total4, C, G, relu, slot,
                                                      dx_colsum ? w.colpart : nullptr);
    M3T_LAUNCH_CHECK();
    return gn_bwd_tail(N, C, dgamma, dbeta, dx_colsum, N * bpc, w, s);
}

// GroupNorm + ReLU + max pooling with a k x k window, stride k, no padding (k = 2 or 3) as ONE operator over N clips of T channels-last frames
// x [N T][H][W][C]: forward writes only the pooled frames yp [N T][H / k][W / k][C] and the winner bytes; backward takes d(yp) and writes dx at full
// resolution.  Statistics (over ALL positions, covered by a window or not), ws, slots and dx_colsum as m3t_gn_cl_fwd / _bwd with R = T H W.
extern "C" int m3t_gn_pool_cl_fwd(const float* x, int N, int T, int H, int W, int C, int G, int k, const float* gamma, const float* beta, float eps,
                                  float* yp, unsigned char* win, float* save_mean, float* save_rstd, float* ws, size_t ws_bytes, void* stream) {
    unsigned long long* slot = m3t_take_amax_out();
    if (T < 1 || H < 1 || W < 1 || (k != 2 && k != 3) || H < k || W < k) return M3T_EINVAL;
    const size_t R = (size_t)T * H * W;
    if (!gncl_shape_ok(N, R, C, G) || !al16(x) || !al16(yp) || !win || ((uintptr_t)win % 4) != 0 || !save_mean || !save_rstd) return M3T_EINVAL;
    const GNWs w = gn_ws(ws, N, R, C);
    if (!ws || ws_bytes < w.bytes || ((uintptr_t)ws % 8) != 0) return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int rc = gn_stats(x, N, R, C, G, eps, save_mean, save_rstd, w, s);
    if (rc) return rc;
    GNPool g;
    g.T = T; g.H = H; g.W = W; g.C = C; g.G = G; g.Ho = H / k; g.Wo = W / k; g.He = (H + k - 1) / k; g.We = (W + k - 1) / k;
    const size_t total4 = (size_t)T * g.Ho * g.Wo * (size_t)(C / 4);
    const dim3 grid(gn_blocks_per_clip(N, total4), N);
    if (k == 2) gnpool_fwd_kernel<2><<<grid, GN_TH, 0, s>>>(x, gamma, beta, save_mean, save_rstd, yp, win, total4, g, slot);
    else gnpool_fwd_kernel<3><<<grid, GN_TH, 0, s>>>(x, gamma, beta, save_mean, save_rstd, yp, win, total4, g, slot);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_gn_pool_cl_bwd(const float* dyp, const float* x, const float* yp, const unsigned char* win, const float* gamma,
                                  const float* save_mean, const float* save_rstd, int N, int T, int H, int W, int C, int G, int k, float* dx,
                                  float* dgamma, float* dbeta, float* dx_colsum, float* ws, size_t ws_bytes, void* stream) {
    unsigned long long* slot = m3t_take_amax_out();
    if (T < 1 || H < 1 || W < 1 || (k != 2 && k != 3) || H < k || W < k) return M3T_EINVAL;
    const size_t R = (size_t)T * H * W;
    if (!gncl_shape_ok(N, R, C, G) || !al16(dyp) || !al16(x) || !al16(yp) || !al16(dx) || !win || ((uintptr_t)win % 4) != 0 || !save_mean || !save_rstd)
        return M3T_EINVAL;
    const GNWs w = gn_ws(ws, N, R, C);
    if (!ws || ws_bytes < w.bytes || ((uintptr_t)ws % 8) != 0) return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    GNPool g;
    g.T = T; g.H = H; g.W = W; g.C = C; g.G = G; g.Ho = H / k; g.Wo = W / k; g.He = (H + k - 1) / k; g.We = (W + k - 1) / k;
    const size_t nwin = (size_t)T * g.Ho * g.Wo;
    const int cpc = gn_chunks_per_clip(N, nwin), groups = GN_TH / (C / 4), CB = gn_cb(C, G);      // (<= the chunks of R rows: ws covers them)
    const size_t wpc = (nwin + cpc - 1) / cpc;
    const size_t shm = (size_t)2 * groups * C * sizeof(double);
    if (k == 2) gnpool_bwd_partial_kernel<2><<<dim3(cpc, N), GN_TH, shm, s>>>(dyp, x, yp, win, save_mean, save_rstd, nwin, g, wpc, w.partial);
    else gnpool_bwd_partial_kernel<3><<<dim3(cpc, N), GN_TH, shm, s>>>(dyp, x, yp, win, save_mean, save_rstd, nwin, g, wpc, w.partial);
    M3T_LAUNCH_CHECK();
    gncl_bwd_final_kernel<<<dim3(C / CB, N), GN_TH, 0, s>>>(w.partial, cpc, (double)(C / G) * (double)R, C, G, CB, gamma, w.chansum, w.sums);
    M3T_LAUNCH_CHECK();
    const size_t total4 = (size_t)T * g.He * g.We * (size_t)(C / 4);
    const int bpc = gn_blocks_per_clip(N, total4);                                  // (<= the blocks of R rows: ws covers them)
    double* colpart = dx_colsum ? w.colpart : nullptr;
    if (k == 2) gnpool_bwd_dx_kernel<2><<<dim3(bpc, N), GN_TH, 0, s>>>(dyp, x, yp, win, gamma, save_mean, save_rstd, w.sums, dx, total4, g, slot, colpart);
    else gnpool_bwd_dx_kernel<3><<<dim3(bpc, N), GN_TH, 0, s>>>(dyp, x, yp, win, gamma, save_mean, save_rstd, w.sums, dx, total4, g, slot, colpart);
    M3T_LAUNCH_CHECK();
    return gn_bwd_tail(N, C, dgamma, dbeta, dx_colsum, N * bpc, w, s);
}
