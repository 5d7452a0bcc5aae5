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
#include "cl_rows.h"

namespace {

constexpr int GN_TH = CL_TH;

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

// GroupNorm's per-thread channel constants (w = gamma rstd, b = beta, k1 = s1 / M, k2 = s2 / M of each element's group) with its formulas and
// its clip: what the fused pooling bodies of csrc/cl_rows.h take as their norm, and what gncl_map_kernel sweeps with
struct GNQuad {
    typedef double acc_t;
    GNStat st;
    float w[4], b[4], k1[4], k2[4];
    int n, T;                                               // the clip (the grid's y) and its frames
    __device__ __forceinline__ void load_stats(const float* mean, const float* rstd, int clip, int G, int cpg, int q) {
        n = clip;
        st = gn_load_stats(mean, rstd, n, G, cpg, q);
    }
    __device__ __forceinline__ void load_fwd(const float* gamma, const float* beta, const float* mean, const float* rstd, int clip, int G, int cpg, int q) {
        load_stats(mean, rstd, clip, G, cpg, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            w[e] = (gamma ? gamma[c] : 1.f) * st.is[e];
            b[e] = beta ? beta[c] : 0.f;
        }
    }
    __device__ __forceinline__ void load_bwd(const float* gamma, const float* mean, const float* rstd, const float* sums, int clip, int G, int cpg, int q) {
        load_stats(mean, rstd, clip, G, cpg, q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e, g = c / cpg;
            w[e] = (gamma ? gamma[c] : 1.f) * st.is[e];
            k1[e] = sums[((size_t)n * 2 + 0) * G + g];
            k2[e] = sums[((size_t)n * 2 + 1) * G + g];
        }
    }
    __device__ __forceinline__ float mask(float dP, float P) const { return gn_mask(dP, P); }
    __device__ __forceinline__ float xhat(float x, int e) const { return (x - st.mu[e]) * st.is[e]; }
    __device__ __forceinline__ float dx(float g, float x, int e) const { return gn_dx(g, x, st.mu[e], st.is[e], w[e], k1[e], k2[e]); }
};

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
    GNQuad gn;
    if (MODE == 1) gn.load_stats(mean, rstd, n, G, C / G, q);
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
                    for (int e = 0; e < 4; ++e) { s[e] += (double)ve[e]; t[e] += (double)(ve[e] * gn.xhat(xe[e], e)); }
                }
            }
        }
        cl_put_groups(red, g, q, groups, C, s, t);
    }
    cl_fold_groups(red, groups, C, partial, (size_t)n * gridDim.x + blockIdx.x);
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
    GNQuad gn;
    if (MODE == 0) gn.load_fwd(gamma, beta, mean, rstd, n, G, cpg, q);
    else gn.load_bwd(gamma, mean, rstd, sums, n, G, cpg, q);
    float mx = 0.f;
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = i0; i < total4; i += (size_t)gridDim.x * GN_TH) {
        const float4 v = reinterpret_cast<const float4*>(a)[base + i];
        const float ve[4] = {v.x, v.y, v.z, v.w};
        float o[4];
        if (MODE == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = gn_map(ve[e], gn.st.mu[e], gn.w[e], gn.b[e], relu);
        } else {
            const float4 xv = reinterpret_cast<const float4*>(x)[base + i];
            const float xe[4] = {xv.x, xv.y, xv.z, xv.w};
            float ye[4] = {1.f, 1.f, 1.f, 1.f};
            if (relu) { const float4 yv = reinterpret_cast<const float4*>(y)[base + i]; ye[0] = yv.x; ye[1] = yv.y; ye[2] = yv.z; ye[3] = yv.w; }
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = gn.dx(relu ? gn_mask(ve[e], ye[e]) : ve[e], xe[e], e);
        }
        reinterpret_cast<float4*>(out)[base + i] = make_float4(o[0], o[1], o[2], o[3]);
        if (slot) mx = cl_max4(mx, o);
        if (MODE == 1 && colpart) { cs[0] += (double)o[0]; cs[1] += (double)o[1]; cs[2] += (double)o[2]; cs[3] += (double)o[3]; }
    }
    if (MODE == 1 && colpart) cl_block_colsum(cs, csum, C, colpart + ((size_t)n * gridDim.x + blockIdx.x) * C);
    if (slot) m3t_block_raise_slot(slot, mx, red4);         // (uniform: every thread of the block gets here)
}

// ---- GroupNorm + ReLU + max pooling (k x k, stride k, no padding) as one operator over a clip's T frames [T][H][W][C]: the bodies of
// csrc/cl_rows.h under GNQuad, the clip on the grid's y
struct GNPool { int T, H, W, Ho, Wo, He, We, C, G; };      // He x We = ceil(H / k) x ceil(W / k): edge positions no window covers (odd H, W)
static bool gnpool_geom(int T, int H, int W, int C, int G, int k, GNPool& g) {
    if (T < 1 || H < 1 || W < 1 || (k != 2 && k != 3) || H < k || W < k) return false;
    g.T = T; g.H = H; g.W = W; g.C = C; g.G = G; g.Ho = H / k; g.Wo = W / k; g.He = (H + k - 1) / k; g.We = (W + k - 1) / k;
    return true;
}

// (own text beside bnpool_fwd_kernel's: shared through a function the K = 3 kernel runs 8-10 % longer, NOTEBOOK section 27)
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
        if (slot) mx = cl_max4(mx, best);
    }
    if (slot) m3t_block_raise_slot(slot, mx, red4);
}

// backward sums over a clip's pooled windows: partial[clip][chunk][2][C] = sum g, sum g xhat with g = dP masked by P, taken at the window's winner
template <int K>
__global__ __launch_bounds__(GN_TH) void gnpool_bwd_partial_kernel(const float* __restrict__ dyp, const float* __restrict__ x, const float* __restrict__ yp,
                                                                   const unsigned char* __restrict__ win, const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd, size_t nwin, GNPool g, size_t win_per_chunk,
                                                                   double* __restrict__ partial) {
    const int c4n = g.C >> 2, q = threadIdx.x % c4n, gi = threadIdx.x / c4n;
    GNQuad gn;
    gn.load_stats(mean, rstd, blockIdx.y, g.G, g.C / g.G, q);
    gn.T = g.T;
    cl_normpool_bwd_partial<K>(dyp, x, yp, win, nwin, g, win_per_chunk, partial, gn, q, gi);
}

// dx at full resolution: a thread = one (extended) window x four channels; positions outside the pooled grid (odd H / W) have g = 0
template <int K>
__global__ __launch_bounds__(GN_TH) void gnpool_bwd_dx_kernel(const float* __restrict__ dyp, const float* __restrict__ x, const float* __restrict__ yp,
                                                              const unsigned char* __restrict__ win, const float* __restrict__ gamma,
                                                              const float* __restrict__ mean, const float* __restrict__ rstd,
                                                              const float* __restrict__ sums, float* __restrict__ dx, size_t total4, GNPool g,
                                                              unsigned long long* __restrict__ slot, double* __restrict__ colpart) {
    const int q = (int)(((size_t)blockIdx.x * GN_TH + threadIdx.x) % (size_t)(g.C >> 2));
    GNQuad gn;
    gn.load_bwd(gamma, mean, rstd, sums, blockIdx.y, g.G, g.C / g.G, q);
    gn.T = g.T;
    cl_normpool_bwd_dx<K>(dyp, x, yp, win, dx, total4, g, slot, colpart, gn, q);
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
    if (!cl_ws_ok(ws, ws_bytes, w.bytes)) return M3T_EINVAL;
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
    if (!cl_ws_ok(ws, ws_bytes, w.bytes)) return M3T_EINVAL;
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
    GNPool g;
    if (!gnpool_geom(T, H, W, C, G, k, g)) return M3T_EINVAL;
    const size_t R = (size_t)T * H * W;
    if (!gncl_shape_ok(N, R, C, G) || !al16(x) || !al16(yp) || !al4(win) || !save_mean || !save_rstd) return M3T_EINVAL;
    const GNWs w = gn_ws(ws, N, R, C);
    if (!cl_ws_ok(ws, ws_bytes, w.bytes)) return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int rc = gn_stats(x, N, R, C, G, eps, save_mean, save_rstd, w, s);
    if (rc) return rc;
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
    GNPool g;
    if (!gnpool_geom(T, H, W, C, G, k, g)) return M3T_EINVAL;
    const size_t R = (size_t)T * H * W;
    if (!gncl_shape_ok(N, R, C, G) || !al16(dyp) || !al16(x) || !al16(yp) || !al16(dx) || !al4(win) || !save_mean || !save_rstd)
        return M3T_EINVAL;
    const GNWs w = gn_ws(ws, N, R, C);
    if (!cl_ws_ok(ws, ws_bytes, w.bytes)) return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
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
