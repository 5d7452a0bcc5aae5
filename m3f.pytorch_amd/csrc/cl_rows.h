// What the channels-last row operators share (csrc/stem_cl.hip, csrc/gn_cl.hip, csrc/vggface.hip): a thread owns one channel quad (four
// channels, one float4) for a whole sweep; a 256-thread block holds 256 / (C / 4) row groups side by side.  Each piece below stands once.
// What differs between the families on purpose stays a template argument or stays in its file, and nothing here chooses between them:
// BatchNorm's (v - mu) w + b against GroupNorm's fmaf, fp32 pre-sums of four rows against fp64 from the first add, float against double
// block partials, P > 0 ? d : 0 against P <= 0 ? 0 : d (they differ on NaN).
#pragma once
#include "common.h"

constexpr int CL_TH = 256;

// ---- host: the pointer rules of every entry point
static inline bool al16(const void* p) { return p && ((uintptr_t)p % 16) == 0; }                  // a tensor swept in float4
static inline bool al16_opt(const void* p) { return ((uintptr_t)p % 16) == 0; }                   // an optional one: null passes
static inline bool al4(const void* p) { return p && ((uintptr_t)p % 4) == 0; }                    // winner bytes, swept in uchar4
static inline bool cl_ws_ok(const void* ws, size_t ws_bytes, size_t need) { return ws && ws_bytes >= need && ((uintptr_t)ws % 8) == 0; }

// ---- the magnitude of a written quad: inf / NaN do not count (m3t_fin_abs)
static __device__ __forceinline__ float cl_max4(float mx, const float (&o)[4]) {
    return fmaxf(fmaxf(mx, fmaxf(m3t_fin_abs(o[0]), m3t_fin_abs(o[1]))), fmaxf(m3t_fin_abs(o[2]), m3t_fin_abs(o[3])));
}

// ---- row index -> (frame, row, column) of a P x A x B grid
static __device__ __forceinline__ void cl_decode(size_t r, int A, int B, size_t& p, int& a, int& b) {
    b = (int)(r % (size_t)B); r /= (size_t)B;
    a = (int)(r % (size_t)A);
    p = r / (size_t)A;
}

// ---- the end of a partial kernel: thread (row group g, quad q) leaves its two sums in red [2][groups][C]; the block folds the groups in
// index order (a fixed order) into out [2][C]
static __device__ __forceinline__ void cl_put_groups(double* red, int g, int q, int groups, int C, const double (&s)[4], const double (&t)[4]) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[(size_t)g * C + 4 * q + e] = s[e]; red[(size_t)(groups + g) * C + 4 * q + e] = t[e]; }
}
static __device__ __forceinline__ void cl_fold_groups(const double* red, int groups, int C, double* __restrict__ partial, size_t chunk) {
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += CL_TH) {
        double a0 = 0.0, b0 = 0.0;
        for (int k = 0; k < groups; ++k) { a0 += red[(size_t)k * C + c]; b0 += red[(size_t)(groups + k) * C + c]; }
        partial[(chunk * 2 + 0) * C + c] = a0;
        partial[(chunk * 2 + 1) * C + c] = b0;
    }
}

// ---- the end of a dx pass that also leaves column sums: a thread's four channels are fixed, cs holds its sums over its rows (T = float
// under BatchNorm, double under GroupNorm); block partial [C] = the 256 / (C / 4) threads that share a quad, in thread order.  A block starts
// at quad 0 (C / 4 divides 256), so the first thread that holds channel c is c / 4.
template <typename T>
static __device__ __forceinline__ void cl_block_colsum(const T (&cs)[4], T* csum, int C, T* __restrict__ colpart_row) {
    const int c4n = C >> 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) csum[threadIdx.x * 4 + e] = cs[e];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += CL_TH) {
        T t = 0;
        for (int th = c >> 2; th < CL_TH; th += c4n) t += csum[th * 4 + (c & 3)];
        colpart_row[c] = t;
    }
    __syncthreads();
}

// ---- BatchNorm's per-thread channel constants and its two formulas: w = gamma invstd, b = beta, k1 = sum g / M, k2 = sum g xhat / M
struct BNQuad {
    float w[4], b[4], mu[4], is[4], k1[4], k2[4];
    __device__ __forceinline__ void load_stats(const float* mean, const float* invstd, int q) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { mu[e] = mean[4 * q + e]; is[e] = invstd[4 * q + e]; }
    }
    __device__ __forceinline__ void load_fwd(const float* gamma, const float* beta, const float* mean,
                                             const float* invstd, int q) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            mu[e] = mean[c];
            w[e] = (gamma ? gamma[c] : 1.f) * invstd[c];
            b[e] = beta ? beta[c] : 0.f;
        }
    }
    __device__ __forceinline__ void load_bwd(const float* gamma, const float* mean, const float* invstd,
                                             const float* sums, int C, float inv_count, int training, int q) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * q + e;
            mu[e] = mean[c]; is[e] = invstd[c];
            w[e] = (gamma ? gamma[c] : 1.f) * is[e];
            k1[e] = training ? sums[c] * inv_count : 0.f;
            k2[e] = training ? sums[C + c] * inv_count : 0.f;
        }
    }
    // (v - mu) w + b and w (g - k1 - xhat k2) with the thread's constant as the first factor of every product: the operand order the kernels'
    // multiplies and FMAs have always had -- where two NaNs meet (a NaN input under NaN statistics) it decides whose sign comes out
    __device__ __forceinline__ float map(float v, int e) const { return w[e] * (v - mu[e]) + b[e]; }
    __device__ __forceinline__ float xhat(float x, int e) const { return is[e] * (x - mu[e]); }
    __device__ __forceinline__ float dx(float g, float x, int e, int training) const {
        return w[e] * (training ? g - k1[e] - k2[e] * xhat(x, e) : g);
    }
};

// ---- norm + ReLU + k x k / stride k / no padding max pooling as ONE operator (the backward kernels bnpool_bwd_* of stem_cl.hip and
// gnpool_bwd_* of gn_cl.hip; the two forward kernels keep their own text, see there): one body per kernel.  y = relu(norm(x)) at full
// resolution is never written and never read: forward keeps the pooled value P and the winner byte; in
// backward an input position's gradient through the pooling is dP of its window if it won, else 0, and the ReLU mask is taken on P (the
// winner's y IS P).  Geometry GEO: H, W, Ho x Wo = floor(H / k) x floor(W / k), He x We = ceil(H / k) x ceil(W / k) (odd H, W: edge positions
// no window covers), C.  The norm N is the family's quad (BNPoolQuad, GNQuad): mask(dP, P), xhat(x, e), dx(g, x, e),
// its accumulator type acc_t for the column sums, and the clip: n (0 under BatchNorm: one run of P frames) of T frames each.
// backward sums over a clip's pooled windows: partial[clip][chunk][2][C] = sum g, sum g xhat with g = dP masked by P, taken at the window's winner
template <int K, class GEO, class N>
static __device__ __forceinline__ void cl_normpool_bwd_partial(const float* __restrict__ dyp, const float* __restrict__ x, const float* __restrict__ yp,
                                                               const unsigned char* __restrict__ win, size_t nwin, const GEO g, size_t win_per_chunk,
                                                               double* __restrict__ partial, const N nm, int q, int gi) {
    extern __shared__ double red[];
    const int C = g.C, c4n = C >> 2, groups = CL_TH / c4n;
    const size_t r0 = (size_t)blockIdx.x * win_per_chunk;
    const size_t r1 = r0 + win_per_chunk < nwin ? r0 + win_per_chunk : nwin;
    const size_t p0 = (size_t)nm.n * nm.T;
    double s[4] = {0.0, 0.0, 0.0, 0.0}, t[4] = {0.0, 0.0, 0.0, 0.0};
    if (gi < groups) {
        for (size_t r = r0 + gi; r < r1; r += groups) {
            int ho, wo;
            size_t p;
            cl_decode(r, g.Ho, g.Wo, p, ho, wo);
            p += p0;
            const size_t o = ((size_t)nm.n * nwin + r) * (size_t)c4n + q;
            const float4 d = reinterpret_cast<const float4*>(dyp)[o];
            const float4 pv = reinterpret_cast<const float4*>(yp)[o];
            const uchar4 wb = reinterpret_cast<const uchar4*>(win)[o];
            const float de[4] = {d.x, d.y, d.z, d.w}, pe[4] = {pv.x, pv.y, pv.z, pv.w};
            const int we[4] = {wb.x, wb.y, wb.z, wb.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float gq = nm.mask(de[e], pe[e]);
                const int wi = we[e] < K * K ? we[e] : 0;                      // (a byte this library did not write must not index outside the window)
                const int dh = wi / K, dw = wi - dh * K;
                const float xv = x[((p * g.H + (size_t)(ho * K + dh)) * g.W + (size_t)(wo * K + dw)) * (size_t)C + 4 * q + e];
                s[e] += (double)gq;
                t[e] += (double)(gq * nm.xhat(xv, e));
            }
        }
        cl_put_groups(red, gi, q, groups, C, s, t);
    }
    cl_fold_groups(red, groups, C, partial, (size_t)nm.n * gridDim.x + blockIdx.x);
}

// dx at full resolution: a thread = one (extended) window x four channels; positions outside the pooled grid (odd H / W) have g = 0
template <int K, class GEO, class N>
static __device__ __forceinline__ void cl_normpool_bwd_dx(const float* __restrict__ dyp, const float* __restrict__ x, const float* __restrict__ yp,
                                                          const unsigned char* __restrict__ win, float* __restrict__ dx, size_t total4, const GEO g,
                                                          unsigned long long* __restrict__ slot, typename N::acc_t* __restrict__ colpart, const N nm,
                                                          int q) {
    typedef typename N::acc_t acc_t;
    __shared__ float red4[4];
    __shared__ acc_t csum[CL_TH * 4];
    const int C = g.C, c4n = C >> 2;
    const size_t p0 = (size_t)nm.n * nm.T;
    float mx = 0.f;
    acc_t cs[4] = {0, 0, 0, 0};
    for (size_t i = (size_t)blockIdx.x * CL_TH + threadIdx.x; i < total4; i += (size_t)gridDim.x * CL_TH) {
        int he, we_;
        size_t p;
        cl_decode(i / (size_t)c4n, g.He, g.We, p, he, we_);
        p += p0;
        const bool pooled = he < g.Ho && we_ < g.Wo;
        float de[4] = {0.f, 0.f, 0.f, 0.f};
        int wi[4] = {-1, -1, -1, -1};
        if (pooled) {
            const size_t o = ((p * g.Ho + he) * g.Wo + we_) * (size_t)c4n + q;
            const float4 d = reinterpret_cast<const float4*>(dyp)[o];
            const float4 pv = reinterpret_cast<const float4*>(yp)[o];
            const uchar4 wb = reinterpret_cast<const uchar4*>(win)[o];
            de[0] = nm.mask(d.x, pv.x); de[1] = nm.mask(d.y, pv.y); de[2] = nm.mask(d.z, pv.z); de[3] = nm.mask(d.w, pv.w);
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
                for (int e = 0; e < 4; ++e) o[e] = nm.dx((wi[e] == dh * K + dw) ? de[e] : 0.f, xe[e], e);
                *reinterpret_cast<float4*>(dx + xo) = make_float4(o[0], o[1], o[2], o[3]);
                if (slot) mx = cl_max4(mx, o);
                if (colpart) { cs[0] += (acc_t)o[0]; cs[1] += (acc_t)o[1]; cs[2] += (acc_t)o[2]; cs[3] += (acc_t)o[3]; }
            }
        }
    }
    if (colpart) cl_block_colsum(cs, csum, C, colpart + ((size_t)nm.n * gridDim.x + blockIdx.x) * C);
    if (slot) m3t_block_raise_slot(slot, mx, red4);
}
