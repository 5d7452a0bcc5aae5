// The 3-D DenseNet of `--backbone densenet` (reference models/densenet.py:5-93, models/backbone.py:375-423) on channels-last rows.
// A dense block is ONE buffer [rows = N T H W][C_final]: each layer's 3x3x3 convolution writes its 32 new channels straight into their columns
// (output leading dimension + column offset), so no layer concatenates anything.  Every BatchNorm of a block reads columns that no later layer
// modifies; the batch statistics of a column are therefore computed once, when the column is written (m3t_dense_col_stats), and serve every
// BatchNorm that reads it.  The operators here:
//   * column statistics over strided rows: fp64 per-chunk partials reduced in a fixed order (deterministic, no atomics)
//   * BatchNorm + ReLU applied from given statistics (forward), its backward with both per-channel reductions as fixed-order partials, the dx
//     pass accumulating into a strided gradient buffer (stream order, no atomics)
//   * transition: BatchNorm + ReLU + 2 x 2 average pooling (floor mode) in one pass; norm5 + ReLU + spatial mean (agg 'ap') or the (c, h, w)
//     reorder the reference's agg 'fc' feeds its Linear; the backward spreads that scatter the pooled gradient back to full resolution
//   * the 3x3x3 stride-1 pad-1 convolution with 32-wide output tiles (forward and, with the flipped weights, the data gradient) and its weight
//     gradient: fp32 FMA, register-tiled 4 x 4 per thread, LDS-staged, zero padding by bounds (no padded copy of the activation)
// Every fused ReLU is m3t_relu (NaN stays NaN).
#include "common.h"

namespace {

constexpr int DN_TH = 256;

inline size_t dn_chunks(size_t rows, size_t per) { return (rows + per - 1) / per; }

inline size_t stats_rows_per_chunk(size_t rows) {
    size_t per = 1024;
    while (dn_chunks(rows, per) > 512) per *= 2;
    return per;
}

// ---- column statistics: part[chunk][2][C] = (sum x, sum x^2) over the chunk's rows, fp64 ------------------------------------------------
__global__ __launch_bounds__(DN_TH) void stats_partial_kernel(const float* __restrict__ x, size_t rows, int ld, int C, size_t per,
                                                              double* __restrict__ part) {
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const size_t r0 = (size_t)blockIdx.y * per;
    const size_t r1 = r0 + per < rows ? r0 + per : rows;
    double s = 0.0, q = 0.0;
    if (c < C) {
        for (size_t r = r0 + rl; r < r1; r += 4) {
            const double v = (double)x[r * (size_t)ld + c];
            s += v;
            q += v * v;
        }
    }
    red[0][rl][cl] = s;
    red[1][rl][cl] = q;
    __syncthreads();
    if (rl == 0 && c < C) {
        double* out = part + (size_t)blockIdx.y * 2 * C;
        out[c] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
        out[C + c] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
    }
}

__global__ __launch_bounds__(DN_TH) void stats_final_kernel(const double* __restrict__ part, int chunks, int C, size_t rows,
                                                            float* __restrict__ mean, float* __restrict__ var) {
    const int c = blockIdx.x * DN_TH + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < chunks; ++k) {
        s += part[(size_t)k * 2 * C + c];
        q += part[(size_t)k * 2 * C + C + c];
    }
    const double m = s / (double)rows;
    const double v = q / (double)rows - m * m;
    mean[c] = (float)m;
    var[c] = (float)(v < 0.0 ? 0.0 : v);              // (a NaN variance stays NaN)
}

__device__ __forceinline__ void bn_coef(const float* mean, const float* var, const float* gamma, const float* beta, float eps, int c,
                                        float& a, float& b) {
    const float is = 1.0f / sqrtf(var[c] + eps);
    a = gamma[c] * is;
    b = beta[c] - mean[c] * a;
}

// ---- BatchNorm + ReLU from given statistics: y[r][c] (ldy) = relu(a_c x[r][c] (ldx) + b_c); C % 4 == 0 ------------------------------------
__global__ __launch_bounds__(DN_TH) void bn_relu_fwd_kernel(const float* __restrict__ x, int ldx, size_t rows, int C, const float* __restrict__ mean,
                                                            const float* __restrict__ var, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float eps, float* __restrict__ y, int ldy) {
    const int c4n = C >> 2;
    const size_t n = rows * (size_t)c4n;
    for (size_t i = (size_t)blockIdx.x * DN_TH + threadIdx.x; i < n; i += (size_t)gridDim.x * DN_TH) {
        const size_t r = i / c4n;
        const int c = (int)(i - r * c4n) * 4;
        const float4 v = *reinterpret_cast<const float4*>(x + r * (size_t)ldx + c);
        float a, b;
        float4 o;
        bn_coef(mean, var, gamma, beta, eps, c + 0, a, b); o.x = m3t_relu(fmaf(v.x, a, b));
        bn_coef(mean, var, gamma, beta, eps, c + 1, a, b); o.y = m3t_relu(fmaf(v.y, a, b));
        bn_coef(mean, var, gamma, beta, eps, c + 2, a, b); o.z = m3t_relu(fmaf(v.z, a, b));
        bn_coef(mean, var, gamma, beta, eps, c + 3, a, b); o.w = m3t_relu(fmaf(v.w, a, b));
        *reinterpret_cast<float4*>(y + r * (size_t)ldy + c) = o;
    }
}

__global__ void bn_running_kernel(const float* __restrict__ mean, const float* __restrict__ var, size_t rows, int C, float* __restrict__ rm,
                                  float* __restrict__ rv, float momentum) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float unb = (float)((double)rows / (double)(rows - 1));
    rm[c] = (1.f - momentum) * rm[c] + momentum * mean[c];
    rv[c] = (1.f - momentum) * rv[c] + momentum * (var[c] * unb);
}

// ---- BatchNorm + ReLU backward -------------------------------------------------------------------------------------------------------------
// g = dy where relu's input > 0 (torch's threshold_backward: g = dy unless the input is <= 0, so a NaN input passes dy), xhat = (x - mean) is;
// part[chunk][2][C] = (sum g, sum g xhat)
__global__ __launch_bounds__(DN_TH) void bn_bwd_partial_kernel(const float* __restrict__ dy, int ldy, const float* __restrict__ x, int ldx,
                                                               size_t rows, int C, size_t per, const float* __restrict__ mean,
                                                               const float* __restrict__ var, const float* __restrict__ gamma,
                                                               const float* __restrict__ beta, float eps, double* __restrict__ part) {
    __shared__ double red[2][4][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + cl;
    const size_t r0 = (size_t)blockIdx.y * per;
    const size_t r1 = r0 + per < rows ? r0 + per : rows;
    double s = 0.0, q = 0.0;
    if (c < C) {
        const float is = 1.0f / sqrtf(var[c] + eps), mu = mean[c];
        float a, b;
        bn_coef(mean, var, gamma, beta, eps, c, a, b);
        for (size_t r = r0 + rl; r < r1; r += 4) {
            const float xv = x[r * (size_t)ldx + c];
            const float g = fmaf(xv, a, b) <= 0.f ? 0.f : dy[r * (size_t)ldy + c];
            s += (double)g;
            q += (double)g * (double)((xv - mu) * is);
        }
    }
    red[0][rl][cl] = s;
    red[1][rl][cl] = q;
    __syncthreads();
    if (rl == 0 && c < C) {
        double* out = part + (size_t)blockIdx.y * 2 * C;
        out[c] = ((red[0][0][cl] + red[0][1][cl]) + red[0][2][cl]) + red[0][3][cl];
        out[C + c] = ((red[1][0][cl] + red[1][1][cl]) + red[1][2][cl]) + red[1][3][cl];
    }
}

// sums[0][c] = dbeta, sums[1][c] = dgamma (fp32), also written to the caller's dgamma / dbeta when given
__global__ __launch_bounds__(DN_TH) void bn_bwd_final_kernel(const double* __restrict__ part, int chunks, int C, float* __restrict__ sums,
                                                             float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * DN_TH + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int k = 0; k < chunks; ++k) {
        s += part[(size_t)k * 2 * C + c];
        q += part[(size_t)k * 2 * C + C + c];
    }
    sums[c] = (float)s;
    sums[C + c] = (float)q;
    if (dbeta) dbeta[c] = (float)s;
    if (dgamma) dgamma[c] = (float)q;
}

// dx (lddx) (+)= a_c (g - sum g / M - xhat sum(g xhat) / M)  (training)  |  a_c g  (eval: running statistics are constants)
__global__ __launch_bounds__(DN_TH) void bn_bwd_dx_kernel(const float* __restrict__ dy, int ldy, const float* __restrict__ x, int ldx, size_t rows,
                                                          int C, const float* __restrict__ mean, const float* __restrict__ var,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                          const float* __restrict__ sums, int training, float* __restrict__ dx, int lddx,
                                                          int accumulate) {
    const size_t n = rows * (size_t)C;
    const float inv_m = 1.0f / (float)rows;
    for (size_t i = (size_t)blockIdx.x * DN_TH + threadIdx.x; i < n; i += (size_t)gridDim.x * DN_TH) {
        const size_t r = i / C;
        const int c = (int)(i - r * C);
        const float xv = x[r * (size_t)ldx + c];
        float a, b;
        bn_coef(mean, var, gamma, beta, eps, c, a, b);
        const float g = fmaf(xv, a, b) <= 0.f ? 0.f : dy[r * (size_t)ldy + c];
        float v;
        if (training) {
            const float is = 1.0f / sqrtf(var[c] + eps);
            const float xh = (xv - mean[c]) * is;
            v = a * (g - sums[c] * inv_m - xh * (sums[C + c] * inv_m));
        } else {
            v = a * g;
        }
        float* d = dx + r * (size_t)lddx + c;
        *d = accumulate ? *d + v : v;
    }
}

// ---- transition: y[p][ho][wo][c] = mean of relu(bn(x)) over the 2 x 2 window (floor mode: an odd last row / column is dropped) ----------
__global__ __launch_bounds__(DN_TH) void pool_fwd_kernel(const float* __restrict__ x, int ldx, size_t P, int H, int W, int C,
                                                         const float* __restrict__ mean, const float* __restrict__ var,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                         float* __restrict__ y) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t n = P * Ho * Wo * (size_t)C;
    for (size_t i = (size_t)blockIdx.x * DN_TH + threadIdx.x; i < n; i += (size_t)gridDim.x * DN_TH) {
        const int c = (int)(i % C);
        const size_t o = i / C;
        const int wo = (int)(o % Wo), ho = (int)((o / Wo) % Ho);
        const size_t p = o / ((size_t)Wo * Ho);
        float a, b;
        bn_coef(mean, var, gamma, beta, eps, c, a, b);
        const size_t r00 = (p * H + 2 * ho) * (size_t)W + 2 * wo;
        const float v00 = m3t_relu(fmaf(x[r00 * ldx + c], a, b));
        const float v01 = m3t_relu(fmaf(x[(r00 + 1) * ldx + c], a, b));
        const float v10 = m3t_relu(fmaf(x[(r00 + W) * ldx + c], a, b));
        const float v11 = m3t_relu(fmaf(x[(r00 + W + 1) * ldx + c], a, b));
        y[i] = (((v00 + v01) + v10) + v11) * 0.25f;
    }
}

// dfull[p][h][w][c] = dy[p][h/2][w/2][c] / 4 inside the pooled area, 0 on a dropped row / column
__global__ __launch_bounds__(DN_TH) void pool_spread_kernel(const float* __restrict__ dy, size_t P, int H, int W, int C, float* __restrict__ dfull) {
    const int Ho = H / 2, Wo = W / 2;
    const size_t n = P * H * W * (size_t)C;
    for (size_t i = (size_t)blockIdx.x * DN_TH + threadIdx.x; i < n; i += (size_t)gridDim.x * DN_TH) {
        const int c = (int)(i % C);
        const size_t o = i / C;
        const int w = (int)(o % W), h = (int)((o / W) % H);
        const size_t p = o / ((size_t)W * H);
        const int ho = h >> 1, wo = w >> 1;
        dfull[i] = (ho < Ho && wo < Wo) ? dy[((p * Ho + ho) * Wo + wo) * (size_t)C + c] * 0.25f : 0.f;
    }
}

// ---- norm5 + ReLU + aggregation: mode 0 ('ap') y[p][c] = mean over hw; mode 1 ('fc') y[p][c * HW + hw] ----------------------------------
__global__ __launch_bounds__(DN_TH) void mean_fwd_kernel(const float* __restrict__ x, int ldx, size_t P, int HW, int C,
                                                         const float* __restrict__ mean, const float* __restrict__ var,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float eps, int mode,
                                                         float* __restrict__ y) {
    const size_t n = P * (size_t)C;
    for (size_t i = (size_t)blockIdx.x * DN_TH + threadIdx.x; i < n; i += (size_t)gridDim.x * DN_TH) {
        const int c = (int)(i % C);
        const size_t p = i / C;
        float a, b;
        bn_coef(mean, var, gamma, beta, eps, c, a, b);
        float s = 0.f;
        for (int k = 0; k < HW; ++k) {
            const float v = m3t_relu(fmaf(x[(p * HW + k) * (size_t)ldx + c], a, b));
            if (mode) y[(p * C + c) * HW + k] = v;
            else s += v;
        }
        if (!mode) y[i] = s / (float)HW;
    }
}

__global__ __launch_bounds__(DN_TH) void mean_spread_kernel(const float* __restrict__ dy, size_t P, int HW, int C, int mode, float* __restrict__ dfull) {
    const size_t n = P * HW * (size_t)C;
    const float inv = 1.0f / (float)HW;
    for (size_t i = (size_t)blockIdx.x * DN_TH + threadIdx.x; i < n; i += (size_t)gridDim.x * DN_TH) {
        const int c = (int)(i % C);
        const size_t o = i / C;
        const int k = (int)(o % HW);
        const size_t p = o / HW;
        dfull[i] = mode ? dy[(p * C + c) * HW + k] : dy[p * C + c] * inv;
    }
}

// ---- 3x3x3 convolution, stride 1, padding 1, channels-last ---------------------------------------------------------------------------
// y[m][co] (ldy) (+)= sum_tap sum_ci x[m + off(tap)][ci] (ldx, zero outside the clip) w[tap][ci][co]; tap = (dt, dh, dw) row-major.
// Tile: 128 output rows x 32 output channels per 256-thread block, 4 rows x 4 channels per thread; the k loop walks (tap, 32 input channels)
// slices staged in LDS, x transposed to [ci][row] so that a thread reads its four rows as one float4.  Ci % 32 == 0, Co % 32 == 0.
constexpr int CV_BM = 128, CV_BN = 32, CV_BK = 32;

struct Geo { int T, H, W; };

__device__ __forceinline__ bool src_row(size_t m, size_t rows, const Geo g, int dt, int dh, int dw, size_t& src) {
    if (m >= rows) return false;
    const int w = (int)(m % g.W), h = (int)((m / g.W) % g.H), t = (int)((m / ((size_t)g.W * g.H)) % g.T);
    const int tt = t + dt - 1, hh = h + dh - 1, ww = w + dw - 1;
    if (tt < 0 || tt >= g.T || hh < 0 || hh >= g.H || ww < 0 || ww >= g.W) return false;
    src = m + (ptrdiff_t)((dt - 1) * g.H * g.W + (dh - 1) * g.W + (dw - 1));
    return true;
}

__global__ __launch_bounds__(DN_TH) void conv333_kernel(const float* __restrict__ x, int ldx, size_t rows, Geo g, int Ci,
                                                        const float* __restrict__ w, float* __restrict__ y, int ldy, int Co, int accumulate) {
    __shared__ __attribute__((aligned(16))) float xs[CV_BK][CV_BM + 4];
    __shared__ __attribute__((aligned(16))) float wsm[CV_BK][CV_BN];
    const int tid = threadIdx.x;
    const int tr = tid >> 3, tc = tid & 7;                    // rows 4 tr .. 4 tr + 3, channels 4 tc .. 4 tc + 3 of the tile
    const size_t m0 = (size_t)blockIdx.x * CV_BM;
    const int co0 = blockIdx.y * CV_BN;
    float acc[4][4] = {};
    for (int tap = 0; tap < 27; ++tap) {
        const int dt = tap / 9, dh = (tap / 3) % 3, dw = tap % 3;
        size_t src[4];
        bool ok[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {                         // this thread stages float4 (row f >> 3, ci 4 (f & 7)) for f = tid + 256 j
            const int f = tid + DN_TH * j;
            ok[j] = src_row(m0 + (f >> 3), rows, g, dt, dh, dw, src[j]);
        }
        for (int c0 = 0; c0 < Ci; c0 += CV_BK) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = tid + DN_TH * j, r = f >> 3, q = (f & 7) * 4;
                float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                if (ok[j]) v = *reinterpret_cast<const float4*>(x + src[j] * (size_t)ldx + c0 + q);
                xs[q + 0][r] = v.x; xs[q + 1][r] = v.y; xs[q + 2][r] = v.z; xs[q + 3][r] = v.w;
            }
            {
                const int k = tid >> 3, q = (tid & 7) * 4;
                *reinterpret_cast<float4*>(&wsm[k][q]) =
                    *reinterpret_cast<const float4*>(w + ((size_t)tap * Ci + c0 + k) * Co + co0 + q);
            }
            __syncthreads();
#pragma unroll 8
            for (int k = 0; k < CV_BK; ++k) {
                const float4 a = *reinterpret_cast<const float4*>(&xs[k][4 * tr]);
                const float4 b = *reinterpret_cast<const float4*>(&wsm[k][4 * tc]);
                const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) acc[i][jj] = fmaf(av[i], bv[jj], acc[i][jj]);
            }
            __syncthreads();
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const size_t m = m0 + 4 * tr + i;
        if (m >= rows) continue;
        float4* d = reinterpret_cast<float4*>(y + m * (size_t)ldy + co0 + 4 * tc);
        float4 o = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        if (accumulate) {
            const float4 p = *d;
            o.x += p.x; o.y += p.y; o.z += p.z; o.w += p.w;
        }
        *d = o;
    }
}

// ---- its weight gradient: part[chunk][tap][ci][co] = sum over the chunk's rows m of x[m + off(tap)][ci] dy[m][co] ---------------------------
// Tile: one tap x 128 input channels x 32 output channels per block, 4 x 4 per thread; 32 rows per LDS stage.  Ci % 128 == 0, Co % 32 == 0.
constexpr int WG_BR = 32, WG_BI = 128, WG_BO = 32;

__global__ __launch_bounds__(DN_TH) void wgrad333_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ dy, int ldy, size_t rows,
                                                         Geo g, int Ci, int Co, size_t per, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float xs[WG_BR][WG_BI];
    __shared__ __attribute__((aligned(16))) float ds[WG_BR][WG_BO];
    const int tid = threadIdx.x;
    const int ti = tid >> 3, to = tid & 7;                    // input channels 4 ti .., output channels 4 to ..
    const int tap = blockIdx.x;
    const int nco = Co / WG_BO;
    const int ci0 = (blockIdx.z / nco) * WG_BI, co0 = (blockIdx.z % nco) * WG_BO;
    const int dt = tap / 9, dh = (tap / 3) % 3, dw = tap % 3;
    const size_t r0 = (size_t)blockIdx.y * per;
    const size_t r1 = r0 + per < rows ? r0 + per : rows;
    float acc[4][4] = {};
    for (size_t rb = r0; rb < r1; rb += WG_BR) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {                         // x: 32 rows x 128 channels = 1024 float4
            const int f = tid + DN_TH * j, r = f >> 5, q = (f & 31) * 4;
            size_t s;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rb + r < r1 && src_row(rb + r, rows, g, dt, dh, dw, s)) v = *reinterpret_cast<const float4*>(x + s * (size_t)ldx + ci0 + q);
            *reinterpret_cast<float4*>(&xs[r][q]) = v;
        }
        {                                                     // dy: 32 rows x 32 channels = 256 float4
            const int r = tid >> 3, q = (tid & 7) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rb + r < r1) v = *reinterpret_cast<const float4*>(dy + (rb + r) * (size_t)ldy + co0 + q);
            *reinterpret_cast<float4*>(&ds[r][q]) = v;
        }
        __syncthreads();
#pragma unroll 8
        for (int r = 0; r < WG_BR; ++r) {
            const float4 a = *reinterpret_cast<const float4*>(&xs[r][4 * ti]);
            const float4 b = *reinterpret_cast<const float4*>(&ds[r][4 * to]);
            const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) acc[i][jj] = fmaf(av[i], bv[jj], acc[i][jj]);
        }
        __syncthreads();
    }
    float* out = part + ((size_t)blockIdx.y * 27 + tap) * (size_t)Ci * Co;
#pragma unroll
    for (int i = 0; i < 4; ++i)
        *reinterpret_cast<float4*>(out + (size_t)(ci0 + 4 * ti + i) * Co + co0 + 4 * to) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
}

__global__ __launch_bounds__(DN_TH) void chunk_sum_kernel(const float* __restrict__ part, int chunks, size_t n, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * DN_TH + threadIdx.x; i < n; i += (size_t)gridDim.x * DN_TH) {
        float s = 0.f;
        for (int k = 0; k < chunks; ++k) s += part[(size_t)k * n + i];
        out[i] = s;
    }
}

inline int grid_for(size_t n) {
    const size_t b = (n + DN_TH - 1) / DN_TH;
    return (int)(b < 8192 ? (b ? b : 1) : 8192);
}

inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

inline size_t wgrad_rows_per_chunk(size_t rows) {
    size_t per = 256;
    while (dn_chunks(rows, per) > 64) per *= 2;
    return per;
}

}  // namespace

extern "C" size_t m3t_dense_stats_ws_bytes(size_t rows, int C) {
    return dn_chunks(rows, stats_rows_per_chunk(rows)) * 2 * (size_t)(C > 0 ? C : 0) * sizeof(double);
}

extern "C" int m3t_dense_col_stats(const float* x, size_t rows, int ld, int C, float* mean, float* var, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !mean || !var || !ws || rows < 1 || C < 1 || ld < C || ws_bytes < m3t_dense_stats_ws_bytes(rows, C) || ((uintptr_t)ws % 8) != 0)
        return M3T_EINVAL;
    const size_t per = stats_rows_per_chunk(rows);
    const int chunks = (int)dn_chunks(rows, per);
    hipStream_t s = (hipStream_t)stream;
    stats_partial_kernel<<<dim3(cdiv(C, 64), chunks), DN_TH, 0, s>>>(x, rows, ld, C, per, (double*)ws);
    stats_final_kernel<<<cdiv(C, DN_TH), DN_TH, 0, s>>>((const double*)ws, chunks, C, rows, mean, var);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_dense_bn_relu_fwd(const float* x, int ldx, size_t rows, int C, const float* mean, const float* var, const float* gamma,
                                     const float* beta, float eps, float* y, int ldy, void* stream) {
    if (!x || !y || !mean || !var || !gamma || !beta || rows < 1 || C < 4 || C % 4 || ldx % 4 || ldy % 4 || ldx < C || ldy < C || !al16(x) ||
        !al16(y))
        return M3T_EINVAL;
    bn_relu_fwd_kernel<<<grid_for(rows * (C / 4)), DN_TH, 0, (hipStream_t)stream>>>(x, ldx, rows, C, mean, var, gamma, beta, eps, y, ldy);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_dense_bn_running(const float* mean, const float* var, size_t rows, int C, float* run_mean, float* run_var, float momentum,
                                    void* stream) {
    if (!mean || !var || !run_mean || !run_var || rows < 2 || C < 1) return M3T_EINVAL;
    bn_running_kernel<<<cdiv(C, DN_TH), DN_TH, 0, (hipStream_t)stream>>>(mean, var, rows, C, run_mean, run_var, momentum);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_dense_bn_relu_bwd(const float* dy, int ldy, const float* x, int ldx, size_t rows, int C, const float* mean, const float* var,
                                     const float* gamma, const float* beta, float eps, int training, float* dx, int lddx, int accumulate,
                                     float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    const size_t need = m3t_dense_stats_ws_bytes(rows, C) + 2 * (size_t)C * sizeof(float);
    if (!dy || !x || !mean || !var || !gamma || !beta || rows < 1 || C < 1 || ldy < C || ldx < C || (dx && lddx < C) || !ws ||
        ws_bytes < need || ((uintptr_t)ws % 8) != 0)
        return M3T_EINVAL;
    const size_t per = stats_rows_per_chunk(rows);
    const int chunks = (int)dn_chunks(rows, per);
    hipStream_t s = (hipStream_t)stream;
    double* part = (double*)ws;
    float* sums = (float*)((char*)ws + m3t_dense_stats_ws_bytes(rows, C));
    bn_bwd_partial_kernel<<<dim3(cdiv(C, 64), chunks), DN_TH, 0, s>>>(dy, ldy, x, ldx, rows, C, per, mean, var, gamma, beta, eps, part);
    bn_bwd_final_kernel<<<cdiv(C, DN_TH), DN_TH, 0, s>>>(part, chunks, C, sums, dgamma, dbeta);
    if (dx)
        bn_bwd_dx_kernel<<<grid_for(rows * C), DN_TH, 0, s>>>(dy, ldy, x, ldx, rows, C, mean, var, gamma, beta, eps, sums, training, dx, lddx,
                                                              accumulate);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_dense_pool_fwd(const float* x, int ldx, size_t P, int H, int W, int C, const float* mean, const float* var, const float* gamma,
                                  const float* beta, float eps, float* y, void* stream) {
    if (!x || !y || !mean || !var || !gamma || !beta || P < 1 || H < 2 || W < 2 || C < 1 || ldx < C) return M3T_EINVAL;
    pool_fwd_kernel<<<grid_for(P * (H / 2) * (W / 2) * (size_t)C), DN_TH, 0, (hipStream_t)stream>>>(x, ldx, P, H, W, C, mean, var, gamma, beta,
                                                                                                    eps, y);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_dense_pool_spread(const float* dy, size_t P, int H, int W, int C, float* dfull, void* stream) {
    if (!dy || !dfull || P < 1 || H < 2 || W < 2 || C < 1) return M3T_EINVAL;
    pool_spread_kernel<<<grid_for(P * H * W * (size_t)C), DN_TH, 0, (hipStream_t)stream>>>(dy, P, H, W, C, dfull);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_dense_mean_fwd(const float* x, int ldx, size_t P, int HW, int C, const float* mean, const float* var, const float* gamma,
                                  const float* beta, float eps, int mode, float* y, void* stream) {
    if (!x || !y || !mean || !var || !gamma || !beta || P < 1 || HW < 1 || C < 1 || ldx < C || (mode != 0 && mode != 1)) return M3T_EINVAL;
    mean_fwd_kernel<<<grid_for(P * (size_t)C), DN_TH, 0, (hipStream_t)stream>>>(x, ldx, P, HW, C, mean, var, gamma, beta, eps, mode, y);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_dense_mean_spread(const float* dy, size_t P, int HW, int C, int mode, float* dfull, void* stream) {
    if (!dy || !dfull || P < 1 || HW < 1 || C < 1 || (mode != 0 && mode != 1)) return M3T_EINVAL;
    mean_spread_kernel<<<grid_for(P * HW * (size_t)C), DN_TH, 0, (hipStream_t)stream>>>(dy, P, HW, C, mode, dfull);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_dense_conv333(const float* x, int ldx, int N, int T, int H, int W, int Ci, const float* w, float* y, int ldy, int Co,
                                 int accumulate, void* stream) {
    if (!x || !w || !y || N < 1 || T < 1 || H < 1 || W < 1 || Ci < CV_BK || Ci % CV_BK || Co < CV_BN || Co % CV_BN || ldx < Ci || ldy < Co ||
        ldx % 4 || ldy % 4 || !al16(x) || !al16(w) || !al16(y))
        return M3T_EINVAL;
    const size_t rows = (size_t)N * T * H * W;
    const size_t tiles = (rows + CV_BM - 1) / CV_BM;
    if (tiles > 0x7fffffff) return M3T_EINVAL;
    conv333_kernel<<<dim3((unsigned)tiles, Co / CV_BN), DN_TH, 0, (hipStream_t)stream>>>(x, ldx, rows, Geo{T, H, W}, Ci, w, y, ldy, Co, accumulate);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t m3t_dense_wgrad_ws_bytes(size_t rows, int Ci, int Co) {
    return dn_chunks(rows, wgrad_rows_per_chunk(rows)) * 27 * (size_t)(Ci > 0 ? Ci : 0) * (size_t)(Co > 0 ? Co : 0) * sizeof(float);
}

extern "C" int m3t_dense_conv333_wgrad(const float* x, int ldx, const float* dy, int ldy, int N, int T, int H, int W, int Ci, int Co, float* dw,
                                       void* ws, size_t ws_bytes, void* stream) {
    const size_t rows = (size_t)N * T * H * W;
    if (!x || !dy || !dw || !ws || N < 1 || T < 1 || H < 1 || W < 1 || Ci < WG_BI || Ci % WG_BI || Co < WG_BO || Co % WG_BO || ldx < Ci ||
        ldy < Co || ldx % 4 || ldy % 4 || !al16(x) || !al16(dy) || !al16(ws) || ws_bytes < m3t_dense_wgrad_ws_bytes(rows, Ci, Co))
        return M3T_EINVAL;
    const size_t per = wgrad_rows_per_chunk(rows);
    const int chunks = (int)dn_chunks(rows, per);
    hipStream_t s = (hipStream_t)stream;
    wgrad333_kernel<<<dim3(27, chunks, (Ci / WG_BI) * (Co / WG_BO)), DN_TH, 0, s>>>(x, ldx, dy, ldy, rows, Geo{T, H, W}, Ci, Co, per, (float*)ws);
    const size_t n = 27 * (size_t)Ci * Co;
    chunk_sum_kernel<<<grid_for(n), DN_TH, 0, s>>>((const float*)ws, chunks, n, dw);
    M3T_LAUNCH_CHECK();
    return 0;
}
