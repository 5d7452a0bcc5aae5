// Attention decoder of --fusion_type att_dec (reference models/rnn.py:84-165: Attention, Decoder, AttEncDec): the T-1 step greedy /
// teacher-forced recurrence, forward and backward, in fp32.  Per forward step three launches (attention over the clip, GRU cell, the
// stacked product [W_hh; W_ah] h_t + the output layer that feeds step t+1), per backward step four (cell backward, context gradient,
// attention backward, hidden-state gradient).  Every reduction walks a fixed order (wave butterflies, sequential loops); no atomics.
// Workgroups of the weight-streaming kernels own weight rows across the whole batch: the 7 MB of decoder weights are read once a step.
#include "common.h"

namespace {

constexpr int NT = 256;          // threads per workgroup, 4 waves
constexpr int MAX_KH = 8;        // H / 64 <= 8  (H <= 512)
constexpr int MAX_T = 8192;      // scores (and their gradients) of one clip live in LDS: <= 64 KiB

static __device__ __forceinline__ float block_max(float v, float* red) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < NT / 64; ++i) r = fmaxf(r, red[i]);
    return r;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// one workgroup per clip: s_tau = v . relu(P[tau] + a), alpha = softmax(s), c = sum_tau alpha_tau enc[tau]
// a: [B] rows of lda; alpha: [B][T]; c: [B] rows of ldc (may be null); a_save: [B][H] copy of a (may be null)
template <int KH>
__global__ __launch_bounds__(NT) void attn_fwd_kernel(const float* __restrict__ enc, const float* __restrict__ P,
                                                      const float* __restrict__ a, int lda, const float* __restrict__ v,
                                                      float* __restrict__ alpha, float* __restrict__ c, int ldc,
                                                      float* __restrict__ a_save, int T, int H) {
    extern __shared__ float s_lds[];
    __shared__ float red[NT / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* ab = a + (size_t)b * lda;
    float ar[KH], vr[KH];
#pragma unroll
    for (int k = 0; k < KH; ++k) { ar[k] = ab[lane + 64 * k]; vr[k] = v[lane + 64 * k]; }
    const float* Pb = P + (size_t)b * T * H;
    for (int tau = w; tau < T; tau += NT / 64) {
        const float* pr = Pb + (size_t)tau * H;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < KH; ++k) s += vr[k] * m3t_relu(pr[lane + 64 * k] + ar[k]);
        s = wave_sum(s);
        if (lane == 0) s_lds[tau] = s;
    }
    __syncthreads();
    float m = -INFINITY;
    for (int tau = threadIdx.x; tau < T; tau += NT) m = fmaxf(m, s_lds[tau]);
    m = block_max(m, red);
    float z = 0.f;
    for (int tau = threadIdx.x; tau < T; tau += NT) { const float e = expf(s_lds[tau] - m); s_lds[tau] = e; z += e; }
    z = block_sum(z, red);
    const float inv = 1.f / z;
    float* al = alpha + (size_t)b * T;
    for (int tau = threadIdx.x; tau < T; tau += NT) { const float x = s_lds[tau] * inv; s_lds[tau] = x; al[tau] = x; }
    __syncthreads();
    const float* eb = enc + (size_t)b * T * H;
    for (int h = threadIdx.x; h < H; h += NT) {
        if (a_save) a_save[(size_t)b * H + h] = ab[h];
        if (!c) continue;
        float acc = 0.f;
        for (int tau = 0; tau < T; ++tau) acc += s_lds[tau] * eb[(size_t)tau * H + h];
        c[(size_t)b * ldc + h] = acc;
    }
}

// GRU cell: gi = W_ih [y_in, c] + b_ih against G [B][4H], which holds W_hh h_{t-1} + b_hh in its first 3H columns.
// Writes h_t and the gates [B][4H] = (r, z, n, W_hn h_{t-1} + b_hn) that backward uses.
__global__ __launch_bounds__(NT) void cell_fwd_kernel(const float* __restrict__ G, const float* __restrict__ x, int H,
                                                      const float* __restrict__ w_ih, const float* __restrict__ b_ih,
                                                      const float* __restrict__ h_prev, float* __restrict__ h_out,
                                                      float* __restrict__ gates, int B) {
    // one wave per unit j: the three W_ih rows of j are read once and dotted with every clip's input [y_in, c]
    const int lane = threadIdx.x & 63;
    const int j = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (j >= H) return;
    const int K = H + 2;
    const float* wr = w_ih + (size_t)j * K;
    const float* wz = w_ih + (size_t)(H + j) * K;
    const float* wn = w_ih + (size_t)(2 * H + j) * K;
    float rr[MAX_KH + 1], rz[MAX_KH + 1], rn[MAX_KH + 1];
    const int KH = H / 64;
#pragma unroll
    for (int k = 0; k < MAX_KH + 1; ++k) {
        const int col = lane + 64 * k;
        const bool ok = k < KH + 1 && col < K;
        rr[k] = ok ? wr[col] : 0.f; rz[k] = ok ? wz[col] : 0.f; rn[k] = ok ? wn[col] : 0.f;
    }
    const float bir = b_ih[j], biz = b_ih[H + j], bin = b_ih[2 * H + j];
    for (int b = 0; b < B; ++b) {
        const float* xb = x + (size_t)b * K;
        float sr = 0.f, sz = 0.f, sn = 0.f;
#pragma unroll
        for (int k = 0; k < MAX_KH + 1; ++k) {
            const int col = lane + 64 * k;
            const float xv = (k < KH + 1 && col < K) ? xb[col] : 0.f;
            sr += rr[k] * xv; sz += rz[k] * xv; sn += rn[k] * xv;
        }
        sr = wave_sum(sr); sz = wave_sum(sz); sn = wave_sum(sn);
        if (lane == 0) {
            const float* gb = G + (size_t)b * 4 * H;
            const float r = 1.f / (1.f + expf(-(sr + bir + gb[j])));
            const float z = 1.f / (1.f + expf(-(sz + biz + gb[H + j])));
            const float ghn = gb[2 * H + j];
            const float n = tanhf(sn + bin + r * ghn);
            const float hp = h_prev[(size_t)b * H + j];
            h_out[(size_t)b * H + j] = (1.f - z) * n + z * hp;
            float* gs = gates + (size_t)b * 4 * H;
            gs[j] = r; gs[H + j] = z; gs[2 * H + j] = n; gs[3 * H + j] = ghn;
        }
    }
}

// G[b][r] = [W_hh; W_ah][r] . h[b] (+ b_hh[r] for r < 3H) for r < 4H; rows 4H, 4H + 1 (when t > 0): y_t = W_o [h_t, c_t] + b_o,
// written to out[b][t] and, for the next step, x_next[b][0..1] = tf[t] ? trg[b][t] : y_t.  One wave per row, all clips.
__global__ __launch_bounds__(NT) void proj_kernel(const float* __restrict__ h, const float* __restrict__ x, const float* __restrict__ w_hh,
                                                  const float* __restrict__ b_hh, const float* __restrict__ w_a, const float* __restrict__ w_o,
                                                  const float* __restrict__ b_o, float* __restrict__ G, float* __restrict__ out,
                                                  float* __restrict__ x_next, const float* __restrict__ trg, const int* __restrict__ tf,
                                                  int t, int B, int L, int H) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    const int KH = H / 64;
    const int rows = 4 * H + (t > 0 ? 2 : 0);
    if (r >= rows) return;
    if (r < 4 * H) {
        const float* w = r < 3 * H ? w_hh + (size_t)r * H : w_a + (size_t)(r - 3 * H) * 2 * H;
        float wr[MAX_KH];
#pragma unroll
        for (int k = 0; k < MAX_KH; ++k) wr[k] = k < KH ? w[lane + 64 * k] : 0.f;
        const float bias = r < 3 * H ? b_hh[r] : 0.f;
        for (int b = 0; b < B; ++b) {
            const float* hb = h + (size_t)b * H;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < MAX_KH; ++k) if (k < KH) s += wr[k] * hb[lane + 64 * k];
            s = wave_sum(s);
            if (lane == 0) G[(size_t)b * 4 * H + r] = s + bias;
        }
        return;
    }
    const int o = r - 4 * H;
    const float* w = w_o + (size_t)o * 2 * H;
    float wh[MAX_KH], wc[MAX_KH];
#pragma unroll
    for (int k = 0; k < MAX_KH; ++k) { wh[k] = k < KH ? w[lane + 64 * k] : 0.f; wc[k] = k < KH ? w[H + lane + 64 * k] : 0.f; }
    const int teach = (tf && trg) ? tf[t] : 0;
    for (int b = 0; b < B; ++b) {
        const float* hb = h + (size_t)b * H;
        const float* cb = x + (size_t)b * (H + 2) + 2;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < MAX_KH; ++k) if (k < KH) s += wh[k] * hb[lane + 64 * k] + wc[k] * cb[lane + 64 * k];
        s = wave_sum(s);
        if (lane == 0) {
            const float y = s + b_o[o];
            out[((size_t)b * L + t) * 2 + o] = y;
            if (x_next) x_next[(size_t)b * (H + 2) + o] = teach ? trg[((size_t)b * L + t) * 2 + o] : y;
        }
    }
}

// x0[b][0..1] = y0 (or 0); hs0 = h0
__global__ void fwd_init_kernel(const float* __restrict__ y0, const float* __restrict__ h0, float* __restrict__ x0,
                                float* __restrict__ hs0, int B, int H) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B * H) hs0[i] = h0[i];
    if (x0 && i < B * 2) x0[(size_t)(i >> 1) * (H + 2) + (i & 1)] = y0 ? y0[i] : 0.f;
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// w_iht [H+2][3H] = W_ih^T; wt [H][4H] = [W_hh^T | W_ah^T]
__global__ void bwd_prep_kernel(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ w_a,
                                float* __restrict__ w_iht, float* __restrict__ wt, int H) {
    const size_t n1 = (size_t)(H + 2) * 3 * H, n2 = (size_t)H * 4 * H;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n1 + n2; i += (size_t)gridDim.x * blockDim.x) {
        if (i < n1) {
            const size_t k = i / (3 * H), m = i % (3 * H);
            w_iht[i] = w_ih[m * (H + 2) + k];
        } else {
            const size_t q = i - n1, k = q / (4 * H), m = q % (4 * H);
            wt[q] = m < (size_t)3 * H ? w_hh[m * H + k] : w_a[(m - 3 * H) * 2 * H + k];
        }
    }
}

// K1, one thread per (clip, unit): dy_t = dout[:, t] + feedback; dh_t += W_o[:, :H]^T dy_t; GRU-cell backward -> dgi, dgh; dhz = z dh_t
__global__ __launch_bounds__(NT) void cell_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ dyin, const int* __restrict__ tf,
                                                      const float* __restrict__ w_o, const float* __restrict__ gates,
                                                      const float* __restrict__ h_prev, const float* __restrict__ dh,
                                                      float* __restrict__ dgi, float* __restrict__ dgh, float* __restrict__ dhz,
                                                      float* __restrict__ dy_save, int t, int B, int L, int H) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, j = i % H;
    const int fb = t + 1 < L && !(tf && tf[t]);        // step t + 1 was fed this step's own y_t: its input gradient flows back
    const float dy0 = dout[((size_t)b * L + t) * 2] + (fb ? dyin[b * 2] : 0.f);
    const float dy1 = dout[((size_t)b * L + t) * 2 + 1] + (fb ? dyin[b * 2 + 1] : 0.f);
    if (j == 0) { dy_save[b * 2] = dy0; dy_save[b * 2 + 1] = dy1; }
    const float g = dh[i] + w_o[j] * dy0 + w_o[2 * H + j] * dy1;
    const float* gs = gates + (size_t)b * 4 * H;
    const float r = gs[j], z = gs[H + j], n = gs[2 * H + j], ghn = gs[3 * H + j];
    const float dn = g * (1.f - z) * (1.f - n * n);
    const float dz = g * (h_prev[i] - n) * z * (1.f - z);
    const float dr = dn * ghn * r * (1.f - r);
    float* gi = dgi + (size_t)b * 3 * H;
    float* gh = dgh + (size_t)b * 3 * H;
    gi[j] = dr; gi[H + j] = dz; gi[2 * H + j] = dn;
    gh[j] = dr; gh[H + j] = dz; gh[2 * H + j] = dn * r;
    dhz[i] = z * g;
}

// K2, one wave per row k of W_ih^T: k >= 2: dc[b][k-2] = W_ih[:, k]^T dgi[b] + W_o[:, H + k - 2]^T dy[b]; k < 2: dyin[b][k] = W_ih[:, k]^T dgi[b]
__global__ __launch_bounds__(NT) void dc_kernel(const float* __restrict__ w_iht, const float* __restrict__ dgi, const float* __restrict__ w_o,
                                                const float* __restrict__ dy, float* __restrict__ dc, float* __restrict__ dyin, int B, int H) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (k >= H + 2) return;
    const int KG = 3 * H / 64;
    const float* w = w_iht + (size_t)k * 3 * H;
    float wr[3 * MAX_KH];
#pragma unroll
    for (int q = 0; q < 3 * MAX_KH; ++q) wr[q] = q < KG ? w[lane + 64 * q] : 0.f;
    const float wo0 = k >= 2 ? w_o[H + k - 2] : 0.f, wo1 = k >= 2 ? w_o[2 * H + H + k - 2] : 0.f;
    for (int b = 0; b < B; ++b) {
        const float* gb = dgi + (size_t)b * 3 * H;
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 3 * MAX_KH; ++q) if (q < KG) s += wr[q] * gb[lane + 64 * q];
        s = wave_sum(s);
        if (lane == 0) {
            if (k >= 2) dc[(size_t)b * H + k - 2] = s + wo0 * dy[b * 2] + wo1 * dy[b * 2 + 1];
            else dyin[b * 2 + k] = s;
        }
    }
}

// K3, one workgroup per clip: d alpha = enc dc (or given), softmax backward, the ReLU mask from P + a, da, dv partial, dP += ...
template <int KH>
__global__ __launch_bounds__(NT) void attn_bwd_kernel(const float* __restrict__ enc, const float* __restrict__ P, const float* __restrict__ a,
                                                      const float* __restrict__ v, const float* __restrict__ alpha,
                                                      const float* __restrict__ dc, const float* __restrict__ dalpha,
                                                      float* __restrict__ dP, float* __restrict__ da, float* __restrict__ dv_acc, int T, int H) {
    extern __shared__ float lds[];
    float* al = lds;          // alpha
    float* ds = lds + T;      // d alpha, then d score
    __shared__ float red[NT / 64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const float* eb = enc + (size_t)b * T * H;
    for (int tau = threadIdx.x; tau < T; tau += NT) al[tau] = alpha[(size_t)b * T + tau];
    if (dalpha) {
        for (int tau = threadIdx.x; tau < T; tau += NT) ds[tau] = dalpha[(size_t)b * T + tau];
    } else {
        float dcr[KH];
#pragma unroll
        for (int k = 0; k < KH; ++k) dcr[k] = dc[(size_t)b * H + lane + 64 * k];
        for (int tau = w; tau < T; tau += NT / 64) {
            const float* er = eb + (size_t)tau * H;
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < KH; ++k) s += dcr[k] * er[lane + 64 * k];
            s = wave_sum(s);
            if (lane == 0) ds[tau] = s;
        }
    }
    __syncthreads();
    float sa = 0.f;
    for (int tau = threadIdx.x; tau < T; tau += NT) sa += al[tau] * ds[tau];
    sa = block_sum(sa, red);
    __syncthreads();
    for (int tau = threadIdx.x; tau < T; tau += NT) ds[tau] = al[tau] * (ds[tau] - sa);
    __syncthreads();
    const float* Pb = P + (size_t)b * T * H;
    float* dPb = dP + (size_t)b * T * H;
    for (int h = threadIdx.x; h < H; h += NT) {
        const float ah = a[(size_t)b * H + h], vh = v[h];
        float dah = 0.f, dvh = 0.f;
        for (int tau = 0; tau < T; ++tau) {
            const float pre = Pb[(size_t)tau * H + h] + ah;
            if (pre > 0.f) {
                const float g = ds[tau] * vh;
                dah += g;
                dvh += ds[tau] * pre;
                dPb[(size_t)tau * H + h] += g;
            }
        }
        da[(size_t)b * H + h] = dah;
        dv_acc[(size_t)b * H + h] += dvh;
    }
}

// K4, one wave per unit k: dh[b][k] = [W_hh^T | W_ah^T][k] . [dgh[b], da[b]] + dhz[b][k]
__global__ __launch_bounds__(NT) void dh_kernel(const float* __restrict__ wt, const float* __restrict__ dgh, const float* __restrict__ da,
                                                const float* __restrict__ dhz, float* __restrict__ dh, int B, int H) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
    if (k >= H) return;
    const int KG = 3 * H / 64, KH = H / 64;
    const float* w = wt + (size_t)k * 4 * H;
    float wg[3 * MAX_KH], wa[MAX_KH];
#pragma unroll
    for (int q = 0; q < 3 * MAX_KH; ++q) wg[q] = q < KG ? w[lane + 64 * q] : 0.f;
#pragma unroll
    for (int q = 0; q < MAX_KH; ++q) wa[q] = q < KH ? w[3 * H + lane + 64 * q] : 0.f;
    for (int b = 0; b < B; ++b) {
        const float* gb = dgh + (size_t)b * 3 * H;
        const float* ab = da + (size_t)b * H;
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 3 * MAX_KH; ++q) if (q < KG) s += wg[q] * gb[lane + 64 * q];
#pragma unroll
        for (int q = 0; q < MAX_KH; ++q) if (q < KH) s += wa[q] * ab[lane + 64 * q];
        s = wave_sum(s);
        if (lane == 0) dh[(size_t)b * H + k] = s + dhz[(size_t)b * H + k];
    }
}

// dW_o [2][2H] = sum_(s,b) dy[s][b]^T [h_{s+1}[b], c_s[b]]; db_o = sum dy; dv = sum_b dv_acc[b].  One thread per output, sequential sums.
__global__ void post_small_kernel(const float* __restrict__ dy, const float* __restrict__ hs, const float* __restrict__ x,
                                  const float* __restrict__ dv_acc, float* __restrict__ dw_o, float* __restrict__ db_o,
                                  float* __restrict__ dv, int N, int B, int H) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < 4 * H) {
        const int o = i / (2 * H), k = i % (2 * H);
        float acc = 0.f;
        for (int n = 0; n < N; ++n) {
            const float xv = k < H ? hs[(size_t)(n + B) * H + k] : x[(size_t)n * (H + 2) + 2 + k - H];
            acc += dy[n * 2 + o] * xv;
        }
        dw_o[i] = acc;
    } else if (i < 4 * H + 2) {
        const int o = i - 4 * H;
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc += dy[n * 2 + o];
        db_o[o] = acc;
    } else if (i < 5 * H + 2) {
        const int h = i - 4 * H - 2;
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += dv_acc[(size_t)b * H + h];
        dv[h] = acc;
    }
}

// d_enc[b][tau][h] += sum_s alpha[s][b][tau] dc[s][b][h]: tiles of 32 frames x 64 units per workgroup, steps staged 32 at a time
constexpr int EG_T = 32, EG_S = 32;
__global__ __launch_bounds__(NT) void enc_grad_kernel(const float* __restrict__ alpha, const float* __restrict__ dc, float* __restrict__ denc,
                                                      int S, int B, int T, int H) {
    __shared__ float al[EG_S][EG_T + 1];
    __shared__ float dl[EG_S][64];
    const int b = blockIdx.z, t0 = blockIdx.x * EG_T, h0 = blockIdx.y * 64;
    const int hl = threadIdx.x & 63, tg = threadIdx.x >> 6;       // 4 groups x 8 frames
    float acc[EG_T / 4];
#pragma unroll
    for (int q = 0; q < EG_T / 4; ++q) acc[q] = 0.f;
    for (int s0 = 0; s0 < S; s0 += EG_S) {
        __syncthreads();
        for (int e = threadIdx.x; e < EG_S * EG_T; e += NT) {
            const int ss = e / EG_T, tt = e % EG_T;
            al[ss][tt] = (s0 + ss < S && t0 + tt < T) ? alpha[((size_t)(s0 + ss) * B + b) * T + t0 + tt] : 0.f;
        }
        for (int e = threadIdx.x; e < EG_S * 64; e += NT) {
            const int ss = e / 64, hh = e % 64;
            dl[ss][hh] = s0 + ss < S ? dc[((size_t)(s0 + ss) * B + b) * H + h0 + hh] : 0.f;
        }
        __syncthreads();
        const int ns = min(EG_S, S - s0);
        for (int ss = 0; ss < ns; ++ss) {
            const float d = dl[ss][hl];
#pragma unroll
            for (int q = 0; q < EG_T / 4; ++q) acc[q] += al[ss][tg * (EG_T / 4) + q] * d;
        }
    }
#pragma unroll
    for (int q = 0; q < EG_T / 4; ++q) {
        const int tau = t0 + tg * (EG_T / 4) + q;
        if (tau < T) denc[((size_t)b * T + tau) * H + h0 + hl] += acc[q];
    }
}

__global__ void sum_halves_kernel(const float* __restrict__ x, float* __restrict__ y, size_t rows, int H) {
    const size_t n = rows * H;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / H, h = i % H;
        y[i] = x[r * 2 * H + h] + x[r * 2 * H + H + h];
    }
}

__global__ void dup_halves_kernel(const float* __restrict__ dy, float* __restrict__ dx, size_t rows, int H) {
    const size_t n = rows * H;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t r = i / H, h = i % H;
        dx[r * 2 * H + h] = dy[i];
        dx[r * 2 * H + H + h] = dy[i];
    }
}

bool dims_ok(int B, int T, int H) { return B >= 1 && T >= 1 && T <= MAX_T && H >= 64 && H % 64 == 0 && H <= 64 * MAX_KH; }

template <int KH>
void launch_attn_fwd(const float* enc, const float* P, const float* a, int lda, const float* v, float* alpha, float* c, int ldc,
                     float* a_save, int B, int T, int H, hipStream_t s) {
    attn_fwd_kernel<KH><<<B, NT, (size_t)T * sizeof(float), s>>>(enc, P, a, lda, v, alpha, c, ldc, a_save, T, H);
}
int attn_fwd(const float* enc, const float* P, const float* a, int lda, const float* v, float* alpha, float* c, int ldc,
             float* a_save, int B, int T, int H, hipStream_t s) {
    switch (H / 64) {
#define M3T_ATTN_F(K) case K: launch_attn_fwd<K>(enc, P, a, lda, v, alpha, c, ldc, a_save, B, T, H, s); break;
        M3T_ATTN_F(1) M3T_ATTN_F(2) M3T_ATTN_F(3) M3T_ATTN_F(4) M3T_ATTN_F(5) M3T_ATTN_F(6) M3T_ATTN_F(7) M3T_ATTN_F(8)
#undef M3T_ATTN_F
        default: return M3T_EINVAL;
    }
    M3T_LAUNCH_CHECK();
    return 0;
}
template <int KH>
void launch_attn_bwd(const float* enc, const float* P, const float* a, const float* v, const float* alpha, const float* dc,
                     const float* dalpha, float* dP, float* da, float* dv_acc, int B, int T, int H, hipStream_t s) {
    attn_bwd_kernel<KH><<<B, NT, (size_t)2 * T * sizeof(float), s>>>(enc, P, a, v, alpha, dc, dalpha, dP, da, dv_acc, T, H);
}
int attn_bwd(const float* enc, const float* P, const float* a, const float* v, const float* alpha, const float* dc,
             const float* dalpha, float* dP, float* da, float* dv_acc, int B, int T, int H, hipStream_t s) {
    switch (H / 64) {
#define M3T_ATTN_B(K) case K: launch_attn_bwd<K>(enc, P, a, v, alpha, dc, dalpha, dP, da, dv_acc, B, T, H, s); break;
        M3T_ATTN_B(1) M3T_ATTN_B(2) M3T_ATTN_B(3) M3T_ATTN_B(4) M3T_ATTN_B(5) M3T_ATTN_B(6) M3T_ATTN_B(7) M3T_ATTN_B(8)
#undef M3T_ATTN_B
        default: return M3T_EINVAL;
    }
    M3T_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int m3t_attdec_fwd(const m3t_attdec_args* p, void* stream) {
    if (!p) return M3T_EINVAL;
    const int B = p->B, T = p->T, L = p->L, H = p->H;
    if (!dims_ok(B, T, H) || L < 1) return M3T_EINVAL;
    if (!p->enc || !p->P || !p->h0 || !p->w_a || !p->v || !p->w_ih || !p->w_hh || !p->b_ih || !p->b_hh || !p->w_o || !p->b_o ||
        !p->out || !p->G || !p->alpha || !p->x || !p->gates || !p->hs || !p->h_last)
        return M3T_EINVAL;
    if (p->tf && !p->trg) return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const size_t BH = (size_t)B * H, BX = (size_t)B * (H + 2);
    hipError_t e = hipMemsetAsync(p->out, 0, sizeof(float) * B * L * 2, s);
    if (e != hipSuccess) return (int)e;
    const bool save = p->save != 0;
    fwd_init_kernel<<<cdiv((int)BH, NT), NT, 0, s>>>(p->y0, p->h0, L > 1 ? p->x : nullptr, p->hs, B, H);
    M3T_LAUNCH_CHECK();
    const int proj_rows = 4 * H + 2;
    proj_kernel<<<cdiv(proj_rows, NT / 64), NT, 0, s>>>(p->hs, nullptr, p->w_hh, p->b_hh, p->w_a, p->w_o, p->b_o, p->G, p->out, nullptr,
                                                        p->trg, p->tf, 0, B, L, H);
    M3T_LAUNCH_CHECK();
    for (int t = 1; t < L; ++t) {
        const int st = t - 1;
        float* x_t = p->x + (save ? (size_t)st : (size_t)(st & 1)) * BX;
        float* x_n = t + 1 < L ? p->x + (save ? (size_t)t : (size_t)(t & 1)) * BX : nullptr;
        const float* h_p = p->hs + (save ? (size_t)st : (size_t)(st & 1)) * BH;
        float* h_t = p->hs + (save ? (size_t)t : (size_t)(t & 1)) * BH;
        float* al = p->alpha + (save ? (size_t)st * B * T : 0);
        float* gt = p->gates + (save ? (size_t)st * 4 * BH : 0);
        float* as = (save && p->a_save) ? p->a_save + (size_t)st * BH : nullptr;
        int rc = attn_fwd(p->enc, p->P, p->G + 3 * H, 4 * H, p->v, al, x_t + 2, H + 2, as, B, T, H, s);
        if (rc) return rc;
        cell_fwd_kernel<<<cdiv(H, NT / 64), NT, 0, s>>>(p->G, x_t, H, p->w_ih, p->b_ih, h_p, h_t, gt, B);
        M3T_LAUNCH_CHECK();
        proj_kernel<<<cdiv(proj_rows, NT / 64), NT, 0, s>>>(h_t, x_t, p->w_hh, p->b_hh, p->w_a, p->w_o, p->b_o, p->G, p->out, x_n,
                                                            p->trg, p->tf, t, B, L, H);
        M3T_LAUNCH_CHECK();
    }
    const float* h_fin = p->hs + (save ? (size_t)(L - 1) : (size_t)((L - 1) & 1)) * BH;
    e = hipMemcpyAsync(p->h_last, h_fin, sizeof(float) * BH, hipMemcpyDeviceToDevice, s);
    return e == hipSuccess ? 0 : (int)e;
}

extern "C" int m3t_attdec_bwd(const m3t_attdec_args* p, void* stream) {
    if (!p) return M3T_EINVAL;
    const int B = p->B, T = p->T, L = p->L, H = p->H;
    if (!dims_ok(B, T, H) || L < 2 || !p->save) return M3T_EINVAL;
    if (!p->dout || !p->dgi || !p->dgh || !p->dc || !p->da || !p->dy || !p->dP || !p->dv_acc || !p->dh || !p->w_iht || !p->wt ||
        !p->dyin || !p->dhz || !p->a_save)
        return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const size_t BH = (size_t)B * H;
    bwd_prep_kernel<<<1024, NT, 0, s>>>(p->w_ih, p->w_hh, p->w_a, p->w_iht, p->wt, H);
    M3T_LAUNCH_CHECK();
    hipError_t e = hipMemsetAsync(p->dP, 0, sizeof(float) * B * T * H, s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dv_acc, 0, sizeof(float) * BH, s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dyin, 0, sizeof(float) * B * 2, s);
    if (e == hipSuccess)
        e = p->dh_last ? hipMemcpyAsync(p->dh, p->dh_last, sizeof(float) * BH, hipMemcpyDeviceToDevice, s)
                       : hipMemsetAsync(p->dh, 0, sizeof(float) * BH, s);
    if (e != hipSuccess) return (int)e;
    for (int t = L - 1; t >= 1; --t) {
        const size_t st = t - 1;
        float* dgi = p->dgi + st * 3 * BH;
        float* dgh = p->dgh + st * 3 * BH;
        float* dc = p->dc + st * BH;
        float* da = p->da + st * BH;
        float* dy = p->dy + st * B * 2;
        cell_bwd_kernel<<<cdiv((int)BH, NT), NT, 0, s>>>(p->dout, p->dyin, p->trg ? p->tf : nullptr, p->w_o, p->gates + st * 4 * BH,
                                                         p->hs + st * BH, p->dh, dgi, dgh, p->dhz, dy, t, B, L, H);
        M3T_LAUNCH_CHECK();
        dc_kernel<<<cdiv(H + 2, NT / 64), NT, 0, s>>>(p->w_iht, dgi, p->w_o, dy, dc, p->dyin, B, H);
        M3T_LAUNCH_CHECK();
        int rc = attn_bwd(p->enc, p->P, p->a_save + st * BH, p->v, p->alpha + st * B * T, dc, nullptr, p->dP, da, p->dv_acc, B, T, H, s);
        if (rc) return rc;
        dh_kernel<<<cdiv(H, NT / 64), NT, 0, s>>>(p->wt, dgh, da, p->dhz, p->dh, B, H);
        M3T_LAUNCH_CHECK();
    }
    if (p->dy0) {
        e = hipMemcpyAsync(p->dy0, p->dyin, sizeof(float) * B * 2, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

extern "C" int m3t_attdec_post(const m3t_attdec_args* p, float* dw_o, float* db_o, float* dv, float* d_enc, void* stream) {
    if (!p) return M3T_EINVAL;
    const int B = p->B, T = p->T, L = p->L, H = p->H;
    if (!dims_ok(B, T, H) || L < 2 || !p->dy || !p->hs || !p->x || !p->dv_acc || !p->alpha || !p->dc) return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int S = L - 1;
    if (dw_o || db_o || dv) {
        if (!dw_o || !db_o || !dv) return M3T_EINVAL;
        post_small_kernel<<<cdiv(5 * H + 2, NT), NT, 0, s>>>(p->dy, p->hs, p->x, p->dv_acc, dw_o, db_o, dv, S * B, B, H);
        M3T_LAUNCH_CHECK();
    }
    if (d_enc) {
        enc_grad_kernel<<<dim3(cdiv(T, EG_T), H / 64, B), NT, 0, s>>>(p->alpha, p->dc, d_enc, S, B, T, H);
        M3T_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int m3t_attdec_attn_fwd(const float* enc, const float* P, const float* a, int lda, const float* v, float* alpha, float* c,
                                   int B, int T, int H, void* stream) {
    if (!dims_ok(B, T, H) || !enc || !P || !a || !v || !alpha || lda < H) return M3T_EINVAL;
    return attn_fwd(enc, P, a, lda, v, alpha, c, H, nullptr, B, T, H, (hipStream_t)stream);
}

extern "C" int m3t_attdec_attn_bwd(const float* enc, const float* P, const float* a, const float* v, const float* alpha,
                                   const float* dalpha, float* dP, float* da, float* dv_acc, int B, int T, int H, void* stream) {
    if (!dims_ok(B, T, H) || !enc || !P || !a || !v || !alpha || !dalpha || !dP || !da || !dv_acc) return M3T_EINVAL;
    return attn_bwd(enc, P, a, v, alpha, nullptr, dalpha, dP, da, dv_acc, B, T, H, (hipStream_t)stream);
}

extern "C" int m3t_attdec_sum_halves(const float* x, float* y, size_t rows, int H, void* stream) {
    if (!x || !y || H <= 0) return M3T_EINVAL;
    if (rows == 0) return 0;
    const size_t n = rows * H;
    const int grid = (int)((n + NT - 1) / NT < 4096 ? (n + NT - 1) / NT : 4096);
    sum_halves_kernel<<<grid, NT, 0, (hipStream_t)stream>>>(x, y, rows, H);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_attdec_dup_halves(const float* dy, float* dx, size_t rows, int H, void* stream) {
    if (!dy || !dx || H <= 0) return M3T_EINVAL;
    if (rows == 0) return 0;
    const size_t n = rows * H;
    const int grid = (int)((n + NT - 1) / NT < 4096 ? (n + NT - 1) / NT : 4096);
    dup_halves_kernel<<<grid, NT, 0, (hipStream_t)stream>>>(dy, dx, rows, H);
    M3T_LAUNCH_CHECK();
    return 0;
}
