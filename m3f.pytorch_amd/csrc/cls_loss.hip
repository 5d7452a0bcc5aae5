// Loss end of the two pre-training tasks (reference models/vox2_model.py:53-67, models/audioset_model.py:34-49): temporal pooling of the
// per-frame logits [B,T,C] to per-clip logits [B,C], softmax cross-entropy (VoxCeleb2, 1000 identities) or binary cross-entropy with logits
// (AudioSet, 527 labels), the top-1 statistic and the gradient.  HBM- and launch-bound: threads run along C (coalesced whatever C is: no
// alignment or divisibility assumption, plain 4-byte accesses), one workgroup per clip for the loss, row reductions in fp64 in a fixed order
// (wavefront butterflies, then the four waves in wave order), no atomics: the same bits run to run.  The mean over clips is a second,
// one-workgroup launch that adds the per-clip partials in clip order.
#include "common.h"
#include <cmath>

namespace {

constexpr int CT = 256;          // threads per workgroup: four waves

// ---- pooling over T of one (clip, class) column; z points at frame 0 of the column, frames are `stride` floats apart ----------------------
// max: the first maximum in time order, NaN above every number (the first NaN stays), as torch.max(dim=1)
__device__ __forceinline__ float pool_max(const float* __restrict__ z, int T, size_t stride, int& arg) {
    float mx = z[0];
    int am = 0;
    for (int t = 1; t < T; ++t) {
        const float v = z[(size_t)t * stride];
        if (m3t_nan_gt(v, mx)) { mx = v; am = t; }
    }
    arg = am;
    return mx;
}
__device__ __forceinline__ float pool_mean(const float* __restrict__ z, int T, size_t stride) {
    double s = 0.0;
    for (int t = 0; t < T; ++t) s += (double)z[(size_t)t * stride];
    return (float)(s / (double)T);
}
// what one frame of the column receives of the pooled gradient g (gT = g / T, computed once per column)
__device__ __forceinline__ float spread(int mode, int t, int arg, float g, float gT) { return mode ? gT : (t == arg ? g : 0.f); }

__global__ __launch_bounds__(CT) void tpool_fwd_kernel(const float* __restrict__ z, int T, int C, size_t n, int mode,
                                                       float* __restrict__ pooled, int* __restrict__ arg) {
    const size_t i = (size_t)blockIdx.x * CT + threadIdx.x;          // (b, c)
    if (i >= n) return;
    const size_t b = i / (size_t)C, c = i - b * (size_t)C;
    const float* col = z + b * (size_t)T * C + c;
    if (mode) {
        pooled[i] = pool_mean(col, T, (size_t)C);
    } else {
        int am;
        pooled[i] = pool_max(col, T, (size_t)C, am);
        arg[i] = am;
    }
}

__global__ __launch_bounds__(CT) void tpool_bwd_kernel(const float* __restrict__ dpooled, const int* __restrict__ arg, int T, int C, size_t n,
                                                       int mode, float* __restrict__ dz) {
    const size_t i = (size_t)blockIdx.x * CT + threadIdx.x;          // (b, t, c): every element of dz written once, no memset
    if (i >= n) return;
    const size_t bt = i / (size_t)C, c = i - bt * (size_t)C;
    const size_t b = bt / (size_t)T;
    const int t = (int)(bt - b * (size_t)T);
    const size_t j = b * (size_t)C + c;
    const float g = dpooled[j];
    dz[i] = spread(mode, t, mode ? 0 : arg[j], g, g / (float)T);
}

// ---- block-wide reductions of a 256-thread workgroup, the same order in every run ----------------------------------------------------------
__device__ __forceinline__ double block_sum_d(double v, double* red /* LDS [4] */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
// (value, index) argmax: the larger value, NaN above all, the lower index on a tie -- a total order, so the butterfly leaves every lane with the winner
__device__ __forceinline__ void block_argmax(float& mx, int& am, float* rv, int* ri /* LDS [4] each */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(mx, o, 64);
        const int oi = __shfl_xor(am, o, 64);
        if (m3t_argmax_wins(ov, oi, mx, am)) { mx = ov; am = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = mx; ri[threadIdx.x >> 6] = am; }
    __syncthreads();
    mx = rv[0]; am = ri[0];
#pragma unroll
    for (int w = 1; w < CT / 64; ++w)
        if (m3t_argmax_wins(rv[w], ri[w], mx, am)) { mx = rv[w]; am = ri[w]; }
}

// One workgroup per clip.  POOL: `in` is z [B,T,C]; the workgroup pools its clip into pooled [B,C] (and arg), reduces the row and writes
// dL/dz into `dout` [B,T,C].  Otherwise `in` is the per-clip logits [B,C] and `dout` [B,C] receives dL/dlogits.  A thread owns the classes
// tid, tid + 256, ... in every phase, so it re-reads only what it wrote itself.  The exponentials and logarithms are fp64: ~4 per thread at
// C = 1000, nothing beside the launch, and the loss and every gradient element are then the float nearest to the exact value.
// part [B][2] (fp64): the clip's loss term and its top-1 hit.
template <bool POOL>
__global__ __launch_bounds__(CT) void cls_loss_kernel(const float* __restrict__ in, int B, int T, int C, int mode, int kind,
                                                      const int64_t* __restrict__ labels, const float* __restrict__ targets,
                                                      float* __restrict__ pooled, int* __restrict__ arg, double* __restrict__ part,
                                                      float* __restrict__ correct, float* __restrict__ dout) {
    __shared__ double red[4];
    __shared__ float rv[4];
    __shared__ int ri[4];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const float* x;
    if (POOL) {
        const float* zb = in + b * (size_t)T * C;
        for (int c = tid; c < C; c += CT) {
            if (mode) {
                pooled[b * (size_t)C + c] = pool_mean(zb + c, T, (size_t)C);
            } else {
                int a;
                pooled[b * (size_t)C + c] = pool_max(zb + c, T, (size_t)C, a);
                arg[b * (size_t)C + c] = a;
            }
        }
        x = pooled + b * (size_t)C;
    } else {
        x = in + b * (size_t)C;
    }
    // top-1: the first maximum of the row
    float mx = -INFINITY;
    int am = 0x7fffffff;
    for (int c = tid; c < C; c += CT) {
        const float v = x[c];
        if (m3t_argmax_wins(v, c, mx, am)) { mx = v; am = c; }
    }
    block_argmax(mx, am, rv, ri);
    const float* tg = kind ? targets + b * (size_t)C : nullptr;
    const double nan_d = (double)__builtin_nanf("");
    double term, hit;
    if (kind == 0) {
        const long long lab = (long long)labels[b];
        const bool lab_ok = lab >= 0 && lab < (long long)C;              // a label outside the row is never used as an index
        double s = 0.0;
        for (int c = tid; c < C; c += CT) s += exp((double)x[c] - (double)mx);
        s = block_sum_d(s, red);
        term = lab_ok ? (log(s) + (double)mx) - (double)x[lab_ok ? lab : 0] : nan_d;
        hit = (lab_ok && (long long)am == lab) ? 1.0 : 0.0;
        const double inv_s = 1.0 / s, inv_b = 1.0 / (double)B;
        for (int c = tid; c < C; c += CT) {
            const double p = exp((double)x[c] - (double)mx) * inv_s;
            const float g = lab_ok ? (float)((p - ((long long)c == lab ? 1.0 : 0.0)) * inv_b) : __builtin_nanf("");
            if (POOL) {
                const float gT = g / (float)T;
                const int a = mode ? 0 : arg[b * (size_t)C + c];
                for (int t = 0; t < T; ++t) dout[(b * (size_t)T + t) * C + c] = spread(mode, t, a, g, gT);
            } else {
                dout[b * (size_t)C + c] = g;
            }
        }
    } else {
        double s = 0.0;
        const double inv_n = 1.0 / ((double)B * (double)C);
        for (int c = tid; c < C; c += CT) {
            const double v = (double)x[c], y = (double)tg[c];
            const double e = exp(-fabs(v));
            s += (v > 0.0 ? v : 0.0) - v * y + log1p(e);                 // max(x, 0) - x y + log1p(exp(-|x|)); a NaN stays one through x y
            const double sg = v >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
            const float g = (float)(((v != v ? v : sg) - y) * inv_n);
            if (POOL) {
                const float gT = g / (float)T;
                const int a = mode ? 0 : arg[b * (size_t)C + c];
                for (int t = 0; t < T; ++t) dout[(b * (size_t)T + t) * C + c] = spread(mode, t, a, g, gT);
            } else {
                dout[b * (size_t)C + c] = g;
            }
        }
        term = block_sum_d(s, red);
        hit = (double)tg[am];                                            // am < C always: C >= 1 and every class was compared
    }
    if (tid == 0) {
        part[2 * b] = term;
        part[2 * b + 1] = hit;
        correct[b] = (float)hit;
    }
}

// the mean over clips: lane l adds its contiguous run of clips in clip order, lane 0 adds the 64 runs in lane order
__global__ __launch_bounds__(64) void cls_finish_kernel(const double* __restrict__ part, int B, double denom, float* __restrict__ out) {
    __shared__ double sl[64], sc[64];
    const int l = threadIdx.x, per = (B + 63) / 64;
    double a = 0.0, h = 0.0;
    for (int b = l * per; b < min(B, (l + 1) * per); ++b) { a += part[2 * (size_t)b]; h += part[2 * (size_t)b + 1]; }
    sl[l] = a; sc[l] = h;
    __syncthreads();
    if (l == 0) {
        a = 0.0; h = 0.0;
        for (int i = 0; i < 64; ++i) { a += sl[i]; h += sc[i]; }
        out[0] = (float)(a / denom);
        out[1] = (float)h;
    }
}

bool dims_ok(int B, int T, int C) { return B >= 1 && T >= 1 && C >= 1; }

int loss_launch(bool pool, const float* in, int B, int T, int C, int mode, int kind, const void* target, float* pooled, int* arg,
                float* out_scalars, float* correct, float* dout, void* ws, size_t ws_bytes, hipStream_t s) {
    if (!dims_ok(B, T, C) || (mode != 0 && mode != 1) || (kind != 0 && kind != 1)) return M3T_EINVAL;
    if (!in || !target || !out_scalars || !correct || !dout || !ws) return M3T_EINVAL;
    if (pool && (!pooled || (mode == 0 && !arg))) return M3T_EINVAL;
    if (ws_bytes < m3t_cls_loss_ws_bytes(B) || ((uintptr_t)ws % 8) != 0) return M3T_EINVAL;
    double* part = reinterpret_cast<double*>(ws);
    const int64_t* labels = kind == 0 ? reinterpret_cast<const int64_t*>(target) : nullptr;
    const float* targets = kind == 1 ? reinterpret_cast<const float*>(target) : nullptr;
    if (pool)
        cls_loss_kernel<true><<<B, CT, 0, s>>>(in, B, T, C, mode, kind, labels, targets, pooled, arg, part, correct, dout);
    else
        cls_loss_kernel<false><<<B, CT, 0, s>>>(in, B, 1, C, 0, kind, labels, targets, nullptr, nullptr, part, correct, dout);
    M3T_LAUNCH_CHECK();
    cls_finish_kernel<<<1, 64, 0, s>>>(part, B, kind ? (double)B * (double)C : (double)B, out_scalars);
    M3T_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int m3t_tpool_fwd(const float* z, int B, int T, int C, int mode, float* pooled, int* arg, void* stream) {
    if (!dims_ok(B, T, C) || (mode != 0 && mode != 1) || !z || !pooled || (mode == 0 && !arg)) return M3T_EINVAL;
    const size_t n = (size_t)B * C, blocks = (n + CT - 1) / CT;
    if (blocks > 0x7fffffffu) return M3T_EINVAL;
    tpool_fwd_kernel<<<(unsigned)blocks, CT, 0, (hipStream_t)stream>>>(z, T, C, n, mode, pooled, arg);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_tpool_bwd(const float* dpooled, const int* arg, int B, int T, int C, int mode, float* dz, void* stream) {
    if (!dims_ok(B, T, C) || (mode != 0 && mode != 1) || !dpooled || !dz || (mode == 0 && !arg)) return M3T_EINVAL;
    const size_t n = (size_t)B * T * C, blocks = (n + CT - 1) / CT;
    if (blocks > 0x7fffffffu) return M3T_EINVAL;
    tpool_bwd_kernel<<<(unsigned)blocks, CT, 0, (hipStream_t)stream>>>(dpooled, arg, T, C, n, mode, dz);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t m3t_cls_loss_ws_bytes(int B) { return B > 0 ? (size_t)B * 2 * sizeof(double) : 0; }

extern "C" int m3t_cls_loss(const float* logits, int B, int C, int kind, const void* target, float* out_scalars, float* correct,
                            float* dlogits, void* ws, size_t ws_bytes, void* stream) {
    return loss_launch(false, logits, B, 1, C, 0, kind, target, nullptr, nullptr, out_scalars, correct, dlogits, ws, ws_bytes,
                       (hipStream_t)stream);
}

extern "C" int m3t_tpool_cls_loss(const float* z, int B, int T, int C, int mode, int kind, const void* target, float* pooled, int* arg,
                                  float* out_scalars, float* correct, float* dz, void* ws, size_t ws_bytes, void* stream) {
    return loss_launch(true, z, B, T, C, mode, kind, target, pooled, arg, out_scalars, correct, dz, ws, ws_bytes, (hipStream_t)stream);
}
