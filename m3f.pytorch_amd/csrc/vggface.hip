// Channels-last operators of the VGGFace front-end.  Reference: models/vggface.py:45-50 -- every Conv2d(3x3, pad 1) is followed by a plain ReLU
// (no normalisation) and every block ends in max_pool2d(2, 2, 0, ceil_mode=True).  The convolutions are the tap walks of csrc/conv3d.hip
// with a unit time tap (bias in the walk); what the chain of csrc/stem_cl.hip lacked is
//   * a plain ReLU over rows [M][C] (stem_cl.hip only has it fused with BatchNorm): forward may run in place; backward writes dx = dy where
//     y > 0 AND the column sums of dx -- the bias gradient of the convolution in front -- from the same pass
//   * ReLU + a 2 x 2 / stride 2 / no padding max pooling with ceil_mode (7 -> 4, 25 -> 13, 13 -> 7: a ragged last window covers only the
//     positions inside the frame) as ONE operator: relu(x) at full resolution is neither written nor kept; forward keeps the pooled value and
//     the winner byte, backward is a gather over the input positions (no atomics) from d(yp), yp and the winner bytes alone
// Rows are swept in 16-byte quads (C % 4 == 0, any C up to 1024: C / 4 need not divide the block); a block owns a contiguous chunk of rows, its
// threads (row group g, quad q) keep their four channels for the whole chunk, column sums are fp64 from the first add to the last (thread ->
// LDS in group order -> block partial -> the blocks' partials in a fixed order): deterministic, no float atomics.  NaN as torch: relu(NaN) = NaN, a NaN wins
// its window, and the ReLU's backward lets dy through where y is NaN (threshold_backward: y <= 0 ? 0 : dy).
#include "cl_rows.h"

namespace {

constexpr int VG_TH = CL_TH;
constexpr int VG_MAX_CHUNKS = 2048;

// torch.relu: v > 0 ? v : (v != v ? v : 0)
__device__ __forceinline__ float vg_relu(float v) { return v > 0.f ? v : (v != v ? v : 0.f); }
// the ReLU's gradient mask as torch's threshold_backward: 0 where y <= 0, dy elsewhere (a NaN y lets dy through)
__device__ __forceinline__ float vg_mask(float dy, float y) { return y <= 0.f ? 0.f : dy; }

static int vg_chunks(size_t M, int C) {
    // ~16 quads per thread and chunk, at most VG_MAX_CHUNKS chunks, at least one row per chunk
    const size_t groups = (size_t)(VG_TH / (C / 4));
    size_t c = (M + groups * 16 - 1) / (groups * 16);
    if (c < 1) c = 1;
    if (c > (size_t)VG_MAX_CHUNKS) c = VG_MAX_CHUNKS;
    return (int)c;
}

static int vg_grid(size_t total4) {
    size_t b = (total4 + (size_t)VG_TH * 8 - 1) / ((size_t)VG_TH * 8);
    if (b < 1) b = 1;
    if (b > 2048) b = 2048;
    return (int)b;
}

// y = relu(x) over total4 quads (y may be x: every quad is read and written by the same thread)
__global__ __launch_bounds__(VG_TH) void vg_relu_fwd_kernel(const float* x, float* y, size_t total4, unsigned long long* __restrict__ slot) {
    __shared__ float red4[4];
    float mx = 0.f;
    for (size_t i = (size_t)blockIdx.x * VG_TH + threadIdx.x; i < total4; i += (size_t)gridDim.x * VG_TH) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        const float o[4] = {vg_relu(v.x), vg_relu(v.y), vg_relu(v.z), vg_relu(v.w)};
        reinterpret_cast<float4*>(y)[i] = make_float4(o[0], o[1], o[2], o[3]);
        if (slot) mx = cl_max4(mx, o);
    }
    if (slot) m3t_block_raise_slot(slot, mx, red4);
}

// a block's column sums: red [groups][C] doubles in LDS -> partial[block][C], the groups in index order
__device__ __forceinline__ void vg_block_colsum(const double (&cs)[4], int g, int q, int groups, int C, double* red, double* __restrict__ partial) {
    if (g < groups) {
#pragma unroll
        for (int e = 0; e < 4; ++e) red[(size_t)g * C + 4 * q + e] = cs[e];
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += VG_TH) {
        double t = 0.0;
        for (int k = 0; k < groups; ++k) t += red[(size_t)k * C + c];
        partial[(size_t)blockIdx.x * C + c] = t;
    }
}

// dx = dy where y > 0; partial[chunk][C] = the chunk's column sums of dx (when asked for).  dx may be dy.
__global__ __launch_bounds__(VG_TH) void vg_relu_bwd_kernel(const float* dy, const float* __restrict__ y, float* dx, size_t M, int C,
                                                           size_t rows_per_chunk, unsigned long long* __restrict__ slot,
                                                           double* __restrict__ partial) {
    extern __shared__ double red[];
    __shared__ float red4[4];
    const int c4n = C >> 2, groups = VG_TH / c4n;
    const int q = threadIdx.x % c4n, g = threadIdx.x / c4n;
    const size_t r0 = (size_t)blockIdx.x * rows_per_chunk;
    const size_t r1 = r0 + rows_per_chunk < M ? r0 + rows_per_chunk : M;
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    float mx = 0.f;
    if (g < groups) {
        for (size_t r = r0 + g; r < r1; r += groups) {
            const size_t i = r * (size_t)c4n + q;
            const float4 d = reinterpret_cast<const float4*>(dy)[i];
            const float4 v = reinterpret_cast<const float4*>(y)[i];
            const float o[4] = {vg_mask(d.x, v.x), vg_mask(d.y, v.y), vg_mask(d.z, v.z), vg_mask(d.w, v.w)};
            reinterpret_cast<float4*>(dx)[i] = make_float4(o[0], o[1], o[2], o[3]);
            if (slot) mx = cl_max4(mx, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) cs[e] += (double)o[e];
        }
    }
    if (partial) vg_block_colsum(cs, g, q, groups, C, red, partial);
    if (slot) m3t_block_raise_slot(slot, mx, red4);          // (uniform: every thread of the block gets here)
}

// out[c] = sum over the chunks' partials in a fixed order: 16 channels per block, the chunks in 16 interleaved phases -- thread (channel, phase)
// adds every sixteenth chunk (eight loads in flight, combined in index order), the phase sums are combined in phase order.  (One thread per
// channel walking 2048 chunks is a chain of 2048 dependent-latency loads: ~1 ms per layer.)
constexpr int VG_FC = 16, VG_FP = VG_TH / VG_FC;
__global__ __launch_bounds__(VG_TH) void vg_colsum_final_kernel(const double* __restrict__ partial, int nchunks, int C, float* __restrict__ out) {
    __shared__ double red[VG_FP][VG_FC];
    const int cl = threadIdx.x % VG_FC, ph = threadIdx.x / VG_FC, c = blockIdx.x * VG_FC + cl;
    double t = 0.0;
    if (c < C) {
        double t8[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int k = ph;
        for (; k + 7 * VG_FP < nchunks; k += 8 * VG_FP) {
#pragma unroll
            for (int u = 0; u < 8; ++u) t8[u] += partial[(size_t)(k + u * VG_FP) * C + c];
        }
        for (; k < nchunks; k += VG_FP) t8[0] += partial[(size_t)k * C + c];
        t = ((t8[0] + t8[1]) + (t8[2] + t8[3])) + ((t8[4] + t8[5]) + (t8[6] + t8[7]));
    }
    red[ph][cl] = t;
    __syncthreads();
    if (ph == 0 && c < C) {
        double s = 0.0;
        for (int k = 0; k < VG_FP; ++k) s += red[k][cl];
        out[c] = (float)s;
    }
}

struct VGPool { int H, W, Ho, Wo, C; };

// row index -> (frame, row, column) of a P x A x B grid; 32-bit division where the index fits (a 64-bit division is ~10 x the instructions)
__device__ __forceinline__ void vg_decode(size_t r, int A, int B, size_t& p, int& a, int& b) {
    if (r <= 0xffffffffull) {
        unsigned rr = (unsigned)r;
        b = (int)(rr % (unsigned)B); rr /= (unsigned)B;
        a = (int)(rr % (unsigned)A);
        p = rr / (unsigned)A;
    } else {
        cl_decode(r, A, B, p, a, b);
    }
}

// thread = (output position, quad): relu inside the window loop, the first maximum in window order wins, NaN wins; a ragged window (ceil_mode)
// covers only the positions inside the frame; winner byte = dh * 2 + dw
__global__ __launch_bounds__(VG_TH) void vg_relu_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ yp, unsigned char* __restrict__ win,
                                                                size_t total4, VGPool g, unsigned long long* __restrict__ slot) {
    __shared__ float red4[4];
    const int c4n = g.C >> 2;
    float mx = 0.f;
    for (size_t i = (size_t)blockIdx.x * VG_TH + threadIdx.x; i < total4; i += (size_t)gridDim.x * VG_TH) {
        int q, ho, wo;
        size_t p, r;
        if (i <= 0xffffffffull) { q = (int)((unsigned)i % (unsigned)c4n); r = (unsigned)i / (unsigned)c4n; }
        else { q = (int)(i % (size_t)c4n); r = i / (size_t)c4n; }
        vg_decode(r, g.Ho, g.Wo, p, ho, wo);
        float best[4] = {0.f, 0.f, 0.f, 0.f};
        int bi[4] = {0, 0, 0, 0};
        bool first = true;
#pragma unroll
        for (int dh = 0; dh < 2; ++dh) {
            const int h = 2 * ho + dh;
            if (h >= g.H) continue;
#pragma unroll
            for (int dw = 0; dw < 2; ++dw) {
                const int w = 2 * wo + dw;
                if (w >= g.W) continue;
                const float4 v = *reinterpret_cast<const float4*>(x + ((p * g.H + h) * g.W + w) * (size_t)g.C + 4 * q);
                const float ve[4] = {vg_relu(v.x), vg_relu(v.y), vg_relu(v.z), vg_relu(v.w)};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (first || m3t_nan_gt(ve[e], best[e])) { best[e] = ve[e]; bi[e] = dh * 2 + dw; }
                first = false;
            }
        }
        reinterpret_cast<float4*>(yp)[i] = make_float4(best[0], best[1], best[2], best[3]);
        reinterpret_cast<uchar4*>(win)[i] = make_uchar4((unsigned char)bi[0], (unsigned char)bi[1], (unsigned char)bi[2], (unsigned char)bi[3]);
        if (slot) mx = cl_max4(mx, best);
    }
    if (slot) m3t_block_raise_slot(slot, mx, red4);
}

// thread = (input position, quad) of a chunk of input rows: dx = d(yp) of the position's window where it won and yp > 0, else 0 (positions no
// window covers -- floor mode, odd H / W -- get 0)
__global__ __launch_bounds__(VG_TH) void vg_relu_pool_bwd_kernel(const float* __restrict__ dyp, const float* __restrict__ yp,
                                                                const unsigned char* __restrict__ win, float* __restrict__ dx, size_t M, VGPool g,
                                                                size_t rows_per_chunk, unsigned long long* __restrict__ slot,
                                                                double* __restrict__ partial) {
    extern __shared__ double red[];
    __shared__ float red4[4];
    const int C = g.C, c4n = C >> 2, groups = VG_TH / c4n;
    const int q = threadIdx.x % c4n, gi = threadIdx.x / c4n;
    const size_t r0 = (size_t)blockIdx.x * rows_per_chunk;
    const size_t r1 = r0 + rows_per_chunk < M ? r0 + rows_per_chunk : M;
    double cs[4] = {0.0, 0.0, 0.0, 0.0};
    float mx = 0.f;
    if (gi < groups) {
        for (size_t r = r0 + gi; r < r1; r += groups) {
            int h, w;
            size_t p;
            vg_decode(r, g.H, g.W, p, h, w);
            const int ho = h >> 1, wo = w >> 1;
            float o[4] = {0.f, 0.f, 0.f, 0.f};
            if (ho < g.Ho && wo < g.Wo) {
                const size_t s = ((p * g.Ho + ho) * g.Wo + wo) * (size_t)c4n + q;
                const float4 d = reinterpret_cast<const float4*>(dyp)[s];
                const float4 v = reinterpret_cast<const float4*>(yp)[s];
                const uchar4 b = reinterpret_cast<const uchar4*>(win)[s];
                const int me = (h & 1) * 2 + (w & 1);
                if (b.x == me) o[0] = vg_mask(d.x, v.x);
                if (b.y == me) o[1] = vg_mask(d.y, v.y);
                if (b.z == me) o[2] = vg_mask(d.z, v.z);
                if (b.w == me) o[3] = vg_mask(d.w, v.w);
            }
            reinterpret_cast<float4*>(dx)[r * (size_t)c4n + q] = make_float4(o[0], o[1], o[2], o[3]);
            if (slot) mx = cl_max4(mx, o);
#pragma unroll
            for (int e = 0; e < 4; ++e) cs[e] += (double)o[e];
        }
    }
    if (partial) vg_block_colsum(cs, gi, q, groups, C, red, partial);
    if (slot) m3t_block_raise_slot(slot, mx, red4);
}

static bool vg_shape_ok(size_t M, int C) { return M > 0 && C > 0 && C % 4 == 0 && C <= 1024; }
static size_t vg_ws_bytes(size_t M, int C) { return (size_t)vg_chunks(M, C) * (size_t)C * sizeof(double); }      // fp64 chunk partials [chunks][C]
static bool vgpool_geom(int H, int W, int C, int ceil_mode, VGPool& g) {
    if (H < 1 || W < 1) return false;
    g.H = H; g.W = W; g.C = C;
    g.Ho = ceil_mode ? (H + 1) / 2 : H / 2; g.Wo = ceil_mode ? (W + 1) / 2 : W / 2;
    return g.Ho >= 1 && g.Wo >= 1;
}

// A backward pass over M rows in chunks: the caller's launch(nch, lds_bytes, rows_per_chunk, partial) writes dx and, when dx_colsum is asked
// for, the chunks' fp64 column sums into ws; then the chunks are folded into dx_colsum.
template <class LAUNCH>
int vg_bwd(size_t M, int C, float* dx_colsum, float* ws, size_t ws_bytes, hipStream_t s, LAUNCH launch) {
    if (dx_colsum && !cl_ws_ok(ws, ws_bytes, vg_ws_bytes(M, C))) return M3T_EINVAL;
    const int nch = vg_chunks(M, C), groups = VG_TH / (C / 4);
    double* partial = dx_colsum ? reinterpret_cast<double*>(ws) : nullptr;
    launch(nch, (size_t)groups * C * sizeof(double), (M + nch - 1) / nch, partial);
    M3T_LAUNCH_CHECK();
    if (dx_colsum) {
        vg_colsum_final_kernel<<<cdiv(C, VG_FC), VG_TH, 0, s>>>(partial, nch, C, dx_colsum);
        M3T_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

// the workspace of the backward passes' column sums
extern "C" size_t m3t_relu_cl_ws_bytes(size_t M, int C) {
    return vg_shape_ok(M, C) ? vg_ws_bytes(M, C) : 0;
}

extern "C" int m3t_relu_cl_fwd(const float* x, size_t M, int C, float* y, void* stream) {
    unsigned long long* slot = m3t_take_amax_out();
    if (!vg_shape_ok(M, C) || !al16(x) || !al16(y)) return M3T_EINVAL;
    const size_t total4 = M * (size_t)(C / 4);
    vg_relu_fwd_kernel<<<vg_grid(total4), VG_TH, 0, (hipStream_t)stream>>>(x, y, total4, slot);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_relu_cl_bwd(const float* dy, const float* y, size_t M, int C, float* dx, float* dx_colsum, float* ws, size_t ws_bytes,
                               void* stream) {
    unsigned long long* slot = m3t_take_amax_out();
    if (!vg_shape_ok(M, C) || !al16(dy) || !al16(y) || !al16(dx)) return M3T_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    return vg_bwd(M, C, dx_colsum, ws, ws_bytes, s, [&](int nch, size_t lds, size_t rpc, double* partial) {
        vg_relu_bwd_kernel<<<nch, VG_TH, lds, s>>>(dy, y, dx, M, C, rpc, slot, partial);
    });
}

extern "C" int m3t_relu_pool_cl_fwd(const float* x, size_t P, int H, int W, int C, int ceil_mode, float* yp, unsigned char* win, void* stream) {
    unsigned long long* slot = m3t_take_amax_out();
    VGPool g;
    if (!vgpool_geom(H, W, C, ceil_mode, g) || !vg_shape_ok(P, C) || !al16(x) || !al16(yp) || !al4(win)) return M3T_EINVAL;
    const size_t total4 = P * (size_t)g.Ho * g.Wo * (size_t)(C / 4);
    vg_relu_pool_fwd_kernel<<<vg_grid(total4), VG_TH, 0, (hipStream_t)stream>>>(x, yp, win, total4, g, slot);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_relu_pool_cl_bwd(const float* dyp, const float* yp, const unsigned char* win, size_t P, int H, int W, int C, int ceil_mode,
                                    float* dx, float* dx_colsum, float* ws, size_t ws_bytes, void* stream) {
    unsigned long long* slot = m3t_take_amax_out();
    VGPool g;
    if (!vgpool_geom(H, W, C, ceil_mode, g) || !vg_shape_ok(P, C) || !al16(dyp) || !al16(yp) || !al16(dx) || !al4(win)) return M3T_EINVAL;
    const size_t M = P * (size_t)H * W;
    hipStream_t s = (hipStream_t)stream;
    return vg_bwd(M, C, dx_colsum, ws, ws_bytes, s, [&](int nch, size_t lds, size_t rpc, double* partial) {
        vg_relu_pool_bwd_kernel<<<nch, VG_TH, lds, s>>>(dyp, yp, win, dx, M, g, rpc, slot, partial);
    });
}
