// The multi-label evaluation epoch on the device (AudioSet pre-training, 527 classes): mean average precision, mean ROC-AUC and what
// d' is computed from, per epoch, without a read-back per batch and without the 43 MB read-back of the scores at its end.
//   cls_eval_append   per batch: the clips' pooled logits and label rows, transposed through an LDS tile into resident CLASS-MAJOR
//                     matrices [C][M] at the clips' item rows; seen[M]; two poison counters (integer atomics, one pair per workgroup)
//   cls_eval_rank     per epoch: one workgroup per class sorts its column descending by value (bitonic network on key << 8 | label,
//                     csrc/cls_eval_core.h) -- in LDS when the padded column fits, otherwise LDS-sized chunks in LDS and the wide strides
//                     in a global workspace -- and walks the tie groups: AP, AUC, P, N
//   cls_eval_reduce   per epoch: the means over the scored classes in class order, the counts, the unseen rows, the counters
// No float atomics, every float64 sum in a fixed order: reruns give the same bits.
#include "common.h"
#include "cls_eval_core.h"
#include <math.h>

namespace {

constexpr int RANK_THREADS = 1024;
constexpr int TILE = 32;

// Tile of 32 clips x 32 classes.  Read: lane -> class (rows of `scores` / `labels` are contiguous over classes); write: lane -> clip,
// so a wave's stores to one class column go to neighbouring item rows when the batch's items are consecutive.
__global__ __launch_bounds__(256) void cls_eval_append_kernel(const float* __restrict__ scores, const float* __restrict__ labels,
                                                              const int* __restrict__ rows, int B, int C, long long M,
                                                              float* __restrict__ col_scores, unsigned char* __restrict__ col_labels,
                                                              unsigned char* __restrict__ seen, unsigned int* __restrict__ counters) {
    __shared__ float ts[TILE][TILE + 1];
    __shared__ float tl[TILE][TILE + 1];
    __shared__ unsigned int bad[2];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int b0 = blockIdx.y * TILE, c0 = blockIdx.x * TILE;
    if (threadIdx.x < 2) bad[threadIdx.x] = 0u;
    unsigned nonfinite = 0, badlabel = 0;
    for (int r = ty; r < TILE; r += 8) {
        const int b = b0 + r, c = c0 + tx;
        if (b < B && c < C) {
            const float s = scores[(size_t)b * C + c], l = labels[(size_t)b * C + c];
            ts[r][tx] = s;
            tl[r][tx] = l;
            nonfinite += (__float_as_uint(s) & 0x7f800000u) == 0x7f800000u;
            badlabel += !(l == 0.0f || l == 1.0f);
        }
    }
    __syncthreads();
    if (nonfinite) atomicAdd(&bad[0], nonfinite);          // LDS integer adds: order-free
    if (badlabel) atomicAdd(&bad[1], badlabel);
    const int b = b0 + tx;
    const long long row = b < B ? (long long)rows[b] : -1;
    if (row >= 0 && row < M) {                             // (the host has validated the table; a row outside the matrices is never written)
        for (int r = ty; r < TILE; r += 8) {
            const int c = c0 + r;
            if (c < C) {
                col_scores[(size_t)c * M + row] = ts[tx][r];
                col_labels[(size_t)c * M + row] = (unsigned char)(tl[tx][r] == 1.0f);
            }
        }
        if (blockIdx.x == 0 && ty == 0) seen[row] = 1;
    }
    __syncthreads();
    if (threadIdx.x < 2 && bad[threadIdx.x]) atomicAdd(&counters[threadIdx.x], bad[threadIdx.x]);
}

// Loads rows g0 .. g0 + n of class column c as sort items into dst (padding past M).
__device__ __forceinline__ void rank_load(const float* __restrict__ s, const unsigned char* __restrict__ l, unsigned M, unsigned g0,
                                          unsigned n, uint64_t* dst) {
    for (unsigned i = threadIdx.x; i < n; i += RANK_THREADS) {
        const unsigned g = g0 + i;
        dst[i] = g < M ? cls_item(__float_as_uint(s[g]), l[g]) : 0ull;
    }
}

// One workgroup of 1024 threads per class.  Dynamic LDS: L items, then two scan buffers of 1024 words.  n2 = the column padded to a
// power of two; n2 <= L: the whole network runs in LDS (ws unused).  Otherwise ws[c][n2]: every L-chunk is sorted in LDS into the
// direction its place in the network asks for, then per stage k > L the strides j >= L run in global memory (a workgroup barrier
// orders them: one workgroup owns the column) and the strides below L in LDS again, chunk by chunk.
__global__ __launch_bounds__(RANK_THREADS) void cls_eval_rank_kernel(const float* __restrict__ col_scores,
                                                                      const unsigned char* __restrict__ col_labels, unsigned M,
                                                                      unsigned n2, unsigned L, uint64_t* __restrict__ ws,
                                                                      double* __restrict__ per_class) {
    extern __shared__ __attribute__((aligned(16))) uint64_t dyn[];
    const unsigned Lu = n2 <= L ? n2 : L;
    uint64_t* items = dyn;
    uint64_t* bufA = dyn + Lu;
    uint64_t* bufB = bufA + RANK_THREADS;
    const unsigned tid = threadIdx.x, nt = RANK_THREADS;
    const size_t c = blockIdx.x;
    const float* s = col_scores + c * M;
    const unsigned char* l = col_labels + c * M;

    unsigned cnt, open_idx, open_cnt;
    if (n2 <= L) {
        rank_load(s, l, M, 0, n2, items);
        __syncthreads();
        for (unsigned k = 2; k <= n2; k <<= 1)
            for (unsigned j = k >> 1; j > 0; j >>= 1) {
                cls_bitonic_step(items, n2, 0u, k, j, tid, nt);
                __syncthreads();
            }
        cls_walk_count(items, M, tid, nt, cnt, open_idx, open_cnt);
    } else {
        uint64_t* g = ws + c * (size_t)n2;
        for (unsigned g0 = 0; g0 < n2; g0 += L) {
            rank_load(s, l, M, g0, L, items);
            __syncthreads();
            for (unsigned k = 2; k <= L; k <<= 1)
                for (unsigned j = k >> 1; j > 0; j >>= 1) {
                    cls_bitonic_step(items, L, g0, k, j, tid, nt);
                    __syncthreads();
                }
            for (unsigned i = tid; i < L; i += nt) g[g0 + i] = items[i];
            __syncthreads();
        }
        for (unsigned k = 2 * L; k <= n2; k <<= 1) {
            for (unsigned j = k >> 1; j >= L; j >>= 1) {
                cls_bitonic_step(g, n2, 0u, k, j, tid, nt);
                __syncthreads();
            }
            for (unsigned g0 = 0; g0 < n2; g0 += L) {
                for (unsigned i = tid; i < L; i += nt) items[i] = g[g0 + i];
                __syncthreads();
                for (unsigned j = L >> 1; j > 0; j >>= 1) {
                    cls_bitonic_step(items, L, g0, k, j, tid, nt);
                    __syncthreads();
                }
                for (unsigned i = tid; i < L; i += nt) g[g0 + i] = items[i];
                __syncthreads();
            }
        }
        cls_walk_count(g, M, tid, nt, cnt, open_idx, open_cnt);
    }
    const uint64_t* sorted = n2 <= L ? items : ws + c * (size_t)n2;

    // positives in front of every chunk: inclusive sum scan, ping-pong
    uint64_t *src = bufA, *dst = bufB;
    src[tid] = cnt;
    __syncthreads();
    for (unsigned d = 1; d < nt; d <<= 1) {
        cls_scan_step(src, dst, d, tid, false);
        __syncthreads();
        uint64_t* t = src; src = dst; dst = t;
    }
    const unsigned base = tid ? (unsigned)src[tid - 1] : 0u;
    const unsigned P = (unsigned)src[nt - 1];
    __syncthreads();
    // the group open where every chunk begins: inclusive max scan
    src[tid] = cls_open_word(open_idx, open_cnt, base);
    __syncthreads();
    for (unsigned d = 1; d < nt; d <<= 1) {
        cls_scan_step(src, dst, d, tid, true);
        __syncthreads();
        uint64_t* t = src; src = dst; dst = t;
    }
    const uint64_t carry = tid ? src[tid - 1] : 0ull;
    __syncthreads();

    double ap;
    uint64_t num;
    cls_walk_score(sorted, M, tid, nt, base, carry, ap, num);
    // both sums over the 1024 threads as fixed trees
    double* red = reinterpret_cast<double*>(bufA);
    red[tid] = ap;
    bufB[tid] = num;
    __syncthreads();
    for (unsigned st = nt >> 1; st > 0; st >>= 1) {
        if (tid < st) {
            red[tid] += red[tid + st];
            bufB[tid] += bufB[tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned N = M - P;
        double* out = per_class + 4 * c;
        out[0] = P ? red[0] / (double)P : (double)NAN;
        out[1] = (P && N) ? (double)bufB[0] / (double)(2ull * (uint64_t)P * (uint64_t)N) : (double)NAN;
        out[2] = (double)P;
        out[3] = (double)N;
    }
}

// out8 = mAP, mAUC, classes scored for AP, for AUC, unseen rows, non-finite scores, labels outside {0, 1}, 0.  The means run over the
// scored classes in class order in float64; with a poison counter above zero both are NaN (the per-class table stays as computed).
__global__ __launch_bounds__(256) void cls_eval_reduce_kernel(const double* __restrict__ per_class, int C,
                                                              const unsigned char* __restrict__ seen, long long M,
                                                              const unsigned int* __restrict__ counters, double* __restrict__ out8) {
    __shared__ unsigned long long red[256];
    unsigned long long unseen = 0;
    for (long long i = threadIdx.x; i < M; i += 256) unseen += seen[i] == 0;
    red[threadIdx.x] = unseen;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double sa = 0.0, su = 0.0;
        int na = 0, nu = 0;
        for (int c = 0; c < C; ++c) {
            const double ap = per_class[4 * (size_t)c], auc = per_class[4 * (size_t)c + 1];
            if (ap == ap) { sa += ap; ++na; }
            if (auc == auc) { su += auc; ++nu; }
        }
        const bool poisoned = counters[0] != 0u || counters[1] != 0u;
        out8[0] = (na && !poisoned) ? sa / (double)na : (double)NAN;
        out8[1] = (nu && !poisoned) ? su / (double)nu : (double)NAN;
        out8[2] = (double)na;
        out8[3] = (double)nu;
        out8[4] = (double)red[0];
        out8[5] = (double)counters[0];
        out8[6] = (double)counters[1];
        out8[7] = 0.0;
    }
}

bool rank_shape(int C, long long M, int lds_rows, unsigned& n2, unsigned& L) {
    if (C <= 0 || M <= 0 || M > M3T_CLS_EVAL_MAX_ROWS || lds_rows < 0) return false;
    const unsigned cap = lds_rows == 0 || lds_rows > M3T_CLS_EVAL_LDS_ROWS ? (unsigned)M3T_CLS_EVAL_LDS_ROWS : (unsigned)lds_rows;
    L = cls_floor_pow2(cap);
    n2 = (unsigned)cls_ceil_pow2((unsigned long long)M);
    return true;
}

}  // namespace

extern "C" int m3t_cls_eval_append(const float* scores, const float* labels, const int* rows, int B, int C, long long M,
                                   float* col_scores, unsigned char* col_labels, unsigned char* seen, unsigned int* counters,
                                   void* stream) {
    if (B == 0) return 0;
    if (!scores || !labels || !rows || !col_scores || !col_labels || !seen || !counters) return M3T_EINVAL;
    if (B < 0 || C <= 0 || M <= 0 || M > M3T_CLS_EVAL_MAX_ROWS || cdiv(B, TILE) > 65535) return M3T_EINVAL;
    cls_eval_append_kernel<<<dim3(cdiv(C, TILE), cdiv(B, TILE)), 256, 0, (hipStream_t)stream>>>(scores, labels, rows, B, C, M, col_scores,
                                                                                                 col_labels, seen, counters);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" size_t m3t_cls_eval_rank_ws_bytes(int C, long long M, int lds_rows) {
    unsigned n2, L;
    if (!rank_shape(C, M, lds_rows, n2, L)) return 0;
    return n2 <= L ? 0 : (size_t)C * n2 * sizeof(uint64_t);
}

extern "C" int m3t_cls_eval_rank(const float* col_scores, const unsigned char* col_labels, int C, long long M, int lds_rows, void* ws,
                                 size_t ws_bytes, double* per_class, void* stream) {
    unsigned n2, L;
    if (!col_scores || !col_labels || !per_class || !rank_shape(C, M, lds_rows, n2, L)) return M3T_EINVAL;
    const size_t need = n2 <= L ? 0 : (size_t)C * n2 * sizeof(uint64_t);
    if (need && (!ws || ws_bytes < need || ((uintptr_t)ws & 7u))) return M3T_EINVAL;
    const size_t lds = ((size_t)(n2 <= L ? n2 : L) + 2 * RANK_THREADS) * sizeof(uint64_t);
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(cls_eval_rank_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    cls_eval_rank_kernel<<<C, RANK_THREADS, lds, (hipStream_t)stream>>>(col_scores, col_labels, (unsigned)M, n2, L, (uint64_t*)ws, per_class);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_cls_eval_reduce(const double* per_class, int C, const unsigned char* seen, long long M, const unsigned int* counters,
                                   double* out8, void* stream) {
    if (!per_class || !seen || !counters || !out8 || C <= 0 || M <= 0) return M3T_EINVAL;
    cls_eval_reduce_kernel<<<1, 256, 0, (hipStream_t)stream>>>(per_class, C, seen, M, counters, out8);
    M3T_LAUNCH_CHECK();
    return 0;
}
