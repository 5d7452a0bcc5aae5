// The expression head in the device-side evaluation epoch (beside evaluate.hip): the 7 expression logits of every frame
// (channels 0..6 of y_hat, model.py:175) get the path valence and arousal have, with the masking and argmax of
// training_step (model.py:171-182) and the stitching of validation_end / test_end (model.py:261-297, 354-366).
//   eval_append_mtl    per batch: eval_append's rows / part, + the 7 logits, the masked labels and a 7x7 confusion per clip
//   eval_gather_expr   per epoch: stitched logit tracks (eval_gather's sum per channel), their argmax, the label track
//   eval_expr_metrics  accuracy, macro-F1, 0.67 F1 + 0.33 accuracy and the per-class table from the confusions
//   expr_mode_tracks   per report: a mode filter over class tracks, all tracks in one launch
//   expr_track_conf    per report: one confusion (and accuracy) per track
// Tiny, latency-bound work in the style of evaluate.hip: 256-thread workgroups, loops that stride over T, no float atomics,
// every floating sum in a fixed order.  Counts are integers (LDS integer atomics): exact, whatever the order.
// Class rule: argmax over the 7 logits as torch.argmax -- the first maximal index, a NaN counts as maximal (the first NaN
// wins).  Class -1 = none.
#include "evaluate_va.h"

namespace {

constexpr int NC = 7;                   // expression classes (model.py:175: y_hat[..., :7])

__device__ __forceinline__ int argmax7(const float (&l)[NC]) {
    float mx = l[0];
    int am = 0;
#pragma unroll
    for (int c = 1; c < NC; ++c)
        if (m3t_nan_gt(l[c], mx)) { mx = l[c]; am = c; }
    return am;
}

// One workgroup per clip n.  expr_rows[n][c][t] = y[n][t][c], c < 7, for t < length[n], else 0 (inputs not loaded).  With
// labels: expr_gt[n][t] = class_expr clipped to 0..6 where t < length and expr_valid, else -1; conf[n][g][p] = the number of
// such frames with label g and argmax p.
__global__ __launch_bounds__(256) void eval_append_mtl_kernel(const float* __restrict__ y, int T, int C,
                                                              const float* __restrict__ lv, const float* __restrict__ la,
                                                              const long long* __restrict__ cls, const unsigned char* __restrict__ vld,
                                                              const long long* __restrict__ length, float* __restrict__ rows,
                                                              double* __restrict__ part, float* __restrict__ expr_rows,
                                                              signed char* __restrict__ expr_gt, int* __restrict__ conf) {
    __shared__ double red[256];
    __shared__ int cnt[NC * NC];
    const long n = blockIdx.x;
    const int len = eval_clip_len(length[n], T);
    eval_append_va(y, n, T, C, len, lv, la, rows, part, red);
    if (cls && threadIdx.x < NC * NC) cnt[threadIdx.x] = 0;
    __syncthreads();
    const float* yn = y + n * (long)T * C;
    float* en = expr_rows + n * (long)NC * T;
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const bool in = t < len;
        float l[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            l[c] = in ? yn[(long)t * C + c] : 0.f;
            en[(long)c * T + t] = l[c];
        }
        if (cls) {
            int g = -1;
            if (in && vld[n * T + t]) {
                const long long k = cls[n * T + t];
                g = k < 0 ? 0 : (k > NC - 1 ? NC - 1 : (int)k);
                atomicAdd(&cnt[g * NC + argmax7(l)], 1);
            }
            expr_gt[n * T + t] = (signed char)g;
        }
    }
    if (!cls) return;
    __syncthreads();
    if (threadIdx.x < NC * NC) conf[n * (NC * NC) + threadIdx.x] = cnt[threadIdx.x];
}

// One thread per output frame; the plan tables and the two searches of eval_gather_kernel (evaluate.hip).  Per channel the
// same sequence: zeros, += per covering segment in ascending start order, * 0.5f from halve_from on.
__global__ __launch_bounds__(256) void eval_gather_expr_kernel(const float* __restrict__ expr_rows, const signed char* __restrict__ expr_gt,
                                                               long W, int T, const long long* __restrict__ seg_dst,
                                                               const long long* __restrict__ seg_len, const long long* __restrict__ seg_row,
                                                               const long long* __restrict__ vid_seg_off,
                                                               const long long* __restrict__ vid_frame_off, int V, long long F,
                                                               long long halve_from, float* __restrict__ logit_tracks,
                                                               signed char* __restrict__ pred, signed char* __restrict__ gt) {
    const long long gf = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gf >= F) return;
    int lo = 0, hi = V;                                   // the last video with vid_frame_off[v] <= gf
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (vid_frame_off[mid] <= gf) lo = mid; else hi = mid;
    }
    const long long f = gf - vid_frame_off[lo];
    const long long s1 = vid_seg_off[lo + 1];
    long long a = vid_seg_off[lo], b = s1;                // the first segment with dst > f - T
    while (a < b) {
        const long long mid = (a + b) >> 1;
        if (seg_dst[mid] > f - T) b = mid; else a = mid + 1;
    }
    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.f;
    bool covered = false;
    int g = -1;
    for (long long s = a; s < s1 && seg_dst[s] <= f; ++s) {
        const long long t = f - seg_dst[s], r = seg_row[s];
        if (t < seg_len[s] && t < T && r >= 0 && r < W) {
            const float* x = expr_rows + (r * NC) * (long long)T + t;
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] = acc[c] + x[(long)c * T];
            if (!covered && expr_gt) g = expr_gt[r * (long long)T + t];
            covered = true;
        }
    }
    if (f >= halve_from) {
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = acc[c] * 0.5f;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) logit_tracks[c * F + gf] = acc[c];
    pred[gf] = (signed char)(covered ? argmax7(acc) : -1);
    if (gt) gt[gf] = (signed char)g;
}

// One workgroup: conf[W][7][7] summed over W (thread i takes i, i + 256, ...; exact integers, so the order is immaterial),
// then thread 0 scores.  out[0..3) = accuracy, macro-F1, 0.67 F1 + 0.33 accuracy; out[3 + c], out[10 + c], out[17 + c] =
// precision, recall, F1 of class c.
__global__ __launch_bounds__(256) void eval_expr_metrics_kernel(const int* __restrict__ conf, long W, double* __restrict__ out) {
    __shared__ unsigned long long tot[NC * NC];
    if (threadIdx.x < NC * NC) tot[threadIdx.x] = 0ull;
    __syncthreads();
    long long c[NC * NC];
#pragma unroll
    for (int k = 0; k < NC * NC; ++k) c[k] = 0;
    for (long w = threadIdx.x; w < W; w += blockDim.x) {
#pragma unroll
        for (int k = 0; k < NC * NC; ++k) c[k] += conf[w * (NC * NC) + k];
    }
#pragma unroll
    for (int k = 0; k < NC * NC; ++k)
        if (c[k]) atomicAdd(&tot[k], (unsigned long long)c[k]);
    __syncthreads();
    if (threadIdx.x != 0) return;
    {
#pragma clang fp contract(off)          // 0.67 f1 + 0.33 acc as two roundings, as the host restatement computes it
        long long all = 0, hit = 0;
        for (int k = 0; k < NC * NC; ++k) all += (long long)tot[k];
        double f1sum = 0.0;
        int present = 0;
        for (int k = 0; k < NC; ++k) {
            const long long tp = (long long)tot[k * NC + k];
            long long row = 0, col = 0;
            for (int j = 0; j < NC; ++j) { row += (long long)tot[k * NC + j]; col += (long long)tot[j * NC + k]; }
            const long long fn = row - tp, fp = col - tp;
            hit += tp;
            const double f1 = (double)(2 * tp) / (double)(2 * tp + fp + fn);
            out[3 + k] = (double)tp / (double)(tp + fp);
            out[10 + k] = (double)tp / (double)(tp + fn);
            out[17 + k] = f1;
            if (tp + fp + fn > 0) { f1sum += f1; ++present; }
        }
        const double acc = (double)hit / (double)all, f1m = f1sum / (double)present;
        out[0] = acc;
        out[1] = f1m;
        out[2] = 0.67 * f1m + 0.33 * acc;
    }
}

// One workgroup per track i = elements offsets[i] .. offsets[i+1] of c.  out[j] = the most frequent class among
// c[max(0, j-h) .. min(n-1, j+h)] (the window is cut at the ends), -1 ignored (and anything else outside 0..6); a tie goes to
// c[j] when it is among the tied classes, else to the smallest one; nothing but -1 in reach: -1.
__global__ __launch_bounds__(256) void expr_mode_tracks_kernel(const signed char* __restrict__ c_all, const long long* __restrict__ offsets,
                                                               int h, signed char* __restrict__ out_all) {
    const long long b = offsets[blockIdx.x], n = offsets[blockIdx.x + 1] - b;
    const signed char* c = c_all + b;
    signed char* out = out_all + b;
    for (long long j = threadIdx.x; j < n; j += blockDim.x) {
        const long long j0 = j - h < 0 ? 0 : j - h, j1 = j + h > n - 1 ? n - 1 : j + h;
        int cnt[NC];
#pragma unroll
        for (int k = 0; k < NC; ++k) cnt[k] = 0;
        for (long long i = j0; i <= j1; ++i) {
            const int v = c[i];
#pragma unroll
            for (int k = 0; k < NC; ++k) cnt[k] += (v == k);
        }
        const int mine = c[j];
        int best = 0, cls = -1;
#pragma unroll
        for (int k = 0; k < NC; ++k) {                    // the smallest class with the largest count; the centre's class on a tie
            if (cnt[k] > best || (cnt[k] == best && best > 0 && k == mine)) { best = cnt[k]; cls = k; }
        }
        out[j] = (signed char)cls;
    }
}

// One workgroup per track: conf[i][g][p] = the number of frames with gt = g and pred = p, both in 0..6; acc[i] (nullable) =
// the trace over the total (0 / 0 = NaN for a track without such a frame).
__global__ __launch_bounds__(256) void expr_track_conf_kernel(const signed char* __restrict__ pred, const signed char* __restrict__ gt,
                                                              const long long* __restrict__ offsets, int* __restrict__ conf,
                                                              double* __restrict__ acc) {
    __shared__ int cnt[NC * NC];
    if (threadIdx.x < NC * NC) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long b = offsets[blockIdx.x], n = offsets[blockIdx.x + 1] - b;
    for (long long j = threadIdx.x; j < n; j += blockDim.x) {
        const int p = pred[b + j], g = gt[b + j];
        if (p >= 0 && p < NC && g >= 0 && g < NC) atomicAdd(&cnt[g * NC + p], 1);
    }
    __syncthreads();
    if (threadIdx.x < NC * NC) conf[(long)blockIdx.x * (NC * NC) + threadIdx.x] = cnt[threadIdx.x];
    if (acc && threadIdx.x == 0) {
        long long all = 0, hit = 0;
        for (int k = 0; k < NC * NC; ++k) all += cnt[k];
        for (int k = 0; k < NC; ++k) hit += cnt[k * NC + k];
        acc[blockIdx.x] = (double)hit / (double)all;
    }
}

}  // namespace

extern "C" int m3t_eval_append_mtl(const float* y_hat, int N, int T, int C, const float* label_valence, const float* label_arousal,
                                   const long long* class_expr, const unsigned char* expr_valid, const long long* length,
                                   float* rows, double* part, float* expr_rows, signed char* expr_gt, int* conf, void* stream) {
    if (N == 0) return 0;
    if (!y_hat || !length || !rows || !expr_rows || N < 0 || T <= 0 || C < 9) return M3T_EINVAL;
    if ((label_valence != nullptr) != (label_arousal != nullptr) || (label_valence && !part)) return M3T_EINVAL;
    if ((class_expr != nullptr) != (expr_valid != nullptr) || (class_expr != nullptr) != (label_valence != nullptr)) return M3T_EINVAL;
    if (class_expr && (!expr_gt || !conf)) return M3T_EINVAL;
    eval_append_mtl_kernel<<<N, 256, 0, (hipStream_t)stream>>>(y_hat, T, C, label_valence, label_arousal, class_expr, expr_valid,
                                                               length, rows, part, expr_rows, expr_gt, conf);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_eval_gather_expr(const float* expr_rows, const signed char* expr_gt, long long W, int T, const long long* seg_dst,
                                    const long long* seg_len, const long long* seg_row, const long long* vid_seg_off,
                                    const long long* vid_frame_off, int V, long long F, long long halve_from, float* logit_tracks,
                                    signed char* pred, signed char* gt, void* stream) {
    if (V == 0 || F == 0) return 0;
    if (!expr_rows || !seg_dst || !seg_len || !seg_row || !vid_seg_off || !vid_frame_off || !logit_tracks || !pred) return M3T_EINVAL;
    if ((gt != nullptr) && !expr_gt) return M3T_EINVAL;
    if (W <= 0 || T <= 0 || V < 0 || F < 0 || (F + 255) / 256 > 0x7fffffffLL) return M3T_EINVAL;
    eval_gather_expr_kernel<<<(unsigned)((F + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        expr_rows, gt ? expr_gt : nullptr, (long)W, T, seg_dst, seg_len, seg_row, vid_seg_off, vid_frame_off, V, F, halve_from,
        logit_tracks, pred, gt);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_eval_expr_metrics(const int* conf, long long W, double* out24, void* stream) {
    if (!conf || !out24 || W <= 0) return M3T_EINVAL;
    eval_expr_metrics_kernel<<<1, 256, 0, (hipStream_t)stream>>>(conf, (long)W, out24);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_expr_mode_tracks(const signed char* c, const long long* offsets, int n_tracks, int window, signed char* out,
                                    void* stream) {
    if (window < 1 || (window & 1) == 0 || n_tracks < 0) return M3T_EINVAL;
    if (n_tracks == 0) return 0;
    if (!c || !offsets || !out) return M3T_EINVAL;
    expr_mode_tracks_kernel<<<n_tracks, 256, 0, (hipStream_t)stream>>>(c, offsets, window / 2, out);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_expr_track_conf(const signed char* pred, const signed char* gt, const long long* offsets, int n_tracks,
                                   int* conf, double* acc, void* stream) {
    if (n_tracks == 0) return 0;
    if (!pred || !gt || !offsets || !conf || n_tracks < 0) return M3T_EINVAL;
    expr_track_conf_kernel<<<n_tracks, 256, 0, (hipStream_t)stream>>>(pred, gt, offsets, conf, acc);
    M3T_LAUNCH_CHECK();
    return 0;
}
