// The evaluation epoch on the device: what AffWild2VA.validation_step / validation_end / test_end and
// get_smoothed_ccc.py do with host tensors, as four kernels that never read back:
//   eval_append   per batch: pick (valence, arousal) of every clip, zero the frames past its length, per-window fp64 moments
//   eval_gather   per epoch: every track of every video from the windows (overlap-add + halving, or concatenation)
//   eval_metrics  per epoch: val_ccc_v / val_ccc_a / val_mse_v / val_mse_a / val_loss from the per-window moments
//   ccc_tracks    per report: the per-video CCCs of the smoothed tracks, all videos x {valence, arousal} in one launch
// Tiny, latency-bound work: plain fp32 / fp64, 256-thread workgroups, no atomics, every sum in a fixed order
// (block_sum_f64, the reduction of postproc.hip), so a result does not depend on the run.
#include "evaluate_va.h"

namespace {

// One workgroup per clip n: eval_append_va (evaluate_va.h), the text m3t_eval_append_mtl runs too.
__global__ __launch_bounds__(256) void eval_append_kernel(const float* __restrict__ y, int T, int C,
                                                          const float* __restrict__ lv, const float* __restrict__ la,
                                                          const long long* __restrict__ length, float* __restrict__ rows,
                                                          double* __restrict__ part) {
    __shared__ double red[256];
    const long n = blockIdx.x;
    eval_append_va(y, n, T, C, eval_clip_len(length[n], T), lv, la, rows, part, red);
}

// One thread per output frame.  Video v owns the frames vid_frame_off[v] .. vid_frame_off[v+1] of every track and the
// segments vid_seg_off[v] .. vid_seg_off[v+1], sorted by destination.  Segment s covers the frames seg_dst[s] .. +seg_len[s]
// of its video with rows[seg_row[s]][q][0 .. seg_len[s]).  The sum is the reference's own sequence (model.py:281-297,
// 358-366): zeros, += per segment in ascending start order, then /= 2 from frame `halve_from` on (x * 0.5f is the same
// fp32 number as x / 2.f).  Every frame is written exactly once; a frame no segment covers is 0.
__global__ __launch_bounds__(256) void eval_gather_kernel(const float* __restrict__ rows, long W, int Q, int T,
                                                          const long long* __restrict__ seg_dst, const long long* __restrict__ seg_len,
                                                          const long long* __restrict__ seg_row,
                                                          const long long* __restrict__ vid_seg_off,
                                                          const long long* __restrict__ vid_frame_off, int V, long long F,
                                                          long long halve_from, float* __restrict__ tracks) {
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
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (long long s = a; s < s1 && seg_dst[s] <= f; ++s) {
        const long long t = f - seg_dst[s], r = seg_row[s];
        if (t < seg_len[s] && t < T && r >= 0 && r < W) {
            const float* x = rows + (r * Q) * (long long)T + t;
            for (int q = 0; q < Q; ++q) acc[q] = acc[q] + x[(long)q * T];
        }
    }
    const bool halve = f >= halve_from;
    for (int q = 0; q < Q; ++q) tracks[q * F + gf] = halve ? acc[q] * 0.5f : acc[q];
}

// One workgroup: part[W][2][7] summed over the windows (thread i takes windows i, i + 256, ...; then the tree), and
// concordance_cc2 as validation_end calls it (models/utils.py:12-22 on torch tensors): unbiased variances, biased
// covariance.  out = val_ccc_v, val_ccc_a, val_mse_v, val_mse_a, val_loss.  No valid frame: 0 / 0 = NaN, as there.
__global__ __launch_bounds__(256) void eval_metrics_kernel(const double* __restrict__ part, long W, double* __restrict__ out) {
    __shared__ double red[256];
    double m[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) m[k] = 0.0;
    for (long w = threadIdx.x; w < W; w += blockDim.x) {
#pragma unroll
        for (int k = 0; k < 14; ++k) m[k] += part[w * 14 + k];
    }
#pragma unroll
    for (int k = 0; k < 14; ++k) m[k] = block_sum_f64(m[k], red);
    if (threadIdx.x == 0) {
        double ccc[2];
        for (int k = 0; k < 2; ++k) {
            const double* s = m + 7 * k;
            const double n = s[0], mp = s[1] / n, mg = s[2] / n;
            // (one valid frame: torch's unbiased variance is NaN; 0 / 0 here too, whatever the rounding of the numerator)
            const double varp = n > 1.0 ? (s[3] - n * mp * mp) / (n - 1.0) : 0.0 / (n - n);
            const double varg = n > 1.0 ? (s[4] - n * mg * mg) / (n - 1.0) : 0.0 / (n - n);
            const double cov = (s[5] - n * mp * mg) / n;
            ccc[k] = 2.0 * cov / (varp + varg + (mp - mg) * (mp - mg));
            out[2 + k] = s[6] / n;
        }
        out[0] = ccc[0];
        out[1] = ccc[1];
        out[4] = 1.0 - 0.5 * (ccc[0] + ccc[1]);
    }
}

// The body of postproc.hip's ccc_masked_kernel per track: the same two passes, thread-to-element mapping and reduction
// tree, so a track gives the bits m3t_ccc_masked gives on it.  Track i = elements offsets[i] .. offsets[i+1] of p, g, g2.
__global__ __launch_bounds__(256) void ccc_tracks_kernel(const double* __restrict__ p_all, const float* __restrict__ g_all,
                                                         const float* __restrict__ g2_all, const long long* __restrict__ offsets,
                                                         int p_unbiased, double* __restrict__ out_all) {
    __shared__ double red[256];
    const long b = offsets[blockIdx.x], n = offsets[blockIdx.x + 1] - b;
    const double* p = p_all + b;
    const float* g = g_all + b;
    const float* g2 = g2_all ? g2_all + b : nullptr;
    double* out = out_all + 2 * (long)blockIdx.x;
    double sp = 0.0, sg = 0.0, cnt = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const bool ok = g[i] >= -1.f && (!g2 || g2[i] >= -1.f);
        if (ok) { sp += p[i]; sg += (double)g[i]; cnt += 1.0; }
    }
    sp = block_sum_f64(sp, red);
    sg = block_sum_f64(sg, red);
    cnt = block_sum_f64(cnt, red);
    const double mp = sp / cnt, mg = sg / cnt;
    double vp = 0.0, vg = 0.0, cv = 0.0;
    for (long i = threadIdx.x; i < n; i += blockDim.x) {
        const bool ok = g[i] >= -1.f && (!g2 || g2[i] >= -1.f);
        if (ok) {
            const double a = p[i] - mp, c = (double)g[i] - mg;
            vp += a * a; vg += c * c; cv += a * c;
        }
    }
    vp = block_sum_f64(vp, red);
    vg = block_sum_f64(vg, red);
    cv = block_sum_f64(cv, red);
    if (threadIdx.x == 0) {
        const double varp = vp / (p_unbiased ? cnt - 1.0 : cnt), varg = vg / cnt, cov = cv / cnt;
        out[0] = 2.0 * cov / (varp + varg + (mp - mg) * (mp - mg));
        out[1] = cnt;
    }
}

}  // namespace

extern "C" int m3t_eval_append(const float* y_hat, int N, int T, int C, const float* label_valence, const float* label_arousal,
                               const long long* length, float* rows, double* part, void* stream) {
    if (N == 0) return 0;
    if (!y_hat || !length || !rows || N < 0 || T <= 0 || C < 2) return M3T_EINVAL;
    if ((label_valence != nullptr) != (label_arousal != nullptr) || (label_valence && !part)) return M3T_EINVAL;
    eval_append_kernel<<<N, 256, 0, (hipStream_t)stream>>>(y_hat, T, C, label_valence, label_arousal, length, rows, part);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_eval_gather(const float* rows, long long W, int Q, int T, const long long* seg_dst, const long long* seg_len,
                               const long long* seg_row, const long long* vid_seg_off, const long long* vid_frame_off, int V,
                               long long F, long long halve_from, float* tracks, void* stream) {
    if (V == 0 || F == 0) return 0;
    if (!rows || !seg_dst || !seg_len || !seg_row || !vid_seg_off || !vid_frame_off || !tracks) return M3T_EINVAL;
    if (W <= 0 || (Q != 2 && Q != 4) || T <= 0 || V < 0 || F < 0 || (F + 255) / 256 > 0x7fffffffLL) return M3T_EINVAL;
    eval_gather_kernel<<<(unsigned)((F + 255) / 256), 256, 0, (hipStream_t)stream>>>(rows, (long)W, Q, T, seg_dst, seg_len, seg_row,
                                                                                       vid_seg_off, vid_frame_off, V, F, halve_from, tracks);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_eval_metrics(const double* part, long long W, double* out5, void* stream) {
    if (!part || !out5 || W <= 0) return M3T_EINVAL;
    eval_metrics_kernel<<<1, 256, 0, (hipStream_t)stream>>>(part, (long)W, out5);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_ccc_tracks(const double* p, const float* g, const float* g2, const long long* offsets, int n_tracks,
                              int p_unbiased, double* out, void* stream) {
    if (n_tracks == 0) return 0;
    if (!p || !g || !offsets || !out || n_tracks < 0) return M3T_EINVAL;
    ccc_tracks_kernel<<<n_tracks, 256, 0, (hipStream_t)stream>>>(p, g, g2, offsets, p_unbiased, out);
    M3T_LAUNCH_CHECK();
    return 0;
}
