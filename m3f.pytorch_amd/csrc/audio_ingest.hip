// Batched audio ingest: what the reference's AudioSet loader does per clip on the host with librosa (models/audioset_dataset.py:58-87:
// temporal crop with np.pad 'wrap', 512-point STFT, 40 Slaney bands, power_to_db, 5-frame context stack) and the AffWild2 loader's stacking
// of pre-extracted tracks (models/dataset.py:83-95, :276-306), for a whole batch in a handful of launches.  A batch is a FLAT buffer plus
// per-clip tables (the style of m3t_smooth_tracks' offsets): clips are not padded to a common length.
//     m3t_audio_frame_batch    PCM (int16 or float32) -> windowed frames of every clip in one matrix [R, n_fft]
//     (m3t_sgemm)              [R, n_fft] x [n_fft, 2 bins]: ONE DFT product for the batch
//     m3t_audio_power_mel      re^2 + im^2 and the (sparse) mel filterbank -> [R, n_mels]
//     m3t_audio_db_stack       per-clip power_to_db (the clip's own maximum over ALL its rows) + context stack -> [N, T, width n_mels]
//     m3t_audio_db_stack_aug   the same launch with the reference's spec_augment masks (audioset_dataset.py:17-55; the cell rule is
//                              audio_aug_core.h) and a mix with a partner clip of the batch, opt-in: training-time augmentation
//     m3t_stack_context_batch  pre-extracted mel tracks -> [N, window, width n_mels] (edge padding, zero clips)
// HBM- and latency-bound glue: no atomics, every reduction in a fixed order, no synchronisation inside a call.  Device-side tables are
// checked against the buffers' sizes in the kernels: a bad entry writes zeros (or nothing), it never leaves an allocation.
#include "common.h"
#include "audio_aug_core.h"

namespace {

// per-clip table of the waveform route, long long [N][8]
enum { C_OFF = 0, C_LEN = 1, C_START = 2, C_NS = 3, C_HOP = 4, C_NF = 5, C_ROW = 6 };
// per-clip table of the track route, long long [N][4]
enum { K_ROW = 0, K_ROWS = 1, K_START = 2, K_LEN = 3 };

__device__ __forceinline__ float pcm(const float* w, long long i) { return w[i]; }
__device__ __forceinline__ float pcm(const int16_t* w, long long i) { return (float)w[i] * (1.0f / 32768.0f); }      // exact in fp32

// frames[row_off + f][k] = window[k] * cpad[f*hop + k], cpad = the clip's crop c with n_fft/2 samples of padding per side,
// c[j] = wave[off + (start + j) mod len], j < nsamples  (frame_window_kernel of audio.hip on the crop of one clip)
template <typename T>
__global__ __launch_bounds__(256) void frame_batch_kernel(const T* __restrict__ wave, long long total, const long long* __restrict__ clips,
                                                          int N, long long R, int n_fft, int pad_mode, const float* __restrict__ window,
                                                          float* __restrict__ frames) {
    const int half = n_fft >> 1;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const long long* c = clips + 8ll * n;
        const long long off = c[C_OFF], len = c[C_LEN], start = c[C_START], ns = c[C_NS], hop = c[C_HOP], nf = c[C_NF], ro = c[C_ROW];
        if (off < 0 || len <= 0 || off > total - len || start < 0 || ns <= 0 || hop <= 0 || nf <= 0 || ro < 0 || ro > R - nf) continue;
        const long long s0 = start % len;
        for (long long f = blockIdx.x; f < nf; f += gridDim.x) {
            float* row = frames + (ro + f) * n_fft;
            for (int k = threadIdx.x; k < n_fft; k += blockDim.x) {
                long long j = f * hop + k - half;
                if (j < 0 || j >= ns) {
                    if (pad_mode == 1 && ns > 1) {           // numpy 'reflect': ... 2 1 | 0 1 2 ... ns-1 | ns-2 ns-3 ...
                        const long long period = 2 * (ns - 1);
                        long long m = j % period;
                        if (m < 0) m += period;
                        j = m < ns ? m : period - m;
                    } else {
                        j = -1;
                    }
                }
                float v = 0.f;
                if (j >= 0) {
                    long long t = s0 + j;                    // np.pad(y, (0, ..), 'wrap'): the clip repeats from its first sample
                    if (t >= len) {
                        t -= len;
                        if (t >= len) t %= len;
                    }
                    v = pcm(wave, off + t);
                }
                row[k] = v * window[k];
            }
        }
    }
}

// spec [R][2 bins] (re | im) -> mel [R][n_mels]: mel[r][b] = sum over the band's bins, in bin order, of w * (re^2 + im^2).
// bands: int [2 n_mels + 1] = n_mels + 1 offsets into `weights`, then the first bin of each band.  One wave per row, one lane per band.
__global__ __launch_bounds__(256) void power_mel_kernel(const float* __restrict__ spec, long long R, int bins, int n_mels,
                                                        const float* __restrict__ weights, const int* __restrict__ bands, int nnz,
                                                        float* __restrict__ mel) {
    extern __shared__ float sm[];
    float* wsm = sm;                                         // [nnz]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    float* pw = sm + nnz + wv * bins;                        // [bins] of this wave's row
    for (int i = threadIdx.x; i < nnz; i += 256) wsm[i] = weights[i];
    int o0 = 0, cnt = 0, lo = 0;
    if (lane < n_mels) {                                     // clamped: a bad table reads inside the two LDS arrays
        o0 = min(max(bands[lane], 0), nnz);
        cnt = min(max(bands[lane + 1] - o0, 0), nnz - o0);
        lo = min(max(bands[n_mels + 1 + lane], 0), bins);
        cnt = min(cnt, bins - lo);
    }
    for (long long base = 4ll * blockIdx.x; base < R; base += 4ll * gridDim.x) {       // (uniform per block: the barriers below)
        const long long r = base + wv;
        __syncthreads();                                     // the weights are staged / the previous row's bands are summed
        if (r < R) {
            const float* s = spec + r * 2 * bins;
            for (int i = lane; i < bins; i += 64) {
                const float re = s[i], im = s[bins + i];
                pw[i] = re * re + im * im;
            }
        }
        __syncthreads();
        if (r < R && lane < n_mels) {
            float acc = 0.f;
            for (int q = 0; q < cnt; ++q) acc = fmaf(wsm[o0 + q], pw[lo + q], acc);
            mel[r * n_mels + lane] = acc;
        }
    }
}

// One workgroup per clip: librosa.power_to_db(S, ref=1, amin, top_db) over the clip's own nf rows (two passes: maximum, then values),
// then the stacking of audioset_dataset.py:77-85: out[n][t] = rows t*step .. +width concatenated, a row >= nf contributes 0.0
__global__ __launch_bounds__(256) void db_stack_kernel(const float* __restrict__ mel, long long R, const long long* __restrict__ clips, int T,
                                                       int n_mels, int step, int width, float amin, float top_db, float* __restrict__ out) {
    __shared__ float red[4];
    const long long n = blockIdx.x;
    const long long* c = clips + 8 * n;
    long long nf = c[C_NF], ro = c[C_ROW];
    if (nf <= 0 || ro < 0 || ro > R - nf) { nf = 0; ro = 0; }            // (a bad table: a zero clip)
    const float* m = mel + ro * n_mels;
    const long long cells = nf * n_mels;
    float mx = -3.0e38f;
    for (long long i = threadIdx.x; i < cells; i += 256) mx = fmaxf(mx, 10.0f * log10f(fmaxf(amin, m[i])));
    mx = wave_max(mx);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float ref = 10.0f * log10f(fmaxf(amin, 1.0f));
    const float floor_db = (mx - ref) - top_db;
    const int W = width * n_mels;
    float* o = out + n * T * W;
    for (int i = threadIdx.x; i < T * W; i += 256) {
        const int t = i / W, r = i - t * W, k = r / n_mels, cc = r - k * n_mels;
        const long long row = (long long)t * step + k;
        float v = 0.f;
        if (row < nf) {
            v = 10.0f * log10f(fmaxf(amin, m[row * n_mels + cc])) - ref;
            if (top_db >= 0.f) v = fmaxf(v, floor_db);
        }
        o[i] = v;
    }
}

// db_stack_kernel's per-clip half for the augmented route: the clip's rows and the floor of its own power_to_db
struct AugClip {
    const float* m;
    long long nf;
    float floor_db;
};

// the clip `n` of the table: its rows (a bad entry: a zero clip) and, by the fixed-order workgroup maximum of db_stack_kernel, its floor
__device__ __forceinline__ AugClip aug_clip(const float* __restrict__ mel, long long R, const long long* __restrict__ clips, long long n,
                                            int n_mels, float amin, float top_db, float ref, float* red) {
    const long long* c = clips + 8 * n;
    long long nf = c[C_NF], ro = c[C_ROW];
    if (nf <= 0 || ro < 0 || ro > R - nf) { nf = 0; ro = 0; }
    const float* m = mel + ro * n_mels;
    const long long cells = nf * n_mels;
    float mx = -3.0e38f;
    for (long long i = threadIdx.x; i < cells; i += 256) mx = fmaxf(mx, 10.0f * log10f(fmaxf(amin, m[i])));
    mx = wave_max(mx);
    __syncthreads();                                         // (red is free: the previous clip's maximum has been read)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    return {m, nf, (mx - ref) - top_db};
}

// the value cell i of the stacked rows takes from one clip: db_stack_kernel's, or exactly 0.0 where audio_aug_core.h says so
__device__ __forceinline__ float aug_value(const AugClip& c, const int* p, int n_mels, int step, int width, float amin, float top_db,
                                           float ref, int i) {
    const long long src = aug_cell(p, c.nf, n_mels, step, width, i);
    if (src < 0) return 0.f;
    float v = 10.0f * log10f(fmaxf(amin, c.m[src])) - ref;
    if (top_db >= 0.f) v = fmaxf(v, c.floor_db);
    return v;
}

// db_stack_kernel with the reference's spec_augment (audioset_dataset.py:17-55) and a mix across the batch.  One workgroup per OUTPUT
// clip n: x[n] = its own masked dB rows (its own nf, floor and masks); with a partner p >= 0 also x[p] (the partner's nf, floor and
// masks), and out[n] = lam32 x[n] + om32 x[p] in two rounded products and one rounded sum.  Without a partner x[n] is written as it is.
__global__ __launch_bounds__(256) void db_stack_aug_kernel(const float* __restrict__ mel, long long R, const long long* __restrict__ clips,
                                                           int N, const int* __restrict__ aug, const float* __restrict__ mixw, int T,
                                                           int n_mels, int step, int width, float amin, float top_db,
                                                           float* __restrict__ out) {
    __shared__ float red[4];
    const long long n = blockIdx.x;
    const int* pa = aug + AUG_INTS * n;
    const int partner = pa[AUG_PARTNER];
    const int W = width * n_mels;
    float* o = out + n * T * W;
    if (partner < -1 || partner >= N) {                      // (a bad table: a zero clip; uniform per workgroup)
        for (int i = threadIdx.x; i < T * W; i += 256) o[i] = 0.f;
        return;
    }
    const float ref = 10.0f * log10f(fmaxf(amin, 1.0f));
    const AugClip a = aug_clip(mel, R, clips, n, n_mels, amin, top_db, ref, red);
    if (partner < 0) {
        for (int i = threadIdx.x; i < T * W; i += 256) o[i] = aug_value(a, pa, n_mels, step, width, amin, top_db, ref, i);
        return;
    }
    const AugClip b = aug_clip(mel, R, clips, partner, n_mels, amin, top_db, ref, red);
    const int* pb = aug + AUG_INTS * (long long)partner;
    const float lam = mixw[2 * n], om = mixw[2 * n + 1];
    for (int i = threadIdx.x; i < T * W; i += 256) {
        const float xa = aug_value(a, pa, n_mels, step, width, amin, top_db, ref, i);
        const float xb = aug_value(b, pb, n_mels, step, width, amin, top_db, ref, i);
        o[i] = __fadd_rn(__fmul_rn(lam, xa), __fmul_rn(om, xb));
    }
}

// models/dataset.py:83-95 and :276-306 for N tracks: out[n][i] = the row m3t_stack_context gives for frame min(i, track_len - 1)
// (np.pad 'edge' of a short window), zeros for track_len == 0 (an invalid clip: fps < 15)
__global__ __launch_bounds__(256) void stack_batch_kernel(const float* __restrict__ mels, long long total_rows, int n_mels,
                                                          const long long* __restrict__ tracks, int N, int window, int step, int width,
                                                          float* __restrict__ out) {
    const int W = width * n_mels;
    const long long cells = (long long)window * W;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const long long* k4 = tracks + 4ll * n;
        long long ro = k4[K_ROW], rows = k4[K_ROWS], start = k4[K_START], tl = k4[K_LEN];
        if (ro < 0 || rows < 0 || ro > total_rows - rows || start < 0 || tl > window) tl = 0;
        float* o = out + (long long)n * cells;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cells; i += 256ll * gridDim.x) {
            const long long f = i / W;
            const int r = (int)(i - f * W), k = r / n_mels, cc = r - k * n_mels;
            float v = 0.f;
            if (tl > 0) {
                const long long row = (start + (f < tl ? f : tl - 1)) * step + k;
                if (row < rows) v = mels[(ro + row) * n_mels + cc];
            }
            o[i] = v;
        }
    }
}

}  // namespace

extern "C" int m3t_audio_frame_batch(const void* wave, int dtype, long long n_samples, const long long* clips, int N, long long R, int n_fft,
                                     int pad_mode, const float* window, float* frames, void* stream) {
    if (N < 0 || R < 0) return M3T_EINVAL;
    if (N == 0 || R == 0) return 0;
    if (!wave || !clips || !window || !frames || n_samples <= 0 || n_fft <= 0 || (n_fft & 1) || (dtype != 0 && dtype != 1) ||
        (pad_mode != 0 && pad_mode != 1))
        return M3T_EINVAL;
    if (((uintptr_t)wave % (dtype == 1 ? 2 : 4)) != 0 || ((uintptr_t)clips % 8) != 0 || ((uintptr_t)window % 4) != 0 ||
        ((uintptr_t)frames % 4) != 0)
        return M3T_EINVAL;
    long long gx = 2 * ((R + N - 1) / N);                    // twice the mean frame count: a longer clip's blocks loop
    gx = gx > 1024 ? 1024 : gx;
    const dim3 grid((unsigned)gx, (unsigned)(N < 65535 ? N : 65535));
    hipStream_t st = (hipStream_t)stream;
    if (dtype == 1)
        frame_batch_kernel<int16_t><<<grid, 256, 0, st>>>((const int16_t*)wave, n_samples, clips, N, R, n_fft, pad_mode, window, frames);
    else
        frame_batch_kernel<float><<<grid, 256, 0, st>>>((const float*)wave, n_samples, clips, N, R, n_fft, pad_mode, window, frames);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_audio_power_mel(const float* spec, long long R, int bins, int n_mels, const float* weights, const int* bands, int nnz,
                                   float* mel, void* stream) {
    if (R < 0) return M3T_EINVAL;
    if (R == 0) return 0;
    if (!spec || !weights || !bands || !mel || bins <= 0 || bins > 2048 || n_mels <= 0 || n_mels > 64 || nnz <= 0 || nnz > 4096)
        return M3T_EINVAL;
    if (((uintptr_t)spec % 4) != 0 || ((uintptr_t)weights % 4) != 0 || ((uintptr_t)bands % 4) != 0 || ((uintptr_t)mel % 4) != 0)
        return M3T_EINVAL;
    const long long blocks = (R + 3) / 4;
    const size_t lds = ((size_t)nnz + 4 * (size_t)bins) * sizeof(float);
    power_mel_kernel<<<(unsigned)(blocks < 8192 ? blocks : 8192), 256, lds, (hipStream_t)stream>>>(spec, R, bins, n_mels, weights, bands, nnz, mel);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_audio_db_stack(const float* mel, long long R, const long long* clips, int N, int T, int n_mels, int step, int width,
                                  float amin, float top_db, float* out, void* stream) {
    if (N < 0 || T < 0) return M3T_EINVAL;
    if (N == 0 || T == 0) return 0;
    if (!mel || !clips || !out || R <= 0 || n_mels <= 0 || step <= 0 || width <= 0 || amin <= 0.f ||
        (long long)T * width * n_mels > 0x7fffffffll)
        return M3T_EINVAL;
    if (((uintptr_t)mel % 4) != 0 || ((uintptr_t)clips % 8) != 0 || ((uintptr_t)out % 4) != 0) return M3T_EINVAL;
    db_stack_kernel<<<(unsigned)N, 256, 0, (hipStream_t)stream>>>(mel, R, clips, T, n_mels, step, width, amin, top_db, out);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_audio_db_stack_aug(const float* mel, long long R, const long long* clips, int N, const int* aug, const float* mixw, int T,
                                      int n_mels, int step, int width, float amin, float top_db, float* out, void* stream) {
    if (N < 0 || T < 0) return M3T_EINVAL;
    if (N == 0 || T == 0) return 0;
    if (!mel || !clips || !aug || !mixw || !out || R <= 0 || n_mels <= 0 || step <= 0 || width <= 0 || amin <= 0.f ||
        (long long)T * width * n_mels > 0x7fffffffll)
        return M3T_EINVAL;
    if (((uintptr_t)mel % 4) != 0 || ((uintptr_t)clips % 8) != 0 || ((uintptr_t)aug % 4) != 0 || ((uintptr_t)mixw % 4) != 0 ||
        ((uintptr_t)out % 4) != 0)
        return M3T_EINVAL;
    db_stack_aug_kernel<<<(unsigned)N, 256, 0, (hipStream_t)stream>>>(mel, R, clips, N, aug, mixw, T, n_mels, step, width, amin, top_db, out);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_stack_context_batch(const float* mels, long long total_rows, int n_mels, const long long* tracks, int N, int window,
                                       int step, int width, float* out, void* stream) {
    if (N < 0 || window < 0) return M3T_EINVAL;
    if (N == 0 || window == 0) return 0;
    if (!mels || !tracks || !out || total_rows <= 0 || n_mels <= 0 || step <= 0 || width <= 0) return M3T_EINVAL;
    if (((uintptr_t)mels % 4) != 0 || ((uintptr_t)tracks % 8) != 0 || ((uintptr_t)out % 4) != 0) return M3T_EINVAL;
    const long long cells = (long long)window * width * n_mels;
    const long long gx = (cells + 255) / 256;
    const dim3 grid((unsigned)(gx < 256 ? gx : 256), (unsigned)(N < 65535 ? N : 65535));
    stack_batch_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(mels, total_rows, n_mels, tracks, N, window, step, width, out);
    M3T_LAUNCH_CHECK();
    return 0;
}
