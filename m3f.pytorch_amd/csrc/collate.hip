// The AffWild2 loader's collate step on the device (reference models/dataset.py:241-343 minus load_video): the side tracks of every video
// (SENet / AU features, log-Mel rows, valence / arousal and expression labels) live in flat device arrays, uploaded once, and ONE launch
// cuts a batch of windows out of them:
//     se_out / au_out   gather + transpose  [rows][C] -> [N][C][window]     (dataset.py:263-275, :313-314)
//     audio_out         m3t_stack_context_batch's rule                        (dataset.py:83-95, :276-278, :302-306)
//     valence / arousal / expr / expr_valid   row gathers                    (dataset.py:284-291, :315-319, :336-341)
// A workgroup does one job of one item: a 32 x 128 tile of a feature track, a slice of the audio clip, or the item's labels; the job kind is
// uniform per workgroup.  Every output is a copy: no arithmetic, no atomics, nothing order-dependent.  Every index is clamped on the
// device: whatever the tables hold, no byte outside the store is read, and an item whose video index is out of range writes zeros.
#include "common.h"

namespace {

// per-video table, long long [V][12] (include/m3t_hip.h)
enum { V_SE = 0, V_AU = 1, V_MEL = 2, V_VA = 3, V_EX = 4, V_FLAGS = 10, V_COLS = 12 };
enum { F_HAS_EXPR = 1, F_AUDIO_OK = 2 };

constexpr int TT = 32;            // frames of a tile
constexpr int TC = 128;           // channels of a tile: a row segment of 512 B, 16 B a lane over half a wave
constexpr int PITCH = TC + 4;     // 33 16-byte slots a row: the transposing ds_read_b128 of 16 lanes at 16 consecutive frames hit 16 slots
                                  // that differ mod 16 (all 64 banks once); the ds_write_b128 of 8 lanes are 128 contiguous bytes

struct Track { long long off, rows; };

struct Args {
    const float* se; long long se_rows; int se_stride, se_dim, se_vec;
    const float* au; long long au_rows; int au_stride, au_dim, au_vec;
    const float* mel; long long mel_rows; int n_mels, step, width, mel_vec;
    const float* va; long long va_rows;
    const long long* expr; long long expr_rows;
    const long long* videos; int n_videos;
    const int* items; int N, window;
    float* se_out; float* au_out; float* audio_out; float* valence_out; float* arousal_out;
    long long* expr_out; unsigned char* expr_valid_out;
    int se_jobs, au_jobs, audio_jobs;                        // workgroups an item per kind, then one for the labels
};

// the rows [off, off + rows) of a flat array of `total` rows, or no rows when the table entry does not fit it
__device__ __forceinline__ Track track_of(const long long* __restrict__ vrow, int kind, long long total) {
    Track t{0, 0};
    if (vrow) {
        const long long off = vrow[2 * kind], rows = vrow[2 * kind + 1];
        if (off >= 0 && rows > 0 && rows <= total && off <= total - rows) t = Track{off, rows};
    }
    return t;
}

// out[n][c][i] = src[off + min(start + min(i, tl - 1), rows - 1)][c] for one TT x TC tile: rows are read along C (16 bytes a lane where the
// row stride allows it), transposed through the padded LDS tile and written along T
__device__ __forceinline__ void gather_tile(const float* __restrict__ src, int stride, int dim, int vec, Track tr, long long start, int tl,
                                            int window, int n, int tile, float* __restrict__ out, float (*lds)[PITCH]) {
    const int nct = (dim + TC - 1) / TC;
    const int c0 = (tile % nct) * TC, t0 = (tile / nct) * TT;
    const int lo = threadIdx.x & 31, hi = threadIdx.x >> 5;
#pragma unroll
    for (int p = 0; p < TT / 8; ++p) {
        const int t = hi + 8 * p, i = t0 + t, c = c0 + 4 * lo;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (i < window && tr.rows > 0 && c < dim) {
            long long r = start + (i < tl ? i : tl - 1);
            r = r < tr.rows ? r : tr.rows - 1;
            const float* row = src + (tr.off + r) * stride;
            if (vec) {                                       // stride % 4 == 0, c % 4 == 0, c < dim <= stride: c + 4 <= stride
                v = *reinterpret_cast<const f32x4*>(row + c);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c + j < dim) v[j] = row[c + j];
            }
        }
        *reinterpret_cast<f32x4*>(&lds[t][4 * lo]) = v;
    }
    __syncthreads();
    const int i = t0 + lo;
#pragma unroll
    for (int p = 0; p < TC / 32; ++p) {
        const int s = hi + 8 * p;
        const f32x4 v = *reinterpret_cast<const f32x4*>(&lds[lo][4 * s]);
        if (i < window) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = c0 + 4 * s + j;
                if (c < dim) out[((long long)n * dim + c) * window + i] = v[j];
            }
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void window_collate_kernel(const Args a) {
    __shared__ __attribute__((aligned(16))) float lds[TT][PITCH];
    const int job = blockIdx.x;
    for (int n = blockIdx.y; n < a.N; n += gridDim.y) {
        const int v = a.items[3 * n];
        const long long* vrow = (v >= 0 && v < a.n_videos) ? a.videos + (long long)V_COLS * v : nullptr;
        long long start = a.items[3 * n + 1];
        int tl = a.items[3 * n + 2];
        start = start < 0 ? 0 : start;
        tl = tl < 1 ? 1 : (tl > a.window ? a.window : tl);
        const long long flags = vrow ? vrow[V_FLAGS] : 0;
        int j = job;
        if (j < a.se_jobs + a.au_jobs) {                     // one call site for both feature kinds
            const bool is_se = j < a.se_jobs;
            const Track tr = is_se ? track_of(vrow, V_SE, a.se_rows) : track_of(vrow, V_AU, a.au_rows);
            gather_tile(is_se ? a.se : a.au, is_se ? a.se_stride : a.au_stride, is_se ? a.se_dim : a.au_dim, is_se ? a.se_vec : a.au_vec, tr,
                        start, tl, a.window, n, is_se ? j : j - a.se_jobs, is_se ? a.se_out : a.au_out, lds);
            continue;
        }
        j -= a.se_jobs + a.au_jobs;
        if (j < a.audio_jobs) {
            // out[n][i][k n_mels + c] = r < rows ? mel[off + r][c] : 0,  r = (start + i') step + k     (stack_batch_kernel of audio_ingest.hip)
            Track tr = track_of(vrow, V_MEL, a.mel_rows);
            if (!(flags & F_AUDIO_OK)) tr.rows = 0;
            const int W = a.width * a.n_mels;
            const long long cells = (long long)a.window * W;
            float* o = a.audio_out + (long long)n * cells;
            if (a.mel_vec) {                                 // n_mels % 4 == 0: a 16-byte cell never crosses a mel row
                for (long long q = (long long)j * 256 + threadIdx.x; 4 * q < cells; q += 256ll * a.audio_jobs) {
                    const long long i = 4 * q, f = i / W;
                    const int r = (int)(i - f * W), k = r / a.n_mels, cc = r - k * a.n_mels;
                    f32x4 val = {0.f, 0.f, 0.f, 0.f};
                    const long long row = (start + (f < tl ? f : tl - 1)) * a.step + k;
                    if (row < tr.rows) val = *reinterpret_cast<const f32x4*>(a.mel + (tr.off + row) * a.n_mels + cc);
                    *reinterpret_cast<f32x4*>(o + i) = val;
                }
            } else {
                for (long long i = (long long)j * 256 + threadIdx.x; i < cells; i += 256ll * a.audio_jobs) {
                    const long long f = i / W;
                    const int r = (int)(i - f * W), k = r / a.n_mels, cc = r - k * a.n_mels;
                    const long long row = (start + (f < tl ? f : tl - 1)) * a.step + k;
                    o[i] = row < tr.rows ? a.mel[(tr.off + row) * a.n_mels + cc] : 0.f;
                }
            }
            continue;
        }
        // labels: va[off + start + i'][0 | 1] as stored; e = expr[off + start + i']: valid = e >= 0, out = clamp(e, 0, 6)
        const Track tv = track_of(vrow, V_VA, a.va_rows);
        Track te = track_of(vrow, V_EX, a.expr_rows);
        if (!(flags & F_HAS_EXPR)) te.rows = 0;
        for (int i = threadIdx.x; i < a.window; i += 256) {
            const long long r = start + (i < tl ? i : tl - 1);
            const long long o = (long long)n * a.window + i;
            if (a.valence_out) {
                float val = 0.f, aro = 0.f;
                if (tv.rows > 0) {
                    const long long rr = tv.off + (r < tv.rows ? r : tv.rows - 1);
                    val = a.va[2 * rr];
                    aro = a.va[2 * rr + 1];
                }
                a.valence_out[o] = val;
                a.arousal_out[o] = aro;
            }
            if (a.expr_out) {
                long long e = 0;
                bool ok = false;
                if (te.rows > 0) {
                    e = a.expr[te.off + (r < te.rows ? r : te.rows - 1)];
                    ok = e >= 0;
                    e = e < 0 ? 0 : (e > 6 ? 6 : e);
                }
                a.expr_out[o] = e;
                a.expr_valid_out[o] = ok ? 1 : 0;
            }
        }
    }
}

inline bool misaligned(const void* p, size_t n) { return ((uintptr_t)p % n) != 0; }

}  // namespace

extern "C" int m3t_window_collate(const float* se, long long se_rows, int se_stride, int se_dim,
                                  const float* au, long long au_rows, int au_stride, int au_dim,
                                  const float* mel, long long mel_rows, int n_mels, int step, int width,
                                  const float* va, long long va_rows, const long long* expr, long long expr_rows,
                                  const long long* videos, int n_videos, const int* items, int N, int window,
                                  float* se_out, float* au_out, float* audio_out, float* valence_out, float* arousal_out,
                                  long long* expr_out, unsigned char* expr_valid_out, void* stream) {
    if (N < 0 || window < 0) return M3T_EINVAL;
    if (N == 0 || window == 0) return 0;
    if (!videos || !items || n_videos <= 0 || misaligned(videos, 8) || misaligned(items, 4)) return M3T_EINVAL;
    if (se_out && (!se || se_rows <= 0 || se_dim <= 0 || se_dim > se_stride || misaligned(se, 4) || misaligned(se_out, 4))) return M3T_EINVAL;
    if (au_out && (!au || au_rows <= 0 || au_dim <= 0 || au_dim > au_stride || misaligned(au, 4) || misaligned(au_out, 4))) return M3T_EINVAL;
    if (audio_out && (!mel || mel_rows <= 0 || n_mels <= 0 || step <= 0 || width <= 0 || misaligned(mel, 4) || misaligned(audio_out, 4) ||
                      (long long)window * width * n_mels > 0x7fffffffll))
        return M3T_EINVAL;
    if ((valence_out == nullptr) != (arousal_out == nullptr) || (expr_out == nullptr) != (expr_valid_out == nullptr)) return M3T_EINVAL;
    if (valence_out && (!va || va_rows <= 0 || misaligned(va, 4) || misaligned(valence_out, 4) || misaligned(arousal_out, 4))) return M3T_EINVAL;
    if (expr_out && (expr_rows < 0 || (expr_rows > 0 && !expr) || misaligned(expr, 8) || misaligned(expr_out, 8))) return M3T_EINVAL;
    Args a;
    a.se = se; a.se_rows = se_rows; a.se_stride = se_stride; a.se_dim = se_dim;
    a.se_vec = (se_out && se_stride % 4 == 0 && !misaligned(se, 16)) ? 1 : 0;
    a.au = au; a.au_rows = au_rows; a.au_stride = au_stride; a.au_dim = au_dim;
    a.au_vec = (au_out && au_stride % 4 == 0 && !misaligned(au, 16)) ? 1 : 0;
    a.mel = mel; a.mel_rows = mel_rows; a.n_mels = n_mels; a.step = step; a.width = width;
    a.mel_vec = (audio_out && n_mels % 4 == 0 && !misaligned(mel, 16) && !misaligned(audio_out, 16)) ? 1 : 0;
    a.va = va; a.va_rows = va_rows; a.expr = expr; a.expr_rows = expr ? expr_rows : 0;
    a.videos = videos; a.n_videos = n_videos; a.items = items; a.N = N; a.window = window;
    a.se_out = se_out; a.au_out = au_out; a.audio_out = audio_out; a.valence_out = valence_out; a.arousal_out = arousal_out;
    a.expr_out = expr_out; a.expr_valid_out = expr_valid_out;
    const int ttiles = cdiv(window, TT);
    a.se_jobs = se_out ? cdiv(se_dim, TC) * ttiles : 0;
    a.au_jobs = au_out ? cdiv(au_dim, TC) * ttiles : 0;
    a.audio_jobs = 0;
    if (audio_out) {                                         // four 16-byte (or 4-byte) cells a thread, 64 workgroups an item at the most
        const long long cells = (long long)window * width * n_mels / (a.mel_vec ? 4 : 1);
        const long long jobs = (cells + 1023) / 1024;
        a.audio_jobs = (int)(jobs < 64 ? jobs : 64);
    }
    const long long jobs = (long long)a.se_jobs + a.au_jobs + a.audio_jobs + ((valence_out || expr_out) ? 1 : 0);
    if (jobs == 0) return 0;
    if (jobs > 0x7fffffffll) return M3T_EINVAL;
    const dim3 grid((unsigned)jobs, (unsigned)(N < 65535 ? N : 65535));
    window_collate_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(a);
    M3T_LAUNCH_CHECK();
    return 0;
}
