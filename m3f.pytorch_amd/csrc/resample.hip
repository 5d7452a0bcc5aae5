// Wave conversion on the device (m3t.audio.decode_waves): the raw interleaved 'data' bytes of a ragged batch of RIFF/WAVE clips of ONE source
// rate -> 16 kHz mono float32, what `librosa.load(path, sr=16000)` hands the reference (models/audioset_dataset.py:61,
// process/extract_melspec.py:13).  The rule is DESIGN.md 4c, the project's own restatement of libsndfile's normalised read, librosa.to_mono and
// resampy 0.2.2's `resample_f` with the 'kaiser_best' table -- none of the three has been run against it.
//
// One launch per rate.  A workgroup of 256 lanes takes one tile of 256 consecutive outputs of one clip (the clip is found by a binary search
// of the table's tile prefix):
//   1. it stages the source frames the tile's filter wings reach into LDS as mono float32 -- every sample kind is decoded and the channels are
//      averaged on the way in, from the bytes at their natural alignment (24-bit samples byte by byte); frames outside the clip stage as 0
//      and are never multiplied (the wings are cut at the clip's ends by the rule itself);
//   2. lane l owns output t0 + l.  Its time register is its wave's first one (accumulated on the host, one per 64 outputs, per rate) carried
//      on by l % 64 sequential fp64 additions, so every register is the plain loop's bit for bit; the fractional arithmetic is fp64 with explicit
//      _rn operations (no contraction: which table entry an output starts from is part of the rule);
//   3. the output is ONE fp32 accumulator, left wing then right wing in tap order, in resampy's own arithmetic: the weight
//      win[i] + eta * delta[i] and the product with the sample in fp64 (its table is float64), the sum stored to fp32 after every tap
//      (its output array is float32).  The interleaved (win, delta) table, 512 KB of float64, is gathered from L2;
//   4. plain vector stores; outputs n_res .. n_out - 1 are 0.0 (librosa's fix_length).
// No atomics, nothing order-dependent, nothing read back: reruns are bit-identical.  LDS per workgroup = the tile's span, 4.2 KB at
// 44.1 kHz, 9.3 KB at 96 kHz.  A 16 kHz clip takes wave_decode_kernel: decode and down-mix only.
// A table row that does not fit the buffers is caught per workgroup (nothing of that clip is read or written); the host refuses it first.
#include "common.h"

namespace {

constexpr int TILE = 256;
constexpr int SEG = 64;                  // outputs per host-accumulated register start: one per wave
constexpr int NWIN = 32769;              // entries of the half filter: 64 zero crossings x 512 + 1
constexpr int NUM_TABLE = 512;
constexpr int LDS_MAX_BYTES = 64 << 10;

enum { KIND_U8 = 0, KIND_I16 = 1, KIND_I24 = 2, KIND_I32 = 3, KIND_F32 = 4 };

__host__ __device__ inline int kind_bytes(int kind) { return kind == KIND_U8 ? 1 : kind == KIND_I16 ? 2 : kind == KIND_I24 ? 3 : 4; }

// one frame -> mono float32.  The scales are powers of two: every product is exact but i32's, whose int -> float conversion rounds once.
__device__ __forceinline__ float mono_frame(const uint8_t* __restrict__ p, int ch, int kind) {
    float acc = 0.f;
    for (int c = 0; c < ch; ++c) {
        float v;
        if (kind == KIND_I16) v = (float)((const int16_t*)p)[c] * (1.f / 32768.f);
        else if (kind == KIND_F32) v = ((const float*)p)[c];
        else if (kind == KIND_I24) {
            const uint8_t* q = p + 3 * c;
            v = (float)((int)q[0] | ((int)q[1] << 8) | ((int)(int8_t)q[2] << 16)) * (1.f / 8388608.f);
        } else if (kind == KIND_I32) v = (float)((const int32_t*)p)[c] * (1.f / 2147483648.f);
        else v = ((float)p[c] - 128.f) * (1.f / 128.f);
        acc = c ? acc + v : v;
    }
    return ch == 1 ? acc : __fdiv_rn(acc, (float)ch);
}

// one tap: float32(float64(acc) + (win + eta * delta) * float64(x)), every operation rounded on its own (no contraction)
__device__ __forceinline__ float tap(float acc, double2 w, double eta, float x) {
    return (float)__dadd_rn((double)acc, __dmul_rn(__dadd_rn(w.x, __dmul_rn(eta, w.y)), (double)x));
}

struct Clip { long long off, frames, out_off, n_res, n_out, tile; int ch, kind; bool ok; };

// the clip and the tile of workgroup `b`: the last row whose tile prefix (column 7) is <= b.  Uniform over the workgroup.
__device__ __forceinline__ Clip find_clip(const long long* __restrict__ clips, int N, long long b, long long n_bytes, long long n_out_total) {
    int lo = 0, hi = N - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (clips[(long long)mid * 8 + 7] <= b) lo = mid; else hi = mid - 1;
    }
    const long long* c = clips + (long long)lo * 8;
    Clip k;
    k.off = c[0]; k.frames = c[1]; k.out_off = c[4]; k.n_res = c[5]; k.n_out = c[6]; k.tile = b - c[7];
    const long long ch = c[2], kind = c[3];
    k.ch = (int)ch; k.kind = (int)kind;
    k.ok = ch >= 1 && ch <= 8 && kind >= 0 && kind <= 4 && k.off >= 0 && k.frames > 0 && k.out_off >= 0 && k.n_res >= 0 && k.n_out >= k.n_res &&
           k.tile >= 0 && k.tile * TILE < k.n_out && k.n_out <= n_out_total - k.out_off;
    if (k.ok) {
        const long long fb = ch * kind_bytes(k.kind), sb = k.kind == KIND_I24 ? 1 : kind_bytes(k.kind);
        k.ok = k.frames <= (n_bytes - k.off) / fb && (k.off % sb) == 0;
    }
    return k;
}

__global__ __launch_bounds__(TILE) void wave_decode_kernel(const uint8_t* __restrict__ bytes, long long n_bytes, const long long* __restrict__ clips,
                                                           int N, float* __restrict__ out, long long n_out_total) {
    const Clip k = find_clip(clips, N, blockIdx.x, n_bytes, n_out_total);
    if (!k.ok) return;
    const long long t = k.tile * TILE + threadIdx.x;
    if (t >= k.n_out) return;
    const long long fb = (long long)k.ch * kind_bytes(k.kind);
    out[k.out_off + t] = (t < k.n_res && t < k.frames) ? mono_frame(bytes + k.off + t * fb, k.ch, k.kind) : 0.f;
}

__global__ __launch_bounds__(TILE) void wave_resample_kernel(const uint8_t* __restrict__ bytes, long long n_bytes, const long long* __restrict__ clips,
                                                             int N, const double2* __restrict__ table, const double* __restrict__ starts,
                                                             long long n_starts, double ratio, double inc, int step, int lds_frames,
                                                             float* __restrict__ out, long long n_out_total) {
    extern __shared__ float x[];
    const Clip k = find_clip(clips, N, blockIdx.x, n_bytes, n_out_total);
    if (!k.ok || (k.tile + 1) * (TILE / SEG) > n_starts) return;
    const long long t0 = k.tile * TILE;
    const long long left = k.n_res - t0;
    const int nt = (int)(left < 0 ? 0 : left < TILE ? left : TILE);            // outputs of the tile the filter computes
    const double r0 = starts[k.tile * (TILE / SEG)];
    const int W = NWIN / step;                                                  // taps of a wing at most
    const long long n0 = (long long)r0;
    const long long lo = n0 - W + 1;                                            // first staged frame
    long long span = (long long)(r0 + inc * (double)(nt > 0 ? nt - 1 : 0)) + 1 - n0 + 2 * (long long)W;
    if (span > lds_frames) span = lds_frames;
    const long long fb = (long long)k.ch * kind_bytes(k.kind);
    if (nt > 0)
        for (long long j = threadIdx.x; j < span; j += TILE) {
            const long long f = lo + j;
            x[j] = (f >= 0 && f < k.frames) ? mono_frame(bytes + k.off + f * fb, k.ch, k.kind) : 0.f;
        }
    __syncthreads();
    const long long t = t0 + threadIdx.x;
    if (t >= k.n_out) return;
    float acc = 0.f;
    if ((int)threadIdx.x < nt) {
        double r = starts[k.tile * (TILE / SEG) + (threadIdx.x / SEG)];
        for (int i = 0; i < (int)(threadIdx.x % SEG); ++i) r = __dadd_rn(r, inc);   // the register of output t: sequential fp64 additions
        const long long n = (long long)r;
        if (!(n >= n0 && n - lo < span)) { out[k.out_off + t] = 0.f; return; }   // (`starts` that are not this rate's registers)
        const double scale = ratio < 1.0 ? ratio : 1.0;
        double frac = __dmul_rn(scale, __dsub_rn(r, (double)n));
        double idx = __dmul_rn(frac, (double)NUM_TABLE);
        int off = (int)idx;
        double eta = __dsub_rn(idx, (double)off);
        // both wings are cut by the clip's ends (the rule) and by the staged span (a guard that never bites a valid table)
        long long imax = min(n + 1, (long long)((NWIN - off) / step));
        imax = min(imax, n - lo + 1);
        const float* xs = x + (n - lo);
        int ti = off;
#pragma unroll 4
        for (int i = 0; i < (int)imax; ++i, ti += step) {
            const double2 w = table[ti];
            acc = tap(acc, w, eta, xs[-i]);
        }
        frac = __dsub_rn(scale, frac);
        idx = __dmul_rn(frac, (double)NUM_TABLE);
        off = (int)idx;
        eta = __dsub_rn(idx, (double)off);
        long long kmax = min(k.frames - n - 1, (long long)((NWIN - off) / step));
        kmax = min(kmax, lo + span - n - 1);
        ti = off;
#pragma unroll 4
        for (int i = 0; i < (int)kmax; ++i, ti += step) {
            const double2 w = table[ti];
            acc = tap(acc, w, eta, xs[i + 1]);
        }
    }
    out[k.out_off + t] = acc;
}

}  // namespace

extern "C" int m3t_wave_convert(const uint8_t* bytes, long long n_bytes, const long long* clips, int N, long long n_tiles, int rate,
                                const double* table, const double* starts, long long n_starts, float* out, long long n_out_total,
                                void* stream) {
    if (N < 0 || n_tiles < 0) return M3T_EINVAL;
    if (N == 0 || n_tiles == 0) return 0;
    if (!bytes || !clips || !out || n_bytes <= 0 || n_out_total <= 0 || rate <= 0 || n_tiles > 0x7fffffffll) return M3T_EINVAL;
    if (((uintptr_t)bytes % 4) != 0 || ((uintptr_t)clips % 8) != 0 || ((uintptr_t)out % 4) != 0) return M3T_EINVAL;
    if (rate == 16000) {
        wave_decode_kernel<<<(unsigned)n_tiles, TILE, 0, (hipStream_t)stream>>>(bytes, n_bytes, clips, N, out, n_out_total);
        M3T_LAUNCH_CHECK();
        return 0;
    }
    if (!table || !starts || n_starts <= 0 || ((uintptr_t)table % 16) != 0 || ((uintptr_t)starts % 8) != 0) return M3T_EINVAL;
    const double ratio = 16000.0 / (double)rate, inc = (double)rate / 16000.0;
    const int step = (int)((ratio < 1.0 ? ratio : 1.0) * NUM_TABLE);
    if (step < 1) return M3T_EINVAL;
    const long long lds_frames = (long long)(inc * (TILE - 1)) + 2ll * (NWIN / step) + 4;
    if (lds_frames * 4 > LDS_MAX_BYTES) return M3T_EINVAL;
    wave_resample_kernel<<<(unsigned)n_tiles, TILE, (size_t)lds_frames * 4, (hipStream_t)stream>>>(
        bytes, n_bytes, clips, N, (const double2*)table, starts, n_starts, ratio, inc, step, (int)lds_frames, out, n_out_total);
    M3T_LAUNCH_CHECK();
    return 0;
}
