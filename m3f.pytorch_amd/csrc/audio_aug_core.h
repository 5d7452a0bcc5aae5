// The cell rule of the augmented AudioSet ingest (csrc/audio_ingest.hip, m3t_audio_db_stack_aug) as one text for the device and the host:
// which value a cell of the stacked [T][width n_mels] rows takes from ONE clip once the reference's spec_augment
// (models/audioset_dataset.py:17-55) has run on that clip's dB spectrogram [n_mels][tau], tau = nf, before the context stack of :77-85.
// The kernel compiles it for the GPU; csrc/audio_aug_host_check.cpp compiles the same text for the host and sweeps it against a direct
// restatement (mask the spectrogram, then stack).  Nothing here touches anything but its arguments, and a mask is only ever COMPARED
// with a position: whatever the table holds, no address is formed from it.
#pragma once

#if defined(__HIPCC__)
#define AUG_HD __host__ __device__ __forceinline__
#else
#define AUG_HD inline
#endif

// per-clip int table, int [N][AUG_INTS]: the two counts, the partner clip of the mix (-1: no mix), then (f0, f) x 4 and (t0, t) x 4
enum { AUG_NFREQ = 0, AUG_NTIME = 1, AUG_PARTNER = 2, AUG_FMASK = 4, AUG_TMASK = 12, AUG_INTS = 20, AUG_MAX_MASKS = 4 };

AUG_HD int aug_count(int v) { return v < 0 ? 0 : (v > AUG_MAX_MASKS ? AUG_MAX_MASKS : v); }

// spec[:, f0:f0+f, :] = 0 and spec[:, :, t0:t0+t] = 0 (:46, :53) seen from one cell: band `band` of frame `row`
AUG_HD bool aug_masked(const int* p, long long row, int band) {
    const int nfm = aug_count(p[AUG_NFREQ]), ntm = aug_count(p[AUG_NTIME]);
    for (int q = 0; q < nfm; ++q) {
        const long long f0 = p[AUG_FMASK + 2 * q], f = p[AUG_FMASK + 2 * q + 1];
        if (band >= f0 && band < f0 + f) return true;
    }
    for (int q = 0; q < ntm; ++q) {
        const long long t0 = p[AUG_TMASK + 2 * q], t = p[AUG_TMASK + 2 * q + 1];
        if (row >= t0 && row < t0 + t) return true;
    }
    return false;
}

// Cell i < T * width * n_mels of a clip's stacked rows: i = (t * width + k) * n_mels + band shows band `band` of frame t * step + k.
// -> the cell's index into the clip's own [nf][n_mels] spectrogram, or -1 when the cell is exactly 0.0: a frame >= nf (the stack's zero
// padding, :82-83) or a masked cell (an assignment: whatever stood there, NaN and inf included, is gone).  p == nullptr: no masks.
AUG_HD long long aug_cell(const int* p, long long nf, int n_mels, int step, int width, long long i) {
    const long long W = (long long)width * n_mels;
    const long long t = i / W, r = i - t * W, k = r / n_mels;
    const int band = (int)(r - k * n_mels);
    const long long row = t * step + k;
    if (row >= nf) return -1;
    if (p && aug_masked(p, row, band)) return -1;
    return row * n_mels + band;
}
