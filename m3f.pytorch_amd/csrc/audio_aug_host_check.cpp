// csrc/audio_aug_core.h -- the cell rule of m3t_audio_db_stack_aug -- compiled for the host and swept against a direct restatement of what
// the reference does (models/audioset_dataset.py:17-55, then :77-85): fill a spectrogram [n_mels][tau] with its own indices, set the masked
// bands and frames to zero as slices, stack `width` frames every `step`, pad a short window with zeros.  A plain program with its own main,
// meant to be built with -fsanitize=address,undefined: every array is a heap block of its exact size, so a read one past a row shows.
//   usage: audio_aug_host_check          runs the built-in sweep; exit 0: every cell of every case agrees
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "audio_aug_core.h"

namespace {

struct Case {
    int T, n_mels, step, width;
    long long nf;
    int p[AUG_INTS];
};

// the reference, literally: zero slices of spec[band][frame], then out[t][k * n_mels + band] = frame t * step + k < nf ? spec : 0
std::vector<long long> restate(const Case& c) {
    std::vector<long long> spec((size_t)(c.n_mels * c.nf));
    for (int b = 0; b < c.n_mels; ++b)
        for (long long f = 0; f < c.nf; ++f) spec[(size_t)(b * c.nf + f)] = 1 + f * c.n_mels + b;     // 1 + the index aug_cell gives
    for (int q = 0; q < c.p[AUG_NFREQ]; ++q) {
        const int f0 = c.p[AUG_FMASK + 2 * q], f = c.p[AUG_FMASK + 2 * q + 1];
        for (int b = f0; b < f0 + f && b < c.n_mels; ++b)
            for (long long fr = 0; fr < c.nf; ++fr) spec[(size_t)(b * c.nf + fr)] = 0;
    }
    for (int q = 0; q < c.p[AUG_NTIME]; ++q) {
        const int t0 = c.p[AUG_TMASK + 2 * q], t = c.p[AUG_TMASK + 2 * q + 1];
        for (long long fr = t0; fr < t0 + t && fr < c.nf; ++fr)
            for (int b = 0; b < c.n_mels; ++b) spec[(size_t)(b * c.nf + fr)] = 0;
    }
    std::vector<long long> out((size_t)c.T * c.width * c.n_mels, 0);
    for (int t = 0; t < c.T; ++t)
        for (int k = 0; k < c.width; ++k) {
            const long long fr = (long long)t * c.step + k;
            if (fr >= c.nf) continue;
            for (int b = 0; b < c.n_mels; ++b) out[((size_t)t * c.width + k) * c.n_mels + b] = spec[(size_t)(b * c.nf + fr)];
        }
    return out;
}

int check(const Case& c, bool with_table) {
    // the table as a heap block of its exact size
    int* p = (int*)malloc(sizeof(int) * AUG_INTS);
    for (int i = 0; i < AUG_INTS; ++i) p[i] = c.p[i];
    Case plain = c;
    if (!with_table) plain.p[AUG_NFREQ] = plain.p[AUG_NTIME] = 0;
    const std::vector<long long> want = restate(plain);
    int bad = 0;
    for (long long i = 0; i < (long long)want.size(); ++i) {
        const long long got = aug_cell(with_table ? p : nullptr, c.nf, c.n_mels, c.step, c.width, i);
        if (got + 1 != want[(size_t)i] || got >= c.nf * c.n_mels) {
            if (!bad)
                fprintf(stderr, "T %d nf %lld mels %d step %d width %d cell %lld: rule %lld, restatement %lld\n", c.T, c.nf, c.n_mels, c.step,
                        c.width, i, got, want[(size_t)i] - 1);
            ++bad;
        }
    }
    free(p);
    return bad;
}

unsigned long long rng = 0x9e3779b97f4a7c15ull;
int draw(int lo, int hi) {              // uniform int in [lo, hi], xorshift
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return lo + (int)(rng % (unsigned long long)(hi - lo + 1));
}

}  // namespace

int main() {
    int cases = 0, bad = 0;
    const int shapes[][3] = {{40, 3, 5}, {40, 1, 1}, {7, 2, 3}, {1, 3, 5}};             // n_mels, step, width
    for (const auto& s : shapes)
        for (int T : {1, 2, 7, 32})
            for (long long nf : {1ll, 2ll, 3ll * T, 3ll * T + 1, 3ll * T + 2, 3ll * T + 5, 1ll * T, 100ll}) {
                for (int rep = 0; rep < 24; ++rep) {
                    Case c{};
                    c.T = T, c.n_mels = s[0], c.step = s[1], c.width = s[2], c.nf = nf;
                    c.p[AUG_PARTNER] = -1;
                    c.p[AUG_NFREQ] = rep < 2 ? 0 : draw(0, AUG_MAX_MASKS);
                    c.p[AUG_NTIME] = rep < 2 ? 0 : draw(0, AUG_MAX_MASKS);
                    for (int q = 0; q < AUG_MAX_MASKS; ++q) {                              // (pairs beyond the counts are filled too: never read)
                        const int f = rep % 3 == 0 ? draw(0, c.n_mels) : draw(0, c.n_mels / 2);
                        c.p[AUG_FMASK + 2 * q] = rep % 4 == 1 ? c.n_mels - f : draw(0, c.n_mels - f);          // f0 + f == n_mels
                        c.p[AUG_FMASK + 2 * q + 1] = f;
                        const int t = rep % 5 == 0 ? (int)nf : draw(0, (int)(nf < 20 ? nf : 20));               // the whole clip
                        c.p[AUG_TMASK + 2 * q] = rep % 4 == 2 ? (int)nf - t : draw(0, (int)nf - t);             // t0 + t == tau
                        c.p[AUG_TMASK + 2 * q + 1] = t;
                    }
                    bad += check(c, true) + check(c, false);
                    cases += 2;
                }
            }
    // counts outside [0, 4] are clamped, never followed
    Case c{};
    c.T = 4, c.n_mels = 40, c.step = 3, c.width = 5, c.nf = 13;
    c.p[AUG_NFREQ] = 1000, c.p[AUG_NTIME] = -7;
    for (int q = 0; q < AUG_MAX_MASKS; ++q) c.p[AUG_FMASK + 2 * q] = 10 * q, c.p[AUG_FMASK + 2 * q + 1] = 3;
    Case clamped = c;
    clamped.p[AUG_NFREQ] = AUG_MAX_MASKS, clamped.p[AUG_NTIME] = 0;
    {
        const std::vector<long long> want = restate(clamped);
        for (long long i = 0; i < (long long)want.size(); ++i) bad += aug_cell(c.p, c.nf, c.n_mels, c.step, c.width, i) + 1 != want[(size_t)i];
        ++cases;
    }
    if (bad) {
        fprintf(stderr, "audio_aug_host_check: %d cells disagree\n", bad);
        return 1;
    }
    printf("audio_aug_host_check: %d cases agree\n", cases);
    return 0;
}
