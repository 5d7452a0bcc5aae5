// The AudioSet loader's label half on the device (reference models/audioset_dataset.py:116-118, :131): the multi-hot rows of every clip of a
// split live in ONE uint8 matrix [n_files][n_classes], uploaded once (m3t.audioset.WaveStore), and one launch writes a batch's float32 rows
//     out[n][c] = (float) table[items[n]][c]
// A flat grid-stride over N * n_classes cells: byte loads, float stores, no atomics, nothing order-dependent.  An item outside
// [0, n_files) leaves its row untouched (the host refuses such an item first): no byte outside the table is read whatever `items` holds.
// m3t_label_rows_mix is the same launch for a batch that is mixed (mixup, after the reference's spec_augment, audioset_dataset.py:17-55):
//     out[n][c] = lam32[n] * table[items[n]][c] + om32[n] * table[items[partner[n]]][c]
#include "common.h"
#include "audio_aug_core.h"

namespace {

__global__ __launch_bounds__(256) void label_rows_kernel(const uint8_t* __restrict__ table, long long n_files, int n_classes,
                                                         const long long* __restrict__ items, long long cells, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cells; i += 256ll * gridDim.x) {
        const long long n = i / n_classes;
        const int c = (int)(i - n * n_classes);
        const long long f = items[n];
        if (f < 0 || f >= n_files) continue;
        out[i] = (float)table[f * n_classes + c];
    }
}

// label_rows_kernel with the batch's mix (m3t_audio_db_stack_aug's tables): a row with a partner p >= 0 is lam32 * row + om32 * the
// partner ITEM's row, two rounded products and one rounded sum; a row without one is the plain copy.  A partner outside [-1, N) or an item
// outside the table leaves the row untouched.
__global__ __launch_bounds__(256) void label_rows_mix_kernel(const uint8_t* __restrict__ table, long long n_files, int n_classes,
                                                             const long long* __restrict__ items, int N, const int* __restrict__ aug,
                                                             const float* __restrict__ mixw, long long cells, float* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < cells; i += 256ll * gridDim.x) {
        const long long n = i / n_classes;
        const int c = (int)(i - n * n_classes);
        const long long f = items[n];
        const int p = aug[AUG_INTS * n + AUG_PARTNER];
        if (f < 0 || f >= n_files || p < -1 || p >= N) continue;
        const float a = (float)table[f * n_classes + c];
        if (p < 0) {
            out[i] = a;
            continue;
        }
        const long long g = items[p];
        if (g < 0 || g >= n_files) continue;
        out[i] = __fadd_rn(__fmul_rn(mixw[2 * n], a), __fmul_rn(mixw[2 * n + 1], (float)table[g * n_classes + c]));
    }
}

}  // namespace

extern "C" int m3t_label_rows_mix(const uint8_t* table, long long n_files, int n_classes, const long long* items, int N, const int* aug,
                                  const float* mixw, float* out, void* stream) {
    if (N < 0) return M3T_EINVAL;
    if (N == 0) return 0;
    if (!table || !items || !aug || !mixw || !out || n_files <= 0 || n_classes <= 0) return M3T_EINVAL;
    if (((uintptr_t)items % 8) != 0 || ((uintptr_t)aug % 4) != 0 || ((uintptr_t)mixw % 4) != 0 || ((uintptr_t)out % 4) != 0) return M3T_EINVAL;
    const long long cells = (long long)N * n_classes;
    const long long blocks = (cells + 255) / 256;
    label_rows_mix_kernel<<<(unsigned)(blocks < 2048 ? blocks : 2048), 256, 0, (hipStream_t)stream>>>(table, n_files, n_classes, items, N, aug,
                                                                                                    mixw, cells, out);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_label_rows(const uint8_t* table, long long n_files, int n_classes, const long long* items, int N, float* out,
                              void* stream) {
    if (N < 0) return M3T_EINVAL;
    if (N == 0) return 0;
    if (!table || !items || !out || n_files <= 0 || n_classes <= 0) return M3T_EINVAL;
    if (((uintptr_t)items % 8) != 0 || ((uintptr_t)out % 4) != 0) return M3T_EINVAL;
    const long long cells = (long long)N * n_classes;
    const long long blocks = (cells + 255) / 256;
    label_rows_kernel<<<(unsigned)(blocks < 2048 ? blocks : 2048), 256, 0, (hipStream_t)stream>>>(table, n_files, n_classes, items, cells, out);
    M3T_LAUNCH_CHECK();
    return 0;
}
