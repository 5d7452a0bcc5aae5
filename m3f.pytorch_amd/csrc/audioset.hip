// The AudioSet loader's label half on the device (reference models/audioset_dataset.py:116-118, :131): the multi-hot rows of every clip of a
// split live in ONE uint8 matrix [n_files][n_classes], uploaded once (m3t.audioset.WaveStore), and one launch writes a batch's float32 rows
//     out[n][c] = (float) table[items[n]][c]
// A flat grid-stride over N * n_classes cells: byte loads, float stores, no atomics, nothing order-dependent.  An item outside
// [0, n_files) leaves its row untouched (the host refuses such an item first): no byte outside the table is read whatever `items` holds.
#include "common.h"

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

}  // namespace

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
