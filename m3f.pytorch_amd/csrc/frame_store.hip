// The resident JPEG frame store's batch step (m3t.jpeg.FrameStore): the scan bytes of every frame of the corpus live on the device in a few
// large chunks, uploaded once, and ONE launch assembles a batch's byte stream -- what m3t_jpeg_decode_walk takes -- from one small int table:
//     dst[dst_off .. dst_off + bytes) = chunk[src_off .. src_off + bytes)   for every row (chunk, src_off, dst_off, bytes) of the table
//     every other 16-byte granule of dst[0 .. dst_bytes) = 0               (the padding behind the rows, pack's 16 zero bytes at the end)
// Form: a flat grid-stride over the DESTINATION granules.  A lane finds its granule's row by a binary search of the destination-offset column
// (ceil(log2(m + 1)) steps over a table of m * 16 bytes that stays in cache), then moves one granule: a 16-byte load and a 16-byte store.
// The rows are ragged (1 KB to 48 KB a frame): cutting the destination rather than the rows keeps every lane's work the same whatever the
// sizes, the lanes of a wave write 1 KiB of consecutive bytes and -- but for the one or two rows that end inside it -- read consecutive
// bytes, and every granule of dst is written exactly once, so there is no memset in front and nothing that depends on an order.  No atomics,
// no communication between workgroups, no LDS.
#include "common.h"

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct GatherArgs {
    const long long* chunks;      // device: the chunks' addresses
    const i32x4* rows;            // device [m]: chunk, src_off, dst_off, bytes
    u32x4* dst;
    long long granules;           // dst_bytes / 16
    int m, n_chunks;
};

__global__ __launch_bounds__(256) void jpeg_gather_kernel(const GatherArgs a) {
    for (long long g = blockIdx.x * 256ll + threadIdx.x; g < a.granules; g += 256ll * gridDim.x) {
        const long long off = 16 * g;
        int lo = 0, hi = a.m;                                  // -> lo = the number of rows that start at or before `off`
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.rows[mid].z <= off) lo = mid + 1; else hi = mid;
        }
        u32x4 v = {0u, 0u, 0u, 0u};
        if (lo > 0) {
            const i32x4 r = a.rows[lo - 1];
            const long long rel = off - r.z;                   // >= 0; a multiple of 16 as every column but the chunk is
            if (rel < r.w && r.x >= 0 && r.x < a.n_chunks && r.y >= 0)
                v = *reinterpret_cast<const u32x4*>(reinterpret_cast<const uint8_t*>(a.chunks[r.x]) + r.y + rel);
        }
        a.dst[g] = v;
    }
}

inline bool misaligned(const void* p, size_t n) { return ((uintptr_t)p % n) != 0; }

}  // namespace

extern "C" int m3t_jpeg_gather(const long long* chunks_h, const long long* chunk_bytes_h, int n_chunks, const long long* chunks_d,
                               const int* rows_h, const int* rows_d, int m, uint8_t* dst, long long dst_bytes, void* stream) {
    if (m < 0 || n_chunks < 0 || !dst || misaligned(dst, 16) || dst_bytes < 16 || (dst_bytes % 16) != 0 || dst_bytes > 0x7fffffffll)
        return M3T_EINVAL;
    if (m > 0) {
        if (!chunks_h || !chunk_bytes_h || !chunks_d || !rows_h || !rows_d || n_chunks == 0 || misaligned(chunks_d, 8) || misaligned(rows_d, 16))
            return M3T_EINVAL;
        for (int c = 0; c < n_chunks; ++c)
            if (chunks_h[c] == 0 || (chunks_h[c] % 16) != 0 || chunk_bytes_h[c] < 0) return M3T_EINVAL;
        long long end = 0;                                     // one past the last destination byte of the rows so far
        for (int r = 0; r < m; ++r) {
            const int chunk = rows_h[4 * r], src = rows_h[4 * r + 1], to = rows_h[4 * r + 2], bytes = rows_h[4 * r + 3];
            if (chunk < 0 || chunk >= n_chunks || src < 0 || to < 0 || bytes < 0 || ((src | to | bytes) & 15) != 0) return M3T_EINVAL;
            if ((long long)src + bytes > chunk_bytes_h[chunk]) return M3T_EINVAL;
            if (to < end || (long long)to + bytes > dst_bytes - 16) return M3T_EINVAL;
            end = (long long)to + bytes;
        }
    }
    GatherArgs a;
    a.chunks = chunks_d; a.rows = reinterpret_cast<const i32x4*>(rows_d); a.dst = reinterpret_cast<u32x4*>(dst);
    a.granules = dst_bytes / 16; a.m = m; a.n_chunks = n_chunks;
    const long long blocks = (a.granules + 255) / 256;          // eight workgroups a CU hold the machine; more only shorten the stride
    jpeg_gather_kernel<<<(unsigned)(blocks < 2048 ? blocks : 2048), 256, 0, (hipStream_t)stream>>>(a);
    M3T_LAUNCH_CHECK();
    return 0;
}
