// Batched baseline-JPEG decode on the GPU: the first line of the reference's load_video (models/dataset.py:64, cv2.imread of one JPEG per
// frame) for a whole batch, from the packed streams m3t.jpeg.pack builds to the uint8 [N][Ts][H][W][3] buffer every later stage takes.
// The sequential rules live in jpeg_core.h (shared with the host check program); this file is their schedule, two launches:
//   1. jpeg_entropy_idct_kernel: one wave per entropy-coded segment (a restart interval, or the whole scan).  The stream comes through
//      LDS in 1 KiB windows read as 16-byte granules, the image's Huffman and quantisation tables sit in LDS beside it.  The symbol walk is
//      sequential: every lane runs it on the same (uniform) state and lane 0 stores the coefficients; after each MCU the lanes take one
//      column, then one row, of its blocks through the integer IDCT and store eight samples each into the block-padded component planes
//      of the image's workspace slot.  An MCU belongs to exactly one segment, so no plane byte has two writers.
//   2. jpeg_pixel_kernel: four pixels a lane -- fancy chroma upsampling from the planes, colour, the caller's channel order -- as three
//      dwords where the destination allows, bytes otherwise.
// Parallel Huffman decoding inside one segment (speculative / self-synchronising) is the follow-up, not attempted here.
#include "common.h"
#include "jpeg_core.h"

namespace {

__constant__ uint8_t k_zigzag[64] = JPEG_ZIGZAG_INIT;

struct JpegArgs {
    const uint8_t* stream; const int* img; const int* seg; const int* slot; const int* quant; const int* huff;
    uint8_t* dst; uint8_t* ws; int* status;
    long long stream_bytes, slot_bytes;
    int n, n_segs, n_quant, n_huff, H, W, order;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(64) void jpeg_entropy_idct_kernel(JpegArgs a) {
    __shared__ uint4 win4[JPEG_WINDOW / 16];
    __shared__ int huff[6 * JPEG_HUFF_INTS];
    __shared__ int quant[3 * JPEG_QUANT_INTS];
    __shared__ int coef32[6 * 32];
    __shared__ int32_t wsp[6 * 64];
    __shared__ uint8_t zz[64];
    const int lane = threadIdx.x;
    const int* sg = a.seg + (long long)JPEG_SEG_COLS * blockIdx.x;
    const int i = sg[0];
    if (i < 0 || i >= a.n) return;                           // (uniform; the host validated the tables, the device only keeps inside them)
    const int* img = a.img + (long long)JPEG_IMG_COLS * i;
    if (!(img[0] & 1)) return;
    int im[JPEG_IMG_COLS];
#pragma unroll
    for (int c = 0; c < JPEG_IMG_COLS; ++c) im[c] = img[c];
    im[1] = im[1] == 1 ? 1 : 3;
    im[2] = im[1] == 1 ? 1 : clampi(im[2], 1, 2);
    im[3] = im[1] == 1 ? 1 : clampi(im[3], 1, 2);
    const JpegGeom g = jpeg_geom(im, a.H, a.W);
    const int total = g.mcus_x * g.mcus_y, Ri = clampi(im[4], 1, total);
    const int k = (int)blockIdx.x - im[5];
    if (k < 0 || (long long)k * Ri >= total) return;
    const int m0 = k * Ri, m1 = min(m0 + Ri, total);
    const long long off = min(max((long long)sg[1], 0ll), a.stream_bytes);
    const long long end = min(off + max(sg[2], 0), a.stream_bytes);

    zz[lane] = k_zigzag[lane];
    for (int c = 0; c < g.ncomp; ++c) {
        const int* hd = a.huff + (long long)JPEG_HUFF_INTS * clampi(im[10 + c], 0, a.n_huff - 1);
        const int* ha = a.huff + (long long)JPEG_HUFF_INTS * clampi(im[13 + c], 0, a.n_huff - 1);
        for (int j = lane; j < JPEG_HUFF_INTS; j += 64) {
            huff[(2 * c) * JPEG_HUFF_INTS + j] = hd[j];
            huff[(2 * c + 1) * JPEG_HUFF_INTS + j] = ha[j];
        }
        if (lane < JPEG_QUANT_INTS) quant[c * JPEG_QUANT_INTS + lane] = a.quant[(long long)JPEG_QUANT_INTS * clampi(im[7 + c], 0, a.n_quant - 1) + lane];
    }
    int16_t* coef = reinterpret_cast<int16_t*>(coef32);
    const uint16_t* q16 = reinterpret_cast<const uint16_t*>(quant);
    uint8_t* planes = a.ws + a.slot_bytes * i;

    JpegReader r;
    jpeg_reader_init(r, reinterpret_cast<const uint8_t*>(win4), (int)off, 0, (int)off, (int)end);
    int pred[3] = {0, 0, 0};
    bool dead = false;
    for (int m = m0; m < m1; ++m) {
        __syncthreads();                                     // (the previous MCU's rows are read; the tables are in place)
#pragma unroll
        for (int j = 0; j < 3; ++j) coef32[lane + 64 * j] = 0;
        __syncthreads();
        for (int b = 0; b < g.blocks && !dead; ++b) {
            // every lane holds the same reader, so this is uniform: keep 512 bytes of stream in front of the reader
            if (r.pos + 512 > r.win_base + r.win_len && r.win_base + r.win_len < r.end) {
                __syncthreads();
                const int base = r.pos & ~15;
                const long long o = (long long)base + 16 * lane;
                win4[lane] = (o + 16 <= a.stream_bytes) ? *reinterpret_cast<const uint4*>(a.stream + o) : make_uint4(0u, 0u, 0u, 0u);
                __syncthreads();
                r.win_base = base; r.win_len = JPEG_WINDOW;
            }
            int comp, y0, x0;
            jpeg_block_place(g, m, b, comp, y0, x0);
            const JpegHuff hd = jpeg_huff_at(huff + (2 * comp) * JPEG_HUFF_INTS), ha = jpeg_huff_at(huff + (2 * comp + 1) * JPEG_HUFF_INTS);
            const int st = jpeg_decode_block(r, hd, ha, zz, pred[comp], coef + 64 * b, lane == 0);
            if (st) { r.status |= st; dead = true; }         // the rest of the segment stays zero coefficients
        }
        __syncthreads();
        const int b = lane >> 3, t = lane & 7;
        int comp = 0, y0 = 0, x0 = 0;
        if (b < g.blocks) {
            jpeg_block_place(g, m, b, comp, y0, x0);
            jpeg_idct_col(coef + 64 * b, q16 + 64 * comp, t, wsp + 64 * b);
        }
        __syncthreads();
        if (b < g.blocks) {
            uint32_t lo, hi;
            jpeg_idct_row(wsp + 64 * b, t, lo, hi);
            // inside the plane by construction: y0 + 8 <= rows, x0 + 8 <= stride (block_place), planes 16-byte aligned, x0 % 8 == 0
            *reinterpret_cast<uint2*>(planes + g.plane[comp] + (long long)(y0 + t) * g.stride[comp] + x0) = make_uint2(lo, hi);
        }
    }
    int st = r.status | (dead ? 0 : jpeg_segment_tail(r));
    if (k > 0 && sg[3] != ((k - 1) & 7)) st |= JPEG_ST_RST;
    if (im[0] & 2) st |= JPEG_ST_RST;
    if (lane == 0 && st) atomicOr(a.status + i, st);
}

__global__ __launch_bounds__(256) void jpeg_pixel_kernel(JpegArgs a) {
    const int H = a.H, W = a.W, G4 = (W + 3) >> 2;
    const long long units = (long long)a.n * H * G4;
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256) {
        const long long row = u / G4;
        const int x0 = (int)(u - row * G4) * 4;
        const int i = (int)(row / H), y = (int)(row - (long long)i * H);
        const int* img = a.img + (long long)JPEG_IMG_COLS * i;
        const int cnt = min(4, W - x0);
        uint32_t px[4] = {0u, 0u, 0u, 0u};
        if (img[0] & 1) {
            int im[4] = {img[0], img[1] == 1 ? 1 : 3, 1, 1};
            if (im[1] == 3) { im[2] = clampi(img[2], 1, 2); im[3] = clampi(img[3], 1, 2); }
            const JpegGeom g = jpeg_geom(im, H, W);
            const uint8_t* planes = a.ws + a.slot_bytes * i;
            for (int j = 0; j < cnt; ++j) {
                const uint32_t p = jpeg_pixel(planes, g, y, x0 + j);
                px[j] = a.order ? p : ((p & 0xFF00u) | (p >> 16) | ((p & 0xFFu) << 16));        // order 0: b | g << 8 | r << 16
            }
        }
        uint8_t* o = a.dst + (((long long)a.slot[i] * H + y) * W + x0) * 3;
        if (cnt == 4 && ((uintptr_t)o & 3) == 0) {
            uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
            o4[0] = px[0] | (px[1] << 24);
            o4[1] = (px[1] >> 8) | (px[2] << 16);
            o4[2] = (px[2] >> 16) | (px[3] << 8);
        } else {
            for (int j = 0; j < cnt; ++j) {
                o[3 * j] = (uint8_t)px[j]; o[3 * j + 1] = (uint8_t)(px[j] >> 8); o[3 * j + 2] = (uint8_t)(px[j] >> 16);
            }
        }
    }
}

}  // namespace

extern "C" size_t m3t_jpeg_workspace_bytes(int n, int H, int W) {
    if (n <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)n * (size_t)jpeg_slot_bytes(H, W);
}

extern "C" int m3t_jpeg_decode(const uint8_t* stream_d, long long stream_bytes, const int* tables_h, const int* tables_d, int n, int n_segs,
                               int n_quant, int n_huff, int H, int W, uint8_t* dst, long long dst_slots, int order, uint8_t* workspace,
                               long long workspace_bytes, int* status, void* stream) {
    if (n <= 0 || !tables_h || !tables_d || !dst || !workspace || !status || (order != 0 && order != 1)) return M3T_EINVAL;
    if ((n_segs > 0 && !stream_d) || ((uintptr_t)stream_d % 16) != 0 || (stream_bytes % 16) != 0 || ((uintptr_t)tables_d % 4) != 0 ||
        ((uintptr_t)workspace % 16) != 0 || ((uintptr_t)status % 4) != 0)
        return M3T_EINVAL;
    if (!jpeg_tables_ok(tables_h, n, n_segs, n_quant, n_huff, H, W, stream_bytes, dst_slots)) return M3T_EINVAL;
    if (workspace_bytes < (long long)m3t_jpeg_workspace_bytes(n, H, W)) return M3T_EINVAL;
    JpegArgs a;
    a.stream = stream_d;
    a.img = tables_d;
    a.seg = a.img + (long long)n * JPEG_IMG_COLS;
    a.slot = a.seg + (long long)n_segs * JPEG_SEG_COLS;
    a.quant = a.slot + n;
    a.huff = a.quant + (long long)n_quant * JPEG_QUANT_INTS;
    a.dst = dst; a.ws = workspace; a.status = status;
    a.stream_bytes = stream_bytes; a.slot_bytes = jpeg_slot_bytes(H, W);
    a.n = n; a.n_segs = n_segs; a.n_quant = n_quant; a.n_huff = n_huff; a.H = H; a.W = W; a.order = order;
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int) * (size_t)n, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (n_segs > 0) {
        jpeg_entropy_idct_kernel<<<(unsigned)n_segs, 64, 0, (hipStream_t)stream>>>(a);
        M3T_LAUNCH_CHECK();
    }
    const long long units = (long long)n * H * ((W + 3) / 4);
    const long long blocks = (units + 255) / 256;
    jpeg_pixel_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, (hipStream_t)stream>>>(a);
    M3T_LAUNCH_CHECK();
    return 0;
}
