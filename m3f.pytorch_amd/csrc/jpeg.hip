// Batched baseline-JPEG decode on the GPU: the first line of the reference's load_video (models/dataset.py:64, cv2.imread of one JPEG per
// frame) for a whole batch, from the packed streams m3t.jpeg.pack builds to the uint8 [N][Ts][H][W][3] buffer every later stage takes.
// The sequential rules live in jpeg_core.h (shared with the host check program, csrc/jpeg_host_check.cpp, as is what resolves a segment
// from the tables and what its status is); this file is their schedule, two launches:
//   1. jpeg_entropy_idct_kernel: one wave per entropy-coded segment (a restart interval, or the whole scan).  The stream comes through
//      LDS in 1 KiB windows read as 16-byte granules, the image's Huffman and quantisation tables sit in LDS beside it.  The symbol walk is
//      sequential: every lane runs it on the same (uniform) state and lane 0 stores the coefficients; after each MCU the lanes take one
//      column, then one row, of its blocks through the integer IDCT and store eight samples each into the block-padded component planes
//      of the image's workspace slot.  An MCU belongs to exactly one segment, so no plane byte has two writers.
//   2. jpeg_pixel_kernel: four pixels a lane -- fancy chroma upsampling from the planes, colour, the caller's channel order -- as three
//      dwords where the destination allows, bytes otherwise.
// m3t_jpeg_decode_walk may route a segment to a second form of launch 1, jpeg_par_kernel: ONE WORKGROUP per segment, every lane walking
// a sub-sequence of it (self-synchronising Huffman decoding).  The per-lane rules, the workgroup's memory and every phase live in
// jpeg_par.h, shared with the host check program, which calls the same phases lane by lane; the kernel here is the list of them.
// Its phases, a barrier between each (several inside most of them) and no word to another workgroup:
//   stage      the segment from HBM into LDS in 16-byte granules, unstuffed on the way (stuffed zeros counted per granule, prefix sum,
//              compaction): positions are plain bit offsets from here on and no reader looks for FF
//   speculate  lane i walks sub-sequence i leniently from (its first bit, block 0, k = 0); with more sub-sequences than lanes a lane
//              takes several
//   exchange   until no exit state changes, at most `sub-sequences` passes: a sub-sequence whose left neighbour's exit state is not the
//              state it last started from is walked again from it
//   index      prefix sum of the blocks begun per sub-sequence; one strict walk per sub-sequence records every block's first bit and DC
//              difference and finds the first error (the lowest sub-sequence wins, and its lane walks it once more to write the error
//              down; the last one carries on over the zero bits past the end until the segment's blocks are done, at most blocks x 64
//              symbols)
//   DC         prefix sum of the differences, a component at a time (wraps at 16 bits like the sequential predictor, so the sums are exact)
//   decode     one lane a block from its first bit into LDS coefficients (blocks after the error stay zero), then eight lanes a block
//              through the same IDCT into the same planes
// The frames are those of the sequential walk for every input, and so is the status: a segment without a marker inside gets it from
// the bit position the walk ended at (jpeg_par_tail), a segment WITH one (damage) has lane 0 repeat the sequential reader's walk for
// the status alone, because what that reader says of a marker depends on how far its look-ahead got.
#include "common.h"
#include "jpeg_core.h"
#include "jpeg_par.h"

namespace {

__constant__ uint8_t k_zigzag[64] = JPEG_ZIGZAG_INIT;

struct JpegArgs {
    const uint8_t* stream; const int* img; const int* seg; const int* slot; const int* quant; const int* huff;
    uint8_t* dst; uint8_t* ws; int* status;
    long long stream_bytes, slot_bytes;
    int n, n_segs, n_quant, n_huff, H, W, order;
    // m3t_jpeg_decode_walk: the routing rule and, for jpeg_par_kernel, the room its arrays have in LDS (the largest taken segment's needs)
    int walk, sub_bytes, par_min, par_max;
    JpegParCaps cap;
    int* walk_stats;
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
    const JpegSegment S = jpeg_segment_resolve(a.img, a.seg, (int)blockIdx.x, a.n, a.H, a.W, a.stream_bytes);
    if (!S.live) return;                                     // (uniform)
    if (jpeg_par_takes(a.walk, S.bytes, S.Ri * S.g.blocks, a.par_min, a.par_max)) return;      // jpeg_par_kernel's
    const JpegGeom g = S.g;                                  // (a copy: the loop below indexes its arrays by the component)

    zz[lane] = k_zigzag[lane];
    jpeg_tables_load(huff, quant, S, g.ncomp, a.huff, a.n_huff, a.quant, a.n_quant, lane, 64);
    int16_t* coef = reinterpret_cast<int16_t*>(coef32);
    const uint16_t* q16 = reinterpret_cast<const uint16_t*>(quant);
    uint8_t* planes = a.ws + a.slot_bytes * S.i;

    JpegReader r;
    jpeg_reader_init(r, reinterpret_cast<const uint8_t*>(win4), (int)S.off, 0, (int)S.off, (int)S.end);
    int pred[3] = {0, 0, 0};
    bool dead = false;
    for (int m = S.m0; m < S.m1; ++m) {
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
    const int st = r.status | (dead ? 0 : jpeg_segment_tail(r)) | jpeg_segment_rst(S);
    if (lane == 0 && st) atomicOr(a.status + S.i, st);
}

// ---- the parallel walk --------------------------------------------------------------------------------------------------------------
// scr[lane] -> the inclusive sums over the workgroup's lanes (every lane calls it, behind the phase that wrote scr)
__device__ __forceinline__ void wg_scan(int* scr) {
    const int t = threadIdx.x, T = blockDim.x;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {
        const int x = t >= d ? scr[t - d] : 0;
        __syncthreads();
        scr[t] += x;
        __syncthreads();
    }
}

// The phases are jpeg_par.h's; here are the barriers between them.  Every return is uniform: no lane is left at a barrier.
__global__ __launch_bounds__(256) void jpeg_par_kernel(JpegArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ JpegParWords words;
    __shared__ uint8_t zz[64];
    const int t = threadIdx.x, T = blockDim.x;
    const JpegSegment S = jpeg_segment_resolve(a.img, a.seg, (int)blockIdx.x, a.n, a.H, a.W, a.stream_bytes);
    if (!S.live) return;
    if (!jpeg_par_takes(a.walk, S.bytes, S.Ri * S.g.blocks, a.par_min, a.par_max)) return;     // jpeg_entropy_idct_kernel's
    JpegParMem m;
    jpeg_par_carve<true>(m, lds, a.cap, T);
    m.w = &words; m.zz = zz;
    if (!jpeg_par_segment(m, S, a.stream, a.ws, a.slot_bytes, a.sub_bytes, a.cap) || T > JPEG_PAR_SCAN_INTS || (T & 63)) return;

    if (t < 64) zz[t] = k_zigzag[t];
    jpeg_tables_load(m.huff, m.quant, S, 3, a.huff, a.n_huff, a.quant, a.n_quant, t, T);
    jpeg_par_begin(m, t, T);
    __syncthreads();
    // ---- stage ----
    jpeg_par_stage_count(m, t, T);
    __syncthreads();
    jpeg_par_stage_sum(m, t, T);
    wg_scan(m.scr);
    jpeg_par_stage_add(m, t, T);
    __syncthreads();
    jpeg_par_stage_write(m, t, T);
    __syncthreads();
    const bool fits = jpeg_par_staged(m);
    jpeg_par_stage_fill(m, t, T);
    if (!fits) return;
    __syncthreads();
    // ---- speculate, exchange ----
    jpeg_par_speculate(m, t, T);
    __syncthreads();
    int passes = 0;
    while (passes < m.n_sub) {
        ++passes;
        jpeg_par_exchange_take(m, t, T);
        __syncthreads();
        jpeg_par_exchange_walk(m, t, T);
        __syncthreads();
        const int any = words.any;
        __syncthreads();
        if (!any) break;
    }
    // ---- index ----
    jpeg_par_index_sum(m, t, T);
    wg_scan(m.scr);
    jpeg_par_index_first(m, t, T);
    __syncthreads();
    jpeg_par_index_walk(m, t, T);
    __syncthreads();
    jpeg_par_index_error(m, t, T);
    __syncthreads();
    // ---- DC ----
    for (int comp = 0; comp < S.g.ncomp; ++comp) {
        jpeg_par_dc_sum(m, t, T, comp);
        wg_scan(m.scr);
        jpeg_par_dc_add(m, t, T, comp);
        __syncthreads();                                     // (after the last: the exchange arrays are dead, the coefficients take their place)
    }
    // ---- decode and transform ----
    for (int r0 = 0; r0 < m.nblk; r0 += T) {
        jpeg_par_decode_zero(m, t, T);
        __syncthreads();
        jpeg_par_decode_block(m, t, T, r0);
        __syncthreads();
        for (int q0 = 0; q0 < T && r0 + q0 < m.nblk; q0 += T >> 3) {
            jpeg_par_idct_col(m, t, T, r0, q0);
            __syncthreads();
            jpeg_par_idct_row(m, t, T, r0, q0);
            __syncthreads();
        }
    }
    // ---- status and stats ----
    if (t == 0) {
        const int st = jpeg_par_status(m, a.stream, a.stream_bytes);
        if (st) atomicOr(a.status + S.i, st);
        if (a.walk_stats) { a.walk_stats[2 * blockIdx.x] = m.n_sub; a.walk_stats[2 * blockIdx.x + 1] = passes; }
    }
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

static int g_par_lanes = 256;

extern "C" int m3t_jpeg_par_max_bytes(void) { return JPEG_PAR_MAX_BYTES; }

extern "C" int m3t_jpeg_par_lanes(int lanes) {
    if (lanes == 0) return g_par_lanes;
    if (lanes != 64 && lanes != 128 && lanes != 256) return -M3T_EINVAL;
    g_par_lanes = lanes;
    return lanes;
}

static int jpeg_decode_impl(const uint8_t* stream_d, long long stream_bytes, const int* tables_h, const int* tables_d, int n, int n_segs,
                            int n_quant, int n_huff, int H, int W, uint8_t* dst, long long dst_slots, int order, uint8_t* workspace,
                            long long workspace_bytes, int* status, int walk, int sub_bytes, int par_min_bytes, int par_max_bytes,
                            int* walk_stats, void* stream) {
    if (n <= 0 || !tables_h || !tables_d || !dst || !workspace || !status || (order != 0 && order != 1)) return M3T_EINVAL;
    if ((n_segs > 0 && !stream_d) || ((uintptr_t)stream_d % 16) != 0 || (stream_bytes % 16) != 0 || ((uintptr_t)tables_d % 4) != 0 ||
        ((uintptr_t)workspace % 16) != 0 || ((uintptr_t)status % 4) != 0)
        return M3T_EINVAL;
    if ((walk != 0 && walk != 1) || sub_bytes < JPEG_PAR_SUB_MIN || sub_bytes > JPEG_PAR_SUB_MAX || (sub_bytes % 16) != 0 || par_min_bytes < 0 ||
        par_max_bytes < 0 || ((uintptr_t)walk_stats % 4) != 0)
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
    a.walk = walk; a.sub_bytes = sub_bytes; a.par_min = par_min_bytes; a.par_max = par_max_bytes < JPEG_PAR_MAX_BYTES ? par_max_bytes : JPEG_PAR_MAX_BYTES;
    a.cap = JpegParCaps{0, 0, 0, 0};
    a.walk_stats = walk_stats;
    // the routing rule over the validated host tables: how many segments the parallel walk takes and what the largest of them needs
    int taken = 0;
    if (walk == 1) {
        for (int s = 0; s < n_segs; ++s) {
            const JpegSegment S = jpeg_segment_resolve(tables_h, tables_h + (long long)n * JPEG_IMG_COLS, s, n, H, W, stream_bytes);
            if (!S.live || !jpeg_par_takes(walk, S.bytes, S.Ri * S.g.blocks, a.par_min, a.par_max)) continue;
            ++taken;
            jpeg_par_caps_add(a.cap, (int)S.off, S.bytes, S.Ri * S.g.blocks, sub_bytes);
        }
        jpeg_par_caps_round(a.cap);
    }
    hipError_t e = hipMemsetAsync(status, 0, sizeof(int) * (size_t)n, (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (walk_stats && n_segs > 0) {
        e = hipMemsetAsync(walk_stats, 0, 2 * sizeof(int) * (size_t)n_segs, (hipStream_t)stream);
        if (e != hipSuccess) return (int)e;
    }
    if (n_segs > taken) {
        jpeg_entropy_idct_kernel<<<(unsigned)n_segs, 64, 0, (hipStream_t)stream>>>(a);
        M3T_LAUNCH_CHECK();
    }
    if (taken > 0) {
        const int T = g_par_lanes;
        JpegParMem unplaced;
        const size_t lds = jpeg_par_carve<false>(unplaced, nullptr, a.cap, T);
        if (lds > (size_t)160 * 1024) return M3T_EINVAL;                     // (not reached: the build's caps keep it under 132 KiB)
        e = hipFuncSetAttribute(reinterpret_cast<const void*>(jpeg_par_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
        jpeg_par_kernel<<<(unsigned)n_segs, T, lds, (hipStream_t)stream>>>(a);
        M3T_LAUNCH_CHECK();
    }
    const long long units = (long long)n * H * ((W + 3) / 4);
    const long long blocks = (units + 255) / 256;
    jpeg_pixel_kernel<<<(unsigned)(blocks < 65536 ? blocks : 65536), 256, 0, (hipStream_t)stream>>>(a);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_jpeg_decode(const uint8_t* stream_d, long long stream_bytes, const int* tables_h, const int* tables_d, int n, int n_segs,
                               int n_quant, int n_huff, int H, int W, uint8_t* dst, long long dst_slots, int order, uint8_t* workspace,
                               long long workspace_bytes, int* status, void* stream) {
    return jpeg_decode_impl(stream_d, stream_bytes, tables_h, tables_d, n, n_segs, n_quant, n_huff, H, W, dst, dst_slots, order, workspace,
                            workspace_bytes, status, 0, JPEG_PAR_SUB_MIN, 0, 0, nullptr, stream);
}

extern "C" int m3t_jpeg_decode_walk(const uint8_t* stream_d, long long stream_bytes, const int* tables_h, const int* tables_d, int n, int n_segs,
                                    int n_quant, int n_huff, int H, int W, uint8_t* dst, long long dst_slots, int order, uint8_t* workspace,
                                    long long workspace_bytes, int* status, int walk, int sub_bytes, int par_min_bytes, int par_max_bytes,
                                    int* walk_stats, void* stream) {
    return jpeg_decode_impl(stream_d, stream_bytes, tables_h, tables_d, n, n_segs, n_quant, n_huff, H, W, dst, dst_slots, order, workspace,
                            workspace_bytes, status, walk, sub_bytes, par_min_bytes, par_max_bytes, walk_stats, stream);
}
