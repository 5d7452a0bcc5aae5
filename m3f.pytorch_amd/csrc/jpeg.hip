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
// m3t_jpeg_decode_walk may route a segment to a second form of launch 1, jpeg_par_kernel: ONE WORKGROUP per segment, every lane walking
// a sub-sequence of it (self-synchronising Huffman decoding; the per-lane rules live in jpeg_par.h, shared with
// csrc/jpeg_par_host_check.cpp).  Its phases, a barrier between each and no word to another workgroup:
//   stage      the segment from HBM into LDS in 16-byte granules, unstuffed on the way (stuffed zeros counted per granule, prefix sum,
//              compaction): positions are plain bit offsets from here on and no reader looks for FF
//   speculate  lane i walks sub-sequence i leniently from (its first bit, block 0, k = 0); with more sub-sequences than lanes a lane
//              takes several
//   exchange   until no exit state changes, at most `sub-sequences` passes: a sub-sequence whose left neighbour's exit state is not the
//              state it last started from is walked again from it
//   index      prefix sum of the blocks begun per sub-sequence; one strict walk per sub-sequence records every block's first bit and DC
//              difference and finds the first error (the lowest sub-sequence wins; the last one carries on over the zero bits past the
//              end until the segment's blocks are done, at most blocks x 64 symbols)
//   DC         per-component prefix sum of the differences (wraps at 16 bits like the sequential predictor, so the sums are exact)
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
    int cap_u, cap_g, cap_nb, cap_sub;
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
    if (jpeg_par_takes(a.walk, sg[2], Ri * g.blocks, a.par_min, a.par_max)) return;      // jpeg_par_kernel's
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

// ---- the parallel walk --------------------------------------------------------------------------------------------------------------
// exclusive prefix sum of one int per lane over the workgroup (every lane calls it; scr: blockDim.x ints)
__device__ __forceinline__ int wg_excl_scan(int v, int* scr) {
    const int t = threadIdx.x, T = blockDim.x;
    __syncthreads();
    scr[t] = v;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {
        const int x = t >= d ? scr[t - d] : 0;
        __syncthreads();
        scr[t] += x;
        __syncthreads();
    }
    return scr[t] - v;
}

// dynamic LDS of jpeg_par_kernel, in bytes from its base (all multiples of 16):
//   tables 9 600 | scan scratch 1 024 | unstuffed image cap_u | block first bits 4 cap_nb | block DC 2 cap_nb | one of
//   { stuffed zeros in front of each granule 2 cap_g } { exchange states 15 cap_sub } { coefficients 132 T, IDCT workspace 32 T }
#define JPEG_PAR_LDS_FIXED (4 * (6 * JPEG_HUFF_INTS + 3 * JPEG_QUANT_INTS) + 1024)
static size_t jpeg_par_lds_bytes(int cap_u, int cap_g, int cap_nb, int cap_sub, int T) {
    size_t u = (size_t)2 * cap_g;
    if ((size_t)15 * cap_sub > u) u = (size_t)15 * cap_sub;
    if ((size_t)164 * T > u) u = (size_t)164 * T;
    return JPEG_PAR_LDS_FIXED + (size_t)cap_u + (size_t)6 * cap_nb + ((u + 15) & ~(size_t)15);
}

__global__ __launch_bounds__(256) void jpeg_par_kernel(JpegArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int sh_marker, sh_ulen, sh_any, sh_errsub, sh_errblock, sh_errst;
    __shared__ uint32_t sh_errbit, sh_done;
    __shared__ uint8_t zz[64];
    const int t = threadIdx.x, T = blockDim.x;
    const int* sg = a.seg + (long long)JPEG_SEG_COLS * blockIdx.x;
    const int i = sg[0];
    if (i < 0 || i >= a.n) return;                           // (uniform, like everything that returns below: no lane is left at a barrier)
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
    const int m0 = k * Ri, m1 = min(m0 + Ri, total), nblk = (m1 - m0) * g.blocks;
    if (!jpeg_par_takes(a.walk, sg[2], Ri * g.blocks, a.par_min, a.par_max)) return;     // jpeg_entropy_idct_kernel's
    const long long off = min(max((long long)sg[1], 0ll), a.stream_bytes);
    const long long end = min(off + max(sg[2], 0), a.stream_bytes);
    const long long base = off & ~15ll;
    const int lo = (int)(off - base), hi = (int)(end - base), G = (hi + 15) >> 4;
    // the host sized the arrays for the largest segment it routed here; a segment that would not fit was not validated by it
    if (G > a.cap_g || hi - lo + 16 > a.cap_u || nblk > a.cap_nb || nblk < 1 || T > 256 || (T & 63)) return;

    int* huff = reinterpret_cast<int*>(lds);
    int* quant = huff + 6 * JPEG_HUFF_INTS;
    int* scr = quant + 3 * JPEG_QUANT_INTS;
    uint8_t* ub = lds + JPEG_PAR_LDS_FIXED;
    uint32_t* bstart = reinterpret_cast<uint32_t*>(ub + a.cap_u);
    int16_t* bdc = reinterpret_cast<int16_t*>(bstart + a.cap_nb);
    unsigned char* uni = reinterpret_cast<unsigned char*>(bdc + a.cap_nb);
    uint16_t* pre = reinterpret_cast<uint16_t*>(uni);                                    // stage
    uint32_t* ex_p = reinterpret_cast<uint32_t*>(uni);                                   // exchange, index
    uint32_t* us_p = ex_p + a.cap_sub;
    uint16_t* ex_bk = reinterpret_cast<uint16_t*>(us_p + a.cap_sub);
    uint16_t* us_bk = ex_bk + a.cap_sub;
    uint16_t* nbs = us_bk + a.cap_sub;
    uint8_t* chg = reinterpret_cast<uint8_t*>(nbs + a.cap_sub);
    int16_t* coef = reinterpret_cast<int16_t*>(uni);                                     // decode
    int32_t* wsp = reinterpret_cast<int32_t*>(coef + T * JPEG_PAR_COEF_STRIDE);

    if (t < 64) zz[t] = k_zigzag[t];
    if (t == 0) {
        sh_marker = JPEG_PAR_NO_MARKER; sh_ulen = 0; sh_errsub = JPEG_PAR_NO_MARKER; sh_errblock = nblk; sh_errst = 0; sh_errbit = 0u; sh_done = 0u;
    }
    for (int c = 0; c < 3; ++c) {
        const int cc = c < g.ncomp ? c : 0;                  // (gray: the unused tables are copies, every read stays inside initialised LDS)
        const int* hd = a.huff + (long long)JPEG_HUFF_INTS * clampi(im[10 + cc], 0, a.n_huff - 1);
        const int* ha = a.huff + (long long)JPEG_HUFF_INTS * clampi(im[13 + cc], 0, a.n_huff - 1);
        for (int j = t; j < JPEG_HUFF_INTS; j += T) {
            huff[(2 * c) * JPEG_HUFF_INTS + j] = hd[j];
            huff[(2 * c + 1) * JPEG_HUFF_INTS + j] = ha[j];
        }
        if (t < JPEG_QUANT_INTS) quant[c * JPEG_QUANT_INTS + t] = a.quant[(long long)JPEG_QUANT_INTS * clampi(im[7 + cc], 0, a.n_quant - 1) + t];
    }
    __syncthreads();

    // ---- stage ----
    const uint8_t* src = a.stream + base;                    // granule gi is src[16 gi, 16 gi + 16): inside the stream, whose size is a multiple of 16
    {
        int mk = JPEG_PAR_NO_MARKER;
        for (int gi = t; gi < G; gi += T) {
            const uint4 q = *reinterpret_cast<const uint4*>(src + 16 * gi);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            const int prev = gi > 0 ? (int)src[16 * gi - 1] : 0;
            const int next = 16 * gi + 16 < hi ? (int)src[16 * gi + 16] : -1;
            pre[gi] = (uint16_t)jpeg_par_granule_count(w, prev, next, 16 * gi, lo, hi, mk);
        }
        if (mk != JPEG_PAR_NO_MARKER) atomicMin(&sh_marker, mk);
    }
    __syncthreads();
    const int marker = sh_marker, uend = min(marker, hi);
    {
        const int C = (G + T - 1) / T, g0 = min(t * C, G), g1 = min(g0 + C, G);
        int run = 0;
        for (int gi = g0; gi < g1; ++gi) { const int c = pre[gi]; pre[gi] = (uint16_t)run; run += c; }
        const int before = wg_excl_scan(run, scr);
        for (int gi = g0; gi < g1; ++gi) pre[gi] = (uint16_t)(pre[gi] + before);
    }
    __syncthreads();
    {
        int top = 0;
        for (int gi = t; gi < G; gi += T) {
            const uint4 q = *reinterpret_cast<const uint4*>(src + 16 * gi);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
            const int prev = gi > 0 ? (int)src[16 * gi - 1] : 0;
            top = max(top, jpeg_par_granule_write(w, prev, 16 * gi, lo, uend, pre[gi], ub, a.cap_u));
        }
        if (top > 0) atomicMax(&sh_ulen, top);
    }
    __syncthreads();
    const int ulen = sh_ulen, nw = jpeg_par_words(ulen);
    for (int j = ulen + t; j < 4 * nw && j < a.cap_u; j += T) ub[j] = 0;
    const int n_sub = jpeg_par_subs(ulen, a.sub_bytes);
    if (n_sub > a.cap_sub || 4 * nw > a.cap_u) return;
    __syncthreads();

    JpegParCtx c;
    c.ubw = reinterpret_cast<const uint32_t*>(ub); c.nw = nw; c.ubits = 8u * (uint32_t)ulen; c.huff = huff;
    c.ncomp = g.ncomp; c.ny = g.hs * g.vs; c.blocks = g.blocks;
    const uint32_t sub_bits = 8u * (uint32_t)a.sub_bytes;
    const int walk_iters = 8 * a.sub_bytes + 1;

    // ---- speculate ----
    for (int s = t; s < n_sub; s += T) {
        JpegParState st = {(uint32_t)s * sub_bits, 0, 0};
        us_p[s] = st.p; us_bk[s] = 0;
        nbs[s] = (uint16_t)jpeg_par_walk(c, st, min((uint32_t)(s + 1) * sub_bits, c.ubits), false, walk_iters);
        ex_p[s] = st.p; ex_bk[s] = (uint16_t)((st.b << 8) | st.k);
    }
    __syncthreads();
    // ---- exchange: at most n_sub passes (pass r makes the exit state of sub-sequence r true at the latest) ----
    int passes = 0;
    while (passes < n_sub) {
        ++passes;
        if (t == 0) sh_any = 0;
        for (int s = t; s < n_sub; s += T) {
            uint8_t ch = 0;
            if (s > 0) {
                const uint32_t p = ex_p[s - 1];
                const uint16_t bk = ex_bk[s - 1];
                if (p != us_p[s] || bk != us_bk[s]) { us_p[s] = p; us_bk[s] = bk; ch = 1; }
            }
            chg[s] = ch;
        }
        __syncthreads();
        bool mine = false;
        for (int s = t; s < n_sub; s += T) {
            if (!chg[s]) continue;
            const int bk = us_bk[s];
            JpegParState st = {us_p[s], bk >> 8, bk & 255};
            nbs[s] = (uint16_t)jpeg_par_walk(c, st, min((uint32_t)(s + 1) * sub_bits, c.ubits), false, walk_iters);
            const uint16_t nbk = (uint16_t)((st.b << 8) | st.k);
            mine |= st.p != ex_p[s] || nbk != ex_bk[s];
            ex_p[s] = st.p; ex_bk[s] = nbk;
        }
        if (mine) sh_any = 1;
        __syncthreads();
        const int any = sh_any;
        __syncthreads();
        if (!any) break;
    }
    // ---- index ----
    {
        const int C = (n_sub + T - 1) / T, s0 = min(t * C, n_sub), s1 = min(s0 + C, n_sub);
        int run = 0;
        for (int s = s0; s < s1; ++s) run += nbs[s];
        int first = wg_excl_scan(run, scr);
        for (int s = s0; s < s1; ++s) { us_p[s] = (uint32_t)first; first += nbs[s]; }         // us_p: now the first block of the sub-sequence
    }
    __syncthreads();
    {
        int e_sub = JPEG_PAR_NO_MARKER, e_block = 0, e_st = 0, e_diff = 0;
        uint32_t e_bit = 0u, e_start = 0u;
        for (int s = t; s < n_sub && e_sub == JPEG_PAR_NO_MARKER; s += T) {
            JpegParState st = {0u, 0, 0};
            if (s > 0) { const int bk = ex_bk[s - 1]; st.p = ex_p[s - 1]; st.b = bk >> 8; st.k = bk & 255; }
            int j = (int)min(us_p[s], (uint32_t)nblk);
            if (st.k) jpeg_par_walk(c, st, 0u, true, JPEG_PAR_FINISH_ITERS);
            if (st.k) continue;
            const bool last = s == n_sub - 1;
            const uint32_t e = min((uint32_t)(s + 1) * sub_bits, c.ubits);
            while (j < nblk && (last || st.p < e)) {             // at most nblk blocks of at most 64 symbols
                const uint32_t p0 = st.p;
                int diff;
                const int rc = jpeg_par_block(c, st.p, jpeg_par_comp(c, j % g.blocks), zz, nullptr, 0, diff);
                if (rc) { e_sub = s; e_block = j; e_st = rc; e_bit = st.p; e_start = p0; e_diff = diff; break; }
                bstart[j] = p0;
                bdc[j] = (int16_t)diff;
                if (++j == nblk) sh_done = st.p;
            }
        }
        if (e_sub != JPEG_PAR_NO_MARKER) atomicMin(&sh_errsub, e_sub);
        __syncthreads();
        // the lowest sub-sequence that raised a status holds the first error of the segment: everything behind it walked from states
        // that mean nothing, and what those lanes recorded (possibly for this very block) is overwritten or never read
        if (e_sub != JPEG_PAR_NO_MARKER && e_sub == sh_errsub) {
            sh_errblock = e_block; sh_errst = e_st; sh_errbit = e_bit;
            bstart[e_block] = e_start; bdc[e_block] = (int16_t)e_diff;
        }
    }
    __syncthreads();
    const int errblock = sh_errblock;
    // ---- DC: inclusive per-component sums in place ----
    {
        const int C = (nblk + T - 1) / T, j0 = min(t * C, nblk), j1 = min(j0 + C, nblk);
        int s0 = 0, s1 = 0, s2 = 0;
        for (int j = j0; j < j1; ++j) {
            const int comp = jpeg_par_comp(c, j % g.blocks), d = bdc[j];
            s0 += comp == 0 ? d : 0; s1 += comp == 1 ? d : 0; s2 += comp == 2 ? d : 0;
        }
        s0 = wg_excl_scan(s0, scr); s1 = wg_excl_scan(s1, scr); s2 = wg_excl_scan(s2, scr);
        for (int j = j0; j < j1; ++j) {
            const int comp = jpeg_par_comp(c, j % g.blocks), d = bdc[j];
            s0 += comp == 0 ? d : 0; s1 += comp == 1 ? d : 0; s2 += comp == 2 ? d : 0;
            bdc[j] = (int16_t)(comp == 0 ? s0 : (comp == 1 ? s1 : s2));
        }
    }
    __syncthreads();                                         // (the exchange arrays are dead from here: the coefficients take their place)
    // ---- decode and transform ----
    const uint16_t* q16 = reinterpret_cast<const uint16_t*>(quant);
    uint8_t* planes = a.ws + a.slot_bytes * i;
    int32_t* coef32 = reinterpret_cast<int32_t*>(coef);
    const int per = T >> 3;                                  // blocks of one transform step: eight lanes a block
    for (int r0 = 0; r0 < nblk; r0 += T) {
        for (int x = t; x < T * (JPEG_PAR_COEF_STRIDE / 2); x += T) coef32[x] = 0;
        __syncthreads();
        {
            const int j = r0 + t;
            if (j < nblk && j <= errblock) {
                uint32_t p = bstart[j];
                int diff;
                jpeg_par_block(c, p, jpeg_par_comp(c, j % g.blocks), zz, coef + t * JPEG_PAR_COEF_STRIDE, bdc[j], diff);
            }
        }
        __syncthreads();
        for (int q0 = 0; q0 < T && r0 + q0 < nblk; q0 += per) {
            const int lb = q0 + (t >> 3), j = r0 + lb, x = t & 7;
            int comp = 0, y0 = 0, x0 = 0;
            if (j < nblk) {
                jpeg_block_place(g, m0 + j / g.blocks, j % g.blocks, comp, y0, x0);
                jpeg_idct_col(coef + lb * JPEG_PAR_COEF_STRIDE, q16 + 64 * comp, x, wsp + (t >> 3) * 64);
            }
            __syncthreads();
            if (j < nblk) {
                uint32_t w0, w1;
                jpeg_idct_row(wsp + (t >> 3) * 64, x, w0, w1);
                // inside the plane as in jpeg_entropy_idct_kernel: the MCU is one of this segment's, y0 + 8 <= rows, x0 + 8 <= stride
                *reinterpret_cast<uint2*>(planes + g.plane[comp] + (long long)(y0 + x) * g.stride[comp] + x0) = make_uint2(w0, w1);
            }
            __syncthreads();
        }
    }
    // ---- status and stats ----
    if (t == 0) {
        int st;
        if (marker < hi) {
            // the sequential reader's walk for the status alone, straight from the stream (a damaged segment; nothing is stored)
            JpegReader r;
            jpeg_reader_init(r, a.stream, 0, (int)min(a.stream_bytes, 0x7fffffffll), (int)off, (int)end);
            int pred[3] = {0, 0, 0};
            bool dead = false;
            for (int j = 0; j < nblk && !dead; ++j) {
                const int comp = jpeg_par_comp(c, j % g.blocks);
                const JpegHuff hd = jpeg_huff_at(huff + (2 * comp) * JPEG_HUFF_INTS), ha = jpeg_huff_at(huff + (2 * comp + 1) * JPEG_HUFF_INTS);
                const int rc = jpeg_decode_block(r, hd, ha, zz, pred[comp], nullptr, false);
                if (rc) { r.status |= rc; dead = true; }
            }
            st = r.status | (dead ? 0 : jpeg_segment_tail(r));
        } else {
            st = jpeg_par_tail(errblock < nblk ? sh_errbit : sh_done, c.ubits, sh_errst);
        }
        if (k > 0 && sg[3] != ((k - 1) & 7)) st |= JPEG_ST_RST;
        if (im[0] & 2) st |= JPEG_ST_RST;
        if (st) atomicOr(a.status + i, st);
        if (a.walk_stats) { a.walk_stats[2 * blockIdx.x] = n_sub; a.walk_stats[2 * blockIdx.x + 1] = passes; }
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
    a.cap_u = a.cap_g = a.cap_nb = a.cap_sub = 0;
    a.walk_stats = walk_stats;
    // the routing rule over the validated host tables: how many segments the parallel walk takes and what the largest of them needs
    int taken = 0;
    if (walk == 1) {
        const int* seg = tables_h + (long long)n * JPEG_IMG_COLS;
        for (int s = 0; s < n_segs; ++s, seg += JPEG_SEG_COLS) {
            const int* im = tables_h + (long long)seg[0] * JPEG_IMG_COLS;
            const JpegGeom g = jpeg_geom(im, H, W);
            const int nb = im[4] * g.blocks;
            if (!jpeg_par_takes(walk, seg[2], nb, a.par_min, a.par_max)) continue;
            ++taken;
            const int hi = (seg[1] & 15) + seg[2];
            a.cap_u = max(a.cap_u, ((seg[2] + 15) & ~15) + 32);
            a.cap_g = max(a.cap_g, (hi + 15) / 16);
            a.cap_nb = max(a.cap_nb, nb);
            a.cap_sub = max(a.cap_sub, jpeg_par_subs(seg[2], sub_bytes));
        }
        a.cap_g = (a.cap_g + 7) & ~7; a.cap_nb = (a.cap_nb + 7) & ~7; a.cap_sub = (a.cap_sub + 15) & ~15;
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
        const size_t lds = jpeg_par_lds_bytes(a.cap_u, a.cap_g, a.cap_nb, a.cap_sub, T);
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
