// The device code of csrc/jpeg.hip on the host: this program includes jpeg_core.h and jpeg_par.h, reads one packed batch (the arguments of
// m3t_jpeg_decode as m3t.jpeg.pack builds them, the file tests/jpeg_cases.py::write_packed writes), decodes it as m3t_jpeg_decode_walk
// would -- per segment the parallel walk where the routing rule takes it, the sequential walk elsewhere -- and writes status and pixels to
// a second file.  Not only the per-lane rules are the kernels' text: what resolves a segment, what its status is, and for the parallel
// walk the workgroup's memory, its sizes, its packed states and every phase are.  The workgroup is emulated by calling each phase of
// jpeg_par.h for every lane index in turn where jpeg_par_kernel calls it once and waits at a barrier, so a pass of the exchange is Jacobi
// (every lane reads what the pass before left), like lanes in lockstep.  Built with -fsanitize=address,undefined it is the memory check
// of that text (as a plain executable); tests/test_jpeg_host.py and tests/test_jpeg_par_host.py compare its results with the goldens.
//   usage : jpeg_host_check packed.bin out.bin                                                   (the sequential walk: walk = 0)
//           jpeg_host_check packed.bin out.bin walk sub_bytes par_min_bytes par_max_bytes lanes
//   input : int32 header[12] = magic, n, n_segs, n_quant, n_huff, H, W, order, dst_slots, stream_bytes, 0, 0 | tables | stream bytes
//   output: int32 status[n] | uint8 dst[dst_slots][H][W][3] (every byte the decoder did not write still GUARD): what
//           tests/jpeg_cases.py::read_result reads; with the walk arguments, beside it out.bin.stats: int32 stats[n_segs][2] =
//           sub-sequences, exchange passes ((0, 0) for a segment the sequential walk took)
// The stream, the workspace, the destination and every array the emulated workgroup keeps are exact-size heap blocks of their own (also
// the arrays that share LDS on the device), the ones written to with guard bytes around them, checked before the program reports
// success; a block the device reuses is refilled with the guard byte where its first tenant dies, so that a late read of it shows.
// Exit 0: decoded (whatever the status words say); 2: refused (M3T_EINVAL's rule: the tables, walk, sub_bytes or the thresholds);
// 3: a guard byte changed; 1: usage or I/O.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "jpeg_par.h"

static const unsigned char GUARD = 0xA5;
static const int GUARD_BYTES = 64;
static const uint8_t kZigzag[64] = JPEG_ZIGZAG_INIT;
static int g_guard_bad = 0;

// a heap block of exactly n elements with guard bytes on both sides
template <class T> struct Guarded {
    unsigned char* raw; T* p; size_t bytes;
    explicit Guarded(size_t n) : bytes(n * sizeof(T)) {
        raw = (unsigned char*)malloc(bytes + 2 * GUARD_BYTES);
        memset(raw, GUARD, bytes + 2 * GUARD_BYTES);
        p = reinterpret_cast<T*>(raw + GUARD_BYTES);
    }
    void dies() { memset(raw + GUARD_BYTES, GUARD, bytes); }
    ~Guarded() {
        for (int j = 0; j < GUARD_BYTES; ++j) g_guard_bad |= raw[j] != GUARD || raw[GUARD_BYTES + bytes + j] != GUARD;
        free(raw);
    }
    Guarded(const Guarded&) = delete;
    Guarded& operator=(const Guarded&) = delete;
};

struct Batch {
    const uint8_t* stream; long long stream_bytes;
    const int* img; const int* seg; const int* quant; const int* huff; int n, n_quant, n_huff, H, W;
    uint8_t* ws; long long slot_bytes;
};

// one block through the IDCT by one lane; quant: as jpeg_tables_load leaves it
static void idct_store(const JpegSegment& S, uint8_t* planes, int m, int b, const int16_t* coef, const int* quant) {
    int comp, y0, x0;
    int32_t wsp[64];
    jpeg_block_place(S.g, m, b, comp, y0, x0);
    for (int x = 0; x < 8; ++x) jpeg_idct_col(coef, reinterpret_cast<const uint16_t*>(quant) + 64 * comp, x, wsp);
    for (int y = 0; y < 8; ++y) {
        uint32_t lo, hi;
        jpeg_idct_row(wsp, y, lo, hi);
        jpeg_store8(planes + jpeg_plane_offset(S.g, comp, y0 + y, x0), lo, hi);
    }
}

// the sequential walk (jpeg_entropy_idct_kernel)
static int seq_segment(const Batch& B, const JpegSegment& S) {
    Guarded<int> huff(6 * JPEG_HUFF_INTS), quant(3 * JPEG_QUANT_INTS);
    jpeg_tables_load(huff.p, quant.p, S, S.g.ncomp, B.huff, B.n_huff, B.quant, B.n_quant, 0, 1);
    JpegReader r;
    jpeg_reader_init(r, B.stream, 0, (int)B.stream_bytes, (int)S.off, (int)S.end);
    int pred[3] = {0, 0, 0};
    bool dead = false;
    for (int m = S.m0; m < S.m1; ++m) {
        int16_t coef[6 * 64];
        memset(coef, 0, sizeof(coef));
        if (!dead) dead = !jpeg_walk_mcu(r, S.g, m, huff.p, kZigzag, pred, coef, true);
        for (int b = 0; b < S.g.blocks; ++b) idct_store(S, B.ws + B.slot_bytes * S.i, m, b, coef + 64 * b, quant.p);
    }
    return r.status | (dead ? 0 : jpeg_segment_tail(r)) | jpeg_segment_rst(S);
}

#define PHASE(f, ...) for (int t = 0; t < T; ++t) f(m, t, T, ##__VA_ARGS__)
#define SCAN() for (int t = 1; t < T; ++t) m.scr[t] += m.scr[t - 1]

// the parallel walk (jpeg_par_kernel) with T emulated lanes; stats: sub-sequences, exchange passes
static int par_segment(const Batch& B, const JpegSegment& S, int sub_bytes, int T, int* stats) {
    JpegParCaps cap = {0, 0, 0, 0};
    jpeg_par_caps_add(cap, (int)S.off, S.bytes, S.Ri * S.g.blocks, sub_bytes);
    jpeg_par_caps_round(cap);
    Guarded<int> huff(6 * JPEG_HUFF_INTS), quant(3 * JPEG_QUANT_INTS), scr((size_t)T);
    Guarded<uint8_t> ub((size_t)cap.u), chg((size_t)cap.sub);
    Guarded<uint32_t> bstart((size_t)cap.nb), ex_p((size_t)cap.sub), us_p((size_t)cap.sub);
    Guarded<int16_t> bdc((size_t)cap.nb), coef((size_t)jpeg_par_coef_count(T));
    Guarded<uint16_t> pre((size_t)cap.g), ex_bk((size_t)cap.sub), us_bk((size_t)cap.sub), nbs((size_t)cap.sub);
    Guarded<int32_t> wsp((size_t)jpeg_par_wsp_count(T));
    JpegParWords words;
    JpegParMem m;
    m.huff = huff.p; m.quant = quant.p; m.scr = scr.p; m.ub = ub.p; m.bstart = bstart.p; m.bdc = bdc.p; m.pre = pre.p;
    m.ex_p = ex_p.p; m.us_p = us_p.p; m.ex_bk = ex_bk.p; m.us_bk = us_bk.p; m.nbs = nbs.p; m.chg = chg.p; m.coef = coef.p; m.wsp = wsp.p;
    m.w = &words; m.zz = kZigzag;
    if (!jpeg_par_segment(m, S, B.stream, B.ws, B.slot_bytes, sub_bytes, cap)) return 0;

    for (int t = 0; t < T; ++t) jpeg_tables_load(m.huff, m.quant, S, 3, B.huff, B.n_huff, B.quant, B.n_quant, t, T);
    PHASE(jpeg_par_begin);
    PHASE(jpeg_par_stage_count);
    PHASE(jpeg_par_stage_sum);
    SCAN();
    PHASE(jpeg_par_stage_add);
    PHASE(jpeg_par_stage_write);
    const bool fits = jpeg_par_staged(m);
    PHASE(jpeg_par_stage_fill);
    if (!fits) return 0;
    pre.dies();
    PHASE(jpeg_par_speculate);
    int passes = 0;
    while (passes < m.n_sub) {
        ++passes;
        PHASE(jpeg_par_exchange_take);
        PHASE(jpeg_par_exchange_walk);
        if (!words.any) break;
    }
    stats[0] = m.n_sub; stats[1] = passes;
    PHASE(jpeg_par_index_sum);
    SCAN();
    PHASE(jpeg_par_index_first);
    PHASE(jpeg_par_index_walk);
    PHASE(jpeg_par_index_error);
    for (int comp = 0; comp < S.g.ncomp; ++comp) {
        PHASE(jpeg_par_dc_sum, comp);
        SCAN();
        PHASE(jpeg_par_dc_add, comp);
    }
    ex_p.dies(); us_p.dies(); ex_bk.dies(); us_bk.dies(); nbs.dies(); chg.dies();
    for (int r0 = 0; r0 < m.nblk; r0 += T) {
        PHASE(jpeg_par_decode_zero);
        PHASE(jpeg_par_decode_block, r0);
        if (T & 7) {             // no kernel's lane count: its eight lanes a block are not emulated, one lane takes a block through the IDCT
            for (int j = r0; j < r0 + T && j < m.nblk; ++j)
                idct_store(S, m.planes, S.m0 + j / S.g.blocks, j % S.g.blocks, m.coef + (j - r0) * JPEG_PAR_COEF_STRIDE, m.quant);
            continue;
        }
        for (int q0 = 0; q0 < T && r0 + q0 < m.nblk; q0 += T >> 3) {
            PHASE(jpeg_par_idct_col, r0, q0);
            PHASE(jpeg_par_idct_row, r0, q0);
        }
    }
    return jpeg_par_status(m, B.stream, B.stream_bytes);
}

int main(int argc, char** argv) {
    if (argc != 3 && argc != 8) {
        fprintf(stderr, "usage: %s packed.bin out.bin [walk sub_bytes par_min_bytes par_max_bytes lanes]\n", argv[0]);
        return 1;
    }
    const bool par = argc == 8;
    const int walk = par ? atoi(argv[3]) : 0, sub_bytes = par ? atoi(argv[4]) : JPEG_PAR_SUB_MIN, par_min = par ? atoi(argv[5]) : 0;
    const int par_max = par ? atoi(argv[6]) : 0, lanes = par ? atoi(argv[7]) : 64;
    if ((walk != 0 && walk != 1) || sub_bytes < JPEG_PAR_SUB_MIN || sub_bytes > JPEG_PAR_SUB_MAX || sub_bytes % 16 != 0 || par_min < 0 || par_max < 0) {
        fprintf(stderr, "walk arguments refused\n");
        return 2;
    }
    if (lanes < 1 || lanes > 1024) { fprintf(stderr, "lanes must be in [1, 1024]\n"); return 1; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int hd[12];
    if (fread(hd, 4, 12, f) != 12 || hd[0] != 0x4A504731) { fprintf(stderr, "bad header\n"); return 1; }
    const int n = hd[1], n_segs = hd[2], n_quant = hd[3], n_huff = hd[4], H = hd[5], W = hd[6], order = hd[7];
    const long long dst_slots = hd[8], stream_bytes = hd[9];
    if (n <= 0 || n > (1 << 20) || n_segs < 0 || n_segs > (1 << 24) || n_quant < 0 || n_quant > 4096 || n_huff < 0 || n_huff > 4096 || stream_bytes < 0) {
        fprintf(stderr, "tables refused\n");
        return 2;
    }
    std::vector<int> t((size_t)jpeg_tables_ints(n, n_segs, n_quant, n_huff));
    if (fread(t.data(), 4, t.size(), f) != t.size()) { fprintf(stderr, "short tables\n"); return 1; }
    uint8_t* stream = (uint8_t*)malloc(stream_bytes ? (size_t)stream_bytes : 1);          // exact size: a read past it is the sanitizer's to see
    if (stream_bytes && fread(stream, 1, (size_t)stream_bytes, f) != (size_t)stream_bytes) { fprintf(stderr, "short stream\n"); return 1; }
    fclose(f);
    if (stream_bytes % 16 != 0 || !jpeg_tables_ok(t.data(), n, n_segs, n_quant, n_huff, H, W, stream_bytes, dst_slots)) {
        fprintf(stderr, "tables refused\n");
        return 2;
    }

    const long long slot_bytes = jpeg_slot_bytes(H, W), ws_bytes = slot_bytes * n, frame = 3ll * H * W, dst_bytes = frame * dst_slots;
    std::vector<int> status((size_t)n, 0), stats((size_t)n_segs * 2 + 2, 0);
    int taken = 0;
    {
        Guarded<uint8_t> ws((size_t)ws_bytes), dst((size_t)dst_bytes);
        Batch B = {stream, stream_bytes, t.data(), nullptr, nullptr, nullptr, n, n_quant, n_huff, H, W, ws.p, slot_bytes};
        B.seg = B.img + (long long)n * JPEG_IMG_COLS;
        const int* slot = B.seg + (long long)n_segs * JPEG_SEG_COLS;
        B.quant = slot + n;
        B.huff = B.quant + (long long)n_quant * JPEG_QUANT_INTS;
        for (int s = 0; s < n_segs; ++s) {
            const JpegSegment S = jpeg_segment_resolve(B.img, B.seg, s, n, H, W, stream_bytes);
            if (!S.live) continue;
            if (jpeg_par_takes(walk, S.bytes, S.Ri * S.g.blocks, par_min, par_max)) {
                status[S.i] |= par_segment(B, S, sub_bytes, lanes, stats.data() + 2 * s);
                ++taken;
            } else {
                status[S.i] |= seq_segment(B, S);
            }
        }
        for (int i = 0; i < n; ++i) {
            const int* im = B.img + (long long)i * JPEG_IMG_COLS;
            uint8_t* o = dst.p + frame * slot[i];
            if (!(im[0] & 1)) { memset(o, 0, (size_t)frame); continue; }
            const JpegGeom g = jpeg_geom(im, H, W);
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x, o += 3) {
                    const uint32_t p = jpeg_pixel(ws.p + slot_bytes * i, g, y, x);
                    o[order ? 0 : 2] = (uint8_t)p; o[1] = (uint8_t)(p >> 8); o[order ? 2 : 0] = (uint8_t)(p >> 16);
                }
        }
        f = fopen(argv[2], "wb");
        if (!f) { perror(argv[2]); return 1; }
        fwrite(status.data(), 4, (size_t)n, f);
        fwrite(dst.p, 1, (size_t)dst_bytes, f);
        fclose(f);
        if (par) {
            const std::string side = std::string(argv[2]) + ".stats";
            f = fopen(side.c_str(), "wb");
            if (!f) { perror(side.c_str()); return 1; }
            fwrite(stats.data(), 4, (size_t)n_segs * 2, f);
            fclose(f);
        }
    }
    free(stream);
    if (g_guard_bad) { fprintf(stderr, "a guard byte changed\n"); return 3; }
    int nz = 0;
    for (int i = 0; i < n; ++i) nz += status[i] != 0;
    printf("decoded %d images, %d with a non-zero status, %d of %d segments by the parallel walk\n", n, nz, taken, n_segs);
    return 0;
}
