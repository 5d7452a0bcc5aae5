// The parallel walk of csrc/jpeg.hip (jpeg_par_kernel, rules in jpeg_par.h) on the host: this program reads one packed batch (the file
// tests/jpeg_cases.py::write_packed writes), decodes it as m3t_jpeg_decode_walk would -- per segment the parallel walk where the routing
// rule takes it, the sequential walk of jpeg_core.h elsewhere -- and writes status and pixels to a second file, the walk stats to a third.
// The workgroup is emulated: every phase of the kernel is a loop over the lane index and a barrier is the end of that loop, so a pass of
// the exchange is Jacobi (every lane reads what the pass before left), like lanes in lockstep.
//   usage : jpeg_par_host_check packed.bin out.bin walk sub_bytes par_min_bytes par_max_bytes lanes
//   input : int32 header[12] = magic, n, n_segs, n_quant, n_huff, H, W, order, dst_slots, stream_bytes, 0, 0 | tables | stream bytes
//   output: int32 status[n] | uint8 dst[dst_slots][H][W][3] (every byte the decoder did not write still GUARD): what
//           tests/jpeg_cases.py::read_result reads; and beside it out.bin.stats: int32 stats[n_segs][2] = sub-sequences, exchange passes
//           ((0, 0) for a segment the sequential walk took)
// The stream, the workspace, the destination and every array the emulated workgroup keeps are exact-size heap blocks, the ones written to
// with guard bytes around them, checked before the program reports success.  Exit 0: decoded (whatever the status words say); 2: refused
// (M3T_EINVAL's rule: the tables, walk, sub_bytes or the thresholds); 3: a guard byte changed; 1: usage or I/O.
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
    void zero() { memset(raw + GUARD_BYTES, 0, bytes); }
    ~Guarded() {
        for (int j = 0; j < GUARD_BYTES; ++j) g_guard_bad |= raw[j] != GUARD || raw[GUARD_BYTES + bytes + j] != GUARD;
        free(raw);
    }
    Guarded(const Guarded&) = delete;
    Guarded& operator=(const Guarded&) = delete;
};

struct Batch {
    const uint8_t* stream; long long stream_bytes;
    const int* t; int n, n_segs, n_quant, H, W;
    uint8_t* ws; long long slot_bytes;
};

struct SegInfo {
    int i, k, m0, m1; const int* im; const int* seg; JpegGeom g;
};

static SegInfo seg_info(const Batch& B, int s) {
    SegInfo S;
    S.seg = B.t + (long long)B.n * JPEG_IMG_COLS + (long long)s * JPEG_SEG_COLS;
    S.i = S.seg[0];
    S.im = B.t + (long long)S.i * JPEG_IMG_COLS;
    S.g = jpeg_geom(S.im, B.H, B.W);
    const int total = S.g.mcus_x * S.g.mcus_y, Ri = S.im[4];
    S.k = s - S.im[5];
    S.m0 = S.k * Ri;
    S.m1 = S.m0 + Ri < total ? S.m0 + Ri : total;
    return S;
}

static const int* quant_of(const Batch& B) { return B.t + (long long)B.n * JPEG_IMG_COLS + (long long)B.n_segs * JPEG_SEG_COLS + B.n; }
static const int* huff_of(const Batch& B) { return quant_of(B) + (long long)B.n_quant * JPEG_QUANT_INTS; }

static void idct_store(const Batch& B, const SegInfo& S, int m, int b, const int16_t* coef) {
    int comp, y0, x0;
    int32_t wsp[64];
    jpeg_block_place(S.g, m, b, comp, y0, x0);
    const uint16_t* q = reinterpret_cast<const uint16_t*>(quant_of(B) + (long long)JPEG_QUANT_INTS * S.im[7 + comp]);
    uint8_t* planes = B.ws + B.slot_bytes * S.i;
    for (int x = 0; x < 8; ++x) jpeg_idct_col(coef, q, x, wsp);
    for (int y = 0; y < 8; ++y) {
        uint32_t w[2];
        jpeg_idct_row(wsp, y, w[0], w[1]);
        uint8_t* o = planes + S.g.plane[comp] + (long long)(y0 + y) * S.g.stride[comp] + x0;
        for (int x = 0; x < 8; ++x) o[x] = (uint8_t)(w[x >> 2] >> (8 * (x & 3)));
    }
}

// the sequential walk (jpeg_entropy_idct_kernel): store = false walks for the status alone
static int seq_segment(const Batch& B, int s, bool store) {
    const SegInfo S = seg_info(B, s);
    const int* huff = huff_of(B);
    JpegReader r;
    jpeg_reader_init(r, B.stream, 0, (int)B.stream_bytes, S.seg[1], S.seg[1] + S.seg[2]);
    int pred[3] = {0, 0, 0};
    bool dead = false;
    for (int m = S.m0; m < S.m1; ++m) {
        int16_t coef[6 * 64];
        memset(coef, 0, sizeof(coef));
        for (int b = 0; b < S.g.blocks && !dead; ++b) {
            int comp, y0, x0;
            jpeg_block_place(S.g, m, b, comp, y0, x0);
            const JpegHuff hd = jpeg_huff_at(huff + (long long)JPEG_HUFF_INTS * S.im[10 + comp]);
            const JpegHuff ha = jpeg_huff_at(huff + (long long)JPEG_HUFF_INTS * S.im[13 + comp]);
            const int st = jpeg_decode_block(r, hd, ha, kZigzag, pred[comp], coef + 64 * b, store);
            if (st) { r.status |= st; dead = true; }
        }
        if (store)
            for (int b = 0; b < S.g.blocks; ++b) idct_store(B, S, m, b, coef + 64 * b);
    }
    int st = r.status | (dead ? 0 : jpeg_segment_tail(r));
    if (S.k > 0 && S.seg[3] != ((S.k - 1) & 7)) st |= JPEG_ST_RST;
    if (S.im[0] & 2) st |= JPEG_ST_RST;
    return st;
}

// the parallel walk (jpeg_par_kernel) with T emulated lanes; stats: sub-sequences, exchange passes
static int par_segment(const Batch& B, int s, int sub_bytes, int T, int* stats) {
    const SegInfo S = seg_info(B, s);
    const JpegGeom& g = S.g;
    const int nblk = (S.m1 - S.m0) * g.blocks;
    const long long off = S.seg[1], end = off + S.seg[2], base = off & ~15ll;
    const int lo = (int)(off - base), hi = (int)(end - base), G = (hi + 15) / 16;

    // the tables where the lanes read them
    Guarded<int> huff(6 * JPEG_HUFF_INTS);
    huff.zero();
    for (int c = 0; c < g.ncomp; ++c) {
        memcpy(huff.p + (2 * c) * JPEG_HUFF_INTS, huff_of(B) + (long long)JPEG_HUFF_INTS * S.im[10 + c], sizeof(int) * JPEG_HUFF_INTS);
        memcpy(huff.p + (2 * c + 1) * JPEG_HUFF_INTS, huff_of(B) + (long long)JPEG_HUFF_INTS * S.im[13 + c], sizeof(int) * JPEG_HUFF_INTS);
    }

    // ---- stage: count the stuffed zeros per granule, prefix sum, compact ----
    const int cap_u = ((S.seg[2] + 15) & ~15) + 16;
    Guarded<uint32_t> ubw((size_t)cap_u / 4);
    Guarded<uint16_t> pre((size_t)(G > 0 ? G : 1));
    uint8_t* ub = reinterpret_cast<uint8_t*>(ubw.p);
    int marker = JPEG_PAR_NO_MARKER;
    auto granule = [&](int gi, uint32_t w[4], int& prev, int& next) {
        memcpy(w, B.stream + base + 16ll * gi, 16);                      // (inside the stream: it is padded to whole granules)
        prev = gi > 0 ? B.stream[base + 16ll * gi - 1] : 0;
        next = 16 * gi + 16 < hi ? B.stream[base + 16ll * gi + 16] : -1;
    };
    for (int t = 0; t < T; ++t)
        for (int gi = t; gi < G; gi += T) {
            uint32_t w[4]; int prev, next;
            granule(gi, w, prev, next);
            pre.p[gi] = (uint16_t)jpeg_par_granule_count(w, prev, next, 16 * gi, lo, hi, marker);
        }
    const int uend = marker < hi ? marker : hi;
    int run = 0;
    for (int gi = 0; gi < G; ++gi) { const int c = pre.p[gi]; pre.p[gi] = (uint16_t)run; run += c; }
    int ulen = 0;
    for (int t = 0; t < T; ++t)
        for (int gi = t; gi < G; gi += T) {
            uint32_t w[4]; int prev, next;
            granule(gi, w, prev, next);
            const int top = jpeg_par_granule_write(w, prev, 16 * gi, lo, uend, pre.p[gi], ub, cap_u);
            if (top > ulen) ulen = top;
        }
    const int nw = jpeg_par_words(ulen);
    for (int j = ulen; j < 4 * nw; ++j) ub[j] = 0;

    JpegParCtx c;
    c.ubw = ubw.p; c.nw = nw; c.ubits = 8u * (uint32_t)ulen; c.huff = huff.p;
    c.ncomp = g.ncomp; c.ny = g.hs * g.vs; c.blocks = g.blocks;
    const int n_sub = jpeg_par_subs(ulen, sub_bytes);
    const uint32_t sub_bits = 8u * (uint32_t)sub_bytes;
    auto end_of = [&](int i) { const uint32_t e = (uint32_t)(i + 1) * sub_bits; return e < c.ubits ? e : c.ubits; };

    // ---- speculate: every sub-sequence from (its first bit, block 0, k = 0) ----
    Guarded<JpegParState> ex((size_t)n_sub), used((size_t)n_sub);
    Guarded<int> nbs((size_t)n_sub), first((size_t)n_sub);
    Guarded<uint8_t> chg((size_t)n_sub);
    for (int t = 0; t < T; ++t)
        for (int i = t; i < n_sub; i += T) {
            JpegParState st = {(uint32_t)i * sub_bits, 0, 0};
            used.p[i] = st;
            nbs.p[i] = jpeg_par_walk(c, st, end_of(i), false, 8 * sub_bytes + 1);
            ex.p[i] = st;
        }
    // ---- exchange: re-walk from the left neighbour's exit state until no exit state changes ----
    int passes = 0;
    bool any = true;
    while (any && passes < n_sub) {
        ++passes;
        any = false;
        for (int t = 0; t < T; ++t)
            for (int i = t; i < n_sub; i += T) {
                chg.p[i] = 0;
                if (i == 0) continue;
                const JpegParState e = ex.p[i - 1];
                if (e.p != used.p[i].p || e.b != used.p[i].b || e.k != used.p[i].k) { used.p[i] = e; chg.p[i] = 1; }
            }
        for (int t = 0; t < T; ++t)
            for (int i = t; i < n_sub; i += T) {
                if (!chg.p[i]) continue;
                JpegParState st = used.p[i];
                nbs.p[i] = jpeg_par_walk(c, st, end_of(i), false, 8 * sub_bytes + 1);
                if (st.p != ex.p[i].p || st.b != ex.p[i].b || st.k != ex.p[i].k) any = true;
                ex.p[i] = st;
            }
    }
    stats[0] = n_sub; stats[1] = passes;
    run = 0;
    for (int i = 0; i < n_sub; ++i) { first.p[i] = run; run += nbs.p[i]; }

    // ---- index: the strict walk of the blocks that begin in each sub-sequence ----
    Guarded<uint32_t> bstart((size_t)nblk);
    Guarded<int16_t> bdc((size_t)nblk);
    bstart.zero(); bdc.zero();
    int errsub = JPEG_PAR_NO_MARKER, errblock = nblk, errst = 0, errdiff = 0;
    uint32_t errbit = 0, errstart = 0, donebit = 0;
    for (int t = 0; t < T; ++t) {
        bool lane_err = false;
        for (int i = t; i < n_sub && !lane_err; i += T) {
            JpegParState st = {0u, 0, 0};
            if (i > 0) st = ex.p[i - 1];                                  // (converged: the state the last walk of i started from)
            int j = first.p[i];
            if (st.k) jpeg_par_walk(c, st, 0u, true, JPEG_PAR_FINISH_ITERS);
            if (st.k) continue;
            const bool last = i == n_sub - 1;
            const uint32_t e = end_of(i);
            while (j < nblk && (last || st.p < e)) {
                const uint32_t p0 = st.p;
                int diff;
                const int rc = jpeg_par_block(c, st.p, jpeg_par_comp(c, j % g.blocks), kZigzag, nullptr, 0, diff);
                if (rc) {
                    lane_err = true;
                    if (i < errsub) { errsub = i; errblock = j; errst = rc; errbit = st.p; errstart = p0; errdiff = diff; }
                    break;
                }
                bstart.p[j] = p0;
                bdc.p[j] = (int16_t)diff;
                if (++j == nblk) donebit = st.p;
            }
        }
    }
    if (errblock < nblk) { bstart.p[errblock] = errstart; bdc.p[errblock] = (int16_t)errdiff; }

    // ---- the DC predictors: per component, the running sum of the differences (wraps at 16 bits) ----
    int pred[3] = {0, 0, 0};
    for (int j = 0; j < nblk; ++j) {
        const int comp = jpeg_par_comp(c, j % g.blocks);
        pred[comp] += bdc.p[j];
        bdc.p[j] = (int16_t)pred[comp];
    }

    // ---- decode and transform: one lane a block, T blocks a round ----
    Guarded<int16_t> coef((size_t)T * JPEG_PAR_COEF_STRIDE);
    for (int r0 = 0; r0 < nblk; r0 += T) {
        coef.zero();
        for (int t = 0; t < T; ++t) {
            const int j = r0 + t;
            if (j >= nblk || j > errblock) continue;
            uint32_t p = bstart.p[j];
            int diff;
            jpeg_par_block(c, p, jpeg_par_comp(c, j % g.blocks), kZigzag, coef.p + t * JPEG_PAR_COEF_STRIDE, bdc.p[j], diff);
        }
        for (int t = 0; t < T; ++t) {
            const int j = r0 + t;
            if (j < nblk) idct_store(B, S, S.m0 + j / g.blocks, j % g.blocks, coef.p + t * JPEG_PAR_COEF_STRIDE);
        }
    }

    // ---- status ----
    int st;
    if (marker < hi) {
        st = seq_segment(B, s, false);                                   // a marker inside: what the sequential reader's look-ahead saw of it
    } else {
        st = jpeg_par_tail(errblock < nblk ? errbit : donebit, c.ubits, errst);
        if (S.k > 0 && S.seg[3] != ((S.k - 1) & 7)) st |= JPEG_ST_RST;
        if (S.im[0] & 2) st |= JPEG_ST_RST;
    }
    return st;
}

int main(int argc, char** argv) {
    if (argc != 8) { fprintf(stderr, "usage: %s packed.bin out.bin walk sub_bytes par_min_bytes par_max_bytes lanes\n", argv[0]); return 1; }
    const int walk = atoi(argv[3]), sub_bytes = atoi(argv[4]), par_min = atoi(argv[5]), par_max = atoi(argv[6]), lanes = atoi(argv[7]);
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
        const int* slot = t.data() + (long long)n * JPEG_IMG_COLS + (long long)n_segs * JPEG_SEG_COLS;
        Batch B = {stream, stream_bytes, t.data(), n, n_segs, n_quant, H, W, ws.p, slot_bytes};
        for (int s = 0; s < n_segs; ++s) {
            const SegInfo S = seg_info(B, s);
            if (jpeg_par_takes(walk, S.seg[2], S.im[4] * S.g.blocks, par_min, par_max)) {
                status[S.i] |= par_segment(B, s, sub_bytes, lanes, stats.data() + 2 * s);
                ++taken;
            } else {
                status[S.i] |= seq_segment(B, s, true);
            }
        }
        for (int i = 0; i < n; ++i) {
            const int* im = t.data() + (long long)i * JPEG_IMG_COLS;
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
        const std::string side = std::string(argv[2]) + ".stats";
        f = fopen(side.c_str(), "wb");
        if (!f) { perror(side.c_str()); return 1; }
        fwrite(stats.data(), 4, (size_t)n_segs * 2, f);
        fclose(f);
    }
    free(stream);
    if (g_guard_bad) { fprintf(stderr, "a guard byte changed\n"); return 3; }
    int nz = 0;
    for (int i = 0; i < n; ++i) nz += status[i] != 0;
    printf("decoded %d images, %d with a non-zero status, %d of %d segments by the parallel walk\n", n, nz, taken, n_segs);
    return 0;
}
