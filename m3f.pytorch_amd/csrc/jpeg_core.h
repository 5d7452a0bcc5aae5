// Baseline-JPEG decoding, the sequential rules as host + device inline functions (include/m3t_hip.h, m3t_jpeg_decode): the bit reader
// with unstuffing, the Huffman lookup, one block's entropy decode, libjpeg's integer IDCT (jidctint.c, jpeg_idct_islow), its "fancy"
// chroma upsampling (jdsample.c) and its colour conversion (jdcolor.c); and what every walk of a segment begins and ends with: the
// segment resolved from the tables (jpeg_segment_resolve), its tables where the walk reads them, its status.  csrc/jpeg.hip runs this
// text on the GPU; the stand-alone program csrc/jpeg_host_check.cpp compiles the same text for the host, which is how it is tested
// without one.
// Rules of this file: every read of the stream is bounded by the segment's end (past it the reader supplies zero bits and the status
// says so), every coefficient index is checked to be < 64, a Huffman miss raises the status and ends the segment, and nothing here
// writes anywhere but into the caller's coefficient block, table copies and plane rows.  All arithmetic is 32-bit and wraps (unsigned) where a damaged stream could
// overflow, so host and device agree on every input.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define JPEG_HD __host__ __device__ __forceinline__
#define JPEG_UNROLL _Pragma("unroll")
#else
#define JPEG_HD inline
#define JPEG_UNROLL
#endif

// status bits of one image (M3T_JPEG_* of include/m3t_hip.h)
#define JPEG_ST_TRUNC 1      // a segment ended before its MCUs did (zero bits were supplied)
#define JPEG_ST_CODE 2       // a bit pattern that is no Huffman code, a coefficient past 63, a DC size above 15
#define JPEG_ST_RST 4        // a restart marker missing, extra, out of order, or a marker inside a segment
#define JPEG_ST_EXTRA 8      // a segment with whole bytes left after its last MCU

// tables, as ints (m3t.jpeg.pack builds them, m3t_jpeg_decode validates them on the host)
#define JPEG_IMG_COLS 16     // flags, ncomp, hs, vs, Ri, seg0, nseg, quant[3], dc[3], ac[3]
#define JPEG_SEG_COLS 4      // image, byte offset, byte length, restart marker in front (-1: first segment, -2: not found, 0..7)
#define JPEG_QUANT_INTS 32   // 64 uint16, natural (row-major) order
#define JPEG_HUFF_INTS 384   // uint16 lut[512] | int maxcode[18] | int valoff[18] | uint8 vals[256] | pad
#define JPEG_HUFF_LUT_BITS 9
#define JPEG_WINDOW 1024     // bytes of stream a reader sees at once; a block consumes fewer than 512 (64 symbols of <= 31 bits, stuffed)

struct JpegHuff {            // one table where the decoder reads it (LDS on the device)
    const uint16_t* lut; const int* maxcode; const int* valoff; const uint8_t* vals;
};
JPEG_HD JpegHuff jpeg_huff_at(const int* t) {
    JpegHuff h;
    h.lut = reinterpret_cast<const uint16_t*>(t);
    h.maxcode = t + 256;
    h.valoff = t + 274;
    h.vals = reinterpret_cast<const uint8_t*>(t + 292);
    return h;
}

// natural index of zig-zag position k: the decoder is handed a copy (LDS on the device)
#define JPEG_ZIGZAG_INIT {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, \
                          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}

// The reader: bytes [pos, end) of the stream are still to come; the window holds bytes [win_base, win_base + win_len) of it.
// buf holds cnt <= 64 valid bits, right-aligned; `fake` of them (the lowest) are zeros supplied past the end.
struct JpegReader {
    const uint8_t* win; int win_base, win_len;
    int pos, end;
    uint64_t buf; int cnt, fake;
    int status;
};

JPEG_HD void jpeg_reader_init(JpegReader& r, const uint8_t* win, int win_base, int win_len, int pos, int end) {
    r.win = win; r.win_base = win_base; r.win_len = win_len; r.pos = pos; r.end = end; r.buf = 0u; r.cnt = 0; r.fake = 0; r.status = 0;
}

// one byte of the stream, or -1 past the end / outside the window (the caller's window always covers a block; the check keeps a broken
// invariant from reading outside the buffer)
JPEG_HD int jpeg_byte(const JpegReader& r, int i) {
    const unsigned o = (unsigned)(i - r.win_base);
    return (i < r.end && o < (unsigned)r.win_len) ? (int)r.win[o] : -1;
}

// called with cnt <= 32 -> 32 <= cnt <= 64: four bytes at once where none of them needs a look (the common case), else byte by byte
JPEG_HD void jpeg_fill(JpegReader& r) {
    const unsigned o = (unsigned)(r.pos - r.win_base);
    if (r.cnt <= 32 && r.pos + 4 <= r.end && r.win_len >= 4 && o <= (unsigned)(r.win_len - 4)) {
        const uint32_t b0 = r.win[o], b1 = r.win[o + 1], b2 = r.win[o + 2], b3 = r.win[o + 3];
        if (b0 != 0xFFu && b1 != 0xFFu && b2 != 0xFFu && b3 != 0xFFu) {
            r.buf = (r.buf << 32) | (uint64_t)((b0 << 24) | (b1 << 16) | (b2 << 8) | b3);
            r.cnt += 32; r.pos += 4;
            return;
        }
    }
    while (r.cnt <= 56) {
        int b = jpeg_byte(r, r.pos);
        if (b == 0xFF) {
            const int b2 = jpeg_byte(r, r.pos + 1);
            if (b2 == 0) {
                r.pos += 2;                      // FF 00 unstuffs to FF
            } else {                             // a marker (or FF as the last byte) inside a segment: nothing more to read
                r.status |= JPEG_ST_RST;
                r.end = r.pos;
                b = -1;
            }
        } else if (b >= 0) {
            r.pos += 1;
        }
        if (b < 0) {
            r.buf <<= 8; r.cnt += 8; r.fake += 8;
        } else {
            r.buf = (r.buf << 8) | (uint64_t)b; r.cnt += 8;
        }
    }
}

JPEG_HD void jpeg_used(JpegReader& r) {          // after consuming: bits taken from the zeros past the end are a truncation
    if (r.cnt < r.fake) { r.status |= JPEG_ST_TRUNC; r.fake = r.cnt; }
}

JPEG_HD int jpeg_bits(JpegReader& r, int n) {    // n <= 16 bits, MSB first
    if (n == 0) return 0;
    if (r.cnt < n) jpeg_fill(r);
    r.cnt -= n;
    const int v = (int)((uint32_t)(r.buf >> r.cnt) & ((1u << n) - 1u));
    jpeg_used(r);
    return v;
}

JPEG_HD int jpeg_extend(int v, int s) {          // the signed value of an s-bit field (T.81 F.2.2.1)
    return (s > 0 && v < (1 << (s - 1))) ? v - (1 << s) + 1 : v;
}

// one Huffman symbol, or -1 for a bit pattern that is no code of the table
JPEG_HD int jpeg_symbol(JpegReader& r, const JpegHuff& h) {
    if (r.cnt <= 32) jpeg_fill(r);               // >= 32 bits: the code and the value bits behind it
    const unsigned v = (unsigned)(r.buf >> (r.cnt - 16)) & 0xFFFFu;
    const unsigned e = h.lut[v >> (16 - JPEG_HUFF_LUT_BITS)];
    int len = (int)(e >> 8), sym = (int)(e & 255u);
    if (e == 0u) {
        sym = -1;
        for (len = JPEG_HUFF_LUT_BITS + 1; len <= 16; ++len) {
            const int code = (int)(v >> (16 - len));
            if (code <= h.maxcode[len]) { sym = h.vals[(h.valoff[len] + code) & 255]; break; }
        }
        if (sym < 0) return -1;
    }
    if (len < 1 || len > 16) return -1;          // (a table m3t_jpeg_decode's validation would have refused)
    r.cnt -= len;
    jpeg_used(r);
    return sym;
}

// One block: coef[64] (natural order, zero-filled by the caller) receives the DC and the AC values; `pred` is the component's DC
// predictor.  Returns 0, or a status that ends the segment.  store = false: walk the symbols without writing (jpeg_segment_status).
JPEG_HD int jpeg_decode_block(JpegReader& r, const JpegHuff& dc, const JpegHuff& ac, const uint8_t* zz, int& pred, int16_t* coef, bool store) {
    int s = jpeg_symbol(r, dc);
    if (s < 0 || s > 15) return JPEG_ST_CODE;
    pred = (int)(int16_t)(pred + jpeg_extend(jpeg_bits(r, s), s));       // (wraps at 16 bits for a damaged stream; never for a valid one)
    if (store) coef[0] = (int16_t)pred;
    for (int k = 1; k < 64;) {
        const int rs = jpeg_symbol(r, ac);
        if (rs < 0) return JPEG_ST_CODE;
        const int run = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (run != 15) break;                // end of block
            k += 16;                             // ZRL
            continue;
        }
        k += run;
        if (k >= 64) return JPEG_ST_CODE;        // a coefficient past the block
        const int v = jpeg_extend(jpeg_bits(r, s), s);
        if (store) coef[zz[k]] = (int16_t)v;
        ++k;
    }
    return 0;
}

// what a finished segment's reader says about its end
JPEG_HD int jpeg_segment_tail(const JpegReader& r) {
    return (r.pos < r.end || r.cnt - r.fake >= 8) ? JPEG_ST_EXTRA : 0;
}

// ---- jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2 -----------------------------------------------------------------------------------
typedef uint32_t jpeg_u;
JPEG_HD int32_t jpeg_sra(jpeg_u x, int n) { return (int32_t)x >> n; }
JPEG_HD jpeg_u jpeg_descale(jpeg_u x, int n) { return (jpeg_u)jpeg_sra(x + ((jpeg_u)1 << (n - 1)), n); }

// eight inputs (already dequantised) -> eight outputs, both passes share the butterfly; shift 11 for columns, 18 for rows
JPEG_HD void jpeg_idct_1d(const jpeg_u c[8], jpeg_u o[8], int shift) {
    jpeg_u z1 = (c[2] + c[6]) * (jpeg_u)4433;
    jpeg_u t2 = z1 - c[6] * (jpeg_u)15137;
    jpeg_u t3 = z1 + c[2] * (jpeg_u)6270;
    jpeg_u t0 = (c[0] + c[4]) << 13;
    jpeg_u t1 = (c[0] - c[4]) << 13;
    const jpeg_u t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    t0 = c[7]; t1 = c[5]; t2 = c[3]; t3 = c[1];
    z1 = t0 + t3;
    jpeg_u z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const jpeg_u z5 = (z3 + z4) * (jpeg_u)9633;
    t0 *= (jpeg_u)2446; t1 *= (jpeg_u)16819; t2 *= (jpeg_u)25172; t3 *= (jpeg_u)12299;
    z1 *= (jpeg_u)(-7373); z2 *= (jpeg_u)(-20995); z3 *= (jpeg_u)(-16069); z4 *= (jpeg_u)(-3196);
    z3 += z5; z4 += z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    o[0] = jpeg_descale(t10 + t3, shift); o[7] = jpeg_descale(t10 - t3, shift);
    o[1] = jpeg_descale(t11 + t2, shift); o[6] = jpeg_descale(t11 - t2, shift);
    o[2] = jpeg_descale(t12 + t1, shift); o[5] = jpeg_descale(t12 - t1, shift);
    o[3] = jpeg_descale(t13 + t0, shift); o[4] = jpeg_descale(t13 - t0, shift);
}

// column x of a block: coef (natural order) times the quantisation table -> ws[8 rows][8] column x
JPEG_HD void jpeg_idct_col(const int16_t* coef, const uint16_t* q, int x, int32_t* ws) {
    jpeg_u c[8], o[8];
    for (int y = 0; y < 8; ++y) c[y] = (jpeg_u)((int)coef[8 * y + x] * (int)q[8 * y + x]);
    jpeg_idct_1d(c, o, 11);
    for (int y = 0; y < 8; ++y) ws[8 * y + x] = (int32_t)o[y];
}

JPEG_HD int jpeg_clamp(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// row y of a block: ws row -> eight samples, packed little-endian into two words (byte x of the row is sample x)
JPEG_HD void jpeg_idct_row(const int32_t* ws, int y, uint32_t& lo, uint32_t& hi) {
    jpeg_u c[8], o[8];
    for (int x = 0; x < 8; ++x) c[x] = (jpeg_u)ws[8 * y + x];
    jpeg_idct_1d(c, o, 18);
    lo = 0u; hi = 0u;
    for (int x = 0; x < 4; ++x) {
        lo |= (uint32_t)jpeg_clamp((int32_t)o[x] + 128) << (8 * x);
        hi |= (uint32_t)jpeg_clamp((int32_t)o[x + 4] + 128) << (8 * x);
    }
}

// ---- geometry of one image ----------------------------------------------------------------------------------------------------------
struct JpegGeom {
    int ncomp, hs, vs;               // luma sampling (chroma is 1 x 1); gray: 1, 1, 1
    int mcus_x, mcus_y, blocks;      // MCU grid and blocks per MCU
    int stride[3], rows[3];          // block-padded plane sizes
    int cw, ch;                      // the chroma planes' real size: ceil(W / hs), ceil(H / vs)
    long long plane[3];              // byte offset of each plane in the image's workspace slot
};

JPEG_HD long long jpeg_slot_bytes(int H, int W) {           // room for any mode: three planes padded to 16 x 16 MCUs
    return 3ll * ((H + 15) & ~15) * ((W + 15) & ~15);
}

JPEG_HD JpegGeom jpeg_geom(const int* img, int H, int W) {
    JpegGeom g;
    g.ncomp = img[1]; g.hs = img[2]; g.vs = img[3];
    g.mcus_x = (W + 8 * g.hs - 1) / (8 * g.hs);
    g.mcus_y = (H + 8 * g.vs - 1) / (8 * g.vs);
    g.blocks = g.ncomp == 1 ? 1 : g.hs * g.vs + 2;
    g.stride[0] = g.mcus_x * g.hs * 8; g.rows[0] = g.mcus_y * g.vs * 8;
    g.stride[1] = g.stride[2] = g.mcus_x * 8; g.rows[1] = g.rows[2] = g.mcus_y * 8;
    g.cw = (W + g.hs - 1) / g.hs; g.ch = (H + g.vs - 1) / g.vs;
    const long long p = (long long)((H + 15) & ~15) * ((W + 15) & ~15);
    g.plane[0] = 0; g.plane[1] = p; g.plane[2] = 2 * p;
    return g;
}

// block b of MCU m: its component and where its 8 x 8 samples go in that component's plane
JPEG_HD void jpeg_block_place(const JpegGeom& g, int m, int b, int& comp, int& y0, int& x0) {
    const int my = m / g.mcus_x, mx = m - my * g.mcus_x, ny = g.hs * g.vs;
    if (g.ncomp == 1 || b < ny) {
        comp = 0;
        const int v = b / g.hs, h = b - v * g.hs;
        y0 = (my * g.vs + v) * 8; x0 = (mx * g.hs + h) * 8;
    } else {
        comp = b - ny + 1;
        y0 = my * 8; x0 = mx * 8;
    }
}

// sample (y, x) of component comp in the slot, without an index into g's arrays (a JpegGeom indexed by a variable lives in scratch)
JPEG_HD long long jpeg_plane_offset(const JpegGeom& g, int comp, int y, int x) {
    return comp * g.plane[1] + (long long)y * (comp ? g.stride[1] : g.stride[0]) + x;
}

// ---- one entropy-coded segment: what it is, its tables, its status ------------------------------------------------------------------------
// aligned 16-byte load and 8-byte store as the device issues them (one instruction) and the host may (no type is punned)
JPEG_HD void jpeg_load16(const uint8_t* p, uint32_t w[4]) { __builtin_memcpy(w, __builtin_assume_aligned(p, 16), 16); }
JPEG_HD void jpeg_store8(uint8_t* p, uint32_t lo, uint32_t hi) {
    const uint32_t w[2] = {lo, hi};
    __builtin_memcpy(__builtin_assume_aligned(p, 8), w, 8);
}

JPEG_HD int jpeg_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct JpegSegment {
    bool live;                       // false: nothing to decode (an index outside the tables, an absent image); nothing else is set then
    int i, k, Ri, m0, m1;            // the image, the segment's number in it, the restart interval, its MCUs [m0, m1)
    int bytes, mark;                 // the table's byte length (what the routing rule reads) and restart marker in front
    long long off, end;              // its bytes in the stream, clamped to it
    int im[JPEG_IMG_COLS];           // the image's row, components and sampling factors normalised
    JpegGeom g;
};

// Segment s of the tables.  The host validated them; the clamps change nothing then and keep every later index inside its table.
JPEG_HD JpegSegment jpeg_segment_resolve(const int* img, const int* seg, int s, int n, int H, int W, long long stream_bytes) {
    JpegSegment S = {};
    const int* sg = seg + (long long)JPEG_SEG_COLS * s;
    S.i = sg[0];
    if (S.i < 0 || S.i >= n) return S;
    const int* row = img + (long long)JPEG_IMG_COLS * S.i;
    if (!(row[0] & 1)) return S;
    JPEG_UNROLL
    for (int c = 0; c < JPEG_IMG_COLS; ++c) S.im[c] = row[c];
    S.im[1] = S.im[1] == 1 ? 1 : 3;
    S.im[2] = S.im[1] == 1 ? 1 : jpeg_clampi(S.im[2], 1, 2);
    S.im[3] = S.im[1] == 1 ? 1 : jpeg_clampi(S.im[3], 1, 2);
    S.g = jpeg_geom(S.im, H, W);
    const int total = S.g.mcus_x * S.g.mcus_y;
    S.Ri = jpeg_clampi(S.im[4], 1, total);
    S.k = s - S.im[5];
    if (S.k < 0 || (long long)S.k * S.Ri >= total) return S;
    S.m0 = S.k * S.Ri; S.m1 = S.m0 + S.Ri < total ? S.m0 + S.Ri : total;
    S.bytes = sg[2]; S.mark = sg[3];
    const long long o = sg[1] < 0 ? 0 : sg[1], len = sg[2] < 0 ? 0 : sg[2];
    S.off = o < stream_bytes ? o : stream_bytes;
    S.end = S.off + len < stream_bytes ? S.off + len : stream_bytes;
    S.live = true;
    return S;
}

// what the tables alone say of a segment: its restart marker is not the one its number asks for, or the packer saw the markers disagree
JPEG_HD int jpeg_segment_rst(const JpegSegment& S) {
    return ((S.k > 0 && S.mark != ((S.k - 1) & 7)) || (S.im[0] & 2)) ? JPEG_ST_RST : 0;
}

// Lane t of T copies the image's tables to where the walk reads them: huff = DC, AC of component 0, 1, .. in lookup form, quant beside
// it, for nc components (behind the image's last one: copies of component 0's, so that every read finds initialised memory).
JPEG_HD void jpeg_tables_load(int* huff, int* quant, const JpegSegment& S, int nc, const int* huff_t, int n_huff, const int* quant_t, int n_quant,
                              int t, int T) {
    JPEG_UNROLL
    for (int c = 0; c < 3; ++c) {                            // (unrolled: the row is read at constant indices and stays in registers)
        if (c >= nc) break;
        const bool own = c < S.g.ncomp;
        const int* hd = huff_t + (long long)JPEG_HUFF_INTS * jpeg_clampi(own ? S.im[10 + c] : S.im[10], 0, n_huff - 1);
        const int* ha = huff_t + (long long)JPEG_HUFF_INTS * jpeg_clampi(own ? S.im[13 + c] : S.im[13], 0, n_huff - 1);
        const int* q = quant_t + (long long)JPEG_QUANT_INTS * jpeg_clampi(own ? S.im[7 + c] : S.im[7], 0, n_quant - 1);
        for (int j = t; j < JPEG_HUFF_INTS; j += T) {
            __builtin_memcpy(huff + (2 * c) * JPEG_HUFF_INTS + j, hd + j, 4);                 // (read as uint16 and uint8 later)
            __builtin_memcpy(huff + (2 * c + 1) * JPEG_HUFF_INTS + j, ha + j, 4);
        }
        for (int j = t; j < JPEG_QUANT_INTS; j += T) __builtin_memcpy(quant + c * JPEG_QUANT_INTS + j, q + j, 4);
    }
}

// the blocks of MCU m through the reader; coef: blocks x 64, zero-filled by the caller, unread with store = false.  False: a status ended
// the segment (it is in r.status).
JPEG_HD bool jpeg_walk_mcu(JpegReader& r, const JpegGeom& g, int m, const int* huff, const uint8_t* zz, int pred[3], int16_t* coef, bool store) {
    for (int b = 0; b < g.blocks; ++b) {
        int comp, y0, x0;
        jpeg_block_place(g, m, b, comp, y0, x0);
        const JpegHuff hd = jpeg_huff_at(huff + (2 * comp) * JPEG_HUFF_INTS), ha = jpeg_huff_at(huff + (2 * comp + 1) * JPEG_HUFF_INTS);
        const int st = jpeg_decode_block(r, hd, ha, zz, pred[comp], store ? coef + 64 * b : nullptr, store);
        if (st) { r.status |= st; return false; }
    }
    return true;
}

// The sequential reader's walk of a segment straight from the stream, for the status alone (nothing is stored): what that reader says of
// a marker inside depends on how far its look-ahead got, so a walk that reads another way asks it.  huff: as jpeg_tables_load leaves it.
JPEG_HD int jpeg_segment_status(const uint8_t* stream, long long stream_bytes, const JpegSegment& S, const int* huff, const uint8_t* zz) {
    JpegReader r;
    jpeg_reader_init(r, stream, 0, (int)(stream_bytes < 0x7fffffffll ? stream_bytes : 0x7fffffffll), (int)S.off, (int)S.end);
    int pred[3] = {0, 0, 0};
    bool dead = false;
    for (int m = S.m0; m < S.m1 && !dead; ++m) dead = !jpeg_walk_mcu(r, S.g, m, huff, zz, pred, nullptr, false);
    return r.status | (dead ? 0 : jpeg_segment_tail(r)) | jpeg_segment_rst(S);
}

// ---- fancy upsampling (jdsample.c) and colour (jdcolor.c) ---------------------------------------------------------------------------
// the chroma sample at output pixel (y, x) of a plane of real size ch x cw
JPEG_HD int jpeg_chroma(const uint8_t* p, int stride, int cw, int ch, int hs, int vs, int y, int x) {
    if (hs == 1) return p[(long long)y * stride + x];
    const int cx = x >> 1;
    if (cw <= 2) return p[(long long)(vs == 2 ? y >> 1 : y) * stride + cx];      // plain replication
    if (vs == 1) {                                                                // h2v1
        const int c = p[(long long)y * stride + cx];
        if (x & 1) return cx == cw - 1 ? c : (3 * c + p[(long long)y * stride + cx + 1] + 2) >> 2;
        return cx == 0 ? c : (3 * c + p[(long long)y * stride + cx - 1] + 1) >> 2;
    }
    const int r = y >> 1;                                                         // h2v2
    int nb = (y & 1) ? r + 1 : r - 1;
    nb = nb < 0 ? 0 : (nb > ch - 1 ? ch - 1 : nb);
    const uint8_t* cur = p + (long long)r * stride;
    const uint8_t* nbr = p + (long long)nb * stride;
    const int s = 3 * cur[cx] + nbr[cx];
    if (x & 1) {
        if (cx == cw - 1) return (4 * s + 7) >> 4;
        return (3 * s + (3 * cur[cx + 1] + nbr[cx + 1]) + 7) >> 4;
    }
    if (cx == 0) return (4 * s + 8) >> 4;
    return (3 * s + (3 * cur[cx - 1] + nbr[cx - 1]) + 8) >> 4;
}

// pixel (y, x) of an image from its planes: r | g << 8 | b << 16
JPEG_HD uint32_t jpeg_pixel(const uint8_t* slot, const JpegGeom& g, int y, int x) {
    const int Y = slot[g.plane[0] + (long long)y * g.stride[0] + x];
    if (g.ncomp == 1) return (uint32_t)Y * 0x010101u;
    const int cb = jpeg_chroma(slot + g.plane[1], g.stride[1], g.cw, g.ch, g.hs, g.vs, y, x) - 128;
    const int cr = jpeg_chroma(slot + g.plane[2], g.stride[2], g.cw, g.ch, g.hs, g.vs, y, x) - 128;
    const int R = jpeg_clamp(Y + ((91881 * cr + 32768) >> 16));
    const int G = jpeg_clamp(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
    const int B = jpeg_clamp(Y + ((116130 * cb + 32768) >> 16));
    return (uint32_t)R | ((uint32_t)G << 8) | ((uint32_t)B << 16);
}

// ---- validation of the tables, on the host (m3t_jpeg_decode; the check program) ------------------------------------------------------
// tables: images [n][16] | segments [n_segs][4] | slots [n] | quant [n_quant][32] | huff [n_huff][384]
inline long long jpeg_tables_ints(int n, int n_segs, int n_quant, int n_huff) {
    return (long long)n * JPEG_IMG_COLS + (long long)n_segs * JPEG_SEG_COLS + n + (long long)n_quant * JPEG_QUANT_INTS +
           (long long)n_huff * JPEG_HUFF_INTS;
}

inline bool jpeg_tables_ok(const int* t, int n, int n_segs, int n_quant, int n_huff, int H, int W, long long stream_bytes, long long dst_slots) {
    if (!t || n <= 0 || n_segs < 0 || n_quant < 0 || n_huff < 0 || H <= 0 || W <= 0 || H > 16384 || W > 16384 || stream_bytes < 0 ||
        stream_bytes > 0x7fffffffll - 2 * JPEG_WINDOW || dst_slots <= 0)
        return false;
    const int* img = t;
    const int* seg = img + (long long)n * JPEG_IMG_COLS;
    const int* slot = seg + (long long)n_segs * JPEG_SEG_COLS;
    const int* huff = slot + n + (long long)n_quant * JPEG_QUANT_INTS;
    for (int i = 0; i < n; ++i, img += JPEG_IMG_COLS) {
        if (slot[i] < 0 || slot[i] >= dst_slots) return false;
        if (!(img[0] & 1)) { if (img[6] != 0) return false; continue; }              // absent: no segments
        const int nc = img[1], hs = img[2], vs = img[3], Ri = img[4], seg0 = img[5], nseg = img[6];
        if (!((nc == 1 && hs == 1 && vs == 1) || (nc == 3 && ((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)))))) return false;
        const long long mcus = (long long)((W + 8 * hs - 1) / (8 * hs)) * ((H + 8 * vs - 1) / (8 * vs));
        if (Ri < 1 || Ri > mcus || nseg != (mcus + Ri - 1) / Ri || seg0 < 0 || (long long)seg0 + nseg > n_segs) return false;
        for (int c = 0; c < nc; ++c)
            if (img[7 + c] < 0 || img[7 + c] >= n_quant || img[10 + c] < 0 || img[10 + c] >= n_huff || img[13 + c] < 0 || img[13 + c] >= n_huff)
                return false;
        for (int k = 0; k < nseg; ++k) {
            const int* s = seg + (long long)(seg0 + k) * JPEG_SEG_COLS;
            if (s[0] != i || s[1] < 0 || s[2] < 0 || (long long)s[1] + s[2] > stream_bytes || s[3] < -2 || s[3] > 7) return false;
        }
    }
    for (int h = 0; h < n_huff; ++h) {
        const JpegHuff u = jpeg_huff_at(huff + (long long)h * JPEG_HUFF_INTS);
        for (int i = 0; i < (1 << JPEG_HUFF_LUT_BITS); ++i) {
            const int len = u.lut[i] >> 8;
            if (u.lut[i] != 0 && (len < 1 || len > JPEG_HUFF_LUT_BITS)) return false;
        }
    }
    return true;
}
