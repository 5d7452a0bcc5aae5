// Baseline-JPEG decoding, the rules of the PARALLEL walk of one entropy-coded segment (include/m3t_hip.h, m3t_jpeg_decode_walk) as host +
// device inline functions: what one lane does in each phase.  csrc/jpeg.hip (jpeg_par_kernel) runs this text with one workgroup per
// segment; the stand-alone program csrc/jpeg_par_host_check.cpp runs the same text on the host, a loop over the lane index per phase.
// The walk works on an UNSTUFFED image of the segment: the bytes in front of the first marker (or lone FF) with every FF 00 turned into
// FF, as 32-bit words in stream order; a position is a plain bit offset into it and bits past its end are zero, which is what the
// sequential reader (jpeg_core.h) supplies there.  Two walks:
//   lenient  jpeg_par_walk: from any state (bit, block of the MCU, zig-zag position k; k = 0: a DC symbol is next).  A bit pattern that
//            is no code skips one bit, a coefficient past 63 closes the block.  From a true state on a sound stream it takes the steps of
//            the strict walk; from a wrong state it tends to fall into step with it (self-synchronisation).
//   strict   jpeg_par_block: one block by the rules of jpeg_decode_block, error for error and bit for bit.
// Rules of this file: every read of the image is bounded by its word count, every loop has a bound that is an argument, every
// coefficient index is checked to be < 64, and nothing here writes anywhere but into the caller's state and coefficient block.
// The host is taken to be little-endian, as the device is.
#pragma once
#include "jpeg_core.h"

#if defined(__HIPCC__)
#define JPEG_PAR_UNROLL _Pragma("unroll")
#else
#define JPEG_PAR_UNROLL
#endif

#define JPEG_PAR_MAX_BYTES 49152     // the largest segment (stuffed bytes) the parallel walk takes in this build
#define JPEG_PAR_MAX_BLOCKS 4096     // the most blocks (MCUs of a segment x blocks of an MCU) it takes
#define JPEG_PAR_SUB_MIN 16
#define JPEG_PAR_SUB_MAX 4096
#define JPEG_PAR_COEF_STRIDE 66      // int16 between the coefficient blocks of neighbouring lanes (33 dwords: no two lanes on one bank pair)
#define JPEG_PAR_FINISH_ITERS 4096   // bound of the walk that closes a block begun in an earlier sub-sequence (a block is < 1 984 bits)
#define JPEG_PAR_NO_MARKER 0x7fffffff

struct JpegParCtx {
    const uint32_t* ubw; int nw;     // the unstuffed image: nw words may be read, whatever lies behind the image's last byte is zero
    uint32_t ubits;                  // 8 x its bytes
    const int* huff;                 // six tables in lookup form: DC, AC of component 0, 1, 2
    int ncomp, ny, blocks;           // components, luma blocks per MCU, blocks per MCU
};

struct JpegParState { uint32_t p; int b, k; };

JPEG_HD int jpeg_par_comp(const JpegParCtx& c, int b) { return (c.ncomp == 1 || b < c.ny) ? 0 : (b - c.ny + 1 > 2 ? 2 : b - c.ny + 1); }

JPEG_HD uint32_t jpeg_par_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }

// the 32 bits from bit p on, MSB first; zero past the image
JPEG_HD uint32_t jpeg_par_peek(const JpegParCtx& c, uint32_t p) {
    const uint32_t w = p >> 5, sh = p & 31u;
    const uint32_t hi = w < (uint32_t)c.nw ? jpeg_par_bswap(c.ubw[w]) : 0u;
    const uint32_t lo = w + 1u < (uint32_t)c.nw ? jpeg_par_bswap(c.ubw[w + 1u]) : 0u;
    return (uint32_t)(((((uint64_t)hi << 32) | lo) << sh) >> 32);
}

// the symbol at the top of v and its length, or -1: jpeg_symbol's lookup without its reader
JPEG_HD int jpeg_par_symbol(uint32_t v32, const JpegHuff& h, int& len) {
    const unsigned v = v32 >> 16;
    const unsigned e = h.lut[v >> (16 - JPEG_HUFF_LUT_BITS)];
    int sym = (int)(e & 255u);
    len = (int)(e >> 8);
    if (e == 0u) {
        sym = -1;
        for (len = JPEG_HUFF_LUT_BITS + 1; len <= 16; ++len) {
            const int code = (int)(v >> (16 - len));
            if (code <= h.maxcode[len]) { sym = h.vals[(h.valoff[len] + code) & 255]; break; }
        }
        if (sym < 0) return -1;
    }
    if (len < 1 || len > 16) return -1;
    return sym;
}

// the s <= 15 bits behind a code of len bits at the top of v (len + s <= 31)
JPEG_HD int jpeg_par_value(uint32_t v32, int len, int s) { return s ? (int)((v32 << len) >> (32 - s)) : 0; }

// The lenient walk.  finish = false: until the first symbol boundary at or after end_bit; finish = true: until the block the state is
// inside closes (k == 0).  Returns the blocks begun (DC symbols taken).  Every step consumes at least one bit; max_iter bounds the steps.
JPEG_HD int jpeg_par_walk(const JpegParCtx& c, JpegParState& s, uint32_t end_bit, bool finish, int max_iter) {
    int nb = 0;
    for (int it = 0; it < max_iter; ++it) {
        if (finish ? s.k == 0 : s.p >= end_bit) break;
        const int comp = jpeg_par_comp(c, s.b);
        const uint32_t v = jpeg_par_peek(c, s.p);
        int len;
        if (s.k == 0) {
            const int sym = jpeg_par_symbol(v, jpeg_huff_at(c.huff + (2 * comp) * JPEG_HUFF_INTS), len);
            if (sym < 0 || sym > 15) { s.p += 1u; continue; }
            s.p += (uint32_t)(len + sym);
            s.k = 1;
            ++nb;
            continue;
        }
        const int sym = jpeg_par_symbol(v, jpeg_huff_at(c.huff + (2 * comp + 1) * JPEG_HUFF_INTS), len);
        if (sym < 0) { s.p += 1u; continue; }
        s.p += (uint32_t)len;
        const int run = sym >> 4, sz = sym & 15;
        bool close;
        if (sz == 0) {
            if (run != 15) close = true;
            else { s.k += 16; close = s.k >= 64; }
        } else {
            s.k += run;
            if (s.k >= 64) close = true;
            else { s.p += (uint32_t)sz; ++s.k; close = s.k >= 64; }
        }
        if (close) { s.k = 0; s.b = s.b + 1 >= c.blocks ? 0 : s.b + 1; }
    }
    return nb;
}

// The strict walk of one block from bit p: jpeg_decode_block on the unstuffed image.  p advances by exactly the bits the sequential reader
// would have consumed, also where it returns a status.  coef: 64 int16 in natural order, zeroed by the caller, or null (walk only);
// dc: what coef[0] receives (the predictor with this block's difference in it, which the caller summed); diff: the DC difference read.
JPEG_HD int jpeg_par_block(const JpegParCtx& c, uint32_t& p, int comp, const uint8_t* zz, int16_t* coef, int dc, int& diff) {
    const JpegHuff hd = jpeg_huff_at(c.huff + (2 * comp) * JPEG_HUFF_INTS), ha = jpeg_huff_at(c.huff + (2 * comp + 1) * JPEG_HUFF_INTS);
    int len;
    uint32_t v = jpeg_par_peek(c, p);
    int s = jpeg_par_symbol(v, hd, len);
    diff = 0;
    if (s < 0) return JPEG_ST_CODE;
    p += (uint32_t)len;
    if (s > 15) return JPEG_ST_CODE;
    diff = jpeg_extend(jpeg_par_value(v, len, s), s);
    p += (uint32_t)s;
    if (coef) coef[0] = (int16_t)dc;
    for (int k = 1; k < 64;) {
        v = jpeg_par_peek(c, p);
        const int rs = jpeg_par_symbol(v, ha, len);
        if (rs < 0) return JPEG_ST_CODE;
        p += (uint32_t)len;
        const int run = rs >> 4;
        s = rs & 15;
        if (s == 0) {
            if (run != 15) break;
            k += 16;
            continue;
        }
        k += run;
        if (k >= 64) return JPEG_ST_CODE;
        const int val = jpeg_extend(jpeg_par_value(v, len, s), s);
        p += (uint32_t)s;
        if (coef) coef[zz[k]] = (int16_t)val;
        ++k;
    }
    return 0;
}

// ---- staging: one 16-byte granule of the stuffed stream ---------------------------------------------------------------------------------
// Positions are relative to the 16-byte aligned address at or below the segment's first byte; the segment is [lo, hi).  w: the granule
// at position q0, little-endian words; prev: the byte in front of it (any value where q0 - 1 < lo); next: the byte behind it, -1 where
// q0 + 16 >= hi.
JPEG_HD int jpeg_par_byte(const uint32_t w[4], int j) { return (int)((w[j >> 2] >> (8 * (j & 3))) & 255u); }

// the stuffed zeros of the granule (a 00 behind an FF, both inside the segment); marker: lowered to the position of an FF inside the
// segment that a non-zero byte or the segment's end follows
JPEG_HD int jpeg_par_granule_count(const uint32_t w[4], int prev, int next, int q0, int lo, int hi, int& marker) {
    int n = 0;
    JPEG_PAR_UNROLL
    for (int j = 0; j < 16; ++j) {
        const int q = q0 + j;
        if (q < lo || q >= hi) continue;
        const int cur = jpeg_par_byte(w, j);
        const int pv = q - 1 >= lo ? (j ? jpeg_par_byte(w, j - 1) : prev) : 0;
        const int nx = q + 1 < hi ? (j < 15 ? jpeg_par_byte(w, j + 1) : next) : -1;
        if (cur == 0 && pv == 0xFF) ++n;
        if (cur == 0xFF && nx != 0 && q < marker) marker = q;
    }
    return n;
}

// write the granule's bytes in front of `uend` (the segment's end or its first marker) to the unstuffed image: byte q goes to
// q - lo - (stuffed zeros in front of it); before: the stuffed zeros in front of this granule.  Returns one past the last index written.
JPEG_HD int jpeg_par_granule_write(const uint32_t w[4], int prev, int q0, int lo, int uend, int before, uint8_t* ub, int ub_bytes) {
    int top = 0;
    JPEG_PAR_UNROLL
    for (int j = 0; j < 16; ++j) {
        const int q = q0 + j;
        if (q < lo || q >= uend) continue;
        const int cur = jpeg_par_byte(w, j);
        const int pv = q - 1 >= lo ? (j ? jpeg_par_byte(w, j - 1) : prev) : 0;
        if (cur == 0 && pv == 0xFF) { ++before; continue; }
        const int d = q - lo - before;
        if (d >= 0 && d < ub_bytes) { ub[d] = (uint8_t)cur; top = d + 1; }
    }
    return top;
}

// ---- routing and sizes, the same on the host and in both kernels -------------------------------------------------------------------------
JPEG_HD bool jpeg_par_takes(int walk, int seg_bytes, int seg_blocks, int par_min_bytes, int par_max_bytes) {
    return walk == 1 && seg_bytes >= par_min_bytes && seg_bytes <= par_max_bytes && seg_bytes <= JPEG_PAR_MAX_BYTES && seg_blocks <= JPEG_PAR_MAX_BLOCKS;
}

JPEG_HD int jpeg_par_subs(int ubytes, int sub_bytes) { const int n = (ubytes + sub_bytes - 1) / sub_bytes; return n < 1 ? 1 : n; }

// the words of an unstuffed image of ubytes bytes that may be read: two zero words behind its last (partly filled) word
JPEG_HD int jpeg_par_words(int ubytes) { return (ubytes + 3) / 4 + 2; }

// the status of a finished parallel walk of a segment without a marker inside: fin = the bit position when the walk ended (after the last
// block, or where the strict walk raised err).  Equal to the sequential reader's: it has consumed zero bits past the end exactly where
// fin > ubits, and it has whole bytes left exactly where ubits - fin >= 8.
JPEG_HD int jpeg_par_tail(uint32_t fin, uint32_t ubits, int err) {
    int st = err;
    if (fin > ubits) st |= JPEG_ST_TRUNC;
    else if (!err && ubits - fin >= 8u) st |= JPEG_ST_EXTRA;
    return st;
}
