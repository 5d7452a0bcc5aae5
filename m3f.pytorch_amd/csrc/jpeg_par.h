// Baseline-JPEG decoding, the PARALLEL walk of one entropy-coded segment (include/m3t_hip.h, m3t_jpeg_decode_walk) as host + device
// inline functions: the rules of one lane AND the schedule of the workgroup -- its memory (JpegParMem, the sizes of its arrays, how they
// share LDS), its packed states and every phase between two barriers as a function of (memory, lane, lanes).  csrc/jpeg.hip
// (jpeg_par_kernel) calls the phases with a barrier between them, one workgroup per segment; the stand-alone program
// csrc/jpeg_host_check.cpp calls the same phases on the host, a loop over the lane index for each, with every array a heap block of its own.
// The walk works on an UNSTUFFED image of the segment: the bytes in front of the first marker (or lone FF) with every FF 00 turned into
// FF, as 32-bit words in stream order; a position is a plain bit offset into it and bits past its end are zero, which is what the
// sequential reader (jpeg_core.h) supplies there.  Two walks:
//   lenient  jpeg_par_walk: from any state (bit, block of the MCU, zig-zag position k; k = 0: a DC symbol is next).  A bit pattern that
//            is no code skips one bit, a coefficient past 63 closes the block.  From a true state on a sound stream it takes the steps of
//            the strict walk; from a wrong state it tends to fall into step with it (self-synchronisation).
//   strict   jpeg_par_block: one block by the rules of jpeg_decode_block, error for error and bit for bit.
// Rules of this file: every read of the image is bounded by its word count, every loop has a bound that is an argument, every
// coefficient index is checked to be < 64, and the per-lane rules write nowhere but into the caller's state and coefficient block.
// A phase contains no barrier and no lane index of its own, and a lane carries nothing from one phase to the next but what is in memory.
// The host is taken to be little-endian, as the device is.
#pragma once
#include <stddef.h>
#include "jpeg_core.h"

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
    JPEG_UNROLL
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
    JPEG_UNROLL
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

// ---- the workgroup: its memory ------------------------------------------------------------------------------------------------------------
// what the arrays of the largest segment need: bytes of the unstuffed image, granules, blocks, sub-sequences
struct JpegParCaps { int u, g, nb, sub; };

// One segment's share: off, bytes as in the tables, blocks = restart interval x blocks of an MCU.  The image is the segment's bytes
// rounded up to whole granules + 16: jpeg_par_granule_write stores below `bytes`, the zero fill and jpeg_par_peek stay below
// 4 jpeg_par_words(bytes) <= bytes + 11, and jpeg_par_segment asks for bytes + 16 -- so + 16 holds all three and more is never touched.
JPEG_HD void jpeg_par_caps_add(JpegParCaps& cap, int off, int bytes, int blocks, int sub_bytes) {
    const int u = ((bytes + 15) & ~15) + 16, g = ((off & 15) + bytes + 15) / 16, sub = jpeg_par_subs(bytes, sub_bytes);
    cap.u = u > cap.u ? u : cap.u; cap.g = g > cap.g ? g : cap.g; cap.nb = blocks > cap.nb ? blocks : cap.nb; cap.sub = sub > cap.sub ? sub : cap.sub;
}
// after the last segment: every array a multiple of 16 bytes
JPEG_HD void jpeg_par_caps_round(JpegParCaps& cap) { cap.g = (cap.g + 7) & ~7; cap.nb = (cap.nb + 7) & ~7; cap.sub = (cap.sub + 15) & ~15; }

#define JPEG_PAR_SCAN_INTS 256                                                       // lanes of a workgroup at the most (on the device)
JPEG_HD int jpeg_par_coef_count(int T) { return T * JPEG_PAR_COEF_STRIDE; }          // a coefficient block a lane
JPEG_HD int jpeg_par_wsp_count(int T) { return (T >> 3) * 64; }                      // an IDCT workspace for every eight lanes

struct JpegParWords {                // the words of the whole workgroup
    int marker, ulen, any;           // position of the first marker (min), bytes of the unstuffed image (max), an exit state changed (or)
    int errsub, errblock, errst;     // the first error: the lowest sub-sequence whose strict walk raised a status (min), its block and status
    uint32_t errbit, done;           // the bit position there; the bit position behind the segment's last block
};

struct JpegParMem {
    int* huff; int* quant;           // [6 JPEG_HUFF_INTS] [3 JPEG_QUANT_INTS]: jpeg_tables_load
    int* scr;                        // [lanes] the scan scratch: a lane's partial, then the inclusive sums
    uint8_t* ub;                     // [cap.u] the unstuffed image
    uint32_t* bstart; int16_t* bdc;  // [cap.nb] every block's first bit; its DC difference, then its DC value
    uint16_t* pre;                   // [cap.g] stage: the stuffed zeros of, then in front of, each granule
    uint32_t* ex_p; uint32_t* us_p;  // [cap.sub] speculate to index: bit of a sub-sequence's exit state and of the state it was walked from
    uint16_t* ex_bk; uint16_t* us_bk;//           (us_p in the index: its first block); (block of the MCU) << 8 | k of the two states;
    uint16_t* nbs; uint8_t* chg;     //           blocks begun; to be walked again in this pass
    int16_t* coef; int32_t* wsp;     // [jpeg_par_coef_count] [jpeg_par_wsp_count] decode
    JpegParWords* w;
    const uint8_t* zz;
    // the segment
    JpegSegment S;
    JpegParCaps cap;
    const uint8_t* src;              // the stream from the 16-byte boundary at or below the segment's first byte: the segment is [lo, hi) of
    int lo, hi, G, nblk, sub_bytes;  // it, G granules; its blocks
    uint8_t* planes;                 // the image's workspace slot
    // known once the segment is staged (jpeg_par_staged)
    JpegParCtx c; int n_sub;
};

template <bool kPlace, class E> JPEG_HD void jpeg_par_take(E*& p, unsigned char* base, size_t& o, int count) {
    p = kPlace ? reinterpret_cast<E*>(base + o) : nullptr;
    o += sizeof(E) * (size_t)count;
}

// The arrays in one block (LDS on the device) from a 16-byte aligned base; kPlace = false: the block's byte count alone, which is
// returned.  pre, the six arrays of the exchange and the two of the decode are never alive together and share their bytes.
template <bool kPlace> JPEG_HD size_t jpeg_par_carve(JpegParMem& m, unsigned char* base, const JpegParCaps& cap, int T) {
    size_t o = 0;
    jpeg_par_take<kPlace>(m.huff, base, o, 6 * JPEG_HUFF_INTS); jpeg_par_take<kPlace>(m.quant, base, o, 3 * JPEG_QUANT_INTS);
    jpeg_par_take<kPlace>(m.scr, base, o, JPEG_PAR_SCAN_INTS);
    jpeg_par_take<kPlace>(m.ub, base, o, cap.u);
    jpeg_par_take<kPlace>(m.bstart, base, o, cap.nb); jpeg_par_take<kPlace>(m.bdc, base, o, cap.nb);
    const size_t shared = o;
    jpeg_par_take<kPlace>(m.pre, base, o, cap.g);
    size_t top = o;
    o = shared;
    jpeg_par_take<kPlace>(m.ex_p, base, o, cap.sub); jpeg_par_take<kPlace>(m.us_p, base, o, cap.sub);
    jpeg_par_take<kPlace>(m.ex_bk, base, o, cap.sub); jpeg_par_take<kPlace>(m.us_bk, base, o, cap.sub);
    jpeg_par_take<kPlace>(m.nbs, base, o, cap.sub); jpeg_par_take<kPlace>(m.chg, base, o, cap.sub);
    top = o > top ? o : top;
    o = shared;
    jpeg_par_take<kPlace>(m.coef, base, o, jpeg_par_coef_count(T)); jpeg_par_take<kPlace>(m.wsp, base, o, jpeg_par_wsp_count(T));
    top = o > top ? o : top;
    return (top + 15) & ~(size_t)15;
}

// the segment's constants; false: it does not fit the arrays (the host sized them for the largest segment it routed here, so a segment that
// does not fit was not validated by it), or has no block
JPEG_HD bool jpeg_par_segment(JpegParMem& m, const JpegSegment& S, const uint8_t* stream, uint8_t* ws, long long slot_bytes, int sub_bytes,
                              const JpegParCaps& cap) {
    const long long base = S.off & ~15ll;
    m.S = S; m.cap = cap; m.sub_bytes = sub_bytes;
    m.src = stream + base;           // granule gi is src[16 gi, 16 gi + 16): inside the stream, whose size is a multiple of 16
    m.lo = (int)(S.off - base); m.hi = (int)(S.end - base); m.G = (m.hi + 15) >> 4;
    m.nblk = (S.m1 - S.m0) * S.g.blocks;
    m.planes = ws + slot_bytes * S.i;
    return m.G <= cap.g && m.hi - m.lo + 16 <= cap.u && m.nblk <= cap.nb && m.nblk >= 1;
}

// ---- the workgroup: what differs between the device and the host ---------------------------------------------------------------------------
// min, max and or into a word of the workgroup: many lanes at once on the device, one after the other on the host
JPEG_HD void jpeg_par_wg_min(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMin(p, v);
#else
    if (v < *p) *p = v;
#endif
}
JPEG_HD void jpeg_par_wg_max(int* p, int v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
JPEG_HD void jpeg_par_wg_or(int* p) { *p = 1; }

// A prefix sum across the lanes: a phase leaves lane t's partial in scr[t], the caller turns scr into its inclusive sums (cooperatively
// on the device, a serial loop on the host), the next phase reads what lies in front of lane t.
JPEG_HD int jpeg_par_before(const int* scr, int t) { return t > 0 ? scr[t - 1] : 0; }

// ---- the workgroup: its phases, each what lane t of T does between two barriers ----------------------------------------------------------------
// the share of lane t in n items cut into T runs: [a, b)
JPEG_HD void jpeg_par_run(int n, int t, int T, int& a, int& b) {
    const int C = (n + T - 1) / T;
    a = t * C < n ? t * C : n; b = a + C < n ? a + C : n;
}

JPEG_HD void jpeg_par_begin(const JpegParMem& m, int t, int T) {
    if (t == 0) {
        JpegParWords& w = *m.w;
        w.marker = JPEG_PAR_NO_MARKER; w.ulen = 0; w.any = 0; w.errsub = JPEG_PAR_NO_MARKER; w.errblock = m.nblk; w.errst = 0; w.errbit = 0u; w.done = 0u;
    }
}

JPEG_HD void jpeg_par_granule(const JpegParMem& m, int gi, uint32_t w[4], int& prev, int& next) {
    jpeg_load16(m.src + 16 * gi, w);
    prev = gi > 0 ? (int)m.src[16 * gi - 1] : 0;
    next = 16 * gi + 16 < m.hi ? (int)m.src[16 * gi + 16] : -1;
}

// stage: the stuffed zeros of every granule and the first marker
JPEG_HD void jpeg_par_stage_count(const JpegParMem& m, int t, int T) {
    int mk = JPEG_PAR_NO_MARKER;
    for (int gi = t; gi < m.G; gi += T) {
        uint32_t w[4]; int prev, next;
        jpeg_par_granule(m, gi, w, prev, next);
        m.pre[gi] = (uint16_t)jpeg_par_granule_count(w, prev, next, 16 * gi, m.lo, m.hi, mk);
    }
    if (mk != JPEG_PAR_NO_MARKER) jpeg_par_wg_min(&m.w->marker, mk);
}
// ... their prefix sum inside a lane's run (scan) ...
JPEG_HD void jpeg_par_stage_sum(const JpegParMem& m, int t, int T) {
    int g0, g1, run = 0;
    jpeg_par_run(m.G, t, T, g0, g1);
    for (int gi = g0; gi < g1; ++gi) { const int c = m.pre[gi]; m.pre[gi] = (uint16_t)run; run += c; }
    m.scr[t] = run;
}
// ... and over the runs
JPEG_HD void jpeg_par_stage_add(const JpegParMem& m, int t, int T) {
    int g0, g1;
    jpeg_par_run(m.G, t, T, g0, g1);
    const int before = jpeg_par_before(m.scr, t);
    for (int gi = g0; gi < g1; ++gi) m.pre[gi] = (uint16_t)(m.pre[gi] + before);
}
// the compaction in front of the first marker
JPEG_HD void jpeg_par_stage_write(const JpegParMem& m, int t, int T) {
    const int uend = m.w->marker < m.hi ? m.w->marker : m.hi;
    int top = 0;
    for (int gi = t; gi < m.G; gi += T) {
        uint32_t w[4]; int prev, next;
        jpeg_par_granule(m, gi, w, prev, next);
        const int d = jpeg_par_granule_write(w, prev, 16 * gi, m.lo, uend, m.pre[gi], m.ub, m.cap.u);
        top = d > top ? d : top;
    }
    if (top > 0) jpeg_par_wg_max(&m.w->ulen, top);
}
// (no phase: every lane, or the host once) the image's size is known; false: it does not fit after all
JPEG_HD bool jpeg_par_staged(JpegParMem& m) {
    const int ulen = m.w->ulen;
    m.c.ubw = reinterpret_cast<const uint32_t*>(m.ub); m.c.nw = jpeg_par_words(ulen); m.c.ubits = 8u * (uint32_t)ulen; m.c.huff = m.huff;
    m.c.ncomp = m.S.g.ncomp; m.c.ny = m.S.g.hs * m.S.g.vs; m.c.blocks = m.S.g.blocks;
    m.n_sub = jpeg_par_subs(ulen, m.sub_bytes);
    return m.n_sub <= m.cap.sub && 4 * m.c.nw <= m.cap.u;
}
// the zero words behind the image
JPEG_HD void jpeg_par_stage_fill(const JpegParMem& m, int t, int T) {
    for (int j = (int)(m.c.ubits >> 3) + t; j < 4 * m.c.nw && j < m.cap.u; j += T) m.ub[j] = 0;
}

JPEG_HD uint32_t jpeg_par_sub_end(const JpegParMem& m, int s) {
    const uint32_t e = (uint32_t)(s + 1) * 8u * (uint32_t)m.sub_bytes;
    return e < m.c.ubits ? e : m.c.ubits;
}
// the lenient walk of sub-sequence s from st; true: its exit state is not the one recorded before
JPEG_HD bool jpeg_par_walk_sub(const JpegParMem& m, int s, JpegParState st) {
    m.nbs[s] = (uint16_t)jpeg_par_walk(m.c, st, jpeg_par_sub_end(m, s), false, 8 * m.sub_bytes + 1);
    const uint16_t bk = (uint16_t)((st.b << 8) | st.k);
    const bool changed = st.p != m.ex_p[s] || bk != m.ex_bk[s];
    m.ex_p[s] = st.p; m.ex_bk[s] = bk;
    return changed;
}

// speculate: every sub-sequence from (its first bit, block 0, k = 0); a lane takes several where there are more than lanes
JPEG_HD void jpeg_par_speculate(const JpegParMem& m, int t, int T) {
    for (int s = t; s < m.n_sub; s += T) {
        const JpegParState st = {(uint32_t)s * 8u * (uint32_t)m.sub_bytes, 0, 0};
        m.us_p[s] = st.p; m.us_bk[s] = 0;
        jpeg_par_walk_sub(m, s, st);             // (nothing was recorded before: what it returns means nothing)
    }
}
// exchange, first half of a pass: a sub-sequence whose left neighbour's exit state is not the state it last started from takes it
JPEG_HD void jpeg_par_exchange_take(const JpegParMem& m, int t, int T) {
    if (t == 0) m.w->any = 0;
    for (int s = t; s < m.n_sub; s += T) {
        uint8_t ch = 0;
        if (s > 0) {
            const uint32_t p = m.ex_p[s - 1];
            const uint16_t bk = m.ex_bk[s - 1];
            if (p != m.us_p[s] || bk != m.us_bk[s]) { m.us_p[s] = p; m.us_bk[s] = bk; ch = 1; }
        }
        m.chg[s] = ch;
    }
}
// ... second half: and is walked again from it.  The loop around the two ends when w->any stays 0, after n_sub passes at the latest (pass r
// makes the exit state of sub-sequence r true).
JPEG_HD void jpeg_par_exchange_walk(const JpegParMem& m, int t, int T) {
    bool mine = false;
    for (int s = t; s < m.n_sub; s += T) {
        if (!m.chg[s]) continue;
        const int bk = m.us_bk[s];
        const JpegParState st = {m.us_p[s], bk >> 8, bk & 255};
        mine |= jpeg_par_walk_sub(m, s, st);
    }
    if (mine) jpeg_par_wg_or(&m.w->any);
}

// index: the blocks begun inside a lane's run of sub-sequences (scan) ...
JPEG_HD void jpeg_par_index_sum(const JpegParMem& m, int t, int T) {
    int s0, s1, run = 0;
    jpeg_par_run(m.n_sub, t, T, s0, s1);
    for (int s = s0; s < s1; ++s) run += m.nbs[s];
    m.scr[t] = run;
}
// ... give every sub-sequence its first block (in us_p)
JPEG_HD void jpeg_par_index_first(const JpegParMem& m, int t, int T) {
    int s0, s1;
    jpeg_par_run(m.n_sub, t, T, s0, s1);
    int first = jpeg_par_before(m.scr, t);
    for (int s = s0; s < s1; ++s) { m.us_p[s] = (uint32_t)first; first += m.nbs[s]; }
}
// The strict walk of the blocks that begin in sub-sequence s (the last one carries on over the zero bits past the end until the
// segment's blocks are done): at most nblk blocks of at most 64 symbols.  Records every block's first bit and DC difference; true: a
// block raised a status, and with `record` that block is written down as the segment's first error.
JPEG_HD bool jpeg_par_index_sub(const JpegParMem& m, int s, bool record) {
    JpegParState st = {0u, 0, 0};
    if (s > 0) { const int bk = m.ex_bk[s - 1]; st.p = m.ex_p[s - 1]; st.b = bk >> 8; st.k = bk & 255; }
    int j = (int)(m.us_p[s] < (uint32_t)m.nblk ? m.us_p[s] : (uint32_t)m.nblk);
    if (st.k) jpeg_par_walk(m.c, st, 0u, true, JPEG_PAR_FINISH_ITERS);
    if (st.k) return false;
    const bool last = s == m.n_sub - 1;
    const uint32_t e = jpeg_par_sub_end(m, s);
    while (j < m.nblk && (last || st.p < e)) {
        const uint32_t p0 = st.p;
        int diff;
        const int rc = jpeg_par_block(m.c, st.p, jpeg_par_comp(m.c, j % m.c.blocks), m.zz, nullptr, 0, diff);
        if (rc && !record) return true;
        m.bstart[j] = p0;
        m.bdc[j] = (int16_t)diff;
        if (rc) { m.w->errblock = j; m.w->errst = rc; m.w->errbit = st.p; return true; }
        if (++j == m.nblk) m.w->done = st.p;
    }
    return false;
}
// every sub-sequence; a lane stops at its first error
JPEG_HD void jpeg_par_index_walk(const JpegParMem& m, int t, int T) {
    for (int s = t; s < m.n_sub; s += T)
        if (jpeg_par_index_sub(m, s, false)) { jpeg_par_wg_min(&m.w->errsub, s); break; }
}
// The lowest sub-sequence that raised a status holds the first error of the segment: everything behind it walked from states that mean
// nothing, and what those lanes recorded (possibly for this very block) is never read or is overwritten here, by its lane walking it again.
JPEG_HD void jpeg_par_index_error(const JpegParMem& m, int t, int T) {
    const int s = m.w->errsub;
    if (s != JPEG_PAR_NO_MARKER && s % T == t) jpeg_par_index_sub(m, s, true);
}

// DC: the differences of component comp become its values, the running sum (it wraps at 16 bits like the sequential predictor, so the sums
// are exact).  Inside a lane's run of blocks (scan) ...
JPEG_HD void jpeg_par_dc_sum(const JpegParMem& m, int t, int T, int comp) {
    int j0, j1, run = 0;
    jpeg_par_run(m.nblk, t, T, j0, j1);
    for (int j = j0; j < j1; ++j) run += jpeg_par_comp(m.c, j % m.c.blocks) == comp ? m.bdc[j] : 0;
    m.scr[t] = run;
}
// ... and over the runs
JPEG_HD void jpeg_par_dc_add(const JpegParMem& m, int t, int T, int comp) {
    int j0, j1;
    jpeg_par_run(m.nblk, t, T, j0, j1);
    int sum = jpeg_par_before(m.scr, t);
    for (int j = j0; j < j1; ++j)
        if (jpeg_par_comp(m.c, j % m.c.blocks) == comp) { sum += m.bdc[j]; m.bdc[j] = (int16_t)sum; }
}

// decode, a round of T blocks from block r0: zero coefficients ...
JPEG_HD void jpeg_par_decode_zero(const JpegParMem& m, int t, int T) {
    const uint32_t zero = 0u;
    for (int x = t; x < jpeg_par_coef_count(T) / 2; x += T) __builtin_memcpy(__builtin_assume_aligned(m.coef + 2 * x, 4), &zero, 4);
}
// ... one lane a block from its first bit (blocks after the error stay zero) ...
JPEG_HD void jpeg_par_decode_block(const JpegParMem& m, int t, int T, int r0) {
    const int j = r0 + t;
    if (j >= m.nblk || j > m.w->errblock) return;
    uint32_t p = m.bstart[j];
    int diff;
    jpeg_par_block(m.c, p, jpeg_par_comp(m.c, j % m.c.blocks), m.zz, m.coef + t * JPEG_PAR_COEF_STRIDE, m.bdc[j], diff);
}
// ... then T / 8 blocks a step from block r0 + q0, eight lanes a block (T a multiple of 8): a column each ...
JPEG_HD void jpeg_par_idct_col(const JpegParMem& m, int t, int T, int r0, int q0) {
    const int lb = q0 + (t >> 3), j = r0 + lb;
    if (j >= m.nblk) return;
    const int comp = jpeg_par_comp(m.c, j % m.c.blocks);
    jpeg_idct_col(m.coef + lb * JPEG_PAR_COEF_STRIDE, reinterpret_cast<const uint16_t*>(m.quant) + 64 * comp, t & 7, m.wsp + (t >> 3) * 64);
}
// ... a row each, into the plane: the MCU is one of this segment's, y0 + 8 <= rows, x0 + 8 <= stride (jpeg_block_place), the slot
// 16-byte aligned and x0 a multiple of 8
JPEG_HD void jpeg_par_idct_row(const JpegParMem& m, int t, int T, int r0, int q0) {
    const int j = r0 + q0 + (t >> 3), y = t & 7;
    if (j >= m.nblk) return;
    int comp, y0, x0;
    uint32_t w0, w1;
    jpeg_block_place(m.S.g, m.S.m0 + j / m.c.blocks, j % m.c.blocks, comp, y0, x0);
    jpeg_idct_row(m.wsp + (t >> 3) * 64, y, w0, w1);
    jpeg_store8(m.planes + jpeg_plane_offset(m.S.g, comp, y0 + y, x0), w0, w1);
}

// The status of the segment (one lane): without a marker inside, from the bit position the walk ended at; WITH one (damage), the sequential
// reader's walk is repeated for it.
JPEG_HD int jpeg_par_status(const JpegParMem& m, const uint8_t* stream, long long stream_bytes) {
    if (m.w->marker < m.hi) return jpeg_segment_status(stream, stream_bytes, m.S, m.huff, m.zz);
    return jpeg_par_tail(m.w->errblock < m.nblk ? m.w->errbit : m.w->done, m.c.ubits, m.w->errst) | jpeg_segment_rst(m.S);
}
