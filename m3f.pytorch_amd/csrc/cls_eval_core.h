// The ranking rules of csrc/cls_eval.hip as one text for the device and the host: the sort key, one bitonic compare-exchange step, the
// two workgroup scans and the walk over a sorted column that yields AP and the ROC-AUC numerator per tie group.  Every function is the work
// of ONE thread `tid` of `nt` between two workgroup barriers; the kernel puts __syncthreads() between the calls, csrc/cls_eval_host_check.cpp
// a loop over tid.  No function here touches anything but its arguments.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CLS_HD __host__ __device__ __forceinline__
#else
#define CLS_HD inline
#endif

// A float's bits -> a 32-bit key whose unsigned order is the order of the VALUES: -0.0 and +0.0 give one key, a denormal keeps its own
// (nothing is flushed), -inf < every finite number < +inf.  NaN patterns land above +inf / below -inf; a column that holds one is
// poisoned by m3t_cls_eval_append's counter and only has to sort without a fault.
CLS_HD uint32_t cls_key(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
// What is sorted: key << 8 | 0x80 | label.  All 32 bits of the key stay; the label rides BELOW it, so it orders rows inside a tie
// group (which the walk never looks at) and cannot split one: groups are runs of equal `item >> 8`.  0 = padding, below every row.
CLS_HD uint64_t cls_item(uint32_t bits, unsigned label) { return ((uint64_t)cls_key(bits) << 8) | 0x80u | (uint64_t)(label & 1u); }
CLS_HD uint64_t cls_group(uint64_t item) { return item >> 8; }

CLS_HD unsigned cls_floor_pow2(unsigned v) {
    unsigned p = 1;
    while (p <= v / 2) p *= 2;
    return p;
}
CLS_HD unsigned long long cls_ceil_pow2(unsigned long long v) {
    unsigned long long p = 1;
    while (p < v) p *= 2;
    return p;
}

// One step (k, j) of the bitonic network on a[0 .. n), n a power of two, whose element i is element g0 + i of the whole sequence
// (g0 a multiple of n): pairs (i, i + j) with bit j of i clear, DESCENDING where bit k of the global index is clear -- the last
// stage (k = the whole length) is descending throughout.  Thread tid takes pairs tid, tid + nt, ...
template <class Ptr>
CLS_HD void cls_bitonic_step(Ptr a, unsigned n, unsigned g0, unsigned k, unsigned j, unsigned tid, unsigned nt) {
    for (unsigned p = tid; p < n / 2; p += nt) {
        const unsigned i = 2 * p - (p & (j - 1)), l = i + j;
        const bool desc = ((g0 + i) & k) == 0;
        const uint64_t x = a[i], y = a[l];
        if (desc ? x < y : x > y) {
            a[i] = y;
            a[l] = x;
        }
    }
}

// Thread tid owns the rows [lo, hi) of the sorted column: nt contiguous chunks of ceil(M / nt) rows.
CLS_HD void cls_chunk(unsigned M, unsigned tid, unsigned nt, unsigned& lo, unsigned& hi) {
    const unsigned per = (M + nt - 1) / nt;
    lo = tid * per < M ? tid * per : M;
    hi = lo + per < M ? lo + per : M;
}

// Row i opens a tie group iff i == 0 or its key differs from row i - 1's.  Over its chunk a thread counts the positives (cnt) and
// remembers its LAST opening row: its index (open_idx, or ~0u for none) and the positives of the chunk in front of it (open_cnt).
template <class Ptr>
CLS_HD void cls_walk_count(Ptr a, unsigned M, unsigned tid, unsigned nt, unsigned& cnt, unsigned& open_idx, unsigned& open_cnt) {
    unsigned lo, hi;
    cls_chunk(M, tid, nt, lo, hi);
    cnt = 0;
    open_idx = ~0u;
    open_cnt = 0;
    for (unsigned i = lo; i < hi; ++i) {
        const uint64_t x = a[i];
        if (i == 0 || cls_group(a[i - 1]) != cls_group(x)) {
            open_idx = i;
            open_cnt = cnt;
        }
        cnt += (unsigned)(x & 1u);
    }
}
// (opening row + 1) << 32 | positives in front of it: both grow along the column, so the group that is open where a chunk begins is the
// MAXIMUM of this word over the threads in front (0: none).
CLS_HD uint64_t cls_open_word(unsigned open_idx, unsigned open_cnt, unsigned base) {
    return open_idx == ~0u ? 0ull : ((uint64_t)(open_idx + 1u) << 32) | (uint64_t)(base + open_cnt);
}

// One step of an inclusive Hillis-Steele scan over nt words: dst[tid] = src[tid] (+ or max) src[tid - d].
CLS_HD void cls_scan_step(const uint64_t* src, uint64_t* dst, unsigned d, unsigned tid, bool take_max) {
    uint64_t v = src[tid];
    if (tid >= d) {
        const uint64_t w = src[tid - d];
        v = take_max ? (w > v ? w : v) : v + w;
    }
    dst[tid] = v;
}

// The walk.  base = positives in front of the chunk, carry = the open word of the group that is open where the chunk begins.  For
// every group that ENDS in the chunk (row i is the last row or row i + 1 has another key), with TP, FP the counts after the group
// and dTP, dFP its own: ap += dTP TP / (TP + FP) -- one correctly rounded float64 division of two exact integers per group with a
// positive, added in row order -- and num += dFP (2 TP_before + dTP), a 64-bit integer: 2 P N AUC.
template <class Ptr>
CLS_HD void cls_walk_score(Ptr a, unsigned M, unsigned tid, unsigned nt, unsigned base, uint64_t carry, double& ap, uint64_t& num) {
    unsigned lo, hi;
    cls_chunk(M, tid, nt, lo, hi);
    unsigned g_idx = carry ? (unsigned)(carry >> 32) - 1u : 0u, g_tp = (unsigned)(carry & 0xffffffffu), tp = base;
    ap = 0.0;
    num = 0;
    for (unsigned i = lo; i < hi; ++i) {
        const uint64_t x = a[i];
        if (i == 0 || cls_group(a[i - 1]) != cls_group(x)) {
            g_idx = i;
            g_tp = tp;
        }
        tp += (unsigned)(x & 1u);
        if (i + 1 == M || cls_group(a[i + 1]) != cls_group(x)) {
            const uint64_t n = (uint64_t)i + 1u, dtp = tp - g_tp, dfp = (n - g_idx) - dtp;
            if (dtp) ap += (double)(dtp * (uint64_t)tp) / (double)n;
            num += dfp * ((uint64_t)g_tp + (uint64_t)tp);
        }
    }
}
