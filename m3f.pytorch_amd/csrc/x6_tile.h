// What the split-product GEMM family states once: the operand split, the LDS stores and fragment reads of the 16-k-stage kernels, the product
// order, the tile order, the plain epilogue and the dynamic-LDS launch.  Included by gemm.hip, gemm_x6.hip, gemm_x6d.hip, gemm_x6w.hip,
// gemm_ring.hip and tcn.hip; what stays in those files is what differs between them: tile geometry, load schedule, CONV / C3 / MW epilogues,
// the DMA ring.  (tests/test_fp16x3_model.py is the same split in float64, shared by the emulators.)
#pragma once
#include "common.h"
#include <atomic>

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// ---- the exact operand split, a PAIR of values at a time ----------------------------------------------------------------------------------
// NS = 1, 2, 3: the value is the sum of NS bf16 terms (3: all 24 significant bits).  One v_cvt_pk_bf16_f32 rounds both values (nearest even),
// the two bf16 are widened back with a shift / a mask, one v_pk_add_f32 forms both remainders: 9 VALU instructions per pair for all three
// terms, against ~17 per ELEMENT for a scalar split -- the splitting, not the MFMAs, was what bounded gemm_x6.hip.
// NS = 4, "fp16x3": the operand, scaled by a power of two s that puts its largest magnitude into [2^14, 2^15) (m3t_f16_scale, common.h), is the
// sum of TWO fp16 terms (hi = rn(s x), lo = rn(s x - hi): 22 significant bits wherever lo is a normal number, absolute error <= 2^-25 / s
// below that); the scales leave in the epilogue.  6 VALU instructions per pair (v_pk_mul, v_cvt_pk_f16_f32, 2 v_cvt_f32_f16, v_pk_fma,
// v_cvt_pk_f16_f32).  Every staged image of the library (gemm.hip's split kernels, tcn.hip's transposing split) is this branch.
// o[s] = the pair's term s, packed (first value in the low half).
constexpr int planes_of(int NS) { return NS == 4 ? 2 : NS; }
template <int NS>
__device__ __forceinline__ void split3_pair(f32x2 v, unsigned (&o)[3], float scale = 1.f) {
    if (NS == 4) {
        const f32x2 vs = v * scale;
        const f16x2 h = __builtin_convertvector(vs, f16x2);
        o[0] = __builtin_bit_cast(unsigned, h);
        const f32x2 r1 = vs - __builtin_convertvector(h, f32x2);
        const f16x2 l = __builtin_convertvector(r1, f16x2);
        o[1] = __builtin_bit_cast(unsigned, l);
        return;
    }
    const bf16x2 h = __builtin_convertvector(v, bf16x2);
    o[0] = __builtin_bit_cast(unsigned, h);
    if (NS == 1) return;
    f32x2 hf;
    hf.x = __uint_as_float(o[0] << 16); hf.y = __uint_as_float(o[0] & 0xffff0000u);
    const f32x2 r1 = v - hf;
    const bf16x2 m = __builtin_convertvector(r1, bf16x2);
    o[1] = __builtin_bit_cast(unsigned, m);
    if (NS == 2) return;
    f32x2 mf;
    mf.x = __uint_as_float(o[1] << 16); mf.y = __uint_as_float(o[1] & 0xffff0000u);
    const f32x2 r2 = r1 - mf;
    const bf16x2 l = __builtin_convertvector(r2, bf16x2);
    o[2] = __builtin_bit_cast(unsigned, l);
}
// four consecutive values (v01, v23) as the 16-byte record of a pre-split fp16x3 image: {hi 0|1, hi 2|3, lo 0|1, lo 2|3}
__device__ __forceinline__ float4 f16x3_record(f32x2 v01, f32x2 v23, float sc) {
    unsigned a[3], b[3];
    split3_pair<4>(v01, a, sc);
    split3_pair<4>(v23, b, sc);
    return make_float4(__uint_as_float(a[0]), __uint_as_float(b[0]), __uint_as_float(a[1]), __uint_as_float(b[1]));
}

// ---- LDS stores and fragment reads of the 16-k-stage kernels (gemm_x6d.hip, gemm_x6w.hip; 256 threads) ------------------------------------
// An operand's stage is, per term, two k-octet planes of PL bytes: one 16-B record per (row, k-octet), a fragment one ds_read_b128.
constexpr int X6_STAGE_K = 16;                     // k per stage; a term of a transposed-read image is X6_STAGE_K k-rows

// K-contiguous operand of NR x 64 rows: thread = (k-quad tid & 3, rows (tid >> 2) + 64 i); r[i] = 4 k of row i; PL = the plane's bytes
template <int NS, int NR, int PL>
__device__ __forceinline__ void kc_store_w(unsigned char* __restrict__ S, const f32x4 (&r)[NR], float scale) {
    const int tid = threadIdx.x;
    unsigned char* q = S + ((tid >> 1) & 1) * PL + (tid >> 2) * 16 + (tid & 1) * 8;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
        unsigned lo[3], hi2[3];
        split3_pair<NS>((f32x2){r[i].x, r[i].y}, lo, scale);
        split3_pair<NS>((f32x2){r[i].z, r[i].w}, hi2, scale);
#pragma unroll
        for (int s = 0; s < planes_of(NS); ++s) *reinterpret_cast<u32x2*>(q + s * 2 * PL + i * 1024) = (u32x2){lo[s], hi2[s]};
    }
}
// row-contiguous operand, one 128-row half: wave w holds k-octet w >> 1 of rows 64 (w & 1) ..+63 of the half; lane = (k-pair g = lane >> 4,
// rows 4 (lane & 15) ..+3); r0, r1 = those 4 rows at k = 8 (w >> 1) + 2 g, + 1.  The four lanes 16 apart hold the four k-pairs of the same
// 4 rows: a 4 x 4 transpose across them (v_permlane16_swap, then v_permlane32_swap: 4 per split) leaves lane g with the complete 16-B record
// of row g -- a wave stores 1 KiB contiguous per split.
template <int NS, int PL>
__device__ __forceinline__ void mc_store_w(unsigned char* __restrict__ S, const f32x4& r0, const f32x4& r1, float scale, int half) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned o[4][3];
    split3_pair<NS>((f32x2){r0.x, r1.x}, o[0], scale);
    split3_pair<NS>((f32x2){r0.y, r1.y}, o[1], scale);
    split3_pair<NS>((f32x2){r0.z, r1.z}, o[2], scale);
    split3_pair<NS>((f32x2){r0.w, r1.w}, o[3], scale);
    unsigned char* q = S + (w >> 1) * PL + (half * 128 + (w & 1) * 64 + (lane & 15) * 4 + (lane >> 4)) * 16;
#pragma unroll
    for (int s = 0; s < planes_of(NS); ++s) {
        // X[g][i] = o[i][s] in lane group g.  permlane16_swap(a, b): a.group1 <-> b.group0, a.group3 <-> b.group2;
        // permlane32_swap(a, b): a.groups{2,3} <-> b.groups{0,1}.  After both: (c0, c1, c2, c3) in group g = X[0..3][g].
        const u32x2 p01 = __builtin_amdgcn_permlane16_swap(o[0][s], o[1][s], false, false);
        const u32x2 p23 = __builtin_amdgcn_permlane16_swap(o[2][s], o[3][s], false, false);
        const u32x2 c02 = __builtin_amdgcn_permlane32_swap(p01.x, p23.x, false, false);
        const u32x2 c13 = __builtin_amdgcn_permlane32_swap(p01.y, p23.y, false, false);
        *reinterpret_cast<u32x4*>(q + s * 2 * PL) = (u32x4){c02.x, c13.x, c02.y, c13.y};
    }
}
// TR (NS = 4): a row-contiguous operand lies in LDS as it lies in memory -- per term [k][rows] halves, a k-row every ROW = 2 x rows + 64 B (the
// four k-rows of one transposed read, and the two 16-row blocks of a 32-lane half, cover the 64 banks once).  TR form of mc_store_w (same
// thread map): the four rows' terms at one k are one 8-byte store per term, no cross-lane traffic.
template <int NS, int ROW>
__device__ __forceinline__ void mc_store_wtr(unsigned char* __restrict__ S, const f32x4& r0, const f32x4& r1, float scale, int half) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned char* q = S + (8 * (w >> 1) + 2 * (lane >> 4)) * ROW + (half * 128 + (w & 1) * 64 + (lane & 15) * 4) * 2;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        const f32x4& r = e ? r1 : r0;
        unsigned a[3], b[3];
        split3_pair<NS>((f32x2){r.x, r.y}, a, scale);
        split3_pair<NS>((f32x2){r.z, r.w}, b, scale);
#pragma unroll
        for (int s = 0; s < planes_of(NS); ++s) *reinterpret_cast<u32x2*>(q + s * X6_STAGE_K * ROW + e * ROW) = (u32x2){a[s], b[s]};
    }
}
// the 32x32x16 operand (lane: row lane & 31, k 8 (lane >> 5) ..+7) from a TR image: per 16-lane group a 4 k x 16 row block, lane 4 q + p of the
// group addressing k-row q, rows 4 p ..+3; `at` = this lane's address for the first four k, the next four lie 4 k-rows on -- two
// ds_read_b64_tr_b16.  (EXEC is all ones at every call: the callers sit in uniform control flow.)  The same eight halves in the same order as
// the 16-B record of the permlane path.
template <int ROW>
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* at) {
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(at));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(at + 4 * ROW));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
}

// ---- c + the products of one 32 x 32 x 16 step, smallest first ----------------------------------------------------------------------------
// fa[s][i], fb[s][j] = term s of A's fragment i, B's fragment j.  NS = 3 (bf16x6): (a3,b1) (a2,b2) (a1,b3) (a2,b1) (a1,b2) (a1,b1) -- the six
// whose weight is >= 2^-16; NS = 2 ("high"): (a2,b2) (a2,b1) (a1,b2) (a1,b1); NS = 1: (a1,b1); NS = 4 (fp16x3): lo hi, hi lo, hi hi (exact in
// fp32; the dropped lo lo is <= 2^-22 relative).  gemm_ring.hip issues the NS = 4 order for two A fragments at a time.
template <int NS, int NP, int NI, int NJ>
__device__ __forceinline__ f32x16 x6_mac(f32x16 c, const bf16x8 (&fa)[NP][NI], int i, const bf16x8 (&fb)[NP][NJ], int j) {
    if constexpr (NS == 4) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[1][i]), __builtin_bit_cast(f16x8, fb[0][j]), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[0][i]), __builtin_bit_cast(f16x8, fb[1][j]), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fa[0][i]), __builtin_bit_cast(f16x8, fb[0][j]), c, 0, 0, 0);
        return c;
    }
    if constexpr (NS == 2) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][i], fb[1][j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[1][i], fb[0][j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][i], fb[1][j], c, 0, 0, 0);
    }
    if constexpr (NS == 3) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[NP - 1][i], fb[0][j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[NP / 2][i], fb[NP / 2][j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][i], fb[NP - 1][j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[NP / 2][i], fb[0][j], c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][i], fb[NP / 2][j], c, 0, 0, 0);
    }
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][i], fb[0][j], c, 0, 0, 0);
}

// ---- XCD-contiguous tile order ---------------------------------------------------------------------------------------------------------------
// Workgroups are dealt round-robin over the 8 XCDs (private L2s), so give each XCD a CONTIGUOUS run of tiles (column tile fastest): neighbours
// then share their A row-panel in that XCD's L2.  lin = the workgroup's linear index, nt = the number of tiles; bijective for any tile count;
// placement only affects speed.
__device__ __forceinline__ int m3t_xcd_tile(int lin, int nt) {
    const int xq = nt >> 3, xr = nt & 7, xcd = lin & 7, slot = lin >> 3;
    return xcd * xq + min(xcd, xr) + slot;
}

// ---- the plain epilogue ------------------------------------------------------------------------------------------------------------------------
// v = one accumulator value with the operand scales already taken out, q = its destination, bv = its column's bias (0 unless direct).
// direct: one K pass, q lies in C; else q lies in this split's slab of ws and m3t_sgemm's reduce applies bias / act / accumulate.
__device__ __forceinline__ void x6_plain_out(float v, float* q, float bv, bool direct, int act, int accumulate) {
    if (direct) {
        v += bv;
        if (act == 1) v = m3t_relu(v);
        if (accumulate) v += *q;
    }
    *q = v;
}

// ---- host: launch a kernel that needs more dynamic LDS than the default limit -------------------------------------------------------------
// The limit is raised once per (kernel, device) -- one bit per device and kernel instantiation, not one flag per process -- then the launch.
// Returns 0, M3T_EINVAL (no current device, or its index past the 32 bits) or the attribute call's error; launch errors are the caller's
// hipGetLastError.
template <auto KERNEL, class P>
inline int x6_launch_dyn_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const P& p) {
    static std::atomic<unsigned> attr_set{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 32) return M3T_EINVAL;
    if (!(attr_set.load(std::memory_order_relaxed) & (1u << dev))) {
        hipError_t ea = hipFuncSetAttribute((const void*)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ea != hipSuccess) return (int)ea;
        attr_set.fetch_or(1u << dev, std::memory_order_relaxed);
    }
    KERNEL<<<grid, block, lds, s>>>(p);
    return 0;
}

}  // namespace
