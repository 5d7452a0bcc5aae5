// Persistent BiGRU scans for gfx950: ONE launch runs all T steps of a level.
//
// Why: in the launch-per-step structure (gru.hip) every step re-reads the workgroup's W_hh slice (96 KB at H = 512)
// through a cold L2 and pays the kernel boundary; measured 6.1 / 6.9 us per step (fwd / bwd) at H = 512.  Here a
// workgroup keeps its W_hh fragments in REGISTERS for the whole scan (48 VGPRs per lane) and only h_t (fwd) or
// dgh_t (bwd) crosses CUs each step.
//
// The exchange (measured alone in tools/persist_probe.hip: 2.0-2.1 us per step for 32 producers -> 32 consumers,
// 64-128 KB gathered per workgroup, no torn granule in 4e10): no grid barrier and no flags.  Every value travels in a
// tagged granule written by ONE naturally aligned agent-scope (sc1, write-through) store and read by agent-scope
// loads:  forward  8 B  {h, tag};   backward 16 B {dr, dz, dn*r, tag};   tag = step + 1, two slots ping-pong by step
// parity (a producer can only overwrite slot p after every consumer of its group has finished reading it, because its
// own next step needs all of their next granules).  A consumer simply re-reads its granules until all tags match.
// Correctness never depends on placement; speed does a little: a group (one scan x one 16-row block, all unit
// blocks) is mapped to blockIdx % G so that it sits on one XCD when G is a multiple of 8.
//
// Residency: every workgroup of the grid must be resident at once (the kernel is launched only when the grid fits the
// CUs at the occupancy HIP reports, and never concurrently with another persistent scan: m3t.ops keeps them on the
// main stream).  Every spin is bounded; a workgroup that gives up raises a sticky host-visible error word and the
// scan finishes with garbage, which the next scan call reports as M3T_ESPIN.
//
// Arithmetic: the same fp32 MFMA 16x16x4 chain, k order, LDS reduction order and gate math as the per-step kernels,
// so results are bit-identical to them (tests assert equality).
#include "gru_common.h"
#include "gru_persist_step.h"      // the exchange state and everything the kernels below share
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <fcntl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

namespace m3t_gru {

namespace {

constexpr int SPIN_LIMIT_DEFAULT = 1 << 21;     // gather attempts (~1 us each) before a workgroup gives up; env M3T_SCAN_SPIN_LIMIT

// ------------------------------------------------------------------------------------------------ forward
template <int NC, int RT>      // NC = H / 128 = k-chunks per wave;  RT = 16-row tiles per workgroup
__global__ __launch_bounds__(NT) void gru_persist_fwd_kernel(FwdGroup g, FragPtrs fp, ExPtrs ex, int B, int T, int G, int nrb,
                                                             unsigned* err) {
    constexpr int ROWS = 16 * RT;
    constexpr int NB = RT == 1 ? 2 : 1;                // RT = 1: double-buffered by step parity, one barrier per step
    constexpr int H = 128 * NC, nch = H >> 4;
    __shared__ float red[NB][NW][3][ROWS][UB + 1];     // 51 KiB either way (static LDS limit 64 KiB); +1: conflict-free reads
    M3T_PERSIST_WHO(ub);
    const m3t_gru_fwd_desc d = g.d[s];
    const int j0 = ub * UB, r0 = rb * ROWS;

    // this workgroup's W_hh fragments stay in registers for all T steps
    float4 wf[NC][3];
    {
        const float4* Wf = reinterpret_cast<const float4*>(fp.wfrag[s] + (size_t)ub * nch * 3 * 256);
#pragma unroll
        for (int m = 0; m < NC; ++m)
#pragma unroll
            for (int ct = 0; ct < 3; ++ct) wf[m][ct] = Wf[((size_t)(wave + m * NW) * 3 + ct) * 64 + lane];     // already bf16-rounded by the prep kernel in M3T_BF16 mode
    }
    // gate-math threads, one (row, unit) each, numbered in GRANULE order: thread i owns granule i of the workgroup's
    // tile, so a wave publishes 64 consecutive granules = whole 128-B lines.  (A wave publishing 16 separate 32-B
    // pieces -- the (row, unit) numbering of the per-step kernels -- doubles the exchange time: write-through partial
    // lines, tools/persist_probe.hip.)  granule (rt*4 + e)*64 + l  <->  row rt*16 + (l & 15), unit 4*(l >> 4) + e
    const bool pw = tid < ROWS * UB;
    const int prow = (tid >> 8) * 16 + (tid & 15), pu = ((tid >> 4) & 3) * 4 + ((tid >> 6) & 3);
    const int pb = r0 + prow, pj = j0 + pu;
    const bool pok = pw && pb < B;
    float br = 0.f, bz = 0.f, bn = 0.f, hprev = 0.f;
    if (pw) { br = d.b_hh[pj]; bz = d.b_hh[H + pj]; bn = d.b_hh[2 * H + pj]; }

    constexpr size_t TILE = (size_t)RT * 256;          // granules one workgroup publishes per step
    unsigned long long* gran = reinterpret_cast<unsigned long long*>(ex.gran[s]);
    const size_t slot = ex.slot[s];
    const size_t grp = (size_t)rb * nch * TILE;
    const size_t pub = grp + (size_t)ub * TILE + tid;
    M3T_PERSIST_POLL_STATE(ub, H >> 4);
    M3T_STAMP_STATE();

    float xrA, xzA, xnA, xrB, xzB, xnB;                // the x-projection's two register sets (M3T_FWD_LOAD_X)
    const float* xq = d.xproj + (size_t)(pb < B ? pb : B - 1) * T * d.ldx + d.xoff + pj;
    M3T_FWD_LOAD_X_FIRST();

#define M3T_STEP_FILE "gru_persist_fwd_step.inc"
#include "gru_persist_ab.inc"
    scan_drain();
    M3T_STAMP_DUMP();
}

// ------------------------------------------------------------------------------------------------ forward, bf16x6
// The recurrent product of the forward scan on the bf16 matrix pipe, still fp32-accurate: h and W_hh are each split
// exactly into three bf16 terms and a product is the six MFMAs of weight >= 2^-16 (as the GEMM, gemm_x6.hip).  Why
// here: at H = 512 the 48 fp32 MFMAs of a wave (two waves share a SIMD) were ~1.5 us of a ~4.5 us step; the 36
// v_mfma_f32_16x16x32_bf16 that replace them cost a third of that.  The split of h is done ONCE by the producer: a
// granule is {h1, h2, h3, tag} (3 x bf16 + a 16-bit tag in 8 bytes), so the consumer only re-pairs 16-bit halves
// (v_perm_b32) into MFMA operands; W_hh is split by the prep kernel into the B-operand order and lives in 72 VGPRs.
// Per wave: chunks c = wave + 8m; MFMA k-step s uses chunks m = 2s (k-groups 0,1) and 2s+1 (k-groups 2,3), lane
// (row = lane & 15, q = lane >> 4) holding units 8(q&1) .. +7 of its chunk.  Granule i of a workgroup's tile:
// jp = i >> 6, hr = (i >> 1) & 31, jlo = i & 1  <->  row hr & 15, unit 8*(hr >> 4) + 2*jp + jlo: one 16-byte load takes
// the granules of two adjacent units, and a wave instruction reads 512 contiguous bytes from each of two producers.  Only the backward scan needs the launch-per-step kernels' bit pattern; results here
// agree with them to fp32 rounding (~1e-6), not bit for bit (M3T_SCAN_FP32 forces the fp32-MFMA kernel).
typedef __bf16 pbf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned pu32x4 __attribute__((ext_vector_type(4)));

// wfrag6[ub][wave][s][ct][t][lane][8 bf16]: split t of W_hh[ct*H + ub*16 + (lane&15)][unit(wave, s, lane>>4, e)]
__global__ void wfrag6_prep_kernel(const float* __restrict__ w_hh, unsigned short* __restrict__ wf, int H, int bf16) {
    const int nch = H >> 4, ks = nch >> 4;            // ks = k-steps per wave = NC / 2
    const size_t total = (size_t)3 * H * H;           // one thread per weight: writes its three terms
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = i & 7, l = (i >> 3) & 63;
        size_t r = i >> 9;
        const int ct = r % 3; r /= 3;
        const int s = r % ks; r /= ks;
        const int w = r % NW, ub = r / NW;
        const int q = l >> 4;
        const int unit = 16 * (w + NW * (2 * s + (q >> 1))) + 8 * (q & 1) + e;
        float x = w_hh[((size_t)ct * H + ub * 16 + (l & 15)) * H + unit];
        if (bf16) x = rbf(x);                         // mixed-precision mode: the operand IS its first term, the other two are zero
        const __bf16 b1 = (__bf16)x;
        const float r1 = x - (float)b1;
        const __bf16 b2 = (__bf16)r1;
        const __bf16 b3 = (__bf16)(r1 - (float)b2);
        const size_t base = ((((size_t)(ub * NW + w) * ks + s) * 3 + ct) * 3) * 512 + (size_t)l * 8 + e;
        wf[base] = __builtin_bit_cast(unsigned short, b1);
        wf[base + 512] = __builtin_bit_cast(unsigned short, b2);
        wf[base + 1024] = __builtin_bit_cast(unsigned short, b3);
    }
}

// fp16x3 form of the forward recurrent product (M3T_GEMM_F16X3, DESIGN.md section 7 / NOTEBOOK.md section 5e): h_t is bounded by 1, so the producers publish it
// as two fp16 terms of 2^14 h; W_hh is split into two fp16 terms per workgroup slice (the 48 gate rows of 16 hidden units), scaled by the
// power of two that puts the slice's largest magnitude into [2^14, 2^15) -- one block per slice measures it and writes
// wfrag3h[ub][wave][s][ct][t < 2][lane][8 fp16] plus inv[ub] = 2^-14 / scale, by which the slice's workgroups unscale their sums.
struct Prep3hArgs { const float* w_hh[M3T_MAX_SCANS]; unsigned short* wf[M3T_MAX_SCANS]; float* inv[M3T_MAX_SCANS]; };
// grid (H / 16 slices, PREP3H_SPLIT, scans): every block of a slice measures the whole slice (48 rows x H values: float4 loads, four
// in flight per thread, L2) and writes its share of the fragments
constexpr int PREP3H_SPLIT = 8;
__global__ __launch_bounds__(256) void wfrag3h_prep_kernel(Prep3hArgs a, int H) {
    const float* __restrict__ w_hh = a.w_hh[blockIdx.z];
    unsigned short* __restrict__ wf = a.wf[blockIdx.z];
    const int ub = blockIdx.x, nch = H >> 4, ks = nch >> 4;
    __shared__ float red[4];
    float m = 0.f;
    const int h4 = H >> 2, tot4 = 48 * h4;
    auto ld = [&](int i) {
        const int rr = i / h4, c = i - rr * h4;
        return *reinterpret_cast<const float4*>(w_hh + ((size_t)(rr >> 4) * H + ub * 16 + (rr & 15)) * H + 4 * c);
    };
    auto fold = [&](const float4& v) {
        m = fmaxf(fmaxf(m, m3t_fin_abs(v.x)), fmaxf(m3t_fin_abs(v.y), fmaxf(m3t_fin_abs(v.z), m3t_fin_abs(v.w))));
    };
    int i = threadIdx.x;
    for (; i + 768 < tot4; i += 1024) {
        const float4 v0 = ld(i), v1 = ld(i + 256), v2 = ld(i + 512), v3 = ld(i + 768);
        fold(v0); fold(v1); fold(v2); fold(v3);
    }
    for (; i < tot4; i += 256) fold(ld(i));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sc, inv;
    m3t_f16_scale(__float_as_uint(m), sc, inv);
    if (threadIdx.x == 0 && blockIdx.y == 0) a.inv[blockIdx.z][ub] = inv * 6.103515625e-05f;       // x 2^-14: the scale of h
    const int per = 3 * 16 * H;                       // weights of this slice, one thread each: [wave][s][ct][lane][8]
    for (int j = blockIdx.y * 256 + threadIdx.x; j < per; j += 256 * PREP3H_SPLIT) {
        const int e = j & 7, l = (j >> 3) & 63;
        int r = j >> 9;
        const int ct = r % 3; r /= 3;
        const int s = r % ks; const int w = r / ks;
        const int q = l >> 4;
        const int unit = 16 * (w + NW * (2 * s + (q >> 1))) + 8 * (q & 1) + e;
        const float x = w_hh[((size_t)ct * H + ub * 16 + (l & 15)) * H + unit] * sc;
        const _Float16 h1 = (_Float16)x;
        const _Float16 h2 = (_Float16)(x - (float)h1);
        const size_t base = ((((size_t)(ub * NW + w) * ks + s) * 3 + ct) * 2) * 512 + (size_t)l * 8 + e;
        wf[base] = __builtin_bit_cast(unsigned short, h1);
        wf[base + 512] = __builtin_bit_cast(unsigned short, h2);
    }
}
typedef _Float16 pf16x8 __attribute__((ext_vector_type(8)));

// UW = 16-unit tiles per workgroup.  UW = 2 (round 4, "wide" workgroups): one workgroup owns 16 rows x 32 units -- the same gather per
// workgroup (h_{t-1} of its 16 rows: the A operand is shared by both unit tiles), twice the W_hh fragments, MFMAs and cells, all eight
// waves do cell math (waves 0-3 tile 0, waves 4-7 tile 1; the two tiles are adjacent in the exchange buffer, so the consumers' gather
// code does not change) -- and a level needs HALF the workgroups: the 4 x H=512 encoder level runs on 128 CUs and leaves room for
// the audio stack's 64-workgroup scans beside it.
// CO (the wide form only): the cell threads' HBM traffic goes through threads numbered in MEMORY order -- thread ti of a tile loads / stores
// the activations of cell (row ti >> 4, unit ti & 15), so a wave instruction covers 4 rows x 16 consecutive units (64-byte / 256-byte
// runs) instead of 64 scattered sectors -- and LDS carries them to / from the cell-math threads (granule order), results one step late.
// In granule order every load and store of a step was 64 separate memory requests per wave: with eight cell-math waves per CU 2500-4600
// requests per CU and step against 500-1000 lines for the gather itself, and the younger waves' stores queued for 1.4 us of a 5.2 us
// wide backward step (wide forward 2.95 -> 2.51 us per step, wide backward 5.2 -> 3.4; with four cell-math waves -- the narrow form --
// the extra LDS hop on the chain costs more than it saves: 3.42 vs 3.30).
// RB (M3T_SCAN_SPREAD): clips per row block.  RB = 8: a workgroup serves rows 0..7 of its 16-row tiles (the granules of rows 0-7 and 8-15 of
// a unit pair are separate 128-byte lines: half the bytes) -- and because the exchange is priced per load INSTRUCTION, not per byte (masking the
// lanes of rows 8-15 alone gained nothing: NOTEBOOK.md R13), the lanes those rows would have used load the odd unit pairs of rows 0-7 instead:
// half the load instructions, one DPP rotate per odd pair behind the wait.  Operand rows 8-15 then hold whatever the rotate left there.  That
// cannot reach a result: row i of an MFMA's output depends on row i of its A operand only, and cells of rows >= RB are never published,
// stored or handed over (plive / pok / hok below).
template <int NC, bool F16 = false, int UW = 1, int RB = 16>
__global__ __launch_bounds__(NT) void gru_persist_fwd6_kernel(FwdGroup g, FragPtrs fp, ExPtrs ex, int B, int T, int G, int nrb,
                                                              unsigned* err) {
    constexpr bool CO = UW == 2;
    constexpr int ROWS = 16, KS = NC / 2, NTERM = F16 ? 2 : 3;
    static_assert(RB == 16 || (RB == 8 && F16), "row blocks: 16 clips, or 8 in the fp16x3 form (the gather deals the units over lane bit 3 for 8 rows)");
    constexpr int H = 128 * NC, nch = H >> 4;
    // partial sums of the waves: [step parity][wave][unit tile][gate][row][UB + 1]; UW = 2 needs 102 KiB: dynamic LDS
    constexpr int RED_FLOATS = 2 * NW * UW * 3 * ROWS * (UB + 1);
    __shared__ float red_s[UW == 1 ? RED_FLOATS : 1];
    extern __shared__ __attribute__((aligned(16))) float red_d[];
    float* const red = UW == 1 ? red_s : red_d;
#define M3T_RED(par_, w_, u_, ct_, r_, c_) red[(((((par_) * NW + (w_)) * UW + (u_)) * 3 + (ct_)) * ROWS + (r_)) * (UB + 1) + (c_)]
    M3T_PERSIST_WHO(ubw);
    const m3t_gru_fwd_desc d = g.d[s];
    const int tu = UW == 1 ? 0 : (tid >> 8);           // the unit tile this thread does cell math for
    const int ub = ubw * UW + tu;
    const int j0 = ub * UB, r0 = rb * RB;

    pbf16x8 wf[UW][KS][3][NTERM];                      // [unit tile][k-step][gate tile][term] (F16: fp16 bit patterns, two terms)
    float winv = 1.f;
    if (F16 && ex.inline_prep) {
        // Round 4: the fp16x3 fragments straight from W_hh, in the kernel (was wfrag3h_prep_kernel: one more launch on the chain in front
        // of every scan).  Lane (n = lane & 15, q = lane >> 4) of wave w holds, per (k-step, gate tile), the 8 consecutive k
        // 16 (w + NW (2k + (q >> 1))) + 8 (q & 1) + e of row ct H + 16 ub + n: two float4 loads.  Pass 1: the maximum of each 16-unit
        // slice (its 48 rows x H values are read exactly once by the workgroup) -> the slice's power-of-two scale; pass 2: the same
        // loads again (L2-hot), scaled and split into two fp16 terms.  Same values as the prep kernel's.
        __shared__ float s_wmax[2][NW];
        const int q_ = lane >> 4;
        float mx[UW];
#pragma unroll
        for (int u = 0; u < UW; ++u) {
            mx[u] = 0.f;
#pragma unroll
            for (int k = 0; k < KS; ++k)
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) {
                    const float4* wp = reinterpret_cast<const float4*>(d.w_hh + ((size_t)ct * H + (ubw * UW + u) * 16 + (lane & 15)) * H +
                                                                       16 * (wave + NW * (2 * k + (q_ >> 1))) + 8 * (q_ & 1));
                    const float4 a = wp[0], b = wp[1];
                    mx[u] = fmaxf(fmaxf(fmaxf(mx[u], m3t_fin_abs(a.x)), fmaxf(m3t_fin_abs(a.y), m3t_fin_abs(a.z))),
                                  fmaxf(fmaxf(m3t_fin_abs(a.w), m3t_fin_abs(b.x)), fmaxf(m3t_fin_abs(b.y), fmaxf(m3t_fin_abs(b.z), m3t_fin_abs(b.w)))));
                }
            mx[u] = wave_max(mx[u]);
            if (lane == 0) s_wmax[u][wave] = mx[u];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < UW; ++u) {
            float m = 0.f;
#pragma unroll
            for (int w = 0; w < NW; ++w) m = fmaxf(m, s_wmax[u][w]);
            float sc, inv;
            m3t_f16_scale(__float_as_uint(m), sc, inv);
            if (u == tu) winv = inv * 6.103515625e-05f;         // x 2^-14: the scale of h
#pragma unroll
            for (int k = 0; k < KS; ++k)
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) {
                    const float4* wp = reinterpret_cast<const float4*>(d.w_hh + ((size_t)ct * H + (ubw * UW + u) * 16 + (lane & 15)) * H +
                                                                       16 * (wave + NW * (2 * k + (q_ >> 1))) + 8 * (q_ & 1));
                    const float4 a = wp[0], b = wp[1];
                    const float xv[8] = {a.x * sc, a.y * sc, a.z * sc, a.w * sc, b.x * sc, b.y * sc, b.z * sc, b.w * sc};
                    pf16x8 h1, h2;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        h1[e] = (_Float16)xv[e];
                        h2[e] = (_Float16)(xv[e] - (float)h1[e]);
                    }
                    wf[u][k][ct][0] = __builtin_bit_cast(pbf16x8, h1);
                    wf[u][k][ct][1] = __builtin_bit_cast(pbf16x8, h2);
                }
        }
    } else {
#pragma unroll
        for (int u = 0; u < UW; ++u) {
            const pu32x4* Wf = reinterpret_cast<const pu32x4*>(fp.wfrag[s]) + ((size_t)((ubw * UW + u) * NW + wave) * KS * 3 * NTERM) * 64 + lane;
#pragma unroll
            for (int k = 0; k < KS; ++k)
#pragma unroll
                for (int ct = 0; ct < 3; ++ct)
#pragma unroll
                    for (int t = 0; t < NTERM; ++t) wf[u][k][ct][t] = __builtin_bit_cast(pbf16x8, Wf[((k * 3 + ct) * NTERM + t) * 64]);
        }
        // F16: 2^-14 / (scale of this slice's W_hh), written by wfrag3h_prep_kernel behind the fragments
        if (F16) winv = reinterpret_cast<const float*>(fp.wfrag[s])[(size_t)4 * H * H + ub];
    }
    // cell-math threads in granule order (see the header): granule ti = jp*64 + hr*2 + jlo  <->  row hr & 15,
    // unit 8*(hr >> 4) + 2*jp + jlo
    const int ti = tid & 255;
    const bool pw = tid < ROWS * UB * UW;
    const int prow = (ti >> 1) & 15, pu = ((ti >> 5) & 1) * 8 + 2 * ((ti >> 6) & 3) + (ti & 1);
    const int pb = r0 + prow, pj = j0 + pu;
    const bool plive = pw && prow < RB;                // publishes: live rows past the batch carry zeros (their consumers check every live row's tag)
    const bool pok = plive && pb < B;
    float br = 0.f, bz = 0.f, bn = 0.f, hprev = 0.f;
    if (pw) { br = d.b_hh[pj]; bz = d.b_hh[H + pj]; bn = d.b_hh[2 * H + pj]; }

    constexpr size_t TILE = 256;
    unsigned long long* gran = reinterpret_cast<unsigned long long*>(ex.gran[s]);
    const size_t slot = ex.slot[s];
    const size_t grp = (size_t)rb * nch * TILE;
    const size_t pub = grp + (size_t)ubw * UW * TILE + tid;
    // this lane's gather base inside a producer tile: chunk m = 2s + (q >> 1); granule pair 2*hr + 64 jp, hr = (q&1)*16 + row
    const int q = lane >> 4;
    // (RB = 8: row lane & 7, and lane bit 3 picks the odd unit pair jp, 64 granules on)
    const size_t lane_off = RB < ROWS ? (size_t)(wave + NW * (q >> 1)) * TILE + 2 * ((q & 1) * 16 + (lane & 7)) + 64 * ((lane >> 3) & 1)
                                      : (size_t)(wave + NW * (q >> 1)) * TILE + 2 * ((q & 1) * 16 + (lane & 15));
    M3T_PERSIST_POLL_STATE(ubw, (H >> 4) / UW);
    M3T_STAMP_STATE();

    const bool MARK_ASC = !d.reverse;
    M3T_MARK_STATE();
    float xrA, xzA, xnA, xrB, xzB, xnB;                // the x-projection's two register sets (M3T_FWD_LOAD_X)
    // memory-side identity of this thread (CO; else = its cell) and the LDS slots of the hand-over, padded one per 16
    const int hrow = CO ? (ti >> 4) : prow, hun = CO ? (ti & 15) : pu;
    const int hb = r0 + hrow, hj = j0 + hun;
    const bool hok = pw && hrow < RB && hb < B;
    const int hg = 64 * ((hun >> 1) & 3) + 2 * (hrow + 16 * (hun >> 3)) + (hun & 1);      // granule index of cell (hrow, hun)
    constexpr int SLOTS = 272;
    const int slot_h = tu * SLOTS + hg + (hg >> 4), slot_c = tu * SLOTS + ti + (ti >> 4);
    f32x4* const sx = reinterpret_cast<f32x4*>(red_d + (UW == 1 ? 0 : RED_FLOATS));      // [parity][UW][SLOTS] (xr, xz, xn, -) of the step
    f32x4* const so = sx + 2 * UW * SLOTS;                                                // [parity][UW][SLOTS] (r, z, n, W_hn h + b_hn)
    float* const sh = reinterpret_cast<float*>(so + 2 * UW * SLOTS);                      // [parity][UW][SLOTS] h_t
    const float* xq = d.xproj + (size_t)(hb < B ? hb : B - 1) * T * d.ldx + d.xoff + hj;
    auto store_results = [&](int step_of, const f32x4& g4, float hv) {      // (CO: the memory-order thread, one step late)
        const int t_ = d.reverse ? T - 1 - step_of : step_of;
        M3T_FWD_STORE_RESULTS(hb, hj, t_, step_of == T - 1, f32x4, g4, hv);
    };
    M3T_FWD_LOAD_X_FIRST();

#define M3T_STEP_FILE "gru_persist_fwd6_step.inc"
#include "gru_persist_ab.inc"
#undef M3T_RED
    scan_drain();
    if (CO) {                                          // the last step's results are still in LDS
        __syncthreads();
        if (hok) store_results(T - 1, so[((T - 1) & 1) * UW * SLOTS + slot_h], sh[((T - 1) & 1) * UW * SLOTS + slot_h]);
    }
    M3T_STAMP_DUMP();
}

// ------------------------------------------------------------------------------------------------ backward, bf16 mode
// M3T_BF16: every operand of the recurrent product is bf16 by definition of the mode, so the exchange shrinks to the
// forward scan's -- an 8-byte granule {bf16 dr, bf16 dz, bf16 dn*r, tag16} in the forward kernel's tile order, 8 instead of
// 16 gather loads per lane -- and the product runs on the bf16 matrix pipe: per k-step of 32 units three
// v_mfma_f32_16x16x32_bf16 (one per gate; 6 per wave at H = 512 instead of 48 fp32 MFMAs), fp32 accumulate.  Same values
// as the fp32-MFMA kernel on rounded operands up to accumulation order (M3T_SCAN_FP32 keeps that kernel and bit-identity
// with the launch-per-step path).  Everything else -- cell math, bias sums, prefetch, poll delay -- is the kernel below.
__global__ void wfrag_bwd16_prep_kernel(const float* __restrict__ w_hh_t, unsigned short* __restrict__ wf, int H, int direct) {
    const int ks = H >> 8;                            // k-steps per wave = NC / 2
    const size_t total = (size_t)3 * H * H;           // [ub][wave][k-step][gate][lane][8]
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = i & 7, l = (i >> 3) & 63;
        size_t r = i >> 9;
        const int gt = r % 3; r /= 3;
        const int sk = r % ks; r /= ks;
        const int w = r % NW, ub = r / NW;
        const int q = l >> 4;
        const int unit = 16 * (w + NW * (2 * sk + (q >> 1))) + 8 * (q & 1) + e;       // the forward kernel's k order
        // direct: the pointer is the untransposed parameter w_hh [3H][H] (M3T_SCAN_WHH)
        const float x = rbf(direct ? w_hh_t[((size_t)gt * H + unit) * H + ub * 16 + (l & 15)]
                                   : w_hh_t[((size_t)ub * 16 + (l & 15)) * 3 * H + (size_t)gt * H + unit]);
        wf[i] = (unsigned short)(__float_as_uint(x) >> 16);
    }
}

template <int NC>
__global__ __launch_bounds__(NT) void gru_persist_bwd16_kernel(BwdGroup g, FragPtrs fp, ExPtrs ex, int B, int T, int G, int nrb,
                                                             unsigned* err) {
    constexpr int ROWS = 16, RT = 1, KS = NC / 2;
    constexpr int H = 128 * NC, H3 = 3 * H, nchh = H >> 4;
    __shared__ float red[2][NW][ROWS][UB + 1];
    M3T_PERSIST_WHO(ub);
    const m3t_gru_bwd_desc d = g.d[s];
    const int j0 = ub * UB, r0 = rb * ROWS;

    pbf16x8 wb[KS][3];                                 // [k-step][gate]: W_hh rows (gate, 32 units of the k-step) x this workgroup's 16 units
    {
        const pu32x4* Wf = reinterpret_cast<const pu32x4*>(fp.wfrag[s]) + ((size_t)(ub * NW + wave) * KS * 3) * 64 + lane;
#pragma unroll
        for (int k = 0; k < KS; ++k)
#pragma unroll
            for (int gt = 0; gt < 3; ++gt) wb[k][gt] = __builtin_bit_cast(pbf16x8, Wf[(k * 3 + gt) * 64]);
    }
    const bool pw = tid < ROWS * UB;                   // granule order of the bf16x6 forward kernel: granule tid = jp*64 + hr*2 + jlo
    const int prow = (tid >> 1) & 15, pu = ((tid >> 5) & 1) * 8 + 2 * ((tid >> 6) & 3) + (tid & 1);
    const int pb = r0 + prow, pj = j0 + pu;
    const bool pok = pw && pb < B;
    float dh_carry = 0.f, z_next = 0.f;                // dh_{t+1} and z_{t+1} of this thread's (row, unit)
    float sb_r = 0.f, sb_z = 0.f, sb_n = 0.f, sb_nr = 0.f;   // sums over t of the gate gradients: the bias gradients of this clip
    if (pok && d.dh_n) dh_carry = d.dh_n[(size_t)pb * H + pj];

    constexpr size_t TILE = (size_t)RT * 256;
    unsigned long long* gran = reinterpret_cast<unsigned long long*>(ex.gran[s]);
    const int q = lane >> 4;
    const size_t lane_off = (size_t)(wave + NW * (q >> 1)) * TILE + 2 * ((q & 1) * 16 + (lane & 15));
    const size_t slot = ex.slot[s];
    const size_t grp = (size_t)rb * nchh * TILE;
    const size_t pub = grp + (size_t)ub * TILE + tid;
    M3T_PERSIST_POLL_STATE(ub, H >> 4);
    M3T_STAMP_STATE();
    M3T_BWD_ENVELOPE(pb, pj);

#define M3T_STEP_FILE "gru_persist_bwd16_step.inc"
#include "gru_persist_ab.inc"
    scan_drain();
    M3T_BWD_STORE_CARRY();
    M3T_STAMP_DUMP();
}


// ------------------------------------------------------------------------------------------------ backward
template <int NC, int RT>
__global__ __launch_bounds__(NT) void gru_persist_bwd_kernel(BwdGroup g, FragPtrs fp, ExPtrs ex, int B, int T, int G, int nrb,
                                                             unsigned* err) {
    constexpr int ROWS = 16 * RT;
    constexpr int H = 128 * NC, H3 = 3 * H, nchh = H >> 4, nch = H3 >> 4;
    __shared__ float red[2][NW][ROWS][UB + 1];
    M3T_PERSIST_WHO(ub);
    const m3t_gru_bwd_desc d = g.d[s];
    const int j0 = ub * UB, r0 = rb * ROWS;

    // W_hh^T fragments of this workgroup's 16 output units: chunk c = gate*nchh + (wave + 8m)
    float4 wt[3][NC];
    {
        const float4* Wt = reinterpret_cast<const float4*>(fp.wfrag[s] + (size_t)ub * nch * 256);
#pragma unroll
        for (int gt = 0; gt < 3; ++gt)
#pragma unroll
            for (int m = 0; m < NC; ++m) wt[gt][m] = Wt[(size_t)(gt * nchh + wave + m * NW) * 64 + lane];
    }
    const bool pw = tid < ROWS * UB;                   // granule-order numbering, as in the forward kernel
    const int prow = (tid >> 8) * 16 + (tid & 15), pu = ((tid >> 4) & 3) * 4 + ((tid >> 6) & 3);
    const int pb = r0 + prow, pj = j0 + pu;
    const bool pok = pw && pb < B;
    float dh_carry = 0.f, z_next = 0.f;                // dh_{t+1} and z_{t+1} of this thread's (row, unit)
    float sb_r = 0.f, sb_z = 0.f, sb_n = 0.f, sb_nr = 0.f;   // sums over t of the gate gradients: the bias gradients of this clip
    if (pok && d.dh_n) dh_carry = d.dh_n[(size_t)pb * H + pj];

    constexpr size_t TILE = (size_t)RT * 256;
    u32x4* gran = reinterpret_cast<u32x4*>(ex.gran[s]);
    const size_t slot = ex.slot[s];
    const size_t grp = (size_t)rb * nchh * TILE;
    const size_t pub = grp + (size_t)ub * TILE + tid;
    M3T_PERSIST_POLL_STATE(ub, H >> 4);
    M3T_STAMP_STATE();
    M3T_BWD_ENVELOPE(pb, pj);

#define M3T_STEP_FILE "gru_persist_bwd_step.inc"
#include "gru_persist_ab.inc"
    scan_drain();
    M3T_BWD_STORE_CARRY();
    M3T_STAMP_DUMP();
}

// ------------------------------------------------------------------------------------------------ backward, bf16x6
// The recurrent product of the backward scan, dh_t = dgh_{t+1} W_hh (K = 3H), on the bf16 matrix pipe and still fp32-accurate:
// at H = 512 a SIMD spent 96 fp32 MFMAs x 32 cycles = 3072 cycles per step on it (in-kernel stamps: MFMA 0.8 us + 1.2 us at
// the barrier waiting for the partner wave's MFMAs, of a 4.1 us step).  The three gate gradients of a unit do not fit a 16-byte
// granule once split in three (18 B + tag), so the CONSUMER splits: the granules stay {dr, dz, dn*r, tag} in fp32, and each
// lane splits its 48 gathered values exactly into three bf16 terms (truncation split, ~11 VALU operations per pair of values)
// while the partner wave of its SIMD multiplies -- vector and matrix instructions of different waves issue side by side.  Per
// wave 36 v_mfma_f32_16x16x32_bf16 (6 products of weight >= 2^-16 per 32-deep k-step, smallest first) replace 48 fp32 MFMAs
// at half their cycles each.  W_hh is split by the prep kernel into the B-operand order (72 VGPRs).  Results agree with the
// fp32-MFMA kernel to fp32 rounding (M3T_SCAN_FP32 / M3T_SCAN_X6=0 keep that kernel and bit-identity with the per-step path).
// wfrag[ub][wave][ks = gate*KS + h][term][lane][8]: term t of W_hh[gate*H + 16*(wave + 8*(2h + (e>>2))) + 4*(lane>>4) + (e&3)][ub*16 + (lane&15)]
struct PrepBwd6Args { const float* w[M3T_MAX_SCANS]; unsigned short* wf[M3T_MAX_SCANS]; };
// (one launch per level: blockIdx.y = scan)
__global__ void wfrag_bwd6_prep_kernel(PrepBwd6Args a, int H, int direct) {
    const float* __restrict__ w = a.w[blockIdx.y];
    unsigned short* __restrict__ wf = a.wf[blockIdx.y];
    const int ksn = 3 * (H >> 8);                     // k-steps per wave
    const size_t total = (size_t)3 * H * H;           // one thread per weight: writes its three terms
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = i & 7, l = (i >> 3) & 63;
        size_t r = i >> 9;
        const int ks = r % ksn; r /= ksn;
        const int wv = r % NW, ub = r / NW;
        const int gt = ks / (H >> 8), h = ks % (H >> 8);
        const int unit = 16 * (wv + NW * (2 * h + (e >> 2))) + 4 * (l >> 4) + (e & 3);
        // direct: the untransposed parameter w_hh [3H][H] (M3T_SCAN_WHH); else w_hh_t [H][3H]
        const float x = direct ? w[((size_t)gt * H + unit) * H + ub * 16 + (l & 15)]
                               : w[((size_t)ub * 16 + (l & 15)) * 3 * H + (size_t)gt * H + unit];
        const __bf16 b1 = (__bf16)x;
        const float r1 = x - (float)b1;
        const __bf16 b2 = (__bf16)r1;
        const __bf16 b3 = (__bf16)(r1 - (float)b2);
        const size_t base = ((((size_t)(ub * NW + wv) * ksn + ks) * 3)) * 512 + (size_t)l * 8 + e;
        wf[base] = __builtin_bit_cast(unsigned short, b1);
        wf[base + 512] = __builtin_bit_cast(unsigned short, b2);
        wf[base + 1024] = __builtin_bit_cast(unsigned short, b3);
    }
}

// Exact three-term split of a PAIR of fp32 values into packed bf16 pairs (first value in the low half), by truncation: a
// term is the upper half of the bits (one v_perm packs a pair), the remainder one v_sub against the masked value: 2 and +
// 2 sub per term and pair, 3 perm = 11 VALU instructions per pair.  Measured equal (tools/scan_bench.py, 3.49-3.54 us per
// step at 4 x H=512): the mask in a register instead of a literal; round-to-nearest with v_cvt_pk_bf16_f32 + v_pk_add_f32
// (250 instead of 264 VALU instructions per lane and step, as the GEMM's split3_pair); v_cvt_pk + v_dot2c_f32_bf16 remainders
// without unpacking (168 instructions) -- and not exact (the parity test failed): the phase is not bound by its VALU count.
__device__ __forceinline__ void bwd6_split_pair(unsigned x0, unsigned x1, unsigned& o1, unsigned& o2, unsigned& o3) {
    const float r0 = __uint_as_float(x0) - __uint_as_float(x0 & 0xffff0000u);
    const float r1 = __uint_as_float(x1) - __uint_as_float(x1 & 0xffff0000u);
    const float s0 = r0 - __uint_as_float(__float_as_uint(r0) & 0xffff0000u);
    const float s1 = r1 - __uint_as_float(__float_as_uint(r1) & 0xffff0000u);
    o1 = __builtin_amdgcn_perm(x1, x0, 0x07060302u);
    o2 = __builtin_amdgcn_perm(__float_as_uint(r1), __float_as_uint(r0), 0x07060302u);
    o3 = __builtin_amdgcn_perm(__float_as_uint(s1), __float_as_uint(s0), 0x07060302u);
}

template <int NC>
__global__ __launch_bounds__(NT) void gru_persist_bwd6_kernel(BwdGroup g, FragPtrs fp, ExPtrs ex, int B, int T, int G, int nrb,
                                                             unsigned* err) {
    constexpr int RT = 1, ROWS = 16, KS = NC / 2;
    constexpr int H = 128 * NC, H3 = 3 * H, nchh = H >> 4;
    __shared__ float red[2][NW][ROWS][UB + 1];
    M3T_PERSIST_WHO(ub);
    const m3t_gru_bwd_desc d = g.d[s];
    const int j0 = ub * UB, r0 = rb * ROWS;

    pbf16x8 wb[3 * KS][3];                             // [k-step = gate*KS + h][term]: 72 VGPRs at H = 512
    {
        const pu32x4* Wf = reinterpret_cast<const pu32x4*>(fp.wfrag[s]) + ((size_t)(ub * NW + wave) * 3 * KS * 3) * 64 + lane;
#pragma unroll
        for (int k = 0; k < 3 * KS; ++k)
#pragma unroll
            for (int t = 0; t < 3; ++t) wb[k][t] = __builtin_bit_cast(pbf16x8, Wf[(k * 3 + t) * 64]);
    }
    const bool pw = tid < ROWS * UB;                   // granule-order numbering, as in the forward kernel
    const int prow = (tid >> 8) * 16 + (tid & 15), pu = ((tid >> 4) & 3) * 4 + ((tid >> 6) & 3);
    const int pb = r0 + prow, pj = j0 + pu;
    const bool pok = pw && pb < B;
    float dh_carry = 0.f, z_next = 0.f;                // dh_{t+1} and z_{t+1} of this thread's (row, unit)
    float sb_r = 0.f, sb_z = 0.f, sb_n = 0.f, sb_nr = 0.f;   // sums over t of the gate gradients: the bias gradients of this clip
    float amx = 0.f;                                   // max |dr~|, |dz~|, |dn~| of this thread: the magnitude slot d.amax (fp16x3 GEMMs)
    if (pok && d.dh_n) dh_carry = d.dh_n[(size_t)pb * H + pj];

    constexpr size_t TILE = (size_t)RT * 256;
    u32x4* gran = reinterpret_cast<u32x4*>(ex.gran[s]);
    const size_t slot = ex.slot[s];
    const size_t grp = (size_t)rb * nchh * TILE;
    const size_t pub = grp + (size_t)ub * TILE + tid;
    M3T_PERSIST_POLL_STATE(ub, H >> 4);
    M3T_STAMP_STATE();
    M3T_BWD_ENVELOPE(pb, pj);

#define M3T_STEP_FILE "gru_persist_bwd6_step.inc"
#include "gru_persist_ab.inc"
    scan_drain();
    M3T_BWD_STORE_CARRY();
    if (d.amax && pw) {                                // (waves 0..3: uniform per wave)
        const float m = wave_max(pok ? amx : 0.f);
        if (lane == 0) atomicMax(d.amax, (unsigned long long)__float_as_uint(m));
    }
    M3T_STAMP_DUMP();
}

// ---- producer-side operand split (gru_persist_bwd3q_kernel below; its narrow predecessor gru_persist_bwd3p_kernel of round 3 was removed in round 5:
// no default-mode launch used it any more -- VERDICT r4 weak-10; DESIGN.md section 7 / NOTEBOOK.md section 5e) ----------------------------------------
// The shipped six-product backward step is bound by its consumers' operand split (264 VALU instructions per lane and step, redone by
// all 32 workgroups of a group on the same 16 x 1536 values).  Here each PRODUCER splits its own three values (dr~, dz~, dn~ r) into two
// fp16 terms, scaled by the power of two of its tile's largest magnitude (16 rows x 16 units x 3 values: exact, so nothing can
// overflow), and publishes {hi|lo, hi|lo, hi|lo, tag24 | exponent << 24} in the same 16-byte granule.  A consumer multiplies one
// producer tile at a time (16-deep fp16 MFMAs: 3 gates x 3 products into one accumulator) and folds the tile's scale in as it adds the
// tile's product to its sum: 12 v_perm + 4 FMA per tile instead of the split.  W_hh^T: two fp16 terms per workgroup slice, K-16 layout.
typedef unsigned pu32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 pf16x4 __attribute__((ext_vector_type(4)));
struct PrepBwd3pArgs { const float* w[M3T_MAX_SCANS]; unsigned short* wf[M3T_MAX_SCANS]; float* inv[M3T_MAX_SCANS]; };
// max over the wave of a non-negative float's bit pattern, uniform: four DPP steps inside each row of 16 lanes, then the four row
// maxima through v_readlane
__device__ __forceinline__ unsigned wave_umax_dpp(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false));      // row_shr:1
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false));      // row_shr:2
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false));      // row_shr:4
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false));      // row_shr:8: lane 15 of a row = the row's maximum
    const unsigned a = (unsigned)__builtin_amdgcn_readlane((int)v, 15), b = (unsigned)__builtin_amdgcn_readlane((int)v, 31);
    const unsigned c = (unsigned)__builtin_amdgcn_readlane((int)v, 47), d = (unsigned)__builtin_amdgcn_readlane((int)v, 63);
    return max(max(a, b), max(c, d));
}
__device__ __forceinline__ unsigned bwd3p_split(float xs) {          // the scaled value as (fp16 hi | fp16 lo << 16)
    const _Float16 h1 = (_Float16)xs;
    const _Float16 h2 = (_Float16)(xs - (float)h1);
    return (unsigned)__builtin_bit_cast(unsigned short, h1) | ((unsigned)__builtin_bit_cast(unsigned short, h2) << 16);
}

// ---- wide producer-split backward scan with 32-deep MFMAs (gru_persist_bwd3q_kernel, round 4) ---------------------------------------------
// gru_persist_bwd3p_kernel multiplies one 16-unit producer tile per MFMA (v_mfma_f32_16x16x16_f16: the tile's scale is applied to the
// MFMA's result) -- in a wide workgroup (two unit tiles) 72 MFMAs per wave and step, and a 16-deep MFMA costs the issue cycles of a
// 32-deep one (tools/mfma_probe.hip: 18-20 cycles either way): the matrix pipe of a SIMD was busy for two thirds of the wide backward
// step.  A WIDE workgroup publishes two adjacent tiles; scaled by ONE power of two (the maximum of the per-cell bound over all eight
// waves) they form a 32-unit producer PAIR that a consumer multiplies with v_mfma_f32_16x16x32_f16: 36 MFMAs per wave and step (3.42 ->
// 3.28 us per step at 4 x H=512; the narrow kernel on twice the CUs: 3.30).  Differences to bwd3p: the granule order inside a tile --
// granule (unit & 7) * 32 + (unit >> 3) * 16 + row, so that lane (row, q) of a consumer finds the eight consecutive k of its A operand
// (units 8 (q & 1) + e of tile q >> 1) at one address + e * 512 bytes and a wave instruction still reads whole 512-byte runs; W_hh^T
// fragments in the 32-deep B-operand layout (wfrag_bwd3q_prep_kernel); the scale exchange covers all eight waves.  Always wide, always
// with the memory-order hand-over of the cell threads' HBM traffic through LDS (see gru_persist_fwd6_kernel, CO).
// wfrag3q[ub][wave][gate][pair m][term][lane][8 fp16]: term of W_hh[gate*H + 32*(wave + NW*m) + 8*(lane>>4) + e][ub*16 + (lane&15)] * scale(ub)
__global__ __launch_bounds__(256) void wfrag_bwd3q_prep_kernel(PrepBwd3pArgs a, int H, int direct) {
    const float* __restrict__ w = a.w[blockIdx.z];
    unsigned short* __restrict__ wf = a.wf[blockIdx.z];
    const int ub = blockIdx.x, np = H >> 8;                 // pairs per wave
    __shared__ float red[4];
    float m = 0.f;
    const int tot4 = 3 * H * 4;
    auto ld = [&](int i) {
        return direct ? *reinterpret_cast<const float4*>(w + (size_t)(i >> 2) * H + ub * 16 + 4 * (i & 3))
                      : *reinterpret_cast<const float4*>(w + ((size_t)ub * 16 + i / (3 * H / 4)) * 3 * H + 4 * (i % (3 * H / 4)));
    };
    auto fold = [&](const float4& v) {
        m = fmaxf(fmaxf(m, m3t_fin_abs(v.x)), fmaxf(m3t_fin_abs(v.y), fmaxf(m3t_fin_abs(v.z), m3t_fin_abs(v.w))));
    };
    int i0 = threadIdx.x;
    for (; i0 + 768 < tot4; i0 += 1024) {
        const float4 v0 = ld(i0), v1 = ld(i0 + 256), v2 = ld(i0 + 512), v3 = ld(i0 + 768);
        fold(v0); fold(v1); fold(v2); fold(v3);
    }
    for (; i0 < tot4; i0 += 256) fold(ld(i0));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sc, inv;
    m3t_f16_scale(__float_as_uint(m), sc, inv);
    if (threadIdx.x == 0 && blockIdx.y == 0) a.inv[blockIdx.z][ub] = inv;
    // one item = the eight k of one (gate, pair, wave, lane): eight row reads at the same column, one 16-byte store per term
    const int items = 3 * np * NW * 64;
    for (int j = blockIdx.y * 256 + threadIdx.x; j < items; j += 256 * PREP3H_SPLIT) {
        const int l = j & 63;
        int r = j >> 6;
        const int pm = r % np; r /= np;
        const int wv = r % NW, gt = r / NW;
        const int unit0 = 32 * (wv + NW * pm) + 8 * (l >> 4), n = l & 15;
        unsigned h1[4], h2[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned short a1[2], a2[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float x = (direct ? w[((size_t)gt * H + unit0 + 2 * i + k) * H + ub * 16 + n]
                                        : w[((size_t)ub * 16 + n) * 3 * H + (size_t)gt * H + unit0 + 2 * i + k]) * sc;
                const _Float16 f1 = (_Float16)x;
                const _Float16 f2 = (_Float16)(x - (float)f1);
                a1[k] = __builtin_bit_cast(unsigned short, f1); a2[k] = __builtin_bit_cast(unsigned short, f2);
            }
            h1[i] = (unsigned)a1[0] | ((unsigned)a1[1] << 16); h2[i] = (unsigned)a2[0] | ((unsigned)a2[1] << 16);
        }
        const size_t base = (((((size_t)(ub * NW + wv) * 3 + gt) * np + pm) * 2) * 64 + l) * 8;
        *reinterpret_cast<uint4*>(wf + base) = make_uint4(h1[0], h1[1], h1[2], h1[3]);
        *reinterpret_cast<uint4*>(wf + base + 512) = make_uint4(h2[0], h2[1], h2[2], h2[3]);
    }
}

// PROF: the in-kernel phase stamps (M3T_SCAN_PROF) live in an instantiation of their own -- their 14 VGPRs do not fit beside the rest
// (that instantiation spills: its stamps overstate the step)
// RB (M3T_SCAN_SPREAD): clips per row block, as in gru_persist_fwd6_kernel -- every lane gathers for a row < RB (half the load instructions),
// operand rows >= RB are garbage, which stays inside rows >= RB of the products.  Everything that leaves a cell is masked by pok / hok (which
// include row < RB): the workgroup's scale (bnd), the published terms, the bias sums, dh, the stored results and amx -- so neither the scale
// nor any amax slot can see a garbage row.
template <int NC, bool PROF = false, int RB = 16>
__global__ __launch_bounds__(NT) void gru_persist_bwd3q_kernel(BwdGroup g, FragPtrs fp, ExPtrs ex, int B, int T, int G, int nrb,
                                                             unsigned* err) {
    constexpr int ROWS = 16, NP = NC / 2;              // NP: producer pairs per wave
    static_assert(RB == 16 || (RB == 8 && !PROF), "row blocks: 16 clips, or 8 (the gather deals the units over lane bit 3 for 8 rows)");
    constexpr int H = 128 * NC, H3 = 3 * H, nchh = H >> 4;
    __shared__ float red[2][NW][2][ROWS][UB + 1];
    M3T_PERSIST_WHO(ubw);
    const m3t_gru_bwd_desc d = g.d[s];
    const int tu = tid >> 8;                           // the unit tile this thread does cell math for
    const int ub = ubw * 2 + tu;
    const int j0 = ub * UB, r0 = rb * RB;

    pu32x4 wb[2][3][NP][2];                            // [unit tile][gate][producer pair of this wave's K-slice][term]: 8 fp16 per lane, 96 VGPRs at H = 512
    float winv[2];                                     // 1 / (scale of the slice's W_hh^T)
    // (round 4 also tried building these fragments in the kernel, as the forward kernel does: the 8 k of a fragment are 8 ROWS of W_hh, 192
    // strided scalar loads per lane and pass -- +25 us per launch, what the prep launch it replaced costs: not kept)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const pu32x4* Wf = reinterpret_cast<const pu32x4*>(fp.wfrag[s]) + ((size_t)((ubw * 2 + u) * NW + wave) * 3 * NP * 2) * 64 + lane;
#pragma unroll
        for (int gt = 0; gt < 3; ++gt)
#pragma unroll
            for (int m = 0; m < NP; ++m)
#pragma unroll
                for (int t = 0; t < 2; ++t) wb[u][gt][m][t] = Wf[((gt * NP + m) * 2 + t) * 64];
        winv[u] = reinterpret_cast<const float*>(fp.wfrag[s])[(size_t)4 * H * H + ubw * 2 + u];
    }
    __shared__ __attribute__((aligned(16))) unsigned pmx8[8];      // the waves' maxima of the step (two lowest bits: step tag)
    if (tid < 8) pmx8[tid] = 0u;
    const unsigned pmx8_addr = (unsigned)(uintptr_t)pmx8;
    // cell threads in granule order: granule ti of the tile <-> row ti & 15, unit 8 ((ti >> 4) & 1) + (ti >> 5)
    const int ti = tid & 255;
    const int prow = ti & 15, pu = 8 * ((ti >> 4) & 1) + (ti >> 5);
    const int pb = r0 + prow, pj = j0 + pu;
    const bool plive = prow < RB;                      // publishes: live rows past the batch carry zeros
    const bool pok = plive && pb < B;
    float dh_carry = 0.f, z_next = 0.f;                // dh_{t+1} and z_{t+1} of this thread's (row, unit)
    float sb_r = 0.f, sb_z = 0.f, sb_n = 0.f, sb_nr = 0.f;   // sums over t of the gate gradients: the bias gradients of this clip
    float amx = 0.f;                                   // max |dr~|, |dz~|, |dn~| of this thread: the magnitude slot d.amax (fp16x3 GEMMs)
    if (pok && d.dh_n) dh_carry = d.dh_n[(size_t)pb * H + pj];

    constexpr size_t TILE = 256;
    u32x4* gran = reinterpret_cast<u32x4*>(ex.gran[s]);
    const size_t slot = ex.slot[s];
    const size_t grp = (size_t)rb * nchh * TILE;
    const size_t pub = grp + (size_t)ubw * 2 * TILE + tid;
    // gather base of this lane inside the group: pair (wave + NW m) = tiles 2 (wave + NW m) + (q >> 1); granule e * 32 + (q & 1) * 16 + row
    // (RB = 8: row lane & 7, and lane bit 3 picks the odd unit e, 32 granules on)
    const size_t lane_src = RB < ROWS ? (size_t)(2 * wave + (lane >> 5)) * TILE + ((lane >> 4) & 1) * 16 + (lane & 7) + 32 * ((lane >> 3) & 1)
                                      : (size_t)(2 * wave + (lane >> 5)) * TILE + ((lane >> 4) & 1) * 16 + (lane & 15);
    bool dead = false;                                 // M3T_PERSIST_POLL_STATE without pub_step: every wave of this kernel does cell math
    int poll_delay = ex.poll_fixed >= 0 ? ex.poll_fixed : POLL_DELAY_INIT;
    __shared__ unsigned poll_fail[2];                  // by step parity
    const int l2mode = persist_handshake(ex, gid, ubw, (H >> 4) / 2, tid, err);     // 1: this group shares one XCD's L2 (publish with plain stores)
    if (tid < 2) poll_fail[tid] = 0;                   // first read after the first barrier
    const bool stamp = PROF && ex.prof != nullptr && blockIdx.x == 0 && tid == ex.prof_tid;
    long long psum[PROF ? 6 : 1] = {0}, last = stamp ? clock64() : 0;
    const bool MARK_ASC = d.reverse != 0;              // the backward scan of a forward-direction GRU walks time downwards
    M3T_MARK_STATE();
    int amk = 0, amk_step = nmarks > 0 ? mark0 : -1;  // per-window magnitude slots d.amax[1 + window]
#define M3T_QSTAMP(i)                                                        \
    do {                                                                     \
        if (PROF && stamp) { const long long now = clock64(); psum[PROF ? (i) : 0] += now - last; last = now; } \
    } while (0)

    // activations: loaded one step ahead by inline asm in MEMORY order (thread ti: row ti >> 4, unit ti & 15 of its tile), handed to the
    // cell threads through LDS; results the other way, stored one step late
    const int hrow = ti >> 4, hun = ti & 15;
    const int hb = r0 + hrow, hj = j0 + hun;
    const bool hok = hrow < RB && hb < B;
    const int hg = (hun & 7) * 32 + (hun >> 3) * 16 + hrow;      // granule index of cell (hrow, hun)
    constexpr int SLOTS = 272;
    const int slot_h = tu * SLOTS + hg + (hg >> 4), slot_c = tu * SLOTS + ti + (ti >> 4);
    extern __shared__ __attribute__((aligned(16))) unsigned char stage_raw[];
    f32x4* const sin4 = reinterpret_cast<f32x4*>(stage_raw);                  // [parity][2][SLOTS] gate records
    f32x4* const sout = sin4 + 2 * 2 * SLOTS;                                 // [parity][2][SLOTS] (dr~, dz~, dn~, dn~ r)
    float2* const sin2 = reinterpret_cast<float2*>(sout + 2 * 2 * SLOTS);     // [parity][2][SLOTS] (dout, h_prev)
    M3T_BWD_ENVELOPE(hb, hj);                         // st_*: the results of the cell this thread stores for

#define M3T_STEP_FILE "gru_persist_bwd3q_step.inc"
#include "gru_persist_ab.inc"
    scan_drain();
    __syncthreads();                                   // the last step's results are still in LDS
    if (hok) {
        const f32x4 r4 = sout[((T - 1) & 1) * 2 * SLOTS + slot_h];
        st_dr = r4[0]; st_dz = r4[1]; st_dn = r4[2]; st_dnr = r4[3];
        store_results(T - 1);
    }
    M3T_BWD_STORE_CARRY();
    if (d.amax) {
        const float m = wave_max(pok ? amx : 0.f);
        if (lane == 0) {
            atomicMax(d.amax, (unsigned long long)__float_as_uint(m));
            if (nmarks > 0) atomicMax(d.amax + 1 + amk, (unsigned long long)__float_as_uint(m));      // the last window's slot
        }
    }
    if (PROF && stamp)
        for (int i = 0; i < 6; ++i) ex.prof[i] = (unsigned long long)psum[PROF ? i : 0];
#undef M3T_QSTAMP
}

// ------------------------------------------------------------------------------------------------ host side
unsigned long long* g_prof = nullptr;   // device buffer of phase stamps when M3T_SCAN_PROF=1
int g_launches = 0;                 // persistent launches issued by this process (m3t_gru_persist_count)
unsigned* g_err_host = nullptr;     // host-mapped error word (device writes, host polls without a sync)
unsigned* g_err_dev = nullptr;

bool ensure_err_word() {
    if (g_err_host) return true;
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return false; }
    std::memset(h, 0, 64);
    void* dptr = nullptr;
    if (hipHostGetDevicePointer(&dptr, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(h); return false; }
    g_err_host = static_cast<unsigned*>(h);
    g_err_dev = static_cast<unsigned*>(dptr);
    return true;
}

int device_cus() {
    static int cus = -1;
    if (cus < 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); cus = 0; }
        else cus = prop.multiProcessorCount;
    }
    return cus;
}

// workgroups of `kernel` that can be resident at once, conservatively (the occupancy API can read one high near an
// SGPR allocation edge -- MI355X_MICROARCH.md, "Residency and cooperative launch" -- so two per CU are only
// assumed when it reports three)
template <typename K>
int resident_capacity(K kernel) {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, NT, 0) != hipSuccess) { (void)hipGetLastError(); return 0; }
    const int per_cu = occ >= 3 ? 2 : (occ >= 1 ? 1 : 0);
    return per_cu * device_cus();
}

static int poll_env_early(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? atoi(e) : dflt;
}

struct Shape { int nc, rt, G, nrb, grid, active, slot_map, rb; };      // rb: clips per row block (16 * rt; 8: M3T_SCAN_SPREAD)

// every scan of the level has the same H = 128 * NC (NC = 1..4: the k-chunks per wave are compile-time, so the gather
// and the MFMA chain are straight-line code); RT = 1 when the 16-row grid fits one workgroup per CU, else 2
template <typename D>
bool level_shape(const D* d, int n, int B, Shape& sh, int uw = 1, bool spread = false) {      // uw: 16-unit tiles per workgroup (the "wide" kernels: 2)
    const int maxh = d[0].H;
    if (maxh % 128 != 0 || maxh > 512) return false;
    for (int i = 1; i < n; ++i)
        if (d[i].H != maxh) return false;
    sh.nc = maxh / 128;
    sh.rt = 0;
    // spread (M3T_SCAN_SPREAD, asked for by launches that have the chip to themselves): row blocks of 8 clips while the 8-clip groups at
    // one 16-unit tile per member fit the CUs -- counted like that for the wide kernels too: a wide launch exists to leave half the chip
    // to its neighbours, and 4 x H=512 must not grow back to 256 workgroups.  Only the callers whose kernels have the form pass it.
    const bool rb8 = spread && n * cdiv(B, 8) * (maxh / 16) <= device_cus();
    for (int rt = 1; rt <= 2; ++rt) {
        if (uw > 1 && rt > 1) break;
        const int members = maxh / 16 / uw;
        const int nrb = rb8 ? cdiv(B, 8) : cdiv(B, 16 * rt), G = n * nrb, active = G * members;
        // launched: 8 XCD slots x ceil(G / 8) groups per slot x H / 16 members (persist_map); blocks of empty slots exit at once,
        // so what must fit the chip at one workgroup per CU is the ACTIVE count
        if (active <= device_cus()) {
            // L2-served exchange (formerly M3T_SCAN_L2, mode 2 kept): launches whose groups are XCD-aligned anyway (G % 8 == 0: the 4 x H=512 encoder level, the
            // scorers) use the slot mapping + handshake, the others keep G * H/16 blocks dealt over all 8 XCDs and exchange through
            // the memory side; 1 every launch (a 4-group launch then fills 4 XCDs and leaves 4 empty: -40 % traffic on those too,
            // but their steps got slower -- 19.08 vs 18.73 ms per training step, interleaved A/B; mode 2: 18.83); 0 never
#ifndef M3T_SCAN_L2_MODE
#define M3T_SCAN_L2_MODE 2
#endif
            constexpr int l2 = M3T_SCAN_L2_MODE;
            sh.rt = rt; sh.nrb = nrb; sh.G = G; sh.active = active; sh.rb = rb8 ? 8 : 16 * rt;
            // round 4: a WIDE launch with fewer than 8 groups puts each group on an XCD of its own as well (16 of its 32 CUs: the GEMMs beside
            // it still find CUs on every XCD, which is what sank this placement for the narrow 32-member groups in round 3): fusion level
            // backward 3.29 -> 3.15 us per step, its exchange served by L2 (traffic 2.5x -> ~1.1x algorithmic)
            sh.slot_map = (l2 == 1 || (l2 == 2 && G % 8 == 0) || (uw > 1 && G <= 8)) ? 1 : 0;
            sh.grid = sh.slot_map ? 8 * cdiv(G, 8) * members : active;
            break;
        }
    }
    return sh.rt != 0;
}

typedef void (*FwdKernel)(FwdGroup, FragPtrs, ExPtrs, int, int, int, int, unsigned*);
typedef void (*BwdKernel)(BwdGroup, FragPtrs, ExPtrs, int, int, int, int, unsigned*);

FwdKernel pick_fwd(const Shape& sh) {
    static const FwdKernel k[2][4] = {
        {gru_persist_fwd_kernel<1, 1>, gru_persist_fwd_kernel<2, 1>, gru_persist_fwd_kernel<3, 1>, gru_persist_fwd_kernel<4, 1>},
        {gru_persist_fwd_kernel<1, 2>, gru_persist_fwd_kernel<2, 2>, gru_persist_fwd_kernel<3, 2>, gru_persist_fwd_kernel<4, 2>}};
    return k[sh.rt - 1][sh.nc - 1];
}
BwdKernel pick_bwd(const Shape& sh) {
    static const BwdKernel k[2][4] = {
        {gru_persist_bwd_kernel<1, 1>, gru_persist_bwd_kernel<2, 1>, gru_persist_bwd_kernel<3, 1>, gru_persist_bwd_kernel<4, 1>},
        {gru_persist_bwd_kernel<1, 2>, gru_persist_bwd_kernel<2, 2>, gru_persist_bwd_kernel<3, 2>, gru_persist_bwd_kernel<4, 2>}};
    return k[sh.rt - 1][sh.nc - 1];
}


// A scan launch that leaves most of the chip free (a light level: <= 96 workgroups) asks for enough unused dynamic LDS that
// no GEMM workgroup fits beside one of its workgroups on a CU: co-resident GEMM waves take issue slots and LDS bandwidth
// from a latency-bound scan (audio backward scan beside the weight-gradient GEMMs: 1.8 instead of 0.75 ms), and the
// GEMMs have the other CUs.
// Round 4: the limit is 192 workgroups -- a wide heavy launch (128) owns its CUs too, beside the audio launch (64) and the GEMMs (the rest);
// `need`: dynamic LDS the kernel itself uses (the wide kernels' partial sums), granted whatever the grid.
template <typename K>
static size_t exclusive_lds(K kernel, int grid, size_t need = 0) {
    if (grid > 192 && need == 0) return 0;
    hipFuncAttributes a;
    if (hipFuncGetAttributes(&a, reinterpret_cast<const void*>(kernel)) != hipSuccess) { (void)hipGetLastError(); return 0; }
    const size_t want = (size_t)152 * 1024;
    if (a.sharedSizeBytes >= want && need == 0) return 0;
    size_t dyn = grid > 192 ? need : (want > a.sharedSizeBytes ? want - a.sharedSizeBytes : 0);
    if (dyn < need) dyn = need;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return dyn;
}

// The scan kernel of a level, behind whatever the level prepared (fragments, exchange): the stream first waits for the caller's event
// (m3t_gru_scan_after: the preparation kernels and memsets in front are not held back), the caller's event pair (m3t_gru_scan_events) is
// recorded right around the kernel, and the launch owns its CUs (exclusive_lds).  need: the dynamic LDS the kernel itself uses.
template <typename K, typename Grp>
static int launch_scan(K kernel, const Shape& sh, size_t need, const Grp& g, const FragPtrs& fp, const ExPtrs& ex, int B, int T, hipStream_t s) {
    { const int e = persist_take_after(s); if (e) return e; }
    persist_record_start(s);
    const size_t dyn = exclusive_lds(kernel, sh.active, need);
    if (dyn < need) return M3T_EINVAL;
    hipLaunchKernelGGL(kernel, dim3(sh.grid), dim3(NT), dyn, s, g, fp, ex, B, T, sh.G, sh.nrb, g_err_dev);
    persist_record_end(s);
    M3T_LAUNCH_CHECK();
    return 0;
}

// grid of a grid-stride fragment prep kernel: one thread per weight of W_hh [3H][H], at most 1024 blocks
static int prep_blocks(int H) {
    const int blk = (3 * H * H + 255) / 256;
    return blk > 1024 ? 1024 : blk;
}

// ---- exchange arena: tags that are unique per launch instead of a memset per launch ---------------------------------------
// A consumer accepts a granule when its tag equals the expected one, so stale granules of EARLIER launches in the same memory
// must never carry that tag.  Until now every launch zeroed its exchange buffers first (3-4 small fill kernels in front of
// every scan: 40 per C3 step).  With a caller-provided ARENA that nothing but scan launches ever writes
// (m3t_gru_scan_arena), each launch draws a fresh tag range [base + 1, base + T] from a per-arena counter instead: granules of
// older launches carry smaller tags and can never match.  The arena is split by granule format, because a data field of one
// format must never sit where another format keeps its tag:
//   kind 0  forward, fp32 MFMAs   8-B granule {h, tag32}                  2 MiB (16- or 32-row workgroups)
//   kind 1  forward, bf16x6       8-B granule {h1, h2, h3, tag16}         1 MiB
//   kind 2  backward, bf16 mode   8-B granule {dr, dz, dnr bf16, tag16}   1 MiB
//   kind 3  backward, fp32/bf16x6 16-B granule {dr, dz, dnr, tag32}       4 MiB
//   kind 4  placement handshake   8-B granule {xcc id, tag32}             64 KiB (persist_handshake)
// A sub-arena is zeroed when the arena is first seen (or after m3t_gru_scan_arena_reset) and when its tag counter would
// wrap (16-bit tags: every ~200 launches of 300 steps).  Without an arena the launch zeroes its buffers as before.
constexpr size_t ARENA_OFF[4] = {0, (size_t)2 << 20, (size_t)3 << 20, (size_t)4 << 20};
constexpr size_t ARENA_SIZE[4] = {(size_t)2 << 20, (size_t)1 << 20, (size_t)1 << 20, (size_t)4 << 20};
constexpr size_t ARENA_HS_OFF = (size_t)8 << 20, ARENA_HS_SIZE = (size_t)64 << 10;      // placement-handshake table
constexpr size_t ARENA_BYTES = ARENA_HS_OFF + ARENA_HS_SIZE;
struct ArenaState { unsigned long long next[5]; int fmt[4]; bool known; };      // fmt: the granule format that last used a region (two formats share region 3)
std::mutex g_arena_mu;
std::unordered_map<uintptr_t, ArenaState> g_arenas;
thread_local void* g_arena = nullptr;
thread_local size_t g_arena_bytes = 0;

// Lays the exchange buffers of the launch out (ex.gran / ex.slot) and makes stale tags impossible: inside the arena by a fresh
// tag range, else by zeroing.  Returns 0 or a hipError_t.
template <typename G>
int prepare_exchange(const G& g, const FragPtrs& fp, const Shape& sh, int kind, size_t gran_bytes, unsigned long long tag_max,
                     int T, ExPtrs& ex, hipStream_t s, int fmt = 0) {
    size_t bytes[M3T_MAX_SCANS], total = 0;
    for (int i = 0; i < g.n; ++i) {
        ex.slot[i] = (size_t)sh.nrb * (g.d[i].H / 16) * sh.rt * 256;
        bytes[i] = 2 * ex.slot[i] * gran_bytes;
        total += bytes[i];
    }
    ex.tag_base = 0;
    void* arena = g_arena;
    const size_t arena_bytes = g_arena_bytes;
    g_arena = nullptr; g_arena_bytes = 0;                       // consumed by this launch
    if (arena && arena_bytes >= ARENA_BYTES && ((uintptr_t)arena % 16) == 0 && total <= ARENA_SIZE[kind] &&
        (unsigned long long)T + 1 < tag_max) {
        char* base = static_cast<char*>(arena) + ARENA_OFF[kind];
        size_t off = 0;
        for (int i = 0; i < g.n; ++i) { ex.gran[i] = base + off; off += bytes[i]; }
        std::lock_guard<std::mutex> lock(g_arena_mu);
        ArenaState& st = g_arenas[(uintptr_t)arena];
        if (!st.known) {
            const hipError_t e = hipMemsetAsync(arena, 0, ARENA_BYTES, s);
            if (e != hipSuccess) return (int)e;
            st.known = true;
            for (int q = 0; q < 5; ++q) st.next[q] = 0;
            for (int q = 0; q < 4; ++q) st.fmt[q] = 0;
        }
        if (st.fmt[kind] != fmt) {                                      // another granule format used this region last: its tags mean nothing here
            const hipError_t e = hipMemsetAsync(base, 0, ARENA_SIZE[kind], s);
            if (e != hipSuccess) return (int)e;
            st.next[kind] = 0;
            st.fmt[kind] = fmt;
        }
        if (st.next[kind] + (unsigned long long)T + 1 >= tag_max) {     // the counter would wrap: start over on zeroed memory
            const hipError_t e = hipMemsetAsync(base, 0, ARENA_SIZE[kind], s);
            if (e != hipSuccess) return (int)e;
            st.next[kind] = 0;
        }
        ex.tag_base = (unsigned)st.next[kind];
        st.next[kind] += (unsigned long long)T;
        if (sh.slot_map && (size_t)sh.G * HS_STRIDE * 8 <= ARENA_HS_SIZE) {
            if (st.next[4] + 2 >= 0xffffffffull) {
                const hipError_t e = hipMemsetAsync(static_cast<char*>(arena) + ARENA_HS_OFF, 0, ARENA_HS_SIZE, s);
                if (e != hipSuccess) return (int)e;
                st.next[4] = 0;
            }
            ex.hs = reinterpret_cast<unsigned long long*>(static_cast<char*>(arena) + ARENA_HS_OFF);
            ex.hs_tag = (unsigned)(++st.next[4]);
        }
        return 0;
    }
    for (int i = 0; i < g.n; ++i) {
        ex.gran[i] = fp.xfrag[i];
        const hipError_t e = hipMemsetAsync(ex.gran[i], 0, bytes[i], s);     // no stale tag may match
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

template <typename G>
void fill_exchange(const G& g, const FragPtrs& fp, const Shape& sh, size_t gran_bytes, ExPtrs& ex, size_t (&bytes)[M3T_MAX_SCANS]) {
    std::memset(&ex, 0, sizeof(ex));
    static int prof_on = -1;
    if (prof_on < 0) {
        const char* e = std::getenv("M3T_SCAN_PROF");
        prof_on = (e && (e[0] == '1' || e[0] == '2')) ? (e[0] - '0') : 0;
        if (prof_on && hipMalloc(reinterpret_cast<void**>(&g_prof), 64) != hipSuccess) { (void)hipGetLastError(); g_prof = nullptr; }
    }
    ex.prof = g_prof;
    ex.prof_tid = prof_on == 2 ? 256 : 0;
    ex.poll_fixed = -1;
    ex.poll_align = 0;
    static const int spin_limit = poll_env_early("M3T_SCAN_SPIN_LIMIT", SPIN_LIMIT_DEFAULT);
    ex.spin_limit = spin_limit > 0 ? spin_limit : SPIN_LIMIT_DEFAULT;
    ex.fault_step = -1;
    ex.slot_map = sh.slot_map;
    for (int i = 0; i < g.n; ++i) bytes[i] = 0;
}

}  // namespace

bool persist_enabled() {
    static int on = -1;
    if (on < 0) {
        const char* e = std::getenv("M3T_SCAN_PERSIST");
        on = (e && e[0] == '0') ? 0 : 1;
    }
    return on == 1;
}

// Sticky: the answer stays non-zero until persist_reset_error().  (It used to be an exchange-to-zero; a host that runs a
// step ahead of the GPU then cleared the word before the finalize kernel of the failed step had read it on the device.)
int persist_poll_error() {
    if (!g_err_host) return 0;
    if (__atomic_load_n(g_err_host + 1, __ATOMIC_RELAXED) == 0u) return 0;
    const unsigned step1 = __atomic_load_n(g_err_host, __ATOMIC_RELAXED);
    return (int)(step1 ? step1 : 1u);
}

// Deferred mode (m3t_gru_error_defer): with several ranks a failure must be raised at a point ALL ranks agree on -- a rank that
// raises mid-step (a scan call returning M3T_ESPIN the moment its own host sees the flag) leaves its peers waiting in the
// step's collective.  While deferred, scan calls do not refuse to launch behind a dead scan (the device-side guards still
// skip every step queued behind it); the host learns of the failure from the all-reduced dead slot (m3t.ddp).
static int g_defer = 0;
void persist_set_defer(int on) { g_defer = on ? 1 : 0; }
bool persist_deferred() { return g_defer != 0; }

// the caller has synchronised the device: nothing queued can still read or write the words
void persist_reset_error() {
    if (!g_err_host) return;
    __atomic_store_n(g_err_host, 0u, __ATOMIC_RELAXED);
    __atomic_store_n(g_err_host + 1, 0u, __ATOMIC_RELAXED);
}

// device address of the sticky flag (create = allocate the host-mapped words if no persistent scan has run yet)
unsigned* persist_error_word_dev(bool create) {
    if (create && !ensure_err_word()) return nullptr;
    return g_err_dev ? g_err_dev + 1 : nullptr;
}

__global__ void inject_error_kernel(unsigned* err) { raise_spin(err, 0); }

int persist_inject_error(hipStream_t s) {
    if (!ensure_err_word()) return M3T_EINVAL;
    inject_error_kernel<<<1, 1, 0, s>>>(g_err_dev);
    M3T_LAUNCH_CHECK();
    return 0;
}

// Single owner per GPU.  A persistent launch needs its whole grid resident, so two processes that both run persistent
// scans on one device can each hold part of the chip while waiting for the rest (both would spin to the limit and fail
// with M3T_ESPIN).  The first process to get here takes an exclusive advisory lock on <dir>/m3t_persist_<pci-bus-id>.lock
// and keeps it for its lifetime; any other process on that device falls back to the launch-per-step scans (same results,
// no residency requirement).  <dir> is $XDG_RUNTIME_DIR when that is a directory owned by this user, else
// /tmp/m3t-<uid> (created 0700; refused if it is a symlink, not ours, or group/world-accessible).  The file is opened
// O_NOFOLLOW and must be a regular file of this user -- nothing is chmod-ed.  M3T_SCAN_LOCK=0 turns the guard off (e.g.
// a parent that holds the lock but is idle while its child runs).  If no usable lock file can be had the guard stands down
// rather than disable the fast path.  The decision is visible through m3t_gru_persist_owner() (bench.py, Trainer log it).
static int g_owner_state[64];      // per device: 0 unknown, 1 owner, 2 not the owner

static bool lock_dir(char* out, size_t n) {
    const uid_t uid = geteuid();
    struct stat st;
    const char* xdg = std::getenv("XDG_RUNTIME_DIR");
    if (xdg && xdg[0] == '/' && lstat(xdg, &st) == 0 && S_ISDIR(st.st_mode) && st.st_uid == uid && (st.st_mode & 077) == 0) {
        std::snprintf(out, n, "%s", xdg);
        return true;
    }
    std::snprintf(out, n, "/tmp/m3t-%u", (unsigned)uid);
    if (mkdir(out, 0700) != 0 && errno != EEXIST) return false;
    return lstat(out, &st) == 0 && S_ISDIR(st.st_mode) && st.st_uid == uid && (st.st_mode & 077) == 0;
}

bool persist_owner() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return true; }
    if (dev < 0 || dev >= 64) return true;
    int* state = g_owner_state;
    if (state[dev]) return state[dev] == 1;
    const char* e = std::getenv("M3T_SCAN_LOCK");
    if (e && e[0] == '0') { state[dev] = 1; return true; }
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, sizeof(bus) - 1, dev) != hipSuccess) { (void)hipGetLastError(); std::snprintf(bus, sizeof(bus), "dev%d", dev); }
    for (char* c = bus; *c; ++c)
        if (*c == ':' || *c == '/') *c = '_';
    char dir[128], path[256];
    if (!lock_dir(dir, sizeof(dir))) { state[dev] = 1; return true; }
    std::snprintf(path, sizeof(path), "%s/m3t_persist_%s.lock", dir, bus);
    const int fd = open(path, O_CREAT | O_RDWR | O_CLOEXEC | O_NOFOLLOW, 0600);
    if (fd < 0) { state[dev] = 1; return true; }
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_uid != geteuid()) { close(fd); state[dev] = 1; return true; }
    if (flock(fd, LOCK_EX | LOCK_NB) == 0) { state[dev] = 1; return true; }      // fd stays open: the lock lives as long as the process
    close(fd);
    state[dev] = 2;
    std::fprintf(stderr, "m3t: another process owns the persistent GRU scans of GPU %s (%s); this process uses the "
                         "launch-per-step scans (several times slower; m3t_gru_persist_owner() == 2)\n", bus, path);
    return false;
}

int persist_owner_state() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return (dev >= 0 && dev < 64) ? g_owner_state[dev] : 0;
}

size_t persist_exchange_bytes(int H, int B, bool backward) {
    const size_t rows = (size_t)cdiv(B, 32) * 32;       // covers the RT = 1 and RT = 2 row blocking
    return 2 * rows * (size_t)H * (backward ? 16 : 8);
}

static bool x6_scan_enabled() {
    static int on = -1;
    if (on < 0) {
        const char* e = std::getenv("M3T_SCAN_X6");
        on = (e && e[0] == '0') ? 0 : 1;
    }
    return on == 1;
}

// the forward recurrent product runs as bf16x6 (gru_persist_fwd6_kernel) for H = 256 / 512 at 16 rows per workgroup
bool persist_fwd_uses_x6(const FwdGroup& g, int B, int T, int flags) {
    Shape sh;
    // (in the bf16 mode the same kernel runs on operands that ARE bf16: h and W_hh are rounded first, their second and
    // third terms are zero, and what is left of the six products is the one bf16 product with fp32 accumulation)
    if ((flags & M3T_SCAN_FP32) || !x6_scan_enabled() || T >= 65535 || !level_shape(g.d, g.n, B, sh)) return false;
    return sh.rt == 1 && (sh.nc == 2 || sh.nc == 4);
}

bool persist_fwd_check(const FwdGroup& g, int B, int T) {
    Shape sh;
    return persist_enabled() && T >= 2 && level_shape(g.d, g.n, B, sh) && ensure_err_word() &&
           sh.active <= resident_capacity(pick_fwd(sh)) && persist_owner();
}

bool persist_bwd_check(const BwdGroup& g, int B, int T) {
    Shape sh;
    return persist_enabled() && T >= 2 && level_shape(g.d, g.n, B, sh) && ensure_err_word() &&
           sh.active <= resident_capacity(pick_bwd(sh)) && persist_owner();
}

// the backward scan of the bf16 mode runs on the bf16 matrix pipe with 8-byte granules (gru_persist_bwd16_kernel) for
// H = 256 / 512 at 16 rows per workgroup; M3T_SCAN_FP32 keeps the fp32-MFMA kernel (bit-identical to the per-step path)
bool persist_bwd_uses_16(const BwdGroup& g, int B, int T, int flags) {
    Shape sh;
    if (!g.bf16 || (flags & M3T_SCAN_FP32) || !x6_scan_enabled() || T >= 65535 || !level_shape(g.d, g.n, B, sh)) return false;
    return sh.rt == 1 && (sh.nc == 2 || sh.nc == 4);
}

// the fp32-accurate backward scan runs its recurrent product as bf16x6 (gru_persist_bwd6_kernel) for H = 256 / 512 at 16
// rows per workgroup; M3T_SCAN_FP32 / M3T_SCAN_X6=0 keep the fp32-MFMA kernel (bit-identical to the per-step path)
bool persist_bwd_uses_x6(const BwdGroup& g, int B, int T, int flags) {
    Shape sh;
    if (g.bf16 || (flags & M3T_SCAN_FP32) || !x6_scan_enabled() || !level_shape(g.d, g.n, B, sh)) return false;
    return sh.rt == 1 && (sh.nc == 2 || sh.nc == 4);
}

// ---- progress marks (m3t_gru_scan_progress) ---------------------------------------------------------------------------------
// Armed by the caller for the NEXT scan call of the thread; consumed by the launch paths whose kernels carry the marks (the fp16x3
// forward kernels, the wide producer-split backward kernel); any other path refuses an armed call (M3T_EINVAL) rather than let the
// caller's consumers wait for signals that never come.  The library keeps, per counter pair, how many arrivals it has asked the device
// for so far (a shadow of the device counters: launches are issued in stream order and every armed launch adds a known amount).
struct ProgressArm { unsigned* ctr; int n; int tb[3]; unsigned* need; };
static thread_local ProgressArm g_prog = {nullptr, 0, {0, 0, 0}, nullptr};
struct ProgressPending { unsigned* ctr; unsigned up, down; };
static thread_local ProgressPending g_prog_pending = {nullptr, 0, 0};
struct ProgressTxn { void commit(); ~ProgressTxn(); };
static std::mutex g_prog_mu;
static std::unordered_map<uintptr_t, std::pair<unsigned, unsigned>> g_prog_total;      // counter address -> arrivals requested so far (up, down)
void persist_set_progress(unsigned* ctr, int n, const int* tb, unsigned* need) {
    g_prog.ctr = ctr; g_prog.n = n; g_prog.need = need;
    for (int i = 0; i < 3; ++i) g_prog.tb[i] = (tb && i < n) ? tb[i] : 0;
}
void persist_drop_progress() { g_prog.ctr = nullptr; g_prog.n = 0; g_prog.need = nullptr; }
bool persist_progress_armed() { return g_prog.ctr != nullptr; }
void persist_forget_progress(unsigned* ctr) {
    std::lock_guard<std::mutex> lock(g_prog_mu);
    if (ctr) g_prog_total.erase((uintptr_t)ctr); else g_prog_total.clear();
}
// fills ex.prog / nmarks / marks and the caller's `need` table; up[i]: scan i walks time upwards.  wg_per_scan: workgroups of one scan.
template <typename G>
static int apply_progress(const G& g, const bool* up, int wg_per_scan, int T, ExPtrs& ex) {
    if (!g_prog.ctr) return 0;
    const ProgressArm a = g_prog;
    persist_drop_progress();
    if (a.n < 1 || a.n > 3 || !a.need) return M3T_EINVAL;
    for (int k = 0; k < a.n; ++k)
        if (a.tb[k] < 4 || a.tb[k] > T - 4 || (k > 0 && a.tb[k] < a.tb[k - 1] + 4)) return M3T_EINVAL;      // (a signal trails its mark by two steps)
    int n_up = 0, n_down = 0;
    for (int i = 0; i < g.n; ++i) (up[i] ? n_up : n_down) += 1;
    ex.prog = a.ctr; ex.nmarks = a.n;
    for (int k = 0; k < a.n; ++k) { ex.marks[0][k] = a.tb[k]; ex.marks[1][k] = T - a.tb[a.n - 1 - k]; }
    std::lock_guard<std::mutex> lock(g_prog_mu);
    std::pair<unsigned, unsigned>& tot = g_prog_total[(uintptr_t)a.ctr];
    for (int k = 0; k < a.n; ++k) {
        a.need[k] = tot.first + (unsigned)(n_up * wg_per_scan * (k + 1));
        a.need[a.n + k] = tot.second + (unsigned)(n_down * wg_per_scan * (k + 1));
    }
    // the shadow totals move only once the launch has SUCCEEDED (ProgressTxn below; ADVICE r5: a launch that failed after this point -- an
    // exchange that could not be prepared, dyn < need, a stream-order error -- left host shadow and device counters apart for good, and
    // every later gate waited for a value that never came)
    g_prog_pending.ctr = a.ctr;
    g_prog_pending.up = (unsigned)(n_up * wg_per_scan * a.n);
    g_prog_pending.down = (unsigned)(n_down * wg_per_scan * a.n);
    return 0;
}
void ProgressTxn::commit() {
    if (!g_prog_pending.ctr) return;
    std::lock_guard<std::mutex> lock(g_prog_mu);
    std::pair<unsigned, unsigned>& tot = g_prog_total[(uintptr_t)g_prog_pending.ctr];
    tot.first += g_prog_pending.up; tot.second += g_prog_pending.down;
    g_prog_pending.ctr = nullptr;
}
ProgressTxn::~ProgressTxn() { g_prog_pending.ctr = nullptr; }      // (not committed: rolled back -- nothing was added)

// m3t_gru_bwd_prepare: the wide producer-split backward kernel's W_hh^T fragments, ahead of the scan (see persist_bwd_launch)
int persist_bwd_prepare(const float* const* w, int n, int H, int direct, float* const* out, hipStream_t s) {
    if (n <= 0) return 0;
    if (n > M3T_MAX_SCANS || !w || !out || H <= 0 || H % 256 != 0 || H > 512) return M3T_EINVAL;
    PrepBwd3pArgs pa;
    for (int i = 0; i < M3T_MAX_SCANS; ++i) {
        const int j = i < n ? i : 0;
        if (!w[j] || !out[j] || ((uintptr_t)out[j] % 16) != 0) return M3T_EINVAL;
        pa.w[i] = w[j]; pa.wf[i] = reinterpret_cast<unsigned short*>(out[j]); pa.inv[i] = out[j] + (size_t)4 * H * H;
    }
    wfrag_bwd3q_prep_kernel<<<dim3(H / 16, PREP3H_SPLIT, n), 256, 0, s>>>(pa, H, direct ? 1 : 0);
    M3T_LAUNCH_CHECK();
    return 0;
}

// the gate: one lane polls a progress counter until it has reached `need` (wrap-safe), then the kernel ends -- what follows it in its stream
// starts behind a kernel boundary (agent-scope acquire: MI355X_MICROARCH.md, "boundary") and reads what the signalling workgroups wrote
// back.  Bounded like every wait of the scans; giving up raises the sticky error word.
__global__ void progress_gate_kernel(const unsigned* ctr, unsigned need, int spin_limit, unsigned* err) {
    if (threadIdx.x != 0) return;
    for (int spins = 0;; ++spins) {
        unsigned v;
        asm volatile("global_load_dword %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(ctr) : "memory");
        if ((int)(v - need) >= 0) return;
        if (spins > spin_limit) { raise_spin(err, 0); return; }
        __builtin_amdgcn_s_sleep(32);
    }
}
int persist_wait_progress(const unsigned* ctr, unsigned need, hipStream_t s) {
    if (!ctr || !ensure_err_word()) return M3T_EINVAL;
    static const int spin_limit = poll_env_early("M3T_SCAN_SPIN_LIMIT", SPIN_LIMIT_DEFAULT);
    progress_gate_kernel<<<1, 64, 0, s>>>(ctr, need, spin_limit > 0 ? spin_limit : SPIN_LIMIT_DEFAULT, g_err_dev);
    M3T_LAUNCH_CHECK();
    return 0;
}

// M3T_SCAN_WIDE=0: keep one 16-unit tile per workgroup for the H = 512 levels in the fp16x3 mode (the round-3 geometry: 256 workgroups for
// the encoder level) instead of the wide kernels (two tiles per workgroup, half the workgroups)
static bool wide_enabled() {
    static int on = -1;
    if (on < 0) { const char* e = getenv("M3T_SCAN_WIDE"); on = (e && e[0] == '0') ? 0 : 1; }
    return on == 1;
}
static bool fwd_is_f16(const FwdGroup& g, int B, int T, int flags) {
    return persist_fwd_uses_x6(g, B, T, flags) && !g.bf16 && (flags & M3T_GEMM_F16X3) && m3t_f16x3_enabled();
}
// unit tiles per workgroup of the level's forward launch
static int fwd_uw(const FwdGroup& g, int B, int T, int flags, const Shape& sh) {
    return ((flags & M3T_SCAN_WIDE) && fwd_is_f16(g, B, T, flags) && (sh.nc == 4 || sh.nc == 2) && sh.rt == 1 && wide_enabled()) ? 2 : 1;
}

// M3T_SCAN_SPREAD: the shape of the level's forward launch with 8-clip row blocks, where that form applies -- the fp16x3 kernels, twice the
// groups still fit the CUs (level_shape); the launch path also requires that no progress marks are armed
// The doubled exchange tiles live in the exchange ARENA only (m3t_gru_scan_arena; the workspace region a launch without one falls back to is
// sized for 16-row blocks): `launching` also asks that this call has been handed one.
static bool spread_exchange_ok(const Shape& s8, int n, int H, int kind, size_t gran_bytes, bool launching) {
    if ((size_t)n * 2 * s8.nrb * (H / 16) * 256 * gran_bytes > ARENA_SIZE[kind]) return false;
    return !launching || (g_arena != nullptr && g_arena_bytes >= ARENA_BYTES && ((uintptr_t)g_arena % 16) == 0);
}
static bool fwd_spread(const FwdGroup& g, int B, int T, int flags, int uw, Shape& sh, bool launching) {
    if (!(flags & M3T_SCAN_SPREAD) || !fwd_is_f16(g, B, T, flags)) return false;
    Shape s8;
    if (!level_shape(g.d, g.n, B, s8, uw, true) || s8.rb != 8 || !spread_exchange_ok(s8, g.n, g.d[0].H, 1, 8, launching)) return false;
    sh = s8;
    return true;
}
// the same for the wide producer-split backward launch (the caller has established that the launch takes that kernel)
static bool bwd_spread(const BwdGroup& g, int B, int flags, Shape& sh, bool launching) {
    if (!(flags & M3T_SCAN_SPREAD)) return false;
    Shape s8;
    if (!level_shape(g.d, g.n, B, s8, 2, true) || s8.rb != 8 || !spread_exchange_ok(s8, g.n, g.d[0].H, 3, 16, launching)) return false;
    sh = s8;
    return true;
}

static int persist_fwd_launch_impl(const FwdGroup& g, const FragPtrs& fp, int B, int T, int flags, hipStream_t s);
int persist_fwd_launch(const FwdGroup& g, const FragPtrs& fp, int B, int T, int flags, hipStream_t s) {
    ProgressTxn txn;
    const int rc = persist_fwd_launch_impl(g, fp, B, T, flags, s);
    if (rc == 0) txn.commit();
    return rc;
}
static int persist_fwd_launch_impl(const FwdGroup& g, const FragPtrs& fp, int B, int T, int flags, hipStream_t s) {
    Shape sh;
    if (!level_shape(g.d, g.n, B, sh) || !ensure_err_word()) return M3T_EINVAL;
    const int uw = fwd_uw(g, B, T, flags, sh);
    if (uw > 1 && !level_shape(g.d, g.n, B, sh, uw)) return M3T_EINVAL;
    if (!persist_progress_armed()) fwd_spread(g, B, T, flags, uw, sh, true);
    {
        // round 4: a NARROW forward launch with fewer than 8 groups is XCD-aligned too (the fusion level: 4 groups of 32 fill 4 XCDs, exchange
        // served by L2: traffic 1.9x -> ~1.1x algorithmic, step 12.17 -> 12.10 ms).  Round 3 lost 0.3 ms with this placement because the
        // weight-gradient GEMMs beside the BACKWARD scans found CUs on four XCDs only; no GEMM runs beside a forward scan.
        if (uw == 1 && !sh.slot_map && sh.G < 8 && fwd_is_f16(g, B, T, flags)) {
            sh.slot_map = 1;
            sh.grid = 8 * (g.d[0].H / 16);
        }
    }
    ExPtrs ex;
    size_t bytes[M3T_MAX_SCANS];
    fill_exchange(g, fp, sh, 8, ex, bytes);
    if (flags & M3T_SCAN_FAULT) ex.fault_step = T / 2;
    {
        // sleep before a step's first gather attempt, in units of 64 cycles: adaptive (-1) in the bf16x6 forward scan, fixed 12 in
        // the fp32 forward scan (0 at H = 128); waves without cell math count it from the workgroup's publish (fp32 forward,
        // backward) -- the measured optima of rounds 1-2, formerly M3T_SCAN_POLL_*
        ex.poll_fixed = persist_fwd_uses_x6(g, B, T, flags) ? -1 : (sh.nc == 1 ? 0 : 12);
        ex.poll_align = persist_fwd_uses_x6(g, B, T, flags) ? 0 : 1;
        // fp16x3 forward at H = 256: the MFMA phase is so short that the waves without cell math reach the gather long before the
        // workgroup's publish, fail, and drive the common adaptive delay past what the cell-math waves need (2.63 us per step;
        // counted from the publish: 1.73; bf16x6: 1.83).  H = 512 is better without (2.55 vs 2.59, fusion level 2.28 vs 2.48).
        if (persist_fwd_uses_x6(g, B, T, flags) && !g.bf16 && (flags & M3T_GEMM_F16X3) && m3t_f16x3_enabled() && sh.nc == 2) ex.poll_align = 1;
        // 8-clip row blocks (M3T_SCAN_SPREAD): with half the load instructions a gather attempt returns sooner, and the adaptive delay settles
        // where most first attempts fail (2.57 us per step at 2 x H=512, the 16-row launch 2.28).  Fixed delays, measured at 4 .. 20: a plateau
        // of 1.81-1.87 (12: 1.81; wide 2.19 against 2.49); H = 256, counted from the publish: 8 -> 1.37 against 1.65 (NOTEBOOK.md R13)
        if (sh.rb == 8) {
            ex.poll_fixed = sh.nc == 2 ? 8 : 12;
            ex.poll_align = sh.nc == 2 ? 1 : 0;
        }
    }
    const bool x6 = persist_fwd_uses_x6(g, B, T, flags);
    if (persist_progress_armed()) {                        // progress marks: the fp16x3 forward kernels carry them
        if (!fwd_is_f16(g, B, T, flags)) { persist_drop_progress(); return M3T_EINVAL; }
        bool up[M3T_MAX_SCANS];
        for (int i = 0; i < g.n; ++i) up[i] = !g.d[i].reverse;
        const int e = apply_progress(g, up, sh.active / g.n, T, ex);
        if (e) return e;
    }
    { const int e = prepare_exchange(g, fp, sh, x6 ? 1 : 0, 8, x6 ? 65535ull : 0xffffffffull, T, ex, s); if (e) return e; }
    ++g_launches;
    if (x6) {
        // fp32 mode with M3T_GEMM_F16X3: the product from two fp16 terms (three MFMAs per k-step and gate) instead of three bf16 terms (six)
        const bool f16 = !g.bf16 && (flags & M3T_GEMM_F16X3) && m3t_f16x3_enabled();
        // round 4: the fp16x3 forward kernels build their fragments themselves (ex.inline_prep) -- no prep launch on the chain in front of
        // the scan (12.15 -> 12.10 ms per C3 step); a W_hh that is not 16-byte aligned keeps the prep kernel
        bool inline_ok = f16;
        for (int i = 0; i < g.n; ++i) inline_ok = inline_ok && ((uintptr_t)g.d[i].w_hh % 16) == 0;
        ex.inline_prep = inline_ok ? 1 : 0;
        if (f16 && !inline_ok) {                                             // W_hh -> B-operand fragments: one launch for the level
            Prep3hArgs pa;
            const int H = g.d[0].H;                                           // (level_shape: every scan of the level has the same H)
            for (int i = 0; i < g.n; ++i) {
                pa.w_hh[i] = g.d[i].w_hh; pa.wf[i] = reinterpret_cast<unsigned short*>(fp.wfrag[i]); pa.inv[i] = fp.wfrag[i] + (size_t)4 * H * H;
            }
            for (int i = g.n; i < M3T_MAX_SCANS; ++i) { pa.w_hh[i] = pa.w_hh[0]; pa.wf[i] = pa.wf[0]; pa.inv[i] = pa.inv[0]; }
            wfrag3h_prep_kernel<<<dim3(H / 16, PREP3H_SPLIT, g.n), 256, 0, s>>>(pa, H);
        }
        for (int i = 0; i < g.n && !f16; ++i) {
            const int H = g.d[i].H;
            wfrag6_prep_kernel<<<prep_blocks(H), 256, 0, s>>>(g.d[i].w_hh, reinterpret_cast<unsigned short*>(fp.wfrag[i]), H, g.bf16);
        }
        M3T_LAUNCH_CHECK();
        if (f16 && uw == 2) {
            const size_t need = (size_t)2 * NW * 2 * 3 * 16 * (UB + 1) * sizeof(float)           // the kernel's partial sums (RED_FLOATS)
                                + (size_t)2 * 2 * 272 * 36;                                      // + the staging slots (sx, so, sh)
            return launch_scan(sh.rb == 8 ? (sh.nc == 2 ? gru_persist_fwd6_kernel<2, true, 2, 8> : gru_persist_fwd6_kernel<4, true, 2, 8>)
                                          : (sh.nc == 2 ? gru_persist_fwd6_kernel<2, true, 2> : gru_persist_fwd6_kernel<4, true, 2>),
                               sh, need, g, fp, ex, B, T, s);
        }
        if (f16 && sh.rb == 8)
            return launch_scan(sh.nc == 2 ? gru_persist_fwd6_kernel<2, true, 1, 8> : gru_persist_fwd6_kernel<4, true, 1, 8>, sh, 0, g, fp, ex, B, T, s);
        if (f16) return launch_scan(sh.nc == 2 ? gru_persist_fwd6_kernel<2, true> : gru_persist_fwd6_kernel<4, true>, sh, 0, g, fp, ex, B, T, s);
        return launch_scan(sh.nc == 2 ? gru_persist_fwd6_kernel<2> : gru_persist_fwd6_kernel<4>, sh, 0, g, fp, ex, B, T, s);
    }
    return launch_scan(pick_fwd(sh), sh, 0, g, fp, ex, B, T, s);
}

// M3T_SCAN_BWD3P=0: the six-product backward scan (consumer-side split) for the H = 512 / 256 levels also in the fp16x3 mode, instead of the
// producer-split kernel (gru_persist_bwd3q_kernel; DESIGN.md section 7 / NOTEBOOK.md section 5e)
static bool bwd3p_enabled() {
    static int on = -1;
    if (on < 0) { const char* e = getenv("M3T_SCAN_BWD3P"); on = (e && e[0] == '0') ? 0 : 1; }
    return on == 1;
}

static int persist_bwd_launch_impl(const BwdGroup& g, const FragPtrs& fp, int B, int T, int flags, hipStream_t s);
int persist_bwd_launch(const BwdGroup& g, const FragPtrs& fp, int B, int T, int flags, hipStream_t s) {
    ProgressTxn txn;
    const int rc = persist_bwd_launch_impl(g, fp, B, T, flags, s);
    if (rc == 0) txn.commit();
    return rc;
}
static int persist_bwd_launch_impl(const BwdGroup& g, const FragPtrs& fp, int B, int T, int flags, hipStream_t s) {
    Shape sh;
    if (!level_shape(g.d, g.n, B, sh) || !ensure_err_word()) return M3T_EINVAL;
    ExPtrs ex;
    size_t bytes[M3T_MAX_SCANS];
    const bool b16 = persist_bwd_uses_16(g, B, T, flags);
    fill_exchange(g, fp, sh, b16 ? 8 : 16, ex, bytes);
    if (flags & M3T_SCAN_FAULT) ex.fault_step = T / 2;
    {
        ex.poll_fixed = 12;
        ex.poll_align = 1;
    }
    // fp32 mode with M3T_GEMM_F16X3: the producer-split kernel (two fp16 terms per value in the granule, 24-bit tags + the tile's exponent)
    // an H = 256 level that asks for the wide form (round 4: every backward level does) takes the wide producer-split kernel too: 32
    // workgroups, one group per XCD, L2-served exchange -- in the C3 step the audio stack's backward scans (beside the heavy level's)
    // 0.80 / 0.96 -> 0.70 / 0.86 ms, the step 12.25 -> 12.15 ms; the NARROW producer-split form lost at H = 256 in round 3 (2.40 -> 2.50)
    const bool wide256 = (flags & M3T_SCAN_WIDE) && sh.rt == 1 && wide_enabled();
    // (round 5: the producer-split form exists only as the WIDE kernel; a launch that does not ask for it -- M3T_SCAN_WIDE=0 -- runs the six-product kernel)
    const bool p3 = !b16 && persist_bwd_uses_x6(g, B, T, flags) && (flags & M3T_GEMM_F16X3) && m3t_f16x3_enabled() && bwd3p_enabled() &&
                    wide256 && (sh.nc == 4 || sh.nc == 2) && (unsigned long long)T + 1 < 0xffffffull;
    const int uw = p3 ? 2 : 1;      // wide workgroups: two unit tiles each, half the grid
    if (uw > 1) {
        if (!level_shape(g.d, g.n, B, sh, uw)) return M3T_EINVAL;
        if (!persist_progress_armed()) bwd_spread(g, B, flags, sh, true);      // (M3T_SCAN_SPREAD: 8-clip row blocks)
        ex.slot_map = sh.slot_map;
    }
    if (persist_progress_armed()) {                        // progress marks: the wide producer-split backward kernel carries them
        if (!(p3 && uw == 2)) { persist_drop_progress(); return M3T_EINVAL; }
        bool up[M3T_MAX_SCANS];
        for (int i = 0; i < g.n; ++i) up[i] = g.d[i].reverse != 0;      // (the backward scan of a forward-direction GRU walks time downwards)
        const int e = apply_progress(g, up, sh.active / g.n, T, ex);
        if (e) return e;
    }
    { const int e = prepare_exchange(g, fp, sh, b16 ? 2 : 3, b16 ? 8 : 16, b16 ? 65535ull : (p3 ? 0xffffffull : 0xffffffffull), T, ex, s, p3 ? 1 : 0); if (e) return e; }
    ++g_launches;
    if (p3) {                                                                // (p3 implies uw == 2) the wide form: 32-deep MFMAs over producer pairs, memory-order hand-over
        const int H = g.d[0].H;                                               // (level_shape: one H per level)
        bool ready = true;                                                   // round 5: fragments prepared ahead of time (m3t_gru_bwd_prepare)
        for (int i = 0; i < g.n; ++i) ready = ready && g.d[i].wfrag != nullptr && ((uintptr_t)g.d[i].wfrag % 16) == 0;
        FragPtrs fq = fp;
        if (ready) {
            for (int i = 0; i < g.n; ++i) fq.wfrag[i] = const_cast<float*>(g.d[i].wfrag);
        } else {
            PrepBwd3pArgs pa;
            for (int i = 0; i < M3T_MAX_SCANS; ++i) {
                const int j = i < g.n ? i : 0;
                pa.w[i] = g.d[j].w_hh_t; pa.wf[i] = reinterpret_cast<unsigned short*>(fp.wfrag[j]); pa.inv[i] = fp.wfrag[j] + (size_t)4 * H * H;
            }
            wfrag_bwd3q_prep_kernel<<<dim3(H / 16, PREP3H_SPLIT, g.n), 256, 0, s>>>(pa, H, (flags & M3T_SCAN_WHH) ? 1 : 0);
            M3T_LAUNCH_CHECK();
        }
        const BwdKernel kq = sh.rb == 8 ? (sh.nc == 2 ? gru_persist_bwd3q_kernel<2, false, 8> : gru_persist_bwd3q_kernel<4, false, 8>)
                             : sh.nc == 2 ? gru_persist_bwd3q_kernel<2> : (ex.prof ? gru_persist_bwd3q_kernel<4, true> : gru_persist_bwd3q_kernel<4>);
        return launch_scan(kq, sh, (size_t)2 * 2 * 272 * 40, g, fq, ex, B, T, s);      // need: the staging slots (sin4, sout, sin2)
    }
    if (b16) {
        for (int i = 0; i < g.n; ++i) {                                      // W_hh^T -> bf16 B-operand fragments
            const int H = g.d[i].H;
            wfrag_bwd16_prep_kernel<<<prep_blocks(H), 256, 0, s>>>(g.d[i].w_hh_t, reinterpret_cast<unsigned short*>(fp.wfrag[i]), H, (flags & M3T_SCAN_WHH) ? 1 : 0);
        }
        M3T_LAUNCH_CHECK();
        return launch_scan(sh.nc == 2 ? gru_persist_bwd16_kernel<2> : gru_persist_bwd16_kernel<4>, sh, 0, g, fp, ex, B, T, s);
    }
    if (persist_bwd_uses_x6(g, B, T, flags)) {
        PrepBwd6Args pa;                                                      // W_hh -> bf16x3 B-operand fragments, every scan of the level
        const int H = g.d[0].H;                                               // (level_shape: one H per level)
        for (int i = 0; i < M3T_MAX_SCANS; ++i) {
            const int j = i < g.n ? i : 0;
            pa.w[i] = g.d[j].w_hh_t; pa.wf[i] = reinterpret_cast<unsigned short*>(fp.wfrag[j]);
        }
        wfrag_bwd6_prep_kernel<<<dim3(prep_blocks(H), g.n), 256, 0, s>>>(pa, H, (flags & M3T_SCAN_WHH) ? 1 : 0);
        M3T_LAUNCH_CHECK();
        return launch_scan(sh.nc == 2 ? gru_persist_bwd6_kernel<2> : gru_persist_bwd6_kernel<4>, sh, 0, g, fp, ex, B, T, s);
    }
    return launch_scan(pick_bwd(sh), sh, 0, g, fp, ex, B, T, s);
}

static thread_local hipEvent_t g_ev_start = nullptr, g_ev_end = nullptr;
void persist_set_events(hipEvent_t a, hipEvent_t b) { g_ev_start = a; g_ev_end = b; }
void persist_drop_events() { g_ev_start = g_ev_end = nullptr; }
void persist_record_start(hipStream_t s) { if (g_ev_start) { (void)hipEventRecord(g_ev_start, s); g_ev_start = nullptr; } }
void persist_record_end(hipStream_t s) { if (g_ev_end) { (void)hipEventRecord(g_ev_end, s); g_ev_end = nullptr; } }

static thread_local hipEvent_t g_after = nullptr;
void persist_set_after(hipEvent_t ev) { g_after = ev; }
void persist_drop_after() { g_after = nullptr; }
int persist_take_after(hipStream_t s) {
    if (!g_after) return 0;
    const hipError_t e = hipStreamWaitEvent(s, g_after, 0);
    g_after = nullptr;
    return (int)e;
}

void persist_set_arena(void* arena, size_t bytes) { g_arena = arena; g_arena_bytes = bytes; }
void persist_drop_arena() { g_arena = nullptr; g_arena_bytes = 0; }
void persist_forget_arena(void* arena) {
    std::lock_guard<std::mutex> lock(g_arena_mu);
    if (arena) g_arenas.erase((uintptr_t)arena); else g_arenas.clear();
}

int persist_launch_count() { return g_launches; }
void persist_count_launch() { ++g_launches; }

int persist_profile(unsigned long long* out6) {
    if (!g_prof || !out6) return M3T_EINVAL;
    return (int)hipMemcpy(out6, g_prof, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
}

}  // namespace m3t_gru

extern "C" int m3t_gru_persist_count(void) { return m3t_gru::persist_launch_count(); }

namespace m3t_gru {
// what m3t_gru_scan_fwd / _bwd would hold resident for one persistent launch (include/m3t_hip.h: m3t_gru_scan_workgroups)
int persist_workgroups(int n, int H, int B, int T, int flags, bool backward) {
    if (n < 1 || n > M3T_MAX_SCANS || H < 1 || B < 1 || T < 2 || (flags & M3T_SCAN_NO_PERSIST) || !persist_enabled()) return 0;
    Shape sh;
    if (backward) {
        BwdGroup g;
        std::memset(&g, 0, sizeof(g));
        g.n = n; g.bf16 = (flags & M3T_BF16) ? 1 : 0;
        for (int i = 0; i < n; ++i) { g.d[i].H = H; g.d[i].gates = reinterpret_cast<const float*>(16); g.d[i].w_hh_t = reinterpret_cast<const float*>(16); }
        if (solo_bwd_ok(g, B, T, flags) || !level_shape(g.d, g.n, B, sh)) return 0;
        const bool b16 = persist_bwd_uses_16(g, B, T, flags);
        const bool wide256 = (flags & M3T_SCAN_WIDE) && sh.rt == 1 && wide_enabled();
        const bool p3 = !b16 && persist_bwd_uses_x6(g, B, T, flags) && (flags & M3T_GEMM_F16X3) && m3t_f16x3_enabled() && bwd3p_enabled() &&
                        wide256 && (sh.nc == 4 || sh.nc == 2) && (unsigned long long)T + 1 < 0xffffffull;
        if (p3 && !level_shape(g.d, g.n, B, sh, 2)) return 0;
        if (p3) bwd_spread(g, B, flags, sh, false);
        return sh.active;
    }
    FwdGroup g;
    std::memset(&g, 0, sizeof(g));
    g.n = n; g.bf16 = (flags & M3T_BF16) ? 1 : 0;
    for (int i = 0; i < n; ++i) { g.d[i].H = H; g.d[i].w_hh = reinterpret_cast<const float*>(16); }
    if (solo_fwd_ok(g, B, T, flags) || !level_shape(g.d, g.n, B, sh)) return 0;
    const int uw = fwd_uw(g, B, T, flags, sh);
    if (uw == 2 && !level_shape(g.d, g.n, B, sh, 2)) return 0;
    fwd_spread(g, B, T, flags, uw, sh, false);
    return sh.active;
}
}  // namespace m3t_gru

namespace m3t_gru {
// would the level's launch carry progress marks (m3t_gru_scan_progress)?  0 / 1.  Same decisions as persist_fwd_launch / persist_bwd_launch.
int persist_progress_ok(int n, int H, int B, int T, int flags, bool backward) {
    if (persist_workgroups(n, H, B, T, flags, backward) <= 0) return 0;
    Shape sh;
    if (backward) {
        BwdGroup g;
        std::memset(&g, 0, sizeof(g));
        g.n = n; g.bf16 = (flags & M3T_BF16) ? 1 : 0;
        for (int i = 0; i < n; ++i) { g.d[i].H = H; g.d[i].gates = reinterpret_cast<const float*>(16); g.d[i].w_hh_t = reinterpret_cast<const float*>(16); }
        if (!level_shape(g.d, g.n, B, sh)) return 0;
        const bool b16 = persist_bwd_uses_16(g, B, T, flags);
        const bool wide256 = (flags & M3T_SCAN_WIDE) && sh.rt == 1 && wide_enabled();
        const bool p3 = !b16 && persist_bwd_uses_x6(g, B, T, flags) && (flags & M3T_GEMM_F16X3) && m3t_f16x3_enabled() && bwd3p_enabled() &&
                        wide256 && (sh.nc == 4 || sh.nc == 2) && (unsigned long long)T + 1 < 0xffffffull;
        return p3 ? 1 : 0;
    }
    FwdGroup g;
    std::memset(&g, 0, sizeof(g));
    g.n = n; g.bf16 = (flags & M3T_BF16) ? 1 : 0;
    for (int i = 0; i < n; ++i) { g.d[i].H = H; g.d[i].w_hh = reinterpret_cast<const float*>(16); }
    return fwd_is_f16(g, B, T, flags) ? 1 : 0;
}
}  // namespace m3t_gru

extern "C" int m3t_gru_scan_workgroups(int n_scans, int H, int B, int T, int flags, int backward) {
    return m3t_gru::persist_workgroups(n_scans, H, B, T, flags, backward != 0);
}

extern "C" int m3t_gru_poll_error(void) { return m3t_gru::persist_poll_error(); }

extern "C" int m3t_gru_error_reset(void) { m3t_gru::persist_reset_error(); return 0; }

extern "C" int m3t_gru_error_defer(int on) { m3t_gru::persist_set_defer(on); return 0; }

extern "C" int m3t_gru_inject_error(void* stream) { return m3t_gru::persist_inject_error((hipStream_t)stream); }

extern "C" int m3t_gru_persist_owner(void) { return m3t_gru::persist_owner_state(); }

extern "C" int m3t_gru_scan_events(void* start, void* end) {
    m3t_gru::persist_set_events((hipEvent_t)start, (hipEvent_t)end);
    return 0;
}

extern "C" int m3t_gru_scan_arena(void* arena, size_t bytes) {
    m3t_gru::persist_set_arena(arena, bytes);
    return 0;
}

extern "C" int m3t_gru_scan_arena_reset(void* arena) {
    m3t_gru::persist_forget_arena(arena);
    return 0;
}

extern "C" int m3t_gru_scan_progress(unsigned* counters, int n_marks, const int* time_bounds, unsigned* need) {
    if (!counters) { m3t_gru::persist_drop_progress(); return 0; }
    if (n_marks < 1 || n_marks > 3 || !time_bounds || !need || ((uintptr_t)counters % 8) != 0) return M3T_EINVAL;
    m3t_gru::persist_set_progress(counters, n_marks, time_bounds, need);
    return 0;
}

extern "C" int m3t_gru_scan_progress_reset(unsigned* counters) {
    m3t_gru::persist_forget_progress(counters);
    return 0;
}

extern "C" int m3t_gru_scan_progress_ok(int n_scans, int H, int B, int T, int flags, int backward) {
    return m3t_gru::persist_progress_ok(n_scans, H, B, T, flags, backward != 0);
}

extern "C" int m3t_stream_wait_progress(const unsigned* counter, unsigned need, void* stream) {
    return m3t_gru::persist_wait_progress(counter, need, (hipStream_t)stream);
}

extern "C" size_t m3t_gru_bwd_prepare_floats(int H) { return H > 0 ? (size_t)4 * H * H + 64 : 0; }

extern "C" int m3t_gru_bwd_prepare(const float* const* w, int n, int H, int whh_direct, float* const* out, void* stream) {
    return m3t_gru::persist_bwd_prepare(w, n, H, whh_direct, out, (hipStream_t)stream);
}

extern "C" int m3t_gru_scan_after(void* event) {
    m3t_gru::persist_set_after((hipEvent_t)event);
    return 0;
}

extern "C" int m3t_gru_persist_profile(unsigned long long* out6) {
    return m3t_gru::persist_profile(out6);
}
