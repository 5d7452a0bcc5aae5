// What the persistent scan kernels of gru_persist.hip share: the exchange state, a workgroup's place in the launch, the gather's
// skeleton, the publish, and the envelopes around the six step bodies (gru_persist_{fwd,fwd6,bwd,bwd6,bwd16,bwd3q}_step.inc).  Each piece
// stands once, under its one explanation.  What differs between the kernels on purpose -- how a wave loads and tag-checks its peers'
// granules, how it multiplies them, how it packs the granule it publishes -- stays in the kernel's own step file; nothing here chooses
// between them.  Pieces are functions where hipcc then emits the instructions it emitted for the written-out text, and macros where they
// declare a kernel's locals under the names the step bodies use or must keep an inline-asm operand list in the kernel's own scope
// (tools/scan_isa_diff.py compares the machine code of every kernel against a parent commit).
#pragma once
#include "gru_common.h"

namespace m3t_gru {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct ExPtrs {
    void* gran[M3T_MAX_SCANS];       // exchange granules: [2 slots][row block][unit block][RT*256]
    size_t slot[M3T_MAX_SCANS];      // granules per slot
    int poll_fixed;                  // >= 0: fixed poll delay (x 64 cycles); < 0: adapted per workgroup
    int poll_align;                  // 1: waves without cell math count the delay from the workgroup's publish
    int spin_limit;                  // gather attempts before a workgroup gives up (raises the error word, finishes with garbage)
    int fault_step;                  // fault injection (flag M3T_SCAN_FAULT): workgroup 0 does not publish this step; -1 = never
    unsigned long long* prof;        // optional in-kernel stamps (M3T_SCAN_PROF=1): 6 phase sums of workgroup 0, wave 0 (M3T_SCAN_PROF=2: wave 4, a wave without cell math)
    int prof_tid;
    int slot_map;                    // 1: persist_map's XCD-slot mapping (grid = 8 * ceil(G/8) * H/16), 0: gid = b % G
    unsigned long long* hs;          // placement-handshake table (arena), or nullptr: no L2-served exchange
    unsigned hs_tag;
    int inline_prep;                 // 1: the kernel builds its W_hh fragments itself from the parameter (no prep launch in front of it)
    unsigned tag_base;               // tags of this launch are tag_base + step + 1 (launch-unique inside an exchange arena: no memset per launch)
    // progress marks (m3t_gru_scan_progress, round 5): consumers of a scan's results need not wait for the launch to end.  prog[0] counts
    // for the scans that walk time upwards, prog[1] for those that walk it downwards; when a workgroup's results of every step < marks[dir][k]
    // are in memory and visible device-wide it adds 1 to its counter (gru_persist_fwd6_kernel / gru_persist_bwd3q_kernel only)
    unsigned* prog;
    int nmarks;
    int marks[2][3];
};

// Progress marks, the two halves of a signal (see ExPtrs.prog).  Results of step k leave a workgroup during step k or k + 1 (the memory-order
// hand-over stores one step late) and have been acknowledged once every wave has passed the gather's `s_waitcnt vmcnt(0)` of step k + 2 at the
// latest -- so: after the BARRIER of step mark + 1 one wave starts the write-back of its XCD's L2 (plain stores stay there:
// MI355X_MICROARCH.md, inter-workgroup visibility), which retires in order in front of that wave's next gather (its `s_waitcnt vmcnt(0)`);
// at the TOP of step mark + 3 -- in front of the gather, where the kernels have registers to spare (behind it the wide forward kernel
// spilled three VGPRs for the atomic's operands) -- the same wave raises the counter.  The write-back overlaps the poll delay and the
// gather's round trip: nothing waits for it.
#define M3T_MARK_STATE()                                                                                         \
    const int mdir = MARK_ASC ? 0 : 1;                                                                           \
    /* (three scalars and selects: a dynamically indexed copy of ex.marks would live in scratch) */               \
    const int mark0 = MARK_ASC ? ex.marks[0][0] : ex.marks[1][0], mark1 = MARK_ASC ? ex.marks[0][1] : ex.marks[1][1],  \
              mark2 = MARK_ASC ? ex.marks[0][2] : ex.marks[1][2];                                                \
    const int nmarks = ex.prog != nullptr ? ex.nmarks : 0;                                                       \
    /* the signalling wave as a SCALAR (the wide kernels sit at 256 VGPRs: a per-lane predicate inside the loop spilled three of them) */ \
    const bool mark_wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) == NW - 1;                           \
    const int mark_off = __builtin_amdgcn_readfirstlane(mdir * 4);    /* byte offset of this scan's counter (an "s" operand that is a select of pointers lands in VGPRs) */ \
    int mk = 0, sig_step = nmarks > 0 ? mark0 + 1 : -1
#define M3T_MARK_AT(k_) ((k_) >= nmarks ? -2 : ((k_) == 0 ? mark0 : ((k_) == 1 ? mark1 : mark2)))
// (one lane adds: exec is narrowed inside the asm; address from SGPRs, operands defined inside: nothing for hipcc to keep in loop-long VGPRs)
#define M3T_MARK_STEP_TOP(step_)                                                                                 \
    do {                                                                                                         \
        if ((step_) == sig_step + 2 && sig_step >= 0) {                                                          \
            if (mark_wave) {                                                                                     \
                unsigned z_, o_;                                                                                 \
                unsigned long long sv_;                                                                          \
                asm volatile("s_mov_b64 %2, exec\n\ts_mov_b64 exec, 1\n\tv_mov_b32 %0, %4\n\tv_mov_b32 %1, 1\n\t" \
                             "global_atomic_add %0, %1, %3\n\ts_mov_b64 exec, %2"                                \
                             : "=&v"(z_), "=&v"(o_), "=&s"(sv_) : "s"(ex.prog), "s"(mark_off) : "memory");       \
            }                                                                                                    \
            ++mk;                                                                                                \
            sig_step = M3T_MARK_AT(mk) + 1;                                                                      \
        }                                                                                                        \
    } while (0)
// (buffer_wbl2 is one cache operation per WAVE instruction, whatever the lanes)
#define M3T_MARK_AFTER_BARRIER(step_)                                                                            \
    do {                                                                                                         \
        if ((step_) == sig_step && mark_wave) asm volatile("buffer_wbl2 sc1" ::: "memory");                      \
    } while (0)

// Polling for the peers' granules.  A gather attempt is a full round trip (~1 us) and the next attempt is only issued
// when it has returned, so an attempt that leaves just before the data becomes visible costs a whole extra round trip --
// and the attempt issued right after a workgroup's own publish is always that attempt (the peers are still in their cell
// phase).  Every wave therefore sleeps `poll_delay` x 64 cycles before its first attempt.  Measured with fixed delays
// (M3T_SCAN_POLL_FWD6 / _FWD / _BWD = n, tools/scan_bench.py, H=512, three boxes): bf16x6 forward 3.1 -> 2.3 us per step
// at 16-24 units; backward 4.8-5.1 -> 3.9-4.7 at 12-18 (the gain varies from box to box, it was never negative); fp32
// forward 4.9 -> 4.2-4.4 at 12-18, nothing at H=128; all worse again beyond ~24.  Policy:
//   * bf16x6 forward: adaptive, one delay per workgroup (the step ends when the slowest of the 8 waves has its data, so
//     per-wave controllers that each sit at their own edge fail somewhere almost every step): a wave whose first attempt
//     failed sets a flag in LDS, after the step's barrier every wave reads it and moves the common delay +2 on a failure,
//     -1 every eighth step otherwise.  It finds the best fixed value (2.3 / 2.6 / 1.76 us at 2x512 / 4x512 / 2x256).
//   * backward and fp32 forward: fixed (12 units; 0 for the fp32 forward at H=128); in the backward scan the four waves
//     that do no cell math arrive at the gather a cell phase early, and their first attempt then fails and their second
//     returns after the cell-math waves' well-timed first one (in-kernel stamps: the cell-math waves waited 0.84 us at
//     the step's barrier): they first wait in LDS for thread 0's "published" mark, so every wave counts the delay from
//     the workgroup's own publish (M3T_SCAN_POLL_ALIGN; backward 4.7 -> 4.2 us per step on the boxes where it was not
//     already there; no gain for the adaptive bf16x6 forward, which finds a delay that suits its early waves).  The same controller over-sleeps
//     them (5.1 us), as do its variants (per-wave; waves without cell math aligned to the workgroup's publish first; a
//     hill-climb on the s_memtime of 8-step windows is too noisy within 300 steps) -- the failure flag does not say
//     what a failure cost there.
constexpr int POLL_DELAY_INIT = 8, POLL_DELAY_MAX = 64;

// phase stamps: s_memtime deltas accumulated by one lane; a uniform scalar branch when profiling is off
#define M3T_STAMP(i)                                                         \
    do {                                                                     \
        if (stamp) { const long long now = clock64(); psum[i] += now - last; last = now; } \
    } while (0)
#define M3T_STAMP_STATE()                                                                                        \
    const bool stamp = ex.prof != nullptr && blockIdx.x == 0 && tid == ex.prof_tid;                              \
    long long psum[6] = {0, 0, 0, 0, 0, 0}, last = stamp ? clock64() : 0
#define M3T_STAMP_DUMP()                                                                                         \
    do {                                                                                                         \
        if (stamp)                                                                                               \
            for (int i = 0; i < 6; ++i) ex.prof[i] = (unsigned long long)psum[i];                                \
    } while (0)

// err[0]: step + 1 of the failing wait (for the message); err[1]: the STICKY flag the device-side guards read
// (m3t_grad_norm_scale, m3t_grad_poison).  Nothing but m3t_gru_error_reset() -- which the host may only call after it has
// synchronised the device -- ever clears either word, so work queued behind a dead scan sees the flag however far ahead
// of the GPU the host runs.
__device__ __forceinline__ void raise_spin(unsigned* err, int step) {
    __hip_atomic_store(err, (unsigned)step + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(err + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Block -> (group, unit block).  A group (one scan x one row block) is the set of workgroups that exchange h_t / dgh_t with each
// other every step.  Blocks b and b + 8 share an XCD (observed dispatch rule: blocks are dealt round-robin over the 8 XCDs), so
// slot = b % 8 names an XCD and a group lives entirely in one slot: group g sits in slot g % 8 (gpx = ceil(G / 8) groups per slot),
// its members are the blocks of that slot.  The launch has 8 * gpx * (H / 16) blocks; blocks of slots that host no group exit at
// once.  Placement is speed only -- persist_handshake() below checks it and falls back -- never correctness.
__device__ __forceinline__ bool persist_map(int b, int G, int slot_map, int& gid, int& ub) {
    if (!slot_map) { gid = b % G; ub = b / G; return true; }      // plain round-robin: a group spans XCDs unless G % 8 == 0
    const int slot = b & 7, j = b >> 3, gpx = (G + 7) >> 3;
    gid = slot + 8 * (j % gpx);
    ub = j / gpx;
    return gid < G;
}

// Placement handshake, once per launch (needs the exchange arena): every workgroup publishes the id of the XCD it runs on
// (HW_REG_XCC_ID) as a tagged 8-byte granule with an agent-scope store, wave 0 gathers the ids of its group's members with
// agent-scope loads (the one exchange of the launch that must not depend on placement) and all members reach the same verdict:
// if they all share one XCD, the group's granules may travel through that XCD's L2 -- PLAIN stores (write-through, the line stays
// in L2) read by the same `sc1` loads (which bypass only the reader's L1) -- instead of through the memory side.  Measured
// (rocprofv3 FETCH_SIZE / WRITE_SIZE): the 4 x H=512 backward launch 2.0 -> 1.4 GB of HBM / fabric traffic (algorithmic 0.94), the
// scorers' 0.45 -> 0.30 GB; step time -1 % (the steps no longer wait on the gather).  A group that spans XCDs keeps sc1 stores: a
// reader's L2 could hold a stale copy of a line another XCD rewrote.  Stale or missing data can only ever delay a consumer (tags),
// so a wrong verdict would end in the bounded-spin error, not in wrong numbers.
constexpr int HS_STRIDE = 32;                          // granules per group in the handshake table (H / 16 <= 32 members)
__device__ __forceinline__ int persist_handshake(const ExPtrs& ex, int gid, int ub, int members, int tid, unsigned* err) {
    __shared__ int s_l2;
    if (ex.hs == nullptr) return 0;
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 0xfu;       // HW_REG_XCC_ID[3:0]
    unsigned long long* hs = ex.hs + (size_t)gid * HS_STRIDE;
    if (tid == 0) {
        const unsigned long long g = ((unsigned long long)ex.hs_tag << 32) | xcc;
        asm volatile("global_store_dwordx2 %0, %1, off sc1" :: "v"(hs + ub), "v"(g) : "memory");
    }
    if (tid < 64) {
        const int lane = tid;
        const unsigned long long* q = hs + (lane < members ? lane : 0);
        bool same = true;
        int spins = 0;
        for (;;) {
            unsigned long long v;
            asm volatile("global_load_dwordx2 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(q) : "memory");
            const bool ok = (unsigned)(v >> 32) == ex.hs_tag;
            same = (unsigned)v == xcc;
            if (__all(ok)) break;
            if (++spins > ex.spin_limit) { same = false; if (lane == 0) raise_spin(err, 0); break; }
            __builtin_amdgcn_s_sleep(2);
        }
        const bool all_same = __all(same);
        if (lane == 0) s_l2 = all_same ? 1 : 0;
    }
    __syncthreads();
    return s_l2;
}

// ------------------------------------------------------------------------------------------------ a workgroup's prologue
// Who this workgroup is: thread / lane / wave, its group `gid` and unit block (named UBN: `ub`, or `ubw` in the wide kernels, whose
// threads derive their own `ub` from it), the scan `s` and row block `rb` of the group.  A block of an XCD slot that hosts no group of
// this launch leaves the kernel here.
#define M3T_PERSIST_WHO(UBN)                                                                                     \
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;                                               \
    int gid, UBN;                                                                                                \
    if (!persist_map((int)blockIdx.x, G, ex.slot_map, gid, UBN)) return;                                         \
    const int s = gid / nrb, rb = gid % nrb
// The poll state (see POLL_DELAY_INIT above) and the handshake's verdict.  `dead`: this wave has hit the spin limit and no longer waits;
// poll_fail: by step parity, first read after the first barrier; pub_step: the steps this workgroup has published (thread 0's mark;
// M3T_GATHER_DELAY below waits for it); l2mode 1: this group shares one XCD's L2 (publish with plain stores).
// (gru_persist_bwd3q_kernel writes its own: all its waves do cell math, so it has no pub_step -- and a macro cut in two around that
// one line changed the order of the stores and with it every forward kernel's register allocation.)
#define M3T_PERSIST_POLL_STATE(UBN, MEMBERS)                                                                     \
    bool dead = false;                                                                                           \
    int poll_delay = ex.poll_fixed >= 0 ? ex.poll_fixed : POLL_DELAY_INIT;                                       \
    __shared__ unsigned poll_fail[2];                                                                            \
    __shared__ int pub_step;                                                                                     \
    const int l2mode = persist_handshake(ex, gid, UBN, MEMBERS, tid, err);                                       \
    if (tid == 0) pub_step = 0;                                                                                  \
    if (tid < 2) poll_fail[tid] = 0

// Order of a step: gather (loads only, inline asm: all loads of the pass in flight, ONE explicit wait -- left to
// hipcc the loads were issued and waited for in groups) -> MFMA -> LDS partials -> barrier -> reduce + cell math ->
// publish -> [results to HBM, next step's inputs from HBM].  The HBM traffic is issued after the publish, so it is in
// flight while the peers' granules travel and is never waited for on the chain.

// ------------------------------------------------------------------------------------------------ gather
// In front of the first attempt: the poll delay.  Waves without cell math arrive a cell phase early; under ex.poll_align they count the
// delay from the workgroup's own publish (thread 0's mark in LDS) too, bounded like every wait.
// (macros: with either wait in a function of its own hipcc placed the loop bounds differently in the forward kernels)
#define M3T_POLL_SLEEP()                                                                                         \
    for (int z = 0; z < poll_delay; ++z) __builtin_amdgcn_s_sleep(1)
#define M3T_GATHER_DELAY(step_)                                                                                  \
    do {                                                                                                         \
        if (!pw && (ex.poll_align & 1)) {                                                                        \
            int w = 0;                                                                                           \
            while (__hip_atomic_load(&pub_step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < (step_) && ++w < ex.spin_limit) __builtin_amdgcn_s_sleep(1); \
        }                                                                                                        \
        M3T_POLL_SLEEP();                                                                                        \
    } while (0)
// The bottom of the retry loop `for (;;) { <the kernel's loads, its s_waitcnt vmcnt(0), launder, ok = every tag matches>; M3T_GATHER_RETRY(ok, step); }`:
// leaves the loop when the whole wave has its granules -- or has given up: at the spin limit the wave raises the sticky error word, turns
// `dead` and from then on takes whatever the first attempt of a step returns (the scan finishes with garbage, bounded).  Uses the
// kernel's dead / spins / lane / err.  (A macro: returned from a function, "done" became a value that hipcc carried in SGPRs around the
// loop -- two to four s_mov more per step body in every forward kernel.)
#define M3T_GATHER_RETRY(ok_, step_)                                                                             \
    if (__all(ok_) || dead) break;                                                                               \
    if (++spins > ex.spin_limit) { dead = true; if (lane == 0) raise_spin(err, step_); break; }                  \
    __builtin_amdgcn_s_sleep(1)
// behind the loop: any wave's failed first attempt counts for the workgroup (the adaptive delay, M3T_POLL_ADAPT)
__device__ __forceinline__ void gather_note_fail(int spins, int lane, unsigned* fail) {
    if (spins > 0 && lane == 0) atomicOr(fail, 1u);
}
// In front of the cell phase, on every path.  Nothing is outstanding here on either path (the gather ended with this very wait; step 0
// had the prologue's): stated again so that EVERY path to the cell phase passes a vmcnt(0) behind the previous step's requests
// (tools/check_inflight.py)
__device__ __forceinline__ void cell_phase_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// Behind the step's barrier: the adaptive poll delay, one value per workgroup (ex.poll_fixed < 0; see POLL_DELAY_INIT).  now_ / next_: the
// step's parity and the next step's -- poll_fail[next_] is next written after the next gather and was last read before this barrier.
// (A macro: as a function it moved an address computation of the fp16x3 forward kernels' prologue.)
#define M3T_POLL_ADAPT(now_, next_, step_)                                                                       \
    do {                                                                                                         \
        if (ex.poll_fixed < 0) {                                                                                 \
            const bool wg_failed = poll_fail[now_] != 0;                                                         \
            if (tid == 0) poll_fail[next_] = 0;                                                                  \
            poll_delay = wg_failed ? min(poll_delay + 2, POLL_DELAY_MAX) : (((step_) & 7) == 0 && poll_delay > 0 ? poll_delay - 1 : poll_delay); \
        }                                                                                                        \
    } while (0)

// ------------------------------------------------------------------------------------------------ publish
// Does this thread publish step `step_`?  Not the last step's (nobody reads it); live_: `true`, or in the kernels with 8-clip row blocks
// the rows that exist (RB == ROWS || plive); and under fault injection (M3T_SCAN_FAULT) workgroup 0 stays silent for one step.  (A macro: as a function's result the condition reached hipcc as one value instead of its short-circuit
// branches, and the forward kernels' cell phase was scheduled differently.)
#define M3T_SCAN_PUBLISHES(step_, live_) ((step_) + 1 < T && (live_) && !((step_) == ex.fault_step && blockIdx.x == 0))
// The publishing store, the only store on the chain: ONE naturally aligned store per granule.  l2mode (persist_handshake): the group
// shares one XCD, a plain store leaves the line in its L2; else agent scope (sc1, write-through).
// (macros: as functions they changed the 8-clip wide forward kernels' register allocation)
#define M3T_PUBLISH8(q_, gq_)                                                                                    \
    do {                                                                                                         \
        unsigned long long* pq_ = (q_);                                                                          \
        if (l2mode) asm volatile("global_store_dwordx2 %0, %1, off" :: "v"(pq_), "v"(gq_) : "memory");           \
        else asm volatile("global_store_dwordx2 %0, %1, off sc1" :: "v"(pq_), "v"(gq_) : "memory");              \
    } while (0)
#define M3T_PUBLISH16(q_, gq_)                                                                                   \
    do {                                                                                                         \
        u32x4* pq_ = (q_);                                                                                       \
        if (l2mode) asm volatile("global_store_dwordx4 %0, %1, off" :: "v"(pq_), "v"(gq_) : "memory");           \
        else asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(pq_), "v"(gq_) : "memory");              \
    } while (0)
// thread 0's mark behind the publish: the other waves' poll delay counts from here (M3T_GATHER_DELAY)
// (a macro: as a function it changed the wide forward kernels' register allocation)
#define M3T_MARK_PUBLISHED(step_)                                                                                \
    do {                                                                                                         \
        if (tid == 0) __hip_atomic_store(&pub_step, (step_) + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); \
    } while (0)

// ------------------------------------------------------------------------------------------------ the kernel's end
// The last step's request for "the next step's inputs" is still in flight and invisible to hipcc (inline asm): a wave must
// not end with a load outstanding into registers that the next wave on this SIMD is about to own
__device__ __forceinline__ void scan_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// ------------------------------------------------------------------------------------------------ forward envelope
// x-projection of the step in (xr, xz, xn).  The next step's is requested right after this step's gather has completed (nothing else
// outstanding then) and has the rest of the step to arrive: requested after the publish it sat in front of the next
// gather's vmcnt(0) (vector-memory operations retire in order).  Inline asm, unconditional (lanes past the batch
// and the step past the end re-read a valid address), two register sets (A: even steps, B: odd; the loop body is
// included twice), defined by the next gather's vmcnt(0) and laundered there -- as in the backward kernels below, compiler-visible
// loads made hipcc wait for them mid-step.  `xq`: the kernel's clamped base pointer of its (row, unit).
#define M3T_FWD_LOAD_X(step_, XR, XZ, XN)                                                                             \
    do {                                                                                                               \
        const int ls_ = (step_) < T ? (step_) : T - 1;                                                                 \
        const float* xa_ = xq + (size_t)(d.reverse ? T - 1 - ls_ : ls_) * d.ldx;                                       \
        asm volatile("global_load_dword %0, %3, off\n\t"                                                               \
                     "global_load_dword %1, %4, off\n\t"                                                               \
                     "global_load_dword %2, %5, off"                                                                   \
                     : "=&v"(XR), "=&v"(XZ), "=&v"(XN) : "v"(xa_), "v"(xa_ + H), "v"(xa_ + 2 * H) : "memory");         \
    } while (0)
// step 0's, waited for twice: by the asm that defines the registers, and visibly to hipcc -- everything loaded so far is in registers
// before the loop, so hipcc places no vmcnt wait for the weight fragments inside the step
#define M3T_FWD_LOAD_X_FIRST()                                                                                         \
    M3T_FWD_LOAD_X(0, xrA, xzA, xnA);                                                                                  \
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(xrA), "+v"(xzA), "+v"(xnA) :: "memory");                                  \
    __builtin_amdgcn_s_waitcnt(0x0F70)                     /* vmcnt(0) */
// results of cell (B_, J_) at time t_ to HBM, off the chain: the hidden state, for the backward scan the gate record
// G4_ = (r, z, n, W_hn h + b_hn) (of vector type V4_: float4 from the cell's registers, f32x4 out of the wide kernels' LDS hand-over),
// and h_n behind the last step.  (A macro: G4_ is only put together where d.gates asks for it -- as a function's argument it was
// built in front of the branch and the fp32 forward kernels' cell phase came out in another order.)
#define M3T_FWD_STORE_RESULTS(B_, J_, t_, last_, V4_, G4_, hv_)                                                        \
    do {                                                                                                               \
        d.out[((size_t)(B_) * T + (t_)) * d.ldo + d.ooff + (J_)] = (hv_);                                              \
        if (d.gates) *reinterpret_cast<V4_*>(d.gates + ((size_t)(B_) * T + (t_)) * 4 * H + 4 * (size_t)(J_)) = (G4_); \
        if (d.h_n && (last_)) d.h_n[(size_t)(B_) * H + (J_)] = (hv_);                                                  \
    } while (0)

// ------------------------------------------------------------------------------------------------ backward envelope
// HBM traffic of a step and the chain.  Vector-memory operations retire in order, so everything a wave has issued
// before its gather loads sits in front of the gather's vmcnt(0): with the step's six result stores and the next
// step's three activation loads issued after the publish (the natural place), every step waited ~0.7 us for each
// group (tools/scan_bench.py ablation), and hipcc added a vmcnt(0) + register copies at the bottom of the step on
// top (2.4 of 5 us, in-kernel stamps).  Now: the results of step t are kept in registers and stored, and the
// activations of step t+1 are requested, right AFTER the gather of step t has completed -- they have the whole
// step (MFMAs, barrier, cell math, publish, the peers' latency) to retire before the next gather waits, and between
// the publish and the next gather a wave has nothing outstanding but the publish itself.  Two register sets (A for
// even steps, B for odd ones; the loop body is included twice) hold the activations; the loads are inline asm,
// UNCONDITIONAL (every thread, every step; lanes past the batch and the step past the end re-read a valid address):
// compiler-visible or conditional definitions make hipcc wait for them or merge them with copies that read
// registers still in flight.  A set is defined by the vmcnt(0) of the gather that precedes its use and laundered there.
// (B_, J_): the (clip, unit) this thread loads and stores for -- its cell's (pb, pj), or in gru_persist_bwd3q_kernel the memory-order
// cell (hb, hj) it hands over through LDS.  Declares the two sets, the clamped base pointers, step 0's loads with their two waits (the
// second visible to hipcc: no wait for the weight fragments inside the loop) and st_*, the results that store_results writes.
#define M3T_BWD_LOAD_STEP(step_, DOUT, G4, HPREV)                                                                     \
    do {                                                                                                               \
        const int ls_ = (step_) < T ? (step_) : T - 1;                                                                 \
        const int lt_ = d.reverse ? ls_ : T - 1 - ls_;                                                                 \
        const int ltp_ = ls_ < T - 1 ? (d.reverse ? lt_ + 1 : lt_ - 1) : lt_;                                          \
        asm volatile("global_load_dword %0, %3, off\n\t"                                                               \
                     "global_load_dwordx4 %1, %4, off\n\t"                                                             \
                     "global_load_dword %2, %5, off"                                                                   \
                     : "=&v"(DOUT), "=&v"(G4), "=&v"(HPREV)                                                            \
                     : "v"(pd0 + (size_t)lt_ * d.ldo), "v"(pg0 + (size_t)lt_ * 4 * H), "v"(ph0 + (size_t)ltp_ * d.ldo)  \
                     : "memory");                                                                                      \
    } while (0)
#define M3T_BWD_ENVELOPE(B_, J_)                                                                                       \
    float doutA, hprevA, doutB, hprevB;                                                                                \
    f32x4 g4A, g4B;                                    /* (r, z, n, W_hn h + b_hn) of this (row, unit, t) */           \
    const int pbc = B_ < B ? B_ : B - 1;                                                                               \
    const float* pd0 = d.dout + (size_t)pbc * T * d.ldo + d.ooff + J_;                                                 \
    const float* pg0 = d.gates + (size_t)pbc * T * 4 * H + 4 * (size_t)J_;                                             \
    const float* ph0 = d.out + (size_t)pbc * T * d.ldo + d.ooff + J_;                                                  \
    M3T_BWD_LOAD_STEP(0, doutA, g4A, hprevA);                                                                          \
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(doutA), "+v"(g4A), "+v"(hprevA) :: "memory");                             \
    __builtin_amdgcn_s_waitcnt(0x0F70);                /* vmcnt(0) */                                                  \
    float st_dr = 0.f, st_dz = 0.f, st_dn = 0.f, st_dnr = 0.f;                                                         \
    auto store_results = [&](int step_of) {                                                                            \
        const int t = d.reverse ? step_of : T - 1 - step_of;                                                           \
        float* gx = d.dgx + ((size_t)B_ * T + t) * d.ldg + d.goff;                                                     \
        gx[J_] = st_dr; gx[H + J_] = st_dz; gx[2 * H + J_] = st_dn;                                                    \
        float* gh = d.dgh + ((size_t)B_ * T + t) * H3;                                                                 \
        gh[J_] = st_dr; gh[H + J_] = st_dz; gh[2 * H + J_] = st_dnr;                                                   \
    }
// behind the loop: dh_0 and the clip's bias-gradient sums of this thread's cell
#define M3T_BWD_STORE_CARRY()                                                                                          \
    do {                                                                                                               \
        if (pok) d.dh[(size_t)pb * H + pj] = dh_carry;                                                                 \
        if (pok && d.db_part) {                                                                                        \
            float* q = d.db_part + (size_t)pb * 4 * H + pj;                                                            \
            q[0] = sb_r; q[H] = sb_z; q[2 * H] = sb_n; q[3 * H] = sb_nr;                                               \
        }                                                                                                              \
    } while (0)

}  // namespace

}  // namespace m3t_gru
