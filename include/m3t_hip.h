/*
 * m3t_hip.h -- C ABI of libm3t_hip.so: the MI355X (gfx950) kernels behind the M3T
 * (sailordiary/m3f.pytorch) forward/backward hot path.
 *
 * The reference has no native code and no operator registry: every function below
 * replaces a stock torch op that a reference module calls (cited per entry, paths
 * relative to the reference root).  The host side (the models package under m3f.pytorch_amd) keeps the
 * reference's Python module API and binds these entry points with ctypes
 * (INTEGRATION.md shows the stub a maintainer would add to the reference itself).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 unless stated; tensors are row-major;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); all work is
 *     enqueued on it, nothing synchronises, no allocation happens inside a call;
 *   - return value: 0 on success, otherwise a hipError_t (launch/config error) or
 *     M3T_EINVAL for bad arguments.  The caller raises;
 *   - kernels are deterministic: fixed reduction order, no floating-point atomics.
 */
#ifndef M3T_HIP_H
#define M3T_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3T_EINVAL 10001
#define M3T_MAX_SCANS 8
#define M3T_ESPIN 10002          /* a persistent scan gave up waiting for a peer workgroup (see m3t_gru_scan_fwd) */
#define M3T_SCAN_NO_PERSIST 1    /* m3t_gru_scan_* flags: take the launch-per-step path */
#define M3T_SCAN_WHH 8           /* m3t_gru_scan_bwd flags: every desc.w_hh_t points at the UNtransposed parameter w_hh [3H][H] (saves the caller
                                  * a transpose per direction in front of the scan); needs H % 16 == 0 and the workspace, else M3T_EINVAL */
#define M3T_SCAN_FP32 4          /* m3t_gru_scan_fwd flags: keep the recurrent product on fp32 MFMAs (bit-identical to the
                                  * launch-per-step kernels) instead of the fp32-accurate bf16x6 form */
#define M3T_SCAN_FAULT 16        /* m3t_gru_scan_* flags, FAULT INJECTION for tests: workgroup 0 of a persistent launch stays silent at step T/2,
                                  * so its peers run into their spin limit (env M3T_SCAN_SPIN_LIMIT lowers it) and the error path below runs */
#define M3T_SCAN_WIDE 32         /* m3t_gru_scan_* flags: run the level with WIDE workgroups where that form exists (H = 512 / 256 in the M3T_GEMM_F16X3 mode;
                                  * other levels ignore the flag): 16 rows x 32 units per workgroup instead of x 16 -- the same gather per workgroup,
                                  * half the workgroups (gru_v | gru_a, 4 scans x 32 clips: 128 instead of 256), each owning its CU, every group on one
                                  * XCD.  m3t.ops asks for it where it makes room for a SECOND persistent scan (the audio stack's scans run at the same
                                  * time as the gru_v | gru_a level's) and for every backward level (the wide backward kernel is no slower than the narrow
                                  * one on twice the CUs).  m3t_gru_scan_workgroups() says what a call would launch.  Same results as without the flag up to
                                  * fp32 rounding (the backward kernel scales per producer workgroup instead of per 16-unit tile). */
#define M3T_SCAN_SPREAD 64       /* m3t_gru_scan_* flags and m3t_gru_scan_workgroups: the caller schedules NOTHING beside this launch, so it may use CUs that
                                  * would stand idle: row blocks of 8 clips instead of 16 -- twice the groups, every workgroup gathers, publishes and does
                                  * cell math for 8 clips (half the bytes of the per-step gather; the 16-row MFMA tiles run half empty).  Taken only by the
                                  * fp16x3 forward kernels (narrow or wide) and the wide producer-split backward kernel, only while
                                  * n_scans * ceil(B / 8) * H / 16 fits the CUs, no progress marks are armed and the call has been handed an exchange
                                  * arena (m3t_gru_scan_arena: the doubled exchange tiles live there only); every other launch ignores the flag.
                                  * Forward results are bit-identical to the 16-row launch; backward results agree to fp32 rounding (a producer's scale
                                  * is taken over 8 rows).  m3t_gru_scan_workgroups() says what a call with an arena would launch. */
#define M3T_BF16 2               /* precision flag shared by m3t_sgemm (= M3T_GEMM_BF16), m3t_conv1d_* and m3t_gru_scan_*:
                                  * matmul operands rounded to bf16 (nearest even), fp32 accumulate, fp32 state/epilogue */
/* m3t_sgemm flags: BACKGROUND caps residency at one workgroup per CU (for GEMMs that run on a side stream
 * beside the latency-critical recurrence, e.g. weight gradients) */
#define M3T_GEMM_BACKGROUND 1
/* mixed precision (config C2 of BASELINE.json: "bf16, fp32 accumulate, fp32 master weights"): both operands are rounded
 * to bf16 (nearest even) before the product, accumulation and epilogue stay fp32.  Interior shapes then run ONE bf16
 * MFMA per tile step instead of the six of the fp32-accurate path. */
#define M3T_GEMM_BF16 2
/* "high" precision in the sense of torch.set_float32_matmul_precision('high'): each fp32 operand is treated as the sum of TWO
 * bfloat16 numbers (16 mantissa bits) and a product is four bf16 MFMAs with fp32 accumulation -- relative error ~2^-16 per term
 * instead of the 2^-23 of the default six-product form ('highest'), 1.3-1.5x the GEMM rate.  Opt-in (m3t.ops.precision("high"));
 * interior shapes only (others run exact fp32); M3T_GEMM_BF16 wins if both are set.  The recurrent scans ignore it. */
#define M3T_GEMM_HIGH 256
/* fp32-accurate products from TWO fp16 terms per operand and three MFMAs (a_hi b_hi + a_hi b_lo + a_lo b_hi, fp32 accumulate) instead
 * of three bf16 terms and six: fp16 holds 11 significant bits, so two terms carry 22 (+ the sign of the remainder) and the dropped
 * a_lo b_lo is <= 2^-22 relative; fp16's narrow exponent range is met by scaling each operand by the power of two that puts its
 * largest magnitude into [2^14, 2^15) -- the library measures max |A|, max |B| with one extra launch in front of the GEMM, on the
 * same stream, no host round trip -- and unscaling in the epilogue (exact).  Elements more than 2^17 below their operand's maximum
 * keep an absolute error of 2^-40 of that maximum instead of a relative one.  Measured against fp64 the mode is as accurate as the
 * six-product form (fewer fp32 accumulate roundings per k) -- DESIGN.md section 7.  Interior shapes only; the BF16 and HIGH flags
 * win if set.  m3t_gru_scan_fwd / m3t_gru_scan_bwd take the flag too: the forward persistent scans then form their recurrent product from
 * two fp16 terms (h is bounded by 1; W_hh is scaled per workgroup slice by the scan's own prep launch), the H = 512 backward
 * persistent scans run the producer-split kernel (two fp16 terms per exchanged value, scaled per producer tile); both fp32-accurate,
 * no slots needed.  Without the flag (or with env M3T_GEMM_F16X3=0) the scans keep the three-bf16-term products. */
#define M3T_GEMM_F16X3 1024
/* scheduling hint: other streams run persistent scans while this GEMM runs (the interleaved encoder level of m3t.ops._MultiBiGRU):
 * take gemm_x6.hip, whose phases only overlap across workgroups, instead of the software-pipelined gemm_x6d.hip -- the faster
 * kernel's higher request rate slows the scans' exchange by as much as it gains (measured: same step time, backward scans
 * 6.8 -> 7.7 ms by events).  Results are bit-identical either way. */
#define M3T_GEMM_BESIDE_SCAN 512
/* the caller promises that nothing else shares the chip while this GEMM runs.  Rounds 2-3 gave such calls a 256 x 256-tile kernel in the
 * six-product mode; it had no fp16x3 form and was removed in round 4 -- the flag is accepted and currently changes nothing. */
#define M3T_GEMM_EXCLUSIVE 8
/* m3t_conv3d_wgrad_taps only: x_cl and dy_cl are the m3t_f16x3_split images of the two operands under amax_x / amax_dy (both required, with
 * M3T_GEMM_F16X3) -- the forward walk and the data gradient's walk have made them already; the same sums, bit for bit (round 6). */
#define M3T_CONV_IMAGES 4096

/* Patch matrix (im2col) of a Conv3d input x [N, Ci, T, H, W] for the weight-gradient GEMM dW = dy^T P of the 3-D conv stems (reference
 * models/backbone.py:73-103,179-271,327-332; forward and data gradient stay on MIOpen): out [rows_pad, Kp] row-major, row = (n, t', h', w'),
 * column = (ci, kt, kh, kw) -- the order of weight.view(Co, -1) -- zero for the convolution's padding, for columns >= Ci kt kh kw and for
 * rows >= N T' H' W' (tile padding of the GEMM).  Kp % 4 == 0, out 16-B aligned.  amax_slot (optional): raised to the bits of max |P|
 * (a magnitude slot of m3t_sgemm_scaled, zero-initialised by the caller).  One launch. */
int m3t_im2col3d(const float* x, int N, int Ci, int T, int H, int W, int kt, int kh, int kw, int st, int sh, int sw,
                 int pt, int ph, int pw, float* out, long long rows_pad, int Kp, unsigned long long* amax_slot, void* stream);

/* The convolutions' data gradient WITHOUT a patch matrix (round 5; reference models/backbone.py:73-103,179-271, models/resnet.py:40-45): a tap-walk
 * contraction over CHANNELS-LAST grids,
 *   dst[(n, t, h, w)][cd] = sum over taps (jt, jh, jw) and channels cs of
 *                           src[(n, t + base_t + sign jt, h + base_h + sign jh, w + base_w + sign jw)][cs] * w_taps[((jt kh + jh) kw + jw) C_src + cs][cd]
 * with src rows on the grid To x Ho x Wo (terms outside it are zero) and dst rows on T x H x W: an implicit GEMM whose A tiles are whole-line loads
 * of shifted source rows (a 32-deep k tile lies inside one tap).  Data gradient of a stride-1 convolution with padding p: src = dy channels-last
 * [N T' H' W'][C_out] (backward has it for the weight gradient anyway), w_taps[(tap, co)][ci] = W[co][ci][tap], base = +p, sign = -1, dst = dx
 * channels-last.  (sign = +1, base = -p, w_taps[(tap, ci)][co]: the forward convolution over a channels-last input.)
 * C_dst % 64 == 0, C_src % 32 == 0, 16-B aligned (any number of rows N T H W since round 6: a ragged last tile reads zeros and is not stored); flags / amax as m3t_sgemm_scaled (NULL slots are measured); ws (optional):
 * split-K slabs for the layers whose tile count does not fill the chip (deterministic reduction, as m3t_sgemm). */
int m3t_conv3d_taps(const float* src, const float* w_taps, float* dst, int N, int C_src, int C_dst, int T, int H, int W,
                    int To, int Ho, int Wo, int kt, int kh, int kw, int base_t, int base_h, int base_w, int sign, int flags,
                    const unsigned long long* amax_src, const unsigned long long* amax_w, float* ws, size_t ws_bytes, float* dst_planes,
                    void* stream);

/* Operands split ONCE (round 5).  In the fp16x3 kernels every workgroup splits the operand tiles it stages -- each element as often as tiles read
 * it, five to six vector instructions per pair beside every MFMA.  m3t_f16x3_split writes the "P4" image of a K-contiguous operand x
 * [rows][cols] (ld): the 16 bytes of four consecutive values become {hi 0|1, hi 2|3, lo 0|1, lo 2|3}, the two fp16 terms of x * s, s the
 * power of two of `slot` (a raised magnitude slot of x) -- same size, same addressing as x.  A kernel that takes images copies them to LDS.
 * m3t_conv3d_taps_pre: m3t_conv3d_taps on the image of src and on w_img[cd][(tap, cs)] (the image of the K-contiguous weight matrix), under
 * the slots the images were made with.  Bit-identical to the in-kernel split (the same roundings).  cols % 4, ld % 4, 16-B aligned. */
int m3t_f16x3_split(const float* x, size_t rows, int cols, size_t ld, float* out, size_t ldo, const unsigned long long* slot, void* stream);
/* ... of a permuted view (round 6): out [R][T * Cc] <- the image of w[r * sR + t * sT + c * sC] -- a convolution's weights [Co][Ci][taps] as the
 * K-contiguous matrix a walk reads ([co][(tap, ci)]: R = Co, Cc = Ci, sR = Ci taps, sT = 1, sC = taps; [ci][(tap, co)]: R = Ci, Cc = Co, sR =
 * taps, sT = 1, sC = Ci taps) without a permute copy in front of the split.  Cc % 4 == 0, out 16-B aligned. */
int m3t_f16x3_split_perm(const float* w, size_t R, int T, int Cc, size_t sR, size_t sT, size_t sC, float* out, const unsigned long long* slot,
                         void* stream);
/* C[M,N] = act(A B^T + bias) (+ C) with A [M][K] and B [N][K] given as images (the NT product of m3t_sgemm_scaled, fp16x3 mode; M % 128 == 0,
 * N % 64 == 0, K % 32 == 0, both slots required) */
int m3t_sgemm_pre(int M, int N, int K, const float* A_img, int lda, const float* B_img, int ldb, float* C, int ldc,
                  const float* bias, int act, int accumulate, const unsigned long long* amax_a, const unsigned long long* amax_b, void* stream);
/* The WEIGHT operand as a staged image (round 5): m3t_f16x3_image_b writes w [N][K] (ld) as [N / 64][K / 8][term][64 rows][8 halves] -- the two
 * fp16 terms of w * s (s from `slot`), every (64-row block, k-octet, term) one contiguous KiB = one LDS-DMA wave instruction; same size as w.
 * m3t_sgemm_bimg: C[M,N] = act(A B^T + bias) (+ C) with B given as that image: the 128 x 256 tile kernel fetches B straight into LDS
 * (global_load_lds_dwordx4: no registers, no conversion, no ds_write for two thirds of the staged bytes), A as m3t_sgemm_scaled.  Bit-identical
 * to m3t_sgemm_scaled with the same slots.  N % 64 (image) / % 256 (product), K % 32, M % 128; amax_a NULL: measured; amax_b required. */
int m3t_f16x3_image_b(const float* w, int N, int K, size_t ld, float* img, const unsigned long long* slot, void* stream);
int m3t_sgemm_bimg(int M, int N, int K, const float* A, int lda, const float* B_img, float* C, int ldc, const float* bias, int act,
                   int accumulate, float* ws, size_t ws_bytes, const unsigned long long* amax_a, const unsigned long long* amax_b, void* stream);
/* Round 6: the fp16x3 product of m3t_sgemm_scaled on the 256 x 256 "ring" kernels (csrc/gemm_ring.hip): both operands reach LDS as raw fp32 by
 * LDS-DMA (global_load_lds_dwordx4) into a ring of four 16-k stages, counted vmcnt in front of the stage's single barrier, the two-term split on
 * the fragment read.  Same arithmetic as m3t_sgemm_scaled under the same slots (same split, same MFMA operand placement, same product and k
 * order, same split-K slabs: bit-identical where both take the same K passes).  transA / transB / seg_* as m3t_sgemm (nn.Linear, the GRU input
 * projections and their gradients: reference models/rnn.py:17,22-55,75; transA = transB = 1 has no caller and is refused); row-contiguous
 * operands (transA = 1, transB = 0) are fetched a k row per LDS-DMA instruction and read back with ds_read2st64_b32 -- no cross-lane
 * transpose.  N % 256 == 0, K % 16 == 0 (K % seg_len == 0, seg_len >= 32 when segmented), any M (M % 4 == 0 with transA = 1), 16-B aligned
 * operands with ld % 4 == 0; splits >= 1 slabs (ws of splits * M * N floats when > 1); NULL slots are measured; `variant` selects a build of
 * the NT main loop (0 = plain, 1 = reads a stage ahead, 2 = v_fma_mix split, 3 = both; the timing-only ablation builds behind
 * profiles/r06_ring_gemm_ablation.txt are refused unless M3T_RING_ABLATIONS is set). */
int m3t_sgemm_ring(int transA, int transB, int M, int N, int K, const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                   const float* bias, int act, int accumulate, int seg_len, int seg_stride, int a_off, int b_off, float* ws, size_t ws_bytes,
                   int splits, const unsigned long long* amax_a, const unsigned long long* amax_b, int variant, void* stream);
int m3t_conv3d_taps_pre(const float* src_img, const float* w_img, float* dst, int N, int C_src, int C_dst, int T, int H, int W,
                        int To, int Ho, int Wo, int kt, int kh, int kw, int base_t, int base_h, int base_w, int sign,
                        const unsigned long long* amax_src, const unsigned long long* amax_w, float* ws, size_t ws_bytes, float* dst_planes,
                    void* stream);

/* The whole convolution without a patch matrix (round 5, second half; reference models/backbone.py:73-103,179-271, models/resnet.py:40-45 --
 * nn.Conv3d / nn.Conv2d forward and backward of the visual stems and the per-frame ResNet).
 * m3t_conv3d_fwd_taps: y_cl[(n, t', h', w')][co] = bias[co] + sum over (kt, kh, kw, ci) of x[(n, t' st + kt - pt, h' sh + kh - ph, w' sw + kw - pw)][ci]
 *   W[co][ci][kt][kh][kw] over the CHANNELS-LAST input, any stride: x_img = the m3t_f16x3_split image of x_cl [N T H W][Ci], w_img = the image
 *   of the K-contiguous weights [Co][(tap, ci)], both under the slots given; bias may be NULL.  Co % 64 == 0, Ci % 32 == 0, any number of rows.
 * m3t_conv3d_wgrad_taps: dwt[(tap, ci)][co] = sum over the rows r = (n, t', h', w') of the dy grid of x_cl[source row of (r, tap)][ci] dy_cl[r][co]
 *   -- the walk turned round: the reduction runs over the rows (deterministic split-K slabs in ws), the tap is picked once per thread from
 *   its output row, every reduction row is decoded on the dy grid by a counter (no division in the loop).  dwt has ceil128(taps Ci) rows
 *   (rows past taps Ci are written as zeros); fp32 operands, split in the kernel -- or, with M3T_CONV_IMAGES, their m3t_f16x3_split images;
 *   flags / amax as m3t_sgemm_scaled (NULL slots are measured).
 *   Co % 64 == 0, Ci % 4 == 0, 16-B aligned; any number of rows (round 6: a ragged last reduction tile reads zeros).
 * With m3t_conv3d_taps(_pre) for the data gradient of the stride-1 layers, no convolution of the path materialises its patches.
 * dst_planes / y_planes (optional, every walk but the weight gradient's): the result is left as channel planes [N][C][T H W] there -- written by
 * the walk's own epilogue when it runs in one K pass (16-byte stores of 4 positions per channel), else reduced into dst / y_cl (then
 * scratch of the same size) and transposed by m3t_btc_to_bct. */
/* The stems' first layers (C_in <= 4; reference models/backbone.py:73-78,179-184): m3t_planes_to_cl4 writes x [N][C][S] channels-last with
 * FOUR channels (missing ones zero; raises the slot armed by m3t_amax_out); m3t_conv3d_fwd_taps4 walks the m3t_f16x3_split image of that
 * against w_img = the image of [Co][kt][kh][8][4] (kernel width padded to eight taps, channels to four, zeros): one 32-deep k tile per
 * (kt, kh) pair.  kw <= 8, Co % 64 == 0, any number of rows.  The weight gradient is m3t_conv3d_wgrad_taps with Ci = 4. */
int m3t_planes_to_cl4(const float* x, float* out, int N, int C, long long S, void* stream);
int m3t_conv3d_fwd_taps4(const float* x_img4, const float* w_img, const float* bias, float* y_cl, int N, int Co, int T, int H, int W,
                         int kt, int kh, int kw, int st, int sh, int sw, int pt, int ph, int pw, const unsigned long long* amax_x,
                         const unsigned long long* amax_w, float* ws, size_t ws_bytes, float* y_planes, void* stream);
int m3t_conv3d_fwd_taps(const float* x_img, const float* w_img, const float* bias, float* y_cl, int N, int Ci, int Co, int T, int H, int W,
                        int kt, int kh, int kw, int st, int sh, int sw, int pt, int ph, int pw, const unsigned long long* amax_x,
                        const unsigned long long* amax_w, float* ws, size_t ws_bytes, float* y_planes, void* stream);
int m3t_conv3d_wgrad_taps(const float* x_cl, const float* dy_cl, float* dwt, int N, int Ci, int Co, int T, int H, int W, int kt, int kh, int kw,
                          int st, int sh, int sw, int pt, int ph, int pw, int flags, const unsigned long long* amax_x,
                          const unsigned long long* amax_dy, float* ws, size_t ws_bytes, void* stream);

/* Magnitude slots from the PRODUCER (fp16x3 mode, see m3t_sgemm_scaled): the NEXT m3t_conv1d_fwd(_scaled) / m3t_mask_pos / m3t_mask_pos_drop /
 * m3t_weight_norm_fwd / m3t_bct_to_btc call of the calling thread raises `slot` (8 bytes, zero-initialised by the caller, epoch 0) to the bits of max |x| over
 * its output (y / out / w_t) -- in the same kernel, one 64-bit atomic max per workgroup -- so that the contraction that consumes the output
 * needs no measuring launch.  Consumed by that call (also when it fails); slot == NULL clears a pending one.  Returns 0. */
int m3t_amax_out(unsigned long long* slot);

/* library / device info: returns the ABI version; arch string copied to `arch` if non-null */
int m3t_version(void);
int m3t_device_arch(char* arch, int cap);

/* ---------------------------------------------------------------------------------
 * Dense contraction on fp32 MFMA (v_mfma_f32_32x32x2_f32), exact fp32:
 *   C[M,N] (ldc) = act( alpha-free  op(A)[M,K] * op(B)[K,N] + bias[N] ) (+ C if accumulate)
 * transA=0: A stored [M][K] (lda)   transA=1: A stored [K][M] (lda)
 * transB=0: B stored [K][N] (ldb)   transB=1: B stored [N][K] (ldb)  <- nn.Linear weight
 * act: 0 none, 1 ReLU.  bias may be NULL.
 * seg_len>0 (only with transA=1, transB=0): the reduction index k walks SEGMENTS:
 *   storage row of A = (k / seg_len) * seg_stride + k % seg_len + a_off, same for B
 *   with b_off (used for dW_hh = sum_t dgh_t^T h_{t-1}: per-clip shifted rows).
 * ws/ws_bytes: optional split-K workspace (deterministic slab reduction); may be NULL.
 * flags: 0 or any of M3T_GEMM_BACKGROUND, M3T_GEMM_BF16, M3T_GEMM_EXCLUSIVE.
 * Replaces: nn.Linear (models/rnn.py:22-55, models/model.py:88, models/att_fusion.py:13),
 * the input projections W_ih x inside nn.GRU (models/rnn.py:17,75) and their autograd. */
int m3t_sgemm(int transA, int transB, int M, int N, int K,
              const float* A, int lda, const float* B, int ldb,
              float* C, int ldc, const float* bias, int act, int accumulate,
              int seg_len, int seg_stride, int a_off, int b_off,
              float* ws, size_t ws_bytes, int flags, void* stream);

/* m3t_sgemm with the callers' MAGNITUDE SLOTS for the M3T_GEMM_F16X3 mode.  A slot is 8 bytes, 8-B aligned, whose low word holds the
 * fp32 bit pattern of an upper bound of max |x| over the operand (any bound is valid; a loose one only costs precision at the small
 * end).  amax_a / amax_b may each be NULL: that operand is then measured by the library (one extra launch on `stream`).  Producers
 * that know their magnitudes for free provide the slots: m3t_absmax (one launch for up to 16 tensors), m3t_gru_scan_bwd
 * (m3t_gru_bwd_desc.amax), a constant (|h| <= 1 for GRU outputs).  Ignored unless the fp16x3 kernel runs. */
int m3t_sgemm_scaled(int transA, int transB, int M, int N, int K,
                     const float* A, int lda, const float* B, int ldb,
                     float* C, int ldc, const float* bias, int act, int accumulate,
                     int seg_len, int seg_stride, int a_off, int b_off,
                     float* ws, size_t ws_bytes, int flags,
                     const unsigned long long* amax_a, const unsigned long long* amax_b, void* stream);

/* The same contraction (transA = 0) over a TIME WINDOW of batch-major sequence tensors: A is a [n_seg, win_stride, *] tensor of which only
 * the frames [win_off, win_off + win_len) of every clip take part -- row m of the product reads storage row
 * (m / win_len) * win_stride + m % win_len + win_off of A and writes the same storage row of C:
 *   C[rows of the window, 0:N] (ldc) = act( A[rows of the window, 0:K] (lda) * op(B)[K,N] + bias ) (+ C if accumulate)
 * Used by the direction-split, time-chunked hand-offs between a BiGRU scan and the projections / data gradients on either side of it
 * (reference models/rnn.py:17,75: layer l+1's input projection is out_fwd W_ih[:, :H]^T + out_rev W_ih[:, H:]^T, and each half is final for the
 * frames its direction's scan has passed: m3t_gru_scan_progress).  Only the 16-bit-term tile kernel has this form: n_seg * win_len % 128 == 0,
 * N % 64 == 0, K % 32 == 0, 16-B aligned operands with ld % 4 == 0, flags without M3T_GEMM_BF16 / _HIGH; else M3T_EINVAL.  One launch, no
 * split-K.  amax_a / amax_b as m3t_sgemm_scaled. */
int m3t_sgemm_window(int transB, int n_seg, int win_len, int win_stride, int win_off, int N, int K,
                     const float* A, int lda, const float* B, int ldb, float* C, int ldc, const float* bias,
                     int act, int accumulate, int flags, const unsigned long long* amax_a, const unsigned long long* amax_b, void* stream);
/* ... and up to M3T_WINDOW_BATCH such problems of ONE shape (same window, N, K, leading dimensions, act) as one launch: the pieces that become
 * ready at one progress mark -- every (stack, direction) pair reading that window -- fill the CUs a scan leaves free as one grid instead of
 * a queue of under-filled launches.  With n > 1 every problem must bring its magnitude slots in the fp16x3 mode. */
#define M3T_WINDOW_BATCH 8
typedef struct {
    const float* A; const float* B; float* C; const float* bias;          /* bias may be NULL */
    const unsigned long long* amax_a; const unsigned long long* amax_b;
    int accumulate;
} m3t_window_problem;
int m3t_sgemm_window_batch(int n, const m3t_window_problem* problems, int transB, int n_seg, int win_len, int win_stride, int win_off,
                           int N, int K, int lda, int ldb, int ldc, int act, int flags, void* stream);

/* slots[i] = max(slots[i], bits of max |x| over x[i] = [rows[i] x cols[i]] fp32 with leading dimension ld[i]) for n <= 16 tensors in
 * ONE launch (cols % 4 == 0, ld % 4 == 0, 16-B aligned).  The caller zero-initialises a slot before its first use. */
int m3t_absmax(int n, const float* const* x, const size_t* rows, const int* cols, const size_t* ld,
               unsigned long long* const* slots, void* stream);

/* Which kernel m3t_sgemm would run for a call of this shape (all operands 16-B aligned, ld % 4 == 0) and how many
 * split-K slabs: *kernel = 0 fp32-MFMA tile kernel, 1 the 16-bit-term 128 x 128 / 128 x 64 tile kernels (formerly also 2: the 256 x 256 tile, removed; only with
 * M3T_GEMM_EXCLUSIVE).  For tools and tests; no device work. */
int m3t_sgemm_plan(int transA, int M, int N, int K, int seg_len, size_t ws_bytes, int flags, int* kernel, int* splits);

/* out[n] (+)= sum_m X[m*ld + n], m<M, n<N  (bias gradients); ws optional (tall inputs) */
int m3t_colsum(const float* X, int M, int N, int ld, float* out, int accumulate,
               float* ws, size_t ws_bytes, void* stream);

/* dst[c][r] = src[r][c]  (src [R][C] with lds, dst [C][R] with ldd) */
int m3t_transpose(const float* src, int R, int C, int lds, float* dst, int ldd, void* stream);

/* y = relu'(a) * dy elementwise: dy[i] = a[i] > 0 ? dy[i] : 0 over n elements (in place on dy) */
int m3t_relu_bwd(const float* a, float* dy, size_t n, void* stream);

/* ---------------------------------------------------------------------------------
 * BiGRU recurrence (the T-step scan inside nn.GRU, models/rnn.py:17,75).
 * One call advances up to M3T_MAX_SCANS INDEPENDENT direction-scans (both directions
 * of a layer; the same layer of independent stacks) in lock-step: one launch per
 * time step covers all of them.  Gate order [r;z;n] (torch):
 *   r = sig(xr + Whr h + bhr); z = sig(xz + Whz h + bhz); n = tanh(xn + r*(Whn h + bhn))
 *   h' = (1-z)*n + z*h ; h0 = 0 ; reverse scans run t = T-1 .. 0.
 * xproj already contains W_ih x + b_ih (m3t_sgemm). */
typedef struct {
    const float* xproj;  /* [B,T,ldx]; this scan reads columns [xoff, xoff+3H)            */
    const float* w_hh;   /* [3H,H]                                                         */
    const float* b_hh;   /* [3H]                                                           */
    float* out;          /* [B,T,ldo]; h_t written to columns [ooff, ooff+H)               */
    float* gates;        /* [B,T,H,4] saved (r,z,n,Whn h + bhn) per unit for backward (16-B aligned); NULL = skip */
    float* h_n;          /* [B,H] final hidden state (NULL = skip)                         */
    int H, reverse, ldx, xoff, ldo, ooff;
} m3t_gru_fwd_desc;

/* ws (optional, 16-B aligned): scratch for the fragment-ordered fast paths -- per scan 3*H*H floats of re-laid
 * weights + 4 * ceil32(B) * H floats of ping-pong state / exchange granules; without it (or when H % 16 != 0) a
 * slower kernel that reads the row-major operands directly is used.  Results are identical on every path, except that the persistent FORWARD scan
 * at H = 256 / 512 runs its recurrent product as bf16x6 (fp32-accurate, ~1e-6 from the fp32-MFMA kernels; flag
 * M3T_SCAN_FP32 or env M3T_SCAN_X6=0 keeps fp32 MFMAs and bit-identity).
 * Execution: a level whose scans all have H = 128 runs ONE launch with one workgroup per (scan, clip) and nothing exchanged
 * between workgroups (gru_solo.hip: fp32 FMA chains, equal to the other paths to fp32 rounding; no residency requirement;
 * flags M3T_SCAN_NO_PERSIST / M3T_SCAN_FP32 or env M3T_SCAN_SOLO=0 keep the paths below).  Otherwise,
 * when every H of the level is a multiple of 128 (<= 512) and the level fits the chip at one workgroup
 * per CU, ONE persistent launch runs all T steps (W_hh held in registers, h_t exchanged between CUs through tagged
 * granules); otherwise one launch per time step.  A persistent launch needs all its workgroups resident: never run
 * two of them concurrently on one device (flags = M3T_SCAN_NO_PERSIST for scans issued on a side stream; env
 * M3T_SCAN_PERSIST=0 disables globally).  One process per device: the first process that launches a persistent scan on a
 * GPU takes an advisory lock ($XDG_RUNTIME_DIR or /tmp/m3t-<uid>/ m3t_persist_<pci-bus-id>.lock, held until it exits); any
 * other process on that GPU gets the launch-per-step path, says so on stderr, and m3t_gru_persist_owner() returns 2 there
 * (env M3T_SCAN_LOCK=0 disables the guard).
 * Error model.  Every wait of a persistent scan is bounded (M3T_SCAN_SPIN_LIMIT gather attempts, default 2^21 ~ 2 s).  A
 * workgroup whose wait expires raises a STICKY host-mapped flag and the scan finishes with INVALID results.  The flag stays
 * set until m3t_gru_error_reset(), which the host may call only after it has synchronised the device.  While it is set:
 * (a) m3t_gru_poll_error() returns non-zero; (b) every m3t_gru_scan_* call returns M3T_ESPIN; (c) m3t_grad_norm_scale, which
 * reads the flag ON THE DEVICE in stream order, zeroes the gradient buffer and returns norm = NaN, and m3t_adam_step /
 * m3t_sgd_step skip an update whose `guard` scalar is not finite.  Because the host never clears the flag on a read, every
 * step queued behind the dead scan is skipped however far ahead of the GPU the host runs: a dead scan can never reach the
 * parameters, with no host synchronisation.  Recovery = synchronise, m3t_gru_error_reset(), redo the step.
 * Several ranks: m3t_grad_poison / m3t_grad_dead_check (below) carry the failure of one rank through the gradient
 * all-reduce to every rank. */
int m3t_gru_scan_fwd(const m3t_gru_fwd_desc* scans, int n_scans, int B, int T,
                     float* ws, size_t ws_bytes, int flags, void* stream);

/* BPTT of the scans above (autograd of nn.GRU).  Per scan:
 *   dgx[B,T,ldg][goff..goff+3H) = grad wrt xproj  = (dr~, dz~, dn~)
 *   dgh[B,T,3H]                 = grad wrt W_hh h + b_hh = (dr~, dz~, dn~ * r)
 * The caller finishes with m3t_sgemm / m3t_colsum: dW_hh = sum dgh_t^T h_{t-1},
 * db_hh = colsum(dgh), dW_ih = dgx^T x, db_ih = colsum(dgx), dx = dgx W_ih. */
typedef struct {
    const float* dout;    /* [B,T,ldo]: grad wrt out, columns [ooff, ooff+H)               */
    const float* out;     /* forward h_t, same layout                                      */
    const float* gates;   /* [B,T,H,4] from forward                                        */
    const float* w_hh_t;  /* [H,3H] = W_hh transposed (m3t_transpose)                      */
    const float* dh_n;    /* [B,H] grad wrt final hidden state, or NULL                    */
    float* dgx;           /* [B,T,ldg], columns [goff, goff+3H)                            */
    float* dgh;           /* [B,T,3H]                                                      */
    float* dh;            /* [B,H] scratch: running dL/dh_t                                */
    float* db_part;       /* optional [B,4,H] scratch: per-clip sums over t of (dr~, dz~, dn~, dn~*r); with it the  */
    float* db_ih;         /* scan also delivers db_ih [3H] = sum_b (dr~,dz~,dn~) and db_hh [3H] = sum_b (dr~,dz~,   */
    float* db_hh;         /* dn~*r) -- the bias gradients, without a pass over dgx / dgh (all three NULL = skip)    */
    int H, reverse, ldo, ooff, ldg, goff;
    unsigned long long* amax;  /* optional magnitude slot (m3t_sgemm_scaled): raised to the bits of max |dgx|, |dgh| of this scan */
    const float* wfrag;        /* optional: W_hh already in the backward scan's fragment order (m3t_gru_bwd_prepare) -- the launch then   */
                               /* runs no preparation kernel in front of the scan; used only when EVERY scan of the call brings one       */
} m3t_gru_bwd_desc;

/* W_hh does not change between the forward and the backward pass of a step: the backward scans' weight re-layout (one launch in front of
 * every backward scan, on the critical chain) can be done any time after the weights are final -- e.g. on an idle stream during the forward
 * pass.  m3t_gru_bwd_prepare writes, for n <= M3T_MAX_SCANS scans of one H, the fragments the wide producer-split backward kernel reads
 * (two fp16 terms of the per-slice scaled W_hh^T + the slices' inverse scales) into out[i] (m3t_gru_bwd_prepare_floats(H) floats each, 16-B
 * aligned); whh_direct = 1: w[i] is W_hh [3H, H] as stored (M3T_SCAN_WHH), 0: its transpose [H, 3H].  A later m3t_gru_scan_bwd whose descs
 * all carry desc.wfrag = out[i] and whose launch takes that kernel (m3t_gru_scan_progress_ok(..., backward = 1) says so) skips its own
 * preparation; any other launch ignores the field.  H % 256 == 0. */
size_t m3t_gru_bwd_prepare_floats(int H);
int m3t_gru_bwd_prepare(const float* const* w, int n, int H, int whh_direct, float* const* out, void* stream);

/* Workgroups (= CUs: a scan workgroup owns its CU) that m3t_gru_scan_fwd (backward = 0) / m3t_gru_scan_bwd (backward = 1) would hold
 * resident for ONE persistent launch over n_scans scans of hidden size H at batch B with `flags`; 0 when that level does not run as a
 * persistent launch that needs residency (launch-per-step path, solo kernels, M3T_SCAN_NO_PERSIST).  Two persistent launches may run
 * at the same time iff the sum of their answers fits the device's CUs, per XCD (ceil(answer / 8) each, 32 CUs per XCD on MI355X):
 * then both grids become resident whatever else is draining from the CUs, and neither can wait for the other forever.  No device work. */
int m3t_gru_scan_workgroups(int n_scans, int H, int B, int T, int flags, int backward);
/* Number of one-launch scans (persistent or solo) this process has issued so far (tests use it to assert which path ran). */
int m3t_gru_persist_count(void);
/* 0, or (step + 1) of a persistent scan that gave up waiting since the last m3t_gru_error_reset() (sticky: reading does
 * NOT clear it).  The words are host-mapped: no synchronisation happens here, so synchronise the scan's stream first if the
 * answer must cover it. */
int m3t_gru_poll_error(void);
/* Clears the scan error state.  ONLY after the device has been synchronised (nothing queued may still read the flag). */
int m3t_gru_error_reset(void);
/* Several ranks (m3t.ddp): on = 1 makes m3t_gru_scan_fwd / _bwd launch even while the sticky flag is set instead of returning
 * M3T_ESPIN.  A rank that raised in the middle of a step -- the moment ITS host happened to see the flag -- would leave its peers
 * waiting in that step's collective; the device-side guards (m3t_grad_norm_scale, the optimizer steps) skip every step queued behind
 * the dead scan anyway, m3t_grad_poison / m3t_grad_dead_check carry the failure to every rank through the all-reduce, and the host
 * raises on ALL ranks at the same step from the all-reduced dead slot.  m3t_gru_poll_error() is unaffected.  Returns 0. */
int m3t_gru_error_defer(int on);
/* Fault injection (tests): a one-thread kernel on `stream` raises the scan error flag exactly as a dying scan would. */
int m3t_gru_inject_error(void* stream);
/* Who owns the persistent scans of the current device: 0 not decided yet (no persistent scan attempted), 1 this process,
 * 2 another process (this one runs the launch-per-step kernels). */
int m3t_gru_persist_owner(void);
/* Exchange arena (optional, speed only).  A persistent scan exchanges h_t / dgh_t between workgroups through tagged granules
 * and must never meet a stale granule whose tag matches; without an arena every launch therefore zeroes its exchange buffers
 * (3-4 fill kernels in front of every scan).  m3t_gru_scan_arena(arena, bytes): the NEXT m3t_gru_scan_fwd / _bwd call of the
 * calling thread keeps its exchange buffers in `arena` (device memory, 16-B aligned, >= 8 MiB + 64 KiB) and draws launch-unique
 * tags from a per-arena counter instead -- no fill kernel, except when the arena is first seen and when a 16-bit tag counter wraps
 * (every ~200 launches).  With an arena the launch also runs a placement handshake: workgroups publish the XCD they sit on, and a
 * group (one scan x one row block) whose members all share an XCD exchanges through that XCD's L2 (plain stores + sc1 loads)
 * instead of through the memory side -- 30-40 % less HBM / fabric traffic per launch, same results; used by the
 * launches whose groups are XCD-aligned by construction (a multiple of 8 groups).  CONTRACT: nothing but scan launches may ever write the arena, and launches that share an arena
 * must be ordered (one stream).  m3t_gru_scan_arena_reset(arena): forget what is known about `arena` (call it when the
 * memory was reallocated or written by anything else; NULL = every arena).  Both return 0. */
int m3t_gru_scan_arena(void* arena, size_t bytes);
int m3t_gru_scan_arena_reset(void* arena);
/* PROGRESS MARKS (round 5): consumers of a persistent scan's results need not wait for the launch to end.  Layer l+1's input projection
 * (reference models/rnn.py:17,75) is out_fwd W_ih[:, :H]^T + out_rev W_ih[:, H:]^T: each half needs ONE direction's scan, and the frames
 * that scan has passed are final.  m3t_gru_scan_progress(counters, n_marks, time_bounds, need): the NEXT m3t_gru_scan_fwd / _bwd call of the
 * calling thread publishes its progress through `counters` (two 32-bit device words, 8-B aligned, zero-initialised ONCE by the caller and
 * from then on written by scan launches only): counters[0] counts for the scans of the call that walk time upwards (forward pass:
 * reverse = 0; backward pass: reverse = 1), counters[1] for those that walk it downwards.  time_bounds[0 .. n_marks) (n_marks <= 3,
 * ascending, 4 <= tb, tb <= T - 4, at least 4 apart) cut [0, T) into n_marks + 1 windows.  Each workgroup adds 1 to its counter once its
 * results -- out / gates (forward), dgx / dgh and the per-window magnitude slots (backward) -- of every frame on the finished side of a bound
 * are in memory and visible device-wide.  On return need[k] (k < n_marks) is the value counters[0] reaches when the upward scans have
 * finished frames [0, time_bounds[k]); need[n_marks + k] the value counters[1] reaches when the downward scans have finished frames
 * [time_bounds[n_marks - 1 - k], T).  A consumer stream waits with m3t_stream_wait_progress (a one-lane gate kernel that polls the word;
 * what follows it starts behind a kernel boundary and reads the written-back data); the last window of each direction is final when the
 * scan launch ends (ordinary stream order / events).  Backward calls with marks armed write their magnitude slots as an ARRAY:
 * desc.amax[0] the whole scan (final at the end of the launch), desc.amax[1 + w] the w-th window IN THE ORDER THE SCAN WALKS THEM.
 * Only the launches whose kernels carry the marks accept an armed call (m3t_gru_scan_progress_ok: the fp16x3 persistent forward kernels,
 * the wide producer-split backward kernel); any other path returns M3T_EINVAL rather than leave consumers waiting.  Consumed by that call
 * (also when it fails); counters == NULL disarms.  m3t_gru_scan_progress_reset(counters): forget the library's count of what it has asked
 * of `counters` (after the caller re-zeroed or freed them; NULL = all).  Every wait is bounded (M3T_SCAN_SPIN_LIMIT): a gate that gives
 * up raises the sticky scan error. */
int m3t_gru_scan_progress(unsigned* counters, int n_marks, const int* time_bounds, unsigned* need);
int m3t_gru_scan_progress_reset(unsigned* counters);
int m3t_gru_scan_progress_ok(int n_scans, int H, int B, int T, int flags, int backward);
int m3t_stream_wait_progress(const unsigned* counter, unsigned need, void* stream);
/* Ordering between scans on different streams without holding back their preparation: the NEXT m3t_gru_scan_fwd /
 * m3t_gru_scan_bwd call of the calling thread makes its stream wait for `event` (a hipEvent_t) right before it launches
 * its scan kernel(s); the weight re-layout kernels and memsets it issues first run as soon as the stream allows.  Used
 * by the host schedule that alternates the persistent scans of two streams (they must never run at the same time).
 * The event is consumed by that call (also when it fails).  Returns 0. */
int m3t_gru_scan_after(void* event);
/* Timing hook: the NEXT m3t_gru_scan_fwd / m3t_gru_scan_bwd call of the calling thread records `start` right before and
 * `end` right after its scan kernel(s) on its stream (two hipEvent_t created with timing enabled) -- not around its weight
 * re-layout kernels, memsets or the m3t_gru_scan_after fence.  bench.py's roofline.achieved uses it.  Returns 0. */
int m3t_gru_scan_events(void* start, void* end);
/* With env M3T_SCAN_PROF=1: s_memtime cycles that workgroup 0 / lane 0 of the LAST persistent launch spent per phase,
 * summed over its T steps: [0] step top, [1] gather (wait for peers), [2] MFMA + LDS partials, [3] barrier,
 * [4] reduce + gate math + publish, [5] stores.  Synchronises the device.  M3T_EINVAL when profiling is off. */
int m3t_gru_persist_profile(unsigned long long* out6);

/* ws as above: per scan 3*H*H + 8 * ceil32(B) * H floats; flags as above. */
int m3t_gru_scan_bwd(const m3t_gru_bwd_desc* scans, int n_scans, int B, int T,
                     float* ws, size_t ws_bytes, int flags, void* stream);

/* ---------------------------------------------------------------------------------
 * Attention-fusion reduction (models/att_fusion.py:21-25) on [B*T] frames of D floats:
 *   w = softmax([sigmoid(s_v), sigmoid(s_a)]);  f = w0 * x_v + w1 * x_a   (index 0 = VIDEO)
 * s_v, s_a: [rows] raw scorer outputs. */
int m3t_att_fuse_fwd(const float* s_v, const float* s_a, const float* x_v, const float* x_a,
                     float* f, int rows, int D, void* stream);
int m3t_att_fuse_bwd(const float* df, const float* s_v, const float* s_a,
                     const float* x_v, const float* x_a,
                     float* ds_v, float* ds_a, float* dx_v, float* dx_a,
                     int rows, int D, void* stream);

/* ---------------------------------------------------------------------------------
 * Loss of AffWild2VA.training_step (models/model.py:132-141,146-182), forward and
 * gradient in one pass over y_hat [rows, C]:
 *   L = w_v * (1 - ccc(y[:,iv], valence)) + w_a * (1 - ccc(y[:,ia], arousal))
 *       + expr_w * mean_rows( CE(y[:, :n_expr], class_expr) * expr_valid )     (n_expr>0)
 * (training_step uses w_v = loss_lambda, w_a = 1 - loss_lambda, expr_w = 0.8).
 * A zero weight skips its term entirely: w_v == 0 (w_a == 0) leaves loss_v (loss_a) at 0 and column iv (ia) of dy
 * untouched by that term, whatever the column holds -- NaN included; expr_w == 0 adds neither the CE term nor its
 * gradient.  The statistics of a skipped term are still reported (ccc_v / ccc_a, loss_expr, n_valid, n_correct) and
 * may then be NaN.
 * ccc per models/utils.py:6-17 (unbiased variance, biased covariance).  With
 * use_mse!=0 the two ccc terms become mean squared errors (models/model.py:143-144).
 * rows == 1: the variances divide by max(rows - 1, 1), so they and the covariance are 0 and ccc = 0 / (y - t)^2:
 * loss_v = 1 and dL/dy = 0 for y != t, NaN for y == t (torch's unbiased variance of one element is NaN: the reference
 * gives NaN for every one-row batch).  The mse form and the CE term are unaffected.
 * The CE term is dropped when no row is valid (model.py:173-174) -- decided on device; it is the mean over ALL rows
 * of the valid rows' cross entropies.  class_expr is read on valid rows only: an invalid row may carry any marker
 * (-1, 255).  n_correct counts the valid rows whose FIRST maximum is the label.
 * out_scalars[8] = {loss, loss_v, loss_a, loss_expr, n_valid, n_correct, ccc_v, ccc_a};
 * dy [rows, C] receives dL/dy_hat (fully written: exactly 0 in every column that belongs to no term).
 * class_expr int64, expr_valid uint8.
 * Precision: every sum over rows, the closed form and each row's regression gradient are evaluated in fp64 and
 * rounded to fp32 once; the per-row cross entropy and its gradient are fp32.  All three forms below are held to
 * 4 x max(fp32 torch's error, 1 ulp) of float64 (tests/test_gpu_fuse_loss.py). */
int m3t_va_loss(const float* y_hat, int rows, int C, int iv, int ia,
                const float* valence, const float* arousal,
                const int64_t* class_expr, const uint8_t* expr_valid, int n_expr,
                float w_v, float w_a, float expr_w, int use_mse,
                float* out_scalars, float* dy, float* ws, size_t ws_bytes, void* stream);
/* ws: 32 floats (16 doubles) per 256 rows = m3t_va_loss_ws_bytes(rows), 8-B aligned.  With it, 1024 < rows <= 32768 run as ONE grid-wide
 * launch (round 6): raw moments in fp64 in one sweep, the blocks meet once inside the kernel (agent-scope release + ticket, bounded wait: a
 * wait that expires gives loss = NaN), every block sums all partials in block order (deterministic) and writes its rows of dL/dy;
 * M3T_VA_LOSS_FUSED=0 or more rows: three short launches (sums -> centred moments -> closed form + gradient, fp64 partials per block);
 * without ws (or with one too small or misaligned), or for rows <= 1024, one workgroup does all passes.  Calls that use the one-launch form
 * share two ticket words per device: they must not run concurrently on two streams. */
size_t m3t_va_loss_ws_bytes(int rows);

/* Round 6: channels-last operators of the 3-D VGG-M stems (csrc/stem_cl.hip; reference models/backbone.py:73-103,179-271: Conv3d -> BatchNorm3d ->
 * ReLU (-> MaxPool3d((1, 2, 2)))).  The tap walks read and write channels-last rows [N T H W][C]; with these two the whole stem stays in that
 * layout -- no planes <-> channels-last transpose between the video and the GRU input.
 * m3t_bn_cl_fwd / _bwd: BatchNorm (+ fused ReLU) over rows x [M][C] at any M (semantics of m3t_bn_rows_fwd / _bwd: batch statistics with
 *   torch's running-statistics update when training, fp64 per-chunk partials reduced in a fixed order); C % 4 == 0, C / 4 divides 256
 *   (C = 64 ... 1024 in powers of two), 16-B aligned tensors; ws: m3t_bn_cl_ws_bytes(M, C) bytes, 8-B aligned.  m3t_amax_out arms the
 *   magnitude slot of y (forward) / dx (backward): the next tap walk scales by it.  dx_colsum [C] (optional): the column sums of dx -- the bias
 *   gradient of the convolution in front of this BatchNorm -- from the dx pass itself (block partials summed in block order).
 * m3t_pool_cl_fwd / _bwd: max pooling of P frames x [P][H][W][C] with a (kh, kw) window, stride (sh, sw), padding (ph, pw) -- nn.MaxPool3d((1,
 *   kh, kw)) on channels-last rows; win [P][Ho][Wo][C] bytes: the winner's place in its window (ties: the first maximum in window order, NaN
 *   wins, as torch); backward is a gather (no atomics, deterministic).  C % 4 == 0, kh kw <= 255, padding < window.  m3t_amax_out arms y's slot.
 * m3t_bn_pool_cl_fwd / _bwd: BatchNorm + ReLU + max pooling with a k x k window, stride k, no padding (k = 2, 3: every pooling layer of the
 *   VGG-M stems) as ONE operator: relu(bn(x)) at full resolution is neither written nor read -- forward keeps the pooled frames yp [P][H / k][W /
 *   k][C] and the winner bytes, backward takes d(yp) and writes dx [P][H][W][C] (an input position's gradient through the pooling is d(yp) of
 *   its window if it won and yp > 0, else 0; positions no window covers get the BatchNorm terms only).  ws, slots, dx_colsum as m3t_bn_cl_*
 *   with M = P H W. */
size_t m3t_bn_cl_ws_bytes(size_t M, int C);
int m3t_bn_pool_cl_fwd(const float* x, size_t P, int H, int W, int C, int k, const float* gamma, const float* beta, float* run_mean, float* run_var,
                       float momentum, float eps, int training, float* yp, unsigned char* win, float* save_mean, float* save_invstd, float* ws,
                       size_t ws_bytes, void* stream);
int m3t_bn_pool_cl_bwd(const float* dyp, const float* x, const float* yp, const unsigned char* win, const float* gamma, const float* save_mean,
                       const float* save_invstd, size_t P, int H, int W, int C, int k, int training, float* dx, float* dgamma, float* dbeta,
                       float* dx_colsum, float* ws, size_t ws_bytes, void* stream);
int m3t_bn_cl_fwd(const float* x, size_t M, int C, const float* gamma, const float* beta, float* run_mean, float* run_var, float momentum,
                  float eps, int training, int relu, float* y, float* save_mean, float* save_invstd, float* ws, size_t ws_bytes, void* stream);
int m3t_bn_cl_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* save_mean, const float* save_invstd, size_t M,
                  int C, int training, int relu, float* dx, float* dgamma, float* dbeta, float* dx_colsum, float* ws, size_t ws_bytes, void* stream);
int m3t_pool_cl_fwd(const float* x, size_t P, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw, float* y, unsigned char* win,
                    void* stream);
int m3t_pool_cl_bwd(const float* dy, const unsigned char* win, size_t P, int H, int W, int C, int kh, int kw, int sh, int sw, int ph, int pw,
                    float* dx, void* stream);

/* The per-frame ResNet-18/34 (v1) on the chain (csrc/stem_cl.hip; opt-in, M3T_RESNET_CL=1): the two operators that close a residual block and
 * close the trunk.  Rows are the frames' positions [P H W][C], P = N T.
 * m3t_bn_add_relu_cl_fwd / _bwd: y = relu(bn(x) + shortcut), the block tail of reference models/resnet.py:37-56 (BasicBlock.forward: out =
 *   bn2(conv2(.)); out += identity; out = relu(out)) as ONE operator over x, shortcut [M][C].  Statistics (fp64 per-chunk partials in a fixed
 *   order), the running-statistics update, save_mean / save_invstd, shapes (C % 4 == 0, C / 4 divides 256, C <= 1024, M > 0; training: M >= 2),
 *   ws (m3t_bn_cl_ws_bytes(M, C) bytes, 8-B aligned) and the slot of y (m3t_amax_out) as m3t_bn_cl_fwd.  Backward works with g = dy (y > 0):
 *   one partial pass (sum g -> dbeta, sum g xhat -> dgamma), one map pass that writes dx (the BatchNorm data gradient of g; eval: g gamma
 *   invstd) and ds = g (the shortcut's gradient); dx_colsum [C] (optional) and dx's slot (m3t_amax_out) as m3t_bn_cl_bwd.  No float atomics:
 *   reruns are bit-identical.  gamma == 0 (zero_init_residual): y = relu(beta + shortcut), dx == 0, dgamma finite.  Bad arguments: M3T_EINVAL
 *   before any launch.
 * m3t_mean_cl_fwd / _bwd: nn.AdaptiveAvgPool2d(1) + flatten (reference models/resnet.py:117-119) over channels-last frames x [P][HW][C] ->
 *   y [P][C]: a frame's rows are added in index order in fp64 (deterministic); backward writes dx [P][HW][C] = dy / HW.  C % 4 == 0, P, HW > 0,
 *   16-B aligned tensors. */
int m3t_bn_add_relu_cl_fwd(const float* x, const float* shortcut, size_t M, int C, const float* gamma, const float* beta, float* run_mean,
                           float* run_var, float momentum, float eps, int training, float* y, float* save_mean, float* save_invstd, float* ws,
                           size_t ws_bytes, void* stream);
int m3t_bn_add_relu_cl_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* save_mean, const float* save_invstd,
                           size_t M, int C, int training, float* dx, float* ds, float* dgamma, float* dbeta, float* dx_colsum, float* ws,
                           size_t ws_bytes, void* stream);
int m3t_mean_cl_fwd(const float* x, size_t P, int HW, int C, float* y, void* stream);
int m3t_mean_cl_bwd(const float* dy, size_t P, int HW, int C, float* dx, void* stream);

/* The per-frame ResNet-18/34 v2 (pre-activation) on the chain (csrc/stem_cl.hip; opt-in, M3T_RESNET_V2_CL=1): the operator that closes a
 * residual sum.  Reference models/resnet.py:157-173, 241-242: a block ends in out + identity, and the very next thing is relu(bn1(.)) of the
 * following block -- or bn5 + relu5 at the trunk's end -- while the sum itself lives on as the next identity.
 * m3t_add_bn_relu_cl_fwd: a, b [M][C] -> TWO outputs, s = a + b and z = relu(bn(s)).  Training (3 launches): the statistics pass reads a and b,
 *   WRITES s and sums the fp32-rounded s (chunks, order and fp64 partials of m3t_bn_cl_fwd), then the running-statistics update and the saved
 *   mean / inv-std, then one map pass s -> z: 20 B per element against 24 for a + b followed by m3t_bn_cl_fwd, and s, z, the saved and the
 *   running statistics are the bits of that pair.  Eval (2 launches): one sweep reads a, b and writes s, z; s may be null there (a caller
 *   under no_grad whose sum is dead skips the write), in training a null s is M3T_EINVAL.  Shapes, ws and z's slot (m3t_amax_out) as
 *   m3t_bn_cl_fwd; s carries no slot (it is only ever an addend).
 * m3t_add_bn_relu_cl_bwd: g = dz (z > 0); one partial pass over (dz, s, z) (sum g -> dbeta, sum g xhat -> dgamma), one map pass that writes a
 *   SINGLE tensor ds = (the BatchNorm data gradient of g; eval: g gamma invstd) + ds_out, the gradient of a and of b alike.  ds_out (optional):
 *   the gradient that reaches s through the next identity, added last; null at the trunk's end and in front of a block with a downsample.
 *   ds_colsum [C] (optional) and ds's slot (m3t_amax_out) as m3t_bn_cl_bwd's of dx: 32 B per element.  No float atomics: reruns are
 *   bit-identical.  gamma == 0: ds == ds_out.  Bad arguments: M3T_EINVAL before any launch. */
int m3t_add_bn_relu_cl_fwd(const float* a, const float* b, size_t M, int C, const float* gamma, const float* beta, float* run_mean, float* run_var,
                           float momentum, float eps, int training, float* s, float* z, float* save_mean, float* save_invstd, float* ws,
                           size_t ws_bytes, void* stream);
int m3t_add_bn_relu_cl_bwd(const float* dz, const float* ds_out, const float* s, const float* z, const float* gamma, const float* save_mean,
                           const float* save_invstd, size_t M, int C, int training, float* ds, float* dgamma, float* dbeta, float* ds_colsum,
                           float* ws, size_t ws_bytes, void* stream);

/* GroupNorm on the channels-last chain (csrc/gn_cl.hip; reference models/backbone.py:63-103,165-271 with norm_layer='gn': Conv3d ->
 * GroupNorm(32, C) -> ReLU (-> MaxPool3d((1, 2, 2)))).  Rows x [N][R][C], R = T H W rows per clip; semantics of F.group_norm(x5d, G, gamma, beta,
 * eps) on [N, C, T, H, W]: one mean and one biased variance per (clip, group) over (C / G) R values -- no running statistics, train == eval.
 * C % 4 == 0 and C / 4 divides 256 (as m3t_bn_cl_*), G divides C (C / G may be below 4: a thread's four channels then straddle two groups),
 * 1 <= N <= 65535, 16-B aligned tensors, ws of m3t_gn_cl_ws_bytes(N, R, C) bytes, 8-B aligned.  A refused call (M3T_EINVAL) launches nothing.
 * Statistics: fp64 sums per (clip, chunk, channel), a chunk never crosses a clip, chunks then the group's channels folded in a fixed order;
 * save_mean / save_rstd [N G], rstd = 1 / sqrt(max(var, 0) + eps).  No float atomics: reruns are bit-identical.
 * m3t_gn_cl_fwd: y = (x - mean) rstd gamma + beta, with `relu` as torch.relu (NaN stays NaN).  gamma / beta NULL: 1 / 0.
 * m3t_gn_cl_bwd: g = dy (0 where y <= 0 if relu); per (clip, group), M = (C / G) R: s1 = sum gamma_c g, s2 = sum gamma_c g xhat,
 *   dx = rstd (gamma_c g - s1 / M - xhat s2 / M); dgamma_c = sum_{n,r} g xhat, dbeta_c = sum_{n,r} g (fp64, clips in order; either may be
 *   NULL).  dx_colsum [C] (optional): the column sums of dx -- under GroupNorm the bias gradient of the convolution in front is NOT zero by
 *   construction -- from the dx pass itself (fp64 per thread, per block, then over the blocks in order).
 * m3t_gn_pool_cl_fwd / _bwd: GroupNorm + ReLU + max pooling with a k x k window, stride k, no padding (k = 2, 3; H, W >= k) as ONE operator
 *   over x [N T][H][W][C]: relu(gn(x)) at full resolution is neither written nor read.  yp [N T][H / k][W / k][C] and one winner byte per element
 *   (ties: the first maximum in window order, NaN wins); positions no window covers (odd H or W) count in the statistics and get the
 *   GroupNorm terms of dx only.  The per-element map is the one of m3t_gn_cl_fwd: the same bits.
 * m3t_amax_out arms the magnitude slot of y / yp (forward) and of dx (backward): the largest finite magnitude. */
size_t m3t_gn_cl_ws_bytes(int N, size_t R, int C);
int m3t_gn_cl_fwd(const float* x, int N, size_t R, int C, int G, const float* gamma, const float* beta, float eps, int relu, float* y,
                  float* save_mean, float* save_rstd, float* ws, size_t ws_bytes, void* stream);
int m3t_gn_cl_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* save_mean, const float* save_rstd, int N,
                  size_t R, int C, int G, int relu, float* dx, float* dgamma, float* dbeta, float* dx_colsum, float* ws, size_t ws_bytes,
                  void* stream);
int m3t_gn_pool_cl_fwd(const float* x, int N, int T, int H, int W, int C, int G, int k, const float* gamma, const float* beta, float eps,
                       float* yp, unsigned char* win, float* save_mean, float* save_rstd, float* ws, size_t ws_bytes, void* stream);
int m3t_gn_pool_cl_bwd(const float* dyp, const float* x, const float* yp, const unsigned char* win, const float* gamma, const float* save_mean,
                       const float* save_rstd, int N, int T, int H, int W, int C, int G, int k, float* dx, float* dgamma, float* dbeta,
                       float* dx_colsum, float* ws, size_t ws_bytes, void* stream);

/* Channels-last operators of the VGGFace front-end (csrc/vggface.hip; reference models/vggface.py:45-50: `x = F.relu(c(x))` after every Conv2d,
 * `F.max_pool2d(x, 2, 2, 0, ceil_mode=True)` at the end of every block).  C % 4 == 0, C <= 1024 (C / 4 need not divide the block), 16-B aligned
 * tensors, any number of rows; a refused call (M3T_EINVAL: C % 4 != 0, H < 1, W < 1, a misaligned pointer, a short workspace) launches nothing.
 * ReLU as torch.relu (NaN stays NaN); its gradient as torch's threshold_backward (0 where y <= 0, dy elsewhere -- a NaN y lets dy through).
 * m3t_amax_out arms the magnitude slot of y / yp (forward) and of dx (backward): one 64-bit atomic max per workgroup.
 * dx_colsum [C] (optional): the column sums of dx -- the bias gradient of the convolution in front -- from the dx pass itself: fp64 per thread,
 *   per workgroup and over the workgroups in a fixed order (no float atomics; reruns are bit-identical); needs ws of m3t_relu_cl_ws_bytes(M, C)
 *   bytes, 8-B aligned (M = P H W for the pooled operator).
 * m3t_relu_cl_fwd / _bwd (models/vggface.py:45-50, line 49): y = relu(x) over rows [M][C], y == x allowed; dx = dy where y > 0 (dx == dy allowed).
 * m3t_relu_pool_cl_fwd / _bwd (models/vggface.py:45-50, lines 49-50): ReLU then a 2 x 2 max pooling with stride 2 and no padding over P frames
 *   x [P][H][W][C] as ONE operator; Ho = ceil_mode ? (H + 1) / 2 : H / 2 (W alike), a ragged last window covers only the positions inside the
 *   frame.  relu(x) at full resolution is neither written nor kept: forward writes yp [P][Ho][Wo][C] and one winner byte per element (dh * 2 +
 *   dw; ties: the first maximum in window order, NaN wins, as torch); backward takes d(yp), yp and the bytes -- not x -- and writes dx
 *   [P][H][W][C] by a gather over the input positions: d(yp) of the position's window where it won and yp > 0, else 0. */
size_t m3t_relu_cl_ws_bytes(size_t M, int C);
int m3t_relu_cl_fwd(const float* x, size_t M, int C, float* y, void* stream);
int m3t_relu_cl_bwd(const float* dy, const float* y, size_t M, int C, float* dx, float* dx_colsum, float* ws, size_t ws_bytes, void* stream);
int m3t_relu_pool_cl_fwd(const float* x, size_t P, int H, int W, int C, int ceil_mode, float* yp, unsigned char* win, void* stream);
int m3t_relu_pool_cl_bwd(const float* dyp, const float* yp, const unsigned char* win, size_t P, int H, int W, int C, int ceil_mode, float* dx,
                         float* dx_colsum, float* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * TCN (models/tcn.py).  Activations are channel-last [B,T,C] inside the library.
 * weight-norm reparametrisation (torch.nn.utils.weight_norm at models/tcn.py:19-20):
 *   w[co][ci][j] = g[co] * v[co][ci][j] / ||v[co]||;  output layout w_t[j][co][ci]
 *   (tap-major, so each tap is a K-contiguous [C_out,C_in] matrix); norm[co] saved. */
int m3t_weight_norm_fwd(const float* v, const float* g, float* w_t, float* norm,
                        int Co, int Ci, int K, void* stream);
/* dw_t [K][Co][Ci] -> dv [Co][Ci][K], dg [Co] */
int m3t_weight_norm_bwd(const float* dw_t, const float* v, const float* g, const float* norm,
                        float* dv, float* dg, int Co, int Ci, int K, void* stream);

/* Dilated causal conv (Conv1d(pad=(k-1)d, dil=d) + Chomp1d, models/tcn.py:7-13,19-21),
 * channel-last, left zero padding, halo staged in LDS:
 *   y[b,t,co] = act( bias[co] + sum_{j,ci} w_t[j][co][ci] * x[b, t-(K-1-j)*d, ci] (+ res[b,t,co]) )
 * act: 0 none, 1 ReLU, 2 ReLU(ReLU(conv) + res) (the block output, models/tcn.py:46);
 * pre (optional, [B,T,Co]) receives the pre-activation conv output (+bias) for backward.
 * drop_mask (optional, [B,T,Co], already scaled by 1/(1-p)) multiplies the ReLU output
 * (nn.Dropout after relu1/relu2 in train mode, models/tcn.py:23,29); NULL in eval mode.
 * anticausal!=0 flips the time direction (x[b, t+(K-1-j)*d]) -- the data-gradient conv. */
int m3t_causal_conv_fwd(const float* x, const float* w_t, const float* bias, const float* res,
                        const float* drop_mask, float* y, float* pre,
                        int B, int T, int Ci, int Co, int K, int dilation,
                        int act, int anticausal, void* stream);
/* dw_t[j][co][ci] = sum_{b,t} dy[b,t,co] * x[b, t-(K-1-j)*d, ci] */
int m3t_causal_conv_wgrad(const float* dy, const float* x, float* dw_t,
                          int B, int T, int Ci, int Co, int K, int dilation,
                          float* ws, size_t ws_bytes, void* stream);
/* General 1-D conv over channel-last rows with `lead` frames of look-ahead (0 <= lead <= (K-1)*d):
 *   y[b,t,co] = act( bias[co] + sum_{j,ci} w_t[j][co][ci] * x[b, t + lead - (K-1-j)*d, ci] ... )
 * lead = 0 is m3t_causal_conv_fwd; lead = pad is nn.Conv1d(k, stride 1, padding=pad) with 2*pad = (K-1)*d --
 * the `tcn_simple` back-end's Conv1d(.,.,5,1,2) / Conv1d(.,.,3,1,1) (reference models/backbone.py:107-111,
 * 214-231).  anticausal != 0 flips time (x[b, t - lead + (K-1-j)*d]): the data gradient.
 * flags: 0 or M3T_BF16 (x and w rounded to bf16 while staged; fp32 accumulate and epilogue).
 * Dropout (nn.Dropout(p) behind each ReLU of the TemporalBlock, reference models/tcn.py:17,23,29): either an explicit
 * pre-scaled mask tensor `drop_mask` [B*T, Co], or drop_p in (0, 1) with drop_mask = NULL: the mask is then generated IN the
 * epilogue -- element (row, col) keeps its value x 1/(1-p) iff word (row & 3) of Philox4x32-10(counter {col, row >> 2, 0, 0},
 * key drop_seed) < (1-p) * 2^32 -- and never exists in memory; m3t_mask_pos_drop regenerates it for the backward pass.
 * Interior shapes ((B*T) % 128 == 0, Co % 128 == 0, Ci % 32 == 0, 16-B aligned operands) run as an implicit GEMM on the
 * bf16 matrix pipe (fp32-accurate bf16x6 products; one bf16 product with M3T_BF16); env M3T_CONV_X6=0 keeps the fp32-MFMA kernel. */
int m3t_conv1d_fwd(const float* x, const float* w_t, const float* bias, const float* res,
                   const float* drop_mask, float* y, float* pre,
                   int B, int T, int Ci, int Co, int K, int dilation, int lead, int act, int anticausal,
                   float drop_p, unsigned long long drop_seed, int flags, void* stream);
/* dw_t[j][co][ci] = sum_{b,t} dy[b,t,co] * x[b, t + lead - (K-1-j)*d, ci] */
int m3t_conv1d_wgrad(const float* dy, const float* x, float* dw_t,
                     int B, int T, int Ci, int Co, int K, int dilation, int lead,
                     float* ws, size_t ws_bytes, int flags, void* stream);
/* m3t_conv1d_fwd / m3t_conv1d_wgrad with the callers' magnitude slots for M3T_GEMM_F16X3 (see m3t_sgemm_scaled; NULL = measured by the
 * library): amax_x over x [B*T][Ci], amax_w over w_t, amax_dy over dy [B*T][Co].  The K taps of a weight gradient share both. */
int m3t_conv1d_fwd_scaled(const float* x, const float* w_t, const float* bias, const float* res,
                          const float* drop_mask, float* y, float* pre,
                          int B, int T, int Ci, int Co, int K, int dilation, int lead, int act, int anticausal,
                          float drop_p, unsigned long long drop_seed, int flags,
                          const unsigned long long* amax_x, const unsigned long long* amax_w, void* stream);
int m3t_conv1d_wgrad_scaled(const float* dy, const float* x, float* dw_t,
                            int B, int T, int Ci, int Co, int K, int dilation, int lead,
                            float* ws, size_t ws_bytes, int flags,
                            const unsigned long long* amax_dy, const unsigned long long* amax_x, void* stream);

/* BatchNorm1d (+ optional fused ReLU) over channel-last rows x [M = B*T, C]
 * (nn.BatchNorm1d(512) + nn.ReLU(True) of `tcn_simple`, reference models/backbone.py:108-110, 217-222).
 * training != 0: batch statistics (biased variance for normalisation; run_mean/run_var, when given, are
 * updated in place with `momentum` and the unbiased variance, as torch); training == 0: running statistics.
 * save_mean / save_invstd [C] receive the statistics used (needed by the backward).
 * ws: m3t_bn_rows_ws_bytes(M, C) bytes, 8-byte aligned (fp64 per-chunk partial sums, fixed-order reduce). */
size_t m3t_bn_rows_ws_bytes(int M, int C);
int m3t_bn_rows_fwd(const float* x, int M, int C, const float* gamma, const float* beta,
                    float* run_mean, float* run_var, float momentum, float eps, int training, int relu,
                    float* y, float* save_mean, float* save_invstd, float* ws, size_t ws_bytes, void* stream);
/* g = dy * (y > 0) when relu; dbeta = sum g, dgamma = sum g*xhat,
 * training: dx = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat));  eval: dx = g*gamma*invstd */
int m3t_bn_rows_bwd(const float* dy, const float* x, const float* y, const float* gamma,
                    const float* save_mean, const float* save_invstd, int M, int C, int training, int relu,
                    float* dx, float* dgamma, float* dbeta, float* ws, size_t ws_bytes, void* stream);
/* BatchNorm3d (+ optional fused ReLU) of the 3-D conv stems, channels-first x [N][C][S] with S = T*H*W contiguous (nn.BatchNorm3d(C) + nn.ReLU(True),
 * reference models/backbone.py:73-103,179-191): same statistics / running-statistics / gradient formulas as the rows form above with M = N*S values per
 * channel.  ws: m3t_bn_planes_ws_bytes(N, C, S) bytes, 8-byte aligned.  (One workgroup per plane chunk of <= 8192 floats: made for the stems'
 * large planes; planes of a few dozen floats work but waste the workgroup.) */
size_t m3t_bn_planes_ws_bytes(int N, int C, int S);
int m3t_bn_planes_fwd(const float* x, int N, int C, int S, const float* gamma, const float* beta, float* run_mean, float* run_var,
                      float momentum, float eps, int training, int relu, float* y, float* save_mean, float* save_invstd,
                      float* ws, size_t ws_bytes, void* stream);
int m3t_bn_planes_bwd(const float* dy, const float* x, const float* y, const float* gamma, const float* save_mean, const float* save_invstd,
                      int N, int C, int S, int training, int relu, float* dx, float* dgamma, float* dbeta, float* ws, size_t ws_bytes,
                      void* stream);
/* nn.MaxPool3d with a (1, kh, kw) window (stride (1, sh, sw), padding (0, ph, pw), floor mode: the 3-D stems' pooling layers, reference
 * models/backbone.py:80,86,92,182) as the 2-D pooling of P = N*C*T planes x [P][H][W] -> y [P][Ho][Wo].  win [P][Ho][Wo] (one byte per
 * output): the winner's position inside its window, dh * kw + dw (kh * kw <= 255), for the backward pass, which is a gather (no atomics:
 * overlapping windows are deterministic).  Ties: the first maximum in row-major window order; NaN wins (torch's kernel). */
int m3t_pool_planes_fwd(const float* x, long long P, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw, float* y,
                        unsigned char* win, void* stream);
int m3t_pool_planes_bwd(const float* dy, const unsigned char* win, long long P, int H, int W, int kh, int kw, int sh, int sw, int ph, int pw,
                        float* dx, void* stream);
/* [B,C,T] <-> [B,T,C] */
int m3t_bct_to_btc(const float* src, float* dst, int B, int C, int T, void* stream);
int m3t_btc_to_bct(const float* src, float* dst, int B, int T, int C, void* stream);
/* m3t_bct_to_btc that also leaves, in part [B * ceil(T / 32)][C], the sums of every channel row over each tile of 32 positions: the column
 * sums of `part` (m3t_colsum) are the per-channel sums of src over (B, T) -- the conv3d bias gradient without another pass over dy */
int m3t_bct_to_btc_sums(const float* src, float* dst, int B, int C, int T, float* part, void* stream);
/* ... straight to the m3t_f16x3_split IMAGE of the channels-last rows (round 6): for a source whose magnitude slot its producer raised
 * (m3t_bn_planes_fwd / _bwd take m3t_amax_out for their y / dx), so that transpose and split are one pass; part as m3t_bct_to_btc_sums
 * or NULL.  C % 4 == 0, 16-B aligned destination. */
int m3t_bct_to_btc_img(const float* src, float* dst_img, int B, int C, int T, const unsigned long long* slot, float* part, void* stream);
/* out[i] = s[i] > 0 ? dy[i] * (mul ? mul[i] : 1) : 0   (ReLU / dropout gradient masks) */
int m3t_mask_pos(const float* s, const float* dy, const float* mul, float* out, size_t n, void* stream);
/* out[i] = max(a[i] + b[i], 0): the residual add + ReLU at the end of a ResNet block (reference models/resnet.py:52-54, 84-86) in one pass;
 * its gradient to both inputs is m3t_mask_pos(out, dout).  Takes m3t_amax_out (max |out|). */
int m3t_add_relu(const float* a, const float* b, float* out, size_t n, void* stream);
/* out[row, col] = s > 0 ? dy * mask(row, col) : 0 over [rows, C] with m3t_conv1d_fwd's in-kernel dropout mask regenerated from
 * (drop_p, drop_seed): the gradient through ReLU -> Dropout without a mask tensor. */
int m3t_mask_pos_drop(const float* s, const float* dy, float* out, int rows, int C, float drop_p,
                      unsigned long long drop_seed, void* stream);

/* ---------------------------------------------------------------------------------
 * CBAM (models/cbam.py), x [N,C,H,W] contiguous.
 * Channel gate (cbam.py:51-58): avg+max over H*W per (n,c) by wavefront shuffles,
 * shared MLP C -> C/r -> C, sigmoid, scale.  pooled [N,2,C] (avg,max), argmax [N,C] int32,
 * hidden [N,2,Cr] pre-ReLU, scale [N,C] are saved for backward. */
int m3t_cbam_channel_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                         float* y, float* pooled, int32_t* argmax, float* hidden, float* scale,
                         int N, int C, int Cr, int HW, void* stream);
int m3t_cbam_channel_bwd(const float* dy, const float* x, const float* w1, const float* w2,
                         const float* pooled, const int32_t* argmax, const float* hidden, const float* scale,
                         float* dx, float* dw1, float* db1, float* dw2, float* db2,
                         int N, int C, int Cr, int HW, float* ws, size_t ws_bytes, void* stream);
/* Spatial gate (cbam.py:61-92): per-pixel (max,mean) over C -> 5x5 conv 2->1 (pad 2) ->
 * BatchNorm2d(1) (training: batch statistics, running stats updated with `momentum`,
 * unbiased running variance) -> sigmoid -> scale.
 * bn = {gamma, beta}; running = {mean, var} (updated in place when training).
 * saved: comp [N,2,HW], cargmax [N,HW] int32, xhat [N,HW], stats[2] = {mean, invstd}, scale [N,HW]. */
int m3t_cbam_spatial_fwd(const float* x, const float* conv_w, const float* bn, float* running,
                         float* y, float* comp, int32_t* cargmax, float* xhat, float* stats, float* scale,
                         int N, int C, int H, int W, int training, float momentum, float eps,
                         float* ws, size_t ws_bytes, void* stream);
int m3t_cbam_spatial_bwd(const float* dy, const float* x, const float* conv_w, const float* bn,
                         const float* comp, const int32_t* cargmax, const float* xhat, const float* stats,
                         const float* scale, float* dx, float* dconv_w, float* dbn,
                         int N, int C, int H, int W, int training, float* ws, size_t ws_bytes, void* stream);

/* CBAM as ONE fused operator (reference models/cbam.py:95-111: SpatialGate(ChannelGate(x))), csrc/cbam_fused.hip: the
 * intermediate x * channel_scale is never written; forward = 2 sweeps (per-frame squeeze + MLP + compress + 5x5 conv | apply),
 * cut only by BatchNorm2d(1)'s global batch statistics, backward = 2 sweeps likewise: 8 HBM passes over a tensor of x's size
 * for forward + backward against 10 + for the two separate gates above, 6 launches + the two-launch parameter-gradient finish.
 * Frames of at most 64 KB with H*W <= 64 (the 7 x 7 and 4 x 4 ResNet-18 stages; C*H*W % 4 == 0, x / dy / dx 16-B aligned) take
 * frame-resident kernels (the frame parked in LDS, read once; environment M3T_CBAM_RESIDENT=0 keeps them on the general kernels):
 * same arithmetic per element, another fixed summation order.
 * Saved for backward: cs [N,C] (channel scale), argmax_p [N,C], pooled [N,2,C], hidden [N,2,Cr], comp [N,2,HW] (max, mean of
 * x * cs over channels), cargmax [N,HW], xhat [N,HW], ss [N,HW] (spatial scale), stats [2] (mean, 1/sqrt(var+eps)).
 * bn_w / bn_b = BatchNorm2d(1)'s gamma / beta (one float each), running_mean / running_var updated in place when training.  m3t_cbam_fused_ok: 1 when the
 * shape is covered (H*W/4 <= 512 float4 units, or H*W <= 512 pixels when H*W % 4 != 0); otherwise use the two gates above.
 * ws: forward 16 N bytes (8-B aligned), backward m3t_cbam_fused_ws_bytes (16-B aligned).  Results equal the two-operator
 * path to fp32 rounding (other summation order); deterministic. */
int m3t_cbam_fused_ok(int C, int Cr, int H, int W);
size_t m3t_cbam_fused_ws_bytes(int N, int C, int Cr, int H, int W);
int m3t_cbam_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                 const float* conv_w, const float* bn_w, const float* bn_b, float* running_mean, float* running_var,
                 float* y, float* cs, int32_t* argmax_p,
                 float* pooled, float* hidden, float* comp, int32_t* cargmax, float* xhat, float* ss, float* stats,
                 int N, int C, int Cr, int H, int W, int training, float momentum, float eps, float* ws,
                 size_t ws_bytes, void* stream);
int m3t_cbam_bwd(const float* dy, const float* x, const float* w1, const float* w2, const float* conv_w,
                 const float* bn_w, const float* cs, const int32_t* argmax_p, const float* pooled,
                 const float* hidden, const float* comp, const int32_t* cargmax, const float* xhat, const float* ss,
                 const float* stats, float* dx, float* dw1, float* db1, float* dw2, float* db2, float* dconv_w,
                 float* dbn_w, float* dbn_b, int N, int C, int Cr, int H, int W, int training, float* ws,
                 size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Data-parallel helpers (train.py:32-41: DDP mean of gradients + clip_grad_norm_(1.0)).
 * After the RCCL all-reduce(sum) of the flat gradient buffer: one pass computes
 * sum(g^2) of g/world (partials[blocks] + final), a second scales by
 * (1/world) * min(1, max_norm/(norm+1e-6)).  norm_out[0] = total norm (pre-clip).
 * When that factor is exactly 1 (world 1 and nothing to clip) the buffer is not written at all.  The sum of squares is an
 * fp32 sum (per-thread partials, a block tree, then <= 1024 block partials).  Edges: an all-zero buffer gives norm 0 and stays
 * untouched; elements whose squares underflow (|g| < ~1e-23) do not count, so a buffer of such elements reads norm 0 and is
 * not clipped; a NaN or inf element, or a sum of squares beyond FLT_MAX although the true norm is representable (4099
 * elements of 1e20), gives a norm that is not finite -- the optimizer steps it guards are then skipped, and the contents of
 * the buffer are unspecified (max_norm / inf = 0 scales it to zero). */
int m3t_grad_norm_scale(float* flat, size_t n, float inv_world, float max_norm,
                        float* norm_out, float* ws, size_t ws_bytes, void* stream);
/* One rank's dead scan must stop every rank: the all-reduce would otherwise spread its garbage while only the failing
 * rank's guard fires.  m3t_grad_poison, BEFORE the all-reduce: if this process's scan error flag is set, flat[0] = NaN (SUM
 * carries it to every rank: every clip norm is NaN, every fused optimizer step skips) and dead[0] = 1, else dead[0] = 0
 * (`dead`: one float of padding that rides in the same all-reduce; NULL = skip).  m3t_grad_dead_check, AFTER the
 * all-reduce: dead[0] != 0 raises this process's scan error flag as well, so every rank's next poll reports the failure
 * (a healthy rank would otherwise wait in its next collective for the rank that raised).  One thread each, stream-ordered. */
int m3t_grad_poison(float* flat, float* dead, void* stream);
int m3t_grad_dead_check(const float* dead, void* stream);

/* ---------------------------------------------------------------------------------
 * Optimizer steps over the flat parameter / gradient buffers (reference
 * models/model.py:388-394).  torch.optim semantics: Adam(lr, betas, eps, weight_decay as L2 on the gradient,
 * bias-corrected, `step` counts from 1); SGD(momentum, weight_decay), dampening 0, no Nesterov.
 * The hyperparameters are the fp32 values passed, and `1 - beta` is formed from them: beta2 = 0.999 arrives as
 * 0.99900001287..., the kernel runs Adam with that value and the bias corrections are computed (in double) from the same
 * value.  A float64 reference must round the hyperparameters to fp32 first to agree to rounding level (tests/optim_ref.py).
 * m3t_adam_step reads and writes float4: p, g, m, v 16-byte aligned, else M3T_EINVAL; m3t_sgd_step takes any alignment.
 * step < 1: M3T_EINVAL.  Nothing is launched on a refused call. */
int m3t_adam_step(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, int step, const float* guard, void* stream);
int m3t_sgd_step(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay,
                 int step, const float* guard, void* stream);
/* guard: optional device scalar (the norm m3t_grad_norm_scale returned).  When it is not finite the kernel changes
 * nothing (parameters and optimizer state keep their values): a step whose gradients came from a failed scan, or
 * overflowed, is skipped on the device.
 * A skipped step still counts: the host cannot know that the device skipped without synchronising, so m3t.optim's
 * FlatAdam / FlatSGD advance `step` on every call.  After a skipped step Adam's bias corrections are those of a larger
 * `step` than the number of updates taken (clean, skipped, clean = the updates of step 1 and step 3); for SGD a skipped
 * first step is harmless: with buf = 0, momentum * buf + g is the first step's buf = g. */

/* ---------------------------------------------------------------------------------
 * Post-processing of prediction tracks (reference models/utils.py:20-33,
 * get_smoothed_ccc.py:13-28, create_submission.py:30-38).
 * n_tracks tracks are concatenated in x; track i = x[offsets[i] .. offsets[i+1]) (offsets: n_tracks+1 int64 on the
 * device).  mode 0 = scipy.signal.wiener(track, window), mode 1 = scipy.signal.medfilt(track, window): centred odd
 * window (<= 129), zero padding, fp64 arithmetic on the fp32 input (squares rounded to fp32 first, as scipy does);
 * y (fp64) has the layout of x. */
int m3t_smooth_tracks(const float* x, const long long* offsets, int n_tracks, int window, int mode, double* y,
                      void* stream);
/* out2[0] = numpy-style CCC (biased variances) of p against g over the frames with g >= -1 (and g2 >= -1 when g2 is
 * given): models/utils.py:20-22 as driven by get_smoothed_ccc.py:19-21; p_unbiased != 0 uses the unbiased variance
 * for p (what the reference computes when the smoothed track is a torch tensor).  out2[1] = number of valid frames. */
int m3t_ccc_masked(const double* p, const float* g, const float* g2, long long n, int p_unbiased, double* out2,
                   void* stream);
/* m3t_ccc_masked on n_tracks tracks in one launch (get_smoothed_ccc.py:18-28, the loop over videos): track i = elements
 * offsets[i] .. offsets[i+1] of p (fp64), g and g2 (fp32; g2 may be null), offsets: n_tracks+1 int64 on the device.
 * out[i][0] = CCC, out[i][1] = number of valid frames: per track the bits m3t_ccc_masked gives (same passes, same
 * thread-to-element mapping, same reduction tree). */
int m3t_ccc_tracks(const double* p, const float* g, const float* g2, const long long* offsets, int n_tracks,
                   int p_unbiased, double* out, void* stream);

/* ---------------------------------------------------------------------------------
 * The evaluation epoch on the device (csrc/evaluate.hip; m3t/evaluate.py): the reference's validation_step /
 * validation_end / test_step / test_end (models/model.py:226-303, 339-373) without a host read-back per batch.
 * No kernel uses atomics; every sum is fp64 in a fixed order.
 *
 * m3t_eval_append, once per batch (model.py:228-246, 320-337: the slicing of y_hat and the labels by `length`):
 * y_hat [N][T][C] fp32, C >= 2, valence = channel C-2, arousal = channel C-1 (model.py:230); label_valence /
 * label_arousal [N][T] fp32, both or neither; length [N] int64 on the device (clamped to [0, T]).
 * rows [N][Q][T], Q = 4 with labels (v_pred, a_pred, v_gt, a_gt), else 2: frames t >= length[n] are 0 and their inputs
 * are not read.  With labels, part [N][2][7] fp64 = n, sum p, sum g, sum p^2, sum g^2, sum p g, sum (p-g)^2 of window n
 * over its valid frames -- t < length, |v_gt| <= 1 and |a_gt| <= 1 (model.py:254; NaN is not valid) -- for valence, arousal. */
int m3t_eval_append(const float* y_hat, int N, int T, int C, const float* label_valence, const float* label_arousal,
                    const long long* length, float* rows, double* part, void* stream);
/* m3t_eval_gather, once per epoch (model.py:261-297, 354-366: group by video, sort by start, overlap-add and halve, or
 * torch.cat): rows [W][Q][T] = the batches' rows concatenated; tracks [Q][F].  All tables int64 on the device: segment s
 * puts rows[seg_row[s]][q][0 .. seg_len[s]) at the frames seg_dst[s] .. of its video; video v owns the segments
 * vid_seg_off[v] .. vid_seg_off[v+1] (ascending seg_dst, no two equal) and the frames vid_frame_off[v] ..
 * vid_frame_off[v+1] of each track, vid_frame_off[V] = F.  Frame f of a video = 0.f + x_1 + x_2 ... over the segments
 * covering it in ascending seg_dst order, times 0.5f when f >= halve_from (window / 2 for overlap-add -- the tail covered
 * once is halved too, as in the reference; any value >= the longest video for concatenation).  Every frame is written once. */
int m3t_eval_gather(const float* rows, long long W, int Q, int T, const long long* seg_dst, const long long* seg_len,
                    const long long* seg_row, const long long* vid_seg_off, const long long* vid_frame_off, int V,
                    long long F, long long halve_from, float* tracks, void* stream);
/* m3t_eval_metrics, once per epoch (model.py:249-259 with models/utils.py:6-18): part [W][2][7] summed in window order ->
 * out5 = val_ccc_v, val_ccc_a, val_mse_v, val_mse_a, val_loss (fp64): unbiased variances, biased covariance,
 * val_loss = 1 - (ccc_v + ccc_a) / 2.  A frame counts once per window that holds it.  No valid frame: NaN. */
int m3t_eval_metrics(const double* part, long long W, double* out5, void* stream);

/* ---------------------------------------------------------------------------------
 * The expression head in the evaluation epoch (csrc/evaluate_expr.hip; m3t/evaluate.py, Evaluator(expr=True)).  The
 * reference trains the head (model.py:169-182) and never validates it; these entry points extend its masking and argmax
 * (model.py:171-182) and its stitching (model.py:261-297, 354-366) to the 7 expression logits, channels 0..6 of y_hat
 * (model.py:175).  Class rule everywhere: argmax over the 7 logits as torch.argmax (the first maximal index; a NaN counts
 * as maximal, so the first NaN wins); class -1 = none.  Classes travel as int8.  Counts are exact integers (LDS integer
 * atomics); no float atomics, every floating sum in a fixed order.
 *
 * m3t_eval_append_mtl, once per batch (model.py:171-182 for the mask and the argmax): everything m3t_eval_append does --
 * rows and part carry the same bits -- and, with C >= 9, expr_rows [N][7][T] fp32 = the 7 logits of frame t < length, 0
 * past it (inputs not read).  With labels (label_valence / label_arousal / class_expr / expr_valid: all or none):
 * class_expr [N][T] int64 (clipped to 0..6), expr_valid [N][T] one byte per frame; expr_gt [N][T] int8 = the label where
 * t < length and expr_valid, else -1; conf [N][7][7] int32 = the number of those frames with label g and prediction p. */
int m3t_eval_append_mtl(const float* y_hat, int N, int T, int C, const float* label_valence, const float* label_arousal,
                        const long long* class_expr, const unsigned char* expr_valid, const long long* length, float* rows,
                        double* part, float* expr_rows, signed char* expr_gt, int* conf, void* stream);
/* m3t_eval_gather_expr, once per epoch (model.py:261-297, 354-366): the plan tables of m3t_eval_gather.  logit_tracks
 * [7][F] fp32: per channel the sequence of m3t_eval_gather (zeros, += per covering segment in ascending start order,
 * * 0.5f from halve_from on).  pred [F] int8 = the argmax of the stitched logits, -1 for a frame no segment covers.
 * gt [F] int8 (nullable; needs expr_gt [W][T]) = the expr_gt of the first covering segment in start order, else -1. */
int m3t_eval_gather_expr(const float* expr_rows, const signed char* expr_gt, long long W, int T, const long long* seg_dst,
                         const long long* seg_len, const long long* seg_row, const long long* vid_seg_off,
                         const long long* vid_frame_off, int V, long long F, long long halve_from, float* logit_tracks,
                         signed char* pred, signed char* gt, void* stream);
/* m3t_eval_expr_metrics (the figures model.py:180-181 starts: acc_expr): conf [W][7][7] int32 ([label][prediction]) summed
 * over W -> out24 fp64 = accuracy, macro-F1, score = 0.67 F1 + 0.33 accuracy (the expression track of ABAW 2020), then
 * precision [7], recall [7], F1 [7].  F1_c = 2 tp / (2 tp + fp + fn); macro-F1 = the mean over the classes with
 * tp + fp + fn > 0, summed in class order (scikit-learn's f1_score(average='macro')).  A zero denominator is 0 / 0 = NaN:
 * every figure without a valid frame, precision of a class never predicted, recall of a class never labelled. */
int m3t_eval_expr_metrics(const int* conf, long long W, double* out24, void* stream);
/* Mode filter over class tracks (int8, the offsets table of m3t_smooth_tracks), odd window = 2h+1 > 0 (else M3T_EINVAL):
 * out[i] = the most frequent class among c[max(0,i-h) .. min(n-1,i+h)] of its track, -1 ignored, no padding; a tie goes to
 * c[i] when it is among the tied classes, else to the smallest; nothing but -1 in reach gives -1.  window 1: identity. */
int m3t_expr_mode_tracks(const signed char* c, const long long* offsets, int n_tracks, int window, signed char* out,
                         void* stream);
/* conf [n_tracks][7][7] int32 = per track the frames with gt = g >= 0 and pred = p >= 0; acc [n_tracks] fp64 (nullable) =
 * the track's accuracy, NaN without such a frame.  m3t_eval_expr_metrics scores conf with W = n_tracks. */
int m3t_expr_track_conf(const signed char* pred, const signed char* gt, const long long* offsets, int n_tracks, int* conf,
                        double* acc, void* stream);

/* ---------------------------------------------------------------------------------
 * Audio front-end: the glue kernels of the log-Mel pipeline that the reference runs offline with
 * librosa (process/extract_melspec.py:13-20) and the context stacking of models/dataset.py:83-95.  The DFT and the
 * mel projection themselves are m3t_sgemm calls (see m3t/audio.py).
 * frames[f][k] = window[k] * ypad[f*hop + k], ypad = y with n_fft/2 samples of padding per side
 * (pad_mode 0 zeros, 1 reflect); n_frames = 1 + n / hop. */
int m3t_frame_window(const float* y, long long n, int n_fft, int hop, int pad_mode, const float* window,
                     float* frames, long long n_frames, void* stream);
/* spec [n_frames][2*bins] = (re | im) -> power [n_frames][bins] = re^2 + im^2 */
int m3t_power_spectrum(const float* spec, long long n_frames, int bins, float* power, void* stream);
/* librosa.power_to_db(S, ref=1.0, amin, top_db): 10 log10(max(amin, S)), floored at (max - top_db) when top_db >= 0.
 * ws: >= 2 KiB of scratch. */
int m3t_power_to_db(const float* s, long long n, float amin, float top_db, float* out, float* ws, size_t ws_bytes,
                    void* stream);
/* out [w_len][width*n_mels]: row i = mel rows (start+i)*step .. +width concatenated, zero rows past the end */
int m3t_stack_context(const float* mel, long long n_rows, int n_mels, long long start, int w_len, int step, int width,
                      float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Batched audio ingest (csrc/audio_ingest.hip): the reference's AudioSet loader (models/audioset_dataset.py:58-87) for a whole batch of
 * decoded clips, and the AffWild2 loader's stacking of pre-extracted tracks (models/dataset.py:83-95, :276-306).  A batch is a FLAT buffer
 * plus per-clip tables on the device (the style of m3t_smooth_tracks' offsets); clips are not padded to a common length.  The pipeline of
 * m3t.audio.ingest: m3t_audio_frame_batch -> m3t_sgemm ([R, n_fft] x [n_fft, 2 bins], one product) -> m3t_audio_power_mel -> m3t_audio_db_stack.
 * clips: device long long [N][8] = off, len, start, nsamples, hop, nf, row_off, 0.  Clip n owns the samples wave[off .. off + len) of the
 * n_samples in `wave`; its rows are row_off .. row_off + nf of the R rows of the batch, nf = 1 + nsamples / hop.  No kernel synchronises,
 * uses float atomics or reduces in a data-dependent order.  A table entry that does not fit the buffers (off + len > n_samples,
 * row_off + nf > R, a negative or zero size) is caught on the device: that clip's frames are not written / its output is zeros, and no byte
 * outside the buffers is touched.  Every entry point: M3T_EINVAL for null or misaligned pointers (wave: its element size, tables: 8 bytes,
 * floats and ints: 4) and non-positive sizes; N == 0 (or no rows / frames to write) returns 0.
 *
 * Framing (audioset_dataset.py:63-70 and librosa.stft(center=True), process/extract_melspec.py:13-20).  For clip n, frame f < nf, tap k < n_fft:
 *     c[j]       = wave[off + (start + j) mod len],  0 <= j < nsamples     (the temporal crop; the modulo is np.pad(y, (0, nsamples - len + 5),
 *                                                                           'wrap') of :65-68 for any start, and no sample wraps when
 *                                                                           start + nsamples <= len)
 *     cpad       = c with n_fft / 2 samples of padding per side (pad_mode 0: zeros, librosa >= 0.10; 1: numpy 'reflect' of the CROP)
 *     frames[row_off + f][k] = window[k] * cpad[f * hop + k]
 * dtype 0: wave is float32; 1: int16, scaled by 1 / 32768 (exact in fp32).  n_fft even.  m3t_frame_window on the crop of one clip gives
 * the same values. */
int m3t_audio_frame_batch(const void* wave, int dtype, long long n_samples, const long long* clips, int N, long long R, int n_fft,
                          int pad_mode, const float* window, float* frames, void* stream);
/* spec [R][2 bins] = (re | im) of the DFT product -> mel [R][n_mels]: mel[r][b] = sum_q weights[bands[b] + q] * |X[r][first_b + q]|^2 for
 * q < bands[b + 1] - bands[b], an fp32 sum in bin order (librosa.feature.melspectrogram's `mel_basis @ |stft|^2` on the non-zero entries of
 * the filterbank only: a Slaney band is one run of bins, a bin feeds at most two bands).  bands: device int [2 n_mels + 1] = n_mels + 1
 * offsets into weights [nnz], then first_b per band; entries are clamped into [0, nnz] / [0, bins] on the device.
 * Limits: bins <= 2048, n_mels <= 64, nnz <= 4096. */
int m3t_audio_power_mel(const float* spec, long long R, int bins, int n_mels, const float* weights, const int* bands, int nnz,
                        float* mel, void* stream);
/* mel [R][n_mels] -> out [N][T][width n_mels].  Per clip n (one workgroup, two passes), with S = its rows row_off .. row_off + nf:
 *     mx   = max over ALL nf rows of 10 log10(max(amin, S))         (another clip's rows are never seen; rows no output frame shows count)
 *     db   = 10 log10(max(amin, S)) - 10 log10(max(amin, 1)),  floored at mx - 10 log10(max(amin, 1)) - top_db when top_db >= 0
 *            (librosa.power_to_db(S, ref=1.0, amin, top_db), audioset_dataset.py:76)
 *     out[n][t][k n_mels + c] = t step + k < nf ? db[t step + k][c] : 0.0f         (audioset_dataset.py:77-85 with step 3, width 5: the
 *                                                                                 reference's zero padding, not the dB floor)
 * Of `clips` only nf and row_off are read.  T width n_mels < 2^31, amin > 0. */
int m3t_audio_db_stack(const float* mel, long long R, const long long* clips, int N, int T, int n_mels, int step, int width,
                       float amin, float top_db, float* out, void* stream);
/* m3t_audio_db_stack with the training-time augmentation of the AudioSet feed, in the same single launch: the reference's spec_augment
 * (models/audioset_dataset.py:17-55), run as if its load_audio called it on the dB spectrogram [1, n_mels, nf] between power_to_db (:76)
 * and the stacking (:77-85), and a mix across the batch (mixup; beyond the reference) applied after the masks.
 * aug: device int [N][20] = n_freq, n_time, partner, 0, (f0, f) x 4, (t0, t) x 4.  mixw: device float [N][2] = lam32, om32.
 * Per clip n, with db and nf as in m3t_audio_db_stack (the clip's own maximum and floor):
 *     x[n][t][k n_mels + c] = 0.0f  if t step + k >= nf, or f0 <= c < f0 + f for one of its n_freq frequency masks, or
 *                                   t0 <= t step + k < t0 + t for one of its n_time time masks       (an assignment: a NaN or inf cell
 *                                   becomes 0.0f; csrc/audio_aug_core.h is this rule, shared with csrc/audio_aug_host_check.cpp)
 *                           = db[t step + k][c]  otherwise
 *     partner == -1:  out[n] = x[n], no multiply
 *     partner >= 0 :  out[n] = __fadd_rn(__fmul_rn(lam32, x[n]), __fmul_rn(om32, x[partner]))   (x[partner]: that clip's own nf, floor, masks)
 * One workgroup per OUTPUT clip: it reduces its own maximum and, when mixing, the partner's; no atomics, a rerun gives the same bits.
 * Counts are clamped into [0, 4]; a mask is only compared with a position, never used as an address; a partner outside [-1, N) gives a
 * zero clip.  The host (m3t.audio.plan_aug) refuses all of these before the launch.  M3T_EINVAL as m3t_audio_db_stack, and for a null or
 * misaligned aug / mixw. */
int m3t_audio_db_stack_aug(const float* mel, long long R, const long long* clips, int N, const int* aug, const float* mixw, int T,
                           int n_mels, int step, int width, float amin, float top_db, float* out, void* stream);
/* The AffWild2 route (dataset.py:83-95, :276-278, :302-306) for N pre-extracted tracks in one launch.  mels: flat [total_rows][n_mels];
 * tracks: device long long [N][4] = row_off, n_rows, start, track_len.  out [N][window][width n_mels]:
 *     i' = min(i, track_len - 1)                                      (rows track_len .. window-1 repeat the last: np.pad 'edge', :303-304)
 *     out[n][i][k n_mels + c] = r < n_rows ? mels[row_off + r][c] : 0.0f,  r = (start + i') step + k       (m3t_stack_context's row)
 * track_len == 0 gives a zero clip (dataset.py:277-278, fps < 15); 0 <= track_len <= window, start >= 0, row_off + n_rows <= total_rows
 * (a track that violates this is a zero clip). */
int m3t_stack_context_batch(const float* mels, long long total_rows, int n_mels, const long long* tracks, int N, int window,
                            int step, int width, float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * The AudioSet label rows (csrc/audioset.hip; m3t.audioset.WaveStore): the reference's loader builds one float32 multi-hot vector per listed
 * clip when it scans the folder and hands a batch a stack of them (models/audioset_dataset.py:116-118, :131).  Here the vectors of a split
 * stay on the device as ONE uint8 matrix table [n_files][n_classes] (0 / 1), and one launch writes a batch's rows:
 *     out[n][c] = (float) table[items[n]][c],   n < N, c < n_classes           (out: float32 [N][n_classes])
 * items: device long long [N], the clips' indices into the table; a repeat is allowed.  A flat grid-stride over N * n_classes cells, byte
 * loads and float stores, no atomics, no order.  An item outside [0, n_files) leaves its row of `out` untouched and reads nothing; the host
 * refuses such an item before the launch (m3t.audioset).  M3T_EINVAL: null pointers, items not 8-byte or out not 4-byte aligned, n_files or
 * n_classes <= 0, N < 0; N == 0 returns 0. */
int m3t_label_rows(const uint8_t* table, long long n_files, int n_classes, const long long* items, int N, float* out, void* stream);
/* m3t_label_rows for a batch mixed by m3t_audio_db_stack_aug (the mix that follows the reference's spec_augment,
 * models/audioset_dataset.py:17-55; aug and mixw are that launch's tables, of which only the partner and the two weights are read):
 *     partner == -1:  out[n][c] = (float) table[items[n]][c]
 *     partner >= 0 :  out[n][c] = __fadd_rn(__fmul_rn(lam32, (float) table[items[n]][c]), __fmul_rn(om32, (float) table[items[partner]][c]))
 * An item outside [0, n_files) (the row's own or its partner's) or a partner outside [-1, N) leaves the row untouched and reads nothing.
 * M3T_EINVAL as m3t_label_rows, and for a null or misaligned aug / mixw. */
int m3t_label_rows_mix(const uint8_t* table, long long n_files, int n_classes, const long long* items, int N, const int* aug,
                       const float* mixw, float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Wave conversion (csrc/resample.hip; m3t.audio.decode_waves): what `librosa.load(path, sr=16000)` does to a file before the reference
 * sees a sample (models/audioset_dataset.py:61, process/extract_melspec.py:13) -- decode to float32, down-mix to mono, resample to 16 kHz
 * with resampy's 'kaiser_best' filter, pad to ceil(frames * 16000 / rate) -- for a ragged batch of clips of ONE source rate in one launch.
 * The rule is DESIGN.md 4c: the project's own restatement of libsndfile, librosa 0.7 and resampy 0.2.2, not a run of them.
 * bytes: the clips' raw interleaved 'data' bodies in one device buffer of n_bytes (4-byte aligned).
 * clips: device long long [N][8] = byte offset, frames, channels (1..8), kind (0 u8, 1 i16, 2 i24, 3 i32, 4 f32), output offset, n_res,
 *        n_out, tile prefix.  A clip's offset is a multiple of its sample size (1 for i24); its outputs are out[output offset .. + n_out);
 *        n_res = int(frames * ratio), n_out = int(ceil(frames * ratio)) in float64, ratio = 16000.0 / rate; it owns the workgroups
 *        tile prefix .. + ceil(n_out / 256) of the n_tiles of the launch (the prefix is non-decreasing: the kernel searches it).
 * Sample to float: (u8 - 128) / 128, i16 / 32768, i24 / 8388608, i32 / 2147483648 rounded once, float32 as stored; mono = the channels
 * summed in order in fp32, divided by their count (one channel: the sample itself).
 * rate == 16000: out[t] = mono[t]; table and starts are not read.
 * Otherwise, with scale = min(1, ratio), step = int(scale * 512), r_0 = 0.0, r_{t+1} = r_t + rate / 16000.0 in float64:
 *     n = int(r_t), frac = scale (r_t - n)
 *     out[t] =   sum_{i < min(n + 1, (32769 - o) / step)}          w(o + i step) mono[n - i],      o, eta from frac 512
 *              + sum_{k < min(frames - n - 1, (32769 - o') / step)} w(o' + k step) mono[n + k + 1],  o', eta' from (scale - frac) 512
 *     w(j) = table[j][0] + eta table[j][1]                                  for t < n_res;   out[t] = 0.0f for n_res <= t < n_out
 * accumulated in ONE fp32 value in that order, in resampy's arithmetic: acc = float(double(acc) + w(j) * double(mono[.])), w(j) and the
 * product in fp64, every operation rounded on its own.  table: device double [32769][2] = (win, delta) of the half filter (already
 * multiplied by ratio when ratio < 1), 16-byte aligned.  starts: device double [n_starts], starts[s] = r_{64 s} as the sequential additions give it
 * (the host accumulates them once per rate; the lanes carry on with the same additions); n_starts >= 4 ceil(n_out / 256) of the longest
 * clip.  No atomics, nothing read back, reruns bit-identical.  A row that does not fit the buffers (or channels / kind out of range, a
 * misaligned offset, too few starts) is caught on the device: nothing of that clip is read or written; the host refuses it first
 * (m3t.audio.plan_convert).  M3T_EINVAL: null or misaligned pointers, non-positive sizes, a rate whose tile span does not fit 64 KB of LDS
 * (above about 600 kHz); N == 0 or n_tiles == 0 returns 0. */
int m3t_wave_convert(const uint8_t* bytes, long long n_bytes, const long long* clips, int N, long long n_tiles, int rate,
                     const double* table, const double* starts, long long n_starts, float* out, long long n_out_total, void* stream);

/* ---------------------------------------------------------------------------------
 * Video ingest: what the reference's two loaders do to pixels between the decoder and the first convolution (models/dataset.py:16-31,46-80
 * and :312, models/vox2_dataset.py:14-50, models/cv_augment.py:6-37) and the normalisation of models/model.py:106, in one pass over the
 * uint8 frames as decoded, frames [N][Ts][Hs][Ws][3] (channel order as stored).  For clip n, output frame t, pixel (y, x), channel c:
 *     f = frame_idx[n][t]                 (device [N][T]; NULL = identity, T <= Ts; -1 = "no frame yet": zeros, dataset.py:68; a missing
 *                                          frame repeats the previous index, dataset.py:67; a short window repeats its last, dataset.py:312)
 *     v = f < 0 ? 0 : frames[n][f][cy + y][cx + (mirror ? W-1-x : x)][c]
 *     o = (cut_y1 <= y < cut_y2 and cut_x1 <= x < cut_x2) ? 0.0f : lut[n][v]
 * geom: device [N][8] ints = cy, cx, mirror, cut_y1, cut_y2, cut_x1, cut_x2, 0.  lut: device float tables of 256 entries, lut_stride 256
 * = one per clip, 0 = one for all: (v - 127.5) / 127.5, with the two uint8 tables of cv_augment.py:16,33 composed in front of it for the
 * VoxCeleb2 colour jitter; the cutout's fill 127.5 (dataset.py:16) normalises to exactly 0.  The kernel only gathers: its values are the
 * table's bits.  Window and frame index are clamped into range on the device; no byte outside frames[0 .. N Ts Hs Ws 3) is read.
 * layout 0: out [N T H W][4], fourth channel 0 -- the image m3t_planes_to_cl4 writes; raises the slot armed by m3t_amax_out the same way.
 * layout 1: out [N][3][T][H][W].  frames and out 16-byte aligned, the tables 4-byte; H <= Hs, W <= Ws (about 1000 pixels per row at most).
 * M3T_EINVAL: null or misaligned pointers, non-positive sizes; N == 0 or T == 0 returns 0. */
int m3t_video_ingest(const uint8_t* frames, int N, int Ts, int Hs, int Ws, const int* frame_idx, int T, const int* geom,
                     const float* lut, int lut_stride, int H, int W, int layout, float* out, void* stream);
/* The same with the reference's 256-pixel branch in front (dataset.py:61,73: crop 224 x 224, cv2.resize to 112 x 112).  H, W are the OUTPUT
 * size; the crop window in the source is 2H x 2W at (cy, cx); mirror and cutout are in output coordinates:
 *     xs = mirror ? W-1-x : x
 *     s  = frames[n][f][cy+2y][cx+2xs][c] + frames[n][f][cy+2y][cx+2xs+1][c] + frames[n][f][cy+2y+1][cx+2xs][c] + frames[n][f][cy+2y+1][cx+2xs+1][c]
 *     v  = f < 0 ? 0 : (s + 2) >> 2
 *     o  = inside the cutout ? 0.0f : lut[n][v]
 * (s + 2) >> 2 is what OpenCV's resize gives 8-bit images at an exact factor of 2 on both axes (INTER_LINEAR takes the integer INTER_AREA
 * path there, by its published source; not checked against a run of it here).  Averaging then mirroring equals the reference's
 * resize-then-flip.  Everything else as m3t_video_ingest; M3T_EINVAL also for 2H > Hs or 2W > Ws. */
int m3t_video_ingest_half(const uint8_t* frames, int N, int Ts, int Hs, int Ws, const int* frame_idx, int T, const int* geom,
                          const float* lut, int lut_stride, int H, int W, int layout, float* out, void* stream);

/* ---------------------------------------------------------------------------------
 * Batched baseline-JPEG decode (csrc/jpeg.hip, rules in csrc/jpeg_core.h): the first line of the reference's load_video
 * (models/dataset.py:64, `cv2.imread` of one JPEG per frame) for a whole batch, writing the uint8 frames m3t_video_ingest takes.
 * Streams: baseline sequential DCT (SOF0), 8 bits, Huffman, one interleaved scan, gray or YCbCr with luma 1x1 / 2x1 / 2x2 and chroma 1x1,
 * optional restart intervals; all n images H x W.  The bits are libjpeg's: jpeg_idct_islow, "fancy" upsampling over the component's real
 * size (replication where the chroma width is <= 2), jdcolor's 16-bit fixed-point colour.  m3t.jpeg.pack builds the arguments:
 *   stream_d  device bytes: the entropy-coded data of every image, 16-byte aligned, stream_bytes a multiple of 16 (zero padded)
 *   tables    ONE int array, given twice -- tables_h on the host (validated here, before any launch) and tables_d, the same ints on the
 *             device (read by the kernels, which clamp what they index with):
 *               images   [n][16]      flags (bit 0 present, bit 1 restart markers miscounted), components, luma h, luma v, MCUs per segment,
 *                                     first segment, segments, quant table of each component [3], DC table [3], AC table [3]
 *               segments [n_segs][4]  image, byte offset, byte length, restart marker in front (-1 first segment, -2 none found, 0..7);
 *                                     segment k of an image holds its MCUs [k Ri, (k + 1) Ri): exactly ceil(MCUs / Ri) rows per image
 *               slots    [n]          destination frame of each image, in [0, dst_slots)
 *               quant    [n_quant][32]  64 uint16 in natural order
 *               huff     [n_huff][384]  uint16 lut[512] (length << 8 | symbol for codes of <= 9 bits, else 0) | int maxcode[18] (-1: none) |
 *                                     int valoff[18] (symbol index minus first code of the length) | uint8 symbols[256]
 *   dst       device uint8 [dst_slots][H][W][3]; order 0 = b, g, r (what cv2.imread returns), 1 = r, g, b.  Only the n named frames are
 *             written; an image that is not present writes zeros (the reference's `img is None`).
 *   workspace device, 16-byte aligned, at least m3t_jpeg_workspace_bytes(n, H, W) (the component planes); contents undefined afterwards
 *   status    device int [n], zeroed here and OR-ed by the kernels: M3T_JPEG_TRUNC | _CODE | _RST | _EXTRA.  A damaged segment keeps
 *             decoding with zero bits or stops with zero coefficients; nothing outside the image's frame and workspace slot is written.
 * Two launches on `stream` (one wave per segment: entropy decode + IDCT; then upsampling + colour), no host synchronisation.
 * M3T_EINVAL: n <= 0, null or misaligned pointers, any table entry out of range (a segment outside the stream buffer, a slot outside
 * dst, a table index past its count, an unsupported sampling, a segment count that does not match the MCU count), a short workspace. */
#define M3T_JPEG_TRUNC 1     /* a segment ended before its MCUs did */
#define M3T_JPEG_CODE 2      /* no such Huffman code, a coefficient past 63, a DC size above 15 */
#define M3T_JPEG_RST 4       /* a restart marker missing, extra or out of order, or a marker inside a segment */
#define M3T_JPEG_EXTRA 8     /* whole bytes left in a segment after its last MCU */
size_t m3t_jpeg_workspace_bytes(int n, int H, int W);
int m3t_jpeg_decode(const uint8_t* stream_d, long long stream_bytes, const int* tables_h, const int* tables_d, int n, int n_segs,
                    int n_quant, int n_huff, int H, int W, uint8_t* dst, long long dst_slots, int order, uint8_t* workspace,
                    long long workspace_bytes, int* status, void* stream);

/* The same decode with a choice of how launch 1 walks a segment's symbols (the first line of models/dataset.py:64's load_video again:
 * the dataset's files carry no restart markers, a frame is ONE segment, and one lane walking its 45 KB is what bounds m3t_jpeg_decode).
 * Every argument up to `status` as m3t_jpeg_decode; the workspace is the same size.
 *   walk           0: the sequential walk for every segment -- m3t_jpeg_decode, byte for byte.  1: per segment, the PARALLEL walk
 *                  (jpeg_par_kernel, rules in csrc/jpeg_par.h) where par_min_bytes <= segment bytes <= min(par_max_bytes,
 *                  m3t_jpeg_par_max_bytes()) and the segment has at most 4 096 blocks, the sequential walk elsewhere; both kernels are
 *                  launched over all segments and each takes its own.  Any other value: M3T_EINVAL.
 *   sub_bytes      the parallel walk's sub-sequence, a multiple of 16 in [16, 4096]; anything else M3T_EINVAL (whatever `walk` is)
 *   par_min_bytes, par_max_bytes   >= 0, else M3T_EINVAL
 *   walk_stats     NULL, or device int [n_segs][2], 4-byte aligned: (sub-sequences, exchange passes executed) of a segment the parallel walk
 *                  took, 1 <= passes <= sub-sequences; (0, 0) of a segment it did not take
 * The parallel walk: one workgroup per segment (m3t_jpeg_par_lanes lanes), no communication between workgroups, no spinning.  The segment
 * is unstuffed into LDS; lane i walks sub-sequence i (sub_bytes of the unstuffed bytes) leniently from (its first bit, block 0, DC next);
 * then every sub-sequence whose left neighbour's exit state changed is walked again from it, until none changes; a strict walk per
 * sub-sequence records each block's first bit and DC difference; prefix sums give the predictors; one lane per block decodes, eight lanes per
 * block transform.  Bounds of its loops, all from host-validated quantities: staging -- the segment's 16-byte granules; a lenient walk --
 * 8 sub_bytes + 1 steps (each consumes a bit); the exchange -- `sub-sequences` passes (pass r makes the exit state of sub-sequence r true
 * at the latest); closing a block begun in an earlier sub-sequence -- 4 096 steps; the strict walks -- the segment's blocks x 64 symbols,
 * also for the last sub-sequence's lane, which carries on over the zero bits behind a truncated segment.  Every read of the stream lies
 * inside the segment's granules, every read of the unstuffed image is checked against its word count, every write goes to the image's own
 * planes in the workspace.
 * Results: frames AND status words equal those of walk = 0 for every input, valid or damaged, whatever sub_bytes, the lane count or the
 * neighbours in the batch.  Status of a parallel segment: the first strict error in block order raises M3T_JPEG_CODE and leaves every
 * later block zero, as the sequential walk does; TRUNC where the walk consumed bits behind the last byte, EXTRA where 8 or more bits are
 * left; a segment with a marker or a lone FF inside (damage; staging sees it wherever it lies, the sequential reader only if its
 * look-ahead reaches it) has one lane repeat the sequential reader's walk for the status alone, so RST and EXTRA are that reader's.
 * All validation happens before any launch.  M3T_EINVAL: as m3t_jpeg_decode, and the cases above.
 * m3t_jpeg_par_max_bytes: the largest segment the parallel walk takes in this build (49 152: the unstuffed segment, the tables, the
 * per-block records and the exchange states share the 160 KiB of LDS of one CU).
 * m3t_jpeg_par_lanes(lanes): 64, 128 or 256 sets the workgroup size of later calls (process-wide; default 256) and returns it; 0 returns
 * the current one; anything else returns -M3T_EINVAL.  Results do not depend on it. */
int m3t_jpeg_decode_walk(const uint8_t* stream_d, long long stream_bytes, const int* tables_h, const int* tables_d, int n, int n_segs,
                         int n_quant, int n_huff, int H, int W, uint8_t* dst, long long dst_slots, int order, uint8_t* workspace,
                         long long workspace_bytes, int* status, int walk, int sub_bytes, int par_min_bytes, int par_max_bytes,
                         int* walk_stats, void* stream);
int m3t_jpeg_par_max_bytes(void);
int m3t_jpeg_par_lanes(int lanes);

/* The resident frame store's batch step (csrc/frame_store.hip; m3t.jpeg.FrameStore): the scan bytes of every frame of a corpus stay on the
 * device in n_chunks buffers, uploaded once, and ONE launch assembles the byte stream of a batch -- m3t_jpeg_decode_walk's stream_d -- from
 * them.  m3t.jpeg.plan_frames builds the table.
 *   chunks_h, chunk_bytes_h  host long long [n_chunks]: the device address of each chunk (16-byte aligned) and its size in bytes
 *   chunks_d                 the same addresses on the device (read by the kernel)
 *   rows      int [m][4] = chunk, source offset, destination offset, bytes; given twice like the decode's tables: rows_h on the host
 *             (validated here, before the launch) and rows_d, the same ints on the device, 16-byte aligned (read by the kernel)
 *   dst       device, 16-byte aligned, dst_bytes a multiple of 16 in [16, 2^31)
 * For every row dst[dst_off .. dst_off + bytes) = chunk[src_off .. src_off + bytes); every other byte of dst[0 .. dst_bytes) is written as
 * zero by the same kernel: one pass over dst, every 16-byte granule stored exactly once, so the result does not depend on any order.  A flat
 * grid-stride over the destination granules; a lane finds its granule's row by a binary search of the destination offsets (at most
 * ceil(log2(m + 1)) steps) and moves 16 bytes.  No atomics, no communication between workgroups, no spinning.  No byte outside a validated
 * source range is read and none outside dst[0 .. dst_bytes) is written.
 * M3T_EINVAL, before any launch: m < 0 or n_chunks < 0; a null or misaligned pointer (dst always; the tables when m > 0); a chunk index
 * out of range; a source range outside its chunk; a negative offset or length, or one that is no multiple of 16; destinations that are not
 * ascending, overlap, or end past dst_bytes - 16 (the stream's closing 16 zero bytes).  m == 0 zero-fills and returns 0. */
int m3t_jpeg_gather(const long long* chunks_h, const long long* chunk_bytes_h, int n_chunks, const long long* chunks_d, const int* rows_h,
                    const int* rows_d, int m, uint8_t* dst, long long dst_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Window collate (csrc/collate.hip): the rest of the AffWild2 loader's __getitem__ (models/dataset.py:241-343 minus load_video) for a whole
 * batch in ONE launch, from side tracks that live on the device (m3t.dataset.TrackStore uploads them once).
 * The store: flat read-only arrays, one per track kind, the rows of the videos one after the other:
 *     se [se_rows][se_stride], au [au_rows][au_stride], mel [mel_rows][n_mels], va [va_rows][2] float32; expr [expr_rows] long long.
 * videos: device long long [n_videos][12] = se_off, se_n, au_off, au_n, mel_off, mel_n, va_off, va_n, expr_off, expr_n, flags, 0
 *     (row offset and row count per kind; flags bit 0: the video has expression labels, bit 1: its audio is valid, fps >= 15).
 * items:  device int [N][3] = video, start, track_len (1 <= track_len <= window) -- the only per-batch table.
 * With i' = min(i, track_len - 1) (np.pad 'edge' up to `window`, dataset.py:308-319), for item n and i < window:
 *     se_out [N][se_dim][window]       = se[se_off + min(start + i', se_n - 1)][c], c < se_dim <= se_stride   (a feature track shorter than
 *                                        the window pads from its own last row, dataset.py:263-270); au_out the same over au_dim <= au_stride
 *     audio_out [N][window][width n_mels] = m3t_stack_context_batch's: r = (start + i') step + k; r < mel_n ? mel[mel_off + r][c] : 0;
 *                                        an audio-invalid video gives zeros (dataset.py:276-278)
 *     valence_out, arousal_out [N][window] = va[va_off + start + i'][0 | 1], as stored
 *     expr_out [N][window] (long long), expr_valid_out [N][window] (bytes 0 / 1): e = expr[expr_off + start + i']: valid = e >= 0,
 *                                        out = min(max(e, 0), 6); a video without expression labels: 0 and 0   (dataset.py:285-291)
 * Every output is optional (NULL; valence with arousal, expr with expr_valid) and every value is a copy: bit-exact, no atomics, no order.
 * Indices are clamped on the device: start below 0 counts as 0, track_len is clamped into [1, window], a label row past the end reads
 * the last row, a table entry that does not fit its array counts as an empty track (zeros), a video index outside [0, n_videos) writes
 * zeros: no byte outside the arrays is read whatever the tables hold.  The host validates first (m3t.dataset.plan).
 * Rows are read 16 bytes a lane where the stride is a multiple of 4 floats and the array 16-byte aligned, else by the float.
 * M3T_EINVAL: null / misaligned pointers of a requested output's inputs (floats and ints 4 bytes, long long 8), dim > stride,
 * non-positive sizes; N == 0 or window == 0 returns 0. */
int m3t_window_collate(const float* se, long long se_rows, int se_stride, int se_dim,
                       const float* au, long long au_rows, int au_stride, int au_dim,
                       const float* mel, long long mel_rows, int n_mels, int step, int width,
                       const float* va, long long va_rows, const long long* expr, long long expr_rows,
                       const long long* videos, int n_videos, const int* items, int N, int window,
                       float* se_out, float* au_out, float* audio_out, float* valence_out, float* arousal_out,
                       long long* expr_out, unsigned char* expr_valid_out, void* stream);


/* ---------------------------------------------------------------------------------
 * Attention decoder of --fusion_type att_dec (csrc/attdec.hip).  Replaces the decoder loop of AttEncDec.forward with
 * Decoder.forward and Attention.forward inside it (reference models/rnn.py:93-136, 145-165) and its autograd.
 * H = hidden width (H % 64 == 0, H <= 512), E = 2 (input and output width), B >= 1 clips, T >= 1 encoder frames (<= 8192),
 * L >= 1 output frames (T, or the target's length with teacher forcing), S = L - 1 decoder steps.
 * Step t = 1 .. L-1, with h_0 = h0, y_in = y0 (or 0) at t = 1:
 *   a = W_ah h_{t-1}, s_tau = v . relu(P[tau] + a), alpha = softmax_tau(s), c = sum_tau alpha_tau enc[tau],
 *   h_t = GRUCell([y_in, c], h_{t-1}), y_t = W_o [h_t, c] + b_o -> out[:, t];  y_in of step t+1 = tf[t] ? trg[:, t] : y_t.
 * P = enc W_ae^T + b_a is the caller's (m3t_sgemm), W_a = [W_ah | W_ae] is the attn weight [H][2H]. */
typedef struct {
    const float* enc;     /* [B][T][H] encoder outputs                                              */
    const float* P;       /* [B][T][H] enc W_ae^T + b_a                                             */
    const float* h0;      /* [B][H]                                                                 */
    const float* w_a;     /* [H][2H] attention weight (W_ah = columns [0, H))                       */
    const float* v;       /* [H]                                                                    */
    const float* w_ih;    /* [3H][2 + H], gates r | z | n as nn.GRU                                 */
    const float* w_hh;    /* [3H][H]                                                                */
    const float* b_ih;    /* [3H]                                                                   */
    const float* b_hh;    /* [3H]                                                                   */
    const float* w_o;     /* [2][2H]                                                                */
    const float* b_o;     /* [2]                                                                    */
    const float* y0;      /* [B][2] input of step 1, NULL = zeros                                   */
    const float* trg;     /* [B][L][2] teacher target, or NULL                                      */
    const int* tf;        /* [L] device flags: tf[t] != 0 feeds trg[:, t] to step t+1; needs trg     */
    float* out;           /* [B][L][2] (out[:, 0] = 0)                                              */
    float* h_last;        /* [B][H] h_{L-1}                                                         */
    float* G;             /* [B][4H] scratch: [W_hh h + b_hh | W_ah h]                               */
    /* per-step records: save != 0 -> S records each (backward), save == 0 -> scratch (alpha, gates: one record; x, hs: two) */
    float* alpha;         /* [S][B][T]                                                              */
    float* a_save;        /* [S][B][H] a of each step (save only)                                    */
    float* x;             /* [S][B][2 + H] the step's input [y_in, c]                                */
    float* gates;         /* [S][B][4H] r, z, n, W_hn h + b_hn                                       */
    float* hs;            /* [L][B][H] h_0 .. h_{L-1}                                                */
    /* backward (m3t_attdec_bwd / m3t_attdec_post) */
    const float* dout;    /* [B][L][2]                                                              */
    const float* dh_last; /* [B][H] gradient of h_last, or NULL                                     */
    float* dgi;           /* [S][B][3H] gradient of W_ih x + b_ih                                   */
    float* dgh;           /* [S][B][3H] gradient of W_hh h + b_hh                                   */
    float* dc;            /* [S][B][H] gradient of the context                                      */
    float* da;            /* [S][B][H] gradient of a                                                */
    float* dy;            /* [S][B][2] total gradient of y_t (output + feedback)                    */
    float* dP;            /* [B][T][H] gradient of P (zeroed by the call, then accumulated per step) */
    float* dv_acc;        /* [B][H] per-clip gradient of v (zeroed by the call)                      */
    float* dh;            /* [B][H] -> gradient of h0                                                */
    float* dy0;           /* [B][2] gradient of y0, or NULL                                          */
    float* w_iht;         /* [2 + H][3H] scratch (W_ih^T)                                            */
    float* wt;            /* [H][4H] scratch ([W_hh^T | W_ah^T])                                     */
    float* dyin;          /* [B][2] scratch                                                         */
    float* dhz;           /* [B][H] scratch                                                         */
    int B, T, L, H, save;
} m3t_attdec_args;
/* forward loop: a prologue (h_0 -> x, G) and three launches per step (attention, GRU cell, [W_hh; W_ah] h_t with the output layer);
 * no host synchronisation.  save = 0 (inference) keeps only scratch records. */
int m3t_attdec_fwd(const m3t_attdec_args* args, void* stream);
/* backward loop over the records of a save != 0 forward (L >= 2): four launches per step (cell backward with the output and feedback
 * gradient, context gradient W_ih[:, 2:]^T dgi + W_o[:, H:]^T dy, attention backward with dP += .. in place, dh_{t-1}).  The
 * feedback W_ih[:, :2]^T dgi_{t+1} reaches y_t only where step t+1 was fed y_t (not teacher-forced).  The caller finishes with
 * m3t_sgemm / m3t_colsum over the records (dW_ih = dgi^T x, dW_hh = dgh^T h_{t-1}, dW_ah = da^T h_{t-1}, dW_ae = dP^T enc,
 * d enc = dP W_ae + m3t_attdec_post) */
int m3t_attdec_bwd(const m3t_attdec_args* args, void* stream);
/* after m3t_attdec_bwd: dw_o [2][2H], db_o [2], dv [H] (all three or none), and d_enc [B][T][H] += sum_t alpha_t^T dc_t per clip
 * (d_enc NULL: skipped).  Fixed-order sums. */
int m3t_attdec_post(const m3t_attdec_args* args, float* dw_o, float* db_o, float* dv, float* d_enc, void* stream);
/* Attention.forward alone (reference models/rnn.py:93-111): alpha [B][T] from P, a ([B] rows of lda) and v; c [B][H] (optional) the
 * context.  Backward from d alpha: dP += .., da = .., dv_acc += .. (per clip; the caller zeroes dP and dv_acc). */
int m3t_attdec_attn_fwd(const float* enc, const float* P, const float* a, int lda, const float* v, float* alpha, float* c,
                        int B, int T, int H, void* stream);
int m3t_attdec_attn_bwd(const float* enc, const float* P, const float* a, const float* v, const float* alpha,
                        const float* dalpha, float* dP, float* da, float* dv_acc, int B, int T, int H, void* stream);
/* the sum of a bidirectional GRU's two halves, y [rows][H] = x[:, :H] + x[:, H:] (reference models/rnn.py:153), and its gradient
 * dx [rows][2H] = [dy, dy] */
int m3t_attdec_sum_halves(const float* x, float* y, size_t rows, int H, void* stream);
int m3t_attdec_dup_halves(const float* dy, float* dx, size_t rows, int H, void* stream);

/* ---------------------------------------------------------------------------------
 * The 3-D DenseNet of --backbone densenet (csrc/dense.hip; reference models/densenet.py:5-93, models/backbone.py:375-423), on channels-last
 * rows [N T H W][C] with a leading dimension: a dense block is one buffer its layers write their new columns into.  fp32 arithmetic, fixed
 * reduction orders, no atomics: bit-identical run to run.
 *
 * Batch statistics of columns [0, C) of x (ld): mean and the biased variance, fp64 per-chunk partials.  Replaces the statistics pass of
 * nn.BatchNorm3d in train mode (densenet.py:8,11,34,62); a column's statistics serve every BatchNorm that reads it.  ws: 8-B aligned,
 * m3t_dense_stats_ws_bytes(rows, C) bytes. */
size_t m3t_dense_stats_ws_bytes(size_t rows, int C);
int m3t_dense_col_stats(const float* x, size_t rows, int ld, int C, float* mean, float* var, void* ws, size_t ws_bytes, void* stream);
/* y (ldy) = relu(gamma (x - mean) / sqrt(var + eps) + beta) over [rows][C] of x (ldx): nn.BatchNorm3d + nn.ReLU (densenet.py:8-9,11-12).
 * C % 4 == 0, ldx % 4 == 0, ldy % 4 == 0, x and y 16-B aligned.  ReLU keeps NaN. */
int m3t_dense_bn_relu_fwd(const float* x, int ldx, size_t rows, int C, const float* mean, const float* var, const float* gamma,
                          const float* beta, float eps, float* y, int ldy, void* stream);
/* running_mean / running_var <- (1 - momentum) running + momentum (mean, var rows / (rows - 1)): the buffer update of a train-mode
 * nn.BatchNorm3d from given batch statistics (rows >= 2). */
int m3t_dense_bn_running(const float* mean, const float* var, size_t rows, int C, float* run_mean, float* run_var, float momentum, void* stream);
/* Backward of m3t_dense_bn_relu_fwd: g = dy where the ReLU's input is not <= 0; dbeta = sum g, dgamma = sum g xhat (either may be NULL);
 * dx (lddx; NULL: skipped) = (or += with accumulate) gamma / sqrt(var + eps) (g - mean g - xhat mean(g xhat)) with training, the same
 * without the two means for running statistics.  ws: 8-B aligned, m3t_dense_stats_ws_bytes(rows, C) + 8 C bytes. */
int m3t_dense_bn_relu_bwd(const float* dy, int ldy, const float* x, int ldx, size_t rows, int C, const float* mean, const float* var,
                          const float* gamma, const float* beta, float eps, int training, float* dx, int lddx, int accumulate,
                          float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream);
/* Transition (densenet.py:32-39): y [P (H/2) (W/2)][C] = AvgPool3d((1, 2, 2)) of relu(bn(x)) over frames x [P H W][C] (ldx), floor mode.
 * The transition's 1x1x1 convolution, which commutes with the pooling, then runs on a quarter of the rows.  The spread is the pooling's
 * backward: dfull [P H W][C] = dy / 4 inside the pooled area, 0 on a dropped last row / column. */
int m3t_dense_pool_fwd(const float* x, int ldx, size_t P, int H, int W, int C, const float* mean, const float* var, const float* gamma,
                       const float* beta, float eps, float* y, void* stream);
int m3t_dense_pool_spread(const float* dy, size_t P, int H, int W, int C, float* dfull, void* stream);
/* norm5 + relu5 + aggregation (densenet.py:61-63,79-91) over frames x [P HW][C] (ldx): mode 0 (agg 'ap', AdaptiveAvgPool2d(1)):
 * y [P][C] = the mean over the frame; mode 1 (agg 'fc'): y [P][C HW] = relu(bn(x)) in (c, h, w) order, the input of DenseNet52_3D.fc.
 * The spread is the backward of the aggregation: dfull [P HW][C]. */
int m3t_dense_mean_fwd(const float* x, int ldx, size_t P, int HW, int C, const float* mean, const float* var, const float* gamma,
                       const float* beta, float eps, int mode, float* y, void* stream);
int m3t_dense_mean_spread(const float* dy, size_t P, int HW, int C, int mode, float* dfull, void* stream);
/* Conv3d(Ci, Co, 3, stride 1, padding 1, bias=False) on channels-last rows (densenet.py:13-14): y [N T H W][Co] (ldy; or += with accumulate)
 * from x (ldx) and w [27][Ci][Co] (tap = (kt, kh, kw) row-major).  With the flipped, transposed weights w'[26 - tap][co][ci] the same call is
 * the layer's data gradient.  Tiles of 128 rows x 32 output channels: Ci % 32 == 0, Co % 32 == 0, ld % 4 == 0, 16-B aligned operands. */
int m3t_dense_conv333(const float* x, int ldx, int N, int T, int H, int W, int Ci, const float* w, float* y, int ldy, int Co,
                      int accumulate, void* stream);
/* Its weight gradient dw [27][Ci][Co] = sum over rows of x[row + tap offset] (ldx) dy[row] (ldy): fixed row chunks, summed in order.
 * Ci % 128 == 0, Co % 32 == 0, ld % 4 == 0, 16-B aligned operands; ws: m3t_dense_wgrad_ws_bytes(N T H W, Ci, Co) bytes. */
size_t m3t_dense_wgrad_ws_bytes(size_t rows, int Ci, int Co);
int m3t_dense_conv333_wgrad(const float* x, int ldx, const float* dy, int ldy, int N, int T, int H, int W, int Ci, int Co, float* dw,
                            void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Loss end of the two pre-training tasks (csrc/cls_loss.hip): VoxCeleb2_1k (models/vox2_model.py) and AudioSet
 * (models/audioset_model.py).  Everything fp32 in memory, labels int64; B, T, C >= 1 and no alignment or divisibility
 * requirement on C; anything else returns M3T_EINVAL.  Row sums and the loss are accumulated in fp64 in a fixed order, no
 * atomics: the same bits run to run.
 *
 * Temporal pooling of per-frame logits z [B,T,C] into pooled [B,C]: mode 0 = maximum over T (audioset_model.py:34-36,
 * `torch.max(self.audio(x), dim=1)[0]`), with arg [B,C] = the frame of the FIRST maximum and NaN above every number; mode 1 = mean
 * over T (the `.mean(dim=1)` of the 'fc' back-end, models/backbone.py:143-145; arg unused, may be NULL).  The backward writes
 * all of dz [B,T,C] in one pass: dpooled[b,c] at t = arg[b,c] and 0 elsewhere, or dpooled[b,c] / T at every t. */
int m3t_tpool_fwd(const float* z, int B, int T, int C, int mode, float* pooled, int* arg, void* stream);
int m3t_tpool_bwd(const float* dpooled, const int* arg, int B, int T, int C, int mode, float* dz, void* stream);
/* Loss, top-1 statistic and gradient from per-clip logits [B,C], one workgroup per clip plus one small launch for the mean over clips
 * (per-clip partials added in clip order).
 *   kind 0: F.cross_entropy(logits, labels) with labels int64 [B] (vox2_model.py:58-67): loss = mean_b (logsumexp(x_b) - x_b[y_b]),
 *           correct[b] = (argmax_c x_b == y_b), dlogits = (softmax - onehot) / B.  A label outside [0, C) indexes nothing: that clip's
 *           loss term and gradient are NaN.
 *   kind 1: F.binary_cross_entropy_with_logits(logits, targets) with targets float [B,C] (audioset_model.py:38-49): mean over all B C
 *           elements of max(x, 0) - x y + log1p(exp(-|x|)), correct[b] = targets[b, argmax_c x_b], dlogits = (sigmoid(x) - y) / (B C).
 * The argmax is the first maximum.  out_scalars[2] = {loss, n_correct}; correct [B] fp32; dlogits [B,C] fully written.
 * ws: m3t_cls_loss_ws_bytes(B) bytes, 8-B aligned. */
size_t m3t_cls_loss_ws_bytes(int B);
int m3t_cls_loss(const float* logits, int B, int C, int kind, const void* target, float* out_scalars, float* correct,
                 float* dlogits, void* ws, size_t ws_bytes, void* stream);
/* The training path (vox2_model.py:61-67, audioset_model.py:41-49: forward, loss, argmax, accuracy): pooling, loss, statistics and
 * dz [B,T,C] = dL/dz from the per-frame logits, in the same two launches.  One workgroup per clip pools its clip (pooled and, for the
 * maximum, arg are outputs), reduces the row and writes its rows of dz: neither dL/dpooled nor a zero-filled buffer exists in memory. */
int m3t_tpool_cls_loss(const float* z, int B, int T, int C, int mode, int kind, const void* target, float* pooled, int* arg,
                       float* out_scalars, float* correct, float* dz, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------------------------
 * Multi-label evaluation epoch on the device (csrc/cls_eval.hip, m3t/cls_evaluate.py): mean average precision, mean ROC-AUC and d' of
 * the AudioSet stage.  The reference has no counterpart (its validation_end reports val_loss and a top-1 val_acc, audioset_model.py:
 * 89-104); the three launches replace a read-back of the [M, C] scores followed by scikit-learn's average_precision_score and
 * roc_auc_score per class on the host.  Resident state, owned by the caller and zero-filled before the first append: col_scores
 * [C][M] fp32 and col_labels [C][M] uint8 (CLASS-major: a class's column is contiguous), seen [M] uint8, counters [2] uint32.
 * 1 <= M <= M3T_CLS_EVAL_MAX_ROWS, C >= 1, no alignment or divisibility requirement; anything else returns M3T_EINVAL.  No float
 * atomics and every float64 sum in a fixed order: the same bits run to run.
 *
 * m3t_cls_eval_append, one launch per batch: scores [B,C] (the pooled per-clip logits of m3t_tpool_cls_loss) and labels [B,C] fp32
 * go to row rows[b] of every class column, transposed through an LDS tile (labels as uint8: 1 where the label is 1.0); seen[rows[b]] = 1;
 * counters[0] += the scores that are NaN or +-inf, counters[1] += the labels that are neither 0.0 nor 1.0.  rows: int32 [B], each in
 * [0, M) (validated by the caller; a row outside is not written).  Writing a row twice with equal values is legal. */
#define M3T_CLS_EVAL_LDS_ROWS 16384     /* the longest column the rank kernel sorts wholly in LDS (128 KiB of items + 16 KiB of scans) */
#define M3T_CLS_EVAL_MAX_ROWS 262144    /* capacity: the longest column at all */
int m3t_cls_eval_append(const float* scores, const float* labels, const int* rows, int B, int C, long long M, float* col_scores,
                        unsigned char* col_labels, unsigned char* seen, unsigned int* counters, void* stream);
/* m3t_cls_eval_rank, one launch for all classes (one workgroup per class): the column is ordered descending by its float32 VALUES
 * (-0.0 ties with +0.0, denormals are kept apart) and scores that compare equal form one threshold group.  With TP, FP the counts after
 * a group and dTP, dFP its own, P and N the column's positives and negatives:
 *   AP  = (1 / P) sum_groups dTP TP / (TP + FP)            float64, one correctly rounded division per group, fixed order
 *   AUC = sum_groups dFP (2 TP_before + dTP) / (2 P N)     the numerator a 64-bit integer (exact), one float64 division
 * -- scikit-learn's average_precision_score and roc_auc_score with their handling of ties.  per_class [C][4] float64 = AP, AUC, P, N;
 * AP is NaN without a positive, AUC without a positive or without a negative.  lds_rows: the longest column sorted wholly in LDS, rounded
 * down to a power of two (0 or above M3T_CLS_EVAL_LDS_ROWS: M3T_CLS_EVAL_LDS_ROWS); a column whose power-of-two padding is longer is
 * sorted in LDS-sized chunks with the wide strides in ws, m3t_cls_eval_rank_ws_bytes(C, M, lds_rows) bytes (0: not needed), 8-B aligned. */
size_t m3t_cls_eval_rank_ws_bytes(int C, long long M, int lds_rows);
int m3t_cls_eval_rank(const float* col_scores, const unsigned char* col_labels, int C, long long M, int lds_rows, void* ws,
                      size_t ws_bytes, double* per_class, void* stream);
/* m3t_cls_eval_reduce, one workgroup: out8 float64 = mAP, mAUC (means over the scored classes in class order; NaN when no class is
 * scored or a counter is above zero), classes scored for AP, for AUC, rows of `seen` still 0, counters[0], counters[1], 0.  out8 and
 * per_class, kept in one buffer, are the epoch's one read-back. */
int m3t_cls_eval_reduce(const double* per_class, int C, const unsigned char* seen, long long M, const unsigned int* counters,
                        double* out8, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* M3T_HIP_H */
