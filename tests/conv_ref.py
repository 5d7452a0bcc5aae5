"""Float64 reference, two fp32 yardsticks and the error bound for the 3-D convolutions of the visual front-ends: ops.conv3d, ops.conv2d and
ops.conv3d_cl of m3t/ops.py (_Conv3dGemmWgrad, _Conv3dCL) on sgemm_x6_kernel with C3 = 1 / 2 / 3 of csrc/gemm_x6.hip (m3t_conv3d_taps_launch,
m3t_conv3d_taps4_launch, m3t_conv3d_wgrad_launch), the entry points m3t_conv3d_fwd_taps, _fwd_taps4, _taps, _taps_pre, _wgrad_taps of
csrc/gemm.hip, and the patch-matrix GEMMs (m3t_im2col3d x W^T, dy^T P).  tests/test_conv_ref_host.py checks this file on the CPU;
tests/test_gpu_conv_fp64.py holds the kernels to it.

Layout: every compared tensor is in torch's layout -- y [N,Co,T',H',W'], dx [N,Ci,T,H,W], dw [Co,Ci,kt,kh,kw], db [Co]; the walks' own
matrices are channels-last rows [(n, t, h, w)][c].

Reference    torch.conv3d and its autograd in float64 on the CPU, on the fp32 inputs, for an upstream gradient `ct` drawn with the case.
             Beside it two plain numpy restatements the host file holds to that autograd within 1e-13: `conv3d_taps_ref` (the tap rule:
             source row = s out + tap - pad, zero outside) and `dgrad_classes_ref` (the parity-class rule of ops._dgrad_plan: input position
             s h' + c receives only the taps s j + r, r = (c + p) mod s, from source row h' + (c + p - r) / s - j).
Yardstick A  (E32)   the same composition in torch float32 on the CPU, one thread.
Yardstick B  (E_emu) `emulate`: a numpy float32 restatement, written from the kernel text, of the products of the path a case reaches
             (`route` restates the dispatch of m3t/ops.py):
  * fp16x3 walks   two fp16 terms of each operand under its slot's power-of-two scale (the slots hold max |x|, max |w|, max |dy|), the three
                   products lo hi, hi lo, hi hi per 16-deep MFMA, k ordered tap-major then channel, times the two inverse scales; every
                   split-K slab its own accumulator, the slabs added in slab order (splitk_reduce*_kernel); bias in fp32 behind the scales
                   (the direct epilogue) or behind the slab sum (the reduce).
  * first layers   m3t_conv3d_fwd_taps4: channels padded to 4, the kernel's width to 8 taps (zero weights, the row not read past kw),
                   K = kt kh 32, k = ((kt, kh), pixel, channel).
  * weight grad    m3t_conv3d_wgrad_taps: dW^T[(tap, ci)][co], the reduction over dy's rows in grid order, padding rows zeros, a ragged
                   last 16-deep block; a first layer reads four-channel rows (cw = 4, the natural taps).  Reading images (M3T_CONV_IMAGES)
                   or splitting in the loop are the same arithmetic (the GPU file runs both: S2).
  * data gradient  one stride-1 walk per parity class over dy's rows with the sub-kernel w[..., r::s], flipped taps
                   (m3t_conv3d_taps_pre; m3t_conv3d_taps splitting in its loop -- S1 -- is the same arithmetic); in the x6 mode the six
                   bf16 products of m3t_conv3d_taps, smallest first.
  * patch matrix   (m3t_im2col3d: columns (ci, kt, kh, kw), zero-padded) through gru_ref.gemm_route / gru_ref.product: forward
                   pat @ W^T, dW = dy^T P (Co % 128 == 0 and Kc % 64 == 0), the transposed and padded dW^T = P_pad^T dy (Co % 64), the
                   Kp = ceil4 form behind a stock forward.
  * bias gradient  fp32 numpy column sums.
  * stock passes   (torch / MIOpen: counted in ops.STOCK_FALLBACKS) are compared all the same, against the fp32 model of the same product.
  Not modelled: which wave owns which k, the two-level fold of very many slabs, split-K inside the patch-matrix GEMMs, the order of the
  column sums -- other summation orders of the same length, which the factor BOUND covers.

Metric  rel_err(got, ref) = max |got - ref| / max |ref| per tensor, never max(1, .); the reference maximum must be finite and non-zero.
Bound   rel_err(gpu) <= BOUND max(E32, E_emu, 2^-24), BOUND = fuse_loss_ref.BOUND = 4.0.  Not fitted to GPU output.  A region that is
        identically zero in the reference (`zero_mask`: the input positions of a parity class without a tap -- W5, the 1 x 1 stride-2
        shortcut -- and the rows behind the last window of P3) must be identically zero.

Statistics  normal | small (ct x 1e-6: gradient-like magnitudes, where max(1, .) made the old bar absolute) | decades (input channel
        magnitudes spread over four decades).  `limits` derives from the emulation alone which tensors of a `decades` case exceed
        BOUND max(E32, 2^-24) (the normwise limit of fp16x3); those are held to BOUND E_emu and must EXCEED the fp32 bar.
        (At four decades no tensor of a convolution does: an element 2^-13 below its operand's maximum still keeps both fp16 terms
        normal -- tests/test_fp16x3_model.py -- and every compared tensor is measured against its own maximum.  The rule stays, so that a
        change of the scaling shows up.)
"""
import collections
import functools

import numpy as np
import torch

from fuse_loss_ref import BOUND
from gru_ref import gemm_route, product as gemm_product, rel_err
from test_fp16x3_model import f16_scale, split_f16, split_bf16, mfma_acc

FLOOR = 2.0 ** -24
_F = np.float32
WS_MIN = 64 << 20            # ops._WS_MIN: the smallest workspace a walk is handed (the plans below are stated for it)
SWITCHES = ("CONV3D_IMPLICIT", "CONV3D_PRESPLIT", "WGRAD_IMAGES")

Case = collections.namedtuple("Case", "id op geo off prec stats fwd dx dw edge")
# op:    conv3d | conv2d (a unit time axis: x [N,C,H,W], a Conv2d weight) | conv3d_cl | conv3d_cl2 (conv3d_cl with a Conv2d weight)
# geo:   (Ci, Co, k, stride, pad, N, T, H, W)
# off:   the switches of m3t/ops.py turned off for the case (SWITCHES);  prec: f16x3 (default) | x6 (ops.precision("x6"))
# fwd:   walk | walk4 (the first layers' four-channel walk) | patch | torch           (the key of ops.CONV3D_CALLS: walk4 counts as walk)
# dx:    walk (pre-split) | walk_loop (split in the loop) | walk_x6 | stock | "" (not asked: x does not require a gradient)
# dw:    walk | dyTP | PTdy | ceil4


def _table():
    W2 = (64, 128, (3, 3, 3), (1, 1, 1), (1, 1, 1), 2, 4, 8, 8)
    W3 = (64, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1), 3, 1, 15, 15)
    F1 = (3, 64, (3, 3, 3), (1, 2, 2), (1, 0, 0), 2, 8, 17, 17)
    P2 = (16, 128, (1, 2, 2), (1, 1, 1), (0, 0, 0), 2, 1, 9, 9)
    n, f = "normal", "f16x3"
    return (
        Case("W1", "conv2d", (32, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 3, 1, 5, 5), (), f, n, "walk", "stock", "walk",
             "one ragged row tile (75 rows); K = 288: no slabs, the direct planes epilogue with bias; dx has no walk (C_in % 64): stock"),
        Case("W2", "conv3d", W2, (), f, n, "walk", "walk", "walk",
             "padding on every axis; K = 1728: forward slabs; dx by m3t_conv3d_taps_pre (K = 3456); weight gradient on images, row split"),
        Case("W3", "conv2d", W3, (), f, n, "walk", "walk", "walk", "stride 2 on an odd grid: four parity classes of unequal size, 192 rows"),
        Case("W4", "conv3d", (64, 128, (3, 3, 3), (2, 2, 2), (1, 1, 1), 2, 5, 9, 7), (), f, n, "walk", "walk", "walk",
             "eight parity classes, ragged everywhere"),
        Case("W5", "conv2d", (64, 128, (1, 1, 1), (1, 2, 2), (0, 0, 0), 8, 1, 16, 16), (), f, n, "walk", "walk", "walk",
             "the 1 x 1 stride-2 shortcut: three of four classes have no tap -- exact zeros in dx; K = 64"),
        Case("W6", "conv3d", (64, 64, (3, 1, 1), (2, 1, 1), (1, 0, 0), 4, 8, 4, 4), (), f, n, "walk", "walk", "walk", "stride on the time axis only"),
        Case("W7", "conv2d", (96, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 8, 1, 8, 8), (), f, n, "walk", "stock", "walk",
             "864 weight-gradient rows padded to 896; a 128-column tile spans three taps"),
        Case("W8", "conv2d", (32, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 32, 1, 14, 14), (), f, n, "walk", "stock", "walk",
             "W % 4 != 0: the weight gradient's row counter carries inside a thread's four rows"),
        Case("F1", "conv3d", F1, (), f, n, "walk4", "", "walk", "fwd_taps4, kw = 3 of 8; weight gradient on fp32 four-channel rows"),
        Case("F2", "conv3d", (3, 64, (5, 7, 7), (1, 2, 2), (2, 3, 3), 1, 8, 32, 32), (), f, n, "walk4", "", "walk",
             "fwd_taps4, seven taps of eight, padding on every axis"),
        Case("F3", "conv3d", (1, 128, (1, 8, 8), (1, 1, 1), (0, 4, 4), 2, 4, 15, 15), (), f, n, "walk4", "", "walk",
             "one channel, all eight taps, C_out = 128"),
        Case("P1", "conv3d", (8, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), 2, 4, 4, 4), (), f, n, "patch", "stock", "PTdy",
             "patch matrix (C_in % 32 != 0, not a first layer): 128 rows, Kc = 216 -> 256 padded; the transposed weight-gradient form"),
        Case("P2", "conv3d", P2, (), f, n, "patch", "stock", "dyTP", "patch matrix; dW = dy^T P with Kc = 64"),
        Case("P3", "conv3d", (8, 24, (3, 2, 3), (2, 1, 2), (0, 1, 1), 3, 8, 7, 9), (), f, n, "torch", "stock", "ceil4",
             "stock forward, HIP weight gradient through the Kp = ceil4 form"),
        Case("P4", "conv3d", W2, ("CONV3D_IMPLICIT",), f, n, "patch", "walk", "dyTP", "the patch-matrix GEMMs on an interior layer"),
        Case("X1", "conv3d", W2, (), "x6", n, "patch", "walk_x6", "dyTP", "six bf16 products: forward, m3t_conv3d_taps (not pre-split), weight gradient"),
        Case("X2", "conv3d", P2, (), "x6", n, "patch", "stock", "dyTP", "six bf16 products on the patch matrix"),
        Case("S1", "conv3d", W2, ("CONV3D_PRESPLIT",), f, n, "walk", "walk_loop", "walk", "m3t_conv3d_taps splitting in its loop (fp16x3)"),
        Case("S2", "conv3d", W2, ("WGRAD_IMAGES",), f, n, "walk", "walk", "walk", "the weight gradient splitting fp32 rows in its loop"),
        Case("T1", "conv3d", (128, 256, (3, 3, 3), (1, 1, 1), (1, 1, 1), 2, 4, 17, 16), (), f, n, "walk", "walk", "walk",
             "the smallest row count (17 row tiles) at which m3t_conv3d_taps_launch takes the 128 x 128 tile with slabs"),
        Case("C1", "conv3d_cl", W2, (), f, n, "walk", "walk", "walk", "a CLTensor without a slot, stride 1"),
        Case("C2", "conv3d_cl", W3, (), f, n, "walk", "walk", "walk", "strided dx on channels-last rows"),
        Case("C3", "conv3d_cl", F1, (), f, n, "walk4", "", "walk", "a first layer from video planes"),
        Case("C4", "conv3d_cl2", (64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), 3, 1, 5, 5), (), f, n, "walk", "walk", "walk",
             "a Conv2d weight: a unit time tap as in models/vggface.py"),
        Case("D1", "conv3d", W2, (), f, "decades", "walk", "walk", "walk", "W2, input channels over four decades"),
        Case("D2", "conv3d_cl", W3, (), f, "decades", "walk", "walk", "walk", "C2, input channels over four decades"),
        Case("M1", "conv3d", W2, (), f, "small", "walk", "walk", "walk", "W2 with ct x 1e-6: gradient-like magnitudes"),
    )


CASES = _table()          # ONE table, imported by both test files; every case is admitted
BY_ID = {c.id: c for c in CASES}
MAX_FLOP = 2 * 2176 * 256 * 27 * 128          # T1's forward: no case may exceed it


def case_id(c):
    return c.id


def grids(c):
    """-> (output grid (T', H', W'), output rows, input rows, taps)"""
    Ci, Co, k, st, pd, N, T, H, W = c.geo
    og = tuple((d + 2 * p - kk) // s + 1 for d, p, kk, s in zip((T, H, W), pd, k, st))
    return og, N * og[0] * og[1] * og[2], N * T * H * W, k[0] * k[1] * k[2]


def flops(c):
    Ci, Co = c.geo[:2]
    _, rows, _, taps = grids(c)
    return 2 * rows * Co * taps * Ci


# ================================================================================================= the dispatch of m3t/ops.py, restated
def channel_width(c):
    """cw of _conv3d_plan: the channel width of the channels-last input a walk reads (0: no walk)"""
    Ci, k = c.geo[0], c.geo[2]
    return Ci if Ci % 32 == 0 else (4 if (Ci <= 4 and k[2] <= 8) else 0)


def route(c):
    """(fwd, dx, dw) as _Conv3dGemmWgrad / _Conv3dCL pick them from shape, precision and switches"""
    Ci, Co, k, st, pd, N, T, H, W = c.geo
    _, rows, srows, taps = grids(c)
    f16, cw = c.prec == "f16x3", channel_width(c)
    on = lambda s: s not in c.off
    asked = c.dx != ""
    if c.op.startswith("conv3d_cl"):
        assert f16 and not c.off and Co % 64 == 0 and cw
        return ("walk" if cw == Ci else "walk4"), ("walk" if asked else ""), "walk"
    walk = on("CONV3D_IMPLICIT") and f16 and cw
    if Co % 64 != 0 or (rows % 128 != 0 and not walk):
        fwd = "torch"
    else:
        fwd = ("walk" if cw == Ci else "walk4") if walk else "patch"
    dx = ""
    if asked:
        dx = "stock"
        if fwd != "torch" and Co % 32 == 0 and Ci % 64 == 0:
            if tuple(st) == (1, 1, 1) and (srows % 128 == 0 or f16):
                dx = ("walk" if on("CONV3D_PRESPLIT") else "walk_loop") if f16 else "walk_x6"
            elif tuple(st) != (1, 1, 1) and on("CONV3D_PRESPLIT") and f16:
                dx = "walk"
    if fwd in ("walk", "walk4"):
        dw = "walk"
    else:
        Kc = Ci * taps
        dw = "dyTP" if (Co % 128 == 0 and Kc % 64 == 0) else ("PTdy" if Co % 64 == 0 else "ceil4")
    return fwd, dx, dw


def stock_calls(c):
    """by how much ops.STOCK_FALLBACKS moves over one forward + backward of the case"""
    return int(c.fwd == "torch") + int(c.dx == "stock")


def _cdiv(a, b):
    return (a + b - 1) // b


def taps_split(rows, Cd, K, ws_bytes=WS_MIN):
    """taps_split of csrc/gemm.hip -> (splits, kchunk, cap binding?)"""
    tiles = _cdiv(rows, 128) * _cdiv(Cd, 128)
    if tiles >= 512:
        return 1, K, False
    sp = _cdiv(640, tiles)
    cap = ws_bytes // (rows * Cd * 4)
    bound = sp > cap
    sp = min(sp, cap, K // 256)
    if sp < 2:
        return 1, K, bound
    kchunk = _cdiv(_cdiv(K, sp), 32) * 32
    return _cdiv(K, kchunk), kchunk, bound


def walk_plan(rows, Cd, K, ws_bytes=WS_MIN):
    """m3t_conv3d_taps_launch / _taps4_launch -> (splits, kchunk, narrow: the 128 x 64 tile)"""
    splits, kchunk, _ = taps_split(rows, Cd, K, ws_bytes)
    narrow = Cd % 128 != 0 or (Cd // 128) * _cdiv(rows, 128) * splits <= 384
    return splits, kchunk, narrow


def wgrad_plan(rows, Kc, Co, ws_bytes=None):
    """m3t_conv3d_wgrad_taps behind the workspace _backward5 asks for (want slabs, at most 512 MiB) -> (splits, kchunk, narrow)"""
    Mp = _cdiv(Kc, 128) * 128
    tiles = (Mp // 128) * _cdiv(Co, 128)
    if ws_bytes is None:
        want = max(1, min(_cdiv(1536, tiles), rows // 256))
        ws_bytes = max(WS_MIN, min(want * Mp * Co * 4, 512 << 20))
    sp = min(_cdiv(1536, tiles), ws_bytes // (Mp * Co * 4), rows // 256)
    splits, kchunk = 1, rows
    if sp >= 2:
        kchunk = _cdiv(_cdiv(rows, sp), 32) * 32
        splits = _cdiv(rows, kchunk)
    narrow = Co % 128 != 0 or (Co // 128) * (Mp // 128) * splits <= 384
    return splits, kchunk, narrow


def dgrad_plan(ks, st, pd, dims):
    """ops._dgrad_plan: [(class, r, taps per axis, the class's sub-grid, base)] for the parity classes that have a tap and a position"""
    plan = []
    for cls in np.ndindex(*st):
        r = [(cls[a] + pd[a]) % st[a] for a in range(3)]
        sub = [len(range(r[a], ks[a], st[a])) for a in range(3)]
        size = [len(range(cls[a], dims[a], st[a])) for a in range(3)]
        if min(sub) >= 1 and min(size) >= 1:
            plan.append((tuple(cls), r, sub, size, [(cls[a] + pd[a] - r[a]) // st[a] for a in range(3)]))
    return plan


def plans(c, ws_bytes=WS_MIN):
    """pass -> [(splits, kchunk, narrow)] of every walk launch of the case (dx: one per parity class)"""
    Ci, Co, k, st, pd, N, T, H, W = c.geo
    _, rows, srows, taps = grids(c)
    cw, out = channel_width(c), {}
    if c.fwd == "walk":
        out["fwd"] = [walk_plan(rows, Co, taps * Ci, ws_bytes)]
    elif c.fwd == "walk4":
        out["fwd"] = [walk_plan(rows, Co, k[0] * k[1] * 32, ws_bytes)]
    if c.dx.startswith("walk"):
        out["dx"] = [walk_plan(N * size[0] * size[1] * size[2], Ci, sub[0] * sub[1] * sub[2] * Co, ws_bytes)
                     for _, _, sub, size, _ in dgrad_plan(k, st, pd, (T, H, W))]
    if c.dw == "walk":
        out["dw"] = [wgrad_plan(rows, taps * cw, Co)]
    return out


# ================================================================================================= the tap rule and the parity-class rule
def to_rows(a):
    """[N,C,T,H,W] -> channels-last [N,T,H,W,C]"""
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 4, 1)))


def to_planes(a):
    """[N,T,H,W,C] -> [N,C,T,H,W]"""
    return np.ascontiguousarray(np.transpose(a, (0, 4, 1, 2, 3)))


def gather(src, grid, stride, base, tap, sign=1, clamp=None):
    """src [N,T,H,W,C] -> [N g0 g1 g2, C]: row (n, o) is src[n, o stride + base + sign tap], zero outside the source grid.  clamp = axis:
    a planted error -- below that axis' lower border the read is clamped to the border instead of zero"""
    idx, ok = [], []
    for a in range(3):
        i = np.arange(grid[a]) * stride[a] + base[a] + sign * tap[a]
        v = (i >= 0) & (i < src.shape[1 + a])
        if clamp == a:
            v = v | (i < 0)
        idx.append(np.clip(i, 0, src.shape[1 + a] - 1))
        ok.append(v)
    out = src[:, idx[0][:, None, None], idx[1][None, :, None], idx[2][None, None, :]]
    m = ok[0][:, None, None] & ok[1][None, :, None] & ok[2][None, None, :]
    return np.where(m[None, ..., None], out, src.dtype.type(0)).reshape(-1, src.shape[-1])


def _taps(k):
    return [(a, b, c_) for a in range(k[0]) for b in range(k[1]) for c_ in range(k[2])]


def conv3d_taps_ref(x, w, b, stride, pad, ct=None):
    """the tap rule in plain numpy, in the dtype of x: y[n, o] = sum_tap x[n, s o + tap - pad] W_tap + b, zero outside; with ct also the
    gradients of sum(y ct) by the same rule turned round -> y, or (y, dx, dw, db)"""
    N, Ci, T, H, W = x.shape
    Co, k = w.shape[0], w.shape[2:]
    og = tuple((d + 2 * p - kk) // s + 1 for d, p, kk, s in zip((T, H, W), pad, k, stride))
    xr = to_rows(x)
    base = [-p for p in pad]
    y = np.zeros((N * og[0] * og[1] * og[2], Co), x.dtype)
    for tap in _taps(k):
        y += gather(xr, og, stride, base, tap) @ w[:, :, tap[0], tap[1], tap[2]].T
    if b is not None:
        y += b
    y = to_planes(y.reshape((N,) + og + (Co,)))
    if ct is None:
        return y
    dy = to_rows(ct).reshape(-1, Co)
    dxr, dw = np.zeros_like(xr), np.zeros_like(w)
    for tap in _taps(k):
        dw[:, :, tap[0], tap[1], tap[2]] = dy.T @ gather(xr, og, stride, base, tap)
        g = (dy @ w[:, :, tap[0], tap[1], tap[2]]).reshape((N,) + og + (Ci,))
        sl_o, sl_s = [], []
        for a in range(3):               # the outputs o whose source row s o + tap - pad lies inside the grid
            o = [i for i in range(og[a]) if 0 <= i * stride[a] + tap[a] - pad[a] < (T, H, W)[a]]
            if not o:
                break
            sl_o.append(slice(o[0], o[-1] + 1))
            s0 = o[0] * stride[a] + tap[a] - pad[a]
            sl_s.append(slice(s0, s0 + (len(o) - 1) * stride[a] + 1, stride[a]))
        else:
            dxr[:, sl_s[0], sl_s[1], sl_s[2]] += g[:, sl_o[0], sl_o[1], sl_o[2]]
    return y, to_planes(dxr), dw, dy.sum(0)


def class_kernel(w, r, st, sub, at_r=False):
    """the sub-kernel w[..., r::s] of a parity class.  at_r: a planted error -- the taps r, r + 1, ... instead of r, r + s, ..."""
    if at_r:
        return w[:, :, r[0]:r[0] + sub[0], r[1]:r[1] + sub[1], r[2]:r[2] + sub[2]]
    return w[:, :, r[0]::st[0], r[1]::st[1], r[2]::st[2]]


def class_walks(dy_rows, w, st, pd, dims, at_r=-1):
    """the data gradient's walks -> [(class, sub-grid, A [class rows, (tap, co)], B [(tap, co), ci])], tap-major then channel"""
    out = []
    for i, (cls, r, sub, size, base) in enumerate(dgrad_plan(tuple(w.shape[2:]), st, pd, dims)):
        ws_ = class_kernel(w, r, st, sub, at_r=i == at_r)
        A = np.concatenate([gather(dy_rows, size, (1, 1, 1), base, j, sign=-1) for j in _taps(sub)], 1)
        Bm = np.ascontiguousarray(np.transpose(ws_, (2, 3, 4, 0, 1))).reshape(-1, w.shape[1])
        out.append((cls, size, A, Bm))
    return out


def dgrad_classes_ref(ct, w, stride, pad, dims):
    """the data gradient by the parity-class rule in plain numpy -> dx [N,Ci,T,H,W]; positions of a class without a tap stay zero"""
    N, Ci = ct.shape[0], w.shape[1]
    dxr = np.zeros((N,) + tuple(dims) + (Ci,), ct.dtype)
    for cls, size, A, Bm in class_walks(to_rows(ct), w, stride, pad, dims):
        dxr[:, cls[0]::stride[0], cls[1]::stride[1], cls[2]::stride[2]] = (A @ Bm).reshape((N,) + tuple(size) + (Ci,))
    return to_planes(dxr)


def zero_mask(c):
    """dx positions that no (output, tap) pair reaches -- a parity class outside ops._dgrad_plan (W5), rows behind the last window (P3):
    identically zero in the reference, and on the GPU"""
    Ci, Co, k, st, pd, N, T, H, W = c.geo
    og = grids(c)[0]
    reach = []
    for a, dim in enumerate((T, H, W)):
        r = np.zeros(dim, bool)
        for o in range(og[a]):
            for j in range(k[a]):
                if 0 <= o * st[a] + j - pd[a] < dim:
                    r[o * st[a] + j - pd[a]] = True
        reach.append(r)
    m = ~(reach[0][:, None, None] & reach[1][None, :, None] & reach[2][None, None, :])
    return np.broadcast_to(m[None, None], (N, Ci, T, H, W))


# ================================================================================================= inputs, reference, yardstick A
def _rs(*key):
    return np.random.RandomState(sum((i + 3) * 7919 * int(k) for i, k in enumerate(key)) % 2 ** 31)


def draw(geo, stats):
    """-> x [N,Ci,T,H,W], w [Co,Ci,kt,kh,kw], b [Co], ct [N,Co,T',H',W'], fp32"""
    Ci, Co, k, st, pd, N, T, H, W = geo
    rs = _rs(Ci, Co, *k, *st, *pd, N, T, H, W)
    og = tuple((d + 2 * p - kk) // s + 1 for d, p, kk, s in zip((T, H, W), pd, k, st))
    x = rs.standard_normal((N, Ci, T, H, W))
    w = rs.standard_normal((Co, Ci) + tuple(k)) * 0.2
    b = rs.standard_normal(Co)
    ct = rs.standard_normal((N, Co) + og)
    if stats == "small":
        ct = ct * 1e-6
    elif stats == "decades":
        x = x * (10.0 ** rs.uniform(-4, 0, Ci))[None, :, None, None, None]
    else:
        assert stats == "normal", stats
    return x.astype(_F), w.astype(_F), b.astype(_F), ct.astype(_F)


def torch_conv(x, w, b, ct, stride, pad, dtype, dx=True):
    """torch.conv3d and its autograd on the CPU in `dtype`, one thread for float32 -> y, dx, dw, db as float64 numpy"""
    n_thr = torch.get_num_threads()
    if dtype == torch.float32:
        torch.set_num_threads(1)
    try:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        xt, wt, bt = t(x).requires_grad_(dx), t(w).requires_grad_(True), t(b).requires_grad_(True)
        y = torch.conv3d(xt, wt, bt, stride, pad)
        g = torch.autograd.grad(y, ([xt] if dx else []) + [wt, bt], t(ct))
        out = {"y": y, "dw": g[-2], "db": g[-1]}
        if dx:
            out["dx"] = g[0]
        return {n: v.detach().double().numpy() for n, v in out.items()}
    finally:
        torch.set_num_threads(n_thr)


def tensor_names(c):
    return ["y"] + (["dx"] if c.dx else []) + ["dw", "db"]


@functools.lru_cache(maxsize=None)
def _data(geo, stats):
    x, w, b, ct = draw(geo, stats)
    st, pd = geo[3], geo[4]
    ref = torch_conv(x, w, b, ct, st, pd, torch.float64)
    yard = torch_conv(x, w, b, ct, st, pd, torch.float32)
    return dict(x=x, w=w, b=b, ct=ct, ref=ref, e32={n: rel_err(yard[n], ref[n]) for n in ref})


def data(c):
    """inputs, float64 reference and yardstick A of a case, once per (geometry, statistics), left unchanged"""
    return _data(c.geo, c.stats)


# ================================================================================================= yardstick B: the products
PLANTS = ("", "lo_hi_tap", "lo_last_tile", "bias_f16", "clamp", "class_r", "tap8", "lo_hi")
PLANT_TEXT = {
    "lo_hi_tap": "lo(A) hi(B) is dropped on one tap of 27 (the centre tap of the forward walk)",
    "lo_last_tile": "the low half of A is dropped on the ragged last 32-deep k tile of the weight gradient (rows 64 .. 74 of 75)",
    "bias_f16": "the bias is rounded to fp16 before the direct epilogue adds it",
    "clamp": "a padding tap is read clamped instead of zero at the lower border of the W axis",
    "class_r": "one parity class's sub-kernel is taken at r, r + 1 instead of r, r + s",
    "tap8": "the first layer's first padding tap (pixel kw of 8) is read and carries a non-zero weight",
    "lo_hi": "lo(A) hi(B) is dropped everywhere in the data gradient's walk",
}


def walk_product(A, Bm, model, amax, plan=(1, None, True), drop=None):
    """A [M,K] @ Bm [K,N] in float32 as sgemm_x6_kernel forms it: per split-K slab one accumulator over 16-deep MFMAs (fp16x3: lo hi, hi lo,
    hi hi under the slots' scales; x6: six bf16 products, smallest first; fp32: one product), the slabs added in order.  drop: the k at
    which a planted error loses the low half of A"""
    A, Bm = np.ascontiguousarray(A, _F), np.ascontiguousarray(Bm, _F)
    K = A.shape[1]
    kchunk = plan[1] or K
    if model == "f16x3":
        sa, ia = f16_scale(_F(amax[0]))
        sb, ib = f16_scale(_F(amax[1]))
        ah, al = split_f16(A, sa)
        bh, bl = split_f16(Bm, sb)
        if drop is not None:
            al = np.where(drop[None, :], _F(0), al)
        terms = lambda s: [(al[:, s], bh[s]), (ah[:, s], bl[s]), (ah[:, s], bh[s])]
    elif model == "x6":
        a, b = split_bf16(A), split_bf16(Bm)
        ia = ib = _F(1)
        terms = lambda s: [(a[2][:, s], b[0][s]), (a[1][:, s], b[1][s]), (a[0][:, s], b[2][s]), (a[1][:, s], b[0][s]), (a[0][:, s], b[1][s]),
                           (a[0][:, s], b[0][s])]
    else:
        assert model == "fp32", model
        ia = ib = _F(1)
        terms = lambda s: [(A[:, s], Bm[s])]
    out = None
    for k0 in range(0, K, kchunk):
        v = ((mfma_acc(terms(slice(k0, min(K, k0 + kchunk))), 16) * ia).astype(_F) * ib).astype(_F)
        out = v if out is None else (out + v).astype(_F)
    return out


def fwd_matrix(xr, c, cw, clamp=None):
    """the forward walk's A [rows, (tap, channel)] over x channels-last (cw channels), natural taps"""
    Ci, Co, k, st, pd = c.geo[:5]
    og = grids(c)[0]
    return np.concatenate([gather(xr, og, st, [-p for p in pd], tap, clamp=clamp) for tap in _taps(k)], 1)


def fwd4_operands(x4, w, c, tap8=False):
    """m3t_conv3d_fwd_taps4: A [rows, ((kt, kh), pixel 0..7, channel 0..3)] (pixels past kw: not read) and B from w8 [Co][kt][kh][8][4]"""
    Ci, Co, k, st, pd = c.geo[:5]
    og, rows = grids(c)[:2]
    cols = []
    for jt in range(k[0]):
        for jh in range(k[1]):
            for q in range(8):
                read = q < k[2] or (tap8 and q == k[2])
                cols.append(gather(x4, og, st, [-p for p in pd], (jt, jh, q)) if read else np.zeros((rows, 4), _F))
    w8 = np.zeros((Co, k[0], k[1], 8, 4), _F)
    w8[:, :, :, :k[2], :Ci] = np.transpose(w, (0, 2, 3, 4, 1))
    if tap8:
        w8[:, :, :, k[2]] = w8[:, :, :, k[2] - 1]
    return np.concatenate(cols, 1), np.ascontiguousarray(w8.reshape(Co, -1).T)


def patch_matrix(xr, c, Kp, rows_p=None):
    """m3t_im2col3d: [rows (zero rows up to rows_p), Kp] with columns (ci, kt, kh, kw), zero-padded"""
    Ci = c.geo[0]
    _, rows, _, taps = grids(c)
    A = fwd_matrix(xr, c, Ci).reshape(rows, taps, Ci).transpose(0, 2, 1).reshape(rows, taps * Ci)
    pat = np.zeros((rows_p or rows, Kp), _F)
    pat[:rows, :taps * Ci] = A
    return pat


def emulate(c, plant=""):
    """one forward + backward of the case in numpy float32 as the path `route` names forms it -> tensor_names(c)"""
    assert plant in PLANTS, plant
    d = data(c)
    Ci, Co, k, st, pd, N, T, H, W = c.geo
    og, rows, srows, taps = grids(c)
    x, w, b, ct = d["x"], d["w"], d["b"], d["ct"]
    xr, dyr = to_rows(x), to_rows(ct)
    dy = dyr.reshape(rows, Co)
    a_x, a_w, a_dy = np.abs(x).max(), np.abs(w).max(), np.abs(ct).max()
    model = c.prec
    pl = plans(c)
    cw = channel_width(c)
    bias = b.astype(np.float16).astype(_F) if plant == "bias_f16" else b
    out = {}
    # ---- forward
    if c.fwd == "walk":
        A = fwd_matrix(xr, c, Ci, clamp=2 if plant == "clamp" else None)
        Bm = np.ascontiguousarray(np.transpose(w, (2, 3, 4, 1, 0))).reshape(taps * Ci, Co)
        drop = None
        if plant == "lo_hi_tap":
            drop = np.zeros(taps * Ci, bool)
            drop[(taps // 2) * Ci:(taps // 2 + 1) * Ci] = True
        y = walk_product(A, Bm, "f16x3", (a_x, a_w), pl["fwd"][0], drop)
    elif c.fwd == "walk4":
        x4 = np.zeros((N, T, H, W, 4), _F)
        x4[..., :Ci] = xr
        A, Bm = fwd4_operands(x4, w, c, tap8=plant == "tap8")
        y = walk_product(A, Bm, "f16x3", (a_x, a_w), pl["fwd"][0])
    elif c.fwd == "patch":
        Kc = taps * Ci
        Kp = Kc if Kc % 64 == 0 else _cdiv(Kc, 128) * 128
        pat = patch_matrix(xr, c, Kp)
        w2 = np.zeros((Co, Kp), _F)
        w2[:, :Kc] = w.reshape(Co, Kc)
        y = gemm_product(pat, w2.T, gemm_route(rows, Co, Kp, model))
    else:
        y = walk_product(patch_matrix(xr, c, taps * Ci), w.reshape(Co, -1).T, "fp32", None)
    out["y"] = to_planes((y + bias).astype(_F).reshape((N,) + og + (Co,)))
    # ---- data gradient
    if c.dx:
        m = {"walk": "f16x3", "walk_loop": "f16x3", "walk_x6": "x6", "stock": "fp32"}[c.dx]
        dxr = np.zeros((N, T, H, W, Ci), _F)
        walks = class_walks(dyr, w, st, pd, (T, H, W), at_r=_class_with_two_taps(c) if plant == "class_r" else -1)
        for i, (cls, size, A, Bm) in enumerate(walks):
            plan = pl["dx"][i] if "dx" in pl else (1, None, True)
            drop = np.ones(A.shape[1], bool) if plant == "lo_hi" else None
            v = walk_product(A, Bm, m, (a_dy, a_w), plan, drop)
            dxr[:, cls[0]::st[0], cls[1]::st[1], cls[2]::st[2]] = v.reshape((N,) + tuple(size) + (Ci,))
        out["dx"] = to_planes(dxr)
    # ---- weight gradient
    if c.dw == "walk":
        if cw == Ci:
            A = fwd_matrix(xr, c, Ci)
        else:
            x4 = np.zeros((N, T, H, W, 4), _F)
            x4[..., :Ci] = xr
            A = fwd_matrix(x4, c, 4)
        drop = None
        if plant == "lo_last_tile":
            drop = np.arange(rows) >= (rows - 1) // 32 * 32
        dwt = walk_product(A.T, dy, "f16x3", (a_x, a_dy), pl["dw"][0], drop)
        dw = dwt.reshape(taps, cw, Co)[:, :Ci].transpose(2, 1, 0).reshape(w.shape)
    else:
        Kc = taps * Ci
        if c.dw == "dyTP":
            dw = gemm_product(dy.T, patch_matrix(xr, c, Kc), gemm_route(Co, Kc, rows, model))
        elif c.dw == "PTdy":
            Kp, rows_p = _cdiv(Kc, 128) * 128, _cdiv(rows, 32) * 32
            dyp = np.zeros((rows_p, Co), _F)
            dyp[:rows] = dy
            dw = gemm_product(patch_matrix(xr, c, Kp, rows_p).T, dyp, gemm_route(Kp, Co, rows_p, model))[:Kc].T
        else:
            Kp = _cdiv(Kc, 4) * 4
            dw = gemm_product(dy.T, patch_matrix(xr, c, Kp), gemm_route(Co, Kp, rows, model))[:, :Kc]
        dw = dw.reshape(w.shape)
    out["dw"] = np.ascontiguousarray(dw)
    out["db"] = dy.sum(0, dtype=_F)
    return out


def _class_with_two_taps(c):
    Ci, Co, k, st, pd, N, T, H, W = c.geo
    for i, (_, _, sub, _, _) in enumerate(dgrad_plan(k, st, pd, (T, H, W))):
        if max(sub) >= 2:
            return i
    raise AssertionError("no parity class of %s has two taps on an axis" % c.id)


@functools.lru_cache(maxsize=None)
def _emulated(geo, stats, off, prec, fwd, dx, dw):
    c = Case("", "", geo, off, prec, stats, fwd, dx, dw, "")
    out, ref = emulate(c), _data(geo, stats)["ref"]
    return {n: rel_err(out[n], ref[n]) for n in tensor_names(c)}


def emulated(c):
    """E_emu per tensor, once per (geometry, statistics, path)"""
    return _emulated(c.geo, c.stats, c.off, c.prec, c.fwd, c.dx, c.dw)


def limits(c):
    """tensor name -> (upper bound on rel_err, lower bound or None); see the module docstring for the `decades` class"""
    d, e_emu = data(c), emulated(c)
    out = {}
    for n in tensor_names(c):
        e32 = max(d["e32"][n], FLOOR)
        if c.stats == "decades" and c.prec == "f16x3" and e_emu[n] > BOUND * e32:
            out[n] = (BOUND * e_emu[n], BOUND * e32)
        else:
            out[n] = (BOUND * max(e32, e_emu[n]), None)
    return out


def check(got, c, quiet=False):
    """got: name -> array (torch's layouts) of tensor_names(c) of some fp32 implementation -> (worst ratio in units of the yardstick, its
    tensor, failures)"""
    d, lim = data(c), limits(c)
    worst, fails = (0.0, ""), []
    for n in tensor_names(c):
        ref = d["ref"][n]
        g = np.asarray(got[n], np.float64).reshape(ref.shape)
        if n == "dx":
            z = zero_mask(c)
            if z.any() and (g[z].any() or not np.isfinite(g[z]).all()):
                fails.append("dx: the positions no tap reaches must be identically zero")
        err = rel_err(g, ref)
        hi, lo = lim[n]
        ratio = BOUND * err / hi
        worst = max(worst, (ratio, n))
        if not err <= hi:
            fails.append("%s: rel_err %.3g > %.3g (%.2f x the yardstick, bound %g)" % (n, err, hi, ratio, BOUND))
        if lo is not None and not err > lo:
            fails.append("%s: rel_err %.3g does not exceed %.3g: the normwise limit of fp16x3 is no longer reached" % (n, err, lo))
    if not quiet:
        print("%-4s worst %6.2f x  %s" % (case_id(c), worst[0], worst[1]))
    return worst[0], worst[1], fails


def close_verdict(got, ref, tol):
    """what close() of tests/test_gpu_parity.py makes of `got`: max |got - ref| <= tol max(1, max |ref|)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()))


CLOSE_TOL = {"y": 1e-4, "dx": 2e-4, "dw": 2e-4, "db": 2e-4}          # the tolerances the four convolution tests of test_gpu_parity.py use
