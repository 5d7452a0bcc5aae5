"""Float64 reference, two fp32 yardsticks and the error bound for the temporal convolutions: csrc/tcn.hip (causal_conv_kernel<0/1>, the
weight-norm kernels), the CONV form of csrc/gemm_x6.hip, m3t_conv1d_wgrad_scaled, m3t_mask_pos / m3t_mask_pos_drop and _TemporalBlock of
m3t/ops.py behind models.tcn.  tests/test_tcn_ref_host.py checks this file on the CPU; tests/test_gpu_tcn_fp64.py holds the kernels to it.

Layout: everything here is channels-last, x [B, T, C], w_t [K][Co][Ci] (the time-flipped data-gradient form reads w_t [K][Ci][Co]).

Reference    float64 on the fp32 inputs and parameters.  The blocks go through oracle.m3t_oracle (weight_norm_fwd/bwd, temporal_block_fwd/bwd
             with masks=, dropout_mask); what the oracle lacks is here: the general tap rule of include/m3t_hip.h (`conv_taps`: lead,
             anticausal), the fused epilogue (`epilogue`: act 0/1/2 with pre, res and mask) and the per-tap weight gradient with its
             span >= T rule (`wgrad_ref`).  The host file holds conv_taps / wgrad_ref to the oracle's causal_conv1d_* and conv1d_same_* and
             to torch's float64 autograd.
Yardstick A  (E32)   torch's float32 CPU autograd, one thread, of the literal composition: F.conv1d for the operator-level cases,
             torch.nn.utils.weight_norm(nn.Conv1d(..., padding=(k-1) d, dilation=d)), chomp, ReLU, x the same pre-scaled mask, the 1x1
             downsample and the final ReLU for the blocks.
Yardstick B  (E_emu) a numpy float32 restatement of the products of the kernel a case reaches, written from the kernel text with
             f16_scale, split_f16, split_bf16 and mfma_acc of tests/test_fp16x3_model.py:
  * fp32     causal_conv_kernel: one fp32 accumulator per output, over 16-channel slabs (a ragged last slab zero-filled), over the taps
             within a slab, two k per MFMA (v_mfma_f32_32x32x2f32);
  * f16x3    the CONV form with NS = 4: two fp16 terms of each operand under its slot's power-of-two scale, products lo hi, hi lo, hi hi
             per 16-deep MFMA, k ordered tap-major then channel, times the two inverse scales;
  * x6       three bf16 terms per operand, six products smallest first (NS = 3);
  the epilogue (bias, pre, ReLU x mask, + res, ReLU) in fp32 as the kernels group it.  Weight gradients and the 1x1 residual products are
  sent by gru_ref.gemm_route to the model plan_gemm of csrc/gemm.hip picks.  Weight-norm, mask_pos and the bias column sums are fp32 numpy.
  Not modelled: the split-K slab order of the weight gradients, which wave owns which k, the order of a wavefront's sum in the weight-norm
  kernels and of the column sums -- other summation orders of the same length, which the factor BOUND covers.

Metric  rel_err(got, ref) = max |got - ref| / max |ref| per tensor, never max(1, .); the reference maximum must be finite and non-zero.
Bound   rel_err(gpu) <= BOUND max(E32, E_emu, 2^-24), BOUND = fuse_loss_ref.BOUND = 4.0.  Not fitted to GPU output.  A tensor that is
        identically zero in the reference (the fully masked taps of W2 and C6b) must be identically zero.

ReLU decisions.  Forward outputs need no care (ReLU is 1-Lipschitz).  The backward pass through a block multiplies by three 0/1 masks, and
a pre-activation closer to zero than the rounding error could flip one.  A block-level case is therefore drawn by `draw_clear`: no
pre-activation of the three ReLUs of any block (a1, a2, s = h2 + res) of the float64 reference may lie within 2^-19 A of zero, A the sum of
the absolute terms of the element (sum |x w| + |b|; for s: that of a2 where the mask keeps it, + |res|) -- four times the per-element bound
DESIGN section 7 states for fp16x3 -- and every ReLU keeps at least 25 % of its pre-activations on either side.  Recipe: the biases b1, b2,
bd carry per-channel offsets of +-3 standard deviations of the bias-free pre-activation about its centre (b = -mean +- 3 std: behind a
ReLU the bias-free pre-activation of conv2 has a mean of its own), so do the input channels when the first block's residual is the
identity; consecutive seeds, the first clear one is taken.  The sign is drawn per channel, with one rule: a deeper identity block adds a
ReLU output, so s = h2 + res >= 0 and its ReLU closes only where both vanish -- there conv2 takes the negative offset on the channels its
residual leaves mostly at zero (else s > 0 on 80 - 98 % and the balance fails at every seed) and the positive one with probability 0.7 on
the others.  Every case of the table is admitted (the host file asserts it); about two seeds in three are clear at 128 channels: A is
~40 std there, so the margin 2^-19 A catches one element of 3 10^5 now and then.

The normwise character of fp16x3: an element far below its operand's maximum keeps an absolute, not a relative error.  On
the `decades` class (input channel magnitudes spread over four decades) `limits` names, from the emulation alone, the tensors this reaches
(E_emu > BOUND max(E32, 2^-24)); they are held to BOUND E_emu and must EXCEED BOUND max(E32, 2^-24), so a change of the scaling shows up.
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from fuse_loss_ref import BOUND
from gru_ref import gemm_route, rel_err
from oracle import m3t_oracle as O
from test_fp16x3_model import f16_scale, split_f16, split_bf16, mfma_acc

FLOOR = 2.0 ** -24
MARGIN = 2.0 ** -19
_F = np.float32
DROP_P = 0.2
FORMS = ("pre", "mask", "drop", "res", "anti")
# pre: act 0, bias, pre buffer | mask: act 1, mask tensor | drop: act 1, in-kernel Philox mask | res: act 2, mask tensor, res
# anti: the data-gradient form: time-flipped, w_t [K][Ci][Co], no bias, res added

Op = collections.namedtuple("Op", "id kernel B T Ci Co K dil lead form prec")
Wg = collections.namedtuple("Wg", "id B T Ci Co K dil lead prec")
Blk = collections.namedtuple("Blk", "id Cin widths K B T train stats prec")
# kernel: "fp32" (causal_conv_kernel) | "conv" (CONV of gemm_x6.hip);  prec: "f16x3" (default) | "x6";  stats: normal | small | decades


def _ops():
    rows = (
        ("E1", "fp32", (3, 37, 20, 36, 3, 4), 0, FORMS),
        ("E2", "fp32", (5, 29, 7, 130, 2, 1), 0, ("pre", "drop", "anti")),
        ("E3", "fp32", (2, 5, 16, 32, 3, 8), 0, ("res", "anti")),
        ("E4", "fp32", (2, 200, 16, 32, 3, 64), 0, ("mask", "anti")),
        ("E5a", "fp32", (1, 1, 4, 4, 5, 1), 2, ("pre", "anti")),
        ("E5b", "fp32", (3, 2, 8, 12, 5, 1), 2, ("pre", "anti")),
        ("E6", "fp32", (4, 96, 64, 128, 3, 2), 0, ("pre", "anti")),           # unaligned operands: an interior shape on the edge kernel
        ("I1", "conv", (4, 96, 64, 128, 3, 2), 0, FORMS),
        ("I2", "conv", (4, 32, 32, 128, 2, 16), 0, ("pre", "anti")),
        ("I2b", "conv", (4, 32, 32, 128, 2, 32), 0, ("mask", "anti")),
        ("I3", "conv", (1, 128, 96, 256, 3, 1), 0, ("drop", "res", "anti")),
        ("I4", "conv", (2, 192, 32, 128, 5, 1), 2, ("pre", "anti")),
    )
    out = []
    for id_, kern, shape, lead, forms in rows:
        for prec in (("f16x3", "x6") if kern == "conv" else ("f16x3",)):
            for form in forms:
                out.append(Op(id_, kern, *shape, lead, form, prec))
    return tuple(out)


def _wgs():
    rows = (("W1", (4, 96, 64, 128, 3, 40), 0, 2), ("W2", (2, 5, 16, 32, 3, 8), 0, 1), ("W3", (3, 37, 20, 36, 3, 4), 0, 1),
            ("W4", (16, 64, 128, 128, 3, 1), 0, 2), ("W5", (2, 192, 32, 128, 5, 1), 2, 2))
    return tuple(Wg(id_, *shape, lead, prec) for id_, shape, lead, n in rows for prec in ("f16x3", "x6")[:n])


BLOCKS = (
    Blk("C1", 64, (128, 128), 3, 4, 96, False, "normal", "f16x3"),
    Blk("C2", 64, (128, 128), 3, 4, 96, True, "normal", "f16x3"),
    Blk("C3", 20, (36, 36, 36), 2, 3, 37, False, "normal", "f16x3"),
    Blk("C3t", 20, (36, 36, 36), 2, 3, 37, True, "normal", "f16x3"),
    Blk("C4", 128, (128,), 3, 2, 64, False, "normal", "f16x3"),
    Blk("C5s", 64, (128, 128), 3, 4, 96, False, "small", "f16x3"),
    Blk("C5d", 64, (128, 128), 3, 4, 96, False, "decades", "f16x3"),
    Blk("C6", 32, (128, 128, 128), 3, 4, 32, False, "normal", "f16x3"),
    Blk("C6b", 32, (128,) * 5, 3, 8, 16, False, "normal", "f16x3"),
    Blk("C1x6", 64, (128, 128), 3, 4, 96, False, "normal", "x6"),
)
OPS, WGS = _ops(), _wgs()
CASES = OPS + WGS + BLOCKS          # ONE table, imported by both test files; every case is admitted


def case_id(c):
    if isinstance(c, Op):
        return "%s-%s-%s" % (c.id, c.form, c.prec)
    return "%s-%s" % (c.id, c.prec)


def interior(B, T, Ci, Co, aligned=True):
    """the predicate of m3t_conv1d_fwd_scaled that sends a shape to the CONV form of gemm_x6.hip"""
    return (B * T) % 128 == 0 and Co % 128 == 0 and Ci % 32 == 0 and aligned


def conv_model(B, T, Ci, Co, prec, aligned=True):
    return prec if interior(B, T, Ci, Co, aligned) else "fp32"


# ================================================================================================= the reference: taps, epilogue, wgrad
def tap_offset(j, K, dil, lead, anti):
    sft = (K - 1 - j) * dil
    return sft - lead if anti else lead - sft


def tap_rows(x, j, K, dil, lead, anti, leak=False):
    """x [B,T,C] -> the rows tap j multiplies, [B,T,C]: x[b, t + off_j] inside the clip, zero outside (include/m3t_hip.h).  leak: a planted
    error -- the row just before a clip's start is taken from the previous clip's last row"""
    B, T, C = x.shape
    off = tap_offset(j, K, dil, lead, anti)
    A = np.zeros_like(x)
    lo, hi = max(0, -off), min(T, T - off)
    if hi > lo:
        A[:, lo:hi] = x[:, lo + off:hi + off]
    if leak and off < 0 and -off - 1 < T:
        A[1:, -off - 1] = x[:-1, T - 1]
    return A


def conv_taps(x, w_t, K, dil, lead=0, anti=False):
    """sum_j x[b, t + off_j] W_j, no bias; w_t [K][Co][Ci], or [K][Ci][Co] when anti"""
    B, T, C = x.shape
    a = 0
    for j in range(K):
        Wj = w_t[j] if anti else w_t[j].T
        a = a + tap_rows(x, j, K, dil, lead, anti).reshape(B * T, C) @ Wj
    return a.reshape(B, T, -1)


def epilogue(v, act, res, mask, res_first=False):
    """the fused tail of the conv kernels on v = conv + bias, in v's dtype"""
    mk = 1 if mask is None else mask
    zero = v.dtype.type(0)
    if act == 1:
        return (np.maximum(v, zero) * mk).astype(v.dtype)
    if act == 2:
        if res_first:
            return np.maximum(((np.maximum(v, zero) + res).astype(v.dtype) * mk).astype(v.dtype), zero)
        return np.maximum(((np.maximum(v, zero) * mk).astype(v.dtype) + res).astype(v.dtype), zero)
    return v if res is None else (v + res).astype(v.dtype)


def wgrad_ref(dy, x, K, dil, lead=0):
    """dw_t[j][co][ci] = sum_{b,t} dy[b,t,co] x[b, t + off_j, ci]; a tap whose shift leaves no row inside the clip (span >= T) is zeros"""
    B, T, Co = dy.shape
    Ci = x.shape[-1]
    out = np.zeros((K, Co, Ci), dy.dtype)
    for j in range(K):
        out[j] = dy.reshape(B * T, Co).T @ tap_rows(x, j, K, dil, lead, False).reshape(B * T, Ci)
    return out


def drop_mask(rows, C, seed, by_row=False):
    """the pre-scaled in-kernel dropout mask (oracle.dropout_mask).  by_row: a planted error -- the Philox counter takes the row, not the
    group of four rows"""
    if not by_row:
        return O.dropout_mask(rows, C, DROP_P, seed)
    r = np.broadcast_to(np.arange(rows, dtype=np.uint32)[:, None], (rows, C))
    col = np.broadcast_to(np.arange(C, dtype=np.uint32)[None, :], (rows, C))
    z = np.zeros((rows, C), np.uint32)
    words = np.stack(O.philox4x32_10(col, r, z, z, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF), 0)
    w = np.take_along_axis(words, (r & 3)[None].astype(np.int64), 0)[0]
    keep = 1.0 - DROP_P
    return (w < np.uint32(int(keep * 4294967296.0))).astype(np.float64) * np.float64(_F(1.0 / keep))


# ================================================================================================= yardstick B: products
def product(A, Bm, model, amax=(None, None), drop_lo=False, kstep=None):
    """A [M,K] @ Bm [K,N] in float32 as the kernels of `model` form it; amax: the operands' magnitude slots (None: measured here)"""
    A, Bm = np.ascontiguousarray(A, _F), np.ascontiguousarray(Bm, _F)
    if model == "fp32":
        return mfma_acc([(A, Bm)], kstep or 16)
    if model == "f16x3":
        sa, ia = f16_scale(_F(np.abs(A).max()) if amax[0] is None else _F(amax[0]))
        sb, ib = f16_scale(_F(np.abs(Bm).max()) if amax[1] is None else _F(amax[1]))
        ah, al = split_f16(A, sa)
        bh, bl = split_f16(Bm, sb)
        terms = [(ah, bl), (ah, bh)] if drop_lo else [(al, bh), (ah, bl), (ah, bh)]
        return ((mfma_acc(terms, 16) * ia).astype(_F) * ib).astype(_F)
    assert model == "x6", model
    a, b = split_bf16(A), split_bf16(Bm)
    return mfma_acc([(a[2], b[0]), (a[1], b[1]), (a[0], b[2]), (a[1], b[0]), (a[0], b[1]), (a[0], b[0])], 16)


PLANTS = ("", "lo_hi", "slot", "slot20", "leak", "slab", "drop_row", "res_first")
PLANT_TEXT = {
    "lo_hi": "the lo hi product of the fp16x3 split is dropped",
    "slot": "the magnitude slot of x is 2^8 too large (harmless: the low fp16 term keeps its bits down to 2^-14 of the scaled maximum)",
    "slot20": "the magnitude slot of x is 2^20 too large",
    "leak": "a tap is shifted by one row at a clip boundary (the previous clip's last row leaks in)",
    "slab": "the last 16-channel slab is skipped",
    "drop_row": "the dropout mask is taken at `row` instead of `row >> 2` groups",
    "res_first": "res is added before instead of after the mask",
}


def emu_conv(x, w_t, bias, res, mask, K, dil, lead, act, anti, model, amax=(None, None), plant=""):
    """m3t_conv1d_fwd_scaled in numpy float32 -> (y, pre)"""
    B, T, C = x.shape
    x, w_t = np.ascontiguousarray(x, _F), np.ascontiguousarray(w_t, _F)
    taps = [tap_rows(x, j, K, dil, lead, anti, leak=plant == "leak").reshape(B * T, C) for j in range(K)]
    Ws = [np.ascontiguousarray(w_t[j] if anti else w_t[j].T) for j in range(K)]
    if model == "fp32":
        slabs = list(range(0, C, 16))
        if plant == "slab":
            slabs = slabs[:-1]
        pad = lambda m, ax: np.concatenate([m, np.zeros(m.shape[:ax] + (16 - m.shape[ax],) + m.shape[ax + 1:], _F)], ax) if m.shape[ax] < 16 else m
        A = np.concatenate([pad(taps[j][:, c0:c0 + 16], 1) for c0 in slabs for j in range(K)], 1) if slabs else np.zeros((B * T, 2), _F)
        Bm = np.concatenate([pad(Ws[j][c0:c0 + 16], 0) for c0 in slabs for j in range(K)], 0) if slabs else np.zeros((2, Ws[0].shape[1]), _F)
        acc = product(A, Bm, "fp32", kstep=2)
    else:
        ax = np.abs(x).max() if amax[0] is None else amax[0]
        aw = np.abs(w_t).max() if amax[1] is None else amax[1]
        if plant.startswith("slot"):
            ax = _F(ax) * _F(2.0 ** int(plant[4:] or 8))
        acc = product(np.concatenate(taps, 1), np.concatenate(Ws, 0), model, (ax, aw), drop_lo=plant == "lo_hi")
    v = acc if bias is None else (acc + bias.astype(_F)).astype(_F)
    v = v.reshape(B, T, -1)
    return epilogue(v, act, None if res is None else res.astype(_F), None if mask is None else mask.astype(_F),
                    res_first=plant == "res_first"), v


def wgrad_route(B, T, Ci, Co, K, dil, lead, prec, j):
    """(model, reduction length, segment length) of tap j of m3t_conv1d_wgrad_scaled, or None for a tap written as zeros"""
    span = abs(tap_offset(j, K, dil, lead, False))
    if span >= T:
        return None
    return gemm_route(Co, Ci, B * (T - span), prec, seg_len=T - span), B * (T - span), T - span


def emu_wgrad(dy, x, K, dil, lead, prec):
    B, T, Co = dy.shape
    Ci = x.shape[-1]
    dy, x = np.ascontiguousarray(dy, _F), np.ascontiguousarray(x, _F)
    amax = (np.abs(dy).max(), np.abs(x).max())          # the K taps share both slots
    out = np.zeros((K, Co, Ci), _F)
    for j in range(K):
        r = wgrad_route(B, T, Ci, Co, K, dil, lead, prec, j)
        if r is None:
            continue
        off = tap_offset(j, K, dil, lead, False)
        ao, bo, L = max(0, -off), max(0, off), r[2]
        out[j] = product(dy[:, ao:ao + L].reshape(-1, Co).T, x[:, bo:bo + L].reshape(-1, Ci), r[0], amax)
    return out


def emu_weight_norm(v, g):
    """weight_norm_fwd_kernel: -> (w_t [K][Co][Ci], norm [Co])"""
    v, g = v.astype(_F), g.reshape(-1).astype(_F)
    nrm = np.sqrt((v * v).astype(_F).sum(axis=(1, 2), dtype=_F)).astype(_F)
    w = (v * (g / nrm).astype(_F)[:, None, None]).astype(_F)
    return np.ascontiguousarray(w.transpose(2, 0, 1)), nrm


def emu_weight_norm_bwd(dw_t, v, g, nrm):
    v, g = v.astype(_F), g.reshape(-1).astype(_F)
    dw = dw_t.transpose(1, 2, 0).astype(_F)
    dot = (dw * v).astype(_F).sum(axis=(1, 2), dtype=_F)
    dg = (dot / nrm).astype(_F)
    a, b = (g / nrm).astype(_F), (dot / (nrm * nrm).astype(_F)).astype(_F)
    dv = (a[:, None, None] * (dw - (v * b[:, None, None]).astype(_F)).astype(_F)).astype(_F)
    return dv, dg.reshape(-1, 1, 1)


# ================================================================================================= operator-level cases
SEED = 0x5DEECE66D1234


def _rs(*key):
    return np.random.RandomState(sum((i + 3) * 7919 * int(k) for i, k in enumerate(key)) % 2 ** 31)


def op_args(c):
    """(act, anti) of a form"""
    return {"pre": (0, 0), "mask": (1, 0), "drop": (1, 0), "res": (2, 0), "anti": (0, 1)}[c.form]


@functools.lru_cache(maxsize=None)
def op_inputs(shape, lead):
    B, T, Ci, Co, K, dil = shape
    rs = _rs(B, T, Ci, Co, K, dil, lead)
    return dict(x=rs.standard_normal((B, T, Ci)).astype(_F), w=(rs.standard_normal((K, Co, Ci)) / np.sqrt(Ci * K)).astype(_F),
                w_anti=(rs.standard_normal((K, Ci, Co)) / np.sqrt(Ci * K)).astype(_F), bias=(0.5 * rs.standard_normal(Co)).astype(_F),
                res=rs.standard_normal((B, T, Co)).astype(_F), mask=((rs.uniform(size=(B, T, Co)) > DROP_P) / _F(1 - DROP_P)).astype(_F))


def op_operands(c):
    """-> (x, w_t, bias, res, mask tensor or None, mask the reference multiplies by or None) of the case's form, fp32"""
    d = op_inputs((c.B, c.T, c.Ci, c.Co, c.K, c.dil), c.lead)
    if c.form == "anti":
        return d["x"], d["w_anti"], None, d["res"], None, None
    if c.form == "pre":
        return d["x"], d["w"], d["bias"], None, None, None
    if c.form == "drop":
        return d["x"], d["w"], d["bias"], None, None, drop_mask(c.B * c.T, c.Co, SEED).reshape(c.B, c.T, c.Co)
    return d["x"], d["w"], d["bias"], (d["res"] if c.form == "res" else None), d["mask"], d["mask"]


def _torch_op(c, x, w_t, bias, res, mk, dtype):
    """the literal torch composition of an operator-level case on the CPU, one thread -> y (and pre) as float64 numpy"""
    n_thr = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        act, anti = op_args(c)
        halo = (c.K - 1) * c.dil
        if anti:      # the data gradient of the forward conv with weight [Ci][Co][K] (Co channels in, Ci out): d / dz of sum(conv(z) x)
            z = torch.zeros(c.B, c.Co, c.T, dtype=dtype, requires_grad=True)
            out = F.conv1d(F.pad(z, (halo - c.lead, c.lead)), t(w_t.transpose(1, 2, 0)), None, dilation=c.dil)
            y, = torch.autograd.grad(out, z, t(x).permute(0, 2, 1))
            y = y.permute(0, 2, 1) + t(res)
            return {"y": y.double().numpy()}
        v = F.conv1d(F.pad(t(x).permute(0, 2, 1), (halo - c.lead, c.lead)), t(w_t.transpose(1, 2, 0)), t(bias), dilation=c.dil).permute(0, 2, 1)
        if act == 0:
            return {"y": v.double().numpy(), "pre": v.double().numpy()}
        h = torch.relu(v) * t(mk)
        if act == 2:
            h = torch.relu(h + t(res))
        return {"y": h.double().numpy()}
    finally:
        torch.set_num_threads(n_thr)


def op_reference(c):
    x, w_t, bias, res, _, mk = op_operands(c)
    act, anti = op_args(c)
    f = lambda a: None if a is None else a.astype(np.float64)
    v = conv_taps(f(x), f(w_t), c.K, c.dil, c.lead, bool(anti))
    if bias is not None:
        v = v + f(bias)
    out = {"y": epilogue(v, act, f(res), f(mk))}
    if c.form == "pre":
        out["pre"] = v
    return out


def _op_key(c):
    return (c.B, c.T, c.Ci, c.Co, c.K, c.dil, c.lead, c.form)


@functools.lru_cache(maxsize=None)
def _op_data(key):
    c = Op("", "", *key[:7], key[7], "")
    ref = op_reference(c)
    yard = _torch_op(c, *op_operands(c)[:4], op_operands(c)[5], torch.float32)
    return dict(ref=ref, e32={n: rel_err(yard[n], ref[n]) for n in ref})


def op_data(c):
    """float64 reference and yardstick A of an operator-level case, once per (shape, form), left unchanged"""
    return _op_data(_op_key(c))


def op_emulate(c, plant="", amax=(None, None), model=None):
    x, w_t, bias, res, _, mk = op_operands(c)
    if plant == "drop_row":
        assert c.form == "drop"
        mk = drop_mask(c.B * c.T, c.Co, SEED, by_row=True).reshape(c.B, c.T, c.Co)
    act, anti = op_args(c)
    y, pre = emu_conv(x, w_t, bias, res, mk, c.K, c.dil, c.lead, act, bool(anti), model or (c.prec if c.kernel == "conv" else "fp32"),
                      amax, plant)
    return {"y": y, "pre": pre} if c.form == "pre" else {"y": y}


@functools.lru_cache(maxsize=None)
def _op_emulated(key, kernel, prec):
    c = Op("", kernel, *key[:7], key[7], prec)
    out, ref = op_emulate(c), _op_data(key)["ref"]
    return {n: rel_err(out[n], ref[n]) for n in ref}


def op_emulated(c):
    return _op_emulated(_op_key(c), c.kernel, c.prec if c.kernel == "conv" else "")


# ================================================================================================= weight-gradient cases
@functools.lru_cache(maxsize=None)
def _wg_data(key):
    B, T, Ci, Co, K, dil, lead = key
    rs = _rs(B, T, Ci, Co, K, dil, lead, 5)
    dy, x = rs.standard_normal((B, T, Co)).astype(_F), rs.standard_normal((B, T, Ci)).astype(_F)
    ref = wgrad_ref(dy.astype(np.float64), x.astype(np.float64), K, dil, lead)
    n_thr = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        w = torch.zeros(Co, Ci, K, requires_grad=True)
        halo = (K - 1) * dil
        out = F.conv1d(F.pad(torch.from_numpy(x).permute(0, 2, 1), (halo - lead, lead)), w, None, dilation=dil)
        g, = torch.autograd.grad(out, w, torch.from_numpy(dy).permute(0, 2, 1))
        yard = g.permute(2, 0, 1).double().numpy()
    finally:
        torch.set_num_threads(n_thr)
    return dict(dy=dy, x=x, ref=ref, yard=yard)


def wg_data(c):
    return _wg_data((c.B, c.T, c.Ci, c.Co, c.K, c.dil, c.lead))


@functools.lru_cache(maxsize=None)
def wg_emulated(c):
    d = wg_data(c)
    return emu_wgrad(d["dy"], d["x"], c.K, c.dil, c.lead, c.prec)


def check_taps(got, c, quiet=False):
    """got [K][Co][Ci] of a weight-gradient case -> (worst ratio, its tap, failures): a tap that is identically zero in the reference must
    be identically zero, every other tap is held to BOUND max(E32, E_emu, 2^-24) of its own maximum"""
    d, emu = wg_data(c), wg_emulated(c)
    worst, fails = (0.0, ""), []
    for j in range(c.K):
        name = "dw_t[%d]" % j
        if not d["ref"][j].any():
            assert wgrad_route(c.B, c.T, c.Ci, c.Co, c.K, c.dil, c.lead, c.prec, j) is None
            if np.asarray(got[j]).any() or not np.isfinite(got[j]).all():
                fails.append("%s: must be identically zero" % name)
            continue
        yard = max(rel_err(d["yard"][j], d["ref"][j]), rel_err(emu[j], d["ref"][j]), FLOOR)
        ratio = rel_err(got[j], d["ref"][j]) / yard
        worst = max(worst, (ratio, name))
        if not ratio <= BOUND:
            fails.append("%s: %.2f x the yardstick %.3g (bound %g)" % (name, ratio, yard, BOUND))
    if not quiet:
        print("%-24s worst %6.2f x  %s" % (case_id(c), worst[0], worst[1]))
    return worst[0], worst[1], fails


def check_op(got, c, quiet=False, e_emu=None):
    """got: name -> array of an operator-level case -> (worst ratio, its tensor, failures)"""
    d, e_emu = op_data(c), (op_emulated(c) if e_emu is None else e_emu)
    worst, fails = (0.0, ""), []
    for n, ref in d["ref"].items():
        yard = max(d["e32"][n], e_emu[n], FLOOR)
        ratio = rel_err(got[n], ref) / yard
        worst = max(worst, (ratio, n))
        if not ratio <= BOUND:
            fails.append("%s: %.2f x the yardstick %.3g (bound %g)" % (n, ratio, yard, BOUND))
    if not quiet:
        print("%-24s worst %6.2f x  %s" % (case_id(c), worst[0], worst[1]))
    return worst[0], worst[1], fails


# ================================================================================================= block-level cases
def levels(c):
    return [(c.Cin if i == 0 else c.widths[i - 1], w, 2 ** i) for i, w in enumerate(c.widths)]


def block_seeds(i):
    return (0x9E3779B97F4A7C15 ^ (2 * i + 1) * 0x1000193) & (2 ** 63 - 1), (0xC2B2AE3D27D4EB4F ^ (2 * i + 2) * 0x1000193) & (2 ** 63 - 1)


def tensor_names(c):
    names = ["y", "dx"]
    for i, (ci, co, _) in enumerate(levels(c)):
        names += ["network.%d.%s" % (i, k) for k in ("conv1.weight_v", "conv1.weight_g", "conv1.bias", "conv2.weight_v", "conv2.weight_g",
                                                     "conv2.bias")]
        if ci != co:
            names += ["network.%d.downsample.weight" % i, "network.%d.downsample.bias" % i]
    return names


def inner_names(c):
    return ["network.%d.%s" % (i, k) for i in range(len(c.widths)) for k in ("h1", "ds", "da2", "da1")]


def _cf(a):
    return np.ascontiguousarray(np.swapaxes(a, 1, 2))          # [B,T,C] <-> [B,C,T]


def draw(c, seed):
    """-> (p name -> fp32 array with models.tcn's names, x [B,T,Cin], ct [B,T,Cout], masks per level or None)"""
    rs = _rs(c.Cin, c.K, c.B, c.T, len(c.widths), 1000 * seed + 17)
    B, T, K = c.B, c.T, c.K
    sign = lambda n: rs.choice([-1.0, 1.0], n)
    off = lambda a, sg: (-a.mean(axis=(0, 2)) + 3.0 * np.maximum(a.std(axis=(0, 2)), 1e-30) * sg).astype(_F)
    x = rs.standard_normal((B, T, c.Cin))
    if c.Cin == c.widths[0]:
        x = x + 3.0 * sign(c.Cin)
    if c.stats == "small":
        x = x * 2.0 ** -20
    elif c.stats == "decades":
        x = x * 10.0 ** rs.uniform(-4, 0, c.Cin)
    x = x.astype(_F)
    masks = None
    if c.train:
        masks = [tuple(_cf(drop_mask(B * T, co, s).reshape(B, T, co)) for s in block_seeds(i)) for i, (_, co, _) in enumerate(levels(c))]
    p, cur = {}, _cf(x.astype(np.float64))
    for i, (ci, co, dil) in enumerate(levels(c)):
        pre = "network.%d." % i
        m = (1.0, 1.0) if masks is None else masks[i]
        h = cur
        for k, cin in (("conv1.", ci), ("conv2.", co)):
            v = (rs.standard_normal((co, cin, K)) / np.sqrt(cin * K)).astype(_F)
            g = (np.sqrt((v.astype(np.float64) ** 2).sum(axis=(1, 2), keepdims=True)) * rs.uniform(0.5, 1.5, (co, 1, 1))).astype(_F)
            w, _ = O.weight_norm_fwd(v.astype(np.float64), g.astype(np.float64))
            a = O.causal_conv1d_fwd(h, w, None, dil)
            sg = sign(co)
            if k == "conv2." and ci == co and i > 0:
                # an identity residual that is a ReLU output: s = h2 + res >= 0, and the output ReLU closes only where both vanish -- the
                # channels the residual leaves (mostly) at zero get the negative offset, the others the positive one more often than not
                sg = np.where((cur > 0).mean(axis=(0, 2)) < 0.5, -1.0, np.where(rs.uniform(size=co) < 0.7, 1.0, -1.0))
            b = off(a, sg)
            p[pre + k + "weight_v"], p[pre + k + "weight_g"], p[pre + k + "bias"] = v, g, b
            h = np.maximum(a + b.astype(np.float64)[None, :, None], 0) * m[0 if k == "conv1." else 1]
        if ci != co:
            wd = (rs.standard_normal((co, ci, 1)) / np.sqrt(ci)).astype(_F)
            r = O.causal_conv1d_fwd(cur, wd.astype(np.float64), None, 1)
            p[pre + "downsample.weight"], p[pre + "downsample.bias"] = wd, off(r, sign(co))
        cur, _ = O.temporal_block_fwd(cur, {n: t.astype(np.float64) for n, t in p.items()}, pre, dil, None if masks is None else masks[i])
    ct = rs.standard_normal((B, T, c.widths[-1]))
    if c.stats == "small":
        ct = ct * 2.0 ** 12
    return p, x, ct.astype(_F), masks


def reference(c, p, x, ct, masks):
    """oracle.m3t_oracle block by block -> (tensors name -> float64 channels-last, clearance: per ReLU (in-margin count, positive
    fraction))"""
    p64 = {n: t.astype(np.float64) for n, t in p.items()}
    cur, caches = _cf(x.astype(np.float64)), []
    for i, (ci, co, dil) in enumerate(levels(c)):
        cur, cache = O.temporal_block_fwd(cur, p64, "network.%d." % i, dil, None if masks is None else masks[i])
        caches.append(cache)
    res = {"y": _cf(cur)}
    dy, clear = _cf(ct.astype(np.float64)), []
    for i in range(len(caches) - 1, -1, -1):
        pre, (ci, co, dil) = "network.%d." % i, levels(c)[i]
        xin, w1, n1, w2, n2, a1, h1, a2, s, has_ds, mk = caches[i]
        m1, m2 = (1.0, 1.0) if mk is None else mk
        ds = dy * (s > 0)
        da2 = ds * m2 * (a2 > 0)
        res[pre + "h1"], res[pre + "ds"], res[pre + "da2"] = _cf(h1), _cf(ds), _cf(da2)
        dy_in, g = O.temporal_block_bwd(dy, caches[i], p64, pre, dil)
        res[pre + "da1"] = _cf(O.causal_conv1d_bwd(da2, h1, w2, dil)[0] * m1 * (a1 > 0))
        res.update(g)
        # the clearance of this block's three ReLUs
        bias = lambda k: np.abs(p64[pre + k + "bias"])[None, :, None]
        A1 = O.causal_conv1d_fwd(np.abs(xin), np.abs(w1), None, dil) + bias("conv1.")
        A2 = O.causal_conv1d_fwd(np.abs(h1), np.abs(w2), None, dil) + bias("conv2.")
        rs_ = s - np.maximum(a2, 0) * m2
        As = np.where(a2 > 0, A2 * m2, 0.0) + np.abs(rs_)
        for nm, a, A in (("a1", a1, A1), ("a2", a2, A2), ("s", s, As)):
            clear.append((pre + nm, int((np.abs(a) < MARGIN * A).sum()), float((a > 0).mean())))
        dy = dy_in
    res["dx"] = _cf(dy)
    for n in list(res):
        if n.endswith("weight_g"):
            res[n] = res[n].reshape(-1, 1, 1)
    return res, clear[::-1]


def is_clear(clear):
    return all(n_in == 0 and 0.25 <= pos <= 0.75 for _, n_in, pos in clear)


def draw_clear(c, tries=8):
    """the first of `tries` consecutive seeds whose float64 reference is clear of ReLU flips and balanced -> (inputs, reference, clearance, seed)"""
    for seed in range(tries):
        inp = draw(c, seed)
        ref, clear = reference(c, *inp)
        if is_clear(clear):
            return inp, ref, clear, seed
    raise AssertionError("%s: no draw clear of ReLU flips among %d seeds: %s" % (c.id, tries, clear))


def torch_net(c, p, x, ct, masks, dtype=torch.float32):
    """the literal reference composition in torch on the CPU, one thread -> tensor_names + inner_names as float64 channels-last numpy"""
    n_thr = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        xin = t(_cf(x)).requires_grad_(True)
        cur, mods, keep, T = xin, [], {}, c.T
        for i, (ci, co, dil) in enumerate(levels(c)):
            pre = "network.%d." % i
            convs = []
            for k, cin in (("conv1.", ci), ("conv2.", co)):
                m = torch.nn.utils.weight_norm(torch.nn.Conv1d(cin, co, c.K, padding=(c.K - 1) * dil, dilation=dil)).to(dtype)
                with torch.no_grad():
                    m.weight_g.copy_(t(p[pre + k + "weight_g"])); m.weight_v.copy_(t(p[pre + k + "weight_v"])); m.bias.copy_(t(p[pre + k + "bias"]))
                convs.append(m)
                mods += [(pre + k + "weight_v", m.weight_v), (pre + k + "weight_g", m.weight_g), (pre + k + "bias", m.bias)]
            m1, m2 = (1.0, 1.0) if masks is None else (t(masks[i][0]), t(masks[i][1]))
            a1 = convs[0](cur)[:, :, :T]
            h1 = torch.relu(a1) * m1
            a2 = convs[1](h1)[:, :, :T]
            h2 = torch.relu(a2) * m2
            if ci != co:
                dsm = torch.nn.Conv1d(ci, co, 1).to(dtype)
                with torch.no_grad():
                    dsm.weight.copy_(t(p[pre + "downsample.weight"])); dsm.bias.copy_(t(p[pre + "downsample.bias"]))
                mods += [(pre + "downsample.weight", dsm.weight), (pre + "downsample.bias", dsm.bias)]
                r = dsm(cur)
            else:
                r = cur
            s = h2 + r
            for nm, v in (("a1", a1), ("a2", a2), ("s", s)):
                v.retain_grad()
                keep[pre + nm] = v
            keep[pre + "h1"] = h1
            cur = torch.relu(s)
        (cur * t(_cf(ct))).sum().backward()
        f = lambda v: v.detach().double().numpy()
        out = {"y": _cf(f(cur)), "dx": _cf(f(xin.grad))}
        out.update({n: f(v.grad) for n, v in mods})
        for i in range(len(c.widths)):
            pre = "network.%d." % i
            out[pre + "h1"] = _cf(f(keep[pre + "h1"]))
            out[pre + "ds"], out[pre + "da2"], out[pre + "da1"] = (_cf(f(keep[pre + k].grad)) for k in ("s", "a2", "a1"))
        return out
    finally:
        torch.set_num_threads(n_thr)


def emulate(c, p, x, ct, masks, plant=""):
    """_TemporalBlock.forward / backward of m3t/ops.py block by block in numpy float32 -> tensor_names + inner_names"""
    B, T, K = c.B, c.T, c.K
    cur, saved = x.astype(_F), []
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, _F)
    for i, (ci, co, dil) in enumerate(levels(c)):
        pre = "network.%d." % i
        m1, m2 = (None, None) if masks is None else (f32(_cf(masks[i][0])), f32(_cf(masks[i][1])))
        w1t, n1 = emu_weight_norm(p[pre + "conv1.weight_v"], p[pre + "conv1.weight_g"])
        w2t, n2 = emu_weight_norm(p[pre + "conv2.weight_v"], p[pre + "conv2.weight_g"])
        h1, _ = emu_conv(cur, w1t, p[pre + "conv1.bias"], None, m1, K, dil, 0, 1, False, conv_model(B, T, ci, co, c.prec), plant=plant)
        if ci != co:
            wd = p[pre + "downsample.weight"][:, :, 0]
            res = (product(cur.reshape(B * T, ci), wd.T, gemm_route(B * T, co, ci, c.prec)) + p[pre + "downsample.bias"]).astype(_F).reshape(B, T, co)
        else:
            wd, res = None, cur
        y, a2 = emu_conv(h1, w2t, p[pre + "conv2.bias"], res, m2, K, dil, 0, 2, False, conv_model(B, T, co, co, c.prec), plant=plant)
        saved.append((cur, w1t, n1, w2t, n2, h1, a2, y, m1, m2, wd))
        cur = y
    out = {"y": cur}
    dy = ct.astype(_F)
    one = _F(1)
    for i in range(len(saved) - 1, -1, -1):
        pre, (ci, co, dil) = "network.%d." % i, levels(c)[i]
        xin, w1t, n1, w2t, n2, h1, a2, y, m1, m2, wd = saved[i]
        ds = np.where(y > 0, dy, _F(0))
        da2 = np.where(a2 > 0, (ds * (one if m2 is None else m2)).astype(_F), _F(0))
        dh1, _ = emu_conv(da2, w2t, None, None, None, K, dil, 0, 0, True, conv_model(B, T, co, co, c.prec))
        da1 = np.where(h1 > 0, (dh1 * (one if m1 is None else m1)).astype(_F), _F(0))
        dw2t, dw1t = emu_wgrad(da2, h1, K, dil, 0, c.prec), emu_wgrad(da1, xin, K, dil, 0, c.prec)
        out[pre + "conv1.bias"] = da1.reshape(B * T, co).sum(0, dtype=_F)
        out[pre + "conv2.bias"] = da2.reshape(B * T, co).sum(0, dtype=_F)
        out[pre + "conv1.weight_v"], out[pre + "conv1.weight_g"] = emu_weight_norm_bwd(dw1t, p[pre + "conv1.weight_v"], p[pre + "conv1.weight_g"], n1)
        out[pre + "conv2.weight_v"], out[pre + "conv2.weight_g"] = emu_weight_norm_bwd(dw2t, p[pre + "conv2.weight_v"], p[pre + "conv2.weight_g"], n2)
        dx, _ = emu_conv(da1, w1t, None, ds if wd is None else None, None, K, dil, 0, 0, True, conv_model(B, T, co, ci, c.prec))
        if wd is not None:
            dx = (dx + product(ds.reshape(B * T, co), wd, gemm_route(B * T, ci, co, c.prec)).reshape(B, T, ci)).astype(_F)
            out[pre + "downsample.weight"] = product(ds.reshape(B * T, co).T, xin.reshape(B * T, ci), gemm_route(co, ci, B * T, c.prec))[:, :, None]
            out[pre + "downsample.bias"] = ds.reshape(B * T, co).sum(0, dtype=_F)
        out[pre + "h1"], out[pre + "ds"], out[pre + "da2"], out[pre + "da1"] = h1, ds, da2, da1
        dy = dx
    out["dx"] = dy
    return out


def _blk_key(c):
    return (c.Cin, c.widths, c.K, c.B, c.T, c.train, c.stats)


@functools.lru_cache(maxsize=None)
def _blk_data(key):
    c = Blk("", *key, "")
    (p, x, ct, masks), ref, clear, seed = draw_clear(c)
    yard = torch_net(c, p, x, ct, masks)
    names = [n for n in tensor_names(c) + inner_names(c)]
    zero = {n for n in names if not ref[n].any()}
    return dict(p=p, x=x, ct=ct, masks=masks, ref=ref, clear=clear, seed=seed, zero=zero,
                e32={n: rel_err(yard[n], ref[n]) for n in names if n not in zero})


def data(c):
    """inputs, float64 reference, clearance and yardstick A of a block-level case, once per (network, input, mode, statistics)"""
    return _blk_data(_blk_key(c))


@functools.lru_cache(maxsize=None)
def emulated(c):
    d = data(c)
    out = emulate(c, d["p"], d["x"], d["ct"], d["masks"])
    return out, {n: rel_err(out[n], d["ref"][n]) for n in d["e32"]}


def limits(c):
    """tensor name -> (upper bound on rel_err, lower bound or None); see the module docstring for the `decades` class"""
    d, (_, e_emu) = data(c), emulated(c)
    out = {}
    for n in d["e32"]:
        e32 = max(d["e32"][n], FLOOR)
        if c.stats == "decades" and c.prec == "f16x3" and e_emu[n] > BOUND * e32:
            out[n] = (BOUND * e_emu[n], BOUND * e32)
        else:
            out[n] = (BOUND * max(e32, e_emu[n]), None)
    return out


def check(got, c, quiet=False):
    """got: name -> array of tensor_names(c) of some fp32 implementation -> (worst ratio in units of the yardstick, its tensor, failures)"""
    d, lim = data(c), limits(c)
    worst, fails = (0.0, ""), []
    for n in tensor_names(c):
        g = np.asarray(got[n], np.float64).reshape(d["ref"][n].shape)
        if n in d["zero"]:
            if g.any() or not np.isfinite(g).all():
                fails.append("%s: must be identically zero" % n)
            continue
        err = rel_err(g, d["ref"][n])
        hi, lo = lim[n]
        ratio = BOUND * err / hi
        worst = max(worst, (ratio, n))
        if not err <= hi:
            fails.append("%s: rel_err %.3g > %.3g (%.2f x the yardstick, bound %g)" % (n, err, hi, ratio, BOUND))
        if lo is not None and not err > lo:
            fails.append("%s: rel_err %.3g does not exceed %.3g: the normwise limit of fp16x3 is no longer reached" % (n, err, lo))
    if not quiet:
        print("%-24s worst %6.2f x  %s" % (case_id(c), worst[0], worst[1]))
    return worst[0], worst[1], fails


def close_verdict(got, ref, tol=1e-4):
    """what close() of tests/test_gpu_parity.py makes of `got`: max |got - ref| <= tol max(1, max |ref|)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.abs(got - ref).max() <= tol * max(1.0, np.abs(ref).max()))
