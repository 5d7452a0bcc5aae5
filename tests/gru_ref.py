"""Float64 reference, two fp32 yardsticks and the error bound for the bidirectional GRU scans (csrc/gru.hip, csrc/gru_solo.hip,
csrc/gru_persist.hip and its *_step.inc files) behind models.rnn.GRU(I, H, L, -1, return_h=True): no FC head, so no ReLU and no
dropout whose decisions could flip between fp32 and float64.  tests/test_gru_ref_host.py checks this file on the CPU;
tests/test_gpu_gru_fp64.py holds the kernels to it.

Every case contracts the output with a fixed `ct` and the final state with a fixed `cth` (loss = sum(y ct) + sum(h_n cth)), so h_n
and dL/dh_n are always in play.  Compared: y, h_n, dx and the eight parameter gradients of every layer: 3 + 8 L tensors.

Reference    oracle.m3t_oracle.bigru_fwd / bigru_bwd in float64 on the fp32 parameters and inputs.
Yardstick A  (E32)   stock torch.nn.GRU in float32 on the CPU, one thread: independent of the library.
Yardstick B  (E_emu) `emulate`: a numpy float32 restatement of the arithmetic of the kernel family a case reaches, written from the
             kernel text:
  * cell     gru_cell_fwd / gru_cell_bwd of csrc/gru_common.h literally: sigmoid(x) = rcp(1 + exp2(-x log2 e)),
             tanh(x) = 1 - 2 rcp(exp2(2 x log2 e) + 1), the same fmaf grouping; np.exp2 and a float32 reciprocal (both correctly
             rounded) stand in for the 1-ulp hardware units.
  * products through the model of the family (f16_scale, split_f16, split_bf16, mfma_acc of tests/test_fp16x3_model.py):
      fp32    one fp32 accumulator over 16-deep blocks (per-step kernels, solo kernels, persistent fp32-MFMA kernels);
      f16x3   forward (gru_persist_fwd6_step.inc, F16): h as two fp16 terms of 2^14 h, W_hh as two fp16 terms under one power-of-two
              scale per 16-unit slice (48 gate rows), products lo hi, hi lo, hi hi in 32-deep blocks, K dealt over eight waves as
              wfrag3h_prep_kernel deals it, the waves' sums added in order, fmaf(sum, 1 / scales, b_hh).  Backward
              (gru_persist_bwd3q_step.inc): what a cell publishes (dr, dz, dn r) as two fp16 terms under one scale per workgroup
              (16 rows x 32 units) taken from |dht| max(1, |W_hn h + b_hn| / 4); per producer pair nine products, then
              fmaf(sum, 1 / scale, acc); W_hh scaled per 16 output units;
      x6      three bf16 terms per operand, six products, smallest first (gru_persist_fwd6_step.inc, !F16; bwd6 likewise).
  * the GEMMs around the scans (input projection, dX, dW_ih, dW_hh) through `gemm_route`: csrc/gemm.hip sends only interior shapes
    (M % 128 == 0, N % 64 == 0, K % 32 == 0) to the split-product kernels of the precision in force, everything else to fp32 MFMAs.
  Not modelled: which wave owns which k in the fp32 kernels, split-K, the time-windowed input projections of deeper layers -- other
  summation orders of the same length, which the factor BOUND covers.

Metric  rel_err(got, ref) = max |got - ref| / max |ref| per tensor, never max(1, .); the reference maximum must be finite and non-zero.
Bound   rel_err(gpu) <= BOUND max(E32, E_emu, 2^-24) per tensor and case, BOUND = 4.0 (fuse_loss_ref.BOUND): a correctly rounded
        emulation against 1-ulp hardware units, and another summation order of the same length.  Not fitted to GPU output.

The stated limit of the cell math.  fast_tanh has an ABSOLUTE error of about 2e-7 (csrc/gru_common.h).  On the `small` class (inputs
and biases x 1e-3: candidate pre-activations of 1e-3) that is a relative error of 1e-4 of the hidden state, hundreds of times E32, and
it is not hidden inside the yardstick: `limits` names, from the emulation alone, the tensors the limit reaches (E_emu > BOUND
max(E32, 2^-24)).  Those are held to LIMIT_REL(case) = BOUND TANH_ABS / s, s = the smallest over the layers of max |h| of the
float64 reference -- every hidden value carries at most the absolute error TANH_ABS (h = (1 - z) n + z h': a convex combination
passes it on without growth), which is TANH_ABS / s of the layer's scale, and every compared tensor is a sum of products that are
linear in those values -- and they must EXCEED BOUND max(E32, 2^-24), so that a change of the cell math shows up.  Every other tensor of
the class is held to BOUND max(E32, 2^-24).
"""
import collections

import numpy as np
import torch

from golden.recipe import draw, fill_by_shapes
from oracle import m3t_oracle as O
from test_fp16x3_model import f16_scale, split_f16, split_bf16, bf16_rn, mfma_acc

BOUND = 4.0
FLOOR = 2.0 ** -24
TANH_ABS = 2e-7          # csrc/gru_common.h: the stated absolute error of fast_tanh
CUS = 256                # compute units of the MI355X: the persistent scans take 32-row workgroups when the 16-row grid exceeds them
_F = np.float32
LOG2E = _F(1.44269504088896341)
TWO_LOG2E = _F(2.88539008177792681)

Case = collections.namedtuple("Case", "family B T I H L switch prec stats")
# switch: "" (default) | "per_step" (ops.SCAN_PER_STEP) | "fp32" (ops.SCAN_FP32) | "wide" (ops.FORCE_WIDE_FWD)
# prec:   "f16x3" (the default precision) | "x6" (ops.precision("x6"))
# stats:  "normal" | "saturated" (inputs x 8) | "small" (inputs and biases x 1e-3) | "one_hot_time" (ct at one step, cth = 0)


def _table():
    rows = (
        # family, (B, T, I, H, L) ..., switch, precisions, shapes that also run saturated + small, shapes that also run one_hot_time
        ("generic per-step", ((37, 6, 30, 20, 2),), "", ("f16x3",), 0, ()),
        ("fragment per-step (graph)", ((5, 33, 40, 48, 2),), "", ("f16x3",), 0, ()),
        ("fragment per-step", ((33, 5, 12, 256, 1),), "per_step", ("f16x3",), 0, ()),
        ("solo", ((5, 9, 20, 128, 2), (40, 6, 16, 128, 1), (1, 2, 8, 128, 1), (21, 11, 12, 128, 2)), "", ("f16x3",), 0, ()),
        ("persistent fp32", ((32, 12, 128, 384, 1),), "", ("f16x3",), None, ()),
        ("persistent fp32", ((33, 5, 12, 256, 1),), "fp32", ("f16x3",), 0, ()),
        ("persistent fp32 (32 rows)", ((100, 3, 8, 512, 1),), "", ("f16x3",), None, ()),
        ("persistent split", ((33, 5, 12, 256, 2), (19, 23, 16, 512, 1), (5, 2, 8, 256, 1), (64, 3, 16, 512, 1)), "", ("f16x3", "x6"), 0, (1,)),
        ("persistent split, wide forward", ((48, 3, 16, 512, 1), (19, 23, 16, 512, 1)), "wide", ("f16x3",), 0, (1,)),
        ("long chain", ((2, 50, 12, 256, 1),), "", ("f16x3",), 0, (0,)),
    )
    out = []
    for family, shapes, switch, precs, extra, hot in rows:
        for prec in precs:
            for i, s in enumerate(shapes):
                out.append(Case(family, *s, switch, prec, "normal"))
                if extra == i:
                    out.append(Case(family, *s, switch, prec, "saturated"))
                    out.append(Case(family, *s, switch, prec, "small"))
                if i in hot:
                    out.append(Case(family, *s, switch, prec, "one_hot_time"))
    return tuple(out)


CASES = _table()          # ONE table, imported by both test files; every case is admitted


def case_id(c):
    return "%s-B%d-T%d-I%d-H%d-L%d-%s-%s" % (c.family.replace(" ", "_").replace(",", ""), c.B, c.T, c.I, c.H, c.L, c.prec, c.stats)


def rows32(c):
    """does the level take 32-row workgroups?  (level_shape in csrc/gru_persist.hip: the 16-row grid must fit one workgroup per CU)"""
    return 2 * ((c.B + 15) // 16) * (c.H // 16) > CUS


def scan_model(c):
    """the product model of the recurrent products of the family the case reaches (persist_fwd_uses_x6 / persist_bwd_uses_x6)"""
    if c.switch in ("per_step", "fp32") or c.H % 128 != 0 or c.H in (128, 384) or rows32(c):
        return "fp32"
    return c.prec


def gemm_route(M, N, K, prec, seg_len=0):
    """plan_gemm in csrc/gemm.hip: only interior shapes reach the split-product kernels"""
    interior = M % 128 == 0 and N % 64 == 0 and K > 0 and (K % 32 == 0 or seg_len >= 32) and (seg_len == 0 or seg_len >= 32)
    return prec if interior else "fp32"


def tensor_names(L):
    names = ["y", "h_n", "dx"]
    for l in range(L):
        for sfx in ("", "_reverse"):
            for kind in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                names.append("gru.%s_l%d%s" % (kind, l, sfx))
    assert len(names) == 3 + 8 * L
    return names


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    top = float(np.abs(ref).max())
    assert top > 0.0 and np.isfinite(top), "the reference is all zero or not finite: the metric would be blind"
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.abs(got - ref).max()) / top


# ================================================================================================= inputs, reference, yardstick A
def param_shapes(I, H, L):
    sh = {}
    for l in range(L):
        for sfx in ("", "_reverse"):
            t = "l%d%s" % (l, sfx)
            sh["gru.weight_ih_" + t] = (3 * H, I if l == 0 else 2 * H)
            sh["gru.weight_hh_" + t] = (3 * H, H)
            sh["gru.bias_ih_" + t] = (3 * H,)
            sh["gru.bias_hh_" + t] = (3 * H,)
    return sh


def make_inputs(c):
    """-> (params name -> fp32 array (models.rnn.GRU's names), x [B,T,I], ct [B,T,2H], cth [2L,B,H])"""
    rs = np.random.RandomState((7 * c.B + 131 * c.T + 17 * c.I + 3 * c.H + c.L) % 2 ** 31)
    p = fill_by_shapes(param_shapes(c.I, c.H, c.L), 91)
    x, ct, cth = draw(rs, (c.B, c.T, c.I)), draw(rs, (c.B, c.T, 2 * c.H)), draw(rs, (2 * c.L, c.B, c.H))
    if c.stats == "saturated":
        x = x * _F(8)
    elif c.stats == "small":
        x = x * _F(1e-3)
        p = {n: (v * _F(1e-3) if ".bias_" in n else v) for n, v in p.items()}
    elif c.stats == "one_hot_time":
        keep = c.T // 3
        ct[:, :keep] = 0
        ct[:, keep + 1:] = 0
        cth[:] = 0
    else:
        assert c.stats == "normal", c.stats
    return p, x, ct, cth


def reference(p, x, ct, cth, L):
    p64 = {n: v.astype(np.float64) for n, v in p.items()}
    y, hn, caches = O.bigru_fwd(x.astype(np.float64), p64, L)
    dx, g = O.bigru_bwd(ct.astype(np.float64), caches, p64, L, dh_n=cth.astype(np.float64))
    res = {"y": y, "h_n": hn, "dx": dx}
    res.update(g)
    scale = min(float(np.abs(caches[2 * l + d][1]).max()) for l in range(L) for d in (0, 1))
    return res, scale


def torch_gru(p, x, ct, cth, L, dtype=torch.float32):
    """stock torch.nn.GRU on the CPU in `dtype`, one thread -> the 3 + 8 L tensors as float64 numpy"""
    n_thr = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        H = p["gru.weight_hh_l0"].shape[1]
        m = torch.nn.GRU(x.shape[-1], H, L, batch_first=True, bidirectional=True).to(dtype)
        with torch.no_grad():
            for n, t in m.named_parameters():
                t.copy_(torch.from_numpy(p["gru." + n]).to(dtype))
        xt = torch.from_numpy(x).to(dtype).requires_grad_(True)
        y, hn = m(xt)
        ((y * torch.from_numpy(ct).to(dtype)).sum() + (hn * torch.from_numpy(cth).to(dtype)).sum()).backward()
        res = {"y": y, "h_n": hn, "dx": xt.grad}
        res.update({"gru." + n: t.grad for n, t in m.named_parameters()})
        return {n: t.detach().double().numpy() for n, t in res.items()}
    finally:
        torch.set_num_threads(n_thr)


# ================================================================================================= yardstick B: the products
def _amax(a, unit):
    return _F(1.0) if unit else _F(np.abs(a).max())


def product(A, Bm, model, unit_a=False, unit_b=False):
    """A [M,K] @ Bm [K,N] in float32 as the GEMM kernels of `model` form it.  unit_*: the operand is a GRU output, |.| <= 1, and
    takes the constant magnitude slot (m3t.ops.amax_one)"""
    A, Bm = np.ascontiguousarray(A, _F), np.ascontiguousarray(Bm, _F)
    if model == "fp32":
        return mfma_acc([(A, Bm)], 16)
    if model == "f16x3":
        sa, ia = f16_scale(_amax(A, unit_a))
        sb, ib = f16_scale(_amax(Bm, unit_b))
        ah, al = split_f16(A, sa)
        bh, bl = split_f16(Bm, sb)
        return (mfma_acc([(al, bh), (ah, bl), (ah, bh)], 32) * ia * ib).astype(_F)
    assert model == "x6", model
    a, b = split_bf16(A), split_bf16(Bm)
    return mfma_acc([(a[2], b[0]), (a[1], b[1]), (a[0], b[2]), (a[1], b[0]), (a[0], b[1]), (a[0], b[0])], 32)


def _wave_k(H, w):
    """the k (hidden units of h_{t-1}) wave w of eight multiplies, as 32-deep blocks (wfrag3h_prep_kernel: unit = 16 (w + 8 (2 s + q / 2)) ...)"""
    if H % 256 != 0:
        return [np.arange(k0, min(k0 + 32, H)) for k0 in range(w * (H // 8), (w + 1) * (H // 8), 32)]
    return [np.concatenate([np.arange(16 * (w + 16 * s), 16 * (w + 16 * s) + 16), np.arange(16 * (w + 16 * s + 8), 16 * (w + 16 * s + 8) + 16)])
            for s in range(H // 256)]


def _acc(acc, A, Bm):
    return (acc + A.astype(np.float64) @ Bm).astype(_F)


class _FwdProduct:
    """gh = h W_hh^T + b_hh of one direction, by model"""

    def __init__(self, w_hh, b_hh, model, drop_lo=False):
        self.model, self.b, self.H = model, b_hh.astype(_F), w_hh.shape[1]
        H = self.H
        if model == "fp32":
            self.wt = np.ascontiguousarray(w_hh.T, _F)
        elif model == "f16x3":
            sc, inv = np.zeros(3 * H, _F), np.zeros(3 * H, _F)
            for ub in range(H // 16):
                rows = np.concatenate([np.arange(g * H + ub * 16, g * H + ub * 16 + 16) for g in range(3)])
                s, i = f16_scale(np.abs(w_hh[rows]).max())
                sc[rows], inv[rows] = s, _F(i * _F(2.0 ** -14))
            ws = (w_hh * sc[:, None]).astype(_F)
            hi = ws.astype(np.float16).astype(_F)
            lo = (ws - hi).astype(_F).astype(np.float16).astype(_F)
            if drop_lo:
                lo = np.zeros_like(lo)
            self.hi, self.lo, self.winv = hi.T.astype(np.float64), lo.T.astype(np.float64), inv
        else:
            self.terms = [t.T.astype(np.float64) for t in split_bf16(np.ascontiguousarray(w_hh, _F))]

    def __call__(self, h):
        B, H = h.shape
        if self.model == "fp32":
            return (mfma_acc([(h, self.wt)], 16) + self.b).astype(_F)
        if self.model == "f16x3":
            hs = (h * _F(16384.0)).astype(_F)
            f1 = hs.astype(np.float16).astype(_F)
            f2 = (hs - f1).astype(_F).astype(np.float16).astype(_F)
            tot = np.zeros((B, 3 * H), _F)
            for w in range(8):
                acc = np.zeros((B, 3 * H), _F)
                for k in _wave_k(H, w):
                    acc = _acc(acc, f2[:, k], self.hi[k])
                    acc = _acc(acc, f1[:, k], self.lo[k])
                    acc = _acc(acc, f1[:, k], self.hi[k])
                tot = (tot + acc).astype(_F)
            return (tot.astype(np.float64) * self.winv + self.b).astype(_F)              # fmaf(sum, winv, b)
        a1, a2, a3 = split_bf16(np.ascontiguousarray(h, _F))
        b1, b2, b3 = self.terms
        tot = np.broadcast_to(self.b, (B, 3 * H)).astype(_F)
        for w in range(8):
            acc = np.zeros((B, 3 * H), _F)
            for k in _wave_k(H, w):
                for A, W in ((a3, b1), (a2, b2), (a1, b3), (a2, b1), (a1, b2), (a1, b1)):
                    acc = _acc(acc, A[:, k], W[k])
            tot = (tot + acc).astype(_F)
        return tot


class _BwdProduct:
    """mm = dgh W_hh of one direction, by model; dgh = (dr, dz, dn r) [B, 3H]"""

    def __init__(self, w_hh, model):
        self.model, self.H = model, w_hh.shape[1]
        H = self.H
        w = np.ascontiguousarray(w_hh, _F)
        if model == "fp32":
            self.w = w
        elif model == "f16x3":
            sc, inv = np.zeros(H, _F), np.zeros(H, _F)
            for ub in range(H // 16):
                s, i = f16_scale(np.abs(w[:, ub * 16:ub * 16 + 16]).max())
                sc[ub * 16:ub * 16 + 16], inv[ub * 16:ub * 16 + 16] = s, i
            ws = (w * sc[None, :]).astype(_F)
            hi = ws.astype(np.float16).astype(_F)
            lo = (ws - hi).astype(_F).astype(np.float16).astype(_F)
            self.hi, self.lo, self.winv = hi.astype(np.float64), lo.astype(np.float64), inv
        else:
            self.terms = [t.astype(np.float64) for t in split_bf16(w)]

    def __call__(self, dgh, bnd):
        """bnd [B, H]: |dht| max(1, |hn| / 4) of the cells that produced dgh (the producers' scale bound)"""
        B, H = dgh.shape[0], self.H
        if self.model == "fp32":
            return mfma_acc([(dgh, self.w)], 16)
        if self.model == "x6":
            a, b = split_bf16(np.ascontiguousarray(dgh, _F)), self.terms
            acc = np.zeros((B, H), _F)
            for k0 in range(0, 3 * H, 32):
                k = slice(k0, k0 + 32)
                for A, W in ((a[2], b[0]), (a[1], b[1]), (a[0], b[2]), (a[1], b[0]), (a[0], b[1]), (a[0], b[0])):
                    acc = _acc(acc, A[:, k], W[k])
            return acc
        psc, pinv = np.zeros((B, H // 32), _F), np.zeros((B, H // 32), _F)
        for rb in range(0, B, 16):
            for p in range(H // 32):
                s, _ = f16_scale(np.abs(bnd[rb:rb + 16, p * 32:p * 32 + 32]).max())
                psc[rb:rb + 16, p] = s
                pinv[rb:rb + 16, p] = np.uint32((254 - (int(s.view(np.uint32)) >> 23)) << 23).view(_F)     # as the consumer rebuilds it from the exponent byte
        tot = np.zeros((B, H), _F)
        for w in range(8):
            acc = np.zeros((B, H), _F)
            for p in range(w, H // 32, 8):
                at = np.zeros((B, H), _F)
                for g in range(3):
                    k = slice(g * H + p * 32, g * H + p * 32 + 32)
                    xs = (dgh[:, k] * psc[:, p:p + 1]).astype(_F)
                    ah = xs.astype(np.float16).astype(_F)
                    al = (xs - ah).astype(_F).astype(np.float16).astype(_F)
                    at = _acc(at, al, self.hi[k])
                    at = _acc(at, ah, self.lo[k])
                    at = _acc(at, ah, self.hi[k])
                acc = (at.astype(np.float64) * pinv[:, p:p + 1] + acc).astype(_F)       # fmaf(at, pinv, acc)
            tot = (tot + (acc * self.winv).astype(_F)).astype(_F)
        return tot


# ================================================================================================= yardstick B: the cell
def fast_sigmoid(x):
    with np.errstate(over="ignore"):
        return (_F(1) / (_F(1) + np.exp2((-LOG2E * x).astype(_F)).astype(_F)).astype(_F)).astype(_F)


def fast_tanh(x):
    with np.errstate(over="ignore"):
        return (_F(1) - (_F(2) * (_F(1) / (np.exp2((TWO_LOG2E * x).astype(_F)).astype(_F) + _F(1)).astype(_F)).astype(_F)).astype(_F)).astype(_F)


def _fma(a, b, c):
    return (a.astype(np.float64) * b + c).astype(_F)


def cell_fwd(xr, xz, xn, hr, hz, hn, hprev):
    r = fast_sigmoid((xr + hr).astype(_F))
    z = fast_sigmoid((xz + hz).astype(_F))
    n = fast_tanh(_fma(r, hn, xn))
    h = _fma(z, (hprev - n).astype(_F), n)
    return r, z, n, h


def cell_bwd(dout, dh_next, z_next, mm, has_next, gr, gz, gn, ghn, hprev):
    carry = _fma(dh_next, z_next, mm) if has_next else dh_next
    dht = (dout + carry).astype(_F)
    one = _F(1)
    dn = ((dht * (one - gz)).astype(_F) * _fma(-gn, gn, np.ones_like(gn))).astype(_F)
    dz = (((dht * (hprev - gn).astype(_F)).astype(_F) * gz).astype(_F) * (one - gz).astype(_F)).astype(_F)
    dr = (((dn * ghn).astype(_F) * gr).astype(_F) * (one - gr).astype(_F)).astype(_F)
    dnr = (dn * gr).astype(_F)
    return dht, dr, dz, dn, dnr


# ================================================================================================= yardstick B: the scans
PLANTS = ("", "a", "b", "c", "d", "e", "f")
PLANT_TEXT = {
    "a": "the low fp16 term of W_hh is dropped (forward, fp16x3)",
    "b": "h is rounded to bf16 once per step",
    "c": "b_hn is added outside r * (...)",
    "d": "the last time step is left out of db_hh",
    "e": "dh_n is ignored for the reverse direction",
    "f": "z_next is taken from the wrong neighbour at a clip's first step",
}


def _scan_fwd(xp, w_hh, b_hh, reverse, model, plant):
    B, T, H = xp.shape[0], xp.shape[1], w_hh.shape[1]
    prod = _FwdProduct(w_hh, b_hh, model, drop_lo=(plant == "a"))
    out, gates = np.zeros((B, T, H), _F), np.zeros((B, T, 4, H), _F)
    h = np.zeros((B, H), _F)
    b = b_hh.astype(_F)
    for step in range(T):
        t = T - 1 - step if reverse else step
        gh = np.broadcast_to(b, (B, 3 * H)) if step == 0 else prod(h)
        hr, hz, hn = gh[:, :H], gh[:, H:2 * H], gh[:, 2 * H:]
        xr, xz, xn = xp[:, t, :H], xp[:, t, H:2 * H], xp[:, t, 2 * H:]
        if plant == "c":
            bn = b[2 * H:]
            r, z, n, hnew = cell_fwd(xr, xz, (xn + bn).astype(_F), hr, hz, (hn - bn).astype(_F), h)
        else:
            r, z, n, hnew = cell_fwd(xr, xz, xn, hr, hz, hn, h)
        if plant == "b":
            hnew = bf16_rn(np.ascontiguousarray(hnew))
        h = hnew
        out[:, t] = h
        gates[:, t, 0], gates[:, t, 1], gates[:, t, 2], gates[:, t, 3] = r, z, n, hn
    return out, h, gates


def _scan_bwd(dout, dhn, out, gates, w_hh, reverse, model, plant):
    """-> dgx [B,T,3H] (dr, dz, dn), dgh [B,T,3H] (dr, dz, dn r), db_ih [3H], db_hh [3H]"""
    B, T, H = out.shape
    prod = _BwdProduct(w_hh, model)
    dgx, dgh = np.zeros((B, T, 3 * H), _F), np.zeros((B, T, 3 * H), _F)
    sb = np.zeros((4, B, H), _F)                                # per-thread sums over the steps: dr, dz, dn, dn r
    sb_hh = np.zeros((3, B, H), _F)
    dh_carry = np.zeros((B, H), _F) if (plant == "e" and reverse) else dhn.astype(_F)
    z_next, prev_dgh, prev_bnd = np.zeros((B, H), _F), None, None
    for step in range(T):
        t = step if reverse else T - 1 - step                   # the forward scan's last step first
        tp = t + 1 if reverse else t - 1                        # the forward scan's previous step
        hprev = out[:, tp] if 0 <= tp < T else np.zeros((B, H), _F)
        gr, gz, gn, ghn = (gates[:, t, k] for k in range(4))
        has_next = step > 0
        mm = prod(prev_dgh, prev_bnd) if has_next else np.zeros((B, H), _F)
        zn = z_next
        if plant == "f" and step == T - 1 and has_next:
            zn = gz                                             # this step's own gate instead of the gate of the step processed before
        dht, dr, dz, dn, dnr = cell_bwd(dout[:, t], dh_carry, zn, mm, has_next, gr, gz, gn, ghn, hprev)
        dgx[:, t] = np.concatenate([dr, dz, dn], 1)
        dgh[:, t] = np.concatenate([dr, dz, dnr], 1)
        prev_dgh = dgh[:, t]
        prev_bnd = (np.abs(dht) * np.maximum(_F(1), _F(0.25) * np.abs(ghn))).astype(_F)
        dh_carry, z_next = dht, gz
        for k, v in enumerate((dr, dz, dn, dnr)):
            sb[k] = (sb[k] + v).astype(_F)
        if not (plant == "d" and t == T - 1):
            for k, v in enumerate((dr, dz, dnr)):
                sb_hh[k] = (sb_hh[k] + v).astype(_F)

    def rows(v):                                                # the batch rows in order, fp32
        acc = np.zeros(v.shape[1:], _F)
        for r_ in v:
            acc = (acc + r_).astype(_F)
        return acc

    db_ih = np.concatenate([rows(sb[0]), rows(sb[1]), rows(sb[2])])
    db_hh = np.concatenate([rows(sb_hh[0]), rows(sb_hh[1]), rows(sb_hh[2])])
    return dgx, dgh, db_ih, db_hh


def emulate(c, p, x, ct, cth, plant=""):
    """the 3 + 8 L tensors as the kernel family of case `c` computes them, in numpy float32.  plant: one of PLANTS (a planted error)"""
    assert plant in PLANTS
    B, T, H, L = c.B, c.T, c.H, c.L
    sm = scan_model(c)
    inp, saved, hns = x.astype(_F), [], []
    for l in range(L):
        I = inp.shape[-1]
        outs = []
        for d in (0, 1):
            s = O._sfx(l, d)
            w_ih, w_hh = p["gru.weight_ih_" + s], p["gru.weight_hh_" + s]
            route = gemm_route(B * T, 3 * H, I, c.prec)
            xp = (product(inp.reshape(B * T, I), w_ih.T, route, unit_a=l > 0) + p["gru.bias_ih_" + s]).astype(_F).reshape(B, T, 3 * H)
            out, hn, gates = _scan_fwd(xp, w_hh, p["gru.bias_hh_" + s], bool(d), sm, plant)
            outs.append(out)
            hns.append(hn)
            saved.append((inp, out, gates))
        inp = np.concatenate(outs, -1)
    res = {"y": inp, "h_n": np.stack(hns, 0)}
    d_in = ct.astype(_F)
    for l in range(L - 1, -1, -1):
        dx_sum = None
        for d in (0, 1):
            s = O._sfx(l, d)
            w_ih, w_hh = p["gru.weight_ih_" + s], p["gru.weight_hh_" + s]
            xin, out, gates = saved[2 * l + d]
            I = xin.shape[-1]
            dgx, dgh, db_ih, db_hh = _scan_bwd(d_in[..., d * H:(d + 1) * H], cth[2 * l + d], out, gates, w_hh, bool(d), sm, plant)
            dx = product(dgx.reshape(B * T, 3 * H), w_ih, gemm_route(B * T, I, 3 * H, c.prec))
            dx_sum = dx if dx_sum is None else (dx_sum + dx).astype(_F)
            res["gru.weight_ih_" + s] = product(dgx.reshape(B * T, 3 * H).T, xin.reshape(B * T, I), gemm_route(3 * H, I, B * T, c.prec),
                                                unit_b=l > 0)
            # dW_hh: the steps that have a previous hidden state, clip by clip (a segmented reduction over B (T - 1) rows)
            if d == 0:
                a, hp = dgh[:, 1:], out[:, :-1]
            else:
                a, hp = dgh[:, :-1], out[:, 1:]
            K = B * (T - 1)
            res["gru.weight_hh_" + s] = product(a.reshape(K, 3 * H).T, hp.reshape(K, H), gemm_route(3 * H, H, K, c.prec, seg_len=T - 1), unit_b=True)
            res["gru.bias_ih_" + s], res["gru.bias_hh_" + s] = db_ih, db_hh
        d_in = dx_sum.reshape(B, T, -1)
    res["dx"] = d_in
    for n, v in res.items():
        assert v.dtype == _F, (n, v.dtype)
    return res


# ================================================================================================= cached per case
_DATA, _EMU = {}, {}


def _data_key(c):
    return (c.B, c.T, c.I, c.H, c.L, c.stats)


def data(c):
    """inputs, float64 reference and yardstick A of a case, computed once per (shape, statistics) and left unchanged"""
    k = _data_key(c)
    if k not in _DATA:
        p, x, ct, cth = make_inputs(c)
        ref, scale = reference(p, x, ct, cth, c.L)
        yard = torch_gru(p, x, ct, cth, c.L)
        names = tensor_names(c.L)
        _DATA[k] = dict(p=p, x=x, ct=ct, cth=cth, ref=ref, scale=scale, e32={n: rel_err(yard[n], ref[n]) for n in names})
    return _DATA[k]


def emulated(c):
    """yardstick B of a case: its tensors and their rel_err, once per (shape, statistics, product models)"""
    k = _data_key(c) + (scan_model(c), c.prec)
    if k not in _EMU:
        d = data(c)
        out = emulate(c, d["p"], d["x"], d["ct"], d["cth"])
        _EMU[k] = (out, {n: rel_err(out[n], d["ref"][n]) for n in tensor_names(c.L)})
    return _EMU[k]


def limits(c):
    """tensor name -> (upper bound on rel_err, lower bound or None).  Ordinary: BOUND max(E32, E_emu, 2^-24).  Class `small`: the
    tensors the stated limit of fast_tanh reaches (decided from the emulation: E_emu > BOUND max(E32, 2^-24)) get
    (BOUND TANH_ABS / s, BOUND max(E32, 2^-24)); the others BOUND max(E32, 2^-24) -- see the module docstring"""
    d, (_, e_emu) = data(c), emulated(c)
    out = {}
    for n in tensor_names(c.L):
        e32 = max(d["e32"][n], FLOOR)
        if c.stats != "small":
            out[n] = (BOUND * max(e32, e_emu[n]), None)
        elif e_emu[n] > BOUND * e32:
            out[n] = (BOUND * TANH_ABS / d["scale"], BOUND * e32)
        else:
            out[n] = (BOUND * e32, None)
    return out


def check(got, c, quiet=False):
    """got: name -> array of the 3 + 8 L tensors of some fp32 implementation on case `c`.  -> (worst ratio rel_err / upper bound x
    BOUND, its tensor, failures).  The ratio is in units of the yardstick: <= BOUND passes.  failures: messages for tensors over
    their upper bound or (class `small`) not over their lower one.  Prints one line per case."""
    d, lim = data(c), limits(c)
    worst, fails, n_cmp = (0.0, ""), [], 0
    for n in tensor_names(c.L):
        err = rel_err(got[n], d["ref"][n])
        hi, lo = lim[n]
        ratio = BOUND * err / hi
        n_cmp += 1
        worst = max(worst, (ratio, n))
        if not err <= hi:
            fails.append("%s: rel_err %.3g > %.3g (%.2f x the yardstick, bound %g)" % (n, err, hi, ratio, BOUND))
        if lo is not None and not err > lo:
            fails.append("%s: rel_err %.3g does not exceed %.3g: the stated limit of fast_tanh is no longer reached" % (n, err, lo))
    assert n_cmp == 3 + 8 * c.L, (n_cmp, c.L)
    if not quiet:
        print("%-70s worst %6.2f x  %s" % (case_id(c), worst[0], worst[1]))
    return worst[0], worst[1], fails
