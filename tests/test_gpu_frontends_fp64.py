"""The visual front-ends as assembled modules against float64, element by element.

Every operator inside the stems, the per-frame ResNet, CBAM and the DenseNet is checked on its own elsewhere (test_gpu_parity.py,
test_gpu_densenet.py); the assembled modules only against the reference's gradient digests, whose bar is absolute below 1.  Here each front-end
runs in fp32 on the HIP library and, as a float64 copy, on stock torch operators on the CPU, on the same video and the same upstream gradient:
the output, the video gradient, every parameter gradient and every BatchNorm buffer must agree to a bar relative to each tensor's OWN maximum.
Part 2 checks the same gradients where training reads them -- the flat buffer of m3t.ddp.FlatGradDDP, written through gradient sinks and
weight-gradient streams -- over one and two backward passes, a weight used twice in one graph on both convolution classes, and a BatchNorm
applied twice inside ops.batch_counters().

Which case reaches which path (geometries asserted in test_the_cases_reach_the_paths_they_are_for):
  vggm_bn     channels-last stem chain (_Conv3dCL, fused BatchNorm + pooling); conv1 3 x 5 x 55 x 55 = 45 375 rows (not a multiple of 128)
  vggm_gn     planes convolutions (_Conv3dGemmWgrad) with stock GroupNorm
  split3      VA_3DVGGM_Split(split_layer=3).features: the two private towers side by side on the side stream
  resnet_v1   per-frame maps 25 -> 13 -> 7 -> 4 (odd grids: every parity class of the stride-2 data gradients); CBAM at 25 x 25 = 625 odd
              pixels takes the two-gate path, 13 x 13 the fused operator, 4 x 4 x 512 the frame-resident kernels (9 frames)
  resnet_v2*  pre-activation blocks (y + shortcut) with and without CBAM; maps 24 -> 12 -> 6 -> 3
  densenet_*  the one-operator dense stack at 20 -> 10 -> 5 -> 2 ('ap') and 28 -> 14 -> 7 -> 3 with the norm5 reorder ('fc')
The video gradient leaves the channels-last chain (its first layer has no data gradient): the cases run twice on the GPU, once with the video
gradient (compared) and once without it (the chain).
"""
import copy
import math
import time
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from golden.recipe import fill_module

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ float64 reference of CBAM
def cbam_stock_forward(self, x):
    """models.cbam.CBAM as stock operators on the module's own parameters and buffers (the float64 copy only: CBAM has no CPU path).
    Channel gate: x * sigmoid(MLP(avg-pool x) + MLP(max-pool x)); spatial gate: x * sigmoid(BatchNorm(conv5x5([max_c x, mean_c x])))."""
    l1, l2 = self.ChannelGate.mlp[1], self.ChannelGate.mlp[3]

    def mlp(v):
        return F.linear(F.relu(F.linear(v, l1.weight, l1.bias)), l2.weight, l2.bias)

    H, W = x.shape[2], x.shape[3]
    att = mlp(F.avg_pool2d(x, (H, W)).flatten(1)) + mlp(F.max_pool2d(x, (H, W)).flatten(1))
    x = x * torch.sigmoid(att)[:, :, None, None]
    comp = torch.cat((x.max(1, keepdim=True)[0], x.mean(1, keepdim=True)), 1)
    conv, bn = self.SpatialGate.spatial.conv, self.SpatialGate.spatial.bn
    s = F.batch_norm(F.conv2d(comp, conv.weight, None, conv.stride, conv.padding), bn.running_mean, bn.running_var, bn.weight, bn.bias,
                     self.training, bn.momentum, bn.eps)
    if self.training:
        bn.num_batches_tracked.add_(1)
    return x * torch.sigmoid(s)


def stock_cbam(m):
    """swap every CBAM of `m` for cbam_stock_forward (module tree, names and state untouched); returns how many"""
    from models.cbam import CBAM
    n = 0
    for mod in m.modules():
        if isinstance(mod, CBAM):
            mod.forward = types.MethodType(cbam_stock_forward, mod)
            n += 1
    return n


# ------------------------------------------------------------------------------------------------ the comparison
def rel_err(got, ref):
    """max |got - ref| / max |ref|: relative to the tensor's own maximum (never to max(1, .)); the reference must not be all zero"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    top = float(ref.abs().max())
    assert top > 0.0 and math.isfinite(top), "the reference is all zero or not finite: the metric would be blind"
    return float((got - ref).abs().max()) / top


def param_kinds(m):
    """parameter name -> 'bn' (a normalisation layer's affine) or 'w' (everything else)"""
    kinds = {}
    for mn, mod in m.named_modules():
        norm = isinstance(mod, (nn.modules.batchnorm._BatchNorm, nn.GroupNorm))
        for pn, _ in mod.named_parameters(recurse=False):
            kinds[(mn + "." if mn else "") + pn] = "bn" if norm else "w"
    return kinds


def biases_before_batchnorm(m):
    """{bias name: weight name} of the convolutions that feed a BatchNorm directly: in train mode their gradient is zero by construction (the
    normalisation removes the batch mean), so its float64 value is rounding noise and the own-maximum metric would be blind"""
    out = {}
    for mn, mod in m.named_modules():
        if isinstance(mod, nn.Sequential):
            kids = list(mod.named_children())
            for (cn, c), (_, nxt) in zip(kids, kids[1:]):
                if isinstance(c, (nn.Conv2d, nn.Conv3d)) and c.bias is not None and isinstance(nxt, nn.modules.batchnorm._BatchNorm):
                    p = (mn + "." if mn else "") + cn
                    out[p + ".bias"] = p + ".weight"
    return out


def compare(got, ref, training, zero_bias):
    """got / ref: {'y': [...], 'dx': tensor or None, 'grads': {name: tensor or None}, 'buffers': {name: tensor}} -> {kind: (worst error, name)}.
    Every entry of ref is compared (the count is asserted); a parameter without a gradient must have none on both sides."""
    worst, n = {}, 0

    def note(kind, name, e):
        if kind not in worst or not (e <= worst[kind][0]):
            worst[kind] = (e, name)

    assert len(got["y"]) == len(ref["y"])
    for i, (a, b) in enumerate(zip(got["y"], ref["y"])):
        note("y", "y%d" % i, rel_err(a, b))
        n += 1
    if got["dx"] is not None:
        note("dx", "video", rel_err(got["dx"], ref["dx"]))
        n += 1
    assert set(got["grads"]) == set(ref["grads"]), set(got["grads"]) ^ set(ref["grads"])
    kinds = ref["kinds"]
    for name, r in ref["grads"].items():
        g = got["grads"][name]
        assert (g is None) == (r is None), "%s: a gradient on one side only (GPU %s, float64 %s)" % (name, g is not None, r is not None)
        if r is None:
            n += 1
            continue
        if training and name in zero_bias:
            # zero by construction: the float64 value is rounding noise next to the layer's weight gradient, the GPU's must be too
            scale = float(ref["grads"][zero_bias[name]].abs().max())
            assert float(r.abs().max()) <= 1e-9 * scale, name
            note("b0", name, float(g.detach().double().abs().max().cpu()) / scale)
        else:
            note(kinds[name], name, rel_err(g, r))
        n += 1
    assert set(got["buffers"]) == set(ref["buffers"])
    for name, r in ref["buffers"].items():
        g = got["buffers"][name]
        if name.endswith("num_batches_tracked"):
            assert int(g) == int(r), (name, int(g), int(r))
        else:
            note("run", name, rel_err(g, r))
        n += 1
    expect = len(ref["y"]) + (got["dx"] is not None) + len(ref["grads"]) + len(ref["buffers"])
    assert n == expect and len(ref["grads"]) == ref["n_params"] and len(ref["buffers"]) == ref["n_buffers"], (n, expect)
    return worst


# ------------------------------------------------------------------------------------------------ the cases
def _vggm(norm):
    from models.backbone import VA_3DVGGM
    return VA_3DVGGM(backend="none", norm_layer=norm)


def _split():
    from models.backbone import VA_3DVGGM_Split
    return VA_3DVGGM_Split(backend="none", split_layer=3)


def _resnet(ver, cbam, T):
    from models.backbone import VA_3DResNet
    return VA_3DResNet(frameLen=T, backend="none", resnet_ver=ver, use_cbam=cbam)


def _densenet(agg, T):
    from models.backbone import VA_3DDenseNet
    return VA_3DDenseNet(frameLen=T, backend="none", frontend_agg_mode=agg)


# name -> (constructor, (B, T, S))
CASES = {
    "vggm_bn": (lambda: _vggm("bn"), (3, 5, 112)),
    "vggm_gn": (lambda: _vggm("gn"), (2, 3, 110)),
    "split3": (_split, (2, 4, 112)),
    "resnet_v1_cbam": (lambda: _resnet("v1", True, 3), (3, 3, 100)),
    "resnet_v2": (lambda: _resnet("v2", False, 3), (2, 3, 96)),
    "resnet_v2_cbam": (lambda: _resnet("v2", True, 3), (2, 3, 96)),
    "densenet_ap": (lambda: _densenet("ap", 3), (2, 3, 80)),
    "densenet_fc": (lambda: _densenet("fc", 2), (1, 2, 112)),
}
SEED = 31
SE_DIM = 8          # the SENet / AU feature widths VA_3DVGGM_Split.features concatenates (no gradient)

# The videos of each case: part 1 and the flat-buffer test run on the first, gradient accumulation on both.  They are chosen -- measured on the
# MI355X -- where no ReLU or max (pooling, CBAM) decision flips between fp32 and float64.  A pre-activation within fp32 rounding of zero, or two
# pooling candidates within rounding of each other, route one element's gradient differently: a legitimate fp32 result that misses float64 by
# 1e-3 ... 2e-1 of the tensor's maximum in the weight gradients upstream of it (one flipped ReLU in 250 880 moves a DenseNet weight gradient by
# 2e-2; the stock fp32 CPU operators show the same jumps, and a 1e-7 relative change of the video in float64 alone reproduces them, while
# 1e-9 changes every tensor by ~1e-8 -- smooth error is not amplified).  Flips are dense in the train-mode DenseNet (1 of 16 videos of
# densenet_ap is free of them: its accumulation test is skipped).  A rounding change in a kernel can move a flip onto these videos: the message
# then names a tensor upstream of a ReLU / pooling, with an error of 1e-3 or more while every other tensor stays near 1e-6.
# (This happened to resnet_v2's video 0 when the plane BatchNorm kernels took their statistic sums in fp64: in float64 its closest
# pre-activation, at resnet.layer2.0.bn1, lies 7 fp32 roundings from zero, and the last bits of that layer's invstd now decide it the other way
# -- dbeta of layer2.0.bn1 and everything upstream moved by 2e-2 ... 5e-2, y and the running statistics stayed at 2e-6 / 2e-7.  Of the videos
# 0 ... 4, 6, 8, 9 measured with those kernels, 1, 3 and 6 are free of flips; the bars are unchanged.)
VIDEOS = {"vggm_bn": (2, 3), "vggm_gn": (0, 1), "split3": (1, 2), "resnet_v1_cbam": (1, 2), "resnet_v2": (1, 3), "resnet_v2_cbam": (7, 4),
          "densenet_ap": (13,), "densenet_fc": (9, 11)}

# Bars: max |err| / max |ref| per case, mode and tensor kind -- y output, dx video gradient, w weight gradients, bn normalisation affine
# gradients, b0 zero-by-construction conv biases (relative to their weight gradient), run running statistics (eval: untouched, exactly).
# Each is ~5 x the worst value measured on the MI355X over the case's videos and both GPU runs (rounded up), none looser than 1e-3.
BARS = {
    ("vggm_bn", "train"): {"b0": 4e-06, "bn": 4e-05, "dx": 5e-06, "run": 1e-06, "w": 9e-06, "y": 2e-05},
    ("vggm_bn", "eval"): {"bn": 3e-05, "dx": 3e-06, "run": 0.0, "w": 3e-05, "y": 2e-06},
    ("vggm_gn", "train"): {"bn": 2e-05, "dx": 3e-06, "w": 7e-06, "y": 4e-06},
    ("vggm_gn", "eval"): {"bn": 9e-06, "dx": 3e-06, "w": 7e-06, "y": 4e-06},
    ("split3", "train"): {"b0": 4e-06, "bn": 3e-05, "dx": 7e-06, "run": 2e-06, "w": 2e-05, "y": 2e-05},
    ("split3", "eval"): {"bn": 3e-05, "dx": 3e-06, "run": 0.0, "w": 2e-05, "y": 3e-06},
    ("resnet_v1_cbam", "train"): {"bn": 6e-05, "dx": 6e-06, "run": 3e-06, "w": 5e-05, "y": 5e-06},
    ("resnet_v1_cbam", "eval"): {"bn": 2e-05, "dx": 2e-06, "run": 0.0, "w": 3e-05, "y": 2e-06},
    ("resnet_v2", "train"): {"bn": 4e-05, "dx": 9e-06, "run": 2e-06, "w": 2e-05, "y": 2e-05},
    ("resnet_v2", "eval"): {"bn": 6e-05, "dx": 3e-06, "run": 0.0, "w": 3e-05, "y": 2e-06},
    ("resnet_v2_cbam", "train"): {"bn": 2e-04, "dx": 4e-06, "run": 3e-06, "w": 3e-05, "y": 6e-06},
    ("resnet_v2_cbam", "eval"): {"bn": 9e-06, "dx": 2e-06, "run": 0.0, "w": 7e-06, "y": 2e-06},
    ("densenet_ap", "train"): {"bn": 6e-04, "dx": 3e-05, "run": 3e-06, "w": 6e-05, "y": 3e-05},
    ("densenet_ap", "eval"): {"bn": 4e-06, "dx": 3e-06, "run": 0.0, "w": 5e-06, "y": 2e-06},
    ("densenet_fc", "train"): {"bn": 1e-03, "dx": 4e-05, "run": 4e-06, "w": 9e-05, "y": 3e-05},
    ("densenet_fc", "eval"): {"bn": 7e-06, "dx": 4e-06, "run": 0.0, "w": 6e-06, "y": 2e-06},
}


def bar(name, training, kind):
    return BARS[(name, "train" if training else "eval")][kind]


def _inputs(name, video_seed):
    B, T, S = CASES[name][1]
    rs = np.random.RandomState(1000 * video_seed + sum(map(ord, name)))
    video = rs.uniform(-1, 1, (B, 3, T, S, S)).astype(np.float32)
    extra = [rs.standard_normal((B, SE_DIM, T)).astype(np.float32) for _ in range(2)] if name == "split3" else []
    return video, extra


def _call(name, m, x, extra):
    from m3t import ops
    if name == "split3":
        with ops.batch_counters():          # (as VA_3DVGGM_Split.forward around features())
            return list(m.features(x, *extra))
    return [m(x)]


def _upstream(name, video_seed, shapes):
    rs = np.random.RandomState(7 + 1000 * video_seed + sum(map(ord, name)))
    return [rs.standard_normal(tuple(s)).astype(np.float32) for s in shapes]


def build(name, training, device=DEV):
    m = fill_module(CASES[name][0](), SEED).to(device)
    return m.train(training)


def step(name, m, video_seed, video_grad=True, dtype=torch.float32, device=DEV):
    """one forward + backward of sum((y * ct).sum()) over the front-end's outputs y, on video `video_seed` and its upstream gradients ct;
    returns (outputs, video gradient)"""
    video, extra = _inputs(name, video_seed)
    x = torch.from_numpy(video).to(device=device, dtype=dtype).requires_grad_(video_grad)
    ys = _call(name, m, x, [torch.from_numpy(e).to(device=device, dtype=dtype) for e in extra])
    ct = _upstream(name, video_seed, [y.shape for y in ys])
    sum((y * torch.from_numpy(c).to(device=device, dtype=dtype)).sum() for y, c in zip(ys, ct)).backward()
    return [y.detach() for y in ys], x.grad


def snapshot(m, ys, dx):
    return {"y": ys, "dx": dx,
            "grads": {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()},
            "buffers": {n: b.detach().clone() for n, b in m.named_buffers()}}


def float64_copy(m):
    ref = copy.deepcopy(m).cpu().double()
    stock_cbam(ref)
    return ref


_REFS = {}


def reference(name, training, passes=1, source=None):
    """the float64 run of case `name`, computed once and kept for the rest of the file: the module built on the GPU in fp32 by
    fill_module, copied to the CPU in float64 with CBAM swapped for stock operators.  passes=2: gradients and buffers after a second
    forward / backward on another video (the sum of both passes)."""
    key = (name, training, passes)
    if key in _REFS:
        return _REFS[key]
    ref = float64_copy(source if source is not None else build(name, training))
    t0 = time.perf_counter()
    for vs in VIDEOS[name][:passes]:
        ys, dx = step(name, ref, vs, True, torch.float64, "cpu")
    out = snapshot(ref, ys, dx)
    out.update(secs=time.perf_counter() - t0, kinds=param_kinds(ref), zero_bias=biases_before_batchnorm(ref),
               n_params=len(list(ref.parameters())), n_buffers=len(list(ref.buffers())))
    _REFS[key] = out
    return out


def _check(name, training, worst, what):
    line = "  ".join("%s %.2e (%s)" % (k, e, n) for k, (e, n) in sorted(worst.items()))
    print("\nfp64 %s %s %s: %s" % (name, "train" if training else "eval", what, line))
    bad = {k: (e, n) for k, (e, n) in worst.items() if not (e <= bar(name, training, k))}
    assert not bad, "%s %s: errors over the bar %s" % (name, what, bad)


# ------------------------------------------------------------------------------------------------ part 1: whole front-ends against float64
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("name", list(CASES))
def test_front_end_against_float64(name, training):
    from m3t import ops
    ref = reference(name, training)
    print("\nfp64 %s reference: %.1f s" % (name, ref["secs"]))
    for video_grad in (True, False):
        m = build(name, training)
        before = dict(ops.STOCK_FALLBACKS)
        ys, dx = step(name, m, VIDEOS[name][0], video_grad)
        torch.cuda.synchronize()
        took = {k: v - before.get(k, 0) for k, v in ops.STOCK_FALLBACKS.items() if v != before.get(k, 0)}
        # the one stock operator allowed: the first layer's data gradient with respect to the (3-channel) video
        assert all(video_grad and k.startswith("conv3d data gradient k(64, 3,") for k in took), took
        worst = compare(snapshot(m, ys, dx), ref, training, ref["zero_bias"])
        _check(name, training, worst, "video grad" if video_grad else "chain")


def test_the_cases_reach_the_paths_they_are_for():
    """the geometries the module docstring promises: ragged conv1 rows, CBAM's three paths, odd per-frame grids, the dense maps"""
    from m3t import ops, _lib
    lib = _lib.load()
    assert 3 * 5 * 55 * 55 == 45375 and 45375 % 128 != 0
    assert not lib.m3t_cbam_fused_ok(64, 4, 25, 25)            # 625 odd pixels: the two gates one after the other
    assert lib.m3t_cbam_fused_ok(128, 8, 13, 13) and lib.m3t_cbam_fused_ok(512, 32, 4, 4)
    seen = {}

    def spy(kind):
        real = getattr(ops, kind)

        def f(x, *a, **k):
            seen.setdefault(kind, set()).add(tuple(x.shape[1:]))
            return real(x, *a, **k)
        return real, f

    saved = {}
    try:
        for kind in ("cbam", "channel_gate", "conv2d"):
            saved[kind], f = spy(kind)
            setattr(ops, kind, f)
        m = build("resnet_v1_cbam", True)
        video, _ = _inputs("resnet_v1_cbam", VIDEOS["resnet_v1_cbam"][0])
        y = m(torch.from_numpy(video).to(DEV))
        torch.cuda.synchronize()
    finally:
        for kind, real in saved.items():
            setattr(ops, kind, real)
    assert seen["channel_gate"] == {(64, 25, 25)}, seen
    assert {(128, 13, 13), (256, 7, 7), (512, 4, 4)} <= seen["cbam"], seen
    assert {s[1:] for s in seen["conv2d"]} >= {(25, 25), (13, 13), (7, 7), (4, 4)} and y.shape == (3, 3, 512)
    m = build("vggm_bn", True)
    x = m.v2p[0](torch.from_numpy(_inputs("vggm_bn", VIDEOS["vggm_bn"][0])[0]).to(DEV))
    assert isinstance(x, ops.CLTensor) and x.data.shape[0] == 45375


# ------------------------------------------------------------------------------------------------ part 2: the flat gradient buffer
def _count_sinks(monkeypatch):
    from m3t import ops
    taken, real = [0], ops._take_sink

    def take(p):
        v = real(p)
        taken[0] += v is not None
        return v
    monkeypatch.setattr(ops, "_take_sink", take)
    return taken


def _flat_run(name, passes, monkeypatch):
    """train mode under FlatGradDDP (gradient sinks and weight-gradient streams on, the default): `passes` forward / backward passes on
    the case's VIDEOS and ONE finish() -> (module, last outputs, {name: flat slice}, sinks taken)"""
    from m3t.ddp import FlatGradDDP
    m = build(name, True)
    taken = _count_sinks(monkeypatch)
    ddp = FlatGradDDP(m, max_norm=0.0)
    try:
        assert ddp.sinks
        ddp.zero_grad()
        for vs in VIDEOS[name][:passes]:
            ys, _ = step(name, m, vs, False)
        ddp.finish()
        torch.cuda.synchronize()
        flat = {n: ddp.flat[ddp.offsets[id(p)]:ddp.offsets[id(p)] + p.numel()].view_as(p).clone() for n, p in m.named_parameters()}
    finally:
        ddp.close()
    return m, ys, flat, taken[0]


def _check_flat(name, passes, monkeypatch):
    ref = reference(name, True, passes)
    m, ys, flat, taken = _flat_run(name, passes, monkeypatch)
    assert taken > 0, taken                         # the sinks were really used
    for n, r in ref["grads"].items():
        if r is None:                               # no gradient: the slice stays as zero_grad() left it
            assert not bool(flat[n].any()), n
            flat[n] = None
    got = {"y": ys, "dx": None, "grads": flat, "buffers": {n: b.detach().clone() for n, b in m.named_buffers()}}
    _check(name, True, compare(got, ref, True, ref["zero_bias"]), "flat buffer, %d pass%s" % (passes, "es" if passes > 1 else ""))


@pytest.mark.parametrize("name", list(CASES))
def test_flat_gradient_buffer_against_float64(name, monkeypatch):
    """each slice of FlatGradDDP's buffer after finish() against the float64 gradients of part 1"""
    _check_flat(name, 1, monkeypatch)


@pytest.mark.parametrize("name", [n for n in CASES if len(VIDEOS[n]) > 1])
def test_gradient_accumulation_against_float64(name, monkeypatch):
    """two forward / backward passes on different videos before one finish(): the second finds every sink taken and hands its gradients to
    autograd, which adds them onto slices the first may still be writing on a weight-gradient stream -- the result is the float64 sum"""
    _check_flat(name, 2, monkeypatch)


def _shared_conv_net(kind):
    """one convolution weight applied twice: to a small input first, then to a large one made of one repeated frame (clip), so that in backward
    the large use runs first, takes the sink and writes it from a long weight-gradient walk on a weight-gradient stream, while the small use
    returns its gradient quickly on the main stream for autograd to add onto the same slice.  The large use's float64 gradient is the repeat
    count times one frame's (clip's)."""
    from m3t import ops
    from models.backbone import Conv3d
    from models.resnet import GemmConv2d
    rs = np.random.RandomState(5)
    if kind == "planes":
        conv = GemmConv2d(64, 64, 3, 1, 1, bias=False)
        lo = rs.standard_normal((2, 64, 9, 9)).astype(np.float32)
        one = rs.standard_normal((1, 64, 56, 56)).astype(np.float32)
        reps = 512                      # 1.6 M rows: a walk of ~120 GFLOP
    else:
        conv = Conv3d(64, 64, 3, 1, 1)
        lo = rs.standard_normal((1, 64, 2, 6, 6)).astype(np.float32)
        one = rs.standard_normal((1, 64, 4, 56, 56)).astype(np.float32)
        reps = 64                       # 0.8 M rows, K = 1728: ~180 GFLOP
    fill_module(conv, 9)
    c_lo = 1000.0 * rs.standard_normal(lo.shape).astype(np.float32)      # (the small use's gradient as large as the big one's)
    c_one = rs.standard_normal(one.shape).astype(np.float32)

    def to_cl(a):
        return ops.CLTensor(a.permute(0, 2, 3, 4, 1).reshape(-1, a.shape[1]).contiguous(), a.shape[0], *a.shape[2:], None)

    def loss(m):
        total = 0
        for x, c, n in ((lo, c_lo, 1), (one, c_one, reps)):
            xd, cd = torch.from_numpy(x).to(DEV), torch.from_numpy(c).to(DEV)
            if n > 1:
                xd, cd = xd.expand((n,) + x.shape[1:]).contiguous(), cd.expand((n,) + c.shape[1:]).contiguous()
            if kind == "planes":
                total = total + (m(xd) * cd).sum()
            else:
                y = m(to_cl(xd))
                assert isinstance(y, ops.CLTensor)          # the channels-last class (_Conv3dCL)
                total = total + (y.data * to_cl(cd).data).sum()
        return total

    def float64_grad():
        from torch.nn.grad import conv2d_weight, conv3d_weight
        fn = conv2d_weight if kind == "planes" else conv3d_weight
        w = conv.weight.detach().double()
        g = 0
        for x, c, n in ((lo, c_lo, 1), (one, c_one, reps)):
            x64, c64 = torch.from_numpy(x).double(), torch.from_numpy(c).double()
            g = g + n * fn(x64, w.shape, c64, conv.stride, conv.padding)
        return g
    return conv, loss, float64_grad


@pytest.mark.parametrize("kind", ["planes", "channels_last"])
def test_shared_conv_weight_with_deferred_sink_write(kind, monkeypatch):
    """the flat slice of a convolution weight used twice in one graph equals plain autograd's sum and the float64 sum -- on the planes class
    (_Conv3dGemmWgrad: GemmConv2d) and on the channels-last class (_Conv3dCL: a stem Conv3d on channels-last rows).  Before the use that finds
    the sink taken returns its gradient to autograd, it must join the weight-gradient stream the other use writes the sink from."""
    from m3t.ddp import FlatGradDDP
    conv, loss, float64_grad = _shared_conv_net(kind)
    plain = copy.deepcopy(conv).to(DEV)
    m = conv.to(DEV)
    taken = _count_sinks(monkeypatch)
    ddp = FlatGradDDP(m, max_norm=0.0)
    try:
        ddp.zero_grad()
        loss(m).backward()
        ddp.finish()
        torch.cuda.synchronize()
        o = ddp.offsets[id(m.weight)]
        flat = ddp.flat[o:o + m.weight.numel()].view_as(m.weight).clone()
        flat_b = ddp.flat[ddp.offsets[id(m.bias)]:ddp.offsets[id(m.bias)] + m.bias.numel()].clone() if m.bias is not None else None
    finally:
        ddp.close()
    assert taken[0] >= 1
    loss(plain).backward()
    torch.cuda.synchronize()
    g64 = float64_grad()
    e_plain, e_64 = rel_err(flat, plain.weight.grad), rel_err(flat, g64)
    print("\nshared %s weight: flat vs autograd %.2e, vs float64 %.2e (autograd vs float64 %.2e)" % (kind, e_plain, e_64, rel_err(plain.weight.grad, g64)))
    assert e_plain <= 1e-6 and e_64 <= 2e-5, (e_plain, e_64)
    if flat_b is not None:
        assert rel_err(flat_b, plain.bias.grad) <= 1e-6


def test_batchnorm_applied_twice_counts_twice(monkeypatch):
    """A PlaneBatchNorm2d applied twice in one train-mode forward inside ops.batch_counters() (as the front-ends' forward passes are): its
    num_batches_tracked advances by 2 and its running statistics equal the stock module's applied twice.  The queued counters are added by ONE
    multi-tensor launch, also when one of them is queued twice (a repeated tensor in that launch is two workgroups racing on one element)."""
    from m3t import ops
    from models.resnet import PlaneBatchNorm2d
    bns = [fill_module(PlaneBatchNorm2d(64, fuse_relu=i == 0), 11 + i).to(DEV).train() for i in range(3)]
    refs = [copy.deepcopy(b).cpu().double() for b in bns]
    x = torch.from_numpy(np.random.RandomState(4).standard_normal((6, 64, 13, 13)).astype(np.float32))
    launches = []
    real_add = torch._foreach_add_

    def counted(*a, **k):
        launches.append(len(a[0]))
        return real_add(*a, **k)
    monkeypatch.setattr(torch, "_foreach_add_", counted)
    for order in ([0, 0], [0, 1, 0, 2], [0, 1, 2]):
        n0 = len(launches)
        with ops.batch_counters():
            y = x.to(DEV)
            for i in order:
                y = bns[i](y)
        y64 = x.double()
        for i in order:
            y64 = refs[i](y64)
        torch.cuda.synchronize()
        assert rel_err(y, y64) <= 1e-5, order
        for b, r in zip(bns, refs):
            assert int(b.num_batches_tracked) == int(r.num_batches_tracked), (order, int(b.num_batches_tracked), int(r.num_batches_tracked))
            assert rel_err(b.running_mean, r.running_mean) <= 1e-5 and rel_err(b.running_var, r.running_var) <= 1e-5, order
        assert launches[n0:] == ([len(set(order))] if len(set(order)) > 1 else []), (order, launches)     # one launch, or one add
    assert [int(b.num_batches_tracked) for b in bns] == [5, 2, 2] and launches == [3, 3]
