"""The whole per-frame ResNet (v1) front-end on the channels-last chain (M3T_RESNET_CL=1) against float64.

Model: VA_3DResNet(frameLen=3, backend='none', resnet_ver='v1', use_cbam=False), parameters filled at random (golden.recipe.fill_module: non-zero
bn2.weight), video [2, 3, 3, 52, 44]: the maps go 26 x 22 -> 13 x 11 -> 7 x 6 -> 4 x 3 -> 2 x 2, every parity class of the stride-2 data
gradients, odd and even sizes in both axes.  Reference: a float64 copy of the module on the CPU (every module takes its stock operator there).
Yardstick: the planes route -- the same weights built with the switch off, the same video, the same process.  Bar, per tensor (output, every
parameter gradient, every BatchNorm buffer): the chain's error <= 4 x max(the planes route's error, 2^-23), errors as max |err| / max |ref|;
num_batches_tracked exactly.  The video has no gradient on the chain (its first layer has no data gradient; a video that requires one keeps the
whole front-end on planes, as before), so there is no video-side dx to compare.

Videos are chosen from the float64 run alone (resnet_ref.pick_video: every ReLU pre-activation and every pooling window clear of what fp32
rounding can move), seeds in steps of 1000 from 0, at most 8: seed 0 is taken in both modes (tests/test_resnet_cl_host.py runs the same
selection without a GPU).

Measured on the MI355X (worst chain / planes error ratio per kind, the bar being 4): train y 1.04 (3.2e-6 vs 3.0e-6), w 1.17, bn 1.29, running
statistics 1.26; eval y 1.00, w 1.00, bn 1.11, running statistics untouched; the flat buffer the same as plain autograd, 60 sinks taken."""
import argparse
import copy
import math

import numpy as np
import pytest
import torch

import resnet_ref as R
from golden.recipe import fill_module

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -23
SEED = 31


@pytest.fixture(autouse=True)
def _switch_restored():
    from m3t import ops
    was = ops.RESNET_CL[0]
    yield
    ops.RESNET_CL[0] = was


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    top = float(ref.abs().max())
    assert top > 0.0 and math.isfinite(top), "the reference is all zero or not finite: the metric would be blind"
    return float((got - ref).abs().max()) / top


def build(on, training, depth=18, ver="v1", cbam=False, fill=True):
    """VA_3DResNet built with the switch `on` (it stays so for the caller's run), filled from SEED"""
    from m3t import ops
    from models.backbone import VA_3DResNet
    ops.RESNET_CL[0] = on
    torch.manual_seed(SEED)
    m = VA_3DResNet(frameLen=3, backend="none", resnet_ver=ver, use_cbam=cbam, resnet_depth=depth)
    if fill:
        fill_module(m, SEED)
    return m.to(DEV).train(training)


def upstream(seed):
    return torch.from_numpy(np.random.RandomState(7 + seed).standard_normal((2, 3, 512)).astype(np.float32))


def step(m, video, ct):
    y = m(video)
    (y * ct).sum().backward()
    return y


def snapshot(m, y):
    return {"y": y.detach(), "grads": {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in m.named_parameters()},
            "buffers": {n: b.detach().clone() for n, b in m.named_buffers()}}


def graph_names(t):
    """the autograd node names reachable from t"""
    seen, names, todo = set(), set(), [t.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__)
        todo.extend(f for f, _ in fn.next_functions)
    return names


def assert_on_chain(names):
    assert not any(n.startswith(("_BctToBtc", "_BtcToBct")) for n in names), "a transpose between the first convolution and the output: %s" % sorted(names)
    assert any(n.startswith("_BNAddReluCL") for n in names) and any(n.startswith("_MeanCL") for n in names), sorted(names)
    assert not any(n.startswith(("_Conv3dGemmWgrad", "_BNPlanes", "_AddRelu", "_PoolPlanes")) for n in names), sorted(names)


_REFS = {}


def reference(training):
    """the float64 run, computed once per mode and shared: video by seed from the float64 module alone, one forward + backward"""
    if training not in _REFS:
        ref = copy.deepcopy(build(False, training)).cpu().double()
        video, taken = R.pick_video(ref, 0)
        print("\n%s: video seed %d taken" % ("train" if training else "eval", taken))
        ct = upstream(taken)
        y = step(ref, video, ct.double())
        _REFS[training] = dict(video=video.float(), ct=ct, **snapshot(ref, y))
    return _REFS[training]


def errors(got, ref):
    """{tensor name: error} over the output, every parameter gradient and every floating buffer; the counters compared exactly"""
    out = {"y": rel_err(got["y"], ref["y"])}
    assert set(got["grads"]) == set(ref["grads"]) and set(got["buffers"]) == set(ref["buffers"])
    for n, r in ref["grads"].items():
        g = got["grads"][n]
        assert (g is None) == (r is None), "%s: a gradient on one side only" % n
        if r is not None:
            out["grad " + n] = rel_err(g, r)
    for n, r in ref["buffers"].items():
        if n.endswith("num_batches_tracked"):
            assert int(got["buffers"][n]) == int(r), (n, int(got["buffers"][n]), int(r))
        else:
            out["buffer " + n] = rel_err(got["buffers"][n], r)
    return out


def kind_of(name):
    if name == "y":
        return "y"
    if name.startswith("buffer"):
        return "run"
    return "bn" if (".bn" in name or ".downsample.1." in name or name.startswith("grad c3d.1.")) else "w"


def within_the_bar(what, e_chain, e_planes):
    assert set(e_chain) == set(e_planes)
    bad, worst = {}, {}
    for n in e_chain:
        ratio = e_chain[n] / max(e_planes[n], FLOOR)
        k = kind_of(n)
        if k not in worst or ratio > worst[k][0]:
            worst[k] = (ratio, n, e_chain[n], e_planes[n])
        if not e_chain[n] <= 4.0 * max(e_planes[n], FLOOR):
            bad[n] = (e_chain[n], e_planes[n])
    for k, (ratio, n, a, b) in sorted(worst.items()):
        print("%s worst %-3s ratio %.2f (chain %.2e, planes %.2e: %s)" % (what, k, ratio, a, b, n))
    assert not bad, "%s: over 4 x max(planes error, 2^-23): %s" % (what, bad)


_PLANES = {}


def planes_errors(training):
    """the yardstick: the planes route (switch off, same weights, same video), once per mode"""
    from m3t import ops
    if training not in _PLANES:
        ref = reference(training)
        m = build(False, training)
        assert not m.c3d[0].cl_chain
        y = step(m, ref["video"].to(DEV), ref["ct"].to(DEV))
        ops.join_wgrad()
        torch.cuda.synchronize()
        assert not any(n.startswith(("_BNAddReluCL", "_MeanCL", "_Conv3dCL")) for n in graph_names(y))
        _PLANES[training] = errors(snapshot(m, y), ref)
    return _PLANES[training]


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_front_end_on_the_chain_against_float64(training):
    from m3t import ops
    ref, e_planes = reference(training), planes_errors(training)
    m = build(True, training)
    assert m.c3d[0].cl_chain
    before, walks = dict(ops.STOCK_FALLBACKS), ops.CONV3D_CALLS["walk"]
    y = step(m, ref["video"].to(DEV), ref["ct"].to(DEV))
    ops.join_wgrad()
    torch.cuda.synchronize()
    assert ops.STOCK_FALLBACKS == before, "a stock operator ran"
    assert ops.CONV3D_CALLS["walk"] == walks + 20            # the stem's convolution and the trunk's 19 (16 in blocks, 3 downsample)
    assert_on_chain(graph_names(y))
    assert y.shape == (2, 3, 512)
    print()
    within_the_bar("train" if training else "eval", errors(snapshot(m, y), ref), e_planes)


def test_flat_gradient_buffer_with_sinks_armed(monkeypatch):
    """train mode under FlatGradDDP (gradient sinks and weight-gradient streams on): each slice of the flat buffer against float64, same bar"""
    from m3t import ops
    from m3t.ddp import FlatGradDDP
    ref, e_planes = reference(True), planes_errors(True)
    m = build(True, True)
    taken, real = [0], ops._take_sink

    def take(p):
        v = real(p)
        taken[0] += v is not None
        return v
    monkeypatch.setattr(ops, "_take_sink", take)
    ddp = FlatGradDDP(m, max_norm=0.0)
    try:
        assert ddp.sinks
        ddp.zero_grad()
        y = m(ref["video"].to(DEV))
        assert_on_chain(graph_names(y))
        (y * ref["ct"].to(DEV)).sum().backward()
        ddp.finish()
        torch.cuda.synchronize()
        flat = {n: ddp.flat[ddp.offsets[id(p)]:ddp.offsets[id(p)] + p.numel()].view_as(p).clone() for n, p in m.named_parameters()}
    finally:
        ddp.close()
    print("\nsinks taken: %d" % taken[0])
    assert taken[0] >= 20, taken[0]                          # (the sinks were really used: at least every convolution weight)
    for n, r in ref["grads"].items():
        if r is None:
            assert not bool(flat[n].any()), n
            flat[n] = None
    got = {"y": y.detach(), "grads": flat, "buffers": {n: b.detach().clone() for n, b in m.named_buffers()}}
    print()
    within_the_bar("flat buffer", errors(got, ref), e_planes)


def test_depth_34_takes_the_chain():
    ref = reference(True)
    m = build(True, True, depth=34)
    y = step(m, ref["video"].to(DEV), ref["ct"].to(DEV))
    torch.cuda.synchronize()
    assert_on_chain(graph_names(y))
    assert y.shape == (2, 3, 512) and bool(torch.isfinite(y).all())
    for n, p in m.named_parameters():
        if not n.startswith("resnet.fc."):
            assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), n


@pytest.mark.parametrize("kw", [dict(ver="v1", cbam=True), dict(ver="v2"), dict(ver="v1", off=True)], ids=["cbam", "v2", "switch_off"])
def test_what_the_chain_does_not_carry_keeps_the_parent_route_bits(kw):
    """use_cbam=True, resnet_ver='v2': built and run with the switch on, the same bits as built and run with it off.  The switch off: a
    model built after the switch went on and off again runs the planes route, the same bits as one built before"""
    from m3t import ops
    ref = reference(True)
    off = kw.pop("off", False)
    outs = []
    for on in (False, True):
        if off:
            ops.RESNET_CL[0] = on                            # (on: flipped on, then off again by build(False, ...))
            m = build(False, True, **kw)
        else:
            m = build(on, True, **kw)
        assert not m.c3d[0].cl_chain
        y = step(m, ref["video"].to(DEV), ref["ct"].to(DEV))
        ops.join_wgrad()
        torch.cuda.synchronize()
        assert not any(n.startswith(("_BNAddReluCL", "_MeanCL", "_Conv3dCL")) for n in graph_names(y))
        outs.append(snapshot(m, y))
    a, b = outs
    assert torch.equal(a["y"], b["y"])
    for n in a["grads"]:
        assert (a["grads"][n] is None) == (b["grads"][n] is None) and (a["grads"][n] is None or torch.equal(a["grads"][n], b["grads"][n])), n
    for n in a["buffers"]:
        assert torch.equal(a["buffers"][n], b["buffers"][n]), n


def test_a_video_that_requires_grad_stays_on_planes():
    """the chain's first layer has no data gradient: such a video takes the parent route end to end, with the parent's video gradient"""
    ref = reference(True)
    outs = []
    for on in (False, True):
        m = build(on, True)
        v = ref["video"].to(DEV).requires_grad_(True)
        y = step(m, v, ref["ct"].to(DEV))
        torch.cuda.synchronize()
        assert not any(n.startswith(("_BNAddReluCL", "_MeanCL", "_Conv3dCL")) for n in graph_names(y))
        outs.append((y.detach(), v.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------ AffWild2VA(backbone='resnet')
def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _affwild(on):
    from m3t import ops
    from models.model import AffWild2VA
    ops.RESNET_CL[0] = on
    torch.manual_seed(SEED)
    return AffWild2VA(_hp(modality="visual", backbone="resnet", loss="ccc", window=3, num_hidden=64)).to(DEV)


def test_uint8_batch_takes_the_cl_layout_and_matches_the_float32_route(monkeypatch):
    """uint8 frames [2, 3, 56, 48, 3] with video_aug (a 44-pixel crop, the second clip mirrored): under the switch the ingest writes the
    channels-last image (a VideoCL) and the output matches the model's own float32-video route on the same crop within 2^-23 of its maximum
    (observed on the MI355X: the same bits)"""
    from m3t import ops, video
    model = _affwild(True).eval()
    assert model.visual.c3d[0].cl_chain
    rs = np.random.RandomState(14)
    u8 = torch.from_numpy(rs.randint(0, 256, (2, 3, 56, 48, 3)).astype(np.uint8)).to(DEV)
    aug = [{"cy": 4, "cx": 2, "size": 44, "mirror": False, "cutout": None, "table": None},
           {"cy": 7, "cx": 0, "size": 44, "mirror": True, "cutout": None, "table": None}]
    layouts, real = [], video.ingest

    def spy(frames, aug_, fidx, layout, **k):
        layouts.append(layout)
        return real(frames, aug_, fidx, layout, **k)
    monkeypatch.setattr(video, "ingest", spy)
    se = torch.zeros(2, 512, 3, device=DEV)
    with torch.no_grad():
        a = model({"video": u8, "video_aug": aug, "se_features": se})
        crops = [u8[0, :, 4:48, 2:46], u8[1, :, 7:51, 0:44].flip(2)]
        f32 = torch.stack(crops).permute(0, 4, 1, 2, 3).float().contiguous()
        b = model({"video": f32, "se_features": se})
    torch.cuda.synchronize()
    assert layouts == ["cl"], layouts
    same = torch.equal(a, b)
    print("\nuint8 route vs float32 route: %s (max |diff| %.3e)" % ("the same bits" if same else "different bits", float((a - b).abs().max())))
    assert a.shape == (2, 3, 2) and float((a - b).abs().max()) <= FLOOR * float(b.abs().max())


def _va_batch(seed, B=2, T=3, H=52, W=44):
    rs = np.random.RandomState(seed)
    f = lambda a: torch.from_numpy(a).to(DEV)
    return {"video": f(rs.randint(0, 256, (B, 3, T, H, W)).astype(np.float32)), "se_features": f(rs.standard_normal((B, 512, T)).astype(np.float32)),
            "label_valence": f(rs.uniform(-1, 1, (B, T)).astype(np.float32)), "label_arousal": f(rs.uniform(-1, 1, (B, T)).astype(np.float32)),
            "vid_name": ["v"] * B, "start": torch.zeros(B, dtype=torch.long), "length": torch.full((B,), T)}


def test_training_step_under_trainer_matches_the_planes_route():
    """two steps of Trainer (fused Adam, gradient sinks) from the model's own initial state (bn2.weight = 0): the loss of each step equals the
    planes route's within 1e-5 relative (measured on the MI355X: 0.99916774 and 0.99782097 on both routes, relative difference 0.0), and the
    optimizer reaches the block tails' BatchNorm"""
    from m3t import ops
    from m3t.trainer import Trainer
    losses = {}
    for on in (False, True):
        model = _affwild(on)
        tr = Trainer.from_hparams(model, model.hparams)
        try:
            bn2 = model.visual.resnet.layer1[0].bn2.weight
            assert not bool(bn2.detach().any())
            before = dict(ops.STOCK_FALLBACKS)
            out = [tr.step(_va_batch(41 + i)) for i in range(2)]
            torch.cuda.synchronize()
            losses[on] = [float(o["loss"].detach()) for o in out]
            assert all(math.isfinite(v) for v in losses[on]) and math.isfinite(float(out[-1]["grad_norm"]))
            assert bool(bn2.detach().any()), "the optimizer step did not reach bn2.weight"
            assert {k: v for k, v in ops.STOCK_FALLBACKS.items() if v != before.get(k, 0)} == {}
        finally:
            tr.ddp.close()
    for i, (a, b) in enumerate(zip(losses[True], losses[False])):
        rel = abs(a - b) / abs(b)
        print("\nstep %d: loss chain %.8f  planes %.8f  relative difference %.2e" % (i, a, b, rel))
        assert rel <= 1e-5, (i, a, b)
