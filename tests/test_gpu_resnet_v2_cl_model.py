"""The whole per-frame ResNet v2 (pre-activation) front-end on the channels-last chain (M3T_RESNET_V2_CL=1) against float64.

Model: VA_3DResNet(frameLen=3, backend='none', resnet_ver='v2', use_cbam=False), parameters filled at random (golden.recipe.fill_module), video
[2, 3, 3, 52, 44]: the maps go 26 x 22 -> 13 x 11 -> 7 x 6 -> 4 x 3 -> 2 x 2, every parity class of the stride-2 data gradients, odd and even sizes
in both axes.  Reference: a float64 copy of the module on the CPU (every module takes its stock operator there).  Yardstick: the planes route --
the same weights built with the switch off, the same video, the same process.  Bar, per tensor (output, every parameter gradient, every
BatchNorm buffer): the chain's error <= 4 x max(the planes route's error, 2^-23), errors as max |err| / max |ref|; num_batches_tracked exactly.
The video has no gradient on the chain (its first layer has no data gradient; a video that requires one keeps the whole front-end on planes, as
before), so there is no video-side dx to compare.

Videos are chosen from the float64 run alone (resnet_ref.pick_video, unchanged: every ReLU pre-activation -- all of v2's BatchNorms carry their
ReLU -- and every pooling window clear of what fp32 rounding can move), seeds in steps of 1000 from 0, at most 8: seed 0 is taken in both modes
(tests/test_resnet_v2_cl_host.py runs the same selection without a GPU).

frontend_agg_mode='fc' cannot run with resnet_ver='v2' on any route: the trunk pools to [N T, 512] before a Linear that expects 512 x 3 x 3
inputs, as in the reference (models/resnet.py:244-249).  What can be held there is held: the switch does not mark such a model and both
builds fail in the same place, on planes.

Measured on the MI355X (worst chain / planes error ratio per kind, the bar being 4): train y 1.09 (3.1e-6 vs 2.8e-6), w 1.10, bn 1.27, running
statistics 1.17; eval y 1.00, w 1.04, bn 1.25, running statistics untouched; the flat buffer the same as plain autograd, 54 sinks taken; the
uint8 route the float32 video's bits; two fused-Adam steps within 2.9e-7 relative of the planes route's losses."""
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
CHAIN_NODES = ("_AddBNReluCL", "_BNAddReluCL", "_MeanCL", "_Conv3dCL", "_BNCL", "_PoolCL")


@pytest.fixture(autouse=True)
def _switches_restored():
    from m3t import ops
    was = ops.RESNET_V2_CL[0], ops.RESNET_CL[0]
    ops.RESNET_CL[0] = False
    yield
    ops.RESNET_V2_CL[0], ops.RESNET_CL[0] = was


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    top = float(ref.abs().max())
    assert top > 0.0 and math.isfinite(top), "the reference is all zero or not finite: the metric would be blind"
    return float((got - ref).abs().max()) / top


def build(on, training, depth=18, ver="v2", cbam=False, agg="ap", backend="none", **kw):
    """VA_3DResNet built with the v2 switch `on` (it stays so for the caller's run), filled from SEED"""
    from m3t import ops
    from models.backbone import VA_3DResNet
    ops.RESNET_V2_CL[0] = on
    torch.manual_seed(SEED)
    m = VA_3DResNet(frameLen=3, backend=backend, resnet_ver=ver, use_cbam=cbam, resnet_depth=depth, frontend_agg_mode=agg, **kw)
    return fill_module(m, SEED).to(DEV).train(training)


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
    assert any(n.startswith("_AddBNReluCL") for n in names) and any(n.startswith("_MeanCL") for n in names), sorted(names)
    assert not any(n.startswith(("_Conv3dGemmWgrad", "_BNPlanes", "_PoolPlanes", "AddBackward")) for n in names), sorted(names)


def assert_on_planes(names):
    assert not any(n.startswith(CHAIN_NODES) for n in names), sorted(names)


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
    return "bn" if (".bn" in name or name.startswith("grad c3d.1.")) else "w"


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


def planes_run(training):
    """the yardstick: the planes route (switch off, same weights, same video), once per mode -> (its snapshot, its errors)"""
    from m3t import ops
    if training not in _PLANES:
        ref = reference(training)
        m = build(False, training)
        assert not m.c3d[0].cl_chain
        y = step(m, ref["video"].to(DEV), ref["ct"].to(DEV))
        ops.join_wgrad()
        torch.cuda.synchronize()
        assert_on_planes(graph_names(y))
        snap = snapshot(m, y)
        _PLANES[training] = (snap, errors(snap, ref))
    return _PLANES[training]


def same_bits(a, b):
    assert torch.equal(a["y"], b["y"])
    for n in a["grads"]:
        assert (a["grads"][n] is None) == (b["grads"][n] is None) and (a["grads"][n] is None or torch.equal(a["grads"][n], b["grads"][n])), n
    for n in a["buffers"]:
        assert torch.equal(a["buffers"][n], b["buffers"][n]), n


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_front_end_on_the_chain_against_float64(training):
    from m3t import ops
    ref, (_, e_planes) = reference(training), planes_run(training)
    m = build(True, training)
    assert m.c3d[0].cl_chain and m.resnet.cl_eligible()
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


def test_inference_under_no_grad_gives_the_bits_of_the_grad_mode_forward():
    """eval under no_grad: the sums nobody reads again are not written (add_bn_relu_cl's need_s) -- the output does not change"""
    ref = reference(False)
    m = build(True, False)
    v = ref["video"].to(DEV)
    y = m(v)
    with torch.no_grad():
        y0 = m(v)
    torch.cuda.synchronize()
    assert_on_chain(graph_names(y))
    assert y0.grad_fn is None and torch.equal(y0, y.detach())


def test_flat_gradient_buffer_with_sinks_armed(monkeypatch):
    """train mode under FlatGradDDP (gradient sinks and weight-gradient streams on): each slice of the flat buffer against float64, same bar"""
    from m3t import ops
    from m3t.ddp import FlatGradDDP
    ref, (_, e_planes) = reference(True), planes_run(True)
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
    assert m.c3d[0].cl_chain and m.resnet.cl_eligible()
    y = step(m, ref["video"].to(DEV), ref["ct"].to(DEV))
    torch.cuda.synchronize()
    assert_on_chain(graph_names(y))
    assert y.shape == (2, 3, 512) and bool(torch.isfinite(y).all())
    for n, p in m.named_parameters():
        if not n.startswith("resnet.fc."):
            assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), n


@pytest.mark.parametrize("kw", [dict(cbam=True), dict(off=True), dict(v1_switch=True)], ids=["cbam", "switch_off", "v1_switch_only"])
def test_what_the_chain_does_not_carry_keeps_the_planes_route_bits(kw):
    """use_cbam=True built and run with the switch on; a model built after the switch went on and off again; v2 under the v1 switch alone: each
    runs the planes route, the same bits as the model built and run with every switch off"""
    from m3t import ops
    ref, (plain, _) = reference(True), planes_run(True)
    if kw.get("off"):
        ops.RESNET_V2_CL[0] = True                           # (flipped on, then off again by build(False, ...))
        m = build(False, True)
    elif kw.get("v1_switch"):
        ops.RESNET_CL[0] = True
        m = build(False, True)
    else:
        m = build(True, True, cbam=True)
        base = build(False, True, cbam=True)
        yb = step(base, ref["video"].to(DEV), ref["ct"].to(DEV))
        ops.join_wgrad()
        torch.cuda.synchronize()
        plain = snapshot(base, yb)
        ops.RESNET_V2_CL[0] = True
    assert not m.c3d[0].cl_chain
    y = step(m, ref["video"].to(DEV), ref["ct"].to(DEV))
    ops.join_wgrad()
    torch.cuda.synchronize()
    assert_on_planes(graph_names(y))
    same_bits(snapshot(m, y), plain)


def test_fc_aggregation_is_not_marked_and_fails_where_it_always_did():
    """(module docstring) v2 + 'fc' has no working forward on any route: the switch changes neither the marking nor the place it fails"""
    ref = reference(True)
    for on in (False, True):
        m = build(on, True, agg="fc")
        assert not m.c3d[0].cl_chain and not m.resnet.cl_eligible()
        with pytest.raises(RuntimeError, match="shape|multipl|size"):
            m(ref["video"].to(DEV))
    torch.cuda.synchronize()


def test_a_video_that_requires_grad_stays_on_planes():
    """the chain's first layer has no data gradient: such a video takes the planes route end to end, with that route's video gradient"""
    ref = reference(True)
    outs = []
    for on in (False, True):
        m = build(on, True)
        v = ref["video"].to(DEV).requires_grad_(True)
        y = step(m, v, ref["ct"].to(DEV))
        torch.cuda.synchronize()
        assert_on_planes(graph_names(y))
        outs.append((y.detach(), v.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_uint8_batch_takes_the_cl_layout_and_gives_the_bits_of_the_float32_video(monkeypatch):
    """uint8 frames [2, 3, 56, 48, 3] with a 44-pixel crop, the second clip mirrored: under the switch m3t.video.ingest_for writes the
    channels-last image (a VideoCL) for this front-end, and the output has the bits of the float32 video (x - 127.5) / 127.5 on the same crop"""
    from m3t import ops, video
    m = build(True, False)
    rs = np.random.RandomState(14)
    u8 = torch.from_numpy(rs.randint(0, 256, (2, 3, 56, 48, 3)).astype(np.uint8)).to(DEV)
    aug = [{"cy": 4, "cx": 2, "size": 44, "mirror": False, "cutout": None, "table": None},
           {"cy": 7, "cx": 0, "size": 44, "mirror": True, "cutout": None, "table": None}]
    layouts, real = [], video.ingest

    def spy(frames, aug_, fidx, layout, **k):
        layouts.append(layout)
        return real(frames, aug_, fidx, layout, **k)
    monkeypatch.setattr(video, "ingest", spy)
    with torch.no_grad():
        x = video.ingest_for(m, u8, aug)
        assert isinstance(x, ops.VideoCL)
        a = m(x)
        crops = [u8[0, :, 4:48, 2:46], u8[1, :, 7:51, 0:44].flip(2)]
        f32 = (torch.stack(crops).permute(0, 4, 1, 2, 3).float().contiguous() - 127.5) / 127.5
        b = m(f32)
    torch.cuda.synchronize()
    assert layouts == ["cl"], layouts
    print("\nuint8 route vs float32 route: max |diff| %.3e" % float((a - b).abs().max()))
    assert a.shape == (2, 3, 512) and torch.equal(a, b)


def test_two_fused_adam_steps_match_the_planes_route():
    """models.model.AffWild2VA(backbone='resnet') builds the v1 trunk, as the reference does, so a Trainer step cannot reach v2: instead
    VA_3DResNet(resnet_ver='v2') + its BiGRU head go through two steps of FlatGradDDP + FlatAdam (fused Adam, gradient sinks) on both routes.
    The loss of each step equals the planes route's within 1e-5 relative -- both are fp32 evaluations of one function whose per-tensor errors
    the tests above hold to ~1e-6 -- and the optimizer reaches the BatchNorms that only the fused operator applies"""
    from m3t import ops
    from m3t.ddp import FlatGradDDP
    from m3t.optim import FlatAdam
    rs = np.random.RandomState(41)
    videos = [torch.from_numpy(((rs.randint(0, 256, (2, 3, 3, 52, 44)) - 127.5) / 127.5).astype(np.float32)).to(DEV) for _ in range(2)]
    target = torch.from_numpy(rs.uniform(-1, 1, (2, 3, 2)).astype(np.float32)).to(DEV)
    losses = {}
    for on in (False, True):
        m = build(on, True, backend="gru", hiddenDim=64)
        assert m.c3d[0].cl_chain == on
        ddp = FlatGradDDP(m, flatten_params=True)
        try:
            opt = FlatAdam(ddp)
            bn1, bn5 = m.resnet.layer1[1].bn1.weight, m.resnet.bn5.bias
            was = bn1.detach().clone(), bn5.detach().clone()
            before = dict(ops.STOCK_FALLBACKS)
            losses[on] = []
            for v in videos:
                ddp.zero_grad()
                y = m(v)
                assert any(n.startswith("_AddBNReluCL") for n in graph_names(y)) == on
                loss = ((y - target) ** 2).mean()
                loss.backward()
                norm = ddp.finish()
                opt.step()
                losses[on].append(float(loss.detach()))
            torch.cuda.synchronize()
            ops.poll_scan_error()
            assert all(math.isfinite(v) for v in losses[on]) and math.isfinite(float(ddp.last_norm))
            assert not torch.equal(bn1.detach(), was[0]) and not torch.equal(bn5.detach(), was[1]), "the optimizer step did not reach bn1 / bn5"
            assert {k: v for k, v in ops.STOCK_FALLBACKS.items() if v != before.get(k, 0)} == {}
            assert int(m.resnet.bn5.num_batches_tracked) == 2 and int(m.resnet.layer1[1].bn1.num_batches_tracked) == 2
        finally:
            ddp.close()
    for i, (a, b) in enumerate(zip(losses[True], losses[False])):
        rel = abs(a - b) / abs(b)
        print("\nstep %d: loss chain %.8f  planes %.8f  relative difference %.2e" % (i, a, b, rel))
        assert rel <= 1e-5, (i, a, b)
