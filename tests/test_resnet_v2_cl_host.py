"""Host side of the per-frame ResNet v2 (pre-activation) on the channels-last chain (M3T_RESNET_V2_CL=1): no GPU.

  * tests/resnet_v2_ref.py -- the float64 restatement the GPU tests compare the kernels with -- agrees with torch's float64 autograd on the CPU:
    s = a + b, z = relu(bn(s)) forward / backward in train and eval mode, with and without ds_out, and with gamma = 0;
  * the six operator cases take seed 0 in both modes, and resnet_ref.pick_video, unchanged, takes seed 0 for a v2 float64 module;
  * ops.add_bn_relu_cl refuses what it does not cover with M3THipError before the library, a slot or a workspace is reached;
  * with ops.RESNET_V2_CL[0] on, VA_3DResNet(resnet_ver='v2') is marked for the chain (depth 18 and 34) and is the same module (tree,
    state_dict, CPU forward) as with the switch off; use_cbam=True, 'fc' and resnet_ver='v1' are not marked by this switch."""
import pytest
import torch

import resnet_ref as R
import resnet_v2_ref as V


def _close(a, b, tol=1e-12):
    top = float(b.abs().max())
    return float((a - b).abs().max()) <= tol * max(top, 1e-300) or (top == 0.0 and not bool(a.any()))


@pytest.mark.parametrize("with_ds_out", [True, False], ids=["ds_out", "no_ds_out"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("zero_gamma", [False, True], ids=["gamma", "gamma0"])
@pytest.mark.parametrize("case", [(3, 64), (130, 8), (24, 512), (2, 4)], ids=lambda c: "x".join(map(str, c)))
def test_reference_agrees_with_torch_float64(case, zero_gamma, training, with_ds_out):
    a, b, gamma, beta, rm, rv, dz, ds_out = V.draw(case, 5)
    if zero_gamma:
        gamma = torch.zeros_like(gamma)
    if not with_ds_out:
        ds_out = None
    f = V.forward(a, b, gamma, beta, rm, rv, training)
    g = V.backward(dz, ds_out, f, gamma, training)
    t = V.torch_autograd(a, b, gamma, beta, rm, rv, training, dz, ds_out)
    assert torch.equal(f["s"], t["s"]) and _close(f["z"], t["z"])
    assert torch.equal(t["ds"], t["ds_b"])                 # (one gradient for both addends)
    for kind in ("ds", "dgamma", "dbeta"):
        assert _close(g[kind], t[kind], 1e-10), kind
    # the BatchNorm part of ds's column sums is zero by construction in train mode: rounding noise against the size of the terms
    scale = float(t["ds"].abs().sum(0).max())
    if scale > 0.0:
        assert float((g["colsum"] - t["colsum"]).abs().max()) <= 1e-12 * scale
    if training and not with_ds_out and not zero_gamma:
        assert float(g["colsum"].abs().max()) <= 1e-12 * scale
    assert _close(f["run_mean"], t["run_mean"]) and _close(f["run_var"], t["run_var"])
    if not training:
        assert torch.equal(f["run_mean"], rm) and torch.equal(f["run_var"], rv)
    if zero_gamma:
        assert torch.equal(f["z"], torch.relu(beta).expand_as(f["z"])) and bool(torch.isfinite(g["dgamma"]).all())
        assert torch.equal(g["ds"], ds_out) if with_ds_out else not bool(g["ds"].any())


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", V.CASES, ids=lambda c: "x".join(map(str, c)))
def test_operator_cases_take_seed_zero(case, training):
    inputs, taken = V.draw_clear(case, training)
    print("\n%s %s: seed %d taken" % (case, "train" if training else "eval", taken))
    assert taken == 0 and len(inputs) == 8 and inputs[7].shape == inputs[0].shape


def _model(depth=18, ver="v2", cbam=False, agg="ap", seed=None):
    from models.backbone import VA_3DResNet
    if seed is not None:
        torch.manual_seed(seed)
    return VA_3DResNet(frameLen=3, backend="none", resnet_ver=ver, use_cbam=cbam, resnet_depth=depth, frontend_agg_mode=agg)


@pytest.fixture
def switch_on():
    from m3t import ops
    was = ops.RESNET_V2_CL[0], ops.RESNET_CL[0]
    ops.RESNET_V2_CL[0], ops.RESNET_CL[0] = True, False
    yield ops
    ops.RESNET_V2_CL[0], ops.RESNET_CL[0] = was


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_model_video_takes_seed_zero(training):
    """the whole-model GPU test's selection (tests/test_gpu_resnet_v2_cl_model.py), run here for the float64 reference alone: pick_video hooks
    every PlaneBatchNorm2d with fuse_relu -- all of v2's BatchNorms -- and the stem"""
    from golden.recipe import fill_module
    from models.resnet import PlaneBatchNorm2d
    m = fill_module(_model(), 31).double().train(training)
    assert all(bn.fuse_relu for bn in m.modules() if isinstance(bn, PlaneBatchNorm2d))
    video, taken = R.pick_video(m, 0)
    print("\n%s: video seed %d taken" % ("train" if training else "eval", taken))
    assert taken == 0 and tuple(video.shape) == R.VIDEO_SHAPE


@pytest.mark.parametrize("depth", [18, 34])
def test_the_v2_trunk_is_marked_for_the_chain(switch_on, depth):
    m = _model(depth=depth)
    assert m.c3d[0].cl_chain and m.resnet.cl_eligible()


@pytest.mark.parametrize("kw", [dict(cbam=True), dict(agg="fc"), dict(ver="v1")], ids=["cbam", "fc", "v1"])
def test_the_switch_marks_nothing_else(switch_on, kw):
    assert not _model(**kw).c3d[0].cl_chain
    if kw.get("ver") != "v1":
        assert not _model(**kw).resnet.cl_eligible()


def test_the_v1_switch_does_not_mark_v2(switch_on):
    ops = switch_on
    ops.RESNET_V2_CL[0], ops.RESNET_CL[0] = False, True
    assert not _model().c3d[0].cl_chain and _model(ver="v1").c3d[0].cl_chain


def test_switch_leaves_the_module_and_its_cpu_forward_unchanged(switch_on):
    ops = switch_on
    on = _model(seed=3)
    ops.RESNET_V2_CL[0] = False
    off = _model(seed=3)
    ops.RESNET_V2_CL[0] = True
    assert on.c3d[0].cl_chain and not off.c3d[0].cl_chain
    assert [(n, type(m).__name__) for n, m in on.named_modules()] == [(n, type(m).__name__) for n, m in off.named_modules()]
    sd_on, sd_off = on.state_dict(), off.state_dict()
    assert list(sd_on) == list(sd_off)
    for k in sd_on:
        assert torch.equal(sd_on[k], sd_off[k]), k
    video = R.draw_video(1).float()
    before = dict(ops.STOCK_FALLBACKS)
    for training in (True, False):
        on.train(training), off.train(training)
        y_on, y_off = on(video), off(video)
        assert y_on.shape == (2, 3, 512) and torch.equal(y_on, y_off)
    assert ops.STOCK_FALLBACKS != before             # (the CPU forward is the stock route, and says so)
    for k in sd_on:
        assert torch.equal(on.state_dict()[k], off.state_dict()[k]), k
    assert int(on.resnet.bn5.num_batches_tracked) == 1 and int(on.resnet.layer1[1].bn1.num_batches_tracked) == 1


def test_operator_refuses_before_anything_is_touched(monkeypatch):
    from m3t import ops
    from m3t._lib import M3THipError

    def touched(*a, **k):
        raise AssertionError("the refusal came after the library / a device allocation was reached")
    for name in ("lib", "amax_slots", "workspace"):
        monkeypatch.setattr(ops, name, touched)
    C = 64
    cl = lambda rows, N, T, H, W, c=C, dt=torch.float32: ops.CLTensor(torch.zeros(rows, c, dtype=dt), N, T, H, W)
    vec = [torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C)]
    for training in (True, False):
        with pytest.raises(M3THipError, match="device"):
            ops.add_bn_relu_cl(cl(12, 1, 2, 2, 3), cl(12, 1, 2, 2, 3), *vec, training, 0.1, 1e-5)
        with pytest.raises(M3THipError, match="device"):
            ops.add_bn_relu_cl(cl(12, 1, 2, 2, 3, dt=torch.float64), cl(12, 1, 2, 2, 3, dt=torch.float64), *vec, training, 0.1, 1e-5)
        with pytest.raises(M3THipError, match="grid"):
            ops.add_bn_relu_cl(cl(12, 1, 2, 2, 3), cl(12, 1, 2, 3, 2), *vec, training, 0.1, 1e-5)
        with pytest.raises(M3THipError, match="grid"):
            ops.add_bn_relu_cl(cl(12, 1, 2, 2, 3), cl(12, 1, 2, 2, 3, 128), *vec, training, 0.1, 1e-5)
        with pytest.raises(M3THipError, match="CLTensor"):
            ops.add_bn_relu_cl(cl(12, 1, 2, 2, 3), torch.zeros(12, C), *vec, training, 0.1, 1e-5)
        with pytest.raises(M3THipError, match="CLTensor"):
            ops.add_bn_relu_cl(torch.zeros(12, C), cl(12, 1, 2, 2, 3), *vec, training, 0.1, 1e-5)
    # channel counts the BatchNorm kernels do not cover are refused on the shape alone -- the check sits behind the device check, so the tensors
    # claim a device they do not live on
    class OnDevice:
        is_cuda, dtype = True, torch.float32

        def __init__(self, c):
            self.shape = (12, c)
    for c in (6, 24, 2048):
        bad = lambda: ops.CLTensor(OnDevice(c), 1, 2, 2, 3)
        with pytest.raises(M3THipError, match="C = %d" % c):
            ops.add_bn_relu_cl(bad(), bad(), *vec, True, 0.1, 1e-5)


def test_resnet_v2_cl_ok_follows_its_own_switch(switch_on):
    ops = switch_on
    x = ops.CLTensor(torch.zeros(12, 64), 1, 2, 2, 3)
    assert not ops.resnet_v2_cl_ok(x) and not ops.resnet_v2_cl_ok(torch.zeros(12, 64))      # (a CPU tensor, a plain tensor)
    assert not ops.resnet_cl_ok(x)
