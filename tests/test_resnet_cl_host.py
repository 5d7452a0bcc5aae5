"""Host side of the per-frame ResNet (v1) on the channels-last chain (M3T_RESNET_CL=1): no GPU.

  * tests/resnet_ref.py -- the float64 restatement the GPU tests compare the kernels with -- agrees with torch's float64 autograd on the CPU:
    relu(bn(x) + s) forward / backward in train and eval mode, with gamma = 0 (the model's initial state), and the spatial mean;
  * the operator cases and the whole-model video find an input clear of ReLU / pooling flips within 8 seeds, from the float64 values alone;
  * with ops.RESNET_CL[0] on, VA_3DResNet(resnet_ver='v1') is the same module (tree, state_dict keys, parameter values for a seed) and its CPU
    forward is unchanged: the chain is not taken;
  * ops.bn_add_relu_cl / ops.mean_cl refuse CPU tensors and mismatched grids with M3THipError before touching a device."""
import pytest
import torch

import resnet_ref as R


def _close(a, b, tol=1e-12):
    top = float(b.abs().max())
    return float((a - b).abs().max()) <= tol * max(top, 1e-300) or (top == 0.0 and not bool(a.any()))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("zero_gamma", [False, True], ids=["gamma", "gamma0"])
@pytest.mark.parametrize("case", [(3, 64), (130, 8), (24, 512)], ids=lambda c: "x".join(map(str, c)))
def test_tail_reference_agrees_with_torch_float64(case, zero_gamma, training):
    x, s, gamma, beta, rm, rv, dy = R.draw(case, 5, zero_gamma)
    f = R.forward(x, s, gamma, beta, rm, rv, training)
    b = R.backward(dy, f, gamma, training)
    t = R.torch_autograd(x, s, gamma, beta, rm, rv, training, dy)
    assert _close(f["y"], t["out"])
    for kind in ("dx", "ds", "dgamma", "dbeta"):
        assert _close(b[kind], t[kind], 1e-10), kind
    # dx's column sums: zero by construction in train mode (the normalisation removes the batch mean) -- rounding noise against the terms' size
    scale = float(t["dx"].abs().sum(0).max())
    assert float((b["colsum"] - t["colsum"]).abs().max()) <= 1e-12 * max(scale, 1e-300)
    if training and not zero_gamma:
        assert float(b["colsum"].abs().max()) <= 1e-12 * scale
    assert _close(f["run_mean"], t["run_mean"]) and _close(f["run_var"], t["run_var"])
    if not training:
        assert torch.equal(f["run_mean"], rm) and torch.equal(f["run_var"], rv)
    if zero_gamma:
        assert torch.equal(f["y"], torch.relu(s)) and not bool(b["dx"].any()) and bool(torch.isfinite(b["dgamma"]).all())


@pytest.mark.parametrize("case", R.MEAN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_mean_reference_agrees_with_torch_float64(case):
    x, dy = R.draw_mean(case)
    P, HW, C = case
    xt = x.clone().requires_grad_(True)
    # [P, HW, C] rows are the frames [P, C, H, W] channels-last: AdaptiveAvgPool2d(1) + flatten of the planes
    y = torch.nn.AdaptiveAvgPool2d(1)(xt.transpose(1, 2).reshape(P, C, HW, 1)).flatten(1)
    y.backward(dy)
    assert _close(R.mean_forward(x), y.detach()) and _close(R.mean_backward(dy, HW), xt.grad)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", R.TAIL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_operator_cases_find_a_clear_draw_within_the_cap(case, training):
    inputs, taken = R.draw_clear(case, training)
    print("\n%s %s: seed %d taken" % (case, "train" if training else "eval", taken))
    assert taken < 8000


def _model(depth=18, ver="v1", cbam=False, agg="ap", seed=None):
    from models.backbone import VA_3DResNet
    if seed is not None:
        torch.manual_seed(seed)
    return VA_3DResNet(frameLen=3, backend="none", resnet_ver=ver, use_cbam=cbam, resnet_depth=depth, frontend_agg_mode=agg)


@pytest.fixture
def switch_on():
    from m3t import ops
    was = ops.RESNET_CL[0]
    ops.RESNET_CL[0] = True
    yield ops
    ops.RESNET_CL[0] = was


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_model_video_found_within_the_cap(training):
    """the whole-model GPU test's selection (tests/test_gpu_resnet_cl_model.py), run here for the float64 reference alone"""
    from golden.recipe import fill_module
    m = fill_module(_model(), 31).double().train(training)
    video, taken = R.pick_video(m, 0)
    print("\n%s: video seed %d taken" % ("train" if training else "eval", taken))
    assert taken < 8000 and tuple(video.shape) == R.VIDEO_SHAPE


def test_switch_leaves_the_module_and_its_cpu_forward_unchanged(switch_on):
    ops = switch_on
    assert ops.RESNET_CL[0]
    on = _model(seed=3)
    ops.RESNET_CL[0] = False
    off = _model(seed=3)
    ops.RESNET_CL[0] = True
    assert on.c3d[0].cl_chain and not off.c3d[0].cl_chain
    assert [(n, type(m).__name__) for n, m in on.named_modules()] == [(n, type(m).__name__) for n, m in off.named_modules()]
    sd_on, sd_off = on.state_dict(), off.state_dict()
    assert list(sd_on) == list(sd_off)
    for k in sd_on:
        assert torch.equal(sd_on[k], sd_off[k]), k
    assert all(float(m.bn2.weight.detach().abs().max()) == 0.0 for m in on.modules() if type(m).__name__ == "BasicBlock")      # zero_init_residual
    video = R.draw_video(1).float()
    before = dict(ops.STOCK_FALLBACKS)
    for training in (True, False):
        on.train(training), off.train(training)
        y_on, y_off = on(video), off(video)
        assert y_on.shape == (2, 3, 512) and torch.equal(y_on, y_off)
    assert ops.STOCK_FALLBACKS != before             # (the CPU forward is the stock route, and says so)
    for k in sd_on:
        assert torch.equal(on.state_dict()[k], off.state_dict()[k]), k


@pytest.mark.parametrize("kw", [dict(ver="v2"), dict(cbam=True), dict(agg="fc")], ids=["v2", "cbam", "fc"])
def test_only_the_eligible_trunk_is_marked_for_the_chain(switch_on, kw):
    assert not _model(**kw).c3d[0].cl_chain
    assert _model(depth=34).c3d[0].cl_chain and _model(depth=34).resnet.cl_eligible()


def test_operators_refuse_cpu_tensors_and_mismatched_grids(monkeypatch):
    from m3t import ops
    from m3t._lib import M3THipError

    def touched(*a, **k):
        raise AssertionError("the refusal came after the library / a device allocation was reached")
    for name in ("lib", "amax_slots", "workspace"):
        monkeypatch.setattr(ops, name, touched)
    C = 64
    cl = lambda rows, N, T, H, W, c=C: ops.CLTensor(torch.zeros(rows, c), N, T, H, W)
    vec = [torch.ones(C), torch.zeros(C), torch.zeros(C), torch.ones(C)]
    with pytest.raises(M3THipError, match="device"):
        ops.bn_add_relu_cl(cl(12, 1, 2, 2, 3), cl(12, 1, 2, 2, 3), *vec, True, 0.1, 1e-5)
    with pytest.raises(M3THipError, match="grid"):
        ops.bn_add_relu_cl(cl(12, 1, 2, 2, 3), cl(12, 1, 2, 3, 2), *vec, True, 0.1, 1e-5)
    with pytest.raises(M3THipError, match="grid"):
        ops.bn_add_relu_cl(cl(12, 1, 2, 2, 3), cl(12, 1, 2, 2, 3, 128), *vec, True, 0.1, 1e-5)
    with pytest.raises(M3THipError, match="CLTensor"):
        ops.bn_add_relu_cl(cl(12, 1, 2, 2, 3), torch.zeros(12, C), *vec, True, 0.1, 1e-5)
    with pytest.raises(M3THipError, match="device"):
        ops.mean_cl(cl(12, 1, 2, 2, 3))
    with pytest.raises(M3THipError, match="CLTensor"):
        ops.mean_cl(torch.zeros(12, C))
