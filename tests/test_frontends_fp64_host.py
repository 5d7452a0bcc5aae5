"""Host side of tests/test_gpu_frontends_fp64.py: the comparison it makes is not blind, and its float64 CBAM (stock operators on the module's
own parameters) is the reference's CBAM."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gpu_frontends_fp64 import biases_before_batchnorm, compare, param_kinds, rel_err, stock_cbam


def _snap(m, y):
    return {"y": [y.detach()], "dx": None, "grads": {n: p.grad.detach().clone() for n, p in m.named_parameters()},
            "buffers": {n: b.detach().clone() for n, b in m.named_buffers()}}


def _conv_bn():
    torch.manual_seed(0)
    m = torch.nn.Sequential(torch.nn.Conv3d(3, 64, 3, bias=False), torch.nn.BatchNorm3d(64)).double().train()
    y = m(torch.randn(2, 3, 3, 6, 6, dtype=torch.float64))
    (y * torch.randn_like(y)).sum().backward()
    ref = _snap(m, y)
    ref.update(kinds=param_kinds(m), n_params=3, n_buffers=3)
    return m, ref


def test_one_percent_in_one_output_channel_fails_the_bar():
    """scale the output channel that holds a compared tensor's largest entry by 1.01: the error is 1e-2 of the tensor's own maximum, ten times
    the loosest bar the GPU test may use"""
    m, ref = _conv_bn()
    assert compare(ref, ref, True, {}) == {k: (0.0, n) for k, (_, n) in compare(ref, ref, True, {}).items()}
    for name in ("0.weight", "1.weight", "1.bias"):
        got = {k: (dict(v) if isinstance(v, dict) else v) for k, v in ref.items()}
        g = ref["grads"][name].clone()
        c = int(np.unravel_index(int(g.abs().argmax()), tuple(g.shape))[0])
        g[c] *= 1.01
        got["grads"] = dict(ref["grads"], **{name: g})
        worst = compare(got, ref, True, {})
        kind = ref["kinds"][name]
        assert worst[kind][1] == name and worst[kind][0] == pytest.approx(0.01, rel=1e-6), worst
        assert worst[kind][0] > 1e-3


def test_the_comparison_is_never_blind():
    m, ref = _conv_bn()
    with pytest.raises(AssertionError):                       # an all-zero reference has no scale
        rel_err(torch.ones(3), torch.zeros(3))
    got = dict(ref, grads={k: v for k, v in ref["grads"].items() if k != "1.bias"})
    with pytest.raises(AssertionError):                       # a gradient left out is not skipped silently
        compare(got, ref, True, {})
    got = dict(ref, grads=dict(ref["grads"], **{"1.bias": None}))
    with pytest.raises(AssertionError):                       # a gradient on one side only
        compare(got, ref, True, {})
    got = dict(ref, buffers=dict(ref["buffers"], **{"1.num_batches_tracked": ref["buffers"]["1.num_batches_tracked"] + 1}))
    with pytest.raises(AssertionError):                       # a counter that moved once too often
        compare(got, ref, True, {})
    assert not (rel_err(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 2.0])) <= 1e-3)     # NaN never passes a bar


def test_conv_biases_in_front_of_batchnorm_are_found():
    from models.backbone import VA_3DVGGM
    zb = biases_before_batchnorm(VA_3DVGGM(backend="none", norm_layer="bn"))
    assert zb == {"v2p.%d.bias" % i: "v2p.%d.weight" % i for i in (0, 4, 8, 12, 15)}
    assert biases_before_batchnorm(VA_3DVGGM(backend="none", norm_layer="gn")) == {}


@pytest.mark.parametrize("name", ["cbam_train", "cbam_eval", "cbam_c64"])
def test_float64_cbam_matches_the_reference_goldens(name):
    """cbam_stock_forward (what the GPU test's float64 copy runs in place of the HIP CBAM) against the reference CBAM's own outputs,
    gradients and running statistics"""
    from models.cbam import CBAM
    g = load_golden(name)
    m = CBAM(g["x"].shape[1])
    with torch.no_grad():
        for n, t in list(m.named_parameters()) + list(m.named_buffers()):
            if "p." + n in g:
                t.copy_(torch.from_numpy(g["p." + n]))
    m = m.double().train(bool(g["training"]))
    assert stock_cbam(m) == 1
    x = torch.tensor(g["x"], dtype=torch.float64, requires_grad=True)
    y = m(x)
    (y * torch.tensor(g["ct"], dtype=torch.float64)).sum().backward()
    assert rel_err(y, torch.from_numpy(g["y"])) <= 1e-5
    assert rel_err(x.grad, torch.from_numpy(g["dx"])) <= 1e-5
    bn = m.SpatialGate.spatial.bn
    assert rel_err(bn.running_mean, torch.from_numpy(g["running_mean_after"])) <= 1e-5
    assert rel_err(bn.running_var, torch.from_numpy(g["running_var_after"])) <= 1e-5
    assert int(bn.num_batches_tracked) == int(bool(g["training"]))
    for n, p in m.named_parameters():
        assert rel_err(p.grad, torch.from_numpy(g["g." + n])) <= 1e-4, n
