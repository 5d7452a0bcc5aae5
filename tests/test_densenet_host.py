"""`--backbone densenet` on the host side (no GPU): the module contract of models/densenet.py / VA_3DDenseNet against the reference
(tests/golden/densenet_*.npz, written by gen_golden_densenet.py) -- names, shapes, the init RNG order, AffWild2VA's construction -- and the
stock-operator path a CPU input takes, forward and backward, against the reference's own run."""
import argparse

import numpy as np
import pytest
import torch

from conftest import load_golden


def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _names_shapes(m):
    items = sorted(list(m.named_parameters()) + list(m.named_buffers()), key=lambda kv: kv[0])
    return [n for n, _ in items], [",".join(str(d) for d in t.shape) for _, t in items]


def _close(got, ref, tol, what):
    got = got.detach().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max())
    assert err <= tol * max(1.0, float(np.abs(ref).max())), (what, err)


def test_densenet_module_imports():
    from models import densenet
    for name in ("_DenseLayer_3D", "_DenseBlock_3D", "_Transition_3D", "DenseNet52_3D"):
        assert hasattr(densenet, name), name
    from models.backbone import VA_3DDenseNet  # noqa: F401


def test_names_and_shapes_match_reference():
    from models.backbone import VA_3DDenseNet
    g = load_golden("densenet_init")
    names, shapes = _names_shapes(VA_3DDenseNet())
    assert names == list(g["va.names"])
    assert shapes == list(g["va.shapes"])
    m = VA_3DDenseNet()
    assert sum(1 for x in m.modules() if isinstance(x, torch.nn.BatchNorm3d)) == 53


@pytest.mark.parametrize("modality", ["visual", "audiovisual"])
def test_affwild2va_builds_densenet_with_reference_keys(modality):
    from models.model import AffWild2VA
    g = load_golden("densenet_init")
    names, shapes = _names_shapes(AffWild2VA(_hp(modality=modality, backbone="densenet")))
    assert names == list(g["%s.names" % modality])
    assert shapes == list(g["%s.shapes" % modality])


def test_init_digests_match_reference_rng_order():
    from models.backbone import VA_3DDenseNet
    from golden.recipe import grad_digest
    g = load_golden("densenet_init")
    torch.manual_seed(int(g["seed"]))
    m = VA_3DDenseNet()
    n_checked = 0
    for n, t in m.state_dict().items():
        if not t.dtype.is_floating_point:
            continue
        # per-gate orthogonal weight_hh of the GRU: LAPACK QR rounding depends on the host BLAS (see test_host_api.py)
        atol = 4e-6 if "weight_hh" in n else 1e-7
        np.testing.assert_allclose(grad_digest(t.numpy()), g["sd." + n], rtol=1e-6, atol=atol, err_msg=n)
        n_checked += 1
    assert n_checked == len([k for k in g if k.startswith("sd.")])


def _model(g, backend=None):
    from models.backbone import VA_3DDenseNet
    from golden.recipe import fill_module
    B, T, S = [int(v) for v in g["dims"]]
    m = fill_module(VA_3DDenseNet(frameLen=T, backend=backend or str(g["backend"]), nClasses=2, nFCs=2, frontend_agg_mode=str(g["agg"])),
                    int(g["seed"]) + 1)
    m = m.train() if int(g["training"]) else m.eval()
    rs = np.random.RandomState(int(g["seed"]))
    x = torch.from_numpy(rs.randint(0, 256, (B, 3, T, S, S)).astype(np.float32))
    return m, ((x - 127.5) / 127.5).requires_grad_(True)


def _check_bn_state(m, g, tol):
    n = 0
    for name, b in m.named_buffers():
        leaf = name.split(".")[-1]
        if leaf not in ("running_mean", "running_var", "num_batches_tracked"):
            continue
        if leaf == "num_batches_tracked":
            assert int(b) == int(g["bn." + name]), name
        else:
            _close(b, g["bn." + name], tol, name)
        n += 1
    return n


@pytest.mark.parametrize("name", ["densenet_eval", "densenet_train"])
def test_cpu_features_match_reference(name):
    """the stock path of a CPU input: the DenseNet's output (the GRU's input, which runs only on the GPU) and, in train mode, every
    BatchNorm buffer after the forward"""
    from models.backbone import VA_3DDenseNet
    g = load_golden(name)
    m, x = _model(g)
    assert isinstance(m, VA_3DDenseNet)
    with torch.no_grad():
        feat = m.densenet(m.c3d(x))
    _close(feat, g["feat"], 1e-5, "feat")
    if int(g["training"]):
        assert _check_bn_state(m, g, 1e-5) == 3 * 53


def test_cpu_forward_backward_match_reference():
    """backend 'none' in train mode: [B, T, 392], every parameter-gradient digest, the input gradient, the BatchNorm buffers"""
    from golden.recipe import grad_digest
    g = load_golden("densenet_feats")
    m, x = _model(g)
    y = m(x)
    _close(y, g["y"], 1e-5, "y")
    (y * torch.from_numpy(g["ct"])).sum().backward()
    n = 0
    for pn, p in m.named_parameters():
        if p.grad is None:                  # (DenseNet52_3D.fc serves agg_mode 'fc' only, as in the reference)
            assert "gd." + pn not in g, pn
            continue
        ref = g["gd." + pn]
        got = grad_digest(p.grad.numpy())
        assert float(np.abs(got - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max())), pn
        n += 1
    assert n == len([k for k in g if k.startswith("gd.")])
    ref = g["dx"]
    assert float(np.abs(grad_digest(x.grad.numpy()) - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    assert _check_bn_state(m, g, 1e-5) == 3 * 53
