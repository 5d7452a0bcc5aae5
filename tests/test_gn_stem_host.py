"""The GroupNorm stems (norm_layer='gn') on the host side (no GPU): the entry points of csrc/gn_cl.hip in the header, the ctypes table and the
library; the module contract of GroupNorm3dReLU inside VA_3DVGGM / VA_3DVGGM_Split against the reference (tests/golden/vggm_gn_init.npz,
written by gen_golden_vggm_gn.py) -- names, shapes, the init RNG order, a strict load of a checkpoint from a plain nn.GroupNorm / nn.ReLU build
-- the stock route of a CPU input; AffWild2VA's norm_layer hparam; and tests/gn_ref.py against torch's float64 autograd."""
import argparse
import os
import re

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gn_ref as R
from conftest import load_golden

ENTRY_POINTS = ("m3t_gn_cl_ws_bytes", "m3t_gn_cl_fwd", "m3t_gn_cl_bwd", "m3t_gn_pool_cl_fwd", "m3t_gn_pool_cl_bwd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _names_shapes(m):
    items = sorted(list(m.named_parameters()) + list(m.named_buffers()), key=lambda kv: kv[0])
    return [n for n, _ in items], [",".join(str(d) for d in t.shape) for _, t in items]


def _ctor(tag):
    from models.backbone import VA_3DVGGM, VA_3DVGGM_Split
    return VA_3DVGGM(norm_layer="gn") if tag == "vggm" else VA_3DVGGM_Split(norm_layer="gn", split_layer=3)


def test_entry_points_declared_bound_and_built():
    from m3t import _lib
    header = open(os.path.join(ROOT, "include", "m3t_hip.h")).read()
    assert "csrc/gn_cl.hip" in header
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.RESTYPES["m3t_gn_cl_ws_bytes"] is _lib.C.c_size_t
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), name


@pytest.mark.parametrize("tag", ["vggm", "split3"])
def test_names_shapes_and_init_digests_match_reference(tag):
    from golden.recipe import grad_digest
    from models.backbone import GroupNorm3dReLU
    g = load_golden("vggm_gn_init")
    torch.manual_seed(int(g["seed"]))
    m = _ctor(tag)
    names, shapes = _names_shapes(m)
    assert names == list(g[tag + ".names"])
    assert shapes == list(g[tag + ".shapes"])
    norms = [x for x in m.modules() if isinstance(x, nn.GroupNorm)]
    assert len(norms) == (5 if tag == "vggm" else 7) and all(isinstance(x, GroupNorm3dReLU) and x.num_groups == 32 for x in norms)
    assert not any(isinstance(x, (nn.ReLU, nn.modules.batchnorm._BatchNorm)) for s in (getattr(m, "v2p", None), getattr(m, "shared", None))
                   if s is not None for x in s)
    n_checked = 0
    for n, t in m.state_dict().items():
        if not t.dtype.is_floating_point:
            continue
        atol = 4e-6 if "weight_hh" in n else 1e-7          # (per-gate orthogonal weight_hh: LAPACK QR rounding depends on the host BLAS)
        np.testing.assert_allclose(grad_digest(t.numpy()), g["%s.sd.%s" % (tag, n)], rtol=1e-6, atol=atol, err_msg=n)
        n_checked += 1
    assert n_checked == len([k for k in g if k.startswith(tag + ".sd.")])


def _plain_stem(norm_channels):
    """the same nn.Sequential from plain nn.GroupNorm / nn.ReLU, as the reference builds it (models/backbone.py:73-103)"""
    mods = []
    cin = 3
    for i, c in enumerate(norm_channels):
        mods += [nn.Conv3d(cin, c, 3, stride=(1, 2, 2) if i == 0 else 1, padding=(1, 0, 0)), nn.GroupNorm(32, c), nn.ReLU(True)]
        if i < 3:
            mods.append(nn.MaxPool3d(kernel_size=(1, 2, 2), stride=(1, 2, 2)))
        cin = c
    return nn.Sequential(*mods)


def test_checkpoint_of_a_plain_groupnorm_build_loads_strictly(tmp_path):
    from models.backbone import VA_3DVGGM
    torch.manual_seed(5)
    plain = _plain_stem([64, 128, 256, 512, 512])
    for p in plain.parameters():
        nn.init.normal_(p)
    path = str(tmp_path / "stem.ckpt")
    torch.save({"state_dict": plain.state_dict()}, path)
    m = VA_3DVGGM(backend="none", norm_layer="gn")
    res = m.v2p.load_state_dict(torch.load(path)["state_dict"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert list(m.v2p.state_dict()) == list(plain.state_dict())
    assert torch.equal(m.v2p[1].weight, plain[1].weight) and torch.equal(m.v2p[15].bias, plain[15].bias)


def test_cpu_input_is_the_stock_route_bit_for_bit():
    from m3t import ops
    from models.backbone import GroupNorm3dReLU
    torch.manual_seed(7)
    gn = GroupNorm3dReLU(32, 64)
    with torch.no_grad():
        gn.weight.normal_()
        gn.bias.normal_()
    x = torch.randn(2, 64, 2, 5, 5) * 0.7 + 3.0
    before = dict(ops.STOCK_FALLBACKS)
    y = gn(x).detach()
    y64 = gn.double()(x.double()).detach()
    assert dict(ops.STOCK_FALLBACKS) == before
    gn.float()
    assert torch.equal(y, F.relu(F.group_norm(x, 32, gn.weight, gn.bias, gn.eps)))
    assert y64.dtype == torch.float64 and float((y64 - y.double()).abs().max()) < 1e-5
    plain = GroupNorm3dReLU(32, 64, affine=False)
    assert torch.equal(plain(x), F.relu(F.group_norm(x, 32, None, None, plain.eps)))
    assert dict(ops.STOCK_FALLBACKS) == before


def test_affwild2va_takes_norm_layer_from_the_hparams():
    from models.model import AffWild2VA
    from models.backbone import GroupNorm3dReLU, BatchNorm3dReLU
    g = load_golden("vggm_gn_init")
    for backbone, tag in (("v2p", "vggm"), ("v2p_split", "split3")):
        a = AffWild2VA(_hp(modality="visual", backbone=backbone, norm_layer="gn", split_layer=3))
        norms = [x for x in a.visual.modules() if isinstance(x, (nn.GroupNorm, nn.BatchNorm3d))]
        assert norms and all(isinstance(x, GroupNorm3dReLU) for x in norms), backbone
        stem = set(n for n in g[tag + ".names"] if n.split(".")[0] in ("v2p", "shared", "v_private", "a_private"))
        assert stem and stem <= set("%s" % n for n, _ in list(a.visual.named_parameters()) + list(a.visual.named_buffers()))
        assert not any("running_mean" in n for n, _ in a.visual.named_buffers())
        b = AffWild2VA(_hp(modality="visual", backbone=backbone, split_layer=3))           # no such attribute: BatchNorm, as before
        assert not hasattr(b.hparams, "norm_layer") or b.hparams.norm_layer == "bn"
        assert any(isinstance(x, BatchNorm3dReLU) for x in b.visual.modules()) and not any(isinstance(x, nn.GroupNorm) for x in b.visual.modules())


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "x".join(map(str, c)))
def test_reference_statement_against_torch_float64_autograd(case):
    """tests/gn_ref.py (forward, the fused pooling with its winner byte, backward) against F.group_norm -> relu -> max_pool3d in float64"""
    N, C, G, T, H, W, k = case
    x, gamma, beta, dout = R.draw(case)
    f = R.forward(x, G, gamma, beta, R.EPS, True, k)
    b = R.backward(dout, x, G, gamma, R.EPS, f, True, k)
    t = R.torch_autograd(x, G, gamma, beta, R.EPS, dout, k)
    out = f["yp"] if k else f["y"]
    assert float((out - t["out"]).abs().max()) <= 1e-13 * float(t["out"].abs().max())
    for kind in ("dx", "dgamma", "dbeta", "colsum"):
        assert float((b[kind] - t[kind]).abs().max()) <= 2e-13 * max(1.0, float(t[kind].abs().max())), kind
    if k:
        # the winner byte: the place of the pooled value in its window, the first of equal values
        w = R._windows(f["y"], k)
        assert torch.equal(w.gather(-1, f["win"].long()[..., None])[..., 0], f["yp"])
        assert torch.equal(R.to_rows(R.from_rows(R.to_rows(x), N, T, H, W)), R.to_rows(x))
    y0 = torch.zeros(1, 4, 1, 2, 2, dtype=torch.float64)
    y0[0, 1, 0, 1, 0] = float("nan")
    y0[0, 2, 0, 0, 1] = 1.0
    y0[0, 2, 0, 1, 1] = 1.0
    _, win = R.pool(y0, 2)
    assert win.flatten().tolist() == [0, 2, 1, 0]          # all equal: the first; NaN wins; two equal maxima: the first
