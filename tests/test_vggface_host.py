"""`--backbone vggface` on the host side (no GPU): the module contract of models/vggface.py / VA_VGGFace against the reference
(tests/golden/vggface_init.npz, written by gen_golden_vggface.py) -- names, shapes, the init RNG order, AffWild2VA's construction, a strict
checkpoint load -- and the new entry points of csrc/vggface.hip in the header, the ctypes table and the library."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from conftest import load_golden

ENTRY_POINTS = ("m3t_relu_cl_ws_bytes", "m3t_relu_cl_fwd", "m3t_relu_cl_bwd", "m3t_relu_pool_cl_fwd", "m3t_relu_pool_cl_bwd")
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


@pytest.fixture(scope="module")
def seeded():
    """VA_VGGFace() after the fixture's seed (built once: 50 M parameters, an orthogonal and a xavier draw each)"""
    from models.backbone import VA_VGGFace
    g = load_golden("vggface_init")
    torch.manual_seed(int(g["seed"]))
    return VA_VGGFace(), g


def test_vggface_module_imports():
    from models import vggface
    for name in ("VGGFace", "_ConvBlock"):
        assert hasattr(vggface, name), name
    from models.backbone import VA_VGGFace  # noqa: F401


def test_names_and_shapes_match_reference(seeded):
    m, g = seeded
    names, shapes = _names_shapes(m)
    assert names == list(g["va.names"])
    assert shapes == list(g["va.shapes"])
    convs = [x for x in m.modules() if isinstance(x, torch.nn.Conv2d)]
    assert len(convs) == 13 and all(c.weight.dim() == 4 and c.kernel_size == (3, 3) and c.padding == (1, 1) for c in convs)
    assert "vgg.conv3.convs.2.weight" in names and "vgg.fc1.bias" in names


def test_init_digests_match_reference_rng_order(seeded):
    from golden.recipe import grad_digest
    m, g = seeded
    n_checked = 0
    for n, t in m.state_dict().items():
        if not t.dtype.is_floating_point:
            continue
        # per-gate orthogonal weight_hh of the GRU: LAPACK QR rounding depends on the host BLAS (see test_host_api.py)
        atol = 4e-6 if "weight_hh" in n else 1e-7
        np.testing.assert_allclose(grad_digest(t.numpy()), g["sd." + n], rtol=1e-6, atol=atol, err_msg=n)
        n_checked += 1
    assert n_checked == len([k for k in g if k.startswith("sd.")])


@pytest.mark.parametrize("modality", ["visual", "audiovisual"])
def test_affwild2va_builds_vggface_with_reference_keys(modality):
    from models.model import AffWild2VA
    from models.backbone import VA_VGGFace
    g = load_golden("vggface_init")
    a = AffWild2VA(_hp(modality=modality, backbone="vggface"))
    assert isinstance(a.visual, VA_VGGFace)
    names, shapes = _names_shapes(a)
    assert names == list(g["%s.names" % modality])
    assert shapes == list(g["%s.shapes" % modality])


def test_unknown_backbone_still_raises():
    from models.model import AffWild2VA
    with pytest.raises(NotImplementedError):
        AffWild2VA(_hp(modality="visual", backbone="vgg19"))


def test_checkpoint_loads_strictly(seeded, tmp_path):
    from models.backbone import VA_VGGFace
    m, _ = seeded
    path = str(tmp_path / "vggface.ckpt")
    torch.save({"state_dict": m.state_dict()}, path)
    fresh = VA_VGGFace()
    res = fresh.load_state_dict(torch.load(path)["state_dict"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert torch.equal(fresh.vgg.conv5.convs[2].weight, m.vgg.conv5.convs[2].weight) and torch.equal(fresh.vgg.fc1.weight, m.vgg.fc1.weight)


def test_entry_points_declared_bound_and_built():
    from m3t import _lib
    header = open(os.path.join(ROOT, "include", "m3t_hip.h")).read()
    assert "models/vggface.py:45-50" in header
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert _lib.RESTYPES["m3t_relu_cl_ws_bytes"] is _lib.C.c_size_t
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        lib = ctypes.CDLL(_lib.LIB_PATH)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), name


def test_stock_path_of_a_cpu_input():
    """off the chain (a CPU input): the stock operators, announced once; two 36 x 36 frames -> [2, 2048] into a matching fc1"""
    from m3t import ops
    from models.vggface import VGGFace
    torch.manual_seed(3)
    v = VGGFace().eval()
    v.fc1 = torch.nn.Linear(2 * 2 * 512, 32)
    x = torch.randn(2, 3, 36, 36)
    assert not ops.vggface_ok(x)
    n0 = ops.STOCK_FALLBACKS.get("models.vggface.VGGFace", 0)
    with torch.no_grad():
        y = v(x)
        h = x
        for blk in (v.conv1, v.conv2, v.conv3, v.conv4, v.conv5):
            for c in blk.convs:
                h = torch.relu(c(h))
            h = torch.nn.functional.max_pool2d(h, 2, 2, 0, ceil_mode=True)
        ref = torch.relu(v.fc1(h.view(2, -1)))
    assert ops.STOCK_FALLBACKS["models.vggface.VGGFace"] == n0 + 1
    assert y.shape == (2, 32) and torch.equal(y, ref)
