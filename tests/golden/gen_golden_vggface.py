#!/usr/bin/env python3
"""Generate tests/golden/vggface_*.npz: the reference's `--backbone vggface` visual tower (VA_VGGFace, models/backbone.py:16-59,
models/vggface.py) run by the REFERENCE itself, imported read-only, on CPU in float32 -- and once more in float64, so that every stored
quantity comes with the reference's own float32-to-float64 gap (`y64`, `feat64`, `gd64.*`).  Like gen_golden.py it runs only in the build
container; the fixtures are data (outputs, the output weights `ct`, gradient digests).  Weights are never stored: they come from the frozen
recipe seed (recipe.fill_module) on both sides.  The recipe's scales (weights ~ N(0, 1 / fan_in), biases ~ 0.1 N(0, 1)) carry the thirteen
unnormalised layers without vanishing or exploding: main() checks that max |feat| and max |y| stay inside 1e-3 .. 1e3 and refuses to write
otherwise.

Backward runs in eval mode, so nn.Dropout draws nothing (torch's CPU dropout stream cannot match the library's Philox mask: there is no
train-mode golden).  The video is not an autograd leaf: the first layer's input has no gradient on the channels-last chain, so no `dx` digest.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_vggface.py
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden as G                                       # noqa: E402  (sets up the reference import path and stubs)
from models.backbone import VA_VGGFace                       # noqa: E402  (reference)
from recipe import fill_module, draw, grad_digest            # noqa: E402

save, hp = G.save, G.hp


def _video(rs, B, T, S):
    x = torch.from_numpy(rs.randint(0, 256, (B, 3, T, S, S)).astype(np.float32))
    return (x - 127.5) / 127.5


def _run(m, x, ct):
    feats = {}
    h = m.vgg.fc1.register_forward_hook(lambda mod, inp, out: feats.__setitem__("feat", out.detach().numpy().copy()))
    y = m(x)
    h.remove()
    (y * ct).sum().backward()
    grads = {n: grad_digest(p.grad.numpy()) for n, p in m.named_parameters() if p.grad is not None}
    return y.detach().numpy(), feats["feat"], grads


def case_vggface(name, seed, B, T, S):
    """VA_VGGFace(hiddenDim=64, nClasses=2, nFCs=2).eval() on a seeded video: y, ct, the output of `fc1` (before ReLU and dropout), every
    parameter-gradient digest -- in float32 and, from the same weights and inputs, in float64"""
    rs = np.random.RandomState(seed)
    m = fill_module(VA_VGGFace(hiddenDim=64, frameLen=T, nClasses=2, nFCs=2), seed + 1).eval()
    x = _video(rs, B, T, S)
    m64 = copy.deepcopy(m).double()
    ct = None
    with torch.no_grad():
        ct = torch.from_numpy(draw(rs, tuple(m(x).shape)))
    y, feat, grads = _run(m, x, ct)
    y64, feat64, grads64 = _run(m64, x.double(), ct.double())
    for what, v in (("feat", feat), ("y", y)):
        mx = float(np.abs(v).max())
        if not 1e-3 <= mx <= 1e3:
            raise SystemExit("%s: max |%s| = %g is outside 1e-3 .. 1e3: the recipe's scales do not carry this network" % (name, what, mx))
    out = {"gd." + n: d for n, d in grads.items()}
    out.update({"gd64." + n: d for n, d in grads64.items()})
    save(name, seed=np.array(seed), dims=np.array([B, T, S]), y=y, ct=ct.numpy(), feat=feat, y64=y64, feat64=feat64,
         param_names=np.array(sorted(n for n, _ in m.named_parameters())), **out)
    print("%s: max|y| %.3g max|feat| %.3g  fp32-fp64 gap: y %.3g feat %.3g gd %.3g" % (
        name, np.abs(y).max(), np.abs(feat).max(), np.abs(y - y64).max() / max(1.0, np.abs(y64).max()),
        np.abs(feat - feat64).max() / max(1.0, np.abs(feat64).max()),
        max(np.abs(grads[n] - grads64[n]).max() / max(1.0, np.abs(grads64[n]).max()) for n in grads)))


def _names_shapes(m, tag):
    items = sorted(list(m.named_parameters()) + list(m.named_buffers()), key=lambda kv: kv[0])
    return {tag + ".names": np.array([n for n, _ in items]),
            tag + ".shapes": np.array([",".join(str(d) for d in t.shape) for _, t in items])}


def case_init(name, seed=12345):
    """state_dict digests after torch.manual_seed(seed); VA_VGGFace() (the reference's init order: the layers' own draws in creation order, the
    GRU's, then VA_VGGFace._initialize_weights), and the names and shapes of VA_VGGFace and of AffWild2VA(backbone='vggface') visual and
    audiovisual (the checkpoint contract)"""
    out = {}
    torch.manual_seed(seed)
    m = VA_VGGFace()
    for n, t in m.state_dict().items():
        if t.dtype.is_floating_point:
            out["sd." + n] = grad_digest(t.numpy())
    out.update(_names_shapes(m, "va"))
    for mod in ("visual", "audiovisual"):
        torch.manual_seed(seed)
        a = G.AffWild2VA(hp(modality=mod, backbone="vggface"))
        out.update(_names_shapes(a, mod))
    save(name, seed=np.array(seed), **out)


def main():
    torch.set_num_threads(8)
    case_init("vggface_init")
    case_vggface("vggface_eval_112", 1400, 1, 2, 112)
    case_vggface("vggface_eval_100", 1410, 2, 3, 100)


if __name__ == "__main__":
    main()
