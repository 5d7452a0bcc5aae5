#!/usr/bin/env python3
"""Generate tests/golden/vggm_gn_*.npz: the reference's VGG-M stems with norm_layer='gn' (models/backbone.py:63-103,165-271: nn.GroupNorm(32, C)
in place of BatchNorm3d), built and run by the REFERENCE itself, imported read-only, on CPU in float32.  Like gen_golden.py it runs only in
the build container; the fixtures are data (names, shapes, digests, outputs).  Weights are never stored: they come from the frozen recipe seed
(recipe.fill_module) on both sides.

  vggm_gn_init    names and shapes of parameters and buffers of VA_3DVGGM(norm_layer='gn') and VA_3DVGGM_Split(norm_layer='gn', split_layer=3),
                  and the digests of their initial weights under torch.manual_seed(12345) (GroupNorm draws nothing: the RNG order is the 'bn' one)
  vggm_gn_b2_t4   VA_3DVGGM(norm_layer='gn', backend='gru') end to end on 2 clips of 4 frames: outputs, the output weights, gradient digests

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_vggm_gn.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden as G                                              # noqa: E402  (sets up the reference import path and stubs)
from models.backbone import VA_3DVGGM, VA_3DVGGM_Split              # noqa: E402  (reference)
from recipe import fill_module, draw, grad_digest                   # noqa: E402

CTORS = {"vggm": lambda: VA_3DVGGM(norm_layer="gn"), "split3": lambda: VA_3DVGGM_Split(norm_layer="gn", split_layer=3)}


def case_init(name, seed=12345):
    out = {}
    for tag, ctor in CTORS.items():
        torch.manual_seed(seed)
        m = ctor()
        items = sorted(list(m.named_parameters()) + list(m.named_buffers()), key=lambda kv: kv[0])
        out[tag + ".names"] = np.array([n for n, _ in items])
        out[tag + ".shapes"] = np.array([",".join(str(d) for d in t.shape) for _, t in items])
        for n, t in m.state_dict().items():
            if t.dtype.is_floating_point:
                out["%s.sd.%s" % (tag, n)] = grad_digest(t.numpy())
    G.save(name, seed=np.array(seed), **out)


def case_vggm_gn(name, seed, B=2, T=4):
    rs = np.random.RandomState(seed)
    m = fill_module(VA_3DVGGM(frameLen=T, backend="gru", nClasses=2, nFCs=2, norm_layer="gn"), seed + 1).eval()
    x = torch.from_numpy(rs.randint(0, 256, (B, 3, T, 112, 112)).astype(np.float32))
    x = (x - 127.5) / 127.5
    y = m(x)
    ct = torch.from_numpy(draw(rs, tuple(y.shape)))
    (y * ct).sum().backward()
    grads = {"gd." + n: grad_digest(p.grad.numpy()) for n, p in m.named_parameters() if p.grad is not None}
    G.save(name, seed=np.array(seed), dims=np.array([B, T]), y=y.detach().numpy(), ct=ct.numpy(),
           param_names=np.array(sorted(n for n, _ in m.named_parameters())), **grads)


def main():
    torch.set_num_threads(8)
    case_init("vggm_gn_init")
    case_vggm_gn("vggm_gn_b2_t4", 1500)


if __name__ == "__main__":
    main()
