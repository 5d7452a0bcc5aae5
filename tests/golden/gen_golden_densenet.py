#!/usr/bin/env python3
"""Generate tests/golden/densenet_*.npz: the reference's `--backbone densenet` visual tower (VA_3DDenseNet, models/backbone.py:375-423,
models/densenet.py:5-93) run by the REFERENCE itself, imported read-only, on CPU in float32.  Like gen_golden.py it runs only in the build
container; the fixtures are data (outputs, the output weights `ct`, gradient digests, BatchNorm buffers; weights come from the frozen recipe
seed).  Dropout3d(p=0) draws no random numbers, so the train-mode cases are deterministic.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_densenet.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden as G                                       # noqa: E402  (sets up the reference import path and stubs)
from models.backbone import VA_3DDenseNet                    # noqa: E402  (reference)
from recipe import fill_module, draw, grad_digest            # noqa: E402

save, hp = G.save, G.hp


def _video(rs, B, T, S):
    x = torch.from_numpy(rs.randint(0, 256, (B, 3, T, S, S)).astype(np.float32))
    return (x - 127.5) / 127.5


def case_densenet(name, seed, B, T, S, training, backend="gru", agg="ap"):
    """VA_3DDenseNet(nClasses=2, nFCs=2) on a seeded video: y, ct, the DenseNet's own output `feat` (the GRU's input), every parameter-gradient
    digest, the input-gradient digest and (train mode) every BatchNorm buffer after the step"""
    rs = np.random.RandomState(seed)
    m = fill_module(VA_3DDenseNet(frameLen=T, backend=backend, nClasses=2, nFCs=2, frontend_agg_mode=agg), seed + 1)
    m = m.train() if training else m.eval()
    x = _video(rs, B, T, S).requires_grad_(True)
    feats = {}
    h = m.densenet.register_forward_hook(lambda mod, inp, out: feats.__setitem__("feat", out.detach().numpy().copy()))
    y = m(x)
    h.remove()
    ct = torch.from_numpy(draw(rs, tuple(y.shape)))
    (y * ct).sum().backward()
    grads = {"gd." + n: grad_digest(p.grad.numpy()) for n, p in m.named_parameters() if p.grad is not None}
    extra = G._bn_state(m) if training else {}
    save(name, seed=np.array(seed), dims=np.array([B, T, S]), training=np.array(int(training)), backend=np.array(backend),
         agg=np.array(agg), y=y.detach().numpy(), ct=ct.numpy(), feat=feats["feat"], dx=grad_digest(x.grad.numpy()),
         param_names=np.array(sorted(n for n, _ in m.named_parameters())), **extra, **grads)


def _names_shapes(m, tag):
    items = sorted(list(m.named_parameters()) + list(m.named_buffers()), key=lambda kv: kv[0])
    return {tag + ".names": np.array([n for n, _ in items]),
            tag + ".shapes": np.array([",".join(str(d) for d in t.shape) for _, t in items])}


def case_init(name, seed=12345):
    """state_dict digests after torch.manual_seed(seed); VA_3DDenseNet() (the reference's init order: DenseNet52_3D's own init, then
    VA_3DDenseNet._initialize_weights, the GRU's in between), and the names and shapes of VA_3DDenseNet and of AffWild2VA(backbone='densenet')
    visual and audiovisual (the checkpoint contract)"""
    out = {}
    torch.manual_seed(seed)
    m = VA_3DDenseNet()
    for n, t in m.state_dict().items():
        if t.dtype.is_floating_point:
            out["sd." + n] = grad_digest(t.numpy())
    out.update(_names_shapes(m, "va"))
    for mod in ("visual", "audiovisual"):
        torch.manual_seed(seed)
        a = G.AffWild2VA(hp(modality=mod, backbone="densenet"))
        out.update(_names_shapes(a, mod))
    save(name, seed=np.array(seed), **out)


def main():
    torch.set_num_threads(8)
    case_init("densenet_init")
    case_densenet("densenet_eval", 1300, 2, 4, 112, training=False)
    case_densenet("densenet_train", 1310, 2, 4, 112, training=True)
    case_densenet("densenet_small_train", 1320, 1, 3, 80, training=True)
    case_densenet("densenet_feats", 1330, 2, 4, 112, training=True, backend="none")
    case_densenet("densenet_fc", 1340, 2, 4, 112, training=False, agg="fc")


if __name__ == "__main__":
    main()
