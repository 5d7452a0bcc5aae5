#!/usr/bin/env python3
"""Generate tests/golden/pretrain_init.npz, vox2_*.npz and audioset_eval*.npz: the reference's two pre-training task modules
(VoxCeleb2_1k, models/vox2_model.py:25-194; AudioSet, models/audioset_model.py:24-175) and its two checkpoint scripts
(process/export_pretrained_ckpts.py, process/merge_av_checkpoints.py) run by the REFERENCE itself, imported read-only, on CPU in float32.
Like gen_golden.py it runs only in the build container; the fixtures are data (names, shapes, flags, digests, outputs, labels, key lists;
weights come from the frozen recipe seed).  AudioSet runs in eval mode: its head's Dropout draws from torch's RNG.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_pretrain.py
"""
import argparse
import copy
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

# models/audioset_dataset.py imports librosa, models/lr_finder.py matplotlib's pyplot: neither is used by what runs here
sys.modules["librosa"] = types.ModuleType("librosa")
_mpl = types.ModuleType("matplotlib")
_mpl.pyplot = types.ModuleType("matplotlib.pyplot")
sys.modules["matplotlib"] = _mpl
sys.modules["matplotlib.pyplot"] = _mpl.pyplot

import gen_golden as G                                       # noqa: E402  (sets up the reference import path and the cv2 / Lightning stubs)
from models.vox2_model import VoxCeleb2_1k                   # noqa: E402  (reference)
from models.audioset_model import AudioSet                   # noqa: E402  (reference)
from recipe import fill_module, draw, grad_digest            # noqa: E402

save = G.save


def hp(cls, **kw):
    ns = cls.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _names_shapes(m, tag):
    items = sorted(list(m.named_parameters()) + list(m.named_buffers()), key=lambda kv: kv[0])
    return {tag + ".names": np.array([n for n, _ in items]),
            tag + ".shapes": np.array([",".join(str(d) for d in t.shape) for _, t in items])}


def _flags(cls):
    return np.array(sorted("%s=%s" % kv for kv in vars(hp(cls)).items()))


def _run_script(rel, args, produced):
    """a reference script as __main__ on temporary files; returns the keys of the checkpoint it writes, in order"""
    cwd, argv = os.getcwd(), sys.argv
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for i, sd in enumerate(args):
            paths.append(os.path.join(d, "in%d.pt" % i))
            torch.save({"state_dict": sd}, paths[-1])
        os.chdir(d)
        sys.argv = [rel] + paths
        try:
            with open(os.devnull, "w") as null:
                out, sys.stdout = sys.stdout, null
                try:
                    runpy.run_path(os.path.join(G.REF, rel), run_name="__main__")
                finally:
                    sys.stdout = out
            ck = torch.load(os.path.join(d, produced))
        finally:
            os.chdir(cwd)
            sys.argv = argv
    return ck["state_dict"]


def case_init(name, seed=12345):
    out = {}
    torch.manual_seed(seed)
    vox = VoxCeleb2_1k(hp(VoxCeleb2_1k))
    torch.manual_seed(seed)
    aud = AudioSet(hp(AudioSet))
    for tag, m in (("vox", vox), ("aud", aud)):
        out.update(_names_shapes(m, tag))
        for n, t in m.state_dict().items():
            if t.dtype.is_floating_point:
                out["sd.%s.%s" % (tag, n)] = grad_digest(t.numpy())
    out["vox.flags"], out["aud.flags"] = _flags(VoxCeleb2_1k), _flags(AudioSet)
    video = _run_script("process/export_pretrained_ckpts.py", [vox.state_dict()], "video_checkpoint.pt")
    out["export.keys"] = np.array(list(video.keys()))
    fused = _run_script("process/merge_av_checkpoints.py", [aud.state_dict(), video], "fused_av.pt")
    out["merge.keys"] = np.array(list(fused.keys()))
    # the same merge with a trained visual AffWild2VA as its video side: the towers' own classifier heads go too
    va = G.AffWild2VA(G.hp(modality="visual", backbone="v2p_split", split_layer=3))
    fused = _run_script("process/merge_av_checkpoints.py", [aud.state_dict(), va.state_dict()], "fused_av.pt")
    out["merge_va.keys"] = np.array(list(fused.keys()))
    save(name, seed=np.array(seed), **out)


def _grads(m):
    return {"gd." + n: grad_digest(p.grad.numpy()) for n, p in m.named_parameters() if p.grad is not None}


def case_vox2(name, seed, B, T, S, training):
    """VoxCeleb2_1k (v2p + fc) on a seeded clip batch: the pooled logits (forward's output inside training_step), training_step's loss and
    train_acc, every parameter-gradient digest, the BatchNorm buffers after the step, then (eval mode) validation_step.  Clip 0 is labelled with its
    own top-1 class (found on a copy of the module, so that no buffer moves), clip 1.. with a seeded class: train_acc is 1 / B."""
    rs = np.random.RandomState(seed)
    m = fill_module(VoxCeleb2_1k(hp(VoxCeleb2_1k, window=T)), seed + 1)
    m = m.train() if training else m.eval()
    x = torch.from_numpy(rs.randint(0, 256, (B, 3, T, S, S)).astype(np.float32))
    label = rs.randint(0, 1000, (B,)).astype(np.int64)
    with torch.no_grad():
        y0 = copy.deepcopy(m)(x)
    label[0] = int(y0[0].argmax())
    for b in range(1, B):
        if label[b] == int(y0[b].argmax()):
            label[b] = (label[b] + 1) % 1000
    got = {}
    h = m.visual.register_forward_hook(lambda mod, inp, out: got.update(y=out.detach().numpy().copy()) if "y" not in got else None)
    batch = {"video": x, "label": torch.from_numpy(label)}
    out = m.training_step(batch, 0)
    out["loss"].backward()
    h.remove()
    extra = G._bn_state(m) if training else {}
    if not training:
        with torch.no_grad():
            val = m.validation_step(batch, 0)
        extra.update(val_loss=np.array(float(val["val_loss"])), correct=val["correct"].numpy().astype(np.float32))
    save(name, seed=np.array(seed), dims=np.array([B, T, S]), training=np.array(int(training)), label=label, y=got["y"],
         loss=np.array(float(out["loss"])), train_acc=np.array(float(out["log"]["train_acc"])), **_grads(m), **extra)


def case_audioset(name, seed, B, T, H):
    """AudioSet in eval mode: per-clip logits, the frame of each maximum, training_step's loss and train_acc, gradient digests.  Multi-hot
    targets with a few ones per row; row 0 also has its top-1 class set (train_acc >= 1 / B)."""
    rs = np.random.RandomState(seed)
    m = fill_module(AudioSet(hp(AudioSet, num_hidden=H, window=T)), seed + 1).eval()
    x = torch.from_numpy(draw(rs, (B, T, 200)))
    target = (rs.uniform(size=(B, 527)) < 0.01).astype(np.float32)
    got = {}
    h = m.audio.register_forward_hook(lambda mod, inp, out: got.__setitem__("z", out.detach()))
    with torch.no_grad():
        y0 = m(x)
    got.clear()
    target[0, int(y0[0].argmax())] = 1.0
    batch = {"audio": x, "label": torch.from_numpy(target)}
    out = m.training_step(batch, 0)
    out["loss"].backward()
    pooled, arg = got["z"].max(dim=1)
    h.remove()
    with torch.no_grad():
        val = m.validation_step(batch, 0)
    save(name, seed=np.array(seed), dims=np.array([B, T, H]), target=target, y=pooled.numpy(), arg=arg.numpy().astype(np.int32),
         loss=np.array(float(out["loss"])), train_acc=np.array(float(out["log"]["train_acc"])), val_loss=np.array(float(val["val_loss"])),
         correct=val["correct"].numpy().astype(np.float32), **_grads(m))


def main():
    torch.set_num_threads(8)
    case_init("pretrain_init")
    case_vox2("vox2_train", 1400, 2, 4, 112, training=True)
    case_vox2("vox2_eval", 1410, 2, 4, 112, training=False)
    case_audioset("audioset_eval", 1420, 3, 8, 16)
    case_audioset("audioset_eval_h256", 1430, 2, 5, 256)


if __name__ == "__main__":
    main()
