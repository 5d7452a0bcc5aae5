#!/usr/bin/env python3
"""Time the two pre-training tasks on one MI355X at the reference's default shapes: VoxCeleb2_1k at 128 clips x 16 frames of 112 x 112
(models/vox2_model.py) and AudioSet at 128 x 32 x 200, num_hidden 256 (models/audioset_model.py).  Per task:

  step_ms        training_step + backward on the library's path (the fused loss operator, m3t.ops.pooled_cls_loss)
  stock_loss_ms  the same module and kernels up to the per-frame logits, then the reference's own loss end as stock torch ops (mean / max
                 over T, F.cross_entropy / F.binary_cross_entropy_with_logits, argmax, the accuracy with its `.item()` as in the reference)
  loss section   from the per-frame logits z to dL/dz alone, both ways (no host read-back on either side), in device-event windows of
                 --loss-iters calls, the two paths alternating over --rounds rounds; the median round is reported with the spread

Prints one JSON line.

    python tools/pretrain_bench.py [--clips 128] [--steps 10] [--warmup 3] [--loss-iters 200] [--rounds 5]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

DEV = "cuda:0"


def hp(cls, **kw):
    ns = cls.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def stock_loss_end(z, target, task):
    """the reference's loss end on per-frame logits (vox2_model.py:59,66-67 with backbone.py:144's mean; audioset_model.py:36,39,46-49)"""
    if task == "vox":
        y_hat = z.mean(dim=1)
        loss = F.cross_entropy(y_hat, target)
        hits = torch.sum(torch.argmax(y_hat, dim=-1) == target)
    else:
        y_hat = torch.max(z, dim=1)[0]
        loss = F.binary_cross_entropy_with_logits(y_hat, target)
        hits = torch.sum(torch.gather(target, 1, torch.argmax(y_hat, dim=-1).view(-1, 1)).view(-1))
    return loss, hits


def event_window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters          # us per call


def loss_section(z, target, task, iters, rounds):
    from m3t import ops
    mode, kind = ("mean", "ce") if task == "vox" else ("max", "bce")

    def hip():
        zz = z.detach().requires_grad_(True)
        loss, _, _ = ops.pooled_cls_loss(zz, target, mode, kind)
        loss.backward()
        return zz.grad

    def stock():
        zz = z.detach().requires_grad_(True)
        loss, _ = stock_loss_end(zz, target, task)
        loss.backward()
        return zz.grad

    err = float((hip() - stock()).abs().max())
    for f in (hip, stock):
        event_window(f, 20)
    res = {"hip": [], "stock": []}
    for _ in range(rounds):
        res["hip"].append(event_window(hip, iters))
        res["stock"].append(event_window(stock, iters))
    out = {"max_abs_diff_dz": err}
    for k, v in res.items():
        v = sorted(v)
        out[k + "_us"] = round(v[len(v) // 2], 2)
        out[k + "_us_min_max"] = [round(v[0], 2), round(v[-1], 2)]
    out["speedup"] = round(out["stock_us"] / out["hip_us"], 3)
    return out


def bench_task(task, clips, a):
    from models.vox2_model import VoxCeleb2_1k
    from models.audioset_model import AudioSet
    torch.manual_seed(0)
    if task == "vox":
        m = VoxCeleb2_1k(hp(VoxCeleb2_1k)).to(DEV).train()
        T = m.hparams.window
        x = torch.randint(0, 256, (clips, 3, T, 112, 112), device=DEV).float()
        batch = {"video": x, "label": torch.randint(0, 1000, (clips,), device=DEV)}
        frames = lambda: m.visual.forward_frames((x - 127.5) / 127.5)
        shape = [clips, T, 1000]
    else:
        m = AudioSet(hp(AudioSet)).to(DEV).train()
        T = m.hparams.window
        x = torch.randn(clips, T, 200, device=DEV)
        batch = {"audio": x, "label": (torch.rand(clips, 527, device=DEV) < 0.01).float()}
        frames = lambda: m.audio(x)
        shape = [clips, T, 527]

    def zero():
        for p in m.parameters():
            p.grad = None

    def step_hip():
        zero()
        m.training_step(batch, 0)["loss"].backward()

    def step_stock():
        zero()
        loss, hits = stock_loss_end(frames(), batch["label"], task)
        acc = hits.item() / clips          # noqa: F841  (the reference's host read-back, vox2_model.py:67 / audioset_model.py:49)
        loss.backward()

    out = {"z_shape": shape}
    # alternate the two paths: other work shares the machine
    hip_ms, stock_ms = [], []
    for _ in range(3):
        hip_ms.append(timed(step_hip, a.steps, a.warmup))
        stock_ms.append(timed(step_stock, a.steps, a.warmup))
    out["step_ms"] = round(sorted(hip_ms)[1], 3)
    out["step_ms_all"] = [round(v, 3) for v in hip_ms]
    out["stock_loss_step_ms"] = round(sorted(stock_ms)[1], 3)
    out["stock_loss_step_ms_all"] = [round(v, 3) for v in stock_ms]
    with torch.no_grad():
        z = frames().detach().clone()
    out["loss_section"] = loss_section(z, batch["label"], task, a.loss_iters, a.rounds)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--loss-iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--tasks", default="vox,aud")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pretrain_bench: no GPU -- these are device timings, there is nothing to report without one")
    res = {"metric": "pretrain_step_ms", "clips": a.clips, "loss_iters": a.loss_iters, "rounds": a.rounds}
    for task in a.tasks.split(","):
        res[task] = bench_task(task, a.clips, a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
