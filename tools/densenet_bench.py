#!/usr/bin/env python3
"""Time VA_3DDenseNet (--backbone densenet) on one MI355X: a training step (forward, (y * ct).sum(), backward) and an inference forward at
8 clips x 64 frames of 112 x 112 (bench.py's ResNet3D leg size), on the library's path and on a stock-torch composition of the same weights
(the reference's modules: nn.Conv3d / nn.BatchNorm3d / torch.cat on MIOpen and the torch kernels, the GRU on nn.GRU) built here.  Prints
one JSON line: ms per leg for both paths, TFLOP/s against the issue's count (1.5 GFLOP per frame forward, 3x for a step), peak
torch.cuda.max_memory_allocated of each path and the per-kernel split from HIP events (m3t.ops.PROFILE: the GRU scans).

    python tools/densenet_bench.py [--clips 8] [--frames 64] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FWD_GFLOP_PER_FRAME = 1.5


class StockDenseNet(nn.Module):
    """the same model as stock torch modules (reference models/backbone.py:375-423): the parameters are shared with `m`"""

    def __init__(self, m):
        super().__init__()
        c = m.c3d
        self.conv, self.bn, self.pool = nn.Conv3d(3, 64, (5, 7, 7), (1, 2, 2), (2, 3, 3), bias=False), nn.BatchNorm3d(64), nn.MaxPool3d((1, 3, 3), (1, 2, 2), (0, 1, 1))
        self.conv.weight, self.bn.weight, self.bn.bias = c[0].weight, c[1].weight, c[1].bias
        self.bn.running_mean, self.bn.running_var = c[1].running_mean.clone(), c[1].running_var.clone()
        self.densenet = m.densenet
        g = m.gru.gru
        self.rnn = nn.GRU(392, g.hidden_size, g.num_layers, batch_first=True, bidirectional=True)
        for n, p in g.named_parameters():
            setattr(self.rnn, n, p)
        self.head = m.gru.fc

    def forward(self, x):
        x = self.pool(torch.relu(self.bn(self.conv(x))))
        x = self.densenet._stock_forward(x)
        return self.head(self.rnn(x)[0])


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps, torch.cuda.max_memory_allocated() / 2**30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from models.backbone import VA_3DDenseNet
    from m3t import ops
    dev = "cuda:0"
    torch.manual_seed(0)
    m = VA_3DDenseNet(frameLen=a.frames).to(dev).train()
    x = (torch.randint(0, 256, (a.clips, 3, a.frames, 112, 112), device=dev).float() - 127.5) / 127.5
    ct = torch.randn(a.clips, a.frames, 2, device=dev)
    frames = a.clips * a.frames

    def step(net):
        def f():
            for p in net.parameters():
                p.grad = None
            (net(x) * ct).sum().backward()
        return f

    def infer(net):
        def f():
            with torch.no_grad():
                net(x)
        return f

    stock0 = dict(ops.STOCK_FALLBACKS)
    hip_step, hip_step_mem = timed(step(m), a.steps, a.warmup)
    stock_used = {k: v - stock0.get(k, 0) for k, v in ops.STOCK_FALLBACKS.items() if v != stock0.get(k, 0)}
    ops.PROFILE_ON[0] = True
    ops.PROFILE.clear()
    step(m)()
    torch.cuda.synchronize()
    split = {}
    for rec in ops.PROFILE:
        k = split.setdefault(rec["kernel"], {"ms": 0.0, "tflops": 0.0, "flop": 0.0})
        k["ms"] += rec["start"].elapsed_time(rec["end"])
        k["flop"] += rec["flops"]
    for k in split.values():
        k["tflops"] = round(k.pop("flop") / (k["ms"] * 1e9), 2) if k["ms"] > 0 else None
        k["ms"] = round(k["ms"], 3)
    ops.PROFILE_ON[0] = False
    m.eval()
    hip_inf, hip_inf_mem = timed(infer(m), a.steps, a.warmup)
    m.train()
    ref = StockDenseNet(m).to(dev).train()
    stock_step, stock_step_mem = timed(step(ref), a.steps, a.warmup)
    ref.eval()
    stock_inf, stock_inf_mem = timed(infer(ref), a.steps, a.warmup)
    gf = FWD_GFLOP_PER_FRAME * frames
    print(json.dumps({
        "metric": "densenet_step_ms", "clips": a.clips, "frames": a.frames,
        "hip": {"step_ms": round(hip_step, 3), "infer_ms": round(hip_inf, 3), "step_tflops": round(3 * gf / hip_step, 2),
                "infer_tflops": round(gf / hip_inf, 2), "peak_gib_step": round(hip_step_mem, 2), "peak_gib_infer": round(hip_inf_mem, 2)},
        "stock": {"step_ms": round(stock_step, 3), "infer_ms": round(stock_inf, 3), "step_tflops": round(3 * gf / stock_step, 2),
                  "infer_tflops": round(gf / stock_inf, 2), "peak_gib_step": round(stock_step_mem, 2), "peak_gib_infer": round(stock_inf_mem, 2)},
        "step_speedup": round(stock_step / hip_step, 3),
        "hip_stock_fallbacks": stock_used,
        "kernel_split": split,
    }))


if __name__ == "__main__":
    main()
