#!/usr/bin/env python3
"""Time VA_VGGFace (--backbone vggface) on one MI355X: a training step (forward, (y * ct).sum(), backward) and a no_grad inference forward at
8 clips x 16 frames of 112 x 112, on the library's channels-last chain and on the same module with the same weights on stock torch
operators (F.conv2d on MIOpen, F.relu, F.max_pool2d(ceil_mode=True), nn.Linear, nn.Dropout, nn.GRU) in the same process.  Prints one JSON
line: ms per leg and peak torch.cuda.max_memory_allocated for both paths, TFLOP/s against 3.9 GFLOP per frame forward (thirteen 3 x 3
convolutions at 112 x 112 and fc1; 3x for a step), and the HIP-event time of relu_cl / relu_pool_cl (csrc/vggface.hip) with its share of
the chain's step and of its inference forward.

    python tools/vggface_bench.py [--clips 8] [--frames 16] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FWD_GFLOP_PER_FRAME = 3.9


class StockVGGFace(nn.Module):
    """the same model on stock torch operators (reference models/backbone.py:16-59, models/vggface.py): the parameters are shared with `m`"""

    def __init__(self, m):
        super().__init__()
        self.vgg = m.vgg
        g = m.gru.gru
        self.rnn = nn.GRU(m.inputDim, g.hidden_size, g.num_layers, batch_first=True, bidirectional=True)
        for n, p in g.named_parameters():
            setattr(self.rnn, n, p)
        self.head = m.gru.fc

    def forward(self, x):
        b = x.size(0)
        x = x.transpose(1, 2).contiguous()
        x = x.view(-1, x.size(2), x.size(3), x.size(4))
        for blk in (self.vgg.conv1, self.vgg.conv2, self.vgg.conv3, self.vgg.conv4, self.vgg.conv5):
            for c in blk.convs:
                x = F.relu(F.conv2d(x, c.weight, c.bias, 1, 1))
            x = F.max_pool2d(x, 2, 2, 0, ceil_mode=True)
        x = x.view(x.size(0), -1)
        x = self.vgg.dropout(F.relu(F.linear(x, self.vgg.fc1.weight, self.vgg.fc1.bias)))
        return self.head(self.rnn(x.view(b, -1, x.size(1)))[0])


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


def relu_split(ops, fn):
    """HIP-event ms of the csrc/vggface.hip operators over one call of fn"""
    ops.PROFILE_ON[0] = True
    ops.PROFILE.clear()
    fn()
    torch.cuda.synchronize()
    split = {}
    for rec in ops.PROFILE:
        if rec["kernel"].startswith("relu_"):
            k = split.setdefault(rec["kernel"], {"ms": 0.0, "bytes": 0.0, "calls": 0})
            k["ms"] += rec["start"].elapsed_time(rec["end"])
            k["bytes"] += rec["bytes"]
            k["calls"] += 1
    ops.PROFILE_ON[0] = False
    ops.PROFILE.clear()
    for k in split.values():
        k["tb_per_s"] = round(k.pop("bytes") / (k["ms"] * 1e9), 2) if k["ms"] > 0 else None
        k["ms"] = round(k["ms"], 3)
    return split, round(sum(k["ms"] for k in split.values()), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from models.backbone import VA_VGGFace
    from m3t import ops
    dev = "cuda:0"
    torch.manual_seed(0)
    m = VA_VGGFace(frameLen=a.frames).to(dev).train()
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
    step_split, step_relu_ms = relu_split(ops, step(m))
    m.eval()
    hip_inf, hip_inf_mem = timed(infer(m), a.steps, a.warmup)
    inf_split, inf_relu_ms = relu_split(ops, infer(m))
    m.train()
    ref = StockVGGFace(m).to(dev).train()
    stock_step, stock_step_mem = timed(step(ref), a.steps, a.warmup)
    ref.eval()
    stock_inf, stock_inf_mem = timed(infer(ref), a.steps, a.warmup)
    gf = FWD_GFLOP_PER_FRAME * frames
    print(json.dumps({
        "metric": "vggface_step_ms", "clips": a.clips, "frames": a.frames,
        "hip": {"step_ms": round(hip_step, 3), "infer_ms": round(hip_inf, 3), "step_tflops": round(3 * gf / hip_step, 2),
                "infer_tflops": round(gf / hip_inf, 2), "peak_gib_step": round(hip_step_mem, 2), "peak_gib_infer": round(hip_inf_mem, 2)},
        "stock": {"step_ms": round(stock_step, 3), "infer_ms": round(stock_inf, 3), "step_tflops": round(3 * gf / stock_step, 2),
                  "infer_tflops": round(gf / stock_inf, 2), "peak_gib_step": round(stock_step_mem, 2), "peak_gib_infer": round(stock_inf_mem, 2)},
        "step_speedup": round(stock_step / hip_step, 3), "infer_speedup": round(stock_inf / hip_inf, 3),
        "hip_stock_fallbacks": stock_used,
        "relu_kernels_step": {"ms": step_relu_ms, "share_of_step": round(step_relu_ms / hip_step, 3), "split": step_split},
        "relu_kernels_infer": {"ms": inf_relu_ms, "share_of_infer": round(inf_relu_ms / hip_inf, 3), "split": inf_split},
    }))


if __name__ == "__main__":
    main()
