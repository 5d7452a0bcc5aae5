#!/usr/bin/env python3
"""Time the GroupNorm stems (norm_layer='gn') on one MI355X: VA_3DVGGM_Split(split_layer=3, norm_layer='gn') + BiGRU at the C5 shape (8 clips x
64 frames x 112 x 112) -- a training step (forward, (y * ct).sum(), backward) and a no_grad inference forward, HIP-event times, warmed up -- on
the channels-last chain (ops.GN_CL[0] = True: csrc/gn_cl.hip) and on the route it replaces (False: planes convolutions, stock GroupNorm + ReLU,
planes pooling) in the SAME process, alternating, `--rounds` times, so that the spread is known.  Both models hold the same weights.

Then each GroupNorm operator alone at the five stem shapes (conv1 55 x 55 x 64 and conv2 25 x 25 x 128 and conv3 10 x 10 x 256 with the 2 x 2
pooling fused, conv4 3 x 3 x 512, conv5 1 x 1 x 512), forward and backward, with the algorithmic bytes over the time as a share of the HBM peak
(8.0 TB/s), and bn_cl / bn_pool_cl at the same shapes beside them.  Prints one JSON line.

    python tools/stem_gn_bench.py [--clips 8] [--frames 64] [--rounds 3] [--steps 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))

HBM_PEAK = 8.0e12
STEM_SHAPES = [("conv1", 55, 64, 2), ("conv2", 25, 128, 2), ("conv3", 10, 256, 2), ("conv4", 3, 512, 0), ("conv5", 1, 512, 0)]


def event_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def op_bytes(M, Mp, C, k):
    """algorithmic bytes (forward, backward): statistics + apply read x twice; backward's two sweeps read what they need once each"""
    if k:
        return (8 * M + 5 * Mp) * C, (13 * Mp + 4 * M + 9 * Mp + 4 * M) * C
    return 12 * M * C, 28 * M * C


def time_op(ops, kind, N, T, S, C, k, steps, warmup):
    dev = "cuda:0"
    M = N * T * S * S
    Mp = N * T * (S // k) * (S // k) if k else M
    x = (0.7 * torch.randn(M, C, device=dev) + 3.0).requires_grad_(True)
    gamma, beta = torch.randn(C, device=dev).requires_grad_(True), torch.randn(C, device=dev).requires_grad_(True)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    dout = torch.randn(Mp, C, device=dev)
    state = {}

    def fwd():
        xc = ops.CLTensor(x, N, T, S, S, None)
        if kind == "gn":
            y = ops.gn_cl(xc, 32, gamma, beta, 1e-5, True, lazy=bool(k))
        else:
            y = ops.bn_cl(xc, gamma, beta, rm, rv, True, 0.1, 1e-5, True, lazy=bool(k))
        if k:
            y = ops.pool_cl(y, (k, k), (k, k), (0, 0))
        state["y"] = y.data

    def bwd():
        x.grad = gamma.grad = beta.grad = None
        state["y"].backward(dout, retain_graph=True)

    f_ms = event_ms(fwd, steps, warmup)
    b_ms = event_ms(bwd, steps, warmup)
    fb, bb = op_bytes(M, Mp, C, k)
    return {"fwd_ms": round(f_ms, 4), "bwd_ms": round(b_ms, 4), "fwd_share_of_hbm_peak": round(fb / (f_ms * 1e-3) / HBM_PEAK, 3),
            "bwd_share_of_hbm_peak": round(bb / (b_ms * 1e-3) / HBM_PEAK, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ops-only", action="store_true")
    a = ap.parse_args()
    from models.backbone import VA_3DVGGM_Split
    from m3t import ops
    dev = "cuda:0"
    res = {"metric": "stem_gn_step_ms", "clips": a.clips, "frames": a.frames, "rounds": a.rounds}
    if not a.ops_only:
        models = {}
        torch.manual_seed(0)
        for on in (True, False):
            ops.GN_CL[0] = on
            m = VA_3DVGGM_Split(frameLen=a.frames, split_layer=3, norm_layer="gn", backend="gru").to(dev)
            if models:
                m.load_state_dict(models[True].state_dict())
            models[on] = m
        x = (torch.randint(0, 256, (a.clips, 3, a.frames, 112, 112), device=dev).float() - 127.5) / 127.5
        se, au = torch.randn(a.clips, 512, a.frames, device=dev), torch.randn(a.clips, 512, a.frames, device=dev)
        ct = torch.randn(a.clips, a.frames, 2, device=dev)

        def step(net):
            def f():
                for p in net.parameters():
                    p.grad = None
                (net(x, se, au) * ct).sum().backward()
            return f

        def infer(net):
            def f():
                with torch.no_grad():
                    net(x, se, au)
            return f

        stock0 = dict(ops.STOCK_FALLBACKS)
        times = {(on, leg): [] for on in (True, False) for leg in ("step", "infer")}
        for _ in range(a.rounds):
            for on in (True, False):
                ops.GN_CL[0] = on
                models[on].train()
                times[(on, "step")].append(event_ms(step(models[on]), a.steps, a.warmup))
                models[on].eval()
                times[(on, "infer")].append(event_ms(infer(models[on]), a.steps, a.warmup))
        ops.GN_CL[0] = True
        res["stock_fallbacks"] = {k: v - stock0.get(k, 0) for k, v in ops.STOCK_FALLBACKS.items() if v != stock0.get(k, 0)}
        for leg in ("step", "infer"):
            on_t, off_t = times[(True, leg)], times[(False, leg)]
            res[leg] = {"chain_ms": [round(t, 3) for t in on_t], "off_ms": [round(t, 3) for t in off_t],
                        "chain_median": round(statistics.median(on_t), 3), "off_median": round(statistics.median(off_t), 3),
                        "spread_ms": round(max(max(on_t) - min(on_t), max(off_t) - min(off_t)), 3),
                        "speedup": round(statistics.median(off_t) / statistics.median(on_t), 3)}
        del models
        torch.cuda.empty_cache()
    res["operators"] = {}
    for name, S, C, k in STEM_SHAPES:
        res["operators"][name] = {"shape": [a.clips, a.frames, S, S, C], "k": k,
                                  "gn": time_op(ops, "gn", a.clips, a.frames, S, C, k, a.steps, a.warmup),
                                  "bn": time_op(ops, "bn", a.clips, a.frames, S, C, k, a.steps, a.warmup)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
