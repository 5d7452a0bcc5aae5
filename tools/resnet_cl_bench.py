#!/usr/bin/env python3
"""Time the per-frame ResNet-18 front-end (`--ver v1`, the default, or `--ver v2`) on one MI355X: VA_3DResNet(resnet_ver, use_cbam=False) + BiGRU at 8 clips x 64 frames x
112 x 112 -- a training step (forward, (y * ct).sum(), backward) and a no_grad inference forward, HIP-event times, warmed up -- on the
channels-last chain (v1: ops.RESNET_CL[0] = True, v2: ops.RESNET_V2_CL[0] = True -- csrc/stem_cl.hip's operators, the walks without transposes) and on the route it
replaces (False: planes, a transpose on each side of every convolution) in the SAME process, alternating, `--rounds` times, so that the spread
is known.  Both models hold the same weights (the BatchNorm affines drawn at random: zero_init_residual's gamma = 0 is the first step only);
the two routes' outputs on the timed input are compared (max |difference| / max |output|).

Then each new operator alone at the four stage shapes (28 x 28 x 64, 14 x 14 x 128, 7 x 7 x 256, 4 x 4 x 512 per frame), forward and backward,
`--reps` calls per timed window, with the algorithmic bytes over the time in GB/s and as a share of the HBM peak (8.0 TB/s) -- and what it
replaces beside it: bn_cl (no ReLU) followed by add_relu at the same shapes, torch's mean for the spatial mean.  With `--ver v2` the operator is
add_bn_relu_cl (the residual sum and the BatchNorm + ReLU behind it, backward with the identity's gradient ds_out) beside torch's a + b followed
by bn_cl.  Prints one JSON line.

    python tools/resnet_cl_bench.py [--ver v1] [--clips 8] [--frames 64] [--rounds 3] [--steps 5] [--warmup 2] [--reps 20] [--ops-only]
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
STAGES = [("layer1", 28, 64), ("layer2", 14, 128), ("layer3", 7, 256), ("layer4", 4, 512)]


def event_ms(fn, steps, warmup, reps=1):
    """median over `steps` windows of `reps` calls each, per call"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out)


def rate(nbytes, ms):
    return {"ms": round(ms, 4), "GBps": round(nbytes / (ms * 1e-3) / 1e9, 1), "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 3)}


def time_tail(ops, P, S, C, steps, warmup, reps):
    """bn_add_relu_cl against bn_cl (no ReLU) + add_relu; algorithmic bytes of the fused form: forward 16 M C (statistics read x; the map reads
    x and the shortcut and writes y), backward 32 M C (the partial pass reads dy, x, y; the map reads them again and writes dx and ds)"""
    dev = "cuda:0"
    M = P * S * S
    x = (0.7 * torch.randn(M, C, device=dev) + 1.0).requires_grad_(True)
    s = torch.randn(M, C, device=dev).requires_grad_(True)
    gamma, beta = torch.randn(C, device=dev).requires_grad_(True), torch.randn(C, device=dev).requires_grad_(True)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    dout = torch.randn(M, C, device=dev)
    state = {}

    def fused():
        xc, sc = ops.CLTensor(x, P, 1, S, S, None), ops.CLTensor(s, P, 1, S, S, None)
        state["y"] = ops.bn_add_relu_cl(xc, sc, gamma, beta, rm, rv, True, 0.1, 1e-5).data

    def split():
        y = ops.bn_cl(ops.CLTensor(x, P, 1, S, S, None), gamma, beta, rm, rv, True, 0.1, 1e-5, False)
        state["y"] = ops.add_relu(y.data, s)

    def bwd():
        x.grad = s.grad = gamma.grad = beta.grad = None
        state["y"].backward(dout, retain_graph=True)

    out = {}
    for name, fwd in (("bn_add_relu_cl", fused), ("bn_cl+add_relu", split)):
        f_ms = event_ms(fwd, steps, warmup, reps)
        b_ms = event_ms(bwd, steps, warmup, reps)
        out[name] = {"fwd": rate(16 * M * C, f_ms), "bwd": rate(32 * M * C, b_ms)}
    return out


def time_seam(ops, P, S, C, steps, warmup, reps):
    """add_bn_relu_cl against a + b followed by bn_cl (ReLU); algorithmic bytes of the fused form: forward 20 M C (the statistics pass reads a and b
    and writes s; the map reads s and writes z), backward 32 M C (the partial pass reads dz, s, z; the map reads them and ds_out and writes ds)"""
    dev = "cuda:0"
    M = P * S * S
    a = (0.7 * torch.randn(M, C, device=dev) + 1.0).requires_grad_(True)
    b = torch.randn(M, C, device=dev).requires_grad_(True)
    gamma, beta = torch.randn(C, device=dev).requires_grad_(True), torch.randn(C, device=dev).requires_grad_(True)
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    dz, ds_out = torch.randn(M, C, device=dev), torch.randn(M, C, device=dev)
    state = {}

    def fused():
        s, z = ops.add_bn_relu_cl(ops.CLTensor(a, P, 1, S, S, None), ops.CLTensor(b, P, 1, S, S, None), gamma, beta, rm, rv, True, 0.1, 1e-5)
        state["out"] = [z.data, s.data]

    def split():
        s = a + b
        state["out"] = [ops.bn_cl(ops.CLTensor(s, P, 1, S, S, None), gamma, beta, rm, rv, True, 0.1, 1e-5, True).data, s]

    def bwd():
        a.grad = b.grad = gamma.grad = beta.grad = None
        torch.autograd.backward(state["out"], [dz, ds_out], retain_graph=True)

    out = {}
    for name, fwd in (("add_bn_relu_cl", fused), ("add+bn_cl", split)):
        f_ms = event_ms(fwd, steps, warmup, reps)
        b_ms = event_ms(bwd, steps, warmup, reps)
        out[name] = {"fwd": rate(20 * M * C, f_ms), "bwd": rate(32 * M * C, b_ms)}
    return out


def time_mean(ops, P, S, C, steps, warmup, reps):
    dev = "cuda:0"
    HW = S * S
    x = torch.randn(P * HW, C, device=dev).requires_grad_(True)
    dout = torch.randn(P, C, device=dev)
    state = {}

    def fused():
        state["y"] = ops.mean_cl(ops.CLTensor(x, P, 1, S, S, None))

    def stock():
        state["y"] = x.view(P, HW, C).mean(1)

    def bwd():
        x.grad = None
        state["y"].backward(dout, retain_graph=True)

    nbytes = 4 * (P * HW + P) * C
    out = {}
    for name, fwd in (("mean_cl", fused), ("torch_mean", stock)):
        f_ms = event_ms(fwd, steps, warmup, reps)
        b_ms = event_ms(bwd, steps, warmup, reps)
        out[name] = {"fwd": rate(nbytes, f_ms), "bwd": rate(nbytes, b_ms)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ver", choices=("v1", "v2"), default="v1")
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ops-only", action="store_true")
    a = ap.parse_args()
    from models.backbone import VA_3DResNet
    from m3t import ops
    dev = "cuda:0"
    switch = ops.RESNET_CL if a.ver == "v1" else ops.RESNET_V2_CL
    res = {"metric": "resnet_cl_step_ms", "ver": a.ver, "clips": a.clips, "frames": a.frames, "rounds": a.rounds}
    if not a.ops_only:
        models = {}
        torch.manual_seed(0)
        for on in (True, False):
            switch[0] = on
            m = VA_3DResNet(frameLen=a.frames, resnet_ver=a.ver, use_cbam=False, backend="gru").to(dev)
            if models:
                m.load_state_dict(models[True].state_dict())
            else:
                with torch.no_grad():
                    for mod in m.modules():
                        if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                            mod.weight.normal_(1.0, 0.1)
                            mod.bias.normal_(0.0, 0.1)
            models[on] = m
        assert models[True].c3d[0].cl_chain and not models[False].c3d[0].cl_chain
        x = (torch.randint(0, 256, (a.clips, 3, a.frames, 112, 112), device=dev).float() - 127.5) / 127.5
        ct = torch.randn(a.clips, a.frames, 2, device=dev)

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
        times = {(on, leg): [] for on in (True, False) for leg in ("step", "infer")}
        for _ in range(a.rounds):
            for on in (True, False):
                switch[0] = on
                models[on].train()
                times[(on, "step")].append(event_ms(step(models[on]), a.steps, a.warmup))
                models[on].eval()
                times[(on, "infer")].append(event_ms(infer(models[on]), a.steps, a.warmup))
        outs = {}
        for on in (True, False):
            switch[0] = on
            with torch.no_grad():
                outs[on] = models[on](x)
        switch[0] = True
        res["eval_output_max_rel_diff"] = float((outs[True] - outs[False]).abs().max() / outs[False].abs().max())
        res["stock_fallbacks"] = {k: v - stock0.get(k, 0) for k, v in ops.STOCK_FALLBACKS.items() if v != stock0.get(k, 0)}
        for leg in ("step", "infer"):
            on_t, off_t = times[(True, leg)], times[(False, leg)]
            res[leg] = {"chain_ms": [round(t, 3) for t in on_t], "planes_ms": [round(t, 3) for t in off_t],
                        "chain_median": round(statistics.median(on_t), 3), "planes_median": round(statistics.median(off_t), 3),
                        "spread_ms": round(max(max(on_t) - min(on_t), max(off_t) - min(off_t)), 3),
                        "speedup": round(statistics.median(off_t) / statistics.median(on_t), 3)}
        del models, outs
        torch.cuda.empty_cache()
    P = a.clips * a.frames
    res["operators"] = {}
    time_op = time_tail if a.ver == "v1" else time_seam
    for name, S, C in STAGES:
        res["operators"][name] = {"shape": [P, S, S, C], **time_op(ops, P, S, C, a.steps, a.warmup, a.reps)}
    if a.ver == "v1":
        res["operators"]["mean"] = {"shape": [P, 4, 4, 512], **time_mean(ops, P, 4, 512, a.steps, a.warmup, a.reps)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
