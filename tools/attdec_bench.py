#!/usr/bin/env python3
"""Time the att_dec decoder (m3t.ops.att_decode, csrc/attdec.hip) at B = 32, T = 300, H = 512 against a stock-torch-op restatement
of the same math on the same GPU (here only, for comparison).  Prints one JSON line:
  hip_fwd_ms (forward that records for backward), hip_fwd_nograd_ms, hip_fwd_bwd_ms, torch_* the same for the restatement,
  speedup_* = torch / hip, and the HBM floor of the forward (P and enc re-read every step).
    python tools/attdec_bench.py [--B 32] [--T 300] [--iters 5] [--warmup 2] [--no-torch]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "m3f.pytorch_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def stock_decode(enc, h, W_a, b_a, v, W_ih, W_hh, b_ih, b_hh, W_o, b_o):
    B, T, H = enc.shape
    P = enc @ W_a[:, H:].T + b_a
    y_in = enc.new_zeros(B, 2)
    outs = [enc.new_zeros(B, 2)]
    for _ in range(1, T):
        a = h @ W_a[:, :H].T
        alpha = torch.softmax((torch.relu(P + a[:, None, :]) * v).sum(-1), dim=1)
        c = torch.bmm(alpha[:, None, :], enc)[:, 0]
        gi = torch.cat([y_in, c], 1) @ W_ih.T + b_ih
        gh = h @ W_hh.T + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        y_in = torch.cat([h, c], 1) @ W_o.T + b_o
        outs.append(y_in)
    return torch.stack(outs, 1)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    from models.rnn import Decoder
    from m3t import ops
    dev = "cuda:0"
    torch.manual_seed(0)
    dec = Decoder(2, 512, 2, 1).to(dev)
    B, T, H = a.B, a.T, 512
    enc = torch.randn(B, T, H, device=dev, requires_grad=True)
    h0 = torch.randn(B, H, device=dev).tanh().requires_grad_(True)
    ct = torch.randn(B, T, 2, device=dev)
    w = dec.weights()

    def hip_fwd():
        return ops.att_decode(enc, h0, *w)[0]

    def hip_fwd_nograd():
        with torch.no_grad():
            return ops.att_decode(enc, h0, *w)[0]

    def hip_fwd_bwd():
        (hip_fwd() * ct).sum().backward()

    res = {"B": B, "T": T, "H": H, "steps": T - 1}
    res["hip_fwd_ms"] = timed(hip_fwd, a.iters, a.warmup)
    res["hip_fwd_nograd_ms"] = timed(hip_fwd_nograd, a.iters, a.warmup)
    res["hip_fwd_bwd_ms"] = timed(hip_fwd_bwd, a.iters, a.warmup)
    if not a.no_torch:
        def t_fwd():
            return stock_decode(enc, h0, *w)

        def t_fwd_nograd():
            with torch.no_grad():
                return stock_decode(enc, h0, *w)

        def t_fwd_bwd():
            (stock_decode(enc, h0, *w) * ct).sum().backward()
        with torch.no_grad():
            diff = float((stock_decode(enc, h0, *w) - ops.att_decode(enc, h0, *w)[0]).abs().max())
        res["torch_fwd_ms"] = timed(t_fwd, a.iters, a.warmup)
        res["torch_fwd_nograd_ms"] = timed(t_fwd_nograd, a.iters, a.warmup)
        res["torch_fwd_bwd_ms"] = timed(t_fwd_bwd, a.iters, a.warmup)
        res["max_abs_diff_vs_torch"] = diff
        for k in ("fwd", "fwd_nograd", "fwd_bwd"):
            res["speedup_" + k] = res["torch_%s_ms" % k] / res["hip_%s_ms" % k]
    # P and enc ([B, T, H] fp32 each) re-read by every step: the forward's traffic floor at HBM rate (8 TB/s)
    gb = 2.0 * B * T * H * 4 * (T - 1) / 1e9
    res["fwd_reread_GB"] = gb
    res["fwd_hbm_floor_ms"] = gb / 8e3 * 1e3
    print(json.dumps(res))


if __name__ == "__main__":
    main()
