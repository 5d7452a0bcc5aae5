#!/usr/bin/env python3
"""Time one synthetic validation epoch on one MI355X, both ways, on the C3 audiovisual graph (m3t/workloads.py, feature
inputs) and on the audio-only model:

  host route    Trainer.validate (validation_step reads every batch back; m3t/stitch.py on the CPU; predictions_val.pt)
                + postproc.smoothed_ccc_report('predictions_val.pt')
  device route  Trainer.evaluate (m3t/evaluate.py: nothing read back until the end; the same file under another name)
                + Trainer.last_eval.smoothed_report()

The epoch: --videos videos of --frames frames as windows of --window frames at stride window / 2, --batch windows per batch in
loader order, test_on_val (overlap-add).  Each route is timed end to end with the host clock around a final device
synchronise, after one warm-up epoch each: --repeats epochs in turn, median.  The two routes must agree on every track bit for bit or the
run fails.  One JSON line.

    python tools/eval_bench.py [--videos 145] [--frames 2000] [--window 32] [--batch 32] [--repeats 3]

--expr: what scoring the expression head costs (m3t/evaluate.py, Evaluator(expr=True)).  The same epoch with expression
labels, three routes in turn in one process, --repeats rounds after one warm-up each, median and spread (max - min):

  va         Trainer.evaluate(batches)                 valence / arousal only
  va_expr    Trainer.evaluate(batches, expr=True)      + the expression head on the device: still one read-back
  host_expr  the va route with the expression part by hand: per batch y_hat[..., :7].argmax(-1).cpu(), a numpy confusion

va_expr and host_expr must agree on the epoch's confusion (through val_acc_expr) or the run fails.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))

from models.model import AffWild2VA  # noqa: E402
from m3t import postproc  # noqa: E402
from m3t.evaluate import Evaluator  # noqa: E402
from m3t.trainer import Trainer  # noqa: E402
from m3t.workloads import AVFeatureGraph  # noqa: E402

DEV = "cuda:0"


class FeatureAV(nn.Module):
    """the C3 graph behind AffWild2VA's evaluation hooks (the hooks only need forward(batch) and hparams)"""

    def __init__(self, hparams):
        super().__init__()
        self.hparams = hparams
        self.graph = AVFeatureGraph()

    def forward(self, batch):
        return self.graph(batch["audio"], batch["video"])

    _window_outputs = AffWild2VA._window_outputs
    validation_step = AffWild2VA.validation_step
    validation_end = AffWild2VA.validation_end


def hparams(**kw):
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def epoch(args, dims, pool=8):
    """the batches of one epoch: names / starts / lengths per window as the loader's collate gives them (CPU tensors); the
    inputs and labels of a batch come from a small pool of device tensors (their values do not matter to the timing)"""
    W = args.window
    wins = [("video%03d" % v, s, min(W, args.frames - s)) for v in range(args.videos) for s in range(0, args.frames, W // 2)]
    gen = torch.Generator(device=DEV).manual_seed(0)
    rnd = lambda *shape: torch.rand(*shape, device=DEV, generator=gen) * 2 - 1
    feats = [{k: rnd(args.batch, W, d) for k, d in dims.items()} for _ in range(pool)]
    labels = []
    for _ in range(pool):
        lv, la = rnd(args.batch, W), rnd(args.batch, W)
        lv[torch.rand(args.batch, W, device=DEV, generator=gen) < 0.2] = -5.0         # unannotated frames
        labels.append((lv, la))
    expr = getattr(args, "expr", False)                # (drawn after everything else: the plain epoch keeps its values)
    exprs = [(torch.randint(0, 7, (args.batch, W), device=DEV, generator=gen),
              torch.rand(args.batch, W, device=DEV, generator=gen) < 0.8) for _ in range(pool if expr else 0)]
    batches = []
    for i in range(0, len(wins), args.batch):
        chunk, j = wins[i:i + args.batch], (i // args.batch) % pool
        n = len(chunk)
        b = {k: v[:n] for k, v in feats[j].items()}
        b.update({"label_valence": labels[j][0][:n], "label_arousal": labels[j][1][:n], "vid_name": [c[0] for c in chunk],
                  "start": torch.tensor([c[1] for c in chunk]), "length": torch.tensor([c[2] for c in chunk])})
        if expr:
            b.update({"class_expr": exprs[j][0][:n], "expr_valid": exprs[j][1][:n]})
        batches.append(b)
    return batches, len(wins)


def timed(fns, repeats):
    """seconds per call of each function, sampled in turn after one warm-up call each: (medians, samples)"""
    for fn in fns:
        fn()                               # warm-up epoch
    out = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out[i].append(time.perf_counter() - t0)
    return [sorted(x)[len(x) // 2] for x in out], out


def bench(name, model, dims, args):
    tr = Trainer.from_hparams(model, model.hparams)
    batches, n_windows = epoch(args, dims)
    sink = lambda *_: None
    kept = {}

    def host():
        tr.validate(batches)
        kept["host"] = postproc.smoothed_ccc_report("predictions_val.pt", out=sink)

    def device():
        tr.evaluate(batches, out_path="predictions_val_device.pt")
        kept["device"] = tr.last_eval.smoothed_report(out=sink)

    (t_host, t_dev), (all_host, all_dev) = timed([host, device], args.repeats)
    ref, got = torch.load("predictions_val.pt"), torch.load("predictions_val_device.pt")
    for k in ref:
        for vid in ref[k]:
            assert torch.equal(ref[k][vid], got[k][vid]), "the two routes disagree on %s of %s" % (k, vid)
    gap = max(abs(kept["host"][k][v] - kept["device"][k][v]) for k in ("ccc_v", "ccc_a") for v in kept["host"][k])
    return {"model": name, "windows": n_windows, "batches": len(batches), "host_route_s": round(t_host, 4),
            "device_route_s": round(t_dev, 4), "host_over_device": round(t_host / t_dev, 3),
            "host_route_all_s": [round(t, 4) for t in all_host], "device_route_all_s": [round(t, 4) for t in all_dev],
            "max_report_diff": gap}


def bench_expr(name, model, dims, args):
    tr = Trainer.from_hparams(model, model.hparams)
    batches, n_windows = epoch(args, dims)
    kept = {}

    def va():
        tr.evaluate(batches, out_path="predictions_val_va.pt")

    def va_expr():
        kept["device"] = tr.evaluate(batches, out_path="predictions_val_expr.pt", expr=True)["log"]["val_acc_expr"]

    def host_expr():
        conf = np.zeros((7, 7), np.int64)
        ev = Evaluator(args.window, overlap=True, with_gt=True)                    # Trainer.evaluate's loop under test_on_val
        model.eval()
        with torch.no_grad():
            for b in batches:
                y = model.forward(b)
                ev.add(y, b)
                pred = y[..., :7].argmax(-1).cpu().numpy()                         # the read-back per batch
                ok = b["expr_valid"].cpu().numpy() & (np.arange(pred.shape[1])[None, :] < b["length"].numpy()[:, None])
                np.add.at(conf, (b["class_expr"].cpu().numpy()[ok], pred[ok]), 1)
        tr.ddp.agree_on_scan_error()
        ev.finish().save("predictions_val_host_expr.pt")
        kept["host"] = float(np.trace(conf)) / float(conf.sum())

    meds, samples = timed([va, va_expr, host_expr], args.repeats)
    assert abs(kept["device"] - kept["host"]) <= 1e-15, "the two expression routes disagree: %r" % kept
    out = {"model": name, "windows": n_windows, "batches": len(batches), "val_acc_expr": kept["device"]}
    for key, med, xs in zip(("va", "va_expr", "host_expr"), meds, samples):
        out[key + "_s"], out[key + "_spread_s"], out[key + "_all_s"] = round(med, 4), round(max(xs) - min(xs), 4), [round(t, 4) for t in xs]
    out["expr_over_va_s"] = round(meds[1] - meds[0], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=145)
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--window", type=int, default=32)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--models", default="c3,audio")
    ap.add_argument("--expr", action="store_true", help="time the expression head: va / va_expr / host_expr (see above)")
    args = ap.parse_args()
    torch.manual_seed(0)
    results = []
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)                      # the routes write their prediction files into the working directory
        for name in args.models.split(","):
            if name == "c3":
                hp = hparams(modality="audiovisual", fusion_type="attention", loss="ccc_mtl", window=args.window, test_on_val=True)
                model, dims = FeatureAV(hp).to(DEV), {"audio": 128, "video": 256}
            elif name == "audio":
                hp = hparams(modality="audio", loss="ccc_mtl", window=args.window, test_on_val=True)
                model, dims = AffWild2VA(hp).to(DEV), {"audio": 200}
            else:
                raise SystemExit("unknown model %r (c3, audio)" % name)
            results.append((bench_expr if args.expr else bench)(name, model, dims, args))
        os.chdir(ROOT)
    print(json.dumps({"videos": args.videos, "frames": args.frames, "window": args.window, "batch": args.batch,
                      "repeats": args.repeats, "expr": args.expr, "results": results}))


if __name__ == "__main__":
    main()
