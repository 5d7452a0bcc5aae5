#!/usr/bin/env python3
"""Time a validation epoch of the AudioSet stage at the size of eval_segments -- 20 371 clips x 527 classes, 0.4 % positives, at least one
positive per class, batches of 128 clips x 32 frames of ready features (num_hidden 256) -- on one MI355X, scored three ways:

  (a) validate        Trainer.validate as today: val_loss and the top-1 val_acc
  (b) evaluate_cls    Trainer.evaluate_cls: the same plus mAP, mean AUC and d', ranked on the device (m3t/cls_evaluate.py)
  (c) host scoring    (a), then the [20 371, 527] scores read back and the ranking figures computed with numpy on the host (the same
                      two formulas per tie group; no scikit-learn)

The legs alternate in one process, `--rounds` rounds of `--samples` samples, each one whole epoch behind a host clock that ends in a device
synchronise; per leg the median of the rounds' medians and their spread.  Then the append launch (one batch) and the rank launch (all
classes) on their own, the share of (b) they take, and the largest difference between the device's and the host's per-class figures.  The
data is synthetic (fixed seed): a feed-shaped object that hands out resident features and label rows, so no corpus is written.

    python tools/cls_eval_bench.py [--items 20371] [--classes 527] [--batch 128] [--frames 32] [--rounds 3] [--samples 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))


def median(xs):
    return sorted(xs)[len(xs) // 2]


def summary(rounds):
    meds = [median(r) for r in rounds]
    flat = [x for r in rounds for x in r]
    return {"median_ms": round(median(meds), 3), "round_medians_ms": [round(m, 3) for m in meds],
            "spread_ms": [round(min(meds), 3), round(max(meds), 3)], "min_ms": round(min(flat), 3), "max_ms": round(max(flat), 3)}


def timed(fn, inner=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / inner


def host_metrics(scores, labels):
    """numpy on the host: (ap [C], auc [C]) by the tie-group formulas of include/m3t_hip.h (m3t_cls_eval_rank); NaN where not scored"""
    M, Cn = scores.shape
    ap, auc = np.full(Cn, np.nan), np.full(Cn, np.nan)
    for c in range(Cn):
        order = np.argsort(-scores[:, c], kind="stable")
        s, y = scores[order, c], labels[order, c].astype(np.int64)
        last = np.flatnonzero(np.append(s[1:] != s[:-1], True))          # the last row of every group
        tp = np.cumsum(y)[last]
        n = last + 1
        P, N = int(tp[-1]), int(M - tp[-1])
        dtp = np.diff(np.concatenate([[0], tp]))
        dfp = np.diff(np.concatenate([[0], n - tp]))
        if P:
            ap[c] = float(np.sum(dtp * tp / n)) / P
        if P and N:
            auc[c] = float(np.sum(dfp * (2 * (tp - dtp) + dtp))) / (2.0 * P * N)
    return ap, auc


class Plan:
    def __init__(self, items, index):
        self.items, self.aug, self.index = items, None, index


class SyntheticFeed:
    """what Trainer.validate / evaluate_cls ask of an epoch feed: files, plans(), batch(plan), iteration; sequential, as the val split is"""

    def __init__(self, M, Cn, B, T, dev):
        rs = np.random.RandomState(0)
        y = (rs.uniform(size=(M, Cn)) < 0.004).astype(np.float32)
        y[rs.randint(0, M, Cn), np.arange(Cn)] = 1.0                     # at least one positive per class
        self.labels_host = y
        self.labels = torch.from_numpy(y).to(dev)
        g = torch.Generator().manual_seed(0)
        self.pool = torch.randn(8 * B, T, 200, generator=g).to(dev)      # the features: eight batches' worth, read at an item-dependent offset
        self.files, self.B, self.M = [None] * M, B, M

    def plans(self):
        for k, a in enumerate(range(0, self.M, self.B)):
            yield Plan(list(range(a, min(a + self.B, self.M))), k)

    def batch(self, plan):
        a, n = plan.items[0], len(plan.items)
        off = (a // self.B) % 7 * self.B
        return {"audio": self.pool[off:off + n], "label": self.labels[a:a + n]}

    def __iter__(self):
        for p in self.plans():
            yield self.batch(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=20371)
    ap.add_argument("--classes", type=int, default=527)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cls_eval_bench needs the GPU: a timing taken anywhere else says nothing")
    if a.classes != 527:
        raise SystemExit("the AudioSet head has 527 classes")
    from m3t import _lib
    from m3t.cls_evaluate import ClsEvaluator
    from m3t.ops import lib, _stream
    from m3t.trainer import Trainer
    from models.audioset_model import AudioSet
    dev = torch.device("cuda", 0)
    hp = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    hp.window, hp.batch_size, hp.scheduler, hp.checkpoint_path = a.frames, a.batch, "none", None
    torch.manual_seed(0)
    model = AudioSet(hp).to(dev).eval()
    tr = Trainer.from_hparams(model, hp, gradient_clip_val=1.0)
    feed = SyntheticFeed(a.items, a.classes, a.batch, a.frames, dev)
    with torch.no_grad():
        scores_dev = torch.cat([model.forward(b["audio"]) for b in feed])          # [M, C], what leg (c) reads back

    def leg_host():
        tr.validate(feed)
        return host_metrics(scores_dev.cpu().numpy(), feed.labels_host)

    legs = [lambda: tr.validate(feed), lambda: tr.evaluate_cls(feed), leg_host]
    for fn in legs[:2]:
        fn()                                                                       # warm-up: code objects, allocator
    rounds = []
    for _ in range(a.rounds):
        out = [[] for _ in legs]
        for _ in range(a.samples):
            for i, fn in enumerate(legs):
                out[i].append(timed(fn))
        rounds.append(out)
    res = [summary([r[i] for r in rounds]) for i in range(3)]
    dev_res = tr.last_eval
    h_ap, h_auc = leg_host()
    diff = lambda x, y: float(np.nanmax(np.abs(x - y)))

    # the two launches on their own, on a filled evaluator
    ev = ClsEvaluator(a.items, a.classes)
    plans = list(feed.plans())
    for p in plans:
        n = len(p.items)
        ev.add(scores_dev[p.items[0]:p.items[0] + n], feed.batch(p)["label"], p.items, torch.zeros((), device=dev), torch.zeros(n, device=dev))
    p0 = plans[0]
    rows = torch.tensor(p0.items, dtype=torch.int32, device=dev)
    s0, l0 = scores_dev[:len(p0.items)].contiguous(), feed.labels[:len(p0.items)].contiguous()
    append_ms = median([timed(lambda: ev.absorb(s0, l0, rows), 50) for _ in range(9)])
    L, st = lib(), _stream()
    ws_bytes = int(L.m3t_cls_eval_rank_ws_bytes(a.classes, a.items, 0))
    ws = torch.empty(max(ws_bytes // 8, 1), dtype=torch.int64, device=dev)
    per = torch.empty(4 * a.classes, dtype=torch.float64, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def rank():
        _lib.check(L.m3t_cls_eval_rank(ptr(ev.scores), ptr(ev.labels), a.classes, a.items, 0, ptr(ws) if ws_bytes else None, ws_bytes,
                                       ptr(per), st), "m3t_cls_eval_rank")
    rank()
    rank_ms = median([timed(rank, 3) for _ in range(9)])
    b_ms = res[1]["median_ms"]
    print(json.dumps({
        "tool": "cls_eval_bench", "items": a.items, "classes": a.classes, "batch": a.batch, "frames": a.frames, "batches": len(plans),
        "validate": res[0], "evaluate_cls": res[1], "validate_plus_host_scoring": res[2],
        "evaluate_cls_minus_validate_ms": round(b_ms - res[0]["median_ms"], 3),
        "evaluate_cls_over_validate": round(b_ms / res[0]["median_ms"], 4),
        "host_scoring_over_evaluate_cls": round(res[2]["median_ms"] / b_ms, 2),
        "append_launch_ms": round(append_ms, 4), "rank_launch_ms": round(rank_ms, 3), "rank_workspace_bytes": ws_bytes,
        "append_share_of_evaluate_cls": round(append_ms * len(plans) / b_ms, 4), "rank_share_of_evaluate_cls": round(rank_ms / b_ms, 4),
        "device": {k: dev_res.metrics[k] for k in ("val_map", "val_auc", "val_dprime", "n_classes_ap", "n_classes_auc")},
        "max_abs_diff_ap_device_vs_host": diff(dev_res.per_class["ap"], h_ap), "max_abs_diff_auc_device_vs_host": diff(dev_res.per_class["auc"], h_auc),
        "note": "one sample = one whole epoch behind a host clock ending in a device synchronise; legs alternate in one process, %d rounds x "
                "%d samples; median_ms = median of the rounds' medians, spread_ms = their min and max; append: 50 launches per sample, "
                "rank: 3, medians of 9" % (a.rounds, a.samples)}), flush=True)


if __name__ == "__main__":
    main()
