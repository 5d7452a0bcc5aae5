"""A multi-label evaluation epoch on the device (csrc/cls_eval.hip): what the AudioSet stage should report about itself -- mean average
precision, mean ROC-AUC and d' over the 527 classes, the figures every published AudioSet number is given in -- beside the val_loss and the
top-1 val_acc of the reference's validation_end (audioset_model.py:89-104), without a read-back per batch and without reading the
[items, classes] scores back at the end of the epoch.

  ev = ClsEvaluator(n_items, n_classes)
  for plan in feed.plans():
      batch = feed.batch(plan)
      pooled, loss, correct = model.eval_scores(batch)
      ev.add(pooled, batch['label'], plan.items, loss, correct)     # ONE m3t_cls_eval_append launch, nothing read back
  res = ev.finish()                                                 # rank + reduce launches, ONE read-back
  res.metrics, res.per_class, res.report(names), res.save('audioset_eval.json')

The rule (include/m3t_hip.h, m3t_cls_eval_rank): per class the items are ordered by their float32 score, equal scores form one threshold
group, AP = (1/P) sum_groups dTP TP / (TP + FP) and AUC = sum_groups dFP (2 TP_before + dTP) / (2 P N) -- scikit-learn's
average_precision_score and roc_auc_score, ties included.  A class without a positive is left out of both means, one without a negative out
of the AUC mean (its AP is 1); their entries are NaN.  val_map / val_auc are the means over the scored classes, val_dprime =
sqrt(2) * Phi^-1(val_auc).  One non-finite score or one label that is neither 0.0 nor 1.0 anywhere in the epoch makes the three ranking figures
NaN and is counted in n_nonfinite / n_bad_labels: nothing is dropped silently.  val_loss and val_acc are reduced as
_classification_epoch_end reduces them and carry its bits.

Capacity: M3T_CLS_EVAL_MAX_ROWS (262 144) items; more raises ValueError before anything is launched.  Columns of up to
M3T_CLS_EVAL_LDS_ROWS (16 384) items are sorted wholly in LDS, longer ones in LDS-sized chunks with the wide strides in a global workspace
(`lds_rows=` lowers the threshold: tests force the long path at small sizes).  There is no CPU path.
"""
import csv
import ctypes as C
import json
import math
import os
import statistics

import numpy as np
import torch

from . import _lib

METRIC_KEYS = ("val_loss", "val_acc", "val_map", "val_auc", "val_dprime", "n_classes_ap", "n_classes_auc", "n_nonfinite", "n_bad_labels")
MAX_ROWS = _lib.M3T_CLS_EVAL_MAX_ROWS
LDS_ROWS = _lib.M3T_CLS_EVAL_LDS_ROWS


def dprime(auc):
    """sqrt(2) * Phi^-1(auc): +-inf at AUC 1 / 0, NaN for NaN"""
    if auc != auc:
        return float("nan")
    if auc >= 1.0:
        return float("inf")
    if auc <= 0.0:
        return float("-inf")
    return math.sqrt(2.0) * statistics.NormalDist().inv_cdf(auc)


def read_class_names(path):
    """display names of class_labels_indices.csv (index,mid,display_name; names may hold commas and quotes), in class order"""
    with open(path, "r", newline="") as f:
        rows = list(csv.reader(f))[1:]
    return [r[2] if len(r) > 2 else (r[1] if len(r) > 1 else str(i)) for i, r in enumerate(rows)]


def _lib_and_stream():
    from .ops import lib, _stream
    return lib(), _stream()


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _check_items(items, n_items, what):
    """host sequence of ints -> int32 numpy [B]; ValueError for anything outside [0, n_items)"""
    arr = np.asarray(items)
    if arr.ndim != 1 or arr.size == 0 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError("%s: items must be a non-empty 1-D sequence of ints" % what)
    bad = np.flatnonzero((arr < 0) | (arr >= n_items))
    if bad.size:
        raise ValueError("%s: item %d of the batch is row %d; the split holds %d" % (what, int(bad[0]), int(arr[bad[0]]), n_items))
    return arr.astype(np.int32)


class ClsEvaluator:
    """Collects one epoch of per-clip scores in class-major matrices on the device.  add() and absorb() queue work on the current
    stream and return; nothing in them waits for the device."""

    def __init__(self, n_items, n_classes, lds_rows=None, device=None):
        self.n_items, self.n_classes = int(n_items), int(n_classes)
        self.lds_rows = 0 if lds_rows is None else int(lds_rows)
        if self.n_items < 1 or self.n_classes < 1:
            raise ValueError("ClsEvaluator: n_items and n_classes must be positive, not %d and %d" % (self.n_items, self.n_classes))
        if self.n_items > MAX_ROWS:
            raise ValueError("ClsEvaluator: %d items; the capacity is %d (M3T_CLS_EVAL_MAX_ROWS)" % (self.n_items, MAX_ROWS))
        if self.lds_rows < 0:
            raise ValueError("ClsEvaluator: lds_rows must be positive")
        if not torch.cuda.is_available():
            raise _lib.M3THipError("m3t.cls_evaluate needs the GPU: the M3T path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self._reset()

    def _reset(self):
        M, Cn, dev = self.n_items, self.n_classes, self.device
        self.scores = torch.zeros(Cn, M, dtype=torch.float32, device=dev)
        self.labels = torch.zeros(Cn, M, dtype=torch.uint8, device=dev)
        self.seen = torch.zeros(M, dtype=torch.uint8, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int32, device=dev)
        self._loss, self._correct, self._items, self._keep = [], [], [], []

    def _scatter(self, scores, labels, items, what):
        if not (isinstance(scores, torch.Tensor) and scores.is_cuda and scores.dtype == torch.float32 and scores.dim() == 2):
            raise _lib.M3THipError("%s: the scores must be a float32 CUDA tensor [B, C]" % what)
        B, Cn = scores.shape
        if Cn != self.n_classes:
            raise ValueError("%s: %d classes per row, the evaluator holds %d" % (what, Cn, self.n_classes))
        if not (isinstance(labels, torch.Tensor) and labels.is_cuda and labels.dtype == torch.float32 and tuple(labels.shape) == (B, Cn)):
            raise ValueError("%s: the labels must be a float32 CUDA tensor [%d, %d]" % (what, B, Cn))
        if isinstance(items, torch.Tensor) and items.is_cuda:          # another rank's shard, as gathered: the kernel skips a row outside
            if items.dtype != torch.int32 or items.dim() != 1:
                raise ValueError("%s: device items must be int32 [B]" % what)
            rows = items.contiguous()
        else:
            host = torch.from_numpy(_check_items(items.tolist() if isinstance(items, torch.Tensor) else items, self.n_items, what))
            self._keep.append(host)                                    # the source of the non-blocking copy: alive until finish()
            rows = host.to(self.device, non_blocking=True)
        if rows.numel() != B:
            raise ValueError("%s: %d score rows, %d items" % (what, B, rows.numel()))
        scores, labels = scores.detach().contiguous(), labels.detach().contiguous()
        lib, stream = _lib_and_stream()
        rc = lib.m3t_cls_eval_append(_ptr(scores), _ptr(labels), _ptr(rows), B, Cn, self.n_items, _ptr(self.scores), _ptr(self.labels),
                                     _ptr(self.seen), _ptr(self.counters), stream)
        _lib.check(rc, "m3t_cls_eval_append")
        return rows

    def add(self, pooled, labels, items, loss, correct):
        """pooled [B, C] float32: the per-clip logits (ops.pooled_cls_loss(..., return_pooled=True)); labels [B, C] float32; items: the
        clips' indices in the split, a host sequence of B ints (validated here, uploaded without a sync); loss (0-dim) and correct [B]:
        the batch's validation_step figures, kept on the device."""
        self._items.append(self._scatter(pooled, labels, items, "ClsEvaluator.add"))
        self._loss.append(loss.detach())
        self._correct.append(correct.detach())

    def absorb(self, scores, labels, items):
        """the same scatter for rows that come from another rank's evaluator (its shard()): scores / labels [B, C] float32, items a host
        sequence or an int32 device tensor.  Rows both hold (DistributedSampler's padding) carry equal values."""
        self._scatter(scores, labels, items, "ClsEvaluator.absorb")

    def shard(self):
        """(scores [n, C] float32, labels [n, C] float32, items int32 [n]) on the device: the rows add() was given, in that order"""
        if not self._items:
            raise ValueError("ClsEvaluator.shard: nothing was added")
        items = torch.cat(self._items)
        idx = items.to(torch.int64)
        return (self.scores.index_select(1, idx).t().contiguous(), self.labels.index_select(1, idx).t().to(torch.float32).contiguous(), items)

    def finish(self):
        if not self._loss:
            raise ValueError("ClsEvaluator.finish: no batches were added")
        M, Cn, dev = self.n_items, self.n_classes, self.device
        lib, stream = _lib_and_stream()
        ws_bytes = int(lib.m3t_cls_eval_rank_ws_bytes(Cn, M, self.lds_rows))
        ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=dev) if ws_bytes else None
        out = torch.empty(8 + 4 * Cn, dtype=torch.float64, device=dev)
        per = C.c_void_p(out.data_ptr() + 64)
        rc = lib.m3t_cls_eval_rank(_ptr(self.scores), _ptr(self.labels), Cn, M, self.lds_rows, _ptr(ws) if ws is not None else None,
                                   ws_bytes, per, stream)
        _lib.check(rc, "m3t_cls_eval_rank")
        _lib.check(lib.m3t_cls_eval_reduce(per, Cn, _ptr(self.seen), M, _ptr(self.counters), _ptr(out), stream), "m3t_cls_eval_reduce")
        # _classification_epoch_end's two reductions (models/vox2_model.py), float32 as there; widened exactly and read back with the rest
        avg_loss = torch.stack(self._loss).mean()
        hits = torch.cat(self._correct)
        tail = torch.stack([avg_loss.to(torch.float64), torch.sum(hits).to(torch.float64)])
        vals = torch.cat([out, tail]).tolist()                          # the epoch's one read-back
        n_hits = len(hits)
        self.seen.zero_()                                               # ready for the next epoch: `seen` says which rows are this epoch's
        self.counters.zero_()
        self._loss, self._correct, self._items, self._keep = [], [], [], []
        head, table, (loss, n_correct) = vals[:8], np.asarray(vals[8:8 + 4 * Cn], np.float64).reshape(Cn, 4), vals[-2:]
        if int(head[4]):
            raise ValueError("ClsEvaluator.finish: %d of the %d items were never appended" % (int(head[4]), M))
        metrics = {"val_loss": loss, "val_acc": n_correct / n_hits, "val_map": head[0], "val_auc": head[1], "val_dprime": dprime(head[1]),
                   "n_classes_ap": int(head[2]), "n_classes_auc": int(head[3]), "n_nonfinite": int(head[5]), "n_bad_labels": int(head[6])}
        per_class = {"ap": table[:, 0].copy(), "auc": table[:, 1].copy(), "P": table[:, 2].astype(np.int64), "N": table[:, 3].astype(np.int64)}
        return ClsEvalResult(metrics, per_class)


class ClsEvalResult:
    """metrics: METRIC_KEYS as Python numbers; per_class: {'ap', 'auc' float64 [C] (NaN: not scored), 'P', 'N' int64 [C]}."""

    def __init__(self, metrics, per_class):
        self.metrics, self.per_class = metrics, per_class

    def _names(self, names):
        Cn = len(self.per_class["ap"])
        if names is None:
            return [str(c) for c in range(Cn)]
        if isinstance(names, (str, os.PathLike)):
            names = read_class_names(names)
        if len(names) != Cn:
            raise ValueError("ClsEvalResult: %d names for %d classes" % (len(names), Cn))
        return list(names)

    def report(self, names=None, top=10, out=print):
        """Prints mAP, mean AUC and d', then the classes with the lowest and the highest AP as `name value` lines (EvalResult.
        smoothed_report's layout; a class that is not scored is in neither list), and returns them.  names: a list, or the path of
        class_labels_indices.csv."""
        m = self.metrics
        names = self._names(names)
        out(m["val_map"])
        out(m["val_auc"])
        out(m["val_dprime"])
        ap = dict((n, float(v)) for n, v in zip(names, self.per_class["ap"]) if v == v)
        for title, sign in (("Lowest AP:", 1), ("Highest AP:", -1)):
            out(title)
            for name, val in sorted(ap.items(), key=lambda kv: sign * kv[1])[:top]:
                out("%s %s" % (name, val))
        return {"ap": ap, "map": m["val_map"], "auc": m["val_auc"], "dprime": m["val_dprime"]}

    def save(self, path, names=None):
        """<path without extension>.json: the metrics (NaN / Infinity as Python's json writes them); .csv: class,name,ap,auc,P,N"""
        root = os.path.splitext(path)[0]
        with open(root + ".json", "w") as f:
            json.dump(self.metrics, f, indent=1, sort_keys=True)
            f.write("\n")
        names = self._names(names)
        with open(root + ".csv", "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["class", "name", "ap", "auc", "P", "N"])
            for c, name in enumerate(names):
                w.writerow([c, name, repr(float(self.per_class["ap"][c])), repr(float(self.per_class["auc"][c])),
                            int(self.per_class["P"][c]), int(self.per_class["N"][c])])
        return root + ".json", root + ".csv"
