"""An evaluation epoch on the device (csrc/evaluate.hip): what the reference does in validation_step /
validation_end / test_step / test_end (models/model.py:226-303, 320-373) and get_smoothed_ccc.py, without a host read-back
per batch.  The host-side route (AffWild2VA's own hooks, m3t/stitch.py, postproc.smoothed_ccc_report) stays as it is; this
module computes the same tracks bit for bit and the same metrics from fp64 sums.

  ev = Evaluator(window, overlap=hparams.test_on_val)      # overlap=False: validation_end's torch.cat per video
  for batch in loader:
      ev.add(model(batch), batch)                           # one m3t_eval_append launch, nothing read back
  res = ev.finish()                                         # cat, plan, one gather launch, one metrics launch, ONE read-back
  res.metrics, res.to_dicts(), res.save('predictions_val.pt'), res.smoothed_report()

`plan_tracks` is the index arithmetic alone (numpy, no GPU).  There is no CPU path for the rest.

Evaluator(..., expr=True) also carries the expression head (channels 0..6 of a 9-channel `mtl` output, which the reference
trains, model.py:169-182, and never validates; csrc/evaluate_expr.hip): add() is still one launch (m3t_eval_append_mtl),
finish() still one read-back, and the result gains res.expr (logits [7, F], pred [F], gt [F]), val_acc_expr / val_f1_expr /
val_score_expr, res.expr_metrics and res.expr_report().  `expr_metrics_from_confusion` is the same arithmetic on the host.
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib

METRIC_KEYS = ("val_ccc_v", "val_ccc_a", "val_mse_v", "val_mse_a", "val_loss")
EXPR_METRIC_KEYS = ("val_acc_expr", "val_f1_expr", "val_score_expr")
EXPR_CLASSES = ("Neutral", "Anger", "Disgust", "Fear", "Happiness", "Sadness", "Surprise")
N_EXPR = len(EXPR_CLASSES)
NO_HALVING = 1 << 62

# the expression tracks of an epoch on the device: logits [7, F] fp32, pred [F] int8 (-1: no window covers the frame),
# gt [F] int8 (-1: not annotated; None without labels)
ExprTracks = namedtuple("ExprTracks", "logits pred gt")

# names: videos in first-seen order; nframes [V]; frame_off / seg_off [V+1]; seg_dst / seg_len / seg_row [S], grouped by
# video and sorted by destination (seg_row = the window's index in the order it was added); halve_from: see m3t_eval_gather
Plan = namedtuple("Plan", "names nframes frame_off seg_off seg_dst seg_len seg_row halve_from")


def plan_tracks(names, starts, lengths, window, overlap):
    """Where every window goes.  names / starts / lengths: one entry per window, in the order the windows were added.
    overlap: the reference's overlap-add (test_end, and validation_end under test_on_val): a window lands at its start frame
    and everything from frame window // 2 on is halved.  Otherwise validation_end's torch.cat: the windows of a video one
    after the other in start order, whether or not they overlap.  A window holds at most T = `window` frames.
    ValueError: two windows of a video with the same start, a length outside [1, T], a negative start, a window that ends
    after the video's last window does (the video has last.start + last.length frames, as in the reference)."""
    T = int(window)
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    if not (len(names) == starts.size == lengths.size):
        raise ValueError("plan_tracks: %d names, %d starts, %d lengths" % (len(names), starts.size, lengths.size))
    if starts.size and int(starts.min()) < 0:
        raise ValueError("plan_tracks: negative start frame %d" % int(starts.min()))
    if lengths.size and (int(lengths.min()) < 1 or int(lengths.max()) > T):
        bad = lengths[(lengths < 1) | (lengths > T)][0]
        raise ValueError("plan_tracks: window length %d outside [1, %d]" % (int(bad), T))
    by_video = {}
    for row, name in enumerate(names):
        by_video.setdefault(name, []).append(row)
    seg_dst, seg_len, seg_row, seg_off, nframes = [], [], [], [0], []
    for name, rows in by_video.items():
        rows = np.asarray(rows, dtype=np.int64)
        rows = rows[np.argsort(starts[rows], kind="stable")]
        st, ln = starts[rows], lengths[rows]
        if st.size > 1 and bool((st[1:] == st[:-1]).any()):
            raise ValueError("plan_tracks: two windows of video %r start at frame %d" % (name, int(st[1:][st[1:] == st[:-1]][0])))
        dst = st if overlap else np.concatenate([[0], np.cumsum(ln)[:-1]])
        if int((dst + ln).max()) > int(dst[-1] + ln[-1]):
            # the reference sizes the track by its last window and fails on the `+=` of a window that runs past it
            raise ValueError("plan_tracks: a window of video %r runs past the end its last window sets (frame %d)" % (name, int(dst[-1] + ln[-1])))
        seg_dst.append(dst); seg_len.append(ln); seg_row.append(rows)
        seg_off.append(seg_off[-1] + rows.size)
        nframes.append(int(dst[-1] + ln[-1]))
    cat = lambda parts: np.concatenate(parts).astype(np.int64) if parts else np.zeros(0, np.int64)
    nframes = np.asarray(nframes, dtype=np.int64)
    return Plan(list(by_video), nframes, np.concatenate([[0], np.cumsum(nframes)]).astype(np.int64),
                np.asarray(seg_off, dtype=np.int64), cat(seg_dst), cat(seg_len), cat(seg_row),
                int(window) // 2 if overlap else NO_HALVING)


def expr_metrics_from_confusion(conf):
    """conf [..., 7, 7] integer counts, conf[g][p] = frames with label g and prediction p (leading axes are summed: windows,
    videos, shards) -> what m3t_eval_expr_metrics writes, in numpy float64: {'acc', 'f1', 'score', 'precision' [7],
    'recall' [7], 'f1_class' [7]}.  F1_c = 2 tp / (2 tp + fp + fn); f1 = the mean over the classes with tp + fp + fn > 0 in
    class order (scikit-learn's f1_score(average='macro')); score = 0.67 f1 + 0.33 acc (ABAW 2020, expression track).  A zero
    denominator is NaN: everything without a frame, precision of a class never predicted, recall of one never labelled."""
    c = np.asarray(conf)
    if c.ndim < 2 or c.shape[-2:] != (N_EXPR, N_EXPR):
        raise ValueError("expr_metrics_from_confusion: conf must be [..., %d, %d], not %s" % (N_EXPR, N_EXPR, list(c.shape)))
    c = c.astype(np.int64).reshape(-1, N_EXPR, N_EXPR).sum(0)
    tp = np.diag(c)
    fp, fn = c.sum(0) - tp, c.sum(1) - tp
    f = lambda a: a.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        prec, rec, f1c = f(tp) / f(tp + fp), f(tp) / f(tp + fn), f(2 * tp) / f(2 * tp + fp + fn)
        present = (tp + fp + fn) > 0
        f1sum = np.float64(0.0)
        for k in range(N_EXPR):
            if present[k]:
                f1sum = f1sum + f1c[k]
        acc = np.float64(tp.sum()) / np.float64(c.sum())
        f1 = f1sum / np.float64(int(present.sum()))
    return {"acc": float(acc), "f1": float(f1), "score": float(np.float64(0.67) * f1 + np.float64(0.33) * acc),
            "precision": prec, "recall": rec, "f1_class": f1c}


def _expr_table(vals):
    """out24 of m3t_eval_expr_metrics (a list of floats) -> the three figures and the per-class table"""
    return vals[:3], {"precision": dict(zip(EXPR_CLASSES, vals[3:10])), "recall": dict(zip(EXPR_CLASSES, vals[10:17])),
                      "f1": dict(zip(EXPR_CLASSES, vals[17:24]))}


def _lib_and_stream():
    from .ops import lib, _stream          # (ops imports torch.distributed and the GRU plumbing: not needed for plan_tracks)
    return lib(), _stream()


def _device():
    if not torch.cuda.is_available():
        raise _lib.M3THipError("m3t.evaluate needs the GPU: the M3T path has no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _ptr(t):
    return C.c_void_p(t.data_ptr())


class Evaluator:
    """Collects one epoch of windows on the device.  add() queues work on the current stream and returns; nothing in it
    waits for the device."""

    def __init__(self, window, overlap, with_gt=True, expr=False):
        self.window, self.overlap, self.with_gt, self.expr = int(window), bool(overlap), bool(with_gt), bool(expr)
        self._reset()

    def _reset(self):
        self._rows, self._part, self._names, self._starts, self._lengths, self._keep = [], [], [], [], [], []
        self._erows, self._egt, self._conf = [], [], []

    def add(self, y_hat, batch):
        """y_hat [N, T, C] (fp32, CUDA): the model's output for `batch`; valence = channel C-2, arousal = C-1.  batch:
        'vid_name' (N names), 'start', 'length' ([N] integer tensors, CPU or CUDA) and, with_gt, 'label_valence' /
        'label_arousal' [N, T].  expr=True: C >= 9, the expression logits are channels 0..6, and with_gt also takes
        'class_expr' (integer classes) and 'expr_valid' [N, T], CPU or CUDA."""
        y = y_hat.detach()
        if self.expr:                                # (what can be said without the device comes first)
            if y.dim() == 3 and y.size(2) < N_EXPR + 2:
                raise ValueError("Evaluator.add: expr=True needs the %d expression logits and valence, arousal (C >= %d); y_hat has %d "
                                 "channels -- fusion_type att_dec and losses without `mtl` have no expression head" % (N_EXPR, N_EXPR + 2, y.size(2)))
            for k in ("class_expr", "expr_valid") if self.with_gt else ():
                if k not in batch:
                    raise ValueError("Evaluator.add: expr=True with labels needs batch[%r]" % k)
        if not y.is_cuda or y.dtype != torch.float32 or y.dim() != 3 or y.size(2) < 2:
            raise _lib.M3THipError("Evaluator.add: y_hat must be a float32 CUDA tensor [N, T, C >= 2]")
        y = y.contiguous()
        N, T, Cn = y.shape
        if T != self.window:
            raise ValueError("Evaluator.add: y_hat has %d frames per clip, the window is %d" % (T, self.window))
        names = list(batch["vid_name"])
        start, length = torch.as_tensor(batch["start"]), torch.as_tensor(batch["length"])
        if not (len(names) == N == start.numel() == length.numel()):
            raise ValueError("Evaluator.add: %d outputs, %d names, %d starts, %d lengths" % (N, len(names), start.numel(), length.numel()))
        dev = y.device
        keep = []                                    # host sources of the non-blocking copies: alive until finish()

        def up(t, dtype):
            t = t.detach().to(dtype)
            if not t.is_cuda:
                keep.append(t)
            return t.to(dev, non_blocking=True).contiguous()
        len_dev = up(length.reshape(-1), torch.int64)
        lv = la = None
        if self.with_gt:
            lv, la = up(batch["label_valence"], torch.float32), up(batch["label_arousal"], torch.float32)
            if tuple(lv.shape) != (N, T) or tuple(la.shape) != (N, T):
                raise ValueError("Evaluator.add: labels must be [%d, %d]" % (N, T))
        cls = vld = None
        if self.expr and self.with_gt:
            cls, vld = up(torch.as_tensor(batch["class_expr"]), torch.int64), up(torch.as_tensor(batch["expr_valid"]), torch.uint8)
            if tuple(cls.shape) != (N, T) or tuple(vld.shape) != (N, T):
                raise ValueError("Evaluator.add: class_expr and expr_valid must be [%d, %d]" % (N, T))
        Q = 4 if self.with_gt else 2
        rows = torch.empty(N, Q, T, dtype=torch.float32, device=dev)
        part = torch.empty(N, 2, 7, dtype=torch.float64, device=dev) if self.with_gt else None
        opt = lambda t: _ptr(t) if t is not None else None
        lib, stream = _lib_and_stream()
        if self.expr:
            erows = torch.empty(N, N_EXPR, T, dtype=torch.float32, device=dev)
            egt = torch.empty(N, T, dtype=torch.int8, device=dev) if self.with_gt else None
            conf = torch.empty(N, N_EXPR, N_EXPR, dtype=torch.int32, device=dev) if self.with_gt else None
            rc = lib.m3t_eval_append_mtl(_ptr(y), N, T, Cn, opt(lv), opt(la), opt(cls), opt(vld), _ptr(len_dev), _ptr(rows),
                                         opt(part), _ptr(erows), opt(egt), opt(conf), stream)
            _lib.check(rc, "m3t_eval_append_mtl")
            self._erows.append(erows)
            if self.with_gt:
                self._egt.append(egt)
                self._conf.append(conf)
        else:
            rc = lib.m3t_eval_append(_ptr(y), N, T, Cn, opt(lv), opt(la), _ptr(len_dev), _ptr(rows), opt(part), stream)
            _lib.check(rc, "m3t_eval_append")
        self._rows.append(rows)
        if self.with_gt:
            self._part.append(part)
        self._names += names
        self._starts.append(start.reshape(-1))       # a CUDA tensor is copied to the host in finish(), not here
        self._lengths.append(length.reshape(-1))
        self._keep.append(keep)

    @staticmethod
    def _to_host(parts):
        """[N_i] integer tensors, some on the device -> one int64 numpy array (one device-to-host copy for the CUDA ones)"""
        cuda = [p for p in parts if p.is_cuda]
        if cuda:
            host = iter(torch.split(torch.cat([p.to(torch.int64) for p in cuda]).cpu(), [p.numel() for p in cuda]))
            parts = [next(host) if p.is_cuda else p for p in parts]
        return torch.cat([p.to(torch.int64) for p in parts]).numpy()

    def finish(self):
        if not self._rows:
            raise ValueError("Evaluator.finish: no windows were added")
        dev = self._rows[0].device
        plan = plan_tracks(self._names, self._to_host(self._starts), self._to_host(self._lengths), self.window, self.overlap)
        rows = torch.cat(self._rows) if len(self._rows) > 1 else self._rows[0]
        W, Q, T = rows.shape
        V, F, S = len(plan.names), int(plan.frame_off[-1]), plan.seg_dst.size
        table = torch.from_numpy(np.concatenate([plan.seg_dst, plan.seg_len, plan.seg_row, plan.seg_off, plan.frame_off]))
        table = table.to(dev)
        tracks = torch.empty(Q, F, dtype=torch.float32, device=dev)
        at = lambda k: C.c_void_p(table.data_ptr() + 8 * k)
        lib, stream = _lib_and_stream()
        rc = lib.m3t_eval_gather(_ptr(rows), W, Q, T, at(0), at(S), at(2 * S), at(3 * S), at(3 * S + V + 1), V, F,
                                 plan.halve_from, _ptr(tracks), stream)
        _lib.check(rc, "m3t_eval_gather")
        one = lambda parts: torch.cat(parts) if len(parts) > 1 else parts[0]
        expr = None
        if self.expr:
            erows, egt = one(self._erows), one(self._egt) if self.with_gt else None
            expr = ExprTracks(torch.empty(N_EXPR, F, dtype=torch.float32, device=dev), torch.empty(F, dtype=torch.int8, device=dev),
                              torch.empty(F, dtype=torch.int8, device=dev) if self.with_gt else None)
            rc = lib.m3t_eval_gather_expr(_ptr(erows), _ptr(egt) if self.with_gt else None, W, T, at(0), at(S), at(2 * S), at(3 * S),
                                          at(3 * S + V + 1), V, F, plan.halve_from, _ptr(expr.logits), _ptr(expr.pred),
                                          _ptr(expr.gt) if self.with_gt else None, stream)
            _lib.check(rc, "m3t_eval_gather_expr")
        metrics = expr_metrics = None
        if self.with_gt:
            part = one(self._part)
            out = torch.empty(5 + 24 * self.expr, dtype=torch.float64, device=dev)         # the VA figures, then the expression ones
            _lib.check(lib.m3t_eval_metrics(_ptr(part), W, _ptr(out), stream), "m3t_eval_metrics")
            if self.expr:
                conf = one(self._conf)
                _lib.check(lib.m3t_eval_expr_metrics(_ptr(conf), W, C.c_void_p(out.data_ptr() + 8 * 5), stream), "m3t_eval_expr_metrics")
            vals = out.tolist()                                    # the epoch's one read-back
            metrics = dict(zip(METRIC_KEYS, vals[:5]))
            if self.expr:
                three, expr_metrics = _expr_table(vals[5:])
                metrics.update(zip(EXPR_METRIC_KEYS, three))
        self._reset()                                              # ready for the next epoch
        return EvalResult(plan.names, plan.frame_off, tracks, metrics, expr, expr_metrics)


class EvalResult:
    """names: the videos; frame_off [V+1] (numpy int64); tracks [Q, F] fp32 on the device, Q = valence_pred, arousal_pred
    (, valence_gt, arousal_gt), video v at tracks[:, frame_off[v]:frame_off[v+1]]; metrics: stitch.val_metrics' keys as
    Python floats (None without labels).  From Evaluator(expr=True): expr = ExprTracks(logits [7, F], pred [F], gt [F] or
    None) on the device with the same frame layout, metrics also holds val_acc_expr / val_f1_expr / val_score_expr, and
    expr_metrics = {'precision' | 'recall' | 'f1': {class name: float}}; otherwise expr and expr_metrics are None."""

    def __init__(self, names, frame_off, tracks, metrics=None, expr=None, expr_metrics=None):
        self.names, self.frame_off, self.tracks, self.metrics = list(names), np.asarray(frame_off, dtype=np.int64), tracks, metrics
        self.expr, self.expr_metrics = expr, expr_metrics

    @property
    def with_gt(self):
        return self.tracks.size(0) == 4

    def to_dicts(self):
        """the dict validation_end saves as predictions_val.pt (test_end: predictions_test.pt, predictions only): per-video
        CPU tensors.  A result with expression tracks adds expr_logits {video: [n, 7] fp32}, expr_pred {video: [n] int8} and,
        with labels, expr_gt {video: [n] int8}."""
        host = self.tracks.cpu()
        lens = np.diff(self.frame_off).tolist()
        split = lambda t: {n: x.clone() for n, x in zip(self.names, torch.split(t, lens))}
        per = lambda q: split(host[q])
        if self.with_gt:
            d = {"valence_gt": per(2), "arousal_gt": per(3), "valence_pred": per(0), "arousal_pred": per(1)}
        else:
            d = {"valence_pred": per(0), "arousal_pred": per(1)}
        if self.expr is not None:
            d["expr_logits"] = split(self.expr.logits.t().contiguous().cpu())
            d["expr_pred"] = split(self.expr.pred.cpu())
            if self.expr.gt is not None:
                d["expr_gt"] = split(self.expr.gt.cpu())
        return d

    def save(self, path):
        torch.save(self.to_dicts(), path)

    @classmethod
    def from_dicts(cls, d):
        """the other way: a loaded predictions_val.pt / predictions_test.pt (tensors or arrays per video)"""
        dev = _device()
        keys = ["valence_pred", "arousal_pred"] + (["valence_gt", "arousal_gt"] if "valence_gt" in d else [])
        names = list(d["valence_gt" if "valence_gt" in d else "valence_pred"].keys())
        flat = lambda x: torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).detach().reshape(-1).to(torch.float32)
        lens = [int(flat(d[keys[0]][n]).numel()) for n in names]
        tracks = torch.stack([torch.cat([flat(d[k][n]) for n in names]) for k in keys]).to(dev)
        expr = None
        if "expr_logits" in d:
            ten = lambda x: torch.as_tensor(np.asarray(x) if not isinstance(x, torch.Tensor) else x).detach()
            logits = torch.cat([ten(d["expr_logits"][n]).to(torch.float32).reshape(-1, N_EXPR) for n in names])
            if logits.size(0) != sum(lens):
                raise ValueError("from_dicts: expr_logits hold %d frames, the valence tracks %d" % (logits.size(0), sum(lens)))
            cat8 = lambda k: torch.cat([ten(d[k][n]).reshape(-1).to(torch.int8) for n in names]).to(dev)
            pred = cat8("expr_pred") if "expr_pred" in d else logits.argmax(1).to(torch.int8).to(dev)
            expr = ExprTracks(logits.t().contiguous().to(dev), pred, cat8("expr_gt") if "expr_gt" in d else None)
        return cls(names, np.concatenate([[0], np.cumsum(lens)]), tracks, None, expr)

    def smoothed_report(self, window=35, mode="wiener", top=10, out=print):
        """postproc.smoothed_ccc_report (get_smoothed_ccc.py:6-43) on the tracks where they are: one smoothing launch, one
        launch for the per-video CCCs, two for the all-video figures, one read-back.  Prints and returns the same."""
        if not self.with_gt:
            raise ValueError("smoothed_report needs the labels (a validation result)")
        if mode not in ("wiener", "median"):
            raise ValueError("mode must be 'wiener' or 'median'")
        V, F = len(self.names), int(self.frame_off[-1])
        if V == 0 or bool((np.diff(self.frame_off) <= 0).any()):
            raise _lib.M3THipError("CCC needs two tracks of the same, non-zero length")
        tr = self.tracks.contiguous()
        dev = tr.device
        offs = torch.from_numpy(np.concatenate([self.frame_off[:-1], self.frame_off + F])).to(dev)
        pred = tr[:2].reshape(-1)                                      # valence tracks, then arousal tracks
        g = tr[2:].reshape(-1)                                         # their labels ...
        g2 = torch.cat([tr[3], tr[2]])                                 # ... and the other track's (both must be annotated)
        sm = torch.empty(2 * F, dtype=torch.float64, device=dev)
        res = torch.empty(2 * V + 2, 2, dtype=torch.float64, device=dev)
        lib, stream = _lib_and_stream()
        _lib.check(lib.m3t_smooth_tracks(_ptr(pred), _ptr(offs), 2 * V, int(window), 1 if mode == "median" else 0, _ptr(sm),
                                         stream), "m3t_smooth_tracks")
        _lib.check(lib.m3t_ccc_tracks(_ptr(sm), _ptr(g), _ptr(g2), _ptr(offs), 2 * V, 1, _ptr(res), stream), "m3t_ccc_tracks")
        for k in (0, 1):
            rc = lib.m3t_ccc_masked(C.c_void_p(sm.data_ptr() + 8 * k * F), C.c_void_p(g.data_ptr() + 4 * k * F),
                                    C.c_void_p(g2.data_ptr() + 4 * k * F), F, 0, C.c_void_p(res.data_ptr() + 16 * (2 * V + k)), stream)
            _lib.check(rc, "m3t_ccc_masked")
        vals = res[:, 0].tolist()                                      # the one read-back
        ccc_v = dict(zip(self.names, vals[:V]))
        ccc_a = dict(zip(self.names, vals[V:2 * V]))
        all_v, all_a = vals[2 * V], vals[2 * V + 1]
        out(all_v)
        out(all_a)
        for title, table, sign in (("Lowest ccc-v:", ccc_v, 1), ("Highest ccc-v:", ccc_v, -1),
                                   ("Lowest ccc-a:", ccc_a, 1), ("Highest ccc-a:", ccc_a, -1)):
            out(title)
            for name, val in sorted(table.items(), key=lambda kv: sign * kv[1])[:top]:
                out("%s %s" % (name, val))
        return {"ccc_v": ccc_v, "ccc_a": ccc_a, "ccc_v_all": all_v, "ccc_a_all": all_a}

    def expr_report(self, window=1, top=10, out=print):
        """The expression counterpart of smoothed_report: a mode filter of `window` frames (odd; 1 = none) over the predicted
        class tracks, one confusion per video, the figures over every frame once -- three launches, one read-back.  Prints
        accuracy, macro-F1 and score = 0.67 F1 + 0.33 accuracy over all videos, then the videos with the lowest and highest
        accuracy (a video without an annotated frame has accuracy NaN and is in neither list), and returns them."""
        if self.expr is None or self.expr.gt is None:
            raise ValueError("expr_report needs expression tracks with labels (Evaluator(expr=True) on a validation epoch)")
        if int(window) < 1 or int(window) % 2 == 0:
            raise ValueError("expr_report: the window must be odd and positive, not %d" % int(window))
        V, F = len(self.names), int(self.frame_off[-1])
        if V == 0:
            raise ValueError("expr_report: no videos")
        pred, gt = self.expr.pred.contiguous(), self.expr.gt.contiguous()
        dev = pred.device
        offs = torch.from_numpy(self.frame_off).to(dev)
        sm = torch.empty(F, dtype=torch.int8, device=dev)
        conf = torch.empty(V, N_EXPR, N_EXPR, dtype=torch.int32, device=dev)
        res = torch.empty(24 + V, dtype=torch.float64, device=dev)     # the figures over all videos, then an accuracy per video
        lib, stream = _lib_and_stream()
        _lib.check(lib.m3t_expr_mode_tracks(_ptr(pred), _ptr(offs), V, int(window), _ptr(sm), stream), "m3t_expr_mode_tracks")
        _lib.check(lib.m3t_expr_track_conf(_ptr(sm), _ptr(gt), _ptr(offs), V, _ptr(conf), C.c_void_p(res.data_ptr() + 8 * 24),
                                           stream), "m3t_expr_track_conf")
        _lib.check(lib.m3t_eval_expr_metrics(_ptr(conf), V, _ptr(res), stream), "m3t_eval_expr_metrics")
        vals = res.tolist()                                            # the one read-back
        (acc_all, f1_all, score_all), per_class = _expr_table(vals[:24])
        acc = dict(zip(self.names, vals[24:]))
        out(acc_all)
        out(f1_all)
        out(score_all)
        ranked = [kv for kv in acc.items() if kv[1] == kv[1]]
        for title, sign in (("Lowest acc-expr:", 1), ("Highest acc-expr:", -1)):
            out(title)
            for name, val in sorted(ranked, key=lambda kv: sign * kv[1])[:top]:
                out("%s %s" % (name, val))
        return {"acc": acc, "acc_all": acc_all, "f1_all": f1_all, "score_all": score_all, "per_class": per_class}
