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
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch

from . import _lib

METRIC_KEYS = ("val_ccc_v", "val_ccc_a", "val_mse_v", "val_mse_a", "val_loss")
NO_HALVING = 1 << 62

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

    def __init__(self, window, overlap, with_gt=True):
        self.window, self.overlap, self.with_gt = int(window), bool(overlap), bool(with_gt)
        self._rows, self._part, self._names, self._starts, self._lengths, self._keep = [], [], [], [], [], []

    def add(self, y_hat, batch):
        """y_hat [N, T, C] (fp32, CUDA): the model's output for `batch`; valence = channel C-2, arousal = C-1.  batch:
        'vid_name' (N names), 'start', 'length' ([N] integer tensors, CPU or CUDA) and, with_gt, 'label_valence' /
        'label_arousal' [N, T]."""
        y = y_hat.detach()
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
        Q = 4 if self.with_gt else 2
        rows = torch.empty(N, Q, T, dtype=torch.float32, device=dev)
        part = torch.empty(N, 2, 7, dtype=torch.float64, device=dev) if self.with_gt else None
        lib, stream = _lib_and_stream()
        rc = lib.m3t_eval_append(_ptr(y), N, T, Cn, _ptr(lv) if self.with_gt else None, _ptr(la) if self.with_gt else None,
                                 _ptr(len_dev), _ptr(rows), _ptr(part) if self.with_gt else None, stream)
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
        metrics = None
        if self.with_gt:
            part = torch.cat(self._part) if len(self._part) > 1 else self._part[0]
            out = torch.empty(5, dtype=torch.float64, device=dev)
            _lib.check(lib.m3t_eval_metrics(_ptr(part), W, _ptr(out), stream), "m3t_eval_metrics")
            metrics = dict(zip(METRIC_KEYS, out.tolist()))         # the epoch's one read-back
        self._rows, self._part, self._names, self._starts, self._lengths, self._keep = [], [], [], [], [], []     # ready for the next epoch
        return EvalResult(plan.names, plan.frame_off, tracks, metrics)


class EvalResult:
    """names: the videos; frame_off [V+1] (numpy int64); tracks [Q, F] fp32 on the device, Q = valence_pred, arousal_pred
    (, valence_gt, arousal_gt), video v at tracks[:, frame_off[v]:frame_off[v+1]]; metrics: stitch.val_metrics' keys as
    Python floats (None without labels)."""

    def __init__(self, names, frame_off, tracks, metrics=None):
        self.names, self.frame_off, self.tracks, self.metrics = list(names), np.asarray(frame_off, dtype=np.int64), tracks, metrics

    @property
    def with_gt(self):
        return self.tracks.size(0) == 4

    def to_dicts(self):
        """the dict validation_end saves as predictions_val.pt (test_end: predictions_test.pt, predictions only): per-video
        CPU tensors"""
        host = self.tracks.cpu()
        lens = np.diff(self.frame_off).tolist()
        per = lambda q: {n: t.clone() for n, t in zip(self.names, torch.split(host[q], lens))}
        if self.with_gt:
            return {"valence_gt": per(2), "arousal_gt": per(3), "valence_pred": per(0), "arousal_pred": per(1)}
        return {"valence_pred": per(0), "arousal_pred": per(1)}

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
        return cls(names, np.concatenate([[0], np.cumsum(lens)]), tracks, None)

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
