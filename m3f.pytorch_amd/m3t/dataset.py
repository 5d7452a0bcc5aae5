"""The AffWild2 loader's collate step with the side tracks resident on the GPU (csrc/collate.hip, m3t_window_collate).

The reference's `AffWild2SequenceDataset.__getitem__` (`models/dataset.py:241-343`) slices, transposes and edge-pads the SENet / AU
feature tracks, stacks the log-Mel rows, slices and pads the labels -- per window, in numpy, on the host -- and the DataLoader stacks the
windows and copies every tensor to the device.  The side data of the whole corpus is a few GB: here it is uploaded ONCE, and a batch of
windows is cut from it by one kernel, from one small int table.

  one_runs / has_label / available_windows / noisy_balanced_windows   the reference's window scans (`dataset.py:36-43, :177-239`), per video
  eval_items / train_items     the window list of a split, in the reference's order and with its `random` draws (`:134-146, :242-250`)
  plan                         host validation of a batch of items, before anything touches a device -> int32 [N, 3]
  layout                       the flat arrays and the per-video table of a set of videos (host only)
  TrackStore                   layout() on the device; collate(items) -> the reference's batch dict; batches(items, batch_size)

An item is (video, start, track_len) -- or (video, start), track_len = window, the training split; `video` is an index or a name.
`batch['video']` stays the caller's (decode, then `m3t.video.ingest`): for a store given `has_image`, collate adds the `video_frame_idx`
rows that go with the frames start .. start + track_len - 1 of each item.  The frames themselves have a resident store of their own,
`m3t.jpeg.FrameStore` (the files' scan bytes on the device, a batch of windows decoded from them; its `has_image(video)` is the array this
store takes).  The file-system scan, the epoch's order of items and draws and the sharding are m3t/feed.py, which drives both stores
(`train_items` draws an epoch's choices in one run; the reference interleaves them with each clip's mirror, crop and cutout draws, which
is the feed's plan).  Out of scope: prefetch threads.
"""
import numpy as np
import torch

from . import _lib
from . import video as _video
from .ops import lib, _stream, M3THipError

TABLE_COLS = 12                     # se_off, se_n, au_off, au_n, mel_off, mel_n, va_off, va_n, expr_off, expr_n, flags, 0 (include/m3t_hip.h)
HAS_EXPR, AUDIO_OK = 1, 2
_KINDS = ("se", "au", "mel", "va", "expr")


# ---- window plans (pure numpy / random) -----------------------------------------------------------------------------------------------
def one_runs(a):
    """int [runs, 2]: (first, one past the last) of every run of entries equal to 1 (`dataset.py:36-43`)"""
    on = np.concatenate(([False], np.equal(np.asarray(a), 1), [False]))
    return np.flatnonzero(on[1:] != on[:-1]).reshape(-1, 2)


def has_label(va):
    """bool [T]: frames whose valence and arousal are both inside [-1, 1] (`dataset.py:185`)"""
    return np.max(np.abs(np.asarray(va)), axis=1) <= 1


def available_windows(has_image, has_label, window, modality):
    """One video's window starts (`dataset.py:217-239`): every start of a full window inside a run of labelled frames (modality 'audio') or
    of frames with both an image and labels (anything else; ValueError when there is none, the reference's assert)."""
    ok = np.asarray(has_label).astype(bool)
    if modality != "audio":
        ok = np.asarray(has_image).astype(bool) & ok
    starts = []
    for first, end in one_runs(ok):
        starts.extend(range(int(first), int(end) - window + 1))
    if modality != "audio" and not starts:
        raise ValueError("no available windows")
    return starts


def noisy_balanced_windows(va, has_image, window, modality):
    """One video's window starts with `--noise_and_balance` (`dataset.py:177-215`) -> (starts, va'): va' is the label track the reference
    leaves behind (unlabelled rows forced to zero for the visual modalities; returned, the argument is not touched).
    'audio': the labelled runs' windows, then some of them again: the reference pairs window k with run k (`zip`), scores the pair by
    the mean valence of the window AT THE RUN'S START, and repeats the windows of the pairs with a negative score; kept as is.
    Otherwise: every start with at most 25 % of its frames missing an image or a label; twice where its mean valence is negative."""
    va = np.array(va, copy=True)
    ok = has_label(va)
    starts = []
    if modality == "audio":
        runs = one_runs(ok)
        for first, end in runs:
            starts.extend(range(int(first), int(end) - window + 1))
        scores = [(w, va[first:first + window, 0].mean()) for w, (first, _) in zip(starts, runs)]
        scores.sort(key=lambda s: s[1])
        below = int(np.searchsorted([s[1] for s in scores], 0))
        starts.extend(s[0] for s in scores[:below])
        return starts, va
    img = np.asarray(has_image).astype(bool)
    va[~ok] = 0
    for s in range(0, len(va) - window + 1):
        missing = max(1 - np.sum(img[s:s + window]) / window, 1 - np.sum(ok[s:s + window]) / window)
        if missing > 0.25:
            continue
        starts.append(s)
        if va[s:s + window, 0].mean() < 0:
            starts.append(s)
    if not starts:
        raise ValueError("no available windows")
    return starts, va


def eval_items(nb_frames, window, inv_test_stride=1):
    """The val / test window list (`dataset.py:141-146, :248-250`): per video in order, starts 0, stride, 2 stride .. < nb_frames with
    stride = window // inv_test_stride -> [(video, start, track_len = min(window, nb_frames - start))]"""
    stride = window // inv_test_stride
    if stride <= 0:
        raise ValueError("eval_items: window // inv_test_stride must be positive")
    return [(v, s, min(window, int(n) - s)) for v, n in enumerate(nb_frames) for s in range(0, int(n), stride)]


def train_items(n_videos, windows_per_epoch, avail, rng):
    """One training epoch's windows with the reference's draws (`dataset.py:137-138, :243-246`): rng.shuffle of list(range(n)) *
    windows_per_epoch, then one rng.choice(avail[video]) per item in iteration order -> [(video, start)]; rng: a random.Random (or the
    `random` module).  avail: window starts per video index (available_windows / noisy_balanced_windows)."""
    src = list(range(n_videos)) * windows_per_epoch
    rng.shuffle(src)
    return [(v, rng.choice(avail[v])) for v in src]


# ---- host validation ------------------------------------------------------------------------------------------------------------------
def plan(videos_meta, items, window, split):
    """Host validation of a batch, before anything touches a device -> int32 [N, 3] = video index, start, track_len.
    videos_meta: per video a dict with 'name' and the row counts 'se', 'au', 'va', 'expr' (None: not stored / no such labels).
    ValueError where the reference raises or would hand the DataLoader a ragged batch: an unknown video, a negative start, track_len
    outside [1, window], start >= the rows of a stored feature track (np.pad 'edge' of an empty slice), and on a labelled split
    (split != 'test') start + track_len beyond the valence / arousal or the expression labels."""
    window = int(window)
    if window <= 0:
        raise ValueError("collate: window must be positive, got %r" % (window,))
    index = {m["name"]: i for i, m in enumerate(videos_meta)}
    table = np.zeros((len(items), 3), np.int32)
    for n, it in enumerate(items):
        if len(it) not in (2, 3):
            raise ValueError("collate: item %d: expected (video, start[, track_len]), got %r" % (n, it))
        v, start = it[0], int(it[1])
        tl = window if len(it) == 2 else int(it[2])
        if isinstance(v, str):
            if v not in index:
                raise ValueError("collate: item %d: unknown video %r" % (n, v))
            v = index[v]
        v = int(v)
        if not 0 <= v < len(videos_meta):
            raise ValueError("collate: item %d: unknown video %d (the store holds %d)" % (n, v, len(videos_meta)))
        m = videos_meta[v]
        if start < 0 or start > 0x7fffffff:
            raise ValueError("collate: item %d: start %d is negative (or beyond 2^31)" % (n, start))
        if not 1 <= tl <= window:
            raise ValueError("collate: item %d: track_len %d outside [1, %d]" % (n, tl, window))
        for kind in ("se", "au"):
            if m.get(kind) is not None and start >= m[kind]:
                raise ValueError("collate: item %d: start %d is past the %d rows of %s's %s track" % (n, start, m[kind], m["name"], kind))
        if split != "test":
            for kind in ("va", "expr"):
                if m.get(kind) is not None and start + tl > m[kind]:
                    raise ValueError("collate: item %d: frames %d .. %d run past the %d %s labels of %s"
                                     % (n, start, start + tl - 1, m[kind], kind, m["name"]))
        table[n] = (v, start, tl)
    return table


def layout(videos, split, se_dim=512, au_dim=256):
    """The store's host image: (meta, table, flat).  videos: an ordered mapping name -> dict of 'nb_frames', 'fps' and the optional arrays
    'mel' [R, n_mels], 'se' [L, >= se_dim], 'au' [L, >= au_dim], 'va' [L, 2] (float32), 'expr' [L] (integers), 'has_image' [L].
    meta: plan()'s per-video dicts (+ 'nb_frames', 'fps', 'has_image'); table: int64 [V, 12] (TABLE_COLS); flat: kind -> one concatenated
    array (float32 kept exactly as given; expr int64), absent for a kind no video has.  A feature kind ('se', 'au') is stored for every
    video or none; 'mel' may be missing where fps < 15 (zero audio, `dataset.py:277-278`) and only there; labels are stored when
    split != 'test', where every video needs 'va' and 'expr' is per video (`dataset.py:285`)."""
    if not videos:
        raise ValueError("TrackStore: no videos")
    labelled = split != "test"
    names = list(videos)
    stored = {k: any(videos[n].get(k) is not None for n in names) for k in _KINDS}
    stored["va"] = stored["expr"] = False
    if labelled:
        stored["va"], stored["expr"] = True, any(videos[n].get("expr") is not None for n in names)
    width = {"se": None, "au": None, "mel": None, "va": 2}
    need = {"se": int(se_dim), "au": int(au_dim), "mel": 1, "va": 2}
    parts = {k: [] for k in _KINDS}
    table = np.zeros((len(names), TABLE_COLS), np.int64)
    meta = []
    for i, name in enumerate(names):
        d = videos[name]
        fps = float(d["fps"])
        m = {"name": name, "nb_frames": int(d["nb_frames"]), "fps": fps, "se": None, "au": None, "va": None, "expr": None,
             "has_image": None if d.get("has_image") is None else np.asarray(d["has_image"]).astype(bool)}
        for col, kind in enumerate(("se", "au", "mel", "va")):
            if not stored[kind]:
                continue
            a = d.get(kind)
            if a is None:
                if kind == "mel" and fps < 15:
                    continue
                raise ValueError("TrackStore: video %r has no %r track" % (name, kind))
            a = np.asarray(a)
            if a.dtype != np.float32 or a.ndim != 2 or a.shape[0] <= 0:
                raise ValueError("TrackStore: %s of %r must be a float32 [rows > 0, width] array, got %s %s" % (kind, name, a.dtype, a.shape))
            if width[kind] is None:
                width[kind] = a.shape[1]
            if a.shape[1] != width[kind] or a.shape[1] < need[kind]:
                raise ValueError("TrackStore: %s of %r is %d wide; the store's rows are %s wide and at least %d are read"
                                 % (kind, name, a.shape[1], width[kind], need[kind]))
            table[i, 2 * col] = sum(p.shape[0] for p in parts[kind])
            table[i, 2 * col + 1] = a.shape[0]
            parts[kind].append(a)
            if kind != "mel":
                m[kind] = int(a.shape[0])
        if stored["expr"] and d.get("expr") is not None:
            e = np.asarray(d["expr"])
            if not np.issubdtype(e.dtype, np.integer) or e.ndim != 1 or e.shape[0] <= 0:
                raise ValueError("TrackStore: expr of %r must be a 1-D integer array" % (name,))
            table[i, 8] = sum(p.shape[0] for p in parts["expr"])
            table[i, 9] = e.shape[0]
            parts["expr"].append(e.astype(np.int64))
            m["expr"] = int(e.shape[0])
            table[i, 10] |= HAS_EXPR
        if fps >= 15 and stored["mel"]:
            table[i, 10] |= AUDIO_OK
        meta.append(m)
    flat = {k: np.ascontiguousarray(np.concatenate(p)) for k, p in parts.items() if p}
    return meta, table, flat


# ---- the store ------------------------------------------------------------------------------------------------------------------------
class TrackStore:
    """The side tracks of a set of videos on the current device, and the collate step over them.

    videos: layout()'s mapping; window: frames per item; split: 'train' / 'val' / 'test' (labels are stored and returned unless 'test').
    se_dim / au_dim: the leading columns of a feature row that a batch carries (the reference reads 512 and `[:, :256]` of 268);
    step / width: the log-Mel context stack (`dataset.py:88`: rows 3 i .. 3 i + 5).  One upload per track kind, at construction."""

    def __init__(self, videos, window, split, se_dim=512, au_dim=256, step=3, width=5):
        self.window, self.split, self.se_dim, self.au_dim, self.step, self.width = int(window), split, int(se_dim), int(au_dim), int(step), int(width)
        if self.window <= 0 or self.step <= 0 or self.width <= 0 or self.se_dim <= 0 or self.au_dim <= 0:
            raise ValueError("TrackStore: window, se_dim, au_dim, step and width must be positive")
        self.meta, self.table, flat = layout(videos, split, se_dim, au_dim)
        self.names = [m["name"] for m in self.meta]
        if not torch.cuda.is_available():
            raise M3THipError("m3t.dataset.TrackStore needs the GPU: the M3T path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device())
        self.arrays = {k: torch.from_numpy(a).to(self.device) for k, a in flat.items()}
        self.videos = torch.from_numpy(self.table.reshape(-1)).to(self.device)
        self.labelled = split != "test"
        self.n_mels = int(flat["mel"].shape[1]) if "mel" in flat else 0
        self.has_image = any(m["has_image"] is not None for m in self.meta)

    @property
    def nbytes(self):
        """bytes of device memory the store holds"""
        return sum(t.numel() * t.element_size() for t in self.arrays.values()) + self.videos.numel() * 8

    def _arg(self, kind):
        t = self.arrays.get(kind)
        return (None, 0, 0) if t is None else (t.data_ptr(), t.shape[0], t.shape[1] if t.dim() == 2 else 1)

    def collate(self, items):
        """items: [(video, start[, track_len])] -> the reference's batch: 'vid_name' (names), 'start', 'length' (CPU int64 [N]) and, on the
        store's device and the current stream, 'se_features' [N, se_dim, window], 'au_features' [N, au_dim, window] (if stored), 'audio'
        [N, window, width n_mels] (if stored; zeros where fps < 15), and unless split == 'test' 'label_valence', 'label_arousal' [N, window]
        float32, 'class_expr' int64, 'expr_valid' bool; 'video_frame_idx' int32 [N, window] (host) where has_image was given: the
        m3t.video.frame_index rows for the frames start .. start + track_len - 1 the caller decodes.  plan() first (ValueError), then one
        upload of the item table and one launch."""
        tab = plan(self.meta, items, self.window, self.split)
        N, W = int(tab.shape[0]), self.window
        if torch.cuda.current_device() != self.device.index:
            raise M3THipError("TrackStore.collate: the store lives on %s, the current device is cuda:%d" % (self.device, torch.cuda.current_device()))
        batch = {"vid_name": [self.names[v] for v in tab[:, 0]],
                 "start": torch.from_numpy(tab[:, 1].astype(np.int64)), "length": torch.from_numpy(tab[:, 2].astype(np.int64))}
        dev = self.device
        new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        se, au, mel = self.arrays.get("se"), self.arrays.get("au"), self.arrays.get("mel")
        if se is not None:
            batch["se_features"] = new((N, self.se_dim, W))
        if au is not None:
            batch["au_features"] = new((N, self.au_dim, W))
        if mel is not None:
            batch["audio"] = new((N, W, self.width * self.n_mels))
        if self.labelled:
            batch["label_valence"], batch["label_arousal"] = new((N, W)), new((N, W))
            batch["class_expr"], batch["expr_valid"] = new((N, W), torch.int64), new((N, W), torch.bool)
        if self.has_image:
            rows = []
            for v, start, tl in tab:
                present = self.meta[v]["has_image"]
                if present is None:
                    raise ValueError("collate: video %r has no has_image array" % (self.names[v],))
                rows.append(_video.frame_index(present[start:start + tl], 0, int(tl), W))
            batch["video_frame_idx"] = torch.from_numpy(np.stack(rows)) if rows else torch.zeros((0, W), dtype=torch.int32)
        if N == 0:
            return batch
        items_dev = torch.from_numpy(tab.reshape(-1)).to(dev, non_blocking=True)
        p = lambda k: batch[k].data_ptr() if k in batch else None
        se_a, au_a, mel_a, va_a, ex_a = (self._arg(k) for k in _KINDS)
        _lib.check(lib().m3t_window_collate(se_a[0], se_a[1], se_a[2], self.se_dim, au_a[0], au_a[1], au_a[2], self.au_dim,
                                            mel_a[0], mel_a[1], self.n_mels, self.step, self.width, va_a[0], va_a[1], ex_a[0], ex_a[1],
                                            self.videos.data_ptr(), len(self.meta), items_dev.data_ptr(), N, W,
                                            p("se_features"), p("au_features"), p("audio"), p("label_valence"), p("label_arousal"),
                                            p("class_expr"), p("expr_valid"), _stream()), "m3t_window_collate")
        return batch

    def batches(self, items, batch_size):
        """collate() over consecutive slices of `items`; the last one may be short"""
        batch_size = int(batch_size)
        if batch_size <= 0:
            raise ValueError("batches: batch_size must be positive")
        for i in range(0, len(items), batch_size):
            yield self.collate(items[i:i + batch_size])
