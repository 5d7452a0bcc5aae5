"""The AffWild2 epoch feed: from a dataset folder to the batch dicts the task module trains and evaluates on.

The reference's loader (`models/dataset.py`, `AffWild2SequenceDataset` behind a `DataLoader`) scans the folder, plans an epoch's windows and
draws, and cuts, decodes and augments every window on the host.  Each of those steps has a device-side counterpart in this package
(m3t.dataset.TrackStore, m3t.jpeg.FrameStore, m3t.video); this module is what joins them, and the one rule none of them holds: the ORDER
in which an epoch consumes `random`, `np.random` and torch's generator.

  scan_affwild      the reference's `__init__` (`dataset.py:111-175`): the folder and the split files -> Corpus.  Host only.
  Corpus            the mapping m3t.dataset.layout takes, per video the frame paths m3t.jpeg.FrameStore takes, the window plan
  AffWild2Feed      plan_epoch(epoch) -> [BatchPlan], host only; iterating it yields the batch dicts: TrackStore.collate and, for the visual
                    modalities, FrameStore.decode, both queued on the current stream; set_epoch / state_dict / load_state_dict
  BatchPlan         one batch: items [(video, start, track_len)], the clips' draws, the batch's index in the epoch

The order of an epoch (`num_workers=0`, which is what the draws of the reference are reproducible for):
  * construction: `random.shuffle` of `list(range(n)) * windows_per_epoch` (training); the `eval_items` list otherwise (`dataset.py:134-146`);
  * the index order is torch's: the plan runs a `torch.utils.data.DataLoader` over a data set whose items are the draws, built with the
    reference's arguments (`model.py:409-446`) -- `shuffle=True` for training (`RandomSampler`), `SequentialSampler` otherwise, a
    `DistributedSampler` when world > 1 (with set_epoch) -- so the order, and what the loader itself takes from torch's generator when an
    epoch starts, are torch's own by construction, the way m3t/trainer.py uses torch's scheduler classes;
  * per item, in this order: `random.choice(avail[video])` (training); for a visual modality `random.random() > 0.5` (the mirror draw, made
    in every split: the reference evaluates it as an argument, `dataset.py:258`); then m3t.video.draw_affwild: crop x, crop y from `random`,
    the cutout's y, x from `np.random`.  Modality 'audio' draws the choice only.
The items of a batch are drawn when the batch is asked for, as the reference's loader does; plan_epoch is that iteration run to its end.

Everything down to "which windows, which draws" runs without a GPU and without initialising one; the stores are built when the first batch
is asked for (or by build_stores()).

One deviation, on purpose: with `resample` the reference forces the unlabelled rows of the valence / arousal track to zero while it
scans the windows (`dataset.py:202`) -- and forgets to when it reads the windows from its cache file instead (`:180-181`).  Here the labels
are the zeroed track whether or not a cache was read.

Out of scope: prefetch threads and a second stream for the next batch (the persistent scans own the CUs: a concurrent decode stream is not
added here), a host arena for a corpus larger than the device, a disk cache of the parsed frame store, the VoxCeleb2 (mp4) loader (the
AudioSet one is m3t/audioset.py), multi-GPU measurements (the sharding rule is tested on the host).
"""
import os
import pickle
import random
import warnings
from collections import OrderedDict

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

from . import dataset as _dataset
from . import video as _video

FOLDS = {"train": "Training_Set", "val": "Validation_Set"}
SPLITS = ("train", "val", "test")
MODALITIES = ("audio", "visual", "audiovisual")


# ---- the folder scan ------------------------------------------------------------------------------------------------------------------
class Corpus:
    """What scan_affwild found.  videos: the ordered mapping name -> dict m3t.dataset.layout takes ('nb_frames', 'fps' and, by modality and
    split, 'se', 'au', 'mel' (memory-mapped), 'va', 'expr', 'has_image'); frames: name -> [path | None] per frame, what m3t.jpeg.FrameStore
    takes (None for modality 'audio'); avail: name -> window starts (training; None otherwise); names; split, modality, release,
    input_size, window, resample, path, base."""
    __slots__ = ("videos", "frames", "avail", "names", "split", "modality", "release", "input_size", "window", "resample", "path", "base")

    @property
    def nb_frames(self):
        return [self.videos[n]["nb_frames"] for n in self.names]


def cache_name(release, split, window, modality, resample):
    """the reference's two cache file names (`dataset.py:179, :219`)"""
    return "%s_%s_%s%d_%s.pkl" % (release, split, "noisybalancedwindow" if resample else "window", window, modality)


def _lines(path, video, what):
    try:
        with open(path, "r") as f:
            return f.read().splitlines()
    except OSError as e:
        who = "" if video is None else "video %r: " % (video,)
        raise ValueError("scan_affwild: %sno %s: %s (%s)" % (who, what, path, e.strerror or e)) from None


def _track(path, video, what):
    try:
        a = np.load(path, mmap_mode="r")
    except OSError as e:
        raise ValueError("scan_affwild: video %r: no %s: %s (%s)" % (video, what, path, e.strerror or e)) from None
    except ValueError as e:
        raise ValueError("scan_affwild: video %r: %s %s cannot be read: %s" % (video, what, path, e)) from None
    return a


def scan_affwild(path, split, modality, release="vipl", input_size=256, splits_dir="splits", resample=False, window=32, cache_dir=None):
    """The reference's `AffWild2SequenceDataset.__init__` (`dataset.py:111-175`), rule for rule -> Corpus.  Host only.
      * frames lie under `path`/cropped_aligned (release 'ibug') or `path`/face_{input_size}, frame i of a video at `<name>/{i+1:05d}.jpg`;
      * `splits_dir`/frames_fps.csv (name,frames,fps) gives nb_frames and fps, `splits_dir`/{split}.csv the videos, in order; modality
        'audio' drops the videos below 15 fps;
      * unless split == 'test': valence / arousal from `path`/annotations/VA_Set/{Training_Set | Validation_Set}/<name>.txt (float32,
        comma separated, one header line); expression labels from `path`/annotations/EXPR_Set/<fold>/<name>.txt (int64, one header line)
        for the videos of the split that `splits_dir`/expr.csv (name,fold) lists;
      * `path`/se101_feats/<name>.npy, AU_feats/<name>.npy (visual modalities) and mel_spec/<name>.npy (audio modalities) are opened
        memory-mapped; the mel file may be absent below 15 fps (zero audio, `dataset.py:277-278`) and only there;
      * has_image is os.path.exists of every frame file, over len(va) frames on a labelled split and nb_frames on 'test';
      * training: the window plan per video -- m3t.dataset.available_windows, or with resample=True noisy_balanced_windows, whose va'
        replaces the video's 'va'.  With cache_dir the plan is read from / written to the reference's file there (cache_name; a pickle
        of name -> list of starts); default: no file is read or written.
    Every refusal is a ValueError that names the video and the file."""
    if split not in SPLITS:
        raise ValueError("scan_affwild: split must be one of %s, got %r" % (SPLITS, split))
    if modality not in MODALITIES:
        raise ValueError("scan_affwild: modality must be one of %s, got %r" % (MODALITIES, modality))
    window = int(window)
    if window <= 0:
        raise ValueError("scan_affwild: window must be positive")
    visual, audio, labelled = "visual" in modality, "audio" in modality, split != "test"
    c = Corpus()
    c.split, c.modality, c.release, c.input_size, c.window, c.resample, c.path = split, modality, release, int(input_size), window, bool(resample), path
    c.base = os.path.join(path, "cropped_aligned" if release == "ibug" else "face_%d" % int(input_size))
    fps_file = os.path.join(splits_dir, "frames_fps.csv")
    nb_frames, fps = {}, {}
    for n, l in enumerate(_lines(fps_file, None, "frame counts")):
        try:
            name, frames, rate = l.split(",")
            nb_frames[name], fps[name] = int(frames), float(rate)
        except ValueError:
            raise ValueError("scan_affwild: %s, line %d: expected name,frames,fps, got %r" % (fps_file, n + 1, l)) from None
    split_file = os.path.join(splits_dir, "%s.csv" % split)
    names = _lines(split_file, None, "video list")
    for name in names:
        if name not in nb_frames:
            raise ValueError("scan_affwild: video %r of %s is not listed in %s" % (name, split_file, fps_file))
    if modality == "audio":
        names = [n for n in names if fps[n] >= 15.0]
    if not names:
        raise ValueError("scan_affwild: %s lists no video (modality %r)" % (split_file, modality))
    expr_fold = {}
    if labelled:
        expr_file = os.path.join(splits_dir, "expr.csv")
        wanted = set(names)
        for n, l in enumerate(_lines(expr_file, None, "expression list")):
            try:
                name, fold = l.split(",")
            except ValueError:
                raise ValueError("scan_affwild: %s, line %d: expected name,fold, got %r" % (expr_file, n + 1, l)) from None
            if name in wanted:
                expr_fold[name] = fold
    c.videos, c.frames, c.names = OrderedDict(), (OrderedDict() if visual else None), list(names)
    for name in names:
        d = {"nb_frames": nb_frames[name], "fps": fps[name]}
        if labelled:
            va_file = os.path.join(path, "annotations", "VA_Set", FOLDS[split], name + ".txt")
            try:
                d["va"] = np.loadtxt(_lines(va_file, name, "valence / arousal annotation"), delimiter=",", skiprows=1, dtype=np.float32).reshape(-1, 2)
            except ValueError as e:
                if str(e).startswith("scan_affwild"):
                    raise
                raise ValueError("scan_affwild: video %r: %s cannot be read as float32 rows of two: %s" % (name, va_file, e)) from None
            if d["va"].shape[0] == 0:
                raise ValueError("scan_affwild: video %r: %s holds no row" % (name, va_file))
            if name in expr_fold:
                ex_file = os.path.join(path, "annotations", "EXPR_Set", expr_fold[name], name + ".txt")
                try:
                    d["expr"] = np.loadtxt(_lines(ex_file, name, "expression annotation"), skiprows=1, dtype=np.int64).reshape(-1)
                except ValueError as e:
                    if str(e).startswith("scan_affwild"):
                        raise
                    raise ValueError("scan_affwild: video %r: %s cannot be read as int64 rows: %s" % (name, ex_file, e)) from None
        if visual:
            d["se"] = _track(os.path.join(path, "se101_feats", name + ".npy"), name, "SENet feature track")
            d["au"] = _track(os.path.join(path, "AU_feats", name + ".npy"), name, "AU feature track")
            count = d["va"].shape[0] if labelled else nb_frames[name]
            fold = os.path.join(c.base, name)
            files = [os.path.join(fold, "%05d.jpg" % (i + 1)) for i in range(count)]
            d["has_image"] = np.array([os.path.exists(f) for f in files], bool)
            c.frames[name] = [f if ok else None for f, ok in zip(files, d["has_image"])]
        if audio:
            mel_file = os.path.join(path, "mel_spec", name + ".npy")
            if fps[name] >= 15.0 or os.path.exists(mel_file):
                d["mel"] = _track(mel_file, name, "log-Mel track (the video has %g fps: only below 15 may it be absent)" % fps[name])
        c.videos[name] = d
    c.avail = None
    if split == "train":
        c.avail = _window_plan(c, cache_dir)
    return c


def _window_plan(c, cache_dir):
    """name -> window starts of the training split (`dataset.py:177-239`), through the reference's cache file when cache_dir is given"""
    plan, cache = None, None
    if cache_dir is not None:
        cache = os.path.join(cache_dir, cache_name(c.release, c.split, c.window, c.modality, c.resample))
        if os.path.exists(cache):
            with open(cache, "rb") as f:
                plan = pickle.load(f)
            if not isinstance(plan, dict) or any(n not in plan or len(plan[n]) == 0 and c.modality != "audio" for n in c.names):
                raise ValueError("scan_affwild: the window cache %s does not cover the videos of this split" % cache)
    fresh = plan is None
    if fresh:
        plan = {}
    for name in c.names:
        d = c.videos[name]
        try:
            if c.resample:
                starts, d["va"] = _dataset.noisy_balanced_windows(d["va"], d.get("has_image"), c.window, c.modality)
            elif fresh:
                starts = _dataset.available_windows(d.get("has_image"), _dataset.has_label(d["va"]), c.window, c.modality)
        except ValueError as e:
            raise ValueError("scan_affwild: video %r: %s (window %d, frames under %s)" % (name, e, c.window, os.path.join(c.base, name))) from None
        if fresh:
            plan[name] = [int(s) for s in starts]
    if fresh and cache is not None:
        os.makedirs(cache_dir, exist_ok=True)
        tmp = "%s.tmp.%d" % (cache, os.getpid())
        with open(tmp, "wb") as f:
            pickle.dump(plan, f)
        os.replace(tmp, cache)
    return plan


# ---- the epoch plan -------------------------------------------------------------------------------------------------------------------
class BatchPlan:
    """One batch of an epoch.  items: [(video index, start, track_len)]; aug: one m3t.video.draw_affwild dict per item (None for modality
    'audio'); index: the batch's position in the epoch; indices: the data set indices the sampler gave."""
    __slots__ = ("items", "aug", "index", "indices")

    def __init__(self, items, aug, index, indices):
        self.items, self.aug, self.index, self.indices = items, aug, index, indices

    def __eq__(self, other):
        return (isinstance(other, BatchPlan) and self.items == other.items and self.index == other.index and self.indices == other.indices
                and _aug_key(self.aug) == _aug_key(other.aug))

    def __repr__(self):
        return "BatchPlan(index=%d, items=%r, aug=%r)" % (self.index, self.items, self.aug)


def _aug_key(aug):
    return None if aug is None else [(a["cy"], a["cx"], a["size"], a["mirror"], a["cutout"], a.get("scale", 1)) for a in aug]


class _Draws(Dataset):
    """the data set the plan's DataLoader reads: item i is (i, video, start, track_len, draw), drawn when it is read"""

    def __init__(self, feed):
        self.feed = feed

    def __len__(self):
        return len(self.feed.sample_src)

    def __getitem__(self, i):
        f = self.feed
        if f.training:
            v = f.sample_src[i]
            start, tl = random.choice(f._avail[v]), f.window
        else:
            v, start, tl = f.sample_src[i]
        aug = None
        if f.visual:
            mirror = random.random() > 0.5
            aug = _video.draw_affwild(f.input_size, f.training, f.release == "vipl", f.cutout, mirror, resize=f.input_size > 128)
        return int(i), int(v), int(start), int(tl), aug


class AffWild2Feed:
    """An epoch of AffWild2 batches from a Corpus (scan_affwild), as the reference's DataLoader over its AffWild2SequenceDataset gives them.

    window, batch_size, split, modality, cutout, input_size, release, windows_per_epoch, inv_test_stride: the reference's (`dataset.py:111`,
    `model.py:409-446`); split, modality, window, input_size and release must be the corpus's.  rank / world: world > 1 shards the indices
    with torch's DistributedSampler (the reference's default one: shuffled, seed 0, set_epoch(epoch)).  sampler: overrides the index order
    -- any iterable of indices, or a callable that makes one from the data set.  visual: the model's front-end, kept as `model_visual` for a
    caller that ingests outside the model (m3t.video.ingest_for(feed.model_visual, ...)); the feed itself hands on the uint8 frames.

    Construction draws the training split's `random.shuffle` and touches no device.  plan_epoch(epoch) is host only.  Iterating builds the
    stores on the current device at the first batch (one TrackStore; for a visual modality one FrameStore, whose has_image arrays the
    TrackStore gets) and yields, per BatchPlan, TrackStore.collate(items) with 'video' (uint8 frames as decoded), 'video_aug' (the draws) and
    'video_frame_idx' added for a visual modality: what AffWild2VA.forward / training_step / validation_step and Evaluator.add take.
    Everything is validated for the whole batch before its first launch and queued on the current stream; there is no read-back per
    batch.  Decode status words other than "ok" are read back once when the epoch ends: `decode_errors` [(video, frame, status)] and ONE
    warning; the epoch is not stopped."""

    def __init__(self, corpus, window, batch_size, split, modality, cutout=False, input_size=256, release="vipl", windows_per_epoch=200,
                 inv_test_stride=1, rank=0, world=1, sampler=None, visual=None):
        for k, v in (("split", split), ("modality", modality), ("window", int(window)), ("input_size", int(input_size)), ("release", release)):
            if getattr(corpus, k) != v:
                raise ValueError("AffWild2Feed: %s is %r, the corpus was scanned with %r" % (k, v, getattr(corpus, k)))
        self.corpus, self.window, self.batch_size, self.split, self.modality = corpus, int(window), int(batch_size), split, modality
        self.cutout, self.input_size, self.release = bool(cutout), int(input_size), release
        self.windows_per_epoch, self.inv_test_stride, self.rank, self.world = int(windows_per_epoch), int(inv_test_stride), int(rank), int(world)
        if self.batch_size <= 0 or self.windows_per_epoch <= 0:
            raise ValueError("AffWild2Feed: batch_size and windows_per_epoch must be positive")
        if self.world <= 0 or not 0 <= self.rank < self.world:
            raise ValueError("AffWild2Feed: rank %d outside a world of %d" % (self.rank, self.world))
        self.training, self.visual = split == "train", "visual" in modality
        self.names = list(corpus.names)
        self.model_visual = visual
        if self.visual:      # an input_size the ingest refuses is refused here (an evaluation draw: no random number is consumed)
            _video.draw_affwild(self.input_size, False, release == "vipl", False, False, resize=self.input_size > 128)
        if self.training:
            self._avail = [corpus.avail[n] for n in self.names]
            for n, a in zip(self.names, self._avail):
                if not a:
                    raise ValueError("AffWild2Feed: video %r has no window of %d frames to draw from" % (n, self.window))
            self.sample_src = list(range(len(self.names))) * self.windows_per_epoch
            random.shuffle(self.sample_src)
        else:
            self._avail = None
            self.sample_src = _dataset.eval_items(corpus.nb_frames, self.window, self.inv_test_stride)
        self._draws = _Draws(self)
        self._sampler = sampler(self._draws) if callable(sampler) else sampler
        self._dist = None
        if self._sampler is None and self.world > 1:
            self._sampler = self._dist = DistributedSampler(self._draws, num_replicas=self.world, rank=self.rank)
        self._loader = DataLoader(self._draws, batch_size=self.batch_size, shuffle=self.training and self._sampler is None,
                                  sampler=self._sampler, num_workers=0, collate_fn=list)
        self.epoch = 0
        self.tracks = self.frames = None
        self.decode_errors = []

    # ---- host ----
    def __len__(self):
        return len(self._loader)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def plans(self, epoch=None):
        """the epoch's BatchPlans one at a time, each drawn when it is asked for (the reference's order with num_workers=0)"""
        if epoch is not None:
            self.set_epoch(epoch)
        if self._dist is not None:
            self._dist.set_epoch(self.epoch)
        elif hasattr(self._sampler, "set_epoch"):
            self._sampler.set_epoch(self.epoch)
        for b, rows in enumerate(self._loader):
            yield BatchPlan([(v, s, tl) for _, v, s, tl, _ in rows], [r[4] for r in rows] if self.visual else None, b, [r[0] for r in rows])

    def plan_epoch(self, epoch=None):
        """-> [BatchPlan] of one epoch (default: the current one); host only, no device is touched.  Consumes the epoch's random numbers."""
        return list(self.plans(epoch))

    def state_dict(self):
        """what a resume between two epochs needs: the epoch, the training split's shuffled order, and the states of `random`, `np.random`
        and torch's default generator"""
        kind, keys, pos, has_gauss, gauss = np.random.get_state()
        return {"epoch": self.epoch, "sample_src": list(self.sample_src) if self.training else None, "random": random.getstate(),
                "numpy": (kind, np.array(keys, copy=True), int(pos), int(has_gauss), float(gauss)), "torch": torch.get_rng_state().clone()}

    def load_state_dict(self, state):
        if self.training:
            src = list(state["sample_src"])
            if sorted(src) != sorted(self.sample_src):
                raise ValueError("AffWild2Feed.load_state_dict: the saved order is of another set of videos or windows_per_epoch")
            self.sample_src = src
        self.epoch = int(state["epoch"])
        random.setstate(state["random"])
        np.random.set_state(tuple(state["numpy"]))
        torch.set_rng_state(state["torch"])

    # ---- device ----
    def build_stores(self):
        """the TrackStore and, for a visual modality, the FrameStore of the corpus on the current device (once)"""
        if self.tracks is not None:
            return self
        videos = self.corpus.videos
        if self.visual:
            from . import jpeg
            self.frames = jpeg.FrameStore(self.corpus.frames, self.window)
            videos = OrderedDict()
            for n in self.names:
                present = self.frames.has_image(n)
                if not np.array_equal(present, self.corpus.videos[n]["has_image"]):
                    raise ValueError("AffWild2Feed: video %r: the frame store holds other frames than the scan found; the window plan was made on the scan's" % (n,))
                videos[n] = dict(self.corpus.videos[n], has_image=present)
        self.tracks = _dataset.TrackStore(videos, self.window, self.split)
        return self

    def batch(self, plan):
        """one BatchPlan -> the batch dict, queued on the current stream.  Host validation of every stage first, then the launches: each
        store validates its own call before it launches, so the track store's and the ingest's checks are made ahead (the cheap ones) and the
        frame store, which repeats nothing, goes first (the ingest's frame index is video.frame_index's, inside [-1, window) by construction)."""
        self.build_stores()
        if self.visual:
            _dataset.plan(self.tracks.meta, plan.items, self.window, self.split)
            _video.plan((len(plan.items), self.window, self.frames.height, self.frames.width, 3), torch.uint8, plan.aug)
            frames, frame_idx, status = self.frames.decode(plan.items)
        batch = self.tracks.collate(plan.items)
        if self.visual:
            if not torch.equal(frame_idx, batch["video_frame_idx"]):
                raise AssertionError("AffWild2Feed: the frame store's and the track store's frame index tables differ (batch %d)" % plan.index)
            batch["video"], batch["video_aug"], batch["video_frame_idx"] = frames, plan.aug, frame_idx
            self._status.append((plan.items, status))
        return batch

    def __iter__(self):
        self.build_stores()
        self._status = []
        self.decode_errors = []
        try:
            for plan in self.plans():
                yield self.batch(plan)
        finally:
            self._report()

    def _report(self):
        """the epoch's decode status words, read back once"""
        held, self._status = self._status, []
        if not held:
            return
        words = torch.cat([s for _, s in held]).cpu().numpy()
        bad = np.flatnonzero(words)
        if bad.size == 0:
            return
        first = np.cumsum([0] + [len(items) * self.window for items, _ in held])
        seen = set()
        for k in bad:
            b = int(np.searchsorted(first, k, side="right")) - 1
            n, t = divmod(int(k - first[b]), self.window)
            v, start, _ = held[b][0][n]
            key = (self.names[v], start + t)
            if key not in seen:
                seen.add(key)
                self.decode_errors.append(key + (int(words[k]),))
        shown = ", ".join("%s frame %d (status %d)" % e for e in self.decode_errors[:8])
        warnings.warn("AffWild2Feed: %d frame(s) of epoch %d did not decode cleanly: %s%s" % (
            len(self.decode_errors), self.epoch, shown, " ..." if len(self.decode_errors) > 8 else ""), RuntimeWarning, stacklevel=2)


def feed_from_hparams(hparams, split, rank=0, world=1, visual=None, cache_dir=None):
    """the feed of one split with the reference's arguments (`model.py:409-446`): inv_test_stride 2 for 'test' and for 'val' under
    test_on_val; hparams.splits_dir (default 'splits'); `--mode` other than 'video' raises NotImplementedError as the reference does"""
    hp = hparams
    if getattr(hp, "mode", "video") != "video":
        raise NotImplementedError("mode %r: the reference implements the 'video' loader only (models/model.py:413-415)" % (hp.mode,))
    stride = 2 if (split == "test" or (split == "val" and getattr(hp, "test_on_val", False))) else 1
    corpus = scan_affwild(hp.dataset_path, split, hp.modality, hp.release, hp.input_size, getattr(hp, "splits_dir", "splits"),
                          bool(getattr(hp, "resample", False)), hp.window, cache_dir)
    return AffWild2Feed(corpus, hp.window, hp.batch_size, split, hp.modality, bool(getattr(hp, "cutout", False)), hp.input_size, hp.release,
                        hp.windows_per_epoch, stride, rank, world, visual=visual)
