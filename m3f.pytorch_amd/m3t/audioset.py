"""The AudioSet epoch feed: from a dataset folder to the batch dicts `models.audioset_model.AudioSet` pre-trains on (stage 2 of the
reference's workflow).  The reference's loader (`models/audioset_dataset.py`, `AudioSetDataset` behind a `DataLoader`) scans the folder,
and per item decodes a whole 10 s clip with librosa, crops it, and computes the log-Mel rows on the host.  Here:

  scan_audioset   the reference's `__init__` (`audioset_dataset.py:99-121`), rule for rule -> Scan (files, uint8 label matrix).  Host only.
  WaveStore       every clip of a split read once (m3t/wav.py) into ONE flat int16 device buffer, the label matrix beside it as uint8;
                  with convert=True clips of any rate, channel count and sample kind, converted on the device (m3t.audio.decode_waves) into
                  ONE flat float32 buffer of 16 kHz mono
  AudioSetFeed    plan_epoch(epoch) -> [BatchPlan], host only; iterating it yields {'audio': float32 [N, window, 200], 'label': float32
                  [N, 527]} on the current stream -- what the reference's loader yields, so AudioSet.training_step / validation_step take it
                  unchanged; set_epoch / state_dict / load_state_dict
  BatchPlan       one batch: the clips' indices, their draws (m3t.audio.draw_audioset), the batch's index in the epoch

The order of an epoch (`num_workers=0`, which is what the reference's draws are reproducible for) is the reference's by construction: the
plan runs torch's own `DataLoader` over a small data set whose item i is (i, draw), drawn when it is read -- `shuffle=True` for training,
sequential otherwise (`audioset_model.py:129-145`), torch's default `DistributedSampler` in BOTH splits when world > 1 (the reference's
`--distributed`).  Per item `random.choice(FPS_VALUES)` then `random.randint(0, tot - nsamples)` (training; `audioset_dataset.py:60, :69`);
an evaluation item draws nothing.

A batch is one small table upload (the ingest's per-clip table and the clips' indices in one copy), ONE launch for the labels
(m3t_label_rows, csrc/audioset.hip) and the ingest's launches (m3t.audio.ingest_planned), which read the crops out of the store in place:
no sample crosses the bus after the store is built, and nothing is read back.

Everything down to "which clips, which draws" runs without a GPU and without initialising one (the clips' lengths come from the files'
headers); the store is built when the first batch is asked for (or by build_store()).

Training-time augmentation, opt-in and for the train split only: `spec_augment` draws the reference's own frequency and time masks
(`audioset_dataset.py:17-55`, m3t.audio.draw_spec_augment) per item, after that item's draws above; `mixup_alpha` draws per batch, right
after its items, `np.random.beta(alpha, alpha, N)` and then `np.random.permutation(N)`.  Both are applied inside the launches a batch
already has (m3t_audio_db_stack_aug, m3t_label_rows_mix); with both off the plans, the generators and the launches are what they were.

Without `convert` a clip that is not 16 kHz, 16-bit, mono is refused with its name, as before.  Out of scope: a
disk cache or a host arena for the store (balanced train is about 7 GB of int16, 14 GB of float32: it fits), prefetch threads, time
warping (the reference removed it), balanced sampling, the VoxCeleb2 loader, multi-GPU measurements (the sharding rule is tested on the host).
"""
import os
import random

import numpy as np
import torch
from torch.utils.data import DataLoader, Dataset
from torch.utils.data.distributed import DistributedSampler

from . import _lib
from . import audio as _audio
from . import wav as _wav
from .ops import lib, _stream, M3THipError

FOLD_MAP = {"train": "balanced_train_segments", "val": "eval_segments"}       # audioset_dataset.py:104
N_CLASSES = 527
SR = 16000
CHUNK_BYTES = 64 << 20


# ---- the folder scan ------------------------------------------------------------------------------------------------------------------
class Scan:
    """What scan_audioset found.  files: the clips' paths in the reference's order; labels: uint8 [F, 527], 1 where the reference's float
    vector is 1.0; split, path.  lengths() reads the files' headers (once) -> int64 [F] samples; a rate other than 16 kHz or an empty clip is
    refused there, with the file named.  A scan made with convert=True takes every file m3t.wav.probe_wave takes, and a clip's length is
    m3t.audio.converted_length of its header -- what the reference's `len(y)` after `librosa.load(path, sr=16000)` would be."""
    __slots__ = ("files", "labels", "split", "path", "convert", "_lengths")

    def __len__(self):
        return len(self.files)

    def lengths(self):
        if self._lengths is None:
            self._lengths = np.array([_clip_samples(f, self.convert) for f in self.files], np.int64)
        return self._lengths


def _clip_samples(path, convert=False):
    if convert:
        info = _wav.probe_wave(path)
        if info.frames <= 0:
            raise ValueError("%s: an empty clip (no whole frame in its 'data' chunk)" % (path,))
        return _audio.converted_length(info.frames, info.rate)
    n, rate = _wav.probe_pcm16(path)
    _check_clip(path, n, rate)
    return n


def _check_clip(path, n, rate):
    if rate != SR:
        raise ValueError("%s: sampled at %d Hz; the store takes %d Hz only (resampling is out of scope: convert the folder first)" % (path, rate, SR))
    if n <= 0:
        raise ValueError("%s: an empty clip (no whole sample in its 'data' chunk)" % (path,))


def _lines(path, what):
    try:
        with open(path, "r") as f:
            return f.read().splitlines()
    except OSError as e:
        raise ValueError("scan_audioset: no %s: %s (%s)" % (what, path, e.strerror or e)) from None


def scan_audioset(path, split, convert=False):
    """The reference's `AudioSetDataset.__init__` (`audioset_dataset.py:99-121`), rule for rule -> Scan.  Host only.
      * `path`/class_labels_indices.csv without its first line: the mid of class i is `l.split(',')[1]` of line i (display names may hold
        commas and quotes: they come third);
      * `path`/{balanced_train_segments | eval_segments}.csv without its first THREE lines: `name, start, end, "mid,mid,..."` split at
        ', ' into four; the mids are `ontology[1:-1].split(',')`;
      * the clip is `path`/<fold>/<name>.wav; a listed clip without a file is skipped silently, before its labels are looked at.
    Where the reference dies with a bare ValueError (a line that does not split into four) or KeyError (a mid that is not in the class
    list), this refuses with the file and the line named."""
    if split not in FOLD_MAP:
        raise ValueError("scan_audioset: split must be one of %s, got %r" % (tuple(FOLD_MAP), split))
    fold = FOLD_MAP[split]
    class_file, annot_file = os.path.join(path, "class_labels_indices.csv"), os.path.join(path, "%s.csv" % fold)
    mid_map = {}
    for i, l in enumerate(_lines(class_file, "class list")[1:]):
        parts = l.split(",")
        if len(parts) < 2:
            raise ValueError("scan_audioset: %s, line %d: expected index,mid,display_name, got %r" % (class_file, i + 2, l))
        mid_map[parts[1]] = i
    if any(i >= N_CLASSES for i in mid_map.values()):
        raise ValueError("scan_audioset: %s lists more than %d classes" % (class_file, N_CLASSES))
    files, rows = [], []
    for n, l in enumerate(_lines(annot_file, "segment list")[3:]):
        parts = l.split(", ")
        if len(parts) != 4:
            raise ValueError("scan_audioset: %s, line %d: expected 'name, start, end, \"mids\"' (four parts at ', '), got %r" % (annot_file, n + 4, l))
        name, _, _, ontology = parts
        wav_path = os.path.join(path, fold, name + ".wav")
        if not os.path.exists(wav_path):
            continue
        row = np.zeros(N_CLASSES, np.uint8)
        for mid in ontology[1:-1].split(","):
            if mid not in mid_map:
                raise ValueError("scan_audioset: %s, line %d: label %r of clip %r is not in %s" % (annot_file, n + 4, mid, name, class_file))
            row[mid_map[mid]] = 1
        files.append(wav_path)
        rows.append(row)
    s = Scan()
    s.files, s.split, s.path, s.convert, s._lengths = files, split, path, bool(convert), None
    s.labels = np.stack(rows) if rows else np.zeros((0, N_CLASSES), np.uint8)
    return s


# ---- the resident store ---------------------------------------------------------------------------------------------------------------
def plan_batch(wave, offsets, lengths, items, draws, window):
    """Host validation of one batch out of a store, before anything touches a device: wave, the store's flat buffer (only its size and dtype
    are looked at); offsets, lengths int64 [F]; items, the clips' indices; draws, one m3t.audio.draw_audioset dict per item or None.
    -> (items int64 [N], table int64 [N, 8], R) -- m3t.audio.plan_waves' store form.  ValueError for an item outside the store.
    (The augmentation of a batch is validated beside it: m3t.audio.plan_aug on the same draws and table.)"""
    items = np.asarray(items)
    if items.ndim != 1 or items.size == 0 or not np.issubdtype(items.dtype, np.integer):
        raise ValueError("WaveStore: a batch needs a non-empty 1-D list of clip indices")
    items = items.astype(np.int64)
    F = int(np.asarray(offsets).shape[0])
    for n in np.flatnonzero((items < 0) | (items >= F)):
        raise ValueError("WaveStore: item %d of the batch is clip %d; the store holds %d" % (n, items[n], F))
    _, table, R = _audio.plan_waves(wave, draws, window, lengths=np.asarray(lengths)[items], offsets=np.asarray(offsets)[items])
    return items, table, R


class WaveStore:
    """The clips of a split on the device.  files: paths read once with m3t.wav.read_pcm16 (a rate other than 16 kHz or an empty clip is
    refused with the file named); labels: uint8 [F, n_classes] or None.  The samples go to ONE flat int16 device buffer `wave`, staged
    through a host buffer of at most `chunk_bytes` (a longer clip goes on its own): the host never holds the corpus.  offsets, lengths:
    int64 [F] on the host, clip i = wave[offsets[i] : offsets[i] + lengths[i]]; label_table: the uint8 matrix on the device.
    lengths (optional): what the files' headers said; the store refuses a file that now reads differently.
    convert=True: every file m3t.wav.read_wave takes, of any rate; the raw bytes go up through a pinned stage of at most `chunk_bytes` and
    m3t.audio.decode_waves turns them into 16 kHz mono on the device, so `wave` is ONE flat float32 buffer (the ingest reads either dtype in
    place) and a clip's length is m3t.audio.converted_length of its header.  A 16 kHz, 16-bit, mono clip holds int16 / 32768 exactly."""

    def __init__(self, files, labels=None, lengths=None, chunk_bytes=CHUNK_BYTES, device=None, convert=False):
        files = list(files)
        if not files:
            raise ValueError("WaveStore: no files")
        if labels is not None:
            labels = np.ascontiguousarray(labels)
            if labels.dtype != np.uint8 or labels.ndim != 2 or labels.shape[0] != len(files):
                raise ValueError("WaveStore: labels must be uint8 [%d, classes]" % len(files))
        if not torch.cuda.is_available():
            raise M3THipError("m3t.audioset.WaveStore needs the GPU: the M3T path has no CPU fallback")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.files = files
        self.convert = bool(convert)
        self.label_table = None if labels is None else torch.from_numpy(labels).to(self.device)
        self.n_classes = 0 if labels is None else int(labels.shape[1])
        if self.convert:
            self.wave, self.offsets, self.lengths = _audio.decode_waves(files, self.device, chunk_bytes)
            if lengths is not None and not np.array_equal(np.asarray(lengths, np.int64), self.lengths):
                i = int(np.flatnonzero(np.asarray(lengths, np.int64) != self.lengths)[0])
                raise ValueError("%s: %d samples after conversion, %d expected from its header when the epoch was planned"
                                 % (files[i], self.lengths[i], np.asarray(lengths)[i]))
            return
        if lengths is None:
            lengths = [_clip_samples(f) for f in files]
        self.lengths = np.asarray(lengths, np.int64).copy()
        if self.lengths.shape != (len(files),) or self.lengths.min() <= 0:
            raise ValueError("WaveStore: one positive length per file is needed")
        self.offsets = np.concatenate([[0], np.cumsum(self.lengths)[:-1]]).astype(np.int64)
        total = int(self.lengths.sum())
        self.wave = torch.empty(total, dtype=torch.int16, device=self.device)
        cap = max(int(chunk_bytes) // 2, 1)
        stage, fill, base = np.empty(min(cap, total), np.int16), 0, 0

        def flush():
            nonlocal fill, base
            if fill:
                self.wave[base:base + fill].copy_(torch.from_numpy(stage[:fill]))      # (pageable memory: the copy has ended when this returns)
                base, fill = base + fill, 0

        for i, f in enumerate(files):
            y, rate = _wav.read_pcm16(f)
            _check_clip(f, y.shape[0], rate)
            if y.shape[0] != self.lengths[i]:
                raise ValueError("%s: %d samples read, %d expected from its header when the epoch was planned" % (f, y.shape[0], self.lengths[i]))
            if y.shape[0] > stage.shape[0] - fill:
                flush()
            if y.shape[0] > stage.shape[0]:
                self.wave[base:base + y.shape[0]].copy_(torch.from_numpy(y))
                base += y.shape[0]
            else:
                stage[fill:fill + y.shape[0]] = y
                fill += y.shape[0]
        flush()
        assert base == total

    def __len__(self):
        return len(self.files)

    @property
    def nbytes(self):
        return int(self.wave.numel()) * self.wave.element_size() + (0 if self.label_table is None else int(self.label_table.numel()))

    def plan(self, items, draws, window):
        return plan_batch(self.wave, self.offsets, self.lengths, items, draws, window)

    def label_rows(self, items_dev, N, mix=None):
        """float32 [N, n_classes]: the rows of the clips `items_dev` (device int64 [N], validated by the caller) -- one launch.
        mix: None, or the batch's two augmentation tables on the device (m3t.audio.plan_aug's, validated by the caller): a row with a
        partner is lam32 * row + om32 * the partner item's row (m3t_label_rows_mix)."""
        if self.label_table is None:
            raise ValueError("WaveStore: built without labels")
        out = torch.empty(N, self.n_classes, dtype=torch.float32, device=self.device)
        if mix is None:
            _lib.check(lib().m3t_label_rows(self.label_table.data_ptr(), len(self.files), self.n_classes, items_dev.data_ptr(), N,
                                          out.data_ptr(), _stream()), "m3t_label_rows")
        else:
            _lib.check(lib().m3t_label_rows_mix(self.label_table.data_ptr(), len(self.files), self.n_classes, items_dev.data_ptr(), N,
                                              mix[0].data_ptr(), mix[1].data_ptr(), out.data_ptr(), _stream()), "m3t_label_rows_mix")
        return out

    def batch(self, items, draws=None, window=32, pad_mode="constant", mix=None):
        """{'audio': float32 [N, window, 200], 'label': float32 [N, n_classes]} of the clips `items` with `draws` (None: the evaluation
        draws), queued on the current stream.  Host validation, ONE table upload, the label launch, the ingest's launches.
        Draws that carry masks (m3t.audio.draw_spec_augment) and mix = (partner, lam) augment the batch inside those same launches
        (m3t.audio.ingest); the labels of a mixed batch are mixed with the same weights.  Without either nothing changes."""
        if pad_mode not in ("constant", "reflect"):
            raise ValueError("pad_mode must be 'constant' or 'reflect'")
        items, table, R = self.plan(items, draws, window)
        tables = _audio.plan_aug(draws, table, mix)
        N = int(items.shape[0])
        if tables is None:
            tab = torch.from_numpy(np.concatenate([table.reshape(-1), items])).to(self.device, non_blocking=True)
            out = {"audio": _audio.ingest_planned(self.wave, tab[:8 * N], N, R, window, pad_mode)}
            if self.label_table is not None:
                out["label"] = self.label_rows(tab[8 * N:], N)
            return out
        flat, split = _audio.pack_tables(table, tables, items)
        tab, aug_tab, items_dev = split(torch.from_numpy(flat).to(self.device, non_blocking=True))
        out = {"audio": _audio.ingest_planned(self.wave, tab, N, R, window, pad_mode, aug_tab=aug_tab)}
        if self.label_table is not None:
            out["label"] = self.label_rows(items_dev, N, aug_tab if mix is not None else None)
        return out


# ---- the epoch plan -------------------------------------------------------------------------------------------------------------------
class BatchPlan:
    """One batch of an epoch.  items: the clips' indices into the scan's files, as the sampler gave them; aug: one m3t.audio.draw_audioset
    dict per item; index: the batch's position in the epoch; mix: None, or the batch's mixup draws (partner [N] ints, lam [N] floats:
    positions in the batch and the float64 weights as drawn)."""
    __slots__ = ("items", "aug", "index", "mix")

    def __init__(self, items, aug, index, mix=None):
        self.items, self.aug, self.index, self.mix = items, aug, index, mix

    def __eq__(self, other):
        return (isinstance(other, BatchPlan) and self.items == other.items and self.index == other.index and self.aug == other.aug
                and self.mix == other.mix)

    def __repr__(self):
        return "BatchPlan(index=%d, items=%r, aug=%r%s)" % (self.index, self.items, self.aug, "" if self.mix is None else ", mix=%r" % (self.mix,))


class _Draws(Dataset):
    """the data set the plan's DataLoader reads: item i is (i, draw), drawn when it is read; spec_aug: m3t.audio.draw_audioset's (the mask
    draws of a training item, after its own), names: the clips' files, for a refusal"""

    def __init__(self, lengths, window, training, spec_aug=None, names=None):
        self.lengths, self.window, self.training, self.spec_aug, self.names = lengths, window, training, spec_aug, names

    def __len__(self):
        return len(self.lengths)

    def __getitem__(self, i):
        if self.spec_aug is None:
            return int(i), _audio.draw_audioset(int(self.lengths[i]), self.window, self.training)
        return int(i), _audio.draw_audioset(int(self.lengths[i]), self.window, self.training, self.spec_aug,
                                            "clip %d" % i if self.names is None else str(self.names[i]))


class AudioSetFeed:
    """An epoch of AudioSet batches from a Scan (scan_audioset), as the reference's DataLoader over its AudioSetDataset gives them.

    window, batch_size, split: the reference's (`audioset_dataset.py:99`, `audioset_model.py:129-145`); split must be the scan's.  rank /
    world: world > 1 shards the indices with torch's DistributedSampler in both splits (the reference's default one: shuffled, seed 0,
    set_epoch(epoch)).  sampler: overrides the index order -- any iterable of indices, or a callable that makes one from the data set.
    pad_mode: the STFT's padding, m3t.audio's ('constant' is librosa >= 0.10's).  convert: the scan's (scan_audioset(..., convert=True));
    given here it must agree with it, since the planned lengths are the scan's.  spec_augment: None, True (the reference's defaults) or a
    dict of F, T, n_freq, n_time (defaults 20, 20, 1, 1; at most 4 masks of a kind); mixup_alpha: 0.0 or the Beta distribution's
    parameter.  Both are ignored for the val split.

    Construction reads the clips' headers (Scan.lengths) and touches no device.  plan_epoch(epoch) is host only.  Iterating builds the
    WaveStore on the current device at the first batch and yields, per BatchPlan, WaveStore.batch(items, draws): validated for the whole
    batch before its first launch, queued on the current stream, nothing read back."""

    def __init__(self, scan, window, batch_size, split, rank=0, world=1, sampler=None, pad_mode="constant", convert=None,
                 spec_augment=None, mixup_alpha=0.0):
        if scan.split != split:
            raise ValueError("AudioSetFeed: split is %r, the folder was scanned for %r" % (split, scan.split))
        self.convert = bool(getattr(scan, "convert", False)) if convert is None else bool(convert)
        if self.convert != bool(getattr(scan, "convert", False)):
            raise ValueError("AudioSetFeed: convert=%r, the folder was scanned with convert=%r" % (self.convert, bool(getattr(scan, "convert", False))))
        self.scan, self.window, self.batch_size, self.split = scan, int(window), int(batch_size), split
        self.rank, self.world, self.pad_mode = int(rank), int(world), pad_mode
        if self.batch_size <= 0 or self.window <= 0:
            raise ValueError("AudioSetFeed: batch_size and window must be positive")
        if self.world <= 0 or not 0 <= self.rank < self.world:
            raise ValueError("AudioSetFeed: rank %d outside a world of %d" % (self.rank, self.world))
        if pad_mode not in ("constant", "reflect"):
            raise ValueError("pad_mode must be 'constant' or 'reflect'")
        if len(scan) == 0:
            raise ValueError("AudioSetFeed: the scan of %s found no clip of split %r" % (scan.path, split))
        self.training = split == "train"
        self.files = list(scan.files)
        self.lengths = scan.lengths()
        # training-time augmentation: the validation split never draws or applies either
        self.spec_augment, self.mixup_alpha = None, 0.0
        if self.training and spec_augment is not None and spec_augment is not False:
            given = {} if spec_augment is True else dict(spec_augment)
            if set(given) - {"F", "T", "n_freq", "n_time"}:
                raise ValueError("AudioSetFeed: spec_augment takes F, T, n_freq, n_time, got %r" % (sorted(given),))
            sa = {"F": 20, "T": 20, "n_freq": 1, "n_time": 1}
            sa.update(given)
            if not (0 <= int(sa["n_freq"]) <= _audio.MAX_MASKS and 0 <= int(sa["n_time"]) <= _audio.MAX_MASKS) or sa["F"] < 0 or sa["T"] < 0:
                raise ValueError("AudioSetFeed: spec_augment needs F, T >= 0 and 0 .. %d masks of each kind, got %r" % (_audio.MAX_MASKS, sa))
            self.spec_augment = sa
        if self.training and mixup_alpha:
            if not float(mixup_alpha) > 0.0:
                raise ValueError("AudioSetFeed: mixup_alpha must be positive (0: no mixup), got %r" % (mixup_alpha,))
            self.mixup_alpha = float(mixup_alpha)
        self._draws = _Draws(self.lengths, self.window, self.training, self.spec_augment, self.files)
        self._sampler = sampler(self._draws) if callable(sampler) else sampler
        self._dist = None
        if self._sampler is None and self.world > 1:
            self._sampler = self._dist = DistributedSampler(self._draws, num_replicas=self.world, rank=self.rank)
        self._loader = DataLoader(self._draws, batch_size=self.batch_size, shuffle=self.training and self._sampler is None,
                                  sampler=self._sampler, num_workers=0, collate_fn=list)
        self.epoch = 0
        self.store = None

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
            mix = None
            if self.mixup_alpha:                # right after the items' draws: the weights, then the partners
                lam = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=len(rows))
                mix = (np.random.permutation(len(rows)).tolist(), lam.tolist())
            yield BatchPlan([i for i, _ in rows], [d for _, d in rows], b, mix)

    def plan_epoch(self, epoch=None):
        """-> [BatchPlan] of one epoch (default: the current one); host only, no device is touched.  Consumes the epoch's random numbers."""
        return list(self.plans(epoch))

    def state_dict(self):
        """what a resume between two epochs needs: the epoch and the states of `random`, `np.random` and torch's default generator"""
        kind, keys, pos, has_gauss, gauss = np.random.get_state()
        return {"epoch": self.epoch, "random": random.getstate(),
                "numpy": (kind, np.array(keys, copy=True), int(pos), int(has_gauss), float(gauss)), "torch": torch.get_rng_state().clone()}

    def load_state_dict(self, state):
        self.epoch = int(state["epoch"])
        random.setstate(state["random"])
        np.random.set_state(tuple(state["numpy"]))
        torch.set_rng_state(state["torch"])

    # ---- device ----
    def build_store(self):
        """the WaveStore of the scan on the current device (once)"""
        if self.store is None:
            self.store = WaveStore(self.files, self.scan.labels, self.lengths, convert=self.convert)
        return self

    def batch(self, plan):
        """one BatchPlan -> the batch dict, queued on the current stream"""
        self.build_store()
        return self.store.batch(plan.items, plan.aug, self.window, self.pad_mode, mix=plan.mix)

    def __iter__(self):
        self.build_store()
        for plan in self.plans():
            yield self.batch(plan)


def feed_from_hparams(hparams, split, rank=0, world=1):
    """the feed of one split with the reference's arguments (`audioset_model.py:129-145`): dataset_path, window, batch_size; convert_audio
    (pretrain_audioset.py --convert_audio), when the namespace has it, is the scan's `convert`; so are the augmentation flags of the driver:
    spec_augment with freq_mask_para / time_mask_para / freq_mask_num / time_mask_num, and mixup_alpha (the train split only)"""
    scan = scan_audioset(hparams.dataset_path, split, convert=bool(getattr(hparams, "convert_audio", False)))
    spec_aug = None
    if getattr(hparams, "spec_augment", False):
        flags = (("F", "freq_mask_para"), ("T", "time_mask_para"), ("n_freq", "freq_mask_num"), ("n_time", "time_mask_num"))
        spec_aug = {k: getattr(hparams, flag) for k, flag in flags if hasattr(hparams, flag)}
    alpha = float(getattr(hparams, "mixup_alpha", 0.0) or 0.0)
    return AudioSetFeed(scan, hparams.window, hparams.batch_size, split, rank, world, spec_augment=spec_aug, mixup_alpha=alpha)
