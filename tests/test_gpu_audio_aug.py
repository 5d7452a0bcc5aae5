"""The augmented AudioSet ingest on the GPU (m3t_audio_db_stack_aug, m3t_label_rows_mix; m3t.audio.ingest / m3t.audioset with masks and
mix) against the numpy oracle of tests/audio_aug_ref.py.

Bound: bit-equality.  The oracle is applied to m3t.audio.ingest's OWN un-augmented output for the same clips and draws, so the spectrogram
(unpinned, held to 2e-3 dB elsewhere) cancels: what is left is a choice per cell (the value or exactly 0.0) and, when mixing, two rounded
float32 products and one rounded float32 sum, which numpy's float32 arithmetic restates exactly.  Labels likewise.

Shapes: N in {1, 2, 3, 5} clips x window in {1, 2, 7, 32} frames; every case rotates the sample type (int16 / float32) and the form (a list,
or one flat buffer with offsets).  Per batch: clips at 30 and 15 fps next to each other (at both, frame 3T + 1 -- the last the stack asks
for -- is == nf and comes out 0.0), clip 1 shorter than its crop (the wrap), clip 2 cut short by two hops (nf smaller: zero padding inside the
stack), clip 4 three hops longer (a mask that reaches frames the stack never reads)."""
import argparse

import numpy as np
import pytest
import torch

import audio_aug_ref as G
import audio_ingest_ref as A
import audioset_feed_ref as F

pytestmark = pytest.mark.gpu
NS, WINDOWS = (1, 2, 3, 5), (1, 2, 7, 32)
PARTNERS = {1: [0], 2: [1, 0], 3: [0, 2, 1], 5: [0, 2, 1, 4, 3]}               # clip 0 is its own partner; 1 <-> 2 and 3 <-> 4 pair 15 with 30 fps
LAMS = [1.0, 0.0, 0.5, 0.3, 0.7321]                                             # exactly 1, exactly 0, 0.5, and two that round


def _bits(t):
    return (t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)).tobytes()


def make_batch(N, T):
    """-> (clips float32, plain draws, masked draws, taus)"""
    clips, plain, masked, taus = [], [], [], []
    for n in range(N):
        fps = 15.0 if n % 2 else 30.0
        d = A.draw(fps, 0, T)
        if n == 2:
            d["nsamples"] -= 2 * d["hop"]
        if n == 4:
            d["nsamples"] += 3 * d["hop"]
        ns = d["nsamples"]
        length = ns // 2 + 3 if n == 1 else ns + 500 * n + 7
        d["start"] = 4 if n == 1 else (length - ns) // 2                 # clip 1: the crop runs over the clip's end more than once
        tau = 1 + ns // d["hop"]
        clips.append(A.signal(length, 40 + n))
        plain.append(d)
        taus.append(tau)
        m = dict(d)
        if n == 0:
            m["fmask"], m["tmask"] = [(33, 7)], [(tau - min(3, tau), min(3, tau))]                     # f0 + f == 40, t0 + t == tau
        elif n == 1:
            m["fmask"], m["tmask"] = [(5, 0)], [(min(2, tau), 0)]                                         # f == 0 and t == 0: nothing masked
        elif n == 2:
            m["fmask"], m["tmask"] = [], [(0, tau)]                                                       # every stacked frame
        elif n == 3:
            m["fmask"] = [(0, 5), (3, 6), (8, 1), (30, 10)]                                               # four of each, overlapping
            m["tmask"] = [(0, min(2, tau)), (min(1, tau), min(2, tau - min(1, tau))), (tau // 2, 1), (tau - 1, 1)]
        else:
            m["tmask"] = [(3 * T, tau - 3 * T)]                                                           # frames 3T .. : only 3T and 3T + 1 are read
        masked.append(m)
    return clips, plain, masked, taus


def run(clips, draws, T, case, mix=None):
    """m3t.audio.ingest in the case's sample type and form"""
    from m3t import audio
    as_i16 = case % 2 == 1
    cl = [np.clip(np.round(c.astype(np.float64) * 32767.0), -32768, 32767).astype(np.int16) if as_i16 else c for c in clips]
    if (case // 2) % 2 == 0:
        return audio.ingest(cl, draws, T, mix=mix)
    order = list(reversed(range(len(cl))))                                       # the store form: another order, a gap in front of every clip
    flat, offs = [], {}
    for i in order:
        flat.append(np.full(3, 9, cl[0].dtype))
        offs[i] = sum(len(x) for x in flat)
        flat.append(cl[i])
    buf = torch.from_numpy(np.concatenate(flat)).cuda()
    return audio.ingest(buf, draws, T, lengths=[len(c) for c in cl], offsets=[offs[i] for i in range(len(cl))], mix=mix)


@pytest.mark.parametrize("T", WINDOWS)
@pytest.mark.parametrize("N", NS)
def test_masks_and_mix_equal_the_oracle_bit_for_bit(N, T):
    case = NS.index(N) + WINDOWS.index(T)
    clips, plain, masked, taus = make_batch(N, T)
    assert all(tau == 3 * T + 1 for n, tau in enumerate(taus) if n not in (2, 4)) and (N < 3 or taus[2] == 3 * T - 1) and (N < 5 or taus[4] == 3 * T + 4)
    mix = (PARTNERS[N], LAMS[:N])
    base = run(clips, plain, T, case).cpu().numpy()
    assert base.shape == (N, T, 200) and np.isfinite(base).all() and (base[0, :, :160] != 0).all()
    assert (base[0, T - 1, 160:] == 0).all()                                     # frame 3T + 1 == nf: the stack's zero padding
    # masks alone: the oracle, and where nothing is masked the un-augmented kernel's own bits
    got = run(clips, masked, T, case)
    want = G.augment(base, masked)
    assert got.dtype == torch.float32 and tuple(got.shape) == (N, T, 200) and _bits(got) == want.tobytes()
    g = got.cpu().numpy()
    for n, m in enumerate(masked):
        z = G.mask_rows(np.ones((T, 200), np.float32), m) == 0
        assert (g[n][z] == 0).all() and not np.signbit(g[n][z]).any() and g[n][~z].tobytes() == base[n][~z].tobytes()
        assert z.any() == (n != 1)
    if N >= 3:
        assert (g[2] == 0).all() and _bits(g[1]) == _bits(base[1])               # every frame masked; f = t = 0 masks nothing
    # masks and mix; mix alone
    got = run(clips, masked, T, case, mix)
    assert _bits(got) == G.augment(base, masked, mix).tobytes()
    assert _bits(got[0]) == _bits(G.mask_rows(base[0], masked[0]) + np.float32(0))          # lam exactly 1 on itself
    alone = run(clips, plain, T, case, mix)
    assert _bits(alone) == G.augment(base, plain, mix).tobytes()
    if N >= 2:
        assert _bits(alone[1]) == _bits(np.float32(0) * base[1] + base[PARTNERS[N][1]])      # lam exactly 0: the partner's rows
    # a rerun gives the same bits
    assert torch.equal(run(clips, masked, T, case, mix), got)


def test_a_nan_or_inf_cell_under_a_mask_becomes_zero():
    """the zero is an assignment: the launch on a hand-made spectrogram that holds NaN and inf"""
    from m3t import _lib, audio
    T, nf = 2, 7
    mel = torch.full((nf, 40), 1e-3, device="cuda")
    mel[2, 5], mel[3, 6], mel[4, 7] = float("nan"), float("inf"), float("inf")
    table = np.array([[0, 1, 0, 1, 1, nf, 0, 0]], np.int64)
    ints, w = audio.plan_aug([dict(fmask=[(5, 2)], tmask=[])], table)
    flat, split = audio.pack_tables(table, (ints, w))
    tab, (ai, af), _ = split(torch.from_numpy(flat).cuda())
    out = torch.empty(1, T, 200, device="cuda")
    rc = _lib.load().m3t_audio_db_stack_aug(mel.data_ptr(), nf, tab.data_ptr(), 1, ai.data_ptr(), af.data_ptr(), T, 40, 3, 5, 1e-10, -1.0,
                                            out.data_ptr(), torch.cuda.current_stream().cuda_stream)            # (top_db < 0: no floor, an inf stays one cell)
    assert rc == 0
    o = out.cpu().numpy().reshape(T, 5, 40)
    assert (o[:, :, 5:7] == 0).all() and np.isinf(o[1, 1, 7]) and np.isfinite(np.delete(o, 7, axis=2)).all()
    assert abs(o[0, 0, 0] + 30.0) < 1e-3
    L = _lib.load()
    args = lambda **kw: [kw.get("mel", mel.data_ptr()), nf, kw.get("tab", tab.data_ptr()), kw.get("N", 1), kw.get("ai", ai.data_ptr()),
                         kw.get("af", af.data_ptr()), kw.get("T", T), 40, 3, 5, kw.get("amin", 1e-10), 80.0, out.data_ptr(), None]
    assert L.m3t_audio_db_stack_aug(*args(N=0)) == 0 and L.m3t_audio_db_stack_aug(*args(T=0)) == 0
    for bad in (dict(mel=None), dict(ai=None), dict(af=None), dict(N=-1), dict(amin=0.0), dict(ai=ai.data_ptr() + 2), dict(tab=tab.data_ptr() + 4)):
        assert L.m3t_audio_db_stack_aug(*args(**bad)) == _lib.M3T_EINVAL, bad


def test_a_partner_outside_the_batch_is_a_zero_clip_on_the_device():
    """the host refuses it first (tests/test_audio_aug_host.py); the raw tables are checked here: no clip outside the table is read"""
    from m3t import audio
    clips, plain, masked, _ = make_batch(3, 2)
    wave, table, R = audio.plan_waves(clips, masked, 2)
    ints, w = audio.plan_aug(masked, table, ([0, 2, 1], [0.5, 0.5, 0.5]))
    good = audio.ingest(clips, masked, 2, mix=([0, 2, 1], [0.5, 0.5, 0.5]))
    for bad in (3, -2, 2 ** 31 - 1):
        broken = ints.copy()
        broken[1, 2] = bad
        flat, split = audio.pack_tables(table, (broken, w))
        tab, aug_tab, _ = split(torch.from_numpy(flat).cuda())
        got = audio.ingest_planned(wave.cuda(), tab, 3, R, 2, aug_tab=aug_tab)
        assert bool((got[1] == 0).all()) and torch.equal(got[0], good[0]) and torch.equal(got[2], good[2])
    with pytest.raises(ValueError, match="augmentation needs device tables"):
        audio.ingest_planned(wave.cuda(), tab, 3, R, 2, aug_tab=(aug_tab[0][:-1], aug_tab[1]))


# ---------------------------------------------------------------------------------------------- the labels
@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return F.write_tree(tmp_path_factory.mktemp("audioset"))


@pytest.mark.parametrize("C", [5, 527])
def test_label_rows_mix_against_numpy(tree, C):
    from m3t import _lib, audio, audioset
    scan = audioset.scan_audioset(tree, "train")
    if C == 5:                  # class 0 in every clip, 1 in clips 0 and 3, 2 in clip 1 only, 3 in clip 4 only, 4 in none
        labels = np.array([[1, 1, 0, 0, 0], [1, 0, 1, 0, 0], [1, 0, 0, 0, 0], [1, 1, 0, 0, 0], [1, 0, 0, 1, 0]], np.uint8)
    else:
        labels = scan.labels
    store = audioset.WaveStore(scan.files, labels)
    items = [3, 0, 4, 1, 3]                                                      # a repeat; 3 and 0 share class 1 when C == 5
    partner, lam = [1, 0, 2, 4, 3], [0.25, 1.0, 0.5, 0.0, 0.7321]
    draws = [audio.draw_audioset(int(store.lengths[i]), 4, False) for i in items]
    want = G.mix_labels(labels[items], partner, lam)
    got = store.batch(items, draws, 4, mix=(partner, lam))["label"]
    assert got.dtype == torch.float32 and tuple(got.shape) == (5, C) and _bits(got) == want.tobytes()
    if C == 5:
        assert want[0].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0] and want[2].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0]       # in both; a clip with itself
        assert want[3, 2] == 0.0 and want[3, 1] == 1.0 and want[4, 2] == np.float32(1) - np.float32(0.7321) and (want[:, 4] == 0).all()
    else:
        assert want[0, 526] == 0.25 and want[0, 0] == 0.75 and set(np.unique(want[0]).tolist()) == {0.0, 0.25, 0.75}
    # masks without a mix: the labels are the plain rows, by the plain launch
    masked = [dict(d, fmask=[(1, 2)]) for d in draws]
    assert _bits(store.batch(items, masked, 4)["label"]) == labels[items].astype(np.float32).tobytes()
    # the raw entry point: a row without a partner is the copy; a partner or an item outside its table leaves the row untouched
    L = _lib.load()
    table = np.zeros((5, 8), np.int64)
    table[:, 5] = 13
    ints, w = audio.plan_aug(draws, table, (partner, lam))
    ints[0, 2], ints[1, 2], ints[2, 2] = -1, 5, -2
    it = torch.tensor([3, 0, 4, 7, 3], dtype=torch.int64, device="cuda")        # item 7 is outside the table; row 4's partner is row 3
    ai, af = torch.from_numpy(ints.reshape(-1)).cuda(), torch.from_numpy(w.reshape(-1)).cuda()
    out = torch.full((5, C), 7.0, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert L.m3t_label_rows_mix(store.label_table.data_ptr(), 5, C, it.data_ptr(), 5, ai.data_ptr(), af.data_ptr(), out.data_ptr(), st) == 0
    assert _bits(out[0]) == labels[3].astype(np.float32).tobytes() and bool((out[1:] == 7.0).all())
    assert L.m3t_label_rows_mix(store.label_table.data_ptr(), 5, C, it.data_ptr(), 0, ai.data_ptr(), af.data_ptr(), out.data_ptr(), None) == 0
    for bad in ((None, 5, C, it.data_ptr(), 5, ai.data_ptr(), af.data_ptr()), (store.label_table.data_ptr(), 5, 0, it.data_ptr(), 5, ai.data_ptr(), af.data_ptr()),
                (store.label_table.data_ptr(), 5, C, it.data_ptr(), 5, None, af.data_ptr()), (store.label_table.data_ptr(), 5, C, it.data_ptr(), 5, ai.data_ptr(), None),
                (store.label_table.data_ptr(), 5, C, it.data_ptr() + 4, 4, ai.data_ptr(), af.data_ptr()),
                (store.label_table.data_ptr(), 5, C, it.data_ptr(), 5, ai.data_ptr() + 2, af.data_ptr())):
        assert L.m3t_label_rows_mix(*bad, out.data_ptr(), None) == _lib.M3T_EINVAL, bad


# ---------------------------------------------------------------------------------------------- the feed and the task module
SA = {"F": 20, "T": 8, "n_freq": 2, "n_time": 1}


def _oracle_batch(feed, plan, clips):
    """the oracle's batch of a plan: the un-augmented ingest of the same clips and draws, masked and mixed in numpy; labels likewise"""
    from m3t import audio
    plain = [{k: d[k] for k in ("fps", "hop", "start", "nsamples")} for d in plan.aug]
    base = audio.ingest([clips[i] for i in plan.items], plain, feed.window).cpu().numpy()
    rows = feed.scan.labels[plan.items]
    return G.augment(base, plan.aug, plan.mix), (rows.astype(np.float32) if plan.mix is None else G.mix_labels(rows, *plan.mix))


def test_an_augmented_epoch_of_the_feed_equals_the_oracle_and_queues_without_a_sync(tree):
    c = F.config("train")
    clips = [F.clip(str(f)) for f in F.golden()["train.files"]]
    feed = F.make_feed(tree, c, spec_augment=SA, mixup_alpha=0.4)
    plans = feed.plan_epoch(0)
    assert [len(p.items) for p in plans] == [2, 2, 1] and all(p.mix is not None and "fmask" in p.aug[0] for p in plans)
    want = [_oracle_batch(feed, p, clips) for p in plans]
    for p in plans:                                                              # warm-up: the store is built, constants are uploaded
        feed.batch(p)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = [feed.batch(p) for p in plans]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for b, (batch, (audio_ref, label_ref)) in enumerate(zip(got, want)):
        assert sorted(batch) == ["audio", "label"] and _bits(batch["audio"]) == audio_ref.tobytes() and _bits(batch["label"]) == label_ref.tobytes(), b
    # the val feed with the same options: the plain feed's batches, bit for bit
    cv = F.config("val")
    plain, opted = F.make_feed(tree, cv), F.make_feed(tree, cv, spec_augment=SA, mixup_alpha=0.4)
    for x, y in zip(plain, opted):
        assert torch.equal(x["audio"], y["audio"]) and torch.equal(x["label"], y["label"])


def test_training_step_on_a_mixed_batch_has_the_loss_of_the_oracle_s_batch(tree):
    """(eval mode: the head's dropout draws its mask per call, so two train-mode calls never share one)"""
    from m3t import audioset, ops
    from models.audioset_model import AudioSet
    ns = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    ns.dataset_path, ns.window, ns.batch_size, ns.checkpoint_path = tree, 4, 2, None
    torch.manual_seed(6)
    model = AudioSet(ns).cuda().eval()
    c = F.config("train")
    clips = [F.clip(str(f)) for f in F.golden()["train.files"]]
    feed = F.make_feed(tree, c, spec_augment=SA, mixup_alpha=0.4)
    drawn = feed.plan_epoch(0)[0]
    plan = audioset.BatchPlan(drawn.items, drawn.aug, 0, ([1, 0], [0.3, 0.6]))    # the drawn batch, each clip mixed with the other
    audio_ref, label_ref = _oracle_batch(feed, plan, clips)
    assert len(set(plan.items)) == 2 and ((label_ref > 0) & (label_ref < 1)).any()
    out = model.training_step(feed.batch(plan), 0)
    x, y = torch.from_numpy(audio_ref).cuda(), torch.from_numpy(label_ref).cuda()
    want = ops.cls_loss(ops.temporal_pool(model.audio(x), 'max'), y, 'bce')[0]
    assert bool(torch.isfinite(out["loss"])) and _bits(out["loss"]) == _bits(want)
    out["loss"].backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    # a PCM batch with the mix beside it takes the same route through the module
    pcm = [clips[i] for i in plan.items]
    S = max(len(p) for p in pcm)
    packed = np.zeros((len(pcm), S), np.int16)
    for n, p in enumerate(pcm):
        packed[n, :len(p)] = p
    batch = {"audio": torch.from_numpy(packed), "audio_aug": plan.aug, "audio_len": [len(p) for p in pcm], "audio_mix": plan.mix, "label": y}
    assert _bits(model.training_step(batch, 1)["loss"]) == _bits(want)
