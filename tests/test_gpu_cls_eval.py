"""The multi-label evaluation epoch on the GPU (csrc/cls_eval.hip, m3t/cls_evaluate.py) against the exact oracle of tests/cls_eval_ref.py.

Bars, all derived (none measured):
  AUC per class      bit-equal to Python's num / (2 P N) of the oracle's integer numerator: both are one correctly rounded division of
                     exactly representable integers
  AP per class       within (P + 2) 2^-52 absolute of the exact rational: twice the worst-case bound of a float64 sum of at most P
                     correctly rounded terms in any order
  val_map / val_auc  within the largest per-class bar plus (C + 1) 2^-53
  P, N, counts       exact;  val_loss / val_acc: Trainer.validate's bits;  two runs: the same bits everywhere

Inputs have fixed seeds and, wherever the case is not about the exclusion rule, at least one positive and one negative per class
(asserted), so that the rule cannot hide a failure.  M = 1 cannot have both: it is checked as the one-row case of that rule."""
import argparse
import math
import os
import wave

import numpy as np
import pytest
import torch

import cls_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _data(M, C, seed, rate=0.3, levels=None, both=True):
    rs = np.random.RandomState(seed)
    s = rs.standard_normal((M, C)).astype(np.float32)
    if levels:
        s = (np.floor(rs.uniform(size=(M, C)) * levels) / levels - 0.5).astype(np.float32)
    y = (rs.uniform(size=(M, C)) < rate).astype(np.float32)
    if both and M >= 2:
        for c in range(C):
            a, b = rs.choice(M, 2, replace=False)
            y[a, c], y[b, c] = 1.0, 0.0
        assert (y.sum(0) >= 1).all() and (y.sum(0) <= M - 1).all()
    return s, y


def _run(s, y, lds_rows=None, batch=128, items=None, seed=0):
    """one epoch through ClsEvaluator in batches of `batch` rows at the item rows `items` (default: a fixed permutation)"""
    from m3t.cls_evaluate import ClsEvaluator
    M, C = s.shape
    rs = np.random.RandomState(1000 + seed)
    items = rs.permutation(M) if items is None else np.asarray(items)
    ev = ClsEvaluator(M, C, lds_rows=lds_rows)
    ts, ty = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    for k, a in enumerate(range(0, M, batch)):
        rows = items[a:a + batch]
        idx = torch.from_numpy(rows.astype(np.int64)).to(DEV)
        hits = torch.from_numpy((rs.uniform(size=rows.size) < 0.5).astype(np.float32)).to(DEV)
        ev.add(ts[idx], ty[idx], rows.tolist(), torch.tensor(0.25 + k, device=DEV), hits)
    return ev.finish()


def _check(res, s, y):
    """every figure of a result against the oracle, at the module's bars -> the oracle's epoch dict"""
    e = R.epoch(s, y)
    pc, m = res.per_class, res.metrics
    assert pc["P"].tolist() == e["P"].tolist() and pc["N"].tolist() == e["N"].tolist()
    assert m["n_classes_ap"] == e["n_classes_ap"] and m["n_classes_auc"] == e["n_classes_auc"]
    assert m["n_nonfinite"] == 0 and m["n_bad_labels"] == 0
    for c in range(s.shape[1]):
        if math.isnan(e["auc"][c]):
            assert math.isnan(pc["auc"][c]), c
        else:
            assert pc["auc"][c] == e["auc"][c], (c, pc["auc"][c], e["auc"][c])                 # bit for bit
        if e["ap_exact"][c] is None:
            assert math.isnan(pc["ap"][c]), c
        else:
            assert abs(R.Fraction(float(pc["ap"][c])) - e["ap_exact"][c]) <= R.Fraction(e["bar_ap"][c]), (c, pc["ap"][c], e["ap"][c])
    for key in ("val_map", "val_auc"):
        if math.isnan(e[key]):
            assert math.isnan(m[key]), key
        else:
            assert abs(m[key] - e[key]) <= e["bar_mean"], (key, m[key], e[key])
    d = R.dprime(m["val_auc"])
    assert (math.isnan(d) and math.isnan(m["val_dprime"])) or m["val_dprime"] == d
    return e


def _same_bits(a, b):
    for k in ("ap", "auc", "P", "N"):
        assert a.per_class[k].tobytes() == b.per_class[k].tobytes(), k
    assert repr(a.metrics) == repr(b.metrics)                                                   # (repr: NaN equals NaN, -0.0 differs from 0.0)


def _forced(M):
    """an lds_rows below M: the chunked path with several chunks"""
    return 16 if M > 16 else 1


# ---------------------------------------------------------------------------------------------- rank: sizes, both paths
@pytest.mark.parametrize("path", ["lds", "chunked"])
@pytest.mark.parametrize("M", [1, 2, 3, 63, 64, 65, 257, 1000])
def test_rank_sizes(M, path):
    for C in (1, 3, 5):
        s, y = _data(M, C, 10 * M + C)
        if M == 1:
            y[:] = 1.0                                        # one row: a positive and no negative -- AP 1, not scored for AUC
        res = _run(s, y, lds_rows=None if path == "lds" else _forced(M), batch=100)
        e = _check(res, s, y)
        if M == 1:
            assert res.per_class["ap"].tolist() == [1.0] * C and e["n_classes_auc"] == 0
        else:
            assert e["n_classes_ap"] == C and e["n_classes_auc"] == C


@pytest.mark.parametrize("dM", [-1, 0, 1])
def test_rank_at_the_true_lds_capacity(dM):
    from m3t import cls_evaluate as E
    M = E.LDS_ROWS + dM                                       # capacity + 1 is the first column that takes the chunked path by itself
    s, y = _data(M, 2, 77 + dM, rate=0.002)
    assert 1 <= y.sum(0).min() and y.sum(0).max() <= 80
    e = _check(_run(s, y, batch=4096), s, y)
    assert e["n_classes_auc"] == 2


def test_rank_full_class_count_and_two_runs():
    s, y = _data(300, 527, 5, rate=0.1)
    a = _run(s, y)
    e = _check(a, s, y)
    assert e["n_classes_ap"] == 527 and e["n_classes_auc"] == 527
    _same_bits(a, _run(s, y))
    _same_bits(_run(s, y, lds_rows=64), _run(s, y, lds_rows=64))


# ---------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("levels", [4, 8])
@pytest.mark.parametrize("lds_rows", [None, 32])
def test_quantised_scores(levels, lds_rows):
    s, y = _data(257, 3, levels, levels=levels)
    assert len(np.unique(s[:, 0])) == levels
    _check(_run(s, y, lds_rows=lds_rows), s, y)


@pytest.mark.parametrize("lds_rows", [None, 16])
def test_all_scores_equal(lds_rows):
    s, y = _data(64, 3, 3)
    s[:] = 0.375
    res = _run(s, y, lds_rows=lds_rows)
    _check(res, s, y)
    for c in range(3):
        P = int(y[:, c].sum())
        assert res.per_class["auc"][c] == 0.5
        assert abs(R.Fraction(float(res.per_class["ap"][c])) - R.Fraction(P, 64)) <= R.Fraction(R.ap_bar(P))


def test_both_zeros_tie_and_denormals_do_not():
    z = np.array([[-0.0], [0.0]], np.float32)
    res = _run(z, np.array([[1.0], [0.0]], np.float32))
    assert res.per_class["auc"][0] == 0.5 and res.per_class["ap"][0] == 0.5               # one group of two
    d = np.array([[1e-40], [2e-40]], np.float32)
    assert d[0, 0] != d[1, 0] and d[0, 0] != 0
    lo = _run(d, np.array([[1.0], [0.0]], np.float32))                                    # the positive ranks below: AUC 0
    hi = _run(d, np.array([[0.0], [1.0]], np.float32))
    assert lo.per_class["auc"][0] == 0.0 and lo.per_class["ap"][0] == 0.5 and hi.per_class["auc"][0] == 1.0 and hi.per_class["ap"][0] == 1.0
    # a longer column with both zeros, negative denormals and their neighbours, against the oracle, on both paths
    rs = np.random.RandomState(9)
    pool = np.array([-0.0, 0.0, 1e-40, 2e-40, -1e-40, 1.0, -1.0, 1.1754944e-38], np.float32)
    s = pool[rs.randint(0, pool.size, (200, 3))]
    _, y = _data(200, 3, 12)
    for lds_rows in (None, 16):
        _check(_run(s, y, lds_rows=lds_rows), s, y)


@pytest.mark.parametrize("lds_rows", [None, 64])
def test_tie_groups_across_the_chunks_of_a_workgroup(lds_rows):
    """2500 rows: a thread of the 1024 walks 3 rows, so runs of 37 equal scores begin and end inside and across the threads' chunks
    (and, on the chunked path, across the 64-row LDS chunks)"""
    M = 2500
    _, y = _data(M, 2, 21)
    s = np.stack([(np.arange(M) // 37).astype(np.float32), ((np.arange(M) + 11) // 5).astype(np.float32)], 1)
    rs = np.random.RandomState(4)
    s = s[rs.permutation(M)]
    _check(_run(s, y, lds_rows=lds_rows, batch=1000), s, y)


# ---------------------------------------------------------------------------------------------- the exclusion rule, d'
def test_classes_without_a_positive_or_a_negative():
    s, y = _data(65, 4, 31)
    y[:, 1] = 0.0                                             # no positive: in neither mean
    y[:, 2] = 1.0                                             # no negative: AP 1, not in the AUC mean
    res = _run(s, y)
    e = _check(res, s, y)
    pc = res.per_class
    assert math.isnan(pc["ap"][1]) and math.isnan(pc["auc"][1]) and (pc["P"][1], pc["N"][1]) == (0, 65)
    assert pc["ap"][2] == 1.0 and math.isnan(pc["auc"][2]) and (pc["P"][2], pc["N"][2]) == (65, 0)
    assert (res.metrics["n_classes_ap"], res.metrics["n_classes_auc"]) == (3, 2) == (e["n_classes_ap"], e["n_classes_auc"])


def test_no_class_scorable():
    s, y = _data(20, 3, 32)
    y[:] = 0.0
    m = _run(s, y).metrics
    assert math.isnan(m["val_map"]) and math.isnan(m["val_auc"]) and math.isnan(m["val_dprime"])
    assert (m["n_classes_ap"], m["n_classes_auc"]) == (0, 0) and m["val_loss"] == 0.25


def test_auc_exactly_zero_and_one():
    y = np.zeros((10, 2), np.float32)
    y[:4] = 1.0
    up = np.arange(10, 0, -1, dtype=np.float32)
    one = _run(np.stack([up, up + 3], 1), y)
    zero = _run(np.stack([-up, -up - 3], 1), y)
    assert one.metrics["val_auc"] == 1.0 and one.metrics["val_dprime"] == math.inf and one.metrics["val_map"] == 1.0
    assert zero.metrics["val_auc"] == 0.0 and zero.metrics["val_dprime"] == -math.inf
    _check(one, np.stack([up, up + 3], 1), y)
    _check(zero, np.stack([-up, -up - 3], 1), y)


# ---------------------------------------------------------------------------------------------- poisoning
@pytest.mark.parametrize("what", ["nan", "inf", "label"])
def test_one_bad_value_poisons_the_ranking_figures_only(what):
    s, y = _data(70, 5, 41)
    clean = _run(s, y, batch=32)
    s2, y2 = s.copy(), y.copy()
    if what == "label":
        y2[33, 2] = 0.5
    else:
        s2[33, 2] = np.nan if what == "nan" else np.inf
    m = _run(s2, y2, batch=32).metrics
    assert (m["n_nonfinite"], m["n_bad_labels"]) == ((0, 1) if what == "label" else (1, 0))
    assert math.isnan(m["val_map"]) and math.isnan(m["val_auc"]) and math.isnan(m["val_dprime"])
    assert m["val_loss"] == clean.metrics["val_loss"] and m["val_acc"] == clean.metrics["val_acc"]
    assert not math.isnan(clean.metrics["val_map"])


# ---------------------------------------------------------------------------------------------- append
@pytest.mark.parametrize("C", [5, 527])
@pytest.mark.parametrize("B", [1, 3, 128])
def test_append_equals_a_numpy_scatter(B, C):
    from m3t.cls_evaluate import ClsEvaluator
    M = 300
    rs = np.random.RandomState(B + C)
    s, y = _data(B, C, B * C, both=False)
    items = rs.choice(M, B, replace=False)                    # permuted, not consecutive
    ev = ClsEvaluator(M, C)
    ev.add(torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV), items.tolist(), torch.tensor(0.0, device=DEV), torch.zeros(B, device=DEV))
    cs, cl, seen = R.scatter(s, y, items, M)
    assert ev.scores.cpu().numpy().tobytes() == cs.tobytes()
    assert ev.labels.cpu().numpy().tobytes() == cl.tobytes() and ev.seen.cpu().numpy().tobytes() == seen.tobytes()
    assert ev.counters.tolist() == [0, 0]
    # a second batch that repeats an item with equal values (DistributedSampler's padding) and adds new ones
    if B >= 3:
        rest = np.setdiff1d(np.arange(M), items)[:2]
        it2 = np.concatenate([items[1:2], rest])
        s2, y2 = np.concatenate([s[1:2], s[:2] + 1]), np.concatenate([y[1:2], 1 - y[:2]])
        ev.absorb(torch.from_numpy(s2).to(DEV), torch.from_numpy(y2).to(DEV), it2.tolist())
        cs[:, it2], cl[:, it2], seen[it2] = s2.T, (y2.T == 1.0).astype(np.uint8), 1
        assert ev.scores.cpu().numpy().tobytes() == cs.tobytes() and ev.labels.cpu().numpy().tobytes() == cl.tobytes()
        assert ev.seen.cpu().numpy().tobytes() == seen.tobytes()


def test_evaluator_host_checks():
    from m3t import cls_evaluate as E
    with pytest.raises(ValueError, match="capacity"):
        E.ClsEvaluator(E.MAX_ROWS + 1, 3)
    s, y = _data(4, 3, 51)
    ts, ty = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    zero, hits = torch.tensor(0.0, device=DEV), torch.zeros(4, device=DEV)
    ev = E.ClsEvaluator(6, 3)
    for bad in ([0, 1, 2, 6], [0, -1, 2, 3]):
        with pytest.raises(ValueError, match="the split holds 6"):
            ev.add(ts, ty, bad, zero, hits)
    assert int(ev.seen.sum()) == 0 and not ev._loss           # refused before the launch
    ev.add(ts, ty, [0, 1, 2, 5], zero, hits)
    with pytest.raises(ValueError, match="2 of the 6 items were never appended"):
        ev.finish()


def test_add_does_not_synchronise():
    from m3t.cls_evaluate import ClsEvaluator
    s, y = _data(40, 527, 61)
    ts, ty = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    loss, hits = torch.tensor(0.5, device=DEV), torch.ones(8, device=DEV)
    warm = ClsEvaluator(40, 527)
    for a in range(0, 40, 8):                                 # library load, allocator warm-up
        warm.add(ts[a:a + 8], ty[a:a + 8], list(range(a, a + 8)), loss, hits)
    warm.finish()
    ev = ClsEvaluator(40, 527)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):                     # the detector works in this build
            torch.ones(1, device=DEV).item()
        for a in range(0, 40, 8):
            ev.add(ts[a:a + 8], ty[a:a + 8], list(range(a, a + 8)), loss, hits)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _check(ev.finish(), s, y)


# ---------------------------------------------------------------------------------------------- ranks
def test_two_ranks_merged_equal_one():
    """DistributedSampler's plans of a world of 2 over 7 items (rank 1 ends on a padded repeat of item 0): two evaluators, merged
    through shard() / absorb() as Trainer.evaluate_cls merges what all_gather returns, give the single-rank bits on both ranks"""
    from torch.utils.data.distributed import DistributedSampler
    from m3t.cls_evaluate import ClsEvaluator
    M, C = 7, 5
    s, y = _data(M, C, 71)
    ts, ty = torch.from_numpy(s).to(DEV), torch.from_numpy(y).to(DEV)
    plans = [list(DistributedSampler(range(M), num_replicas=2, rank=r, shuffle=False)) for r in (0, 1)]
    assert sorted(plans[0] + plans[1]) == [0, 0, 1, 2, 3, 4, 5, 6]

    def rank_eval(r):
        ev = ClsEvaluator(M, C)
        for a in (0, 2):
            rows = plans[r][a:a + 2]
            idx = torch.tensor(rows, device=DEV)
            ev.add(ts[idx], ty[idx], rows, torch.tensor(1.0 + a, device=DEV), torch.ones(2, device=DEV))
        return ev

    single = ClsEvaluator(M, C)
    single.add(ts, ty, list(range(M)), torch.tensor(1.0, device=DEV), torch.ones(M, device=DEV))
    want = single.finish()
    _check(want, s, y)
    for me in (0, 1):
        evs = [rank_eval(0), rank_eval(1)]
        with pytest.raises(ValueError, match="never appended"):
            rank_eval(me).finish()                            # a rank alone has not seen the split
        evs[me].absorb(*evs[1 - me].shard())
        got = evs[me].finish()
        for k in ("ap", "auc", "P", "N"):
            assert got.per_class[k].tobytes() == want.per_class[k].tobytes()
        for k in ("val_map", "val_auc", "val_dprime", "n_classes_ap", "n_classes_auc"):
            assert repr(got.metrics[k]) == repr(want.metrics[k])


# ---------------------------------------------------------------------------------------------- end to end
def _write_tree(root, n_clips=9, n_classes=527):
    rs = np.random.RandomState(81)
    os.makedirs(os.path.join(root, "eval_segments"))
    with open(os.path.join(root, "class_labels_indices.csv"), "w") as f:
        f.write("index,mid,display_name\n")
        for c in range(n_classes):
            f.write('%d,/m/%03d,"class %d"\n' % (c, c, c))
    with open(os.path.join(root, "eval_segments.csv"), "w") as f:
        f.write("# a\n# b\n# YTID, start_seconds, end_seconds, positive_labels\n")
        for i in range(n_clips):
            mids = ",".join("/m/%03d" % c for c in range(n_classes) if (c + i) % 3 == 0)
            f.write('clip%d, 0.000, 10.000, "%s"\n' % (i, mids))
            with wave.open(os.path.join(root, "eval_segments", "clip%d.wav" % i), "wb") as w:
                w.setnchannels(1)
                w.setsampwidth(2)
                w.setframerate(16000)
                w.writeframes((rs.standard_normal(3000 + 100 * i) * 3000).astype("<i2").tobytes())
    return root


def test_evaluate_cls_end_to_end(tmp_path):
    from m3t.trainer import Trainer
    from models.audioset_model import AudioSet
    tree = _write_tree(str(tmp_path / "audioset"))
    hp = AudioSet.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    hp.dataset_path, hp.window, hp.batch_size, hp.num_hidden, hp.checkpoint_path, hp.scheduler = tree, 4, 4, 16, None, "none"
    torch.manual_seed(3)
    model = AudioSet(hp).cuda().eval()
    tr = Trainer.from_hparams(model, hp, gradient_clip_val=1.0)
    feed = model.val_dataloader()
    assert len(feed.files) == 9 and len(feed) == 3
    want = tr.validate(feed)
    got = tr.evaluate_cls(feed)
    assert got["val_loss"] == float(want["val_loss"]) and got["log"]["val_acc"] == want["log"]["val_acc"]      # float32 bits, widened exactly
    assert sorted(got["progress_bar"]) == ["val_acc", "val_auc", "val_dprime", "val_loss", "val_map"]
    # the scores are model.forward's; the labels the scan's
    scores = np.concatenate([model.forward(b["audio"]).detach().cpu().numpy() for b in feed])
    labels = feed.scan.labels.astype(np.float32)
    assert scores.shape == labels.shape == (9, 527) and (labels.sum(0) == 3).all()
    assert tr.last_eval.metrics == got["log"]
    e = _check(tr.last_eval, scores, labels)
    assert e["n_classes_auc"] == 527
    first = tr.last_eval
    tr.evaluate_cls(feed)
    _same_bits(first, tr.last_eval)
