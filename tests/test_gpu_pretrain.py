"""The pre-training tasks on the MI355X: the three loss-end operators of csrc/cls_loss.hip against the float64 restatement
(tests/pretrain_ref.py) -- awkward shapes, ties, large logits, NaN -- and the task modules VoxCeleb2_1k / AudioSet against the reference's own
runs (tests/golden/vox2_*.npz, audioset_eval*.npz), a float64 stock-torch composition (train-mode dropout, the default shapes), the trainer
loop and the checkpoint surgery.

Operator tolerance: the yardstick of a tensor is E32 = the largest error of torch's own float32 CPU result of the same formula on the
same inputs, measured against float64; an element of the GPU result may be off by 4 E32, or by 4 ulp of its reference value where that is
more.  The factor 4 allows for another summation order over up to 1025 terms.  Each test prints the worst ratio error / max(E32, ulp) it saw
(bound: 4)."""
import argparse
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pretrain_cases as P
import pretrain_ref as R
from conftest import load_golden
from golden.recipe import fill_module, grad_digest, draw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = [0.0]


# ------------------------------------------------------------------ operators
def _torch32(z, target, mode, kind):
    """torch's float32 CPU composition: pooled, loss, dpooled, dz"""
    zt = torch.from_numpy(z).requires_grad_(True)
    pooled = zt.mean(dim=1) if mode else zt.max(dim=1)[0]
    pooled.retain_grad()
    tt = torch.from_numpy(target)
    loss = F.cross_entropy(pooled, tt) if kind == 0 else F.binary_cross_entropy_with_logits(pooled, tt)
    loss.backward()
    return dict(pooled=pooled.detach().numpy(), loss=loss.detach().numpy(), dpooled=pooled.grad.numpy(), dz=zt.grad.numpy())


def _ratio(got, ref, yard32, what):
    """worst of |got - ref| / max(E32, ulp32(|ref|)) over the tensor; asserts it is at most 4"""
    got = np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), what
    e32 = float(np.abs(np.asarray(yard32, np.float64) - ref).max()) if ref.size else 0.0
    unit = np.maximum(e32, np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    r = float((np.abs(got - ref) / unit).max()) if ref.size else 0.0
    WORST[0] = max(WORST[0], r)
    assert r <= 4.0, "%s: error / max(E32 = %.3e, ulp) = %.2f" % (what, e32, r)
    return r


def _run_ops(z, target, mode, kind):
    """fused and two-step paths on the GPU; returns their outputs as dicts"""
    from m3t import ops
    tt = torch.from_numpy(target).to(DEV)
    zf = torch.from_numpy(z).to(DEV).requires_grad_(True)
    loss, stats, correct, pooled, arg = ops.pooled_cls_loss(zf, tt, mode, kind, return_pooled=True)
    loss.backward()
    fused = dict(loss=loss.detach(), stats=stats, correct=correct, pooled=pooled, arg=arg, dz=zf.grad)
    z2 = torch.from_numpy(z).to(DEV).requires_grad_(True)
    if mode == 0:
        p2, a2 = ops.temporal_pool(z2, mode, return_indices=True)
    else:
        p2, a2 = ops.temporal_pool(z2, mode), torch.empty(0, dtype=torch.int32, device=DEV)
    p2.retain_grad()
    loss2, stats2, correct2 = ops.cls_loss(p2, tt, kind)
    loss2.backward()
    two = dict(loss=loss2.detach(), stats=stats2, correct=correct2, pooled=p2.detach(), arg=a2, dz=z2.grad, dpooled=p2.grad)
    return fused, two


def _same_bits(a, b, what):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _check_against_ref(z, target, mode, kind, tag):
    r = R.pooled_cls_loss(z, target, mode, kind)
    y = _torch32(z, target, mode, kind)
    fused, two = _run_ops(z, target, mode, kind)
    worst = 0.0
    for name, out in (("fused", fused), ("two-step", two)):
        worst = max(worst, _ratio(out["pooled"], r["pooled"], y["pooled"], "%s %s pooled" % (tag, name)),
                    _ratio(out["loss"], r["loss"], y["loss"], "%s %s loss" % (tag, name)),
                    _ratio(out["dz"], r["dz"], y["dz"], "%s %s dz" % (tag, name)))
        np.testing.assert_array_equal(out["correct"].cpu().numpy(), r["correct"], err_msg="%s %s correct" % (tag, name))
        assert out["stats"].shape == (2,) and float(out["stats"][1]) == r["n_correct"] and float(out["stats"][0]) == float(out["loss"])
        if mode == 0:
            np.testing.assert_array_equal(out["arg"].cpu().numpy(), r["arg"], err_msg="%s %s arg" % (tag, name))
    worst = max(worst, _ratio(two["dpooled"], r["dpooled"], y["dpooled"], tag + " dlogits"))
    for k in ("loss", "stats", "correct", "pooled", "arg", "dz"):          # one arithmetic behind both paths
        _same_bits(fused[k], two[k], "%s fused vs two-step %s" % (tag, k))
    return worst


@pytest.mark.parametrize("kind", [0, 1], ids=["ce", "bce"])
@pytest.mark.parametrize("mode", [0, 1], ids=["max", "mean"])
@pytest.mark.parametrize("B,T,C", P.SHAPES)
def test_operators_match_float64_restatement(B, T, C, mode, kind):
    z, target = P.make_case(B, T, C, mode, kind)
    assert P.top2_margin(R.tpool_fwd(z, mode)[0]) > P.MARGIN          # (tests/test_pretrain_host.py checks every case on the CPU)
    worst = _check_against_ref(z, target, mode, kind, "B%d T%d C%d" % (B, T, C))
    print("worst error / max(E32, ulp) = %.3f (bound 4); over this run so far %.3f" % (worst, WORST[0]))


@pytest.mark.parametrize("kind", [0, 1], ids=["ce", "bce"])
def test_first_index_wins_ties_in_time_and_class(kind):
    from m3t import ops
    z = np.zeros((2, 3, 5), np.float32)
    z[0, 1, 2] = z[0, 2, 2] = 1.0          # clip 0: column 2 has its maximum at frames 1 and 2 ...
    z[0, 0, 0] = 1.0                       # ... and ties with column 0 for the top-1 class
    z[1] = -2.0                            # clip 1: everything ties
    target = np.array([0, 3], np.int64) if kind == 0 else np.eye(5, dtype=np.float32)[[0, 1]]
    r = R.pooled_cls_loss(z, target, 0, kind)
    fused, two = _run_ops(z, target, 0, kind)
    for out in (fused, two):
        arg, dz = out["arg"].cpu().numpy(), out["dz"].cpu().numpy()
        assert arg[0, 2] == 1 and (arg[1] == 0).all()
        np.testing.assert_array_equal(arg, r["arg"])
        np.testing.assert_array_equal(out["correct"].cpu().numpy(), r["correct"])
        assert out["correct"].cpu().tolist() == ([1.0, 0.0] if kind == 0 else [1.0, 0.0])
        assert np.count_nonzero(dz[0, :, 2]) == 1 and dz[0, 1, 2] != 0          # the gradient lands on one element only
        assert np.count_nonzero(dz[1, 1:]) == 0 and np.count_nonzero(dz[1, 0]) == 5
        np.testing.assert_allclose(dz, r["dz"], rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("kind", [0, 1], ids=["ce", "bce"])
@pytest.mark.parametrize("mode", [0, 1], ids=["max", "mean"])
@pytest.mark.parametrize("mag", [80.0, 1e4])
def test_large_logits_stay_finite_and_exact(mag, mode, kind):
    rs = np.random.RandomState(int(mag) + 2 * mode + kind)
    B, T, C = 3, 2, 65
    z = (np.where(rs.uniform(size=(B, T, C)) < 0.5, -1.0, 1.0) * mag).astype(np.float32)
    z[0, :, 5] = mag * 1.5                 # one clear winner in clip 0; the other clips tie at +mag (first index wins)
    target = rs.randint(0, C, (B,)).astype(np.int64) if kind == 0 else (rs.uniform(size=(B, C)) < 0.3).astype(np.float32)
    r = R.pooled_cls_loss(z, target, mode, kind)
    worst = _check_against_ref(z, target, mode, kind, "mag %g" % mag)
    fused, _ = _run_ops(z, target, mode, kind)
    # logsumexp / log1p exact to rounding: the float next to the float64 value
    assert abs(float(fused["loss"]) - r["loss"]) <= float(np.spacing(np.float32(abs(r["loss"])))), (float(fused["loss"]), r["loss"])
    print("worst error / max(E32, ulp) = %.3f (bound 4)" % worst)


@pytest.mark.parametrize("kind", [0, 1], ids=["ce", "bce"])
@pytest.mark.parametrize("mode", [0, 1], ids=["max", "mean"])
def test_nan_in_one_clip_stays_in_that_clip(mode, kind):
    z, target = P.make_case(3, 2, 7, mode, kind)
    zn = z.copy()
    zn[1, 0, 3] = np.nan
    r = R.pooled_cls_loss(zn, target, mode, kind)
    clean, _ = _run_ops(z, target, mode, kind)
    for out in _run_ops(zn, target, mode, kind):
        dz, pooled = out["dz"].cpu().numpy(), out["pooled"].cpu().numpy()
        assert np.isnan(float(out["loss"])) and np.isnan(pooled[1, 3]) and np.isnan(dz[1, :, 3]).any()
        np.testing.assert_array_equal(np.isnan(pooled), np.isnan(r["pooled"]))
        np.testing.assert_array_equal(np.isnan(dz), np.isnan(r["dz"]))
        ok = ~np.isnan(r["dz"])
        np.testing.assert_allclose(dz[ok], r["dz"][ok], rtol=1e-5, atol=1e-9)
        np.testing.assert_array_equal(out["correct"].cpu().numpy(), r["correct"])
        if mode == 0:
            np.testing.assert_array_equal(out["arg"].cpu().numpy(), r["arg"])
        for b in (0, 2):                   # the other clips' rows: the bits of the run without the NaN
            assert dz[b].tobytes() == clean["dz"][b].cpu().numpy().tobytes()
            assert pooled[b].tobytes() == clean["pooled"][b].cpu().numpy().tobytes()


def test_reruns_are_bit_identical_and_grad_scales():
    from m3t import ops
    z, target = P.make_case(257, 2, 1000, 1, 0)
    a, _ = _run_ops(z, target, 1, 0)
    b, _ = _run_ops(z, target, 1, 0)
    for k in ("loss", "dz", "pooled", "correct"):
        _same_bits(a[k], b[k], k)
    zt = torch.from_numpy(z).to(DEV).requires_grad_(True)
    loss, _, _ = ops.pooled_cls_loss(zt, torch.from_numpy(target).to(DEV), 1, 0)
    (2.0 * loss).backward()
    assert torch.equal(zt.grad, 2.0 * a["dz"])


# ------------------------------------------------------------------ modules
def _hp(cls, **kw):
    ns = cls.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _close(a, b, tol, what):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max())
    print("%s: max abs err %.3e (bound %.1e x max(1, %.3e))" % (what, err, tol, float(np.abs(b).max())))
    assert err <= tol * max(1.0, float(np.abs(b).max())), "%s: max abs err %.3e" % (what, err)


def _digest_ok(grad, ref, tol, what):
    got = grad_digest(grad.detach().double().cpu().numpy())
    scale = max(1.0, float(np.abs(ref[2:]).max()))
    e_n, e_h = abs(got[0] - ref[0]) / max(1.0, ref[0]), float(np.abs(got[2:] - ref[2:]).max()) / scale
    assert e_n <= tol and e_h <= tol, "%s: norm off by %.3e, head by %.3e (relative; bound %.1e)" % (what, e_n, e_h, tol)
    return max(e_n, e_h)


def _acc_exact(acc, ref, B):
    """train_acc = n_correct / B in float32, n_correct the reference's count"""
    n = round(float(ref) * B)
    assert abs(float(ref) * B - n) < 1e-9 and np.float32(float(acc)) == np.float32(n) / np.float32(B), (float(acc), float(ref))


def _vox(g_or_T, seed=None, training=True):
    from models.vox2_model import VoxCeleb2_1k
    T = int(g_or_T["dims"][1]) if isinstance(g_or_T, dict) else g_or_T
    seed = int(g_or_T["seed"]) if isinstance(g_or_T, dict) else seed
    m = fill_module(VoxCeleb2_1k(_hp(VoxCeleb2_1k, window=T)), seed + 1).to(DEV)
    return m.train() if training else m.eval()


def _vox_batch(seed, B, T, S, label=None):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.randint(0, 256, (B, 3, T, S, S)).astype(np.float32)).to(DEV)
    label = rs.randint(0, 1000, (B,)).astype(np.int64) if label is None else label
    return {"video": x, "label": torch.from_numpy(label).to(DEV)}


@pytest.mark.parametrize("name", ["vox2_train", "vox2_eval"])
def test_vox2_golden(name):
    g = load_golden(name)
    B, T, S = [int(v) for v in g["dims"]]
    training = bool(int(g["training"]))
    m = _vox(g, training=training)
    batch = _vox_batch(int(g["seed"]), B, T, S, g["label"])
    with torch.no_grad():
        y = copy.deepcopy(m)(batch["video"])          # (a copy: a train-mode forward moves the BatchNorm buffers)
    _close(y, g["y"], 1e-4, "pooled logits")
    out = m.training_step(batch, 0)
    _close(out["loss"], g["loss"], 1e-4, "loss")
    _acc_exact(out["log"]["train_acc"], g["train_acc"], B)
    out["loss"].backward()
    assert sorted(n for n, p in m.named_parameters() if p.grad is not None) == sorted(k[3:] for k in g if k.startswith("gd."))
    worst = max(_digest_ok(p.grad, g["gd." + n], 2e-4, n) for n, p in m.named_parameters())
    print("worst gradient-digest error %.3e (bound 2e-4)" % worst)
    if training:
        n_checked = 0
        for n, b in m.named_buffers():
            leaf = n.split(".")[-1]
            if leaf == "num_batches_tracked":
                assert int(b) == int(g["bn." + n]), n
            else:
                _close(b, g["bn." + n], 2e-4, n)
            n_checked += 1
        assert n_checked == 3 * 5
    else:
        val = m.validation_step(batch, 0)
        _close(val["val_loss"], g["val_loss"], 1e-4, "val_loss")
        np.testing.assert_array_equal(val["correct"].float().cpu().numpy(), g["correct"])
        assert not val["val_loss"].requires_grad


def _audioset(H, T, seed, training=False):
    from models.audioset_model import AudioSet
    m = fill_module(AudioSet(_hp(AudioSet, num_hidden=H, window=T)), seed + 1).to(DEV)
    return m.train() if training else m.eval()


@pytest.mark.parametrize("name", ["audioset_eval", "audioset_eval_h256"])
def test_audioset_golden(name):
    from m3t import ops
    g = load_golden(name)
    B, T, H = [int(v) for v in g["dims"]]
    m = _audioset(H, T, int(g["seed"]))
    rs = np.random.RandomState(int(g["seed"]))
    batch = {"audio": torch.from_numpy(draw(rs, (B, T, 200))).to(DEV), "label": torch.from_numpy(g["target"]).to(DEV)}
    with torch.no_grad():
        y = m(batch["audio"])
        _, arg = ops.temporal_pool(m.audio(batch["audio"]), "max", return_indices=True)
    _close(y, g["y"], 1e-4, "pooled logits")
    np.testing.assert_array_equal(arg.cpu().numpy(), g["arg"])
    out = m.training_step(batch, 0)
    _close(out["loss"], g["loss"], 1e-4, "loss")
    _acc_exact(out["log"]["train_acc"], g["train_acc"], B)
    out["loss"].backward()
    assert sorted(n for n, p in m.named_parameters() if p.grad is not None) == sorted(k[3:] for k in g if k.startswith("gd."))
    worst = max(_digest_ok(p.grad, g["gd." + n], 2e-4, n) for n, p in m.named_parameters())
    print("worst gradient-digest error %.3e (bound 2e-4)" % worst)
    val = m.validation_step(batch, 0)
    _close(val["val_loss"], g["val_loss"], 1e-4, "val_loss")
    np.testing.assert_array_equal(val["correct"].cpu().numpy(), g["correct"])


def _param_grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("task", ["vox", "aud"])
def test_forward_then_loss_equals_training_step(task):
    """forward() + ce_loss / bce_loss (temporal pooling and loss as two differentiable operators) against training_step (the fused one)"""
    if task == "vox":
        # eval mode: in front of a batch-statistics BatchNorm a convolution's bias has an exactly zero gradient, and what either path
        # leaves there is rounding residue (1e-7 of sums that cancel) with nothing to scale a comparison by
        m, batch, key, lossf = _vox(3, seed=21, training=False), _vox_batch(22, 2, 3, 112), "video", "ce_loss"
    else:
        m = _audioset(16, 6, 23)
        rs = np.random.RandomState(24)
        batch = {"audio": torch.from_numpy(draw(rs, (3, 6, 200))).to(DEV),
                 "label": torch.from_numpy((rs.uniform(size=(3, 527)) < 0.02).astype(np.float32)).to(DEV)}
        key, lossf = "audio", "bce_loss"
    m2 = copy.deepcopy(m)
    out = m.training_step(batch, 0)
    out["loss"].backward()
    y_hat = m2(batch[key])
    assert y_hat.requires_grad and y_hat.shape == (batch[key].shape[0], 1000 if task == "vox" else 527)
    loss2 = getattr(m2, lossf)(y_hat, batch["label"])
    loss2.backward()
    assert abs(float(loss2) - float(out["loss"])) <= 4 * float(np.spacing(np.float32(abs(float(loss2)))))
    g1, g2 = _param_grads(m), _param_grads(m2)
    for n in g1:
        scale = max(float(g2[n].abs().max()), 1e-30)
        assert float((g1[n] - g2[n]).abs().max()) <= 1e-5 * scale, n


def _audioset_ref64(m, x, target, seeds=None):
    """float64 stock-torch composition with m's weights: nn.GRU, the head (with the oracle's dropout masks for `seeds`), temporal max,
    BCE-with-logits, top-1 -- returns (pooled, loss, n_correct, {name: grad})"""
    from oracle import m3t_oracle as O
    H = m.audio.hidden_size
    gru = torch.nn.GRU(200, H, 2, batch_first=True, bidirectional=True).double()
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    gru.load_state_dict({k[len("audio.gru."):]: v for k, v in sd.items() if k.startswith("audio.gru.")})
    w = {k[len("audio."):]: v.clone().requires_grad_(True) for k, v in sd.items() if k.startswith("audio.fc.")}
    xd, td = x.detach().double().cpu(), target.detach().double().cpu()
    B, T = xd.shape[:2]
    h = gru(xd)[0].reshape(B * T, 2 * H)
    h = torch.relu(F.linear(h, w["fc.0.weight"], w["fc.0.bias"]))
    if seeds is not None:
        h = h * torch.from_numpy(O.dropout_mask(B * T, H, 0.5, seeds[0]))
    z = F.linear(h, w["fc.3.weight"], w["fc.3.bias"]).reshape(B, T, 527)
    pooled = z.max(dim=1)[0]
    loss = F.binary_cross_entropy_with_logits(pooled, td)
    loss.backward()
    n_correct = float(td.gather(1, pooled.argmax(dim=-1).view(-1, 1)).sum())
    grads = {"audio.gru." + n: p.grad for n, p in gru.named_parameters()}
    grads.update({"audio." + n: p.grad for n, p in w.items()})
    return pooled.detach(), float(loss.detach()), n_correct, grads


def _aud_batch(seed, B, T):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(draw(rs, (B, T, 200))).to(DEV)
    t = (rs.uniform(size=(B, 527)) < 0.01).astype(np.float32)
    return {"audio": x, "label": torch.from_numpy(t).to(DEV)}


def test_audioset_train_mode_dropout_matches_float64_with_oracle_masks():
    m = _audioset(16, 7, 31, training=True)
    seeds = [0x1234567811223344, 0x0FEDCBA987654321]
    m.audio.drop_seeds = seeds
    batch = _aud_batch(32, 3, 7)
    out = m.training_step(batch, 0)
    out["loss"].backward()
    pooled, loss, n_correct, grads = _audioset_ref64(m, batch["audio"], batch["label"], seeds)
    _close(out["loss"], loss, 1e-4, "loss (train mode, pinned seeds)")
    assert float(out["log"]["train_acc"]) * 3 == pytest.approx(n_correct)
    for n, p in m.named_parameters():
        _digest_ok(p.grad, grad_digest(grads[n].numpy()), 2e-4, n)
    with torch.no_grad():
        y = m(batch["audio"])
        _close(y, pooled, 1e-4, "pooled logits (train mode, pinned seeds)")
        m.audio.drop_seeds = [1, 2]
        y2 = m(batch["audio"])
        y_eval = m.eval()(batch["audio"])
        m.audio.drop_seeds = seeds
        y_eval2 = m(batch["audio"])
    assert not torch.equal(y2, y) and not torch.equal(y_eval, y) and torch.equal(y_eval, y_eval2)


def test_audioset_default_shape_trainer_step_matches_float64():
    """128 x 32 x 200, num_hidden 256 (the reference's defaults) through Trainer.step: loss, accuracy and the (clipped) gradients the
    optimizer saw against the float64 composition of the weights before the step"""
    from models.audioset_model import AudioSet
    from m3t.trainer import Trainer
    hp = _hp(AudioSet, learning_rate=1e-3)
    m = fill_module(AudioSet(hp), 41).to(DEV)
    seeds = [11, 12]
    m.audio.drop_seeds = seeds
    batch = _aud_batch(42, hp.batch_size, hp.window)
    assert batch["audio"].shape == (128, 32, 200)
    before = copy.deepcopy(m).train()
    tr = Trainer.from_hparams(m, hp, checkpoint_path=None)
    out = tr.step(batch)
    pooled, loss, n_correct, grads = _audioset_ref64(before, batch["audio"], batch["label"], seeds)
    _close(out["loss"], loss, 1e-4, "loss")
    assert torch.is_tensor(out["log"]["train_acc"]) and float(out["log"]["train_acc"]) * 128 == pytest.approx(n_correct)
    norm = float(np.sqrt(sum(float((g * g).sum()) for g in grads.values())))
    _close(out["grad_norm"].reshape(()), norm, 2e-4, "gradient norm")
    coef = min(1.0, 1.0 / (norm + 1e-6))
    worst = max(_digest_ok(p.grad, grad_digest(grads[n].numpy() * coef), 2e-4, n) for n, p in m.named_parameters())
    print("worst gradient-digest error %.3e (bound 2e-4)" % worst)


VOX_DEFAULT_CLIPS = 128      # the reference's batch_size (vox2_model.py:178)


def test_vox_default_shape_trainer_step():
    """128 clips x 16 frames x 112 x 112 (the reference's defaults) through Trainer.step: the scans and the loss take B = 128.  No CPU
    reference at that size."""
    from models.vox2_model import VoxCeleb2_1k
    from m3t.trainer import Trainer
    hp = _hp(VoxCeleb2_1k, learning_rate=1e-3)
    m = fill_module(VoxCeleb2_1k(hp), 51).to(DEV)
    tr = Trainer.from_hparams(m, hp, checkpoint_path=None)
    batch = _vox_batch(52, VOX_DEFAULT_CLIPS, hp.window, 112)
    out = tr.step(batch)
    acc = float(out["log"]["train_acc"])
    assert np.isfinite(float(out["loss"])) and np.isfinite(float(out["grad_norm"])) and float(out["grad_norm"]) > 0
    assert 0.0 <= acc <= 1.0 and acc * VOX_DEFAULT_CLIPS == round(acc * VOX_DEFAULT_CLIPS)


@pytest.mark.parametrize("task", ["vox", "aud"])
def test_trainer_steps_validate_and_checkpoint_surgery(task, tmp_path):
    from m3t import checkpoints
    from m3t.trainer import Trainer
    from models.model import AffWild2VA
    from models.vox2_model import VoxCeleb2_1k
    from models.audioset_model import AudioSet
    torch.manual_seed(61)
    if task == "vox":
        hp = _hp(VoxCeleb2_1k, window=3, learning_rate=1e-3, checkpoint_path=str(tmp_path / "vox2"))
        m, batches = VoxCeleb2_1k(hp).to(DEV), [_vox_batch(62 + i, 2, 3, 112) for i in range(2)]
    else:
        hp = _hp(AudioSet, window=6, learning_rate=1e-3, checkpoint_path=str(tmp_path / "audioset"))     # num_hidden 256: AffWild2VA's audio GRU
        m, batches = AudioSet(hp).to(DEV), [_aud_batch(64 + i, 3, 6) for i in range(2)]
    tr = Trainer.from_hparams(m, hp)
    for i in range(3):
        out = tr.step(batches[i % 2])
        assert np.isfinite(float(out["loss"])) and set(out["log"]) == {"loss", "train_acc"}
    res = tr.validate(batches)
    assert np.isfinite(float(res["val_loss"])) and 0.0 <= res["log"]["val_acc"] <= 1.0
    assert tr.end_epoch(float(res["val_loss"]))                      # the best-val_loss checkpoint
    ck = torch.load(os.path.join(hp.checkpoint_path, "best.ckpt"), map_location="cpu")
    assert list(ck["state_dict"]) == list(m.state_dict())
    av = AffWild2VA(_hp(AffWild2VA, modality="audiovisual", backbone="v2p_split", split_layer=3))
    if task == "vox":
        video = checkpoints.export_pretrained_video(ck)
        fused = checkpoints.merge_av({k: v for k, v in av.state_dict().items() if k.startswith("audio.")}, video)
        pairs = [("visual.v2p.0.weight", "visual.shared.0.weight"), ("visual.v2p.12.weight", "visual.v_private.0.weight"),
                 ("visual.v2p.16.weight", "visual.a_private.4.weight"), ("visual.v2p.1.running_var", "visual.shared.1.running_var")]
    else:
        fused = checkpoints.merge_av(ck, {k: v for k, v in av.state_dict().items() if k.startswith("visual.")})
        pairs = [(k, k) for k in ck["state_dict"] if k.startswith("audio.gru.")]
    res = av.load_state_dict(fused["state_dict"], strict=False)
    assert res.unexpected_keys == [] and not any(k.startswith("audio.fc") for k in fused["state_dict"])
    for src, dst in pairs:
        assert torch.equal(av.state_dict()[dst], m.state_dict()[src].cpu()), (src, dst)


@pytest.mark.parametrize("task", ["vox", "aud"])
def test_training_step_has_no_host_sync(task, monkeypatch):
    """M3T_STEP_SYNC unset: nothing between the forward pass and the end of backward waits for the device, and train_acc is a 0-dim
    device tensor; M3T_STEP_SYNC=1: a Python float with the same value"""
    import models.audioset_model as am
    import models.vox2_model as vm
    monkeypatch.setattr(vm, "_STEP_SYNC", False)
    monkeypatch.setattr(am, "_STEP_SYNC", False)
    if task == "vox":
        m, batch = _vox(3, seed=71), _vox_batch(72, 2, 3, 112)
    else:
        m, batch = _audioset(16, 6, 73, training=True), _aud_batch(74, 3, 6)
        m.audio.drop_seeds = [5, 6]
    m.training_step(batch, 0)["loss"].backward()          # warm-up: lazy initialisation may synchronise
    torch.cuda.synchronize()
    m.zero_grad()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = m.training_step(batch, 1)
        out["loss"].backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    acc = out["log"]["train_acc"]
    assert torch.is_tensor(acc) and acc.is_cuda and acc.dim() == 0 and not acc.requires_grad
    assert out["progress_bar"]["train_acc"] is acc
    monkeypatch.setattr(vm, "_STEP_SYNC", True)
    monkeypatch.setattr(am, "_STEP_SYNC", True)
    acc2 = m.eval().training_step(batch, 2)["log"]["train_acc"]
    assert isinstance(acc2, float) and 0.0 <= acc2 <= 1.0
    monkeypatch.setattr(vm, "_STEP_SYNC", False)
    monkeypatch.setattr(am, "_STEP_SYNC", False)
    assert float(m.training_step(batch, 3)["log"]["train_acc"]) == pytest.approx(acc2, rel=1e-6)
