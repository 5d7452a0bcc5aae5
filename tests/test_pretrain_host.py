"""The pre-training tasks on the host side (no GPU): the module contracts of models/vox2_model.py and models/audioset_model.py against
the reference (tests/golden/pretrain_init.npz, vox2_*.npz, written by gen_golden_pretrain.py) -- names, shapes, flags, the init RNG order --
the checkpoint surgery of m3t/checkpoints.py against the reference scripts' key lists, the float64 restatement of the loss end
(tests/pretrain_ref.py) against torch's float64 autograd, the stock path a CPU tensor takes through m3t.ops against the restatement, and
VoxCeleb2_1k's CPU path against the reference's own run."""
import argparse
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pretrain_cases as P
import pretrain_ref as R
from conftest import load_golden


def _hp(cls, **kw):
    ns = cls.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _modules():
    from models.vox2_model import VoxCeleb2_1k
    from models.audioset_model import AudioSet
    return {"vox": VoxCeleb2_1k, "aud": AudioSet}


def _names_shapes(m):
    items = sorted(list(m.named_parameters()) + list(m.named_buffers()), key=lambda kv: kv[0])
    return [n for n, _ in items], [",".join(str(d) for d in t.shape) for _, t in items]


def _rel(got, ref):
    got = got.detach().double().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    ref = np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))


# ------------------------------------------------------------------ module contract
@pytest.mark.parametrize("tag", ["vox", "aud"])
def test_names_shapes_and_flags_match_reference(tag):
    g = load_golden("pretrain_init")
    cls = _modules()[tag]
    names, shapes = _names_shapes(cls(_hp(cls)))
    assert names == list(g[tag + ".names"])
    assert shapes == list(g[tag + ".shapes"])
    assert sorted("%s=%s" % kv for kv in vars(_hp(cls)).items()) == list(g[tag + ".flags"])


def test_state_dict_keys_end_as_the_reference_heads():
    mods = _modules()
    vox, aud = mods["vox"](_hp(mods["vox"])), mods["aud"](_hp(mods["aud"]))
    assert {k.rsplit(".", 1)[0] for k in vox.state_dict() if k.startswith("visual.fc")} == {"visual.fc.0", "visual.fc.2"}
    assert {k.rsplit(".", 1)[0] for k in aud.state_dict() if k.startswith("audio.fc")} == {"audio.fc.0", "audio.fc.3"}


@pytest.mark.parametrize("tag", ["vox", "aud"])
def test_init_digests_match_reference_rng_order(tag):
    from golden.recipe import grad_digest
    g = load_golden("pretrain_init")
    cls = _modules()[tag]
    torch.manual_seed(int(g["seed"]))
    m = cls(_hp(cls))
    n_checked = 0
    for n, t in m.state_dict().items():
        if not t.dtype.is_floating_point:
            continue
        # per-gate orthogonal weight_hh of the GRU: LAPACK QR rounding depends on the host BLAS (see test_host_api.py)
        atol = 4e-6 if "weight_hh" in n else 1e-7
        np.testing.assert_allclose(grad_digest(t.numpy()), g["sd.%s.%s" % (tag, n)], rtol=1e-6, atol=atol, err_msg=n)
        n_checked += 1
    assert n_checked == len([k for k in g if k.startswith("sd.%s." % tag)])


@pytest.mark.parametrize("backbone", ["resnet", "densenet"])
def test_vox_constructor_accepts_the_other_backbones(backbone):
    cls = _modules()["vox"]
    m = cls(_hp(cls, backbone=backbone, backend="gru"))
    assert any(k.startswith("visual.") for k in m.state_dict())


@pytest.mark.parametrize("tag", ["vox", "aud"])
def test_lr_range_finder_is_out_of_scope(tag):
    cls = _modules()[tag]
    m = cls(_hp(cls, test_lr=True))
    with pytest.raises(NotImplementedError, match="LR range finder"):
        m.configure_optimizers()


@pytest.mark.parametrize("tag", ["vox", "aud"])
@pytest.mark.parametrize("scheduler", ["plateau", "exp", "cyclic"])
def test_configure_optimizers_as_reference(tag, scheduler):
    cls = _modules()[tag]
    m = cls(_hp(cls, scheduler=scheduler, num_hidden=16) if tag == "aud" else _hp(cls, scheduler=scheduler))
    res = m.configure_optimizers()
    opt = res if scheduler == "cyclic" else res[0][0]
    assert isinstance(opt, torch.optim.SGD if tag == "vox" else torch.optim.Adam)
    assert opt.defaults["weight_decay"] == (5e-4 if tag == "vox" else 1e-4)
    if scheduler == "cyclic":
        assert m.cyclic_scheduler.total_size == 2 * (5000 if tag == "vox" else 480)
        m.on_batch_end()
    else:
        assert type(res[1][0]).__name__ == {"plateau": "ReduceLROnPlateau", "exp": "ExponentialLR"}[scheduler]


def test_validation_end_as_reference():
    cls = _modules()["aud"]
    m = cls(_hp(cls, num_hidden=16))
    outs = [{"val_loss": torch.tensor(1.0), "correct": torch.tensor([1.0, 0.0])}, {"val_loss": torch.tensor(2.0), "correct": torch.tensor([1.0, 1.0])}]
    res = m.validation_end(outs)
    assert float(res["val_loss"]) == 1.5 and res["log"]["val_acc"] == 0.75 and res["progress_bar"]["val_acc"] == 0.75


# ------------------------------------------------------------------ checkpoint surgery
def test_surgery_key_lists_match_reference_scripts():
    from m3t import checkpoints
    from models.model import AffWild2VA
    g = load_golden("pretrain_init")
    mods = _modules()
    vox, aud = mods["vox"](_hp(mods["vox"])), mods["aud"](_hp(mods["aud"]))
    video = checkpoints.export_pretrained_video(vox.state_dict())
    assert list(video) == ["state_dict"]
    assert list(video["state_dict"]) == list(g["export.keys"])
    fused = checkpoints.merge_av({"state_dict": aud.state_dict()}, video)
    assert list(fused["state_dict"]) == list(g["merge.keys"])
    va = AffWild2VA(_hp(AffWild2VA, modality="visual", backbone="v2p_split", split_layer=3))
    assert list(checkpoints.merge_av(aud.state_dict(), va.state_dict())["state_dict"]) == list(g["merge_va.keys"])


def test_merged_checkpoint_loads_into_affwild2va_bit_equal():
    from m3t import checkpoints
    from models.model import AffWild2VA
    mods = _modules()
    torch.manual_seed(5)
    vox, aud = mods["vox"](_hp(mods["vox"])), mods["aud"](_hp(mods["aud"]))
    for b in vox.buffers():                   # running statistics that differ from a fresh module's
        if b.dtype.is_floating_point:
            b.uniform_(0.5, 1.5)
    fused = checkpoints.merge_av(aud.state_dict(), checkpoints.export_pretrained_video(vox.state_dict()))
    av = AffWild2VA(_hp(AffWild2VA, modality="audiovisual", backbone="v2p_split", split_layer=3))
    res = av.load_state_dict(fused["state_dict"], strict=False)
    assert res.unexpected_keys == []
    assert all(k.startswith(("visual.gru_", "proj_v.", "fusion.")) for k in res.missing_keys), res.missing_keys
    sd, n = av.state_dict(), 0
    for k, w in vox.state_dict().items():
        if k.startswith("visual.fc"):
            continue
        i, rest = int(k.split(".")[2]), k.split(".", 3)[3]
        for nk in (["visual.shared.%d.%s" % (i, rest)] if i < 12 else ["visual.%s_private.%d.%s" % (t, i - 12, rest) for t in "va"]):
            assert torch.equal(sd[nk], w), nk
            n += 1
    for k, w in aud.state_dict().items():
        if k.startswith("audio.gru"):
            assert torch.equal(sd[k], w), k
            n += 1
    assert n == len(fused["state_dict"])
    assert not any(k.startswith("audio.fc") for k in fused["state_dict"])


# ------------------------------------------------------------------ the restatement against torch's float64 autograd
CASES = [(3, 5, 7), (1, 1, 1), (2, 2, 65), (4, 3, 527)]


@pytest.mark.parametrize("B,T,C", CASES)
@pytest.mark.parametrize("mode", [R.MAX, R.MEAN])
@pytest.mark.parametrize("kind", [R.CE, R.BCE])
def test_restatement_agrees_with_torch_float64(B, T, C, mode, kind):
    rs = np.random.RandomState(100 * B + 10 * T + C + mode + 2 * kind)
    z = rs.standard_normal((B, T, C)) * 3
    target = rs.randint(0, C, (B,)) if kind == R.CE else (rs.uniform(size=(B, C)) < 0.3).astype(np.float64)
    r = R.pooled_cls_loss(z, target, mode, kind)
    zt = torch.from_numpy(z).requires_grad_(True)
    pooled = zt.mean(dim=1) if mode == R.MEAN else zt.max(dim=1)[0]
    pooled.retain_grad()
    tt = torch.from_numpy(target)
    loss = F.cross_entropy(pooled, tt) if kind == R.CE else F.binary_cross_entropy_with_logits(pooled, tt)
    loss.backward()
    top = pooled.argmax(dim=-1)
    correct = (top == tt).double() if kind == R.CE else tt.gather(1, top.view(-1, 1)).view(-1)
    np.testing.assert_allclose(r["pooled"], pooled.detach().numpy(), rtol=1e-15, atol=0)
    np.testing.assert_allclose(r["loss"], float(loss.detach()), rtol=1e-14)
    np.testing.assert_allclose(r["dpooled"], pooled.grad.numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_allclose(r["dz"], zt.grad.numpy(), rtol=1e-12, atol=1e-18)
    np.testing.assert_array_equal(r["correct"], correct.numpy())
    if mode == R.MAX:
        np.testing.assert_array_equal(r["arg"], zt.detach().max(dim=1)[1].numpy())


def test_restatement_first_index_wins_on_ties():
    z = np.zeros((1, 3, 4))
    z[0, 1, 2] = z[0, 2, 2] = 1.0          # a tie in time in column 2 ...
    z[0, 0, 0] = 1.0                       # ... and with column 0 in class
    r = R.pooled_cls_loss(z, np.array([0]), R.MAX, R.CE)
    assert r["arg"][0, 2] == 1 and r["correct"][0] == 1.0
    assert np.count_nonzero(r["dz"][0, :, 2]) == 1 and r["dz"][0, 1, 2] != 0


def test_every_gpu_operator_case_has_a_clear_top1():
    """the seeded cases of tests/test_gpu_pretrain.py: the float64 top-2 margin of every row exceeds 1e-3 and no column has two equal
    maxima in time, so indices and `correct` cannot depend on rounding.  No case is excluded."""
    for dim, want in ((0, {1, 3, 257}), (1, {1, 2, 5}), (2, {1, 7, 63, 64, 65, 527, 1000, 1025})):
        assert {s[dim] for s in P.SHAPES} == want
    assert {(1, 527), (2, 1000)} <= {(t, c) for _, t, c in P.SHAPES} and (257, 2, 1000) in P.SHAPES and (1, 1, 1) in P.SHAPES
    for B, T, C in P.SHAPES:
        for mode in (R.MAX, R.MEAN):
            for kind in (R.CE, R.BCE):
                z, target = P.make_case(B, T, C, mode, kind)
                assert P.top2_margin(R.tpool_fwd(z, mode)[0]) > P.MARGIN, (B, T, C, mode, kind)
                if T > 1 and mode == R.MAX:
                    s = np.sort(z, axis=1)
                    assert not (s[:, -1] == s[:, -2]).any(), (B, T, C, mode, kind)
                if kind == R.CE:
                    assert 0 < R.cls_loss(R.tpool_fwd(z, mode)[0], target, kind)[1] or B == 1


def test_library_rejects_bad_arguments_without_a_device():
    """B, T, C >= 1, a known mode and kind, non-null buffers: anything else is M3T_EINVAL before a launch"""
    from m3t import _lib
    lib = _lib.load()
    one = 16          # a non-null address that is never dereferenced: every call below fails its argument check first
    assert lib.m3t_tpool_fwd(one, 0, 1, 1, 0, one, one, None) == _lib.M3T_EINVAL
    assert lib.m3t_tpool_fwd(one, 1, 1, 1, 2, one, one, None) == _lib.M3T_EINVAL
    assert lib.m3t_tpool_fwd(one, 1, 1, 1, 0, one, None, None) == _lib.M3T_EINVAL
    assert lib.m3t_tpool_bwd(one, one, 1, 0, 1, 0, one, None) == _lib.M3T_EINVAL
    assert lib.m3t_tpool_bwd(None, one, 1, 1, 1, 0, one, None) == _lib.M3T_EINVAL
    assert lib.m3t_cls_loss(one, 1, 0, 0, one, one, one, one, one, 16, None) == _lib.M3T_EINVAL
    assert lib.m3t_cls_loss(one, 1, 1, 2, one, one, one, one, one, 16, None) == _lib.M3T_EINVAL
    assert lib.m3t_cls_loss(one, 2, 1, 0, one, one, one, one, one, 16, None) == _lib.M3T_EINVAL          # workspace too small
    assert lib.m3t_tpool_cls_loss(one, 1, 1, 1, 0, 0, one, one, None, one, one, one, one, 16, None) == _lib.M3T_EINVAL
    assert lib.m3t_tpool_cls_loss(one, 1, 1, -1, 0, 0, one, one, one, one, one, one, one, 16, None) == _lib.M3T_EINVAL
    assert lib.m3t_cls_loss_ws_bytes(3) == 48 and lib.m3t_cls_loss_ws_bytes(0) == 0


# ------------------------------------------------------------------ the CPU path of the ops wrappers
@pytest.mark.parametrize("B,T,C", CASES)
@pytest.mark.parametrize("mode", ["max", "mean"])
@pytest.mark.parametrize("kind", ["ce", "bce"])
def test_ops_cpu_path_agrees_with_restatement(B, T, C, mode, kind):
    from m3t import ops
    rs = np.random.RandomState(7 + 100 * B + 10 * T + C)
    z = (rs.standard_normal((B, T, C)) * 3).astype(np.float32)
    target = rs.randint(0, C, (B,)).astype(np.int64) if kind == "ce" else (rs.uniform(size=(B, C)) < 0.3).astype(np.float32)
    r = R.pooled_cls_loss(z, target, ops.POOL_MODES[mode], ops.LOSS_KINDS[kind])
    tt = torch.from_numpy(target)
    # fused entry point
    zt = torch.from_numpy(z).requires_grad_(True)
    loss, stats, correct, pooled, arg = ops.pooled_cls_loss(zt, tt, mode, kind, return_pooled=True)
    loss.backward()
    assert _rel(pooled, r["pooled"]) < 1e-6 and abs(float(loss) - r["loss"]) < 1e-5 * max(1.0, abs(r["loss"]))
    assert _rel(zt.grad, r["dz"]) < 1e-6
    assert stats.shape == (2,) and float(stats[0]) == float(loss) and float(stats[1]) == r["n_correct"]
    np.testing.assert_array_equal(correct.numpy(), r["correct"])
    if mode == "max":
        np.testing.assert_array_equal(arg.numpy(), r["arg"])
    # two steps
    z2 = torch.from_numpy(z).requires_grad_(True)
    loss2, stats2, correct2 = ops.cls_loss(ops.temporal_pool(z2, mode), tt, kind)
    loss2.backward()
    assert float(loss2) == float(loss) and torch.equal(z2.grad, zt.grad) and torch.equal(correct2, correct) and torch.equal(stats2, stats)
    assert not stats.requires_grad and not correct.requires_grad


def test_ops_reject_bad_shapes():
    from m3t import ops
    with pytest.raises(ValueError):
        ops.cls_loss(torch.zeros(2, 4, 10), torch.zeros(2, dtype=torch.int64), "ce")       # per-frame logits: the reference's own failure
    with pytest.raises(ValueError):
        ops.cls_loss(torch.zeros(2, 10), torch.zeros(2, 9), "bce")
    with pytest.raises(ValueError):
        ops.temporal_pool(torch.zeros(2, 10), "max")
    with pytest.raises(KeyError):
        ops.temporal_pool(torch.zeros(2, 3, 10), "median")


# ------------------------------------------------------------------ VoxCeleb2_1k on the CPU path against the reference's run
def _vox(g):
    from golden.recipe import fill_module
    cls = _modules()["vox"]
    B, T, S = [int(v) for v in g["dims"]]
    m = fill_module(cls(_hp(cls, window=T)), int(g["seed"]) + 1)
    m = m.train() if int(g["training"]) else m.eval()
    rs = np.random.RandomState(int(g["seed"]))
    x = torch.from_numpy(rs.randint(0, 256, (B, 3, T, S, S)).astype(np.float32))
    return m, {"video": x, "label": torch.from_numpy(g["label"])}


@pytest.mark.parametrize("name", ["vox2_eval", "vox2_train"])
def test_vox_cpu_step_matches_reference(name):
    from golden.recipe import grad_digest
    g = load_golden(name)
    m, batch = _vox(g)
    with torch.no_grad():
        y = copy.deepcopy(m)(batch["video"])        # (a copy: a train-mode forward moves the BatchNorm buffers)
    assert _rel(y, g["y"]) <= 1e-5
    out = m.training_step(batch, 0)
    assert set(out) == {"loss", "progress_bar", "log"} and set(out["log"]) == {"loss", "train_acc"} == set(out["progress_bar"])
    assert abs(float(out["loss"]) - float(g["loss"])) <= 1e-5 * max(1.0, abs(float(g["loss"])))
    assert float(out["log"]["train_acc"]) == float(g["train_acc"])
    out["loss"].backward()
    n = 0
    for pn, p in m.named_parameters():
        ref = g["gd." + pn]
        assert float(np.abs(grad_digest(p.grad.numpy()) - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max())), pn
        n += 1
    assert n == len([k for k in g if k.startswith("gd.")])
    if int(g["training"]):
        nb = 0
        for bn_name, b in m.named_buffers():
            leaf = bn_name.split(".")[-1]
            if leaf == "num_batches_tracked":
                assert int(b) == int(g["bn." + bn_name]), bn_name
            else:
                assert _rel(b, g["bn." + bn_name]) <= 1e-5, bn_name
            nb += 1
        assert nb == 3 * 5
    else:
        val = m.validation_step(batch, 0)
        assert set(val) == {"val_loss", "correct"}
        assert abs(float(val["val_loss"]) - float(g["val_loss"])) <= 1e-5 * max(1.0, abs(float(g["val_loss"])))
        np.testing.assert_array_equal(val["correct"].float().numpy(), g["correct"])
        assert float(m.ce_loss(m(batch["video"]), batch["label"])) == pytest.approx(float(g["loss"]), rel=1e-5)
