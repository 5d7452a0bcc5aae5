"""Cached weight magnitudes (m3t.ops.weight_amax / _frozen_weight_amax) after writes that ._version does not see (GPU).

The fp16x3 contractions scale each operand by a power of two taken from its max |x| (csrc/common.h m3t_f16_scale), and under no_grad
a weight matrix is measured once and its slot reused.  A weight written afterwards through a raw pointer (FlatAdam / FlatSGD), through
FlatGradDDP.flat_params, or through .data keeps its ._version: without the weight generation (ops.weights_changed) the next forward
scales by the old maximum -- wrong in the last bits, or inf once the weight outgrew the fp16 range of its old scale.

Invariant: after a write, the next no_grad forward is bit-identical to the same forward with every magnitude cache emptied (a fresh
measurement of the same weights gives the same slot), finite, and within 1e-5 of an fp64 restatement."""
import argparse
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class _Stack(torch.nn.Module):
    """three weight matrices through ops.linear (ReLU epilogue between them) at shapes that take the fp16x3 path with cached weight
    slots (rows % 128, N % 64, K % 32); the first one starts small so that one optimizer step multiplies its max |w| by more than 8"""

    def __init__(self, d=64, h=128, o=64):
        super().__init__()
        torch.manual_seed(7)
        self.l1, self.l2, self.l3 = torch.nn.Linear(d, h), torch.nn.Linear(h, h), torch.nn.Linear(h, o)
        with torch.no_grad():
            self.l1.weight.mul_(0.05)

    def forward(self, x):
        from m3t import ops
        h = ops.linear(x, self.l1.weight, self.l1.bias, 1)
        h = ops.linear(h, self.l2.weight, self.l2.bias, 1)
        return ops.linear(h, self.l3.weight, self.l3.bias, 0)

    def ref64(self, x):
        p = [t.detach().double().cpu() for t in (self.l1.weight, self.l1.bias, self.l2.weight, self.l2.bias, self.l3.weight, self.l3.bias)]
        h = torch.relu(x.double().cpu() @ p[0].T + p[1])
        h = torch.relu(h @ p[2].T + p[3])
        return h @ p[4].T + p[5]


def _empty_caches():
    from m3t import ops
    ops._W_AMAX_FROZEN.clear()
    ops.drop_weight_amax()


def _forwards(net, x):
    """(a bare ops.linear on l1's weight -- the one an optimizer step grows most --, the whole stack) under no_grad"""
    from m3t import ops
    with torch.no_grad():
        return ops.linear(x, net.l1.weight, None, 0), net(x)


def _check_after_write(net, x, write):
    _forwards(net, x)                       # measures (and caches) every weight of the current state
    torch.cuda.synchronize()
    write()
    got = _forwards(net, x)
    torch.cuda.synchronize()
    _empty_caches()
    fresh = _forwards(net, x)
    for g, f, what in zip(got, fresh, ("linear", "stack")):
        assert torch.isfinite(g).all(), "%s: non-finite output after the write (stale scale)" % what
        assert torch.equal(g, f), "%s: differs from the emptied-cache run by %.3e" % (what, float((g - f).abs().max()))
    y64 = net.ref64(x)
    err = float((got[1].double().cpu() - y64).abs().max())
    assert err <= 1e-5 * max(1.0, float(y64.abs().max())), err


def _x(seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(4, 64, 64, generator=g).to(DEV)


def _train_step(net, ddp, opt, x):
    ddp.zero_grad()
    net(x).square().mean().backward()
    ddp.finish()
    opt.step()


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_flat_optimizer_step_invalidates_cached_scales(kind):
    from m3t.ddp import FlatGradDDP
    from m3t.optim import FlatAdam, FlatSGD
    net = _Stack().to(DEV)
    ddp = FlatGradDDP(net, max_norm=0.0, flatten_params=True)
    opt = FlatAdam(ddp, lr=0.1, weight_decay=0.0) if kind == "adam" else FlatSGD(ddp, lr=20.0, momentum=0.0, weight_decay=0.0)
    x = _x()
    before = float(net.l1.weight.abs().max())
    _check_after_write(net, x, lambda: _train_step(net, ddp, opt, x))
    grown = float(net.l1.weight.abs().max()) / before
    if kind == "adam":
        assert grown >= 8.0, "the step must take the weight far past its fp16 scale range (grew %.1fx)" % grown
    else:
        assert grown != 1.0


def test_in_place_op_on_flat_params():
    from m3t import ops
    from m3t.ddp import FlatGradDDP
    net = _Stack().to(DEV)
    ddp = FlatGradDDP(net, max_norm=0.0, flatten_params=True)

    def write():
        ddp.flat_params.mul_(16)
        ops.invalidate_weight_amax()        # (a flat_params write is a .data write: the caller invalidates)
    _check_after_write(net, _x(), write)


def test_flattening_and_broadcast_state():
    """FlatGradDDP(flatten_params=True) re-points every .data (the weights keep their values: the cache may not misread the new
    storage); broadcast_state at world size 1 writes nothing"""
    from m3t.ddp import FlatGradDDP
    net = _Stack().to(DEV)
    box = []
    _check_after_write(net, _x(), lambda: box.append(FlatGradDDP(net, max_norm=0.0, flatten_params=True)))
    _check_after_write(net, _x(), lambda: box[0].broadcast_state())


def test_dot_data_writes_with_invalidate():
    from m3t import ops
    net = _Stack().to(DEV)
    src = [p.detach().clone() * 3 for p in net.parameters()]

    def copy():
        for p, s in zip(net.parameters(), src):
            p.data.copy_(s)
        ops.invalidate_weight_amax()

    def mul():
        for p in net.parameters():
            p.data.mul_(16)
        ops.invalidate_weight_amax()
    _check_after_write(net, _x(), copy)
    _check_after_write(net, _x(), mul)


def test_trainer_load_checkpoint_invalidates(tmp_path):
    from m3t import ops
    from m3t.trainer import Trainer
    net = _Stack().to(DEV)
    tr = Trainer(net, learning_rate=1e-3)
    orig = tr.ddp.flat_params.clone()
    tr.ddp.flat_params.mul_(16)
    ops.invalidate_weight_amax()
    path = os.path.join(tmp_path, "big.ckpt")
    tr.save_checkpoint(path)
    tr.ddp.flat_params.copy_(orig)
    ops.invalidate_weight_amax()
    _check_after_write(net, _x(), lambda: tr.load_checkpoint(path))
    assert torch.equal(tr.ddp.flat_params, orig * 16)


# ---------------------------------------------------------------------------------------------------------- the Trainer's own flow
def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _audio_batch(B=4, T=40, seed=0):
    rs = np.random.RandomState(seed)
    f = lambda a: torch.from_numpy(a).to(DEV)       # noqa: E731
    audio = rs.standard_normal((B, T, 200)).astype(np.float32)
    val = np.tanh(audio[..., :20].mean(-1) * 3).astype(np.float32)
    aro = np.tanh(audio[..., 20:40].mean(-1) * 3).astype(np.float32)
    return {"audio": f(audio), "label_valence": f(val), "label_arousal": f(aro),
            "class_expr": f(rs.randint(0, 7, (B, T)).astype(np.int64)), "expr_valid": f(rs.uniform(size=(B, T)) < 0.7),
            "vid_name": ["v%d" % (i + B * seed) for i in range(B)], "start": torch.zeros(B, dtype=torch.long),
            "length": torch.full((B,), T, dtype=torch.long)}


def _same(a, b, where=""):
    if torch.is_tensor(a):
        assert torch.equal(a, b), where
        if a.is_floating_point():
            assert torch.isfinite(a).all(), where
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for i, (u, v) in enumerate(zip(a, b)):
            _same(u, v, "%s[%d]" % (where, i))
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), where
        for k in a:
            _same(a[k], b[k], "%s.%s" % (where, k))
    elif isinstance(a, float):
        assert a == b and np.isfinite(a), (where, a, b)
    else:
        assert a == b, where


def _checked_validate(tr, log):
    """Trainer.validate, followed by the same validation with every magnitude cache emptied: predictions and val_loss bit for bit"""
    from m3t import ops
    orig = tr.validate

    def validate(batches):
        tr.model.eval()
        outs = [tr.model.validation_step(b, i) for i, b in enumerate(batches)]
        res = orig(batches)
        _empty_caches()
        outs2 = [tr.model.validation_step(b, i) for i, b in enumerate(batches)]
        res2 = orig(batches)
        _same(outs, outs2, "validation_step")
        _same(float(res["val_loss"]), float(res2["val_loss"]), "val_loss")
        log.append(float(res["val_loss"]))
        return res
    tr.validate = validate
    ops.invalidate_weight_amax()
    return tr


def test_trainer_fit_validation_matches_fresh_measurement(tmp_path, monkeypatch):
    from models.model import AffWild2VA
    from m3t.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(12345)
    model = AffWild2VA(_hp(modality="audio", loss="ccc_mtl", learning_rate=2e-2, window=40)).to(DEV)
    tr = Trainer.from_hparams(model, model.hparams)
    tr.freeze_gc = False
    log = []
    _checked_validate(tr, log)
    batches = [_audio_batch(seed=s) for s in range(3)]
    val = [_audio_batch(seed=10 + s) for s in range(2)]
    w0 = tr.ddp.flat_params.clone()
    tr.fit(batches, val_batches=val, max_epochs=2)
    assert len(log) == 2
    assert float((tr.ddp.flat_params - w0).abs().max()) > 0.05, "the learning rate must move the weights far"
    path = os.path.join(tmp_path, "ck.pt")
    tr.save_checkpoint(path)
    tr.validate(val)
    for b in batches:
        tr.step(b)                              # move the weights on, then go back to the checkpoint
    tr.validate(val)
    tr.load_checkpoint(path)
    tr.validate(val)
    assert log[-1] == log[2], "the reloaded weights must validate as before"


def test_frozen_cache_measures_once_without_a_write(tmp_path, monkeypatch):
    """the cache still works: a second validation with no write in between measures no weight again; a step makes it measure again"""
    from models.model import AffWild2VA
    from m3t import ops
    from m3t.trainer import Trainer
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(3)
    model = AffWild2VA(_hp(modality="audio", loss="ccc_mtl", learning_rate=1e-3, window=40)).to(DEV)
    tr = Trainer.from_hparams(model, model.hparams)
    ptrs = {p.data_ptr() for p in model.parameters()}
    count = [0]
    real = ops.measure_amax

    def counting(items):
        count[0] += sum(1 for t, _ in items if t.data_ptr() in ptrs)
        return real(items)
    monkeypatch.setattr(ops, "measure_amax", counting)
    val = [_audio_batch(seed=20)]
    tr.validate(val)
    first = count[0]
    assert first > 0
    tr.validate(val)
    assert count[0] == first, "a validation with no write in between measured %d weights again" % (count[0] - first)
    tr.step(_audio_batch(seed=21))
    n = count[0]
    tr.validate(val)
    assert count[0] - n == first, "after an optimizer step every weight is measured again (%d of %d)" % (count[0] - n, first)
