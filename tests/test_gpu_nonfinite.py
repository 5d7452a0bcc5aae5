"""NaN / inf inputs through the HIP operators against fp64 references (GPU).

torch.relu, torch.max and max_pool keep a NaN; fmaxf(NaN, 0.f) is 0.  A fused ReLU written with fmaxf turned a NaN into 0 -- with a
training-mode BatchNorm a whole channel of zeros -- so the loss and the gradient norm of a corrupt batch came out finite and the
optimizer's non-finite guard never fired.  Every fused ReLU now uses m3t_relu (csrc/common.h) and the CBAM max reductions let NaN win.

Elementwise and normalisation operators: NaN masks equal, inf masks equal with signs, finite entries within the family's bar.
Contractions: the fp16x3 split turns inf into NaN (inf - inf), so only the non-finite masks are compared; around a ReLU epilogue an
fp64 -inf becomes 0 while the kernel's NaN stays, so the kernel's non-finite mask must lie between the reference's after and before
the activation.  TCN, CBAM and the attention score take NaN only: an inf there meets weights of both signs and the fp64 result
mixes +inf, -inf, 0 and NaN in ways the split does not reproduce."""
import argparse

import numpy as np
import pytest
import torch

from golden.recipe import fill_module, draw
from oracle import m3t_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
NAN, INF = float("nan"), float("inf")


def dev(a, grad=False):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.astype(np.float32) if a.dtype == np.float64 else a).to(DEV)
    return t.requires_grad_(True) if grad else t


def plant(a, spots):
    a = np.array(a, dtype=np.float32)           # (the fp64 references start from the float32 inputs the kernels see)
    for idx, v in spots:
        a[idx] = v
    return a


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(t) else np.asarray(t, dtype=np.float64)


def same_nonfinite(y, ref, tol=TOL, what=""):
    """NaN masks equal, inf masks equal with signs, finite entries close"""
    y, ref = _np(y), _np(ref)
    assert y.shape == ref.shape, (what, y.shape, ref.shape)
    assert np.array_equal(np.isnan(y), np.isnan(ref)), "%s: NaN at %d places, the reference at %d" % (what, np.isnan(y).sum(), np.isnan(ref).sum())
    assert np.array_equal(np.isposinf(y), np.isposinf(ref)) and np.array_equal(np.isneginf(y), np.isneginf(ref)), "%s: inf masks" % what
    fin = np.isfinite(ref)
    assert fin.any(), "%s: nothing finite left to compare" % what
    err = float(np.abs(y[fin] - ref[fin]).max())
    assert err <= tol * max(1.0, float(np.abs(ref[fin]).max())), "%s: finite entries off by %.3e" % (what, err)


def nonfinite_between(y, ref_post, ref_pre=None, what=""):
    """~isfinite(kernel) contains ~isfinite(fp64 after the activation) and lies inside ~isfinite(fp64 before it)"""
    y, post = ~np.isfinite(_np(y)), ~np.isfinite(_np(ref_post))
    pre = post if ref_pre is None else ~np.isfinite(_np(ref_pre))
    assert post.any(), what
    assert not (post & ~y).any(), "%s: %d non-finite reference entries came out finite" % (what, int((post & ~y).sum()))
    assert not (y & ~pre).any(), "%s: %d entries non-finite where the reference is finite" % (what, int((y & ~pre).sum()))


# ---------------------------------------------------------------------------------------------------- elementwise / normalisation
@pytest.mark.parametrize("shape", [(3, 64, 8, 8), (2, 5, 7, 3)])           # float4 body / scalar tail
def test_add_relu(shape):
    from m3t import ops
    rs = np.random.RandomState(1)
    a, b = draw(rs, shape), draw(rs, shape)
    last = tuple(s - 1 for s in shape)
    a = plant(a, [((0, 0, 0, 0), NAN), ((0, 1, 0, 1), INF), ((0, 2, 1, 0), -INF), (last, NAN), ((shape[0] - 1, 1, 1, 1), INF)])
    b = plant(b, [((0, 1, 0, 2), NAN), ((shape[0] - 1, 1, 1, 1), -INF), ((0, 3, 2, 2), INF)])
    y = ops.add_relu(dev(a), dev(b))
    ref = torch.relu(torch.from_numpy(a).double() + torch.from_numpy(b).double())
    same_nonfinite(y, ref, 1e-6, "add_relu")


def _bn_pair(mod, ref, C_, rs):
    with torch.no_grad():
        for p_, q_ in ((mod.weight, ref.weight), (mod.bias, ref.bias), (mod.running_mean, ref.running_mean), (mod.running_var, ref.running_var)):
            v = rs.uniform(0.5, 1.5, C_) if p_ is mod.weight or p_ is mod.running_var else rs.uniform(-0.5, 0.5, C_)
            p_.copy_(torch.from_numpy(v.astype(np.float32)))
            q_.copy_(torch.from_numpy(v.astype(np.float32)).double())


def _spots(shape, C_):
    """NaN / +inf / -inf in separate channels, in the first and the last frames"""
    n1 = shape[0] - 1
    rest = tuple(s - 1 for s in shape[2:])
    zero = tuple(0 for _ in shape[2:])
    return [((0, 0) + zero, NAN), ((n1, C_ - 1) + rest, NAN), ((0, 2) + rest, INF), ((n1, C_ - 2) + zero, -INF)]


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("N,C_,T,H,W", [(3, 16, 5, 7, 9), (2, 64, 4, 12, 12)])
def test_batchnorm3d_relu_planes(N, C_, T, H, W, training):
    from models.backbone import BatchNorm3dReLU
    rs = np.random.RandomState(C_ + H)
    m, ref = BatchNorm3dReLU(C_).to(DEV), torch.nn.BatchNorm3d(C_).double()
    _bn_pair(m, ref, C_, rs)
    m.train(training); ref.train(training)
    xn = plant(draw(rs, (N, C_, T, H, W)), _spots((N, C_, T, H, W), C_))
    with torch.no_grad():
        y = m(dev(xn))
        y64 = torch.relu(ref(torch.from_numpy(xn).double()))
    if training:
        assert torch.isnan(y64[:, 0]).all()
    same_nonfinite(y, y64, TOL, "BatchNorm3dReLU")


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("N,C_,H,W", [(37, 64, 28, 28), (19, 256, 7, 7), (9, 16, 4, 4)])
def test_plane_batchnorm2d_relu(N, C_, H, W, training):
    from models.resnet import PlaneBatchNorm2d
    rs = np.random.RandomState(N + C_)
    m, ref = PlaneBatchNorm2d(C_, fuse_relu=True).to(DEV), torch.nn.BatchNorm2d(C_).double()
    _bn_pair(m, ref, C_, rs)
    m.train(training); ref.train(training)
    xn = plant(draw(rs, (N, C_, H, W)), _spots((N, C_, H, W), C_))
    with torch.no_grad():
        y = m(dev(xn))
        y64 = torch.relu(ref(torch.from_numpy(xn).double()))
    same_nonfinite(y, y64, TOL, "PlaneBatchNorm2d")


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("training", [True, False])
def test_channels_last_bn_relu_and_pool(training, fused):
    """ops.bn_cl (+ReLU) on rows [N T H W][C], and with lazy=True the BatchNorm + ReLU applied inside the (1, 2, 2) max pooling"""
    from m3t import ops
    F = torch.nn.functional
    N, C_, T, H, W = 3, 64, 2, 8, 6
    rs = np.random.RandomState(5)
    xn = plant(draw(rs, (N, C_, T, H, W)) * 2.0 + 0.3, _spots((N, C_, T, H, W), C_))
    gam, bet = plant(1.0 + 0.1 * draw(rs, (C_,)), []), plant(0.1 * draw(rs, (C_,)), [])
    rm, rv = plant(0.1 * draw(rs, (C_,)), []), plant(np.abs(draw(rs, (C_,))) * 0.5 + 0.5, [])
    to_cl = lambda a: np.ascontiguousarray(np.transpose(a, (0, 2, 3, 4, 1))).reshape(-1, a.shape[1])      # noqa: E731
    with torch.no_grad():
        xc = ops.CLTensor(dev(to_cl(xn)), N, T, H, W, None)
        y = ops.bn_cl(xc, dev(gam), dev(bet), dev(rm.copy()), dev(rv.copy()), training, 0.1, 1e-5, True, lazy=fused)
        z = ops.pool_cl(y, (2, 2), (2, 2), (0, 0)) if fused else None
        if fused:
            assert y._pending is not None, "the pooling did not take the fused operator"
        d = lambda a: torch.from_numpy(a).double()      # noqa: E731
        y64 = torch.relu(F.batch_norm(d(xn), d(rm.copy()), d(rv.copy()), d(gam), d(bet), training, 0.1, 1e-5))
    if fused:
        z64 = F.max_pool3d(y64, (1, 2, 2), (1, 2, 2))
        same_nonfinite(z.data, to_cl(z64.numpy()), TOL, "bn_cl + pool_cl")
    else:
        same_nonfinite(y.data, to_cl(y64.numpy()), TOL, "bn_cl")


# ---------------------------------------------------------------------------------------------------------------- contractions
@pytest.mark.parametrize("mode", ["fp32", "x6", "high"])
@pytest.mark.parametrize("M,K,N", [(200, 64, 96), (1000, 256, 512)])
def test_linear_relu_epilogue(mode, M, K, N):
    from m3t import ops
    rs = np.random.RandomState(M + K)
    xn = plant(draw(rs, (M, K)), [((0, 3), NAN), ((1, 0), INF), ((2, K - 1), -INF), ((M - 1, K - 1), NAN), ((M - 2, 5), INF)])
    wn, bn = plant(draw(rs, (N, K)) / np.sqrt(K), []), plant(draw(rs, (N,)), [])
    pre = torch.from_numpy(xn).double() @ torch.from_numpy(wn).double().T + torch.from_numpy(bn).double()
    with ops.precision(mode), torch.no_grad():
        y1 = ops.linear(dev(xn), dev(wn), dev(bn), 1)
        y0 = ops.linear(dev(xn), dev(wn), dev(bn), 0)
    nonfinite_between(y1, torch.relu(pre), pre, "linear+relu")
    nonfinite_between(y0, pre, None, "linear")


@pytest.mark.parametrize("mode", ["fp32", "x6", "high"])
@pytest.mark.parametrize("M,N,K", [(64, 64, 32), (384, 256, 128), (2048, 512, 256)])
def test_sgemm_relu_epilogue(mode, M, N, K):
    """m3t_sgemm C = relu(A B^T + bias): NaN / inf in rows of A in the first and the last row tile"""
    from m3t import ops
    rs = np.random.RandomState(M + N)
    an = plant(draw(rs, (M, K)), [((0, 0), NAN), ((1, K - 1), INF), ((M - 1, 1), NAN), ((M - 3, 0), -INF)])
    bn, bias = plant(draw(rs, (N, K)) / np.sqrt(K), []), plant(draw(rs, (N,)), [])
    pre = torch.from_numpy(an).double() @ torch.from_numpy(bn).double().T + torch.from_numpy(bias).double()
    c = torch.empty(M, N, device=DEV)
    with ops.precision(mode):
        ops.sgemm(0, 1, M, N, K, dev(an), 0, K, dev(bn), 0, K, c, 0, N, bias=dev(bias), act=1)
    nonfinite_between(c, torch.relu(pre), pre, "sgemm+relu")


@pytest.mark.parametrize("C_in,widths,B,T", [(16, [32, 32], 2, 40), (128, [512, 512], 3, 100)])    # fp32-MFMA conv / bf16x6 implicit GEMM
def test_temporal_blocks(C_in, widths, B, T):
    """TemporalConvNet eval: conv1 with the act-1 epilogue, conv2 with act 2 (ReLU, + residual, ReLU) -- NaN in the first and the last clip"""
    from models.tcn import TemporalConvNet
    rs = np.random.RandomState(C_in)
    m = fill_module(TemporalConvNet(C_in, widths, 3), 12).to(DEV).eval()
    xn = plant(draw(rs, (B, C_in, T)), [((0, 0, 3), NAN), ((B - 1, C_in - 1, T - 1), NAN), ((B - 1, 2, T // 2), NAN)])
    p = {n: t.detach().cpu().numpy().astype(np.float64) for n, t in m.named_parameters()}
    y_ref, _ = O.tcn_fwd(xn.astype(np.float64), p, 2)
    with torch.no_grad():
        y = m(dev(xn))
    assert np.isnan(y_ref[0]).any() and np.isfinite(y_ref[0, :, :3]).all()
    nonfinite_between(y, y_ref, None, "tcn")


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("C_,H,W,N", [(64, 8, 8, 4), (32, 9, 5, 3)])
def test_cbam(C_, H, W, N, training, fused):
    """the channel gate's MLP ReLU and max over each plane, the spatial gate's max over channels (fused operator and the two gates)"""
    from models.cbam import CBAM
    from m3t import ops
    rs = np.random.RandomState(C_ + H)
    m = fill_module(CBAM(C_), 77).to(DEV).train(training)
    p = {n: t.detach().cpu().numpy().astype(np.float64) for n, t in list(m.named_parameters()) + list(m.named_buffers()) if t.dtype.is_floating_point}
    xn = plant(draw(rs, (N, C_, H, W)), [((0, 0, 0, 0), NAN), ((N - 1, C_ - 1, H - 1, W - 1), NAN)])
    y_ref, _, _ = O.cbam_fwd(xn.astype(np.float64), p, training)
    saved = ops.CBAM_FUSED[0]
    ops.CBAM_FUSED[0] = fused
    try:
        with torch.no_grad():
            y = m(dev(xn))
    finally:
        ops.CBAM_FUSED[0] = saved
    if not training:
        assert np.isfinite(y_ref[1:N - 1]).all()
    nonfinite_between(y, y_ref, None, "cbam")


def test_attention_weights_of_the_decoder():
    """ops.attention_weights: softmax_tau(v . relu(W_a [h; enc_tau] + b_a)); a NaN in one frame of a clip makes the clip's weights NaN"""
    from m3t import ops
    rs = np.random.RandomState(9)
    B, T, H = 4, 37, 128
    hn, en = draw(rs, (B, H)), draw(rs, (B, T, H))
    en = plant(en, [((0, 0, 0), NAN), ((B - 1, T - 1, H - 1), NAN)])
    hn = plant(hn, [((2, 5), NAN)])
    wa, ba, vv = plant(draw(rs, (H, 2 * H)) / np.sqrt(2 * H), []), plant(draw(rs, (H,)), []), plant(draw(rs, (H,)), [])
    with torch.no_grad():
        alpha = ops.attention_weights(dev(hn), dev(en), dev(wa), dev(ba), dev(vv))
    d = lambda a: torch.from_numpy(a).double()      # noqa: E731
    cat = torch.cat([d(hn)[:, None, :].expand(B, T, H), d(en)], -1)
    ref = torch.softmax(torch.relu(cat @ d(wa).T + d(ba)) @ d(vv), -1)
    assert torch.isnan(ref[0]).all() and torch.isfinite(ref[1]).all()
    same_nonfinite(alpha, ref, 1e-5, "attention weights")


# ---------------------------------------------------------------------------------------------------------------- controls
def test_bigru_and_va_loss_propagate_nan():
    from models.rnn import GRU
    from m3t import ops
    torch.manual_seed(4)
    g = GRU(12, 16, 2, 3, 2).to(DEV).eval()
    rs = np.random.RandomState(2)
    xn = plant(draw(rs, (4, 9, 12)), [((1, 5, 3), NAN)])
    with torch.no_grad():
        y = g(dev(xn))
    bad = ~torch.isfinite(y).cpu()
    assert bad[1].all() and not bad[[0, 2, 3]].any(), "a bidirectional scan spreads a NaN over exactly its own clip"
    B, T = 3, 20
    yn = plant(draw(rs, (B, T, 9)), [((1, 4, 7), NAN)])
    val, aro = draw(rs, (B, T), "uniform_pm1"), draw(rs, (B, T), "uniform_pm1")
    expr = rs.randint(0, 7, (B, T)).astype(np.int64)
    valid = np.ones((B, T), dtype=bool)
    loss, _ = ops.va_loss(dev(yn), dev(val), dev(aro), dev(expr), dev(valid), iv=7, ia=8, n_expr=7)
    l_ref, _, _ = O.training_loss_fwd_bwd(yn.astype(np.float64), val.astype(np.float64), aro.astype(np.float64), expr, valid)
    assert not np.isfinite(l_ref)
    assert not torch.isfinite(loss).item()


# ---------------------------------------------------------------------------------------------------------------- end to end
def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _audio_batch(B=4, T=40, seed=0, nan_at=None):
    rs = np.random.RandomState(seed)
    f = lambda a: torch.from_numpy(a).to(DEV)       # noqa: E731
    audio = rs.standard_normal((B, T, 200)).astype(np.float32)
    val = np.tanh(audio[..., :20].mean(-1) * 3).astype(np.float32)
    aro = np.tanh(audio[..., 20:40].mean(-1) * 3).astype(np.float32)
    if nan_at is not None:
        audio[nan_at] = np.nan
    return {"audio": f(audio), "label_valence": f(val), "label_arousal": f(aro),
            "class_expr": f(rs.randint(0, 7, (B, T)).astype(np.int64)), "expr_valid": f(rs.uniform(size=(B, T)) < 0.7),
            "vid_name": ["v%d" % i for i in range(B)], "start": torch.zeros(B, dtype=torch.long),
            "length": torch.full((B,), T, dtype=torch.long)}


def test_audio_model_with_one_nan_feature():
    """C1 (audio): eval output non-finite over exactly the clip that holds the NaN (its BiGRU spans the clip), training_step's loss
    non-finite; through Trainer.step the gradient norm is non-finite and FlatAdam changes neither the weights nor m and v"""
    from models.model import AffWild2VA
    from m3t.trainer import Trainer
    torch.manual_seed(12345)
    model = AffWild2VA(_hp(modality="audio", loss="ccc_mtl", learning_rate=1e-3)).to(DEV)
    tr = Trainer.from_hparams(model, model.hparams)
    tr.freeze_gc = False
    tr.step(_audio_batch(seed=1))                   # a clean step first: m and v are not zero
    bad = _audio_batch(seed=2, nan_at=(2, 17, 33))
    model.eval()
    with torch.no_grad():
        y = model(bad)
    nf = ~torch.isfinite(y).cpu()
    assert nf[2].any() and not nf[[0, 1, 3]].any()
    assert nf[2].reshape(nf.shape[1], -1).any(-1).all()
    model.train()
    out = model.training_step(bad, 0)
    assert not torch.isfinite(out["loss"]).item()
    params, m, v = tr.ddp.flat_params.clone(), tr.opt.m.clone(), tr.opt.v.clone()
    out = tr.step(bad)
    torch.cuda.synchronize()
    assert not torch.isfinite(out["loss"]).item()
    assert not np.isfinite(float(out["grad_norm"]))
    assert torch.equal(tr.ddp.flat_params, params) and torch.equal(tr.opt.m, m) and torch.equal(tr.opt.v, v)
