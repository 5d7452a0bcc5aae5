"""`--backbone densenet` on the MI355X: VA_3DDenseNet end to end against the reference's own runs (tests/golden/densenet_*.npz), the
properties of the one-operator feature stack (no stock operator, bit-identical reruns, one path whatever the grad mode, NaN propagation, weight
writes by the flat optimizer) and every entry point of csrc/dense.hip against an fp64 torch restatement at awkward shapes."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from golden.recipe import fill_module, grad_digest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(a, b, tol, what):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max())
    assert err <= tol * max(1.0, float(np.abs(b).max())), "%s: max abs err %.3e" % (what, err)


def _digest_ok(grad, ref, tol, what):
    got = grad_digest(grad.detach().cpu().numpy())
    assert abs(got[0] - ref[0]) <= tol * max(1.0, ref[0]), (what, got[0], ref[0])
    scale = max(1.0, float(np.abs(ref[2:]).max()))
    assert float(np.abs(got[2:] - ref[2:]).max()) <= tol * scale, (what, got[2:], ref[2:])


def _model(seed, T, backend="gru", agg="ap", training=False):
    from models.backbone import VA_3DDenseNet
    m = fill_module(VA_3DDenseNet(frameLen=T, backend=backend, nClasses=2, nFCs=2, frontend_agg_mode=agg), seed + 1).to(DEV)
    return m.train() if training else m.eval()


def _video(seed, B, T, S):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.randint(0, 256, (B, 3, T, S, S)).astype(np.float32)).to(DEV)
    return (x - 127.5) / 127.5


# gradient-digest bars: 2e-3 as the ResNet3D goldens; densenet_feats (backend 'none': 392 random output weights per frame, train mode) is
# conditioned worse -- the reference's own float32 run differs from its float64 run by up to 5.0e-3 in these digests (measured on CPU: norm2 of
# denseblock2.denselayer4, 3.3e-3 for c3d.0.weight), so the fixture carries that much fp32 rounding itself
DIGEST_TOL = {"densenet_feats": 1e-2}


@pytest.mark.parametrize("name", ["densenet_eval", "densenet_train", "densenet_small_train", "densenet_feats", "densenet_fc"])
def test_densenet_golden(name):
    g = load_golden(name)
    seed = int(g["seed"])
    B, T, S = [int(v) for v in g["dims"]]
    training = bool(int(g["training"]))
    m = _model(seed, T, str(g["backend"]), str(g["agg"]), training)
    x = _video(seed, B, T, S).requires_grad_(True)
    y = m(x)
    _close(y, g["y"], 2e-4, "y")
    (y * torch.from_numpy(g["ct"]).to(DEV)).sum().backward()
    names = sorted(n for n, p in m.named_parameters() if p.grad is not None)
    assert names == sorted(k[3:] for k in g if k.startswith("gd."))
    for n, p in m.named_parameters():
        if p.grad is not None:
            _digest_ok(p.grad, g["gd." + n], DIGEST_TOL.get(name, 2e-3), n)
    _digest_ok(x.grad, g["dx"], DIGEST_TOL.get(name, 2e-3), "dx")
    if training:
        n_checked = 0
        for n, b in m.named_buffers():
            leaf = n.split(".")[-1]
            if leaf == "num_batches_tracked":
                assert int(b) == int(g["bn." + n]), n
            elif leaf in ("running_mean", "running_var"):
                _close(b, g["bn." + n], 2e-4, n)
            else:
                continue
            n_checked += 1
        assert n_checked == 3 * 53


def _step(m, x, ct):
    y = m(x)
    (y * ct).sum().backward()
    torch.cuda.synchronize()
    return y.detach()


def test_training_step_takes_no_stock_operator():
    from m3t import ops
    m = _model(5, 4, training=True)
    x = _video(6, 2, 4, 112)
    before = dict(ops.STOCK_FALLBACKS)
    _step(m, x, torch.ones(2, 4, 2, device=DEV))
    assert {k: v for k, v in ops.STOCK_FALLBACKS.items() if v != before.get(k, 0)} == {}


def test_two_identical_steps_are_bit_identical():
    m1 = _model(7, 3, training=True)
    m2 = copy.deepcopy(m1)
    x = _video(8, 2, 3, 80)
    ct = torch.randn(2, 3, 2, generator=torch.Generator().manual_seed(1)).to(DEV)
    y1, y2 = _step(m1, x, ct), _step(m2, x, ct)
    assert torch.equal(y1, y2)
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        if p1.grad is None:                 # (densenet.fc: agg_mode 'fc' only)
            assert p2.grad is None and n.startswith("densenet.fc."), n
            continue
        assert torch.equal(p1.grad, p2.grad), n
    for (n, b1), b2 in zip(m1.named_buffers(), m2.buffers()):
        assert torch.equal(b1, b2), n


def test_no_grad_eval_equals_grad_mode_eval():
    m = _model(9, 3)
    x = _video(10, 2, 3, 80)
    with torch.no_grad():
        a = m(x)
    b = m(x)
    assert torch.equal(a, b.detach())


def test_nan_in_one_frame_reaches_the_output():
    m = _model(11, 4)
    x = _video(12, 2, 4, 80)
    x[1, :, 2, 10, 10] = float("nan")
    with torch.no_grad():
        y = m(x)
    assert torch.isnan(y[1]).any(), "a NaN frame was zeroed on its way to the output"
    assert not torch.isnan(y[0]).any()


def test_flat_adam_step_then_forward_matches_emptied_caches():
    from m3t import ops
    from m3t.ddp import FlatGradDDP
    from m3t.optim import FlatAdam
    m = _model(13, 3, training=True)
    ddp = FlatGradDDP(m, max_norm=0.0, flatten_params=True)
    opt = FlatAdam(ddp, lr=0.1, weight_decay=0.0)
    x = _video(14, 2, 3, 80)
    ddp.zero_grad()
    (m(x) * torch.ones(2, 3, 2, device=DEV)).sum().backward()
    ddp.finish()
    opt.step()
    m.eval()
    with torch.no_grad():
        got = m(x)
    torch.cuda.synchronize()
    ops._W_AMAX_FROZEN.clear()
    ops.drop_weight_amax()
    with torch.no_grad():
        fresh = m(x)
    assert torch.isfinite(got).all()
    assert torch.equal(got, fresh)


# ------------------------------------------------------------------------------------------- entry points against fp64 restatements
def _lib():
    from m3t import _lib as L
    return L, L.load()


def _p(t, off=0):
    return t.data_ptr() + 4 * off


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bn_ref(x64, mean, var, gamma, beta, eps=1e-5):
    return torch.relu((x64 - mean) / torch.sqrt(var + eps) * gamma + beta)


@pytest.mark.parametrize("C,rows", [(200, 300), (144, 131), (32, 97), (392, 18)])
def test_stats_bn_relu_forward_and_backward(C, rows):
    """a strided column prefix (ld = C + 24, as a dense block's buffer), C % 32 in {0, 8, 16}, ragged row counts"""
    L, lib = _lib()
    g = torch.Generator().manual_seed(C + rows)
    ld = C + 24
    buf = (torch.randn(rows, ld, generator=g) * 2 + 0.5).to(DEV)
    x = buf[:, :C]
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    mean, var = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    ws = torch.empty(int(lib.m3t_dense_stats_ws_bytes(rows, C)) // 4 + 2 * C + 2, device=DEV)
    L.check(lib.m3t_dense_col_stats(_p(buf), rows, ld, C, _p(mean), _p(var), _p(ws), ws.numel() * 4, _stream()), "stats")
    x64 = x.double()
    _close(mean, x64.mean(0), 1e-6, "mean")
    _close(var, x64.var(0, unbiased=False), 1e-5, "var")
    y = torch.empty(rows, C, device=DEV)
    L.check(lib.m3t_dense_bn_relu_fwd(_p(buf), ld, rows, C, _p(mean), _p(var), _p(gamma), _p(beta), 1e-5, _p(y), C, _stream()), "fwd")
    _close(y, _bn_ref(x64, x64.mean(0), x64.var(0, unbiased=False), gamma.double(), beta.double()), 1e-5, "y")
    rm, rv = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    L.check(lib.m3t_dense_bn_running(_p(mean), _p(var), rows, C, _p(rm), _p(rv), 0.1, _stream()), "running")
    _close(rm, 0.1 * x64.mean(0), 1e-6, "running_mean")
    _close(rv, 0.9 + 0.1 * x64.var(0, unbiased=True), 1e-5, "running_var")
    dy = torch.randn(rows, C, generator=g).to(DEV)
    for training in (1, 0):
        xr = x64.clone().requires_grad_(True)
        gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        if training:
            yr = _bn_ref(xr, xr.mean(0), xr.var(0, unbiased=False), gr, br)
        else:
            yr = _bn_ref(xr, mean.double(), var.double(), gr, br)
        (yr * dy.double()).sum().backward()
        dbuf = torch.full((rows, ld), 0.25, device=DEV)
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        L.check(lib.m3t_dense_bn_relu_bwd(_p(dy), C, _p(buf), ld, rows, C, _p(mean), _p(var), _p(gamma), _p(beta), 1e-5, training, _p(dbuf), ld,
                                          1, _p(dg), _p(db), _p(ws), ws.numel() * 4, _stream()), "bwd")
        _close(dbuf[:, :C], xr.grad + 0.25, 1e-5, "dx (accumulated) training=%d" % training)
        assert torch.equal(dbuf[:, C:], torch.full((rows, ld - C), 0.25, device=DEV)), "columns past C written"
        _close(dg, gr.grad, 1e-4, "dgamma")
        _close(db, br.grad, 1e-4, "dbeta")


@pytest.mark.parametrize("H,W", [(7, 7), (5, 6), (2, 3)])
def test_transition_pool_and_spread(H, W):
    """BatchNorm + ReLU + AvgPool3d((1, 2, 2)) floor mode: 7 -> 3, odd widths"""
    L, lib = _lib()
    P, C, ld = 3, 200, 232
    g = torch.Generator().manual_seed(H * 10 + W)
    buf = torch.randn(P * H * W, ld, generator=g).to(DEV)
    mean, var = torch.randn(C, generator=g).to(DEV) * 0.1, torch.rand(C, generator=g).to(DEV) + 0.5
    gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV) * 0.1
    y = torch.empty(P * (H // 2) * (W // 2), C, device=DEV)
    L.check(lib.m3t_dense_pool_fwd(_p(buf), ld, P, H, W, C, _p(mean), _p(var), _p(gamma), _p(beta), 1e-5, _p(y), _stream()), "pool")
    a = _bn_ref(buf[:, :C].double(), mean.double(), var.double(), gamma.double(), beta.double())
    ref = F.avg_pool2d(a.view(P, H, W, C).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(-1, C)
    _close(y, ref, 1e-5, "pooled")
    dy = torch.randn(y.shape, generator=g).to(DEV)
    d = torch.empty(P * H * W, C, device=DEV)
    L.check(lib.m3t_dense_pool_spread(_p(dy), P, H, W, C, _p(d), _stream()), "spread")
    t = torch.zeros(P, C, H, W, dtype=torch.float64, requires_grad=True)
    (F.avg_pool2d(t, 2) * dy.double().cpu().view(P, H // 2, W // 2, C).permute(0, 3, 1, 2)).sum().backward()
    _close(d, t.grad.permute(0, 2, 3, 1).reshape(-1, C), 1e-6, "spread")


@pytest.mark.parametrize("mode", [0, 1])
def test_norm5_mean_and_spread(mode):
    L, lib = _lib()
    P, HW, C, ld = 5, 9, 392, 400
    g = torch.Generator().manual_seed(mode)
    buf = torch.randn(P * HW, ld, generator=g).to(DEV)
    mean, var = torch.randn(C, generator=g).to(DEV) * 0.1, torch.rand(C, generator=g).to(DEV) + 0.5
    gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV) * 0.1
    y = torch.empty(P, C * (HW if mode else 1), device=DEV)
    L.check(lib.m3t_dense_mean_fwd(_p(buf), ld, P, HW, C, _p(mean), _p(var), _p(gamma), _p(beta), 1e-5, mode, _p(y), _stream()), "mean")
    a = _bn_ref(buf[:, :C].double(), mean.double(), var.double(), gamma.double(), beta.double()).view(P, HW, C)
    ref = a.permute(0, 2, 1).reshape(P, C * HW) if mode else a.mean(1)
    _close(y, ref, 1e-5, "y")
    dy = torch.randn(y.shape, generator=g).to(DEV)
    d = torch.empty(P * HW, C, device=DEV)
    L.check(lib.m3t_dense_mean_spread(_p(dy), P, HW, C, mode, _p(d), _stream()), "spread")
    refd = dy.double().view(P, C, HW).permute(0, 2, 1) if mode else (dy.double() / HW).view(P, 1, C).expand(P, HW, C)
    _close(d, refd.reshape(P * HW, C), 1e-6, "spread")


@pytest.mark.parametrize("grid", [(1, 3, 5, 7), (2, 2, 3, 3)])
def test_conv333_forward_data_and_weight_gradient(grid):
    """Co = 32 written into columns [40, 72) of a 104-wide buffer; the data gradient (Ci = 32 -> 128) read from those strided columns; row
    counts 105 and 36 (not multiples of 128)"""
    L, lib = _lib()
    N, T, H, W = grid
    rows = N * T * H * W
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, 128, generator=g).to(DEV)
    w = (torch.randn(32, 128, 3, 3, 3, generator=g) / 60).to(DEV)
    ld, off = 104, 40
    buf = torch.full((rows, ld), 3.0, device=DEV)
    wimg = w.permute(2, 3, 4, 1, 0).reshape(27, 128, 32).contiguous()
    L.check(lib.m3t_dense_conv333(_p(x), 128, N, T, H, W, 128, _p(wimg), _p(buf, off), ld, 32, 0, _stream()), "fwd")
    xp = x.double().view(N, T, H, W, 128).permute(0, 4, 1, 2, 3).requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    yr = F.conv3d(xp, w64, padding=1)
    _close(buf[:, off:off + 32], yr.permute(0, 2, 3, 4, 1).reshape(rows, 32), 1e-5, "y")
    assert torch.equal(buf[:, :off], torch.full((rows, off), 3.0, device=DEV))
    assert torch.equal(buf[:, off + 32:], torch.full((rows, ld - off - 32), 3.0, device=DEV))
    dy = torch.randn(rows, 32, generator=g).to(DEV)
    buf[:, off:off + 32] = dy
    (yr * dy.double().view(N, T, H, W, 32).permute(0, 4, 1, 2, 3)).sum().backward()
    wflip = w.flip(2, 3, 4).permute(2, 3, 4, 0, 1).reshape(27, 32, 128).contiguous()
    dx = torch.empty(rows, 128, device=DEV)
    L.check(lib.m3t_dense_conv333(_p(buf, off), ld, N, T, H, W, 32, _p(wflip), _p(dx), 128, 128, 0, _stream()), "dgrad")
    _close(dx, xp.grad.permute(0, 2, 3, 4, 1).reshape(rows, 128), 1e-5, "dx")
    ws = torch.empty(int(lib.m3t_dense_wgrad_ws_bytes(rows, 128, 32)) // 4 + 4, device=DEV)
    dw = torch.empty(27, 128, 32, device=DEV)
    L.check(lib.m3t_dense_conv333_wgrad(_p(x), 128, _p(buf, off), ld, N, T, H, W, 128, 32, _p(dw), _p(ws), ws.numel() * 4, _stream()), "wgrad")
    _close(dw.permute(2, 1, 0).reshape(32, 128, 3, 3, 3), w64.grad, 1e-5, "dw")


def test_entry_points_refuse_what_they_do_not_cover():
    L, lib = _lib()
    x = torch.zeros(64, 128, device=DEV)
    w = torch.zeros(27 * 128 * 32, device=DEV)
    assert lib.m3t_dense_conv333(_p(x), 128, 1, 1, 8, 8, 128, _p(w), _p(x), 128, 16, 0, _stream()) == L.M3T_EINVAL      # Co % 32
    assert lib.m3t_dense_conv333(_p(x), 128, 1, 1, 8, 8, 120, _p(w), _p(x), 128, 32, 0, _stream()) == L.M3T_EINVAL      # Ci % 32
    assert lib.m3t_dense_bn_relu_fwd(_p(x), 128, 64, 6, _p(w), _p(w), _p(w), _p(w), 1e-5, _p(x), 128, _stream()) == L.M3T_EINVAL   # C % 4
