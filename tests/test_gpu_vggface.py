"""`--backbone vggface` on the MI355X: the entry points of csrc/vggface.hip (plain ReLU, ReLU + ceil-mode pooling) against the stock float32
operators bit for bit, the per-frame convolutions on the channels-last chain against F.conv2d in float64, VA_VGGFace end to end against the
reference's own runs (tests/golden/vggface_*.npz) and the properties of the chain (no stock operator, bit-identical reruns, one path whatever
the grad mode, seeded dropout, the uint8 route, refusals)."""
import argparse
import copy
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from golden.recipe import fill_module, grad_digest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cl(a):
    """planes [P, C, H, W] -> CLTensor (rows (p, h, w) x C), every frame a clip of one"""
    from m3t import ops
    P, Cc, H, W = a.shape
    return ops.CLTensor(a.permute(0, 2, 3, 1).reshape(-1, Cc).contiguous(), P, 1, H, W, None)


def _planes(rows, P, H, W):
    return rows.view(P, H, W, -1).permute(0, 3, 1, 2)


def _ulp32(v):
    """the spacing of float32 at |v| (float64 tensor in, float64 out)"""
    a = v.abs().clamp_min(2.0 ** -126).float()
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).double()


def _colsum_ok(csum, dx_rows, what):
    """the column sums the dx pass hands to the convolution in front (its bias gradient): within 1 ulp of fp32 of the fp64 column sum"""
    ref = dx_rows.double().sum(0)
    err = (csum.double() - ref).abs()
    assert bool((err <= _ulp32(ref)).all()), (what, float(err.max()))


def _handed(dx):
    """(slot, colsum) a backward kernel left for the gradient tensor object `dx` (m3t.ops._note_grad_slot)"""
    from m3t import ops
    slot, csum = ops._grad_slot(dx)
    assert slot is not None and csum is not None, "the backward pass did not hand its slot and column sums over"
    return slot, csum


def _slot_bits(slot):
    return int(slot.view(torch.int64)[0].item())


def _bits_of_max(t):
    return int(t.abs().max().view(torch.int32).item())


# ------------------------------------------------------------------------------------------- ReLU + 2 x 2 pooling, ceil mode
POOL_CASES = [(H, W, True) for H, W in ((7, 7), (5, 6), (2, 3), (1, 4), (1, 1))] + [(7, 7, False), (5, 6, False)]


def _pool_step(x, ceil_mode, dyp=None, seed=0):
    """-> (yp rows, dx rows, colsum, slots) of relu_pool_cl and the stock (yp, dx) in planes"""
    from m3t import ops
    P, Cc, H, W = x.shape
    xc = _cl(x)
    xc._data.requires_grad_(True)
    grads = {}
    xc._data.register_hook(lambda g: grads.__setitem__("dx", g))
    y = ops.relu_pool_cl(xc, ceil_mode=ceil_mode)
    xs = x.clone().requires_grad_(True)
    ys = F.max_pool2d(F.relu(xs), 2, 2, 0, ceil_mode=ceil_mode)
    assert (y.N * y.T, y.H, y.W) == (P, ys.shape[2], ys.shape[3])
    if dyp is None:
        dyp = torch.randn(ys.shape, generator=torch.Generator().manual_seed(seed)).to(DEV)
    (y.data * dyp.permute(0, 2, 3, 1).reshape(-1, Cc)).sum().backward()
    (ys * dyp).sum().backward()
    torch.cuda.synchronize()
    return y, grads["dx"], ys.detach(), xs.grad


@pytest.mark.parametrize("C", [64, 12])
@pytest.mark.parametrize("H,W,ceil_mode", POOL_CASES)
def test_relu_pool_equals_stock(H, W, ceil_mode, C):
    P = 3
    g = torch.Generator().manual_seed(100 * H + 10 * W + C + int(ceil_mode))
    x = torch.randn(P, C, H, W, generator=g).to(DEV)            # (continuous values: no ties between positive values)
    y, dx, ys, dxs = _pool_step(x, ceil_mode, seed=H + W)
    assert torch.equal(_planes(y.data.detach(), P, y.H, y.W), ys)
    assert torch.equal(_planes(dx, P, H, W), dxs)
    slot, csum = _handed(dx)
    _colsum_ok(csum, dx, "relu_pool colsum")
    assert _slot_bits(slot) == _bits_of_max(dx)
    assert _slot_bits(y.slot) == _bits_of_max(ys)


def test_relu_pool_first_of_equal_values_wins():
    P, C, H, W = 2, 12, 3, 4
    x = torch.full((P, C, H, W), -1.0)
    x[:, :, 0, 1] = 2.0; x[:, :, 1, 0] = 2.0; x[:, :, 1, 1] = 2.0      # window (0, 0): three equal maxima, (0, 1) first in window order
    x[:, :, 2, 2] = 5.0; x[:, :, 2, 3] = 5.0                           # ragged window (1, 1): two equal maxima, (2, 2) first
    # window (0, 1) and (1, 0): all negative -> relu makes four (two) equal zeros, the first position wins and passes nothing (yp = 0)
    y, dx, ys, dxs = _pool_step(x.to(DEV), True, seed=3)
    assert torch.equal(_planes(y.data.detach(), P, y.H, y.W), ys)
    got = _planes(dx, P, H, W)
    assert torch.equal(got, dxs)
    assert bool((got[:, :, 0, 1] != 0).all()) and bool((got[:, :, 1, 0] == 0).all()) and bool((got[:, :, 1, 1] == 0).all())
    assert bool((got[:, :, 2, 2] != 0).all()) and bool((got[:, :, 2, 3] == 0).all())


def test_relu_pool_nan_reaches_the_pooled_frame():
    P, C, H, W = 2, 64, 5, 5
    x = torch.randn(P, C, H, W, generator=torch.Generator().manual_seed(4))
    x[1, 3, 4, 4] = float("nan")            # alone in its ragged window
    x[0, 5, 1, 1] = float("nan")            # last of a full window whose first value is the largest number
    x[0, 5, 0, 0] = 9.0
    y, dx, ys, dxs = _pool_step(x.to(DEV), True, seed=5)
    yp = _planes(y.data.detach(), P, y.H, y.W)
    assert bool(torch.isnan(yp[1, 3, 2, 2])) and bool(torch.isnan(yp[0, 5, 0, 0]))
    assert torch.equal(torch.isnan(yp), torch.isnan(ys))
    assert torch.equal(torch.nan_to_num(yp, nan=-7.0), torch.nan_to_num(ys, nan=-7.0))
    assert torch.equal(_planes(dx, P, H, W), dxs)        # (torch lets the gradient through a NaN winner; so does the gather)


# ------------------------------------------------------------------------------------------- plain ReLU
@pytest.mark.parametrize("C", [64, 12])
@pytest.mark.parametrize("M", [1, 97, 300])
def test_relu_equals_stock(M, C):
    from m3t import ops
    g = torch.Generator().manual_seed(M + C)
    x = torch.randn(M, C, generator=g).to(DEV)
    dy = torch.randn(M, C, generator=g).to(DEV)
    xd = x.clone().requires_grad_(True)
    grads = {}
    xd.register_hook(lambda t: grads.__setitem__("dx", t))
    y = ops.relu_cl(ops.CLTensor(xd, 1, 1, 1, M, None))
    (y.data * dy).sum().backward()
    xs = x.clone().requires_grad_(True)
    ys = F.relu(xs)
    (ys * dy).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(y.data.detach(), ys.detach())
    assert torch.equal(grads["dx"], xs.grad)
    assert _slot_bits(y.slot) == _bits_of_max(ys)
    slot, csum = _handed(grads["dx"])
    assert _slot_bits(slot) == _bits_of_max(xs.grad)
    _colsum_ok(csum, grads["dx"], "relu colsum")


def test_relu_in_place_and_nan():
    from m3t import ops
    M, C = 97, 12
    g = torch.Generator().manual_seed(8)
    x = torch.randn(M, C, generator=g).to(DEV)
    x[5, 7] = float("nan")
    dy = torch.randn(M, C, generator=g).to(DEV)
    leaf = x.clone().requires_grad_(True)
    pre = leaf * 1.0                                      # (a non-leaf, as a convolution's output)
    ptr = pre.data_ptr()
    y = ops.relu_cl(ops.CLTensor(pre, 1, 1, 1, M, None), inplace=True)
    assert y.data.data_ptr() == ptr, "in-place ReLU allocated a new tensor"
    (y.data * dy).sum().backward()
    xs = x.clone().requires_grad_(True)
    ys = F.relu(xs)
    (ys * dy).sum().backward()
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.data[5, 7])) and int(torch.isnan(y.data).sum()) == 1
    assert torch.equal(torch.nan_to_num(y.data.detach(), nan=-7.0), torch.nan_to_num(ys.detach(), nan=-7.0))
    assert torch.equal(leaf.grad, xs.grad)               # (threshold_backward lets dy through where y is NaN)
    fin = torch.nan_to_num(ys.detach(), nan=0.0)
    assert _slot_bits(y.slot) == _bits_of_max(fin)       # (inf / NaN do not count towards the magnitude)


# ------------------------------------------------------------------------------------------- per-frame convolutions on the chain
def _rel_err(got, ref):
    """max |got - ref| / max |ref| (tests/test_gpu_frontends_fp64.py: relative to the tensor's own maximum)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    top = float(ref.abs().max())
    assert top > 0.0 and math.isfinite(top)
    return float((got - ref).abs().max()) / top


WALK_BAR = 2e-5          # the bar of the walks against float64 in tests/test_gpu_frontends_fp64.py (fp16x3 products: ~2^-21 per term)


@pytest.mark.parametrize("Ci,first,dgrad", [(32, False, False), (64, False, True), (3, True, False)])
def test_conv2d_weight_on_the_chain_against_float64(Ci, first, dgrad):
    """2 clips x 2 frames of 5 x 6; frame 1 of every clip is 1000 times frame 0's magnitude, so a tap that crossed a frame boundary (a time
    tap other than the unit one) would swamp frame 0's outputs and gradients.  Forward, weight gradient and the bias gradient through the
    column-sum hand-over of relu_cl's backward for C_in = 32, 64 and the first layer (C_in = 3, the video's planes); the data gradient at
    C_in = 64 -- the data-gradient walk writes 64-channel tiles, C_in = 32 has none on the chain (m3t_conv3d_taps: C_dst % 64)."""
    from m3t import ops
    B, T, H, W, Co = 2, 2, 5, 6, 64
    rs = np.random.RandomState(Ci)
    conv = fill_module(torch.nn.Conv2d(Ci, Co, 3, 1, 1), 21 + Ci).to(DEV)
    x = rs.standard_normal((B, Ci, T, H, W)).astype(np.float32)
    x[:, :, 1] *= 1000.0
    ct = rs.standard_normal((B, Co, T, H, W)).astype(np.float32)
    ct[:, :, 0] *= 1000.0                     # (and the gradients the other way round)
    xd, ctd = torch.from_numpy(x).to(DEV), torch.from_numpy(ct).to(DEV)
    ct_rows = ctd.permute(0, 2, 3, 4, 1).reshape(-1, Co)
    assert ops.vggface_ok(xd)
    if first:
        xin, leaf = xd, None
    else:
        leaf = xd.permute(0, 2, 3, 4, 1).reshape(-1, Ci).contiguous().requires_grad_(dgrad)
        xin = ops.CLTensor(leaf, B, T, H, W, None)
    assert ops.conv3d_cl_ok(xin, conv.weight, conv.stride, conv.padding, conv.groups, conv.dilation, conv.padding_mode)
    pre = ops.conv3d_cl(xin, conv.weight, conv.bias, conv.stride, conv.padding)
    assert (pre.N, pre.T, pre.H, pre.W, pre.C) == (B, T, H, W, Co)
    y_pre = pre.data.detach().clone()
    y = ops.relu_cl(pre, inplace=True)
    (y.data * ct_rows).sum().backward()
    torch.cuda.synchronize()
    assert conv.weight.grad.shape == conv.weight.shape
    # float64: every frame on its own through F.conv2d
    w64, b64 = conv.weight.detach().double().cpu().requires_grad_(True), conv.bias.detach().double().cpu().requires_grad_(True)
    f64 = torch.from_numpy(x).double().permute(0, 2, 1, 3, 4).reshape(B * T, Ci, H, W).requires_grad_(True)
    p64 = F.conv2d(f64, w64, b64, 1, 1)
    c64 = torch.from_numpy(ct).double().permute(0, 2, 1, 3, 4).reshape(B * T, Co, H, W)
    (F.relu(p64) * c64).sum().backward()
    rows64 = lambda t: t.permute(0, 2, 3, 1).reshape(B * T * H * W, -1)
    errs = {"y": _rel_err(y_pre, rows64(p64)), "dw": _rel_err(conv.weight.grad, w64.grad), "db": _rel_err(conv.bias.grad, b64.grad)}
    if dgrad:
        errs["dx"] = _rel_err(leaf.grad, rows64(f64.grad))
    print("\nconv2d on the chain, C_in %d: %s" % (Ci, errs))
    for k, e in errs.items():
        assert e <= WALK_BAR, (k, e)


# ------------------------------------------------------------------------------------------- VA_VGGFace against the reference's runs
@pytest.fixture(scope="module")
def va_cpu():
    """VA_VGGFace(hiddenDim=64, nClasses=2, nFCs=2) built once on the host (42 M parameters: thirteen xavier draws and fc1's); the tests fill
    copies of it from their recipe seeds"""
    from models.backbone import VA_VGGFace
    return VA_VGGFace(hiddenDim=64, frameLen=2, nClasses=2, nFCs=2)


def _model(va_cpu, seed, T, training=False):
    m = fill_module(copy.deepcopy(va_cpu), seed + 1).to(DEV)
    m.frameLen = T
    return m.train() if training else m.eval()


def _video(seed, B, T, S, u8=False):
    rs = np.random.RandomState(seed)
    v = rs.randint(0, 256, (B, 3, T, S, S))
    if u8:
        return torch.from_numpy(v.astype(np.uint8)).to(DEV)
    x = torch.from_numpy(v.astype(np.float32)).to(DEV)
    return (x - 127.5) / 127.5


def _close(a, b, tol, what):
    a = a.detach().double().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)
    b = b.detach().double().cpu().numpy() if torch.is_tensor(b) else np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float(np.abs(a - b).max())
    print("%s: max abs err %.3e (bar %.3e)" % (what, err, tol * max(1.0, float(np.abs(b).max()))))
    assert err <= tol * max(1.0, float(np.abs(b).max())), "%s: max abs err %.3e" % (what, err)


def _digest_err(got, ref):
    return max(abs(got[0] - ref[0]) / max(1.0, ref[0]), float(np.abs(got[2:] - ref[2:]).max()) / max(1.0, float(np.abs(ref[2:]).max())))


# bars of the ResNet3D / DenseNet goldens (tests/test_gpu_densenet.py): outputs 2e-4 of max(1, max |ref|), gradient digests 2e-3
Y_TOL, DIGEST_TOL = 2e-4, 2e-3


@pytest.mark.parametrize("name", ["vggface_eval_112", "vggface_eval_100"])
def test_vggface_golden(va_cpu, name):
    """eval mode (dropout draws nothing): y, the fc1 features (the fixture keeps fc1's output before the ReLU; the module's GEMM applies the ReLU
    in its epilogue, so the comparison is with relu(feat)) and every parameter-gradient digest.  100 x 100: 100 -> 50 -> 25 -> 13 -> 7 -> 4,
    three ragged poolings."""
    g = load_golden(name)
    seed = int(g["seed"])
    B, T, S = [int(v) for v in g["dims"]]
    m = _model(va_cpu, seed, T)
    x = _video(seed, B, T, S)
    feats = {}
    h = m.vgg.register_forward_hook(lambda mod, inp, out: feats.__setitem__("feat", out.detach()))
    y = m(x)
    h.remove()
    _close(y, g["y"], Y_TOL, "y")
    _close(feats["feat"], np.maximum(g["feat"], 0.0), Y_TOL, "feat")
    (y * torch.from_numpy(g["ct"]).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    names = sorted(n for n, p in m.named_parameters() if p.grad is not None)
    assert names == sorted(k[3:] for k in g if k.startswith("gd."))
    worst = ("", 0.0)
    for n, p in m.named_parameters():
        e = _digest_err(grad_digest(p.grad.detach().cpu().numpy()), g["gd." + n])
        gap = _digest_err(g["gd." + n], g["gd64." + n])
        if e > worst[1]:
            worst = (n, e)
        assert e <= DIGEST_TOL, "%s: digest error %.3e (the reference's own fp32-fp64 gap: %.3e)" % (n, e, gap)
    print("worst gradient digest: %s %.3e" % worst)


def _step(m, x, ct):
    y = m(x)
    (y * ct).sum().backward()
    torch.cuda.synchronize()
    return y.detach()


SMALL = (2, 2, 36)          # 36 -> 18 -> 9 -> 5 -> 3 -> 2: two ragged poolings, 2 x 2 x 512 = 2048 features: fc1 gets a 2048-column slice


@pytest.fixture(scope="module")
def small_cpu(va_cpu):
    """VA_VGGFace whose fc1 takes the 2 x 2 x 512 map of a 36 x 36 frame (the properties below need the chain, not 112 x 112 frames), filled
    once from the recipe"""
    m = fill_module(copy.deepcopy(va_cpu), 5)
    lin = torch.nn.Linear(2 * 2 * 512, 4096)
    with torch.no_grad():
        lin.weight.copy_(m.vgg.fc1.weight[:, :2048])
        lin.bias.copy_(m.vgg.fc1.bias)
    m.vgg.fc1 = lin
    return m


def _small_model(small_cpu, training):
    m = copy.deepcopy(small_cpu).to(DEV)
    return m.train() if training else m.eval()


def test_training_step_takes_no_stock_operator(small_cpu):
    from m3t import ops
    m = _small_model(small_cpu, True)
    x = _video(6, *SMALL)
    before = dict(ops.STOCK_FALLBACKS)
    walks = ops.CONV3D_CALLS["walk"]
    _step(m, x, torch.ones(2, 2, 2, device=DEV))
    assert {k: v for k, v in ops.STOCK_FALLBACKS.items() if v != before.get(k, 0)} == {}
    assert ops.CONV3D_CALLS["walk"] - walks == 13
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_two_identical_steps_are_bit_identical(small_cpu):
    m1 = _small_model(small_cpu, True)
    m1.vgg.drop_seed = 1234
    m2 = copy.deepcopy(m1)
    x = _video(8, *SMALL)
    ct = torch.randn(2, 2, 2, generator=torch.Generator().manual_seed(1)).to(DEV)
    y1, y2 = _step(m1, x, ct), _step(m2, x, ct)
    assert torch.equal(y1, y2)
    for (n, p1), p2 in zip(m1.named_parameters(), m2.parameters()):
        assert torch.equal(p1.grad, p2.grad), n


def test_no_grad_eval_equals_grad_mode_eval(small_cpu):
    m = _small_model(small_cpu, False)
    x = _video(10, *SMALL)
    with torch.no_grad():
        a = m(x)
    b = m(x)
    assert torch.equal(a, b.detach())


def test_seeded_dropout_repeats_and_differs_from_eval(small_cpu):
    m = _small_model(small_cpu, True)
    x = _video(12, *SMALL)
    m.vgg.drop_seed = 99
    with torch.no_grad():
        a, b = m(x), m(x)
        m.vgg.drop_seed = 100
        c = m(x)
        m.eval()
        e = m(x)
    assert torch.equal(a, b)
    assert not torch.equal(a, c) and not torch.equal(a, e)


def test_uint8_batch_equals_float32_batch(small_cpu):
    from m3t import ops, video
    m = _small_model(small_cpu, False)
    u8 = _video(14, *SMALL, u8=True)                                     # [B, 3, T, S, S]
    frames = u8.permute(0, 2, 3, 4, 1).contiguous()                     # as decoded: [N, Ts, Hs, Ws, 3]
    xin = video.ingest_for(m, frames)
    assert isinstance(xin, ops.VideoCL)
    with torch.no_grad():
        a = m(xin)
        b = m((u8.float() - 127.5) / 127.5)
    assert torch.equal(a, b)


def test_entry_points_refuse_without_launching():
    from m3t import _lib as L
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    x = torch.full((64, 16), -1.0, device=DEV)
    y = torch.full((64, 16), 5.0, device=DEV)
    win = torch.zeros(64, 16, dtype=torch.uint8, device=DEV)
    cs = torch.full((16,), 5.0, device=DEV)
    ws = torch.zeros(4096, device=DEV)
    p = lambda t, off=0: t.data_ptr() + 4 * off
    need = int(lib.m3t_relu_cl_ws_bytes(64, 16))
    assert need > 8
    assert lib.m3t_relu_cl_fwd(p(x), 64, 6, p(y), s) == L.M3T_EINVAL                                            # C % 4
    assert lib.m3t_relu_cl_fwd(p(x, 1), 64, 16, p(y), s) == L.M3T_EINVAL                                        # misaligned
    assert lib.m3t_relu_cl_bwd(p(x), p(x), 64, 6, p(y), p(cs), p(ws), ws.numel() * 4, s) == L.M3T_EINVAL         # C % 4
    assert lib.m3t_relu_cl_bwd(p(x), p(x), 64, 16, p(y), p(cs), p(ws), need - 8, s) == L.M3T_EINVAL              # short workspace
    assert lib.m3t_relu_pool_cl_fwd(p(x), 4, 4, 4, 6, 1, p(y), win.data_ptr(), s) == L.M3T_EINVAL                # C % 4
    assert lib.m3t_relu_pool_cl_fwd(p(x), 4, 0, 4, 16, 1, p(y), win.data_ptr(), s) == L.M3T_EINVAL               # H < 1
    assert lib.m3t_relu_pool_cl_fwd(p(x), 4, 4, 0, 16, 1, p(y), win.data_ptr(), s) == L.M3T_EINVAL               # W < 1
    assert lib.m3t_relu_pool_cl_bwd(p(x), p(x), win.data_ptr(), 4, 4, 4, 6, 1, p(y), p(cs), p(ws), ws.numel() * 4, s) == L.M3T_EINVAL
    assert lib.m3t_relu_pool_cl_bwd(p(x), p(x), win.data_ptr(), 4, 4, 4, 16, 1, p(y), p(cs), p(ws), need - 8, s) == L.M3T_EINVAL
    assert lib.m3t_relu_pool_cl_bwd(p(x), p(x), win.data_ptr(), 4, 4, 0, 16, 1, p(y), p(cs), p(ws), ws.numel() * 4, s) == L.M3T_EINVAL
    torch.cuda.synchronize()
    assert bool((y == 5.0).all()) and bool((cs == 5.0).all()) and bool((win == 0).all()), "a refused call wrote its outputs"


# ------------------------------------------------------------------------------------------- AffWild2VA(backbone='vggface') in the trainer
def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _va_batch(seed, T=2, S=112, start=0):
    rs = np.random.RandomState(seed)
    f = lambda a: torch.from_numpy(a).to(DEV)
    return {"video": f(rs.randint(0, 256, (1, 3, T, S, S)).astype(np.float32)), "se_features": f(rs.standard_normal((1, 512, T)).astype(np.float32)),
            "label_valence": f(rs.uniform(-1, 1, (1, T)).astype(np.float32)), "label_arousal": f(rs.uniform(-1, 1, (1, T)).astype(np.float32)),
            "vid_name": ["v"], "start": torch.tensor([start]), "length": torch.tensor([T])}


@pytest.fixture(scope="module")
def va_trainer():
    from models.model import AffWild2VA
    from m3t.trainer import Trainer
    torch.manual_seed(31)
    model = AffWild2VA(_hp(modality="visual", backbone="vggface", loss="ccc", window=2, num_hidden=64)).to(DEV)
    tr = Trainer.from_hparams(model, model.hparams)
    yield tr
    tr.ddp.close()


def test_trainer_step_through_affwild2va(va_trainer):
    from m3t import ops
    before = dict(ops.STOCK_FALLBACKS)
    w0 = va_trainer.model.visual.vgg.conv3.convs[1].weight.detach().clone()
    out = va_trainer.step(_va_batch(41))
    torch.cuda.synchronize()
    assert math.isfinite(float(out["loss"].detach())) and math.isfinite(float(out["grad_norm"]))
    assert not torch.equal(w0, va_trainer.model.visual.vgg.conv3.convs[1].weight.detach()), "the optimizer step did not reach the convolutions"
    assert {k: v for k, v in ops.STOCK_FALLBACKS.items() if v != before.get(k, 0)} == {}


def test_trainer_evaluate_through_affwild2va(va_trainer, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    res = va_trainer.evaluate([_va_batch(42), _va_batch(43, start=2)])
    assert math.isfinite(res["val_loss"]) and set(res["progress_bar"]) == {"val_ccc_v", "val_ccc_a"}
