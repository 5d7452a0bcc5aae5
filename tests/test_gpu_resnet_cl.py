"""The two operators that put the per-frame ResNet (v1) on the channels-last chain (csrc/stem_cl.hip m3t_bn_add_relu_cl_* / m3t_mean_cl_*,
m3t.ops.bn_add_relu_cl / mean_cl), and the strided data gradient of _Conv3dCL with a CLTensor input, against float64.

The bar is the project's precedent (tests/test_gpu_gn_cl.py): the yardstick is the error the STOCK fp32 route (F.batch_norm -> add -> relu, and
mean, on the same device and inputs; for the data gradient the planes route m3t.ops.conv2d) makes against the same float64 result
(tests/resnet_ref.py, itself checked against torch's float64 autograd in tests/test_resnet_cl_host.py).  The new operator must stay within
4 x max(that error, 2^-23) per tensor.  Metric: max |err| / max |ref| per tensor, no element left out.  One tensor has no maximum of its own:
in train mode dx's column sums are zero by construction (the normalisation removes the batch mean), so their error -- the chain's and the
yardstick's alike -- is taken relative to the largest column sum of |dx|, the size of the terms that cancel.

Inputs are drawn clear of ReLU flips (resnet_ref.clear_of_flips: a pre-activation within fp32 rounding of zero flips its mask in ANY fp32
route and is no error of the operator), seeds tried in steps of 1000 from 0, at most 8.  With the margins of resnet_ref every case takes its
first seed except (4099, 64) in train mode: seed 0 skipped (one of its 262 336 pre-activations lies within the margin), 1000 taken.

NaN: the float64 reference decides which outputs are NaN (g = dy (y > 0) is 0 where y is NaN, so dbeta and ds stay finite; 0 x NaN keeps
dgamma NaN); the test asserts that pattern, whatever it is.

Measured on the MI355X (worst chain / stock error ratio per kind over the four shapes and both modes, the bar being 4): out 0.87, dx 2.07 (the
three-row case in train mode, 4.1e-7 against 2.0e-7; <= 0.99 elsewhere), ds exact, dgamma 1.05, dbeta 0.57, colsum 1.32, running statistics
0.89; mean_cl out 0.37, dx 0.27; the strided data gradient 1.00 throughout (the planes route's own error)."""
import pytest
import torch
import torch.nn.functional as F

import resnet_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -23
KINDS = ("out", "dx", "ds", "dgamma", "dbeta", "colsum", "run_mean", "run_var")


def rel_err(got, ref, top=None):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    top = float(ref.abs().max()) if top is None else top
    assert top > 0.0 and top == top and top != float("inf"), "the reference is all zero or not finite: the metric would be blind"
    return float((got - ref).abs().max()) / top


def _slot_bits(slot):
    return int(slot.view(torch.int64)[0].item())


def _bits_of_max_finite(t):
    a = t.detach().abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    return int(a.max().view(torch.int32).item())


def run(case, inputs, training):
    """the operator through m3t.ops on the GPU, forward and backward"""
    from m3t import ops
    M, C = case
    x, s, gamma, beta, rm, rv, dy = inputs
    dev = lambda t: t.float().to(DEV)
    xr, sr, ga, be = (dev(t).requires_grad_(True) for t in (x, s, gamma, beta))
    rm_, rv_ = dev(rm), dev(rv)
    grads = {}
    xr.register_hook(lambda g: grads.__setitem__("dx", g))
    sr.register_hook(lambda g: grads.__setitem__("ds", g))
    y = ops.bn_add_relu_cl(ops.CLTensor(xr, 1, 1, 1, M), ops.CLTensor(sr, 1, 1, 1, M), ga, be, rm_, rv_, training, R.MOMENTUM, R.EPS)
    assert isinstance(y, ops.CLTensor) and (y.N, y.T, y.H, y.W, y.C) == (1, 1, 1, M, C)
    assert type(y.data.grad_fn).__name__.startswith("_BNAddReluCL")
    y.data.backward(dev(dy))
    torch.cuda.synchronize()
    dx, ds = grads["dx"], grads["ds"]
    assert ops._grad_slot(ds) == (None, None), "ds is an ordinary tensor: no slot rides on it"
    slot, csum = ops._grad_slot(dx)
    assert slot is not None and csum is not None, "the backward pass did not hand dx's slot and column sums over"
    return dict(out=y.data.detach(), dx=dx, ds=ds, dgamma=ga.grad, dbeta=be.grad, colsum=csum, run_mean=rm_, run_var=rv_, y_slot=y.slot,
                dx_slot=slot)


def stock(inputs, training):
    x, s, gamma, beta, rm, rv, dy = (t.float().to(DEV) for t in inputs)
    return R.torch_autograd(x, s, gamma, beta, rm, rv, training, dy)


def reference_of(inputs, training):
    x, s, gamma, beta, rm, rv, dy = inputs
    f = R.forward(x, s, gamma, beta, rm, rv, training)
    b = R.backward(dy, f, gamma, training)
    return dict(out=f["y"], run_mean=f["run_mean"], run_var=f["run_var"], **b)


_REF = {}


def reference(case, training):
    """float64 on the CPU, computed once per case and mode and shared"""
    key = (case, training)
    if key not in _REF:
        inputs, taken = R.draw_clear(case, training)
        print("\n%s %s: seed %d taken" % (case, "train" if training else "eval", taken))
        _REF[key] = dict(inputs=inputs, **reference_of(inputs, training))
    return _REF[key]


def within_the_bar(what, got, stk, ref, training, kinds=KINDS):
    bad, ratios = {}, {}
    for kind in kinds:
        if kind.startswith("run_") and not training:
            assert torch.equal(got[kind].cpu().double(), ref[kind]), "%s: eval mode touched %s" % (what, kind)
            continue
        # train-mode column sums of dx cancel to zero: measured against the size of what cancels (module docstring)
        top = float(ref["dx"].abs().sum(0).max()) if (kind == "colsum" and training) else None
        e_new, e_stock = rel_err(got[kind], ref[kind], top), rel_err(stk[kind], ref[kind], top)
        ratios[kind] = e_new / max(e_stock, FLOOR)
        print("%s %-8s chain %.2e  stock %.2e  ratio %.2f" % (what, kind, e_new, e_stock, ratios[kind]))
        if not e_new <= 4.0 * max(e_stock, FLOOR):
            bad[kind] = (e_new, e_stock)
    assert not bad, "%s: over 4 x max(stock error, 2^-23): %s" % (what, bad)
    return ratios


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", R.TAIL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bn_add_relu_against_float64(case, training):
    ref = reference(case, training)
    got, stk = run(case, ref["inputs"], training), stock(ref["inputs"], training)
    print()
    within_the_bar("%s %s" % (case, "train" if training else "eval"), got, stk, ref, training)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_gamma_zero_is_the_initial_state(training):
    """zero_init_residual: gamma = 0 (and beta = 0) -> y = relu(s) bit for bit, dx exactly 0, dgamma within the bar"""
    case = (1030, 256)
    inputs = R.draw(case, 2, zero_gamma=True)
    assert R.clear_of_flips(*inputs[:6], training)
    ref = reference_of(inputs, training)
    got, stk = run(case, inputs, training), stock(inputs, training)
    assert torch.equal(got["out"], torch.relu(inputs[1].float().to(DEV)))
    assert not bool(got["dx"].any()) and not bool(got["colsum"].any())
    assert bool(torch.isfinite(got["dgamma"]).all())
    print()
    within_the_bar("gamma = 0 %s" % ("train" if training else "eval"), got, stk, ref, training, ("out", "ds", "dgamma", "dbeta", "run_mean", "run_var"))


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_nan_in_one_channel_follows_the_reference(training):
    case = (24, 512)
    inputs = list(R.draw(case, 3))
    inputs[0][5, 7] = float("nan")
    ref = reference_of(inputs, training)
    got = run(case, inputs, training)
    for kind in KINDS:
        assert torch.equal(torch.isnan(got[kind]).cpu(), torch.isnan(ref[kind])), kind
        assert bool(torch.isfinite(got[kind][~torch.isnan(got[kind])]).all()), kind
    assert bool(torch.isnan(ref["out"]).any()) and bool(torch.isnan(ref["dgamma"]).any())          # (the case is not vacuous)
    assert _slot_bits(got["y_slot"]) == _bits_of_max_finite(got["out"]) and _slot_bits(got["dx_slot"]) == _bits_of_max_finite(got["dx"])


@pytest.mark.parametrize("case", [(4099, 64), (24, 512)], ids=lambda c: "x".join(map(str, c)))
def test_slots_and_handover(case):
    """y.slot and the handed-over dx slot hold the bits of the largest finite magnitude; ds is an ordinary tensor (asserted in run())"""
    ref = reference(case, True)
    got = run(case, ref["inputs"], True)
    assert _slot_bits(got["y_slot"]) == _bits_of_max_finite(got["out"])
    assert _slot_bits(got["dx_slot"]) == _bits_of_max_finite(got["dx"])
    assert got["colsum"].shape == (case[1],) and got["ds"].shape == got["dx"].shape


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", [(4099, 64), (1030, 256)], ids=lambda c: "x".join(map(str, c)))
def test_two_runs_are_bit_identical(case, training):
    ref = reference(case, training)
    a, b = run(case, ref["inputs"], training), run(case, ref["inputs"], training)
    for kind in KINDS:
        assert torch.equal(a[kind], b[kind]), kind


# ------------------------------------------------------------------------------------------------ the spatial mean
def run_mean_cl(case, x, dy):
    from m3t import ops
    P, HW, C = case
    xr = x.reshape(P * HW, C).float().to(DEV).requires_grad_(True)
    y = ops.mean_cl(ops.CLTensor(xr, P, 1, HW, 1))
    assert torch.is_tensor(y) and y.shape == (P, C) and type(y.grad_fn).__name__.startswith("_MeanCL")
    y.backward(dy.float().to(DEV))
    torch.cuda.synchronize()
    return dict(out=y.detach(), dx=xr.grad.view(P, HW, C))


@pytest.mark.parametrize("case", R.MEAN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_mean_against_float64_and_reruns(case):
    x, dy = R.draw_mean(case)
    ref = dict(out=R.mean_forward(x), dx=R.mean_backward(dy, case[1]))
    a, b = run_mean_cl(case, x, dy), run_mean_cl(case, x, dy)
    xs = x.float().to(DEV).requires_grad_(True)
    ys = xs.mean(1)
    ys.backward(dy.float().to(DEV))
    stk = dict(out=ys.detach(), dx=xs.grad)
    print()
    for kind in ("out", "dx"):
        assert torch.equal(a[kind], b[kind]), kind
        e_new, e_stock = rel_err(a[kind], ref[kind]), rel_err(stk[kind], ref[kind])
        print("mean %s %-3s chain %.2e  stock %.2e  ratio %.2f" % (case, kind, e_new, e_stock, e_new / max(e_stock, FLOOR)))
        assert e_new <= 4.0 * max(e_stock, FLOOR), (kind, e_new, e_stock)


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_points_refuse_without_launching():
    from m3t import _lib as L
    lib = L.load()
    s = torch.cuda.current_stream().cuda_stream
    M, C = 48, 64
    x = torch.full((M, C), 1.0, device=DEV)
    y = torch.full((M, C), 5.0, device=DEV)
    y2 = torch.full((M, C), 5.0, device=DEV)
    st = torch.full((2, C), 5.0, device=DEV)
    vec = torch.full((5, C), 5.0, device=DEV)
    need = int(lib.m3t_bn_cl_ws_bytes(M, C))
    assert need > 8
    ws = torch.zeros(need // 4 + 64, device=DEV)
    p = lambda t, off=0: t.data_ptr() + 4 * off
    nb = ws.numel() * 4
    E = L.M3T_EINVAL

    def fwd(x_=p(x), s_=p(x), M_=M, C_=C, y_=p(y), ws_=p(ws), nb_=nb, st_=p(st[0])):
        return lib.m3t_bn_add_relu_cl_fwd(x_, s_, M_, C_, p(vec[0]), p(vec[1]), p(vec[3]), p(vec[4]), 0.1, 1e-5, 1, y_, st_, p(st[1]), ws_, nb_, s)

    def bwd(dy_=p(x), x_=p(x), M_=M, C_=C, dx_=p(y), ds_=p(y2), ws_=p(ws), nb_=nb, st_=p(st[0])):
        return lib.m3t_bn_add_relu_cl_bwd(dy_, x_, p(x), p(vec[0]), st_, p(st[1]), M_, C_, 1, dx_, ds_, p(vec[0]), p(vec[1]), p(vec[2]), ws_, nb_, s)

    for f in (fwd, bwd):
        assert f(C_=6) == E and f(C_=24) == E and f(C_=2048) == E and f(C_=0) == E, f.__name__
        assert f(M_=0) == E, f.__name__
        assert f(ws_=p(ws, 1)) == E and f(nb_=need - 8) == E and f(ws_=None) == E, f.__name__
        assert f(x_=None) == E and f(x_=p(x, 1)) == E and f(st_=None) == E, f.__name__
    assert fwd(s_=None) == E and fwd(s_=p(x, 1)) == E and fwd(y_=None) == E and fwd(y_=p(y, 1)) == E and fwd(M_=1) == E
    assert bwd(dy_=None) == E and bwd(dx_=None) == E and bwd(ds_=None) == E and bwd(dx_=p(y, 1)) == E and bwd(ds_=p(y2, 1)) == E
    # eval mode without running statistics
    assert lib.m3t_bn_add_relu_cl_fwd(p(x), p(x), M, C, p(vec[0]), p(vec[1]), None, None, 0.1, 1e-5, 0, p(y), p(st[0]), p(st[1]), p(ws), nb, s) == E

    def mf(x_=p(x), P_=4, HW_=12, C_=C, y_=p(y)):
        return lib.m3t_mean_cl_fwd(x_, P_, HW_, C_, y_, s)

    def mb(dy_=p(x), P_=4, HW_=12, C_=C, dx_=p(y)):
        return lib.m3t_mean_cl_bwd(dy_, P_, HW_, C_, dx_, s)

    for f in (mf, mb):
        assert f(C_=6) == E and f(C_=0) == E and f(P_=0) == E and f(HW_=0) == E, f.__name__
    assert mf(x_=None) == E and mf(y_=None) == E and mf(x_=p(x, 1)) == E and mb(dy_=None) == E and mb(dx_=None) == E and mb(dx_=p(y, 1)) == E
    torch.cuda.synchronize()
    assert bool((y == 5.0).all()) and bool((y2 == 5.0).all()) and bool((st == 5.0).all()) and bool((vec == 5.0).all()), "a refused call wrote its outputs"
    assert fwd() == 0 and bwd() == 0 and mf() == 0 and mb() == 0              # (the accepted forms of the same calls)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the strided data gradient alone
# (P frames, kernel, stride, padding, H, W): 64 -> 128 channels; odd and even grids in both axes; with 1 x 1 stride 2 three of the four parity
# classes receive no tap
DGRAD_CASES = [(3, 3, 2, 1, 13, 11), (3, 3, 2, 1, 7, 6), (3, 1, 2, 0, 13, 11), (3, 1, 2, 0, 4, 3)]


@pytest.mark.parametrize("case", DGRAD_CASES, ids=lambda c: "p%d_k%d_s%d_p%d_%dx%d" % c)
def test_strided_data_gradient_of_a_cltensor_input(case):
    """_Conv3dCL.backward's data gradient by parity classes with a CLTensor input (no caller before the ResNet chain), against a float64
    conv2d autograd; yardstick: the planes route m3t.ops.conv2d on the same tensors"""
    from m3t import ops
    P, k, st, pd, H, W = case
    Ci, Co = 64, 128
    gen = torch.Generator().manual_seed(sum(case))
    x = torch.randn(P, Ci, H, W, generator=gen).float()
    w = (torch.randn(Co, Ci, k, k, generator=gen) / (Ci * k * k) ** 0.5).float()
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, st, pd)
    dy = torch.randn(y64.shape, generator=gen).float()
    y64.backward(dy.double())
    Ho, Wo = y64.shape[2:]
    ref = dict(y=y64.detach(), dx=x64.grad, dw=w64.grad)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()
    planes = lambda r, h, w_: r.view(P, h, w_, -1).permute(0, 3, 1, 2)

    wc = torch.nn.Parameter(w.to(DEV))
    xr = rows(x).to(DEV).requires_grad_(True)
    calls = ops.CONV3D_CALLS["walk"]
    yc = ops.conv3d_cl(ops.CLTensor(xr, P, 1, H, W), wc, None, (st, st), (pd, pd))
    assert ops.CONV3D_CALLS["walk"] == calls + 1 and (yc.N, yc.T, yc.H, yc.W, yc.C) == (P, 1, Ho, Wo, Co)
    assert type(yc.data.grad_fn).__name__.startswith("_Conv3dCL")
    yc.data.backward(rows(dy).to(DEV))
    ops.join_wgrad(torch.device(DEV))
    torch.cuda.synchronize()
    got = dict(y=planes(yc.data.detach(), Ho, Wo), dx=planes(xr.grad, H, W), dw=wc.grad)

    wp = torch.nn.Parameter(w.to(DEV))
    xp = x.to(DEV).requires_grad_(True)
    yp = ops.conv2d(xp, wp, None, (st, st), (pd, pd))
    yp.backward(dy.to(DEV))
    ops.join_wgrad(torch.device(DEV))
    torch.cuda.synchronize()
    stk = dict(y=yp.detach(), dx=xp.grad, dw=wp.grad)
    print()
    bad = {}
    for kind in ("y", "dx", "dw"):
        e_new, e_stock = rel_err(got[kind], ref[kind]), rel_err(stk[kind], ref[kind])
        print("dgrad %s %-2s chain %.2e  planes %.2e  ratio %.2f" % (case, kind, e_new, e_stock, e_new / max(e_stock, FLOOR)))
        if not e_new <= 4.0 * max(e_stock, FLOOR):
            bad[kind] = (e_new, e_stock)
    assert not bad, bad
