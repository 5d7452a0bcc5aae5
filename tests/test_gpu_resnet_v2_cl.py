"""The operator that puts the per-frame ResNet v2 (pre-activation) on the channels-last chain (csrc/stem_cl.hip m3t_add_bn_relu_cl_*,
m3t.ops.add_bn_relu_cl: s = a + b and z = relu(bn(s)) from one operator, one gradient tensor ds for both addends) against float64.

The bar is the project's (tests/test_gpu_gn_cl.py, tests/test_gpu_resnet_cl.py): the yardstick is the error the STOCK fp32 route (add ->
F.batch_norm -> relu with a second use of s, on the same device and inputs) makes against the same float64 result (tests/resnet_v2_ref.py, itself
checked against torch's float64 autograd in tests/test_resnet_v2_cl_host.py).  The operator must stay within 4 x max(that error, 2^-23) per
tensor.  Metric: max |err| / max |ref| per tensor, no element left out.  In train mode the BatchNorm part of ds's column sums cancels to zero
(the normalisation removes the batch mean), so their error -- the chain's and the yardstick's alike -- is taken relative to the largest column
sum of |ds|, the size of the terms that cancel.

Inputs are drawn clear of ReLU flips (resnet_v2_ref.clear_of_flips), seeds in steps of 1000 from 0, at most 8: every case takes seed 0 in both
modes (tests/test_resnet_v2_cl_host.py asserts it without a GPU).

Because the statistics pass sums the fp32-rounded s in bn_cl's order and the map pass is bn_cl's, s, z, the running statistics and z's slot are
the BITS of torch's a + b followed by ops.bn_cl(relu=True): asserted, both modes, all six cases.

NaN: the float64 reference decides which outputs are NaN (g = dz (z > 0) is 0 where z is NaN, so dbeta stays finite; 0 x NaN keeps dgamma NaN);
the test asserts that pattern, whatever it is.

Measured on the MI355X (worst chain / stock error ratio per kind over the six shapes, both modes, with and without ds_out, the bar being 4):
s 0.45 (the stock sum's bits), z 1.80, ds 2.74 (the three-row case in train mode with ds_out, 2.1e-6 against 7.6e-7), dgamma 2.25 ((2, 4) in
train mode, 2.7e-7 against a stock error under the 2^-23 floor), dbeta 0.57, colsum 1.18, running statistics 0.97."""
import pytest
import torch

import resnet_v2_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -23
KINDS = ("s", "z", "ds", "dgamma", "dbeta", "colsum", "run_mean", "run_var")
MODES = pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
DS_OUT = pytest.mark.parametrize("with_ds_out", [True, False], ids=["ds_out", "no_ds_out"])
ALL_CASES = pytest.mark.parametrize("case", V.CASES, ids=lambda c: "x".join(map(str, c)))


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


def run(case, inputs, training, with_ds_out):
    """the operator through m3t.ops on the GPU, forward and backward"""
    from m3t import ops
    M, C = case
    a, b, gamma, beta, rm, rv, dz, ds_out = inputs
    dev = lambda t: t.float().to(DEV)
    ar, br, ga, be = (dev(t).requires_grad_(True) for t in (a, b, gamma, beta))
    rm_, rv_ = dev(rm), dev(rv)
    grads = {}
    ar.register_hook(lambda g: grads.__setitem__("ds", g))
    br.register_hook(lambda g: grads.__setitem__("ds_b", g))
    s, z = ops.add_bn_relu_cl(ops.CLTensor(ar, 1, 1, 1, M), ops.CLTensor(br, 1, 1, 1, M), ga, be, rm_, rv_, training, V.MOMENTUM, V.EPS)
    for t in (s, z):
        assert isinstance(t, ops.CLTensor) and (t.N, t.T, t.H, t.W, t.C) == (1, 1, 1, M, C)
        assert type(t.data.grad_fn).__name__.startswith("_AddBNReluCL")
    assert s.slot is None and z.slot is not None, "s carries no magnitude slot, z does"
    if with_ds_out:
        torch.autograd.backward([z.data, s.data], [dev(dz), dev(ds_out)])
    else:
        z.data.backward(dev(dz))
    torch.cuda.synchronize()
    ds = grads["ds"]
    assert torch.equal(ds, grads["ds_b"]), "a and b did not get the same gradient"
    slot, csum = ops._grad_slot(ds)
    assert slot is not None and csum is not None, "the backward pass did not hand ds's slot and column sums over"
    return dict(s=s.data.detach(), z=z.data.detach(), ds=ds, dgamma=ga.grad, dbeta=be.grad, colsum=csum, run_mean=rm_, run_var=rv_,
                z_slot=z.slot, ds_slot=slot)


def stock(inputs, training, with_ds_out):
    a, b, gamma, beta, rm, rv, dz, ds_out = (t.float().to(DEV) for t in inputs)
    return V.torch_autograd(a, b, gamma, beta, rm, rv, training, dz, ds_out if with_ds_out else None)


def reference_of(inputs, training, with_ds_out):
    a, b, gamma, beta, rm, rv, dz, ds_out = inputs
    f = V.forward(a, b, gamma, beta, rm, rv, training)
    g = V.backward(dz, ds_out if with_ds_out else None, f, gamma, training)
    return dict(s=f["s"], z=f["z"], run_mean=f["run_mean"], run_var=f["run_var"], **g)


_REF = {}


def reference(case, training, with_ds_out):
    """float64 on the CPU, computed once per case, mode and form and shared"""
    key = (case, training)
    if key not in _REF:
        inputs, taken = V.draw_clear(case, training)
        print("\n%s %s: seed %d taken" % (case, "train" if training else "eval", taken))
        _REF[key] = {"inputs": inputs}
    if with_ds_out not in _REF[key]:
        _REF[key][with_ds_out] = reference_of(_REF[key]["inputs"], training, with_ds_out)
    return dict(inputs=_REF[key]["inputs"], **_REF[key][with_ds_out])


def within_the_bar(what, got, stk, ref, training, kinds=KINDS):
    bad = {}
    for kind in kinds:
        if kind.startswith("run_") and not training:
            assert torch.equal(got[kind].cpu().double(), ref[kind]), "%s: eval mode touched %s" % (what, kind)
            continue
        # train-mode column sums: the BatchNorm part cancels to zero -- measured against the size of what cancels (module docstring)
        top = float(ref["ds"].abs().sum(0).max()) if (kind == "colsum" and training) else None
        e_new, e_stock = rel_err(got[kind], ref[kind], top), rel_err(stk[kind], ref[kind], top)
        print("%s %-8s chain %.2e  stock %.2e  ratio %.2f" % (what, kind, e_new, e_stock, e_new / max(e_stock, FLOOR)))
        if not e_new <= 4.0 * max(e_stock, FLOOR):
            bad[kind] = (e_new, e_stock)
    assert not bad, "%s: over 4 x max(stock error, 2^-23): %s" % (what, bad)


def _name(case, training, with_ds_out):
    return "%s %s %s" % (case, "train" if training else "eval", "ds_out" if with_ds_out else "no ds_out")


@DS_OUT
@MODES
@ALL_CASES
def test_add_bn_relu_against_float64(case, training, with_ds_out):
    ref = reference(case, training, with_ds_out)
    got, stk = run(case, ref["inputs"], training, with_ds_out), stock(ref["inputs"], training, with_ds_out)
    print()
    within_the_bar(_name(case, training, with_ds_out), got, stk, ref, training)
    # the slots hold the bits of the largest finite magnitude of what the kernels wrote
    assert _slot_bits(got["z_slot"]) == _bits_of_max_finite(got["z"])
    assert _slot_bits(got["ds_slot"]) == _bits_of_max_finite(got["ds"])
    assert got["colsum"].shape == (case[1],)


@MODES
@ALL_CASES
def test_forward_is_the_bits_of_add_then_bn_cl(case, training):
    from m3t import ops
    M, C = case
    a, b, gamma, beta, rm, rv = (t.float().to(DEV) for t in reference(case, training, True)["inputs"][:6])
    rm1, rv1, rm2, rv2 = rm.clone(), rv.clone(), rm.clone(), rv.clone()
    cl = lambda t: ops.CLTensor(t, 1, 1, 1, M)
    with torch.no_grad():
        s, z = ops.add_bn_relu_cl(cl(a), cl(b), gamma, beta, rm1, rv1, training, V.MOMENTUM, V.EPS)
        s2 = a + b
        z2 = ops.bn_cl(cl(s2), gamma, beta, rm2, rv2, training, V.MOMENTUM, V.EPS, True)
    torch.cuda.synchronize()
    assert torch.equal(s.data, s2) and torch.equal(z.data, z2.data)
    assert torch.equal(rm1, rm2) and torch.equal(rv1, rv2)
    assert (torch.equal(rm1, rm) and torch.equal(rv1, rv)) != training         # eval: untouched; train: updated
    assert _slot_bits(z.slot) == _slot_bits(z2.slot) == _bits_of_max_finite(z2.data)


@MODES
@pytest.mark.parametrize("case", [(4099, 64), (2, 4), (257, 1024)], ids=lambda c: "x".join(map(str, c)))
def test_eval_forward_without_s_gives_the_same_z(case, training):
    """need_s=False under no_grad: in eval mode the sum is not written (s is None) and z has the same bits; in train mode the statistics pass
    needs s whatever the caller says"""
    from m3t import ops
    M, C = case
    a, b, gamma, beta, rm, rv = (t.float().to(DEV) for t in reference(case, training, True)["inputs"][:6])
    cl = lambda t: ops.CLTensor(t, 1, 1, 1, M)
    with torch.no_grad():
        s1, z1 = ops.add_bn_relu_cl(cl(a), cl(b), gamma, beta, rm.clone(), rv.clone(), training, V.MOMENTUM, V.EPS)
        s0, z0 = ops.add_bn_relu_cl(cl(a), cl(b), gamma, beta, rm.clone(), rv.clone(), training, V.MOMENTUM, V.EPS, need_s=False)
    s2, z2 = ops.add_bn_relu_cl(cl(a), cl(b), gamma, beta, rm.clone(), rv.clone(), training, V.MOMENTUM, V.EPS, need_s=False)
    torch.cuda.synchronize()
    assert (s0 is None) == (not training) and s2 is not None       # (grad mode on: backward would need s)
    assert torch.equal(z0.data, z1.data) and torch.equal(z2.data, z1.data) and _slot_bits(z0.slot) == _slot_bits(z1.slot)
    assert s0 is None or torch.equal(s0.data, s1.data)


@DS_OUT
@MODES
def test_gamma_zero(training, with_ds_out):
    """gamma = 0: z = relu(beta) and nothing comes back through the BatchNorm -- ds is ds_out bit for bit (or exactly zero)"""
    case = (1030, 256)
    inputs = list(V.draw(case, 2))
    inputs[2] = torch.zeros_like(inputs[2])
    assert V.clear_of_flips(*inputs[:6], training)
    ref = reference_of(inputs, training, with_ds_out)
    got, stk = run(case, inputs, training, with_ds_out), stock(inputs, training, with_ds_out)
    assert torch.equal(got["z"], torch.relu(inputs[3].float().to(DEV)).expand_as(got["z"]))
    if with_ds_out:
        assert torch.equal(got["ds"], inputs[7].float().to(DEV))
    else:
        assert not bool(got["ds"].any()) and not bool(got["colsum"].any())
    assert bool(torch.isfinite(got["dgamma"]).all())
    print()
    kinds = ("s", "z", "dgamma", "dbeta", "run_mean", "run_var") + (("ds", "colsum") if with_ds_out else ())
    within_the_bar("gamma = 0 " + _name(case, training, with_ds_out), got, stk, ref, training, kinds)


@DS_OUT
@MODES
@pytest.mark.parametrize("case", [(4099, 64), (1030, 256), (2, 4)], ids=lambda c: "x".join(map(str, c)))
def test_two_runs_are_bit_identical(case, training, with_ds_out):
    ref = reference(case, training, with_ds_out)
    x, y = run(case, ref["inputs"], training, with_ds_out), run(case, ref["inputs"], training, with_ds_out)
    for kind in KINDS:
        assert torch.equal(x[kind], y[kind]), kind
    assert _slot_bits(x["z_slot"]) == _slot_bits(y["z_slot"]) and _slot_bits(x["ds_slot"]) == _slot_bits(y["ds_slot"])


@DS_OUT
@MODES
def test_nan_in_one_element_follows_the_reference(training, with_ds_out):
    case = (24, 512)
    inputs = list(V.draw(case, 3))
    inputs[0][5, 7] = float("nan")
    ref = reference_of(inputs, training, with_ds_out)
    got = run(case, inputs, training, with_ds_out)
    for kind in KINDS:
        assert torch.equal(torch.isnan(got[kind]).cpu(), torch.isnan(ref[kind])), kind
        assert bool(torch.isfinite(got[kind][~torch.isnan(got[kind])]).all()), kind
    assert bool(torch.isnan(ref["s"]).any()) and bool(torch.isnan(ref["z"]).any()) and bool(torch.isnan(ref["dgamma"]).any())      # (not vacuous)
    assert _slot_bits(got["z_slot"]) == _bits_of_max_finite(got["z"]) and _slot_bits(got["ds_slot"]) == _bits_of_max_finite(got["ds"])


def test_a_missing_dz_passes_ds_out_through():
    """only s is used downstream: backward gets no dz -- ds is ds_out itself, the affine gradients are zero, nothing is launched"""
    from m3t import ops
    case = (24, 512)
    a, b, gamma, beta, rm, rv, dz, ds_out = (t.float().to(DEV) for t in V.draw(case, 4))
    ar, br, ga, be = (t.requires_grad_(True) for t in (a, b, gamma, beta))
    s, z = ops.add_bn_relu_cl(ops.CLTensor(ar, 1, 1, 1, 24), ops.CLTensor(br, 1, 1, 1, 24), ga, be, rm, rv, True, V.MOMENTUM, V.EPS)
    s.data.backward(ds_out)
    torch.cuda.synchronize()
    assert torch.equal(ar.grad, ds_out) and torch.equal(br.grad, ds_out)
    assert not bool(ga.grad.any()) and not bool(be.grad.any())


def test_entry_points_refuse_without_launching():
    from m3t import _lib as L
    lib = L.load()
    st_ = torch.cuda.current_stream().cuda_stream
    M, C = 48, 64
    x = torch.full((M, C), 1.0, device=DEV)
    s = torch.full((M, C), 5.0, device=DEV)
    z = torch.full((M, C), 5.0, device=DEV)
    st = torch.full((2, C), 5.0, device=DEV)
    vec = torch.full((5, C), 5.0, device=DEV)
    need = int(lib.m3t_bn_cl_ws_bytes(M, C))
    ws = torch.zeros(need // 4 + 64, device=DEV)
    p = lambda t, off=0: t.data_ptr() + 4 * off
    nb = ws.numel() * 4
    E = L.M3T_EINVAL

    def fwd(a_=p(x), b_=p(x), M_=M, C_=C, s_=p(s), z_=p(z), ws_=p(ws), nb_=nb, m_=p(st[0]), training=1):
        return lib.m3t_add_bn_relu_cl_fwd(a_, b_, M_, C_, p(vec[0]), p(vec[1]), p(vec[3]), p(vec[4]), 0.1, 1e-5, training, s_, z_, m_, p(st[1]), ws_, nb_, st_)

    def bwd(dz_=p(x), o_=p(x), s_=p(x), z_=p(x), M_=M, C_=C, ds_=p(z), ws_=p(ws), nb_=nb, m_=p(st[0])):
        return lib.m3t_add_bn_relu_cl_bwd(dz_, o_, s_, z_, p(vec[0]), m_, p(st[1]), M_, C_, 1, ds_, p(vec[0]), p(vec[1]), p(vec[2]), ws_, nb_, st_)

    for f in (fwd, bwd):
        assert f(C_=6) == E and f(C_=24) == E and f(C_=2048) == E and f(C_=0) == E, f.__name__
        assert f(M_=0) == E, f.__name__
        assert f(ws_=p(ws, 1)) == E and f(nb_=need - 8) == E and f(ws_=None) == E, f.__name__
        assert f(m_=None) == E and f(s_=p(x, 1)) == E and f(z_=None) == E and f(z_=p(z, 1)) == E, f.__name__
    assert fwd(a_=None) == E and fwd(b_=None) == E and fwd(a_=p(x, 1)) == E and fwd(b_=p(x, 1)) == E and fwd(M_=1) == E
    assert fwd(s_=None) == E, "training needs s"
    assert bwd(dz_=None) == E and bwd(s_=None) == E and bwd(ds_=None) == E and bwd(ds_=p(z, 1)) == E and bwd(dz_=p(x, 1)) == E and bwd(o_=p(x, 1)) == E
    # eval mode without running statistics
    assert lib.m3t_add_bn_relu_cl_fwd(p(x), p(x), M, C, p(vec[0]), p(vec[1]), None, None, 0.1, 1e-5, 0, p(s), p(z), p(st[0]), p(st[1]), p(ws), nb, st_) == E
    torch.cuda.synchronize()
    assert bool((s == 5.0).all()) and bool((z == 5.0).all()) and bool((st == 5.0).all()) and bool((vec == 5.0).all()), "a refused call wrote its outputs"
    assert fwd() == 0 and bwd() == 0 and bwd(o_=None) == 0 and fwd(s_=None, training=0) == 0      # (the accepted forms of the same calls)
    torch.cuda.synchronize()
