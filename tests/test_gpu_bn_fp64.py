"""The three BatchNorm (+ReLU) families of csrc/bn.hip -- the row kernels behind `tcn_simple` (m3t_bn_rows_*), the chunked channel-plane
kernels of the 3-D stems (m3t_bn_planes_*, S > 1024) and the small-plane kernels of the per-frame ResNet (S <= 1024) -- against float64.

Two bars.

The yardstick bar is the project's precedent (tests/test_gpu_gn_cl.py, tests/test_gpu_resnet_cl.py): the error the STOCK fp32 route
(F.batch_norm -> relu on the same device and the same inputs, bn_ref.torch_autograd) makes against the same float64 result (tests/bn_ref.py,
itself checked against torch's float64 autograd in tests/test_bn_ref_host.py).  Every tensor -- out, dx, dgamma, dbeta, run_mean, run_var --
must stay within 4 x max(that error, 2^-23).  Metric: max |err| / max |ref| per tensor, no element left out.  In eval mode the running
statistics must be untouched, bit for bit.

The saved-statistics bar does not lean on the yardstick: save_mean and save_invstd, read through the C ABI in train mode, must satisfy
|invstd - ref| <= 2^-23 ref and |mean - ref| <= 2^-23 max(|ref mean|, ref std).  Sums of exact fp32 inputs taken in double are exact to about
2^-50; the statistic is then rounded once to fp32, which costs 2^-24; the factor 2 is the margin.  A variance that loses its digits to the
mean (sum x^2 / count - mean^2 from fp32 sums) cannot pass this, however poor the stock route itself may be at mean 1000.

How the operators are reached: planes through m3t.ops.bn_planes with autograd (the saved statistics and the unaligned cases through the C
ABI); rows through the C ABI only (their one caller, _TcnSimple, welds them to a convolution), with relu 0 and 1.

Inputs are drawn clear of ReLU flips (bn_ref.clear_of_flips: a pre-activation within fp32 rounding of zero flips its mask in ANY fp32 route
and is no error of the operator), seeds tried in steps of 1000 from 0, at most 8.  With the margins of bn_ref every case takes its first seed
except (33, 4, 8196) in both modes and (2, 4, 1023) in eval mode: seed 0 skipped, 1000 taken.  Rows (8200, 512) -- 4.2 M pre-activations -- cannot clear within 8 draws
(tests/test_bn_ref_host.py shows it) and run without the ReLU.  The large-mean inputs run without the ReLU too: at mean 1000 the mean's own
fp32 rounding moves every pre-activation by about 3e-5, so flips would be dense.

NaN: the float64 reference decides which outputs are NaN (g = dy (y > 0) is 0 where y is NaN, so dbeta stays finite with the ReLU on; 0 x NaN
keeps dgamma NaN); the test asserts that pattern, whatever it is.

Measured on the MI355X (worst chain / stock error ratio per kind, the bar being 4):
  planes, 14 cases x 2 modes and the two unaligned ones:
    out 1.26 ((2, 4, 8192) eval), dx 1.09 ((5, 8, 3) train), dgamma 1.36, dbeta 1.46 ((2, 8, 784) eval), run_mean 0.85, run_var 0.59;
  rows: out 0.99, dx 0.99, dgamma 0.98 (all (2, 64) train, where dx cancels to 5e-5 of its terms in either route), dbeta 0.44, run_mean 0.95,
    run_var 0.68;
  large mean: out 0.50, dx 0.95, dgamma 0.62, dbeta 0.76, run_mean 0.66, run_var 0.60 -- the rows at mean 1000; the planes stay below 0.01,
    because the stock route on this device is itself poor there (its out errs by 1e-4 at mean 30 and by 3.5e-2 .. 8e-2 at mean 1000);
  saved statistics (x 2^-23, the bar being 1): invstd <= 0.49, mean <= 0.50 over every case, the large means included.
The backward sums of the plane kernels (fp32 per thread) needed no change: dgamma and dbeta stay below 1.5.

The large-mean cases on the parent commit, whose plane kernels summed x and x^2 in fp32 per thread before widening (same inputs, same run):
  | case, mean        | parent invstd error | this commit | parent out error | this commit |
  | (6, 8, 784), 30   | 230 x 2^-23         | 0.43        | 1.11e-5          | 2.46e-7     |
  | (70, 8, 16), 30   | 71.3                | 0.43        | 4.47e-6          | 1.78e-7     |
  | (2, 4, 8196), 30  | 17.3                | 0.25        | 1.73e-6          | 1.81e-7     |
  | (6, 8, 784), 1000 | 2.92e5 (3.5 %)      | 0.24        | 1.34e-2          | 7.09e-6     |
  | (70, 8, 16), 1000 | 3.3e4               | 0.36        | 1.72e-3          | 1.92e-6     |
  | (2, 4, 8196), 1000| 8.0e3               | 0.15        | 7.87e-4          | 5.01e-6     |
  | rows (129, 64)    | 0.49 / 0.45         | the same (the row kernels were fp64 from the first add already)          |
All six plane cases FAIL the saved-statistics bar on the parent and pass the yardstick bar there (worst ratio 1.38, dgamma): the stock route's
own error at these means is larger than the parent's.  The parent also misses the saved-statistics bar at ordinary inputs (mean 1, spread
0.7) on three small-plane cases: invstd 1.15 ((5, 8, 3)), 1.16 ((2, 8, 784)), 1.59 ((2, 4, 1023)) x 2^-23.
"""
import pytest
import torch

import bn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FLOOR = 2.0 ** -23
KINDS = ("out", "dx", "dgamma", "dbeta", "run_mean", "run_var")
_ID = lambda c: "x".join(map(str, c))


def rel_err(got, ref):
    """max |got - ref| / max |ref| (as tests/test_gpu_gn_cl.py)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    top = float(ref.abs().max())
    assert top > 0.0 and top == top and top != float("inf"), "the reference is all zero or not finite: the metric would be blind"
    return float((got - ref).abs().max()) / top


def _slot_bits(slot):
    return int(slot.view(torch.int64)[0].item())


def _bits_of_max_finite(t):
    a = t.detach().abs()
    a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    return int(a.max().view(torch.int32).item())


def _dev(t):
    return t.float().to(DEV)


def run_ops(inputs, training, relu):
    """the plane kernels through m3t.ops.bn_planes on the GPU, forward and backward by autograd"""
    from m3t import ops
    x, gamma, beta, rm, rv, dy = inputs
    xr, ga, be = (_dev(t).requires_grad_(True) for t in (x, gamma, beta))
    rm_, rv_ = _dev(rm), _dev(rv)
    grads = {}
    xr.register_hook(lambda g: grads.__setitem__("dx", g))
    y = ops.bn_planes(xr, ga, be, rm_, rv_, training, R.MOMENTUM, R.EPS, relu)
    assert type(y.grad_fn).__name__.startswith("_BNPlanes"), type(y.grad_fn).__name__
    tag = getattr(y, "_m3t_amax", None)
    y.backward(_dev(dy))
    torch.cuda.synchronize()
    dx = grads["dx"]
    dx_slot = ops._grad_slot(dx)[0]
    if ops.TRANSPOSE_IMAGES[0]:
        assert tag is not None and dx_slot is not None, "the operator did not hand its magnitude slots over"
    return dict(out=y.detach(), dx=dx, dgamma=ga.grad, dbeta=be.grad, run_mean=rm_, run_var=rv_, y_slot=None if tag is None else tag[0],
                dx_slot=dx_slot)


def run_abi(case, inputs, training, relu, off=0):
    """m3t_bn_planes_* / m3t_bn_rows_* through the C ABI, forward then backward; off: x, y, dy, dx start `off` floats into 16-byte-aligned
    buffers (off = 1: S % 4 == 0 planes must take the scalar sweep).  Also -> mean, invstd: the saved statistics"""
    from m3t import _lib as L
    lib = L.load()
    x, gamma, beta, rm, rv, dy = inputs
    rows = len(case) == 2
    C, n = case[1], x.numel()

    def buf(t=None):
        b = torch.zeros(n + 8, device=DEV)
        assert b.data_ptr() % 16 == 0
        if t is not None:
            b[off:off + n] = _dev(t).flatten()
        return b
    xb, dyb, yb, dxb = buf(x), buf(dy), buf(), buf()
    p = lambda b: b.data_ptr() + 4 * off
    ga, be, rm_, rv_ = (_dev(t) for t in (gamma, beta, rm, rv))
    mean, invstd, dga, dbe = (torch.full((C,), 7.0, device=DEV) for _ in range(4))
    need = int(lib.m3t_bn_rows_ws_bytes(*case) if rows else lib.m3t_bn_planes_ws_bytes(*case))
    ws = torch.zeros(need // 4 + 64, device=DEV)
    nb, s = ws.numel() * 4, torch.cuda.current_stream().cuda_stream
    q = lambda t: t.data_ptr()
    tr, rl = int(training), int(relu)
    if rows:
        rc_f = lib.m3t_bn_rows_fwd(p(xb), case[0], C, q(ga), q(be), q(rm_), q(rv_), R.MOMENTUM, R.EPS, tr, rl, p(yb), q(mean), q(invstd), q(ws), nb, s)
        rc_b = lib.m3t_bn_rows_bwd(p(dyb), p(xb), p(yb), q(ga), q(mean), q(invstd), case[0], C, tr, rl, p(dxb), q(dga), q(dbe), q(ws), nb, s)
    else:
        N, _, S = case
        rc_f = lib.m3t_bn_planes_fwd(p(xb), N, C, S, q(ga), q(be), q(rm_), q(rv_), R.MOMENTUM, R.EPS, tr, rl, p(yb), q(mean), q(invstd), q(ws), nb, s)
        rc_b = lib.m3t_bn_planes_bwd(p(dyb), p(xb), p(yb), q(ga), q(mean), q(invstd), N, C, S, tr, rl, p(dxb), q(dga), q(dbe), q(ws), nb, s)
    torch.cuda.synchronize()
    assert rc_f == 0 and rc_b == 0, (rc_f, rc_b)
    for b in (yb, dxb):          # nothing written in front of or behind the tensor
        assert not bool(b[:off].any()) and not bool(b[off + n:].any()), "a kernel wrote outside its tensor"
    return dict(out=yb[off:off + n].view(x.shape), dx=dxb[off:off + n].view(x.shape), dgamma=dga, dbeta=dbe, run_mean=rm_, run_var=rv_,
                mean=mean, invstd=invstd)


def stock(inputs, training, relu):
    """the stock fp32 route on the same device and inputs"""
    x, gamma, beta, rm, rv, dy = (_dev(t) for t in inputs)
    return R.torch_autograd(x, gamma, beta, rm, rv, training, relu, dy)


def reference_of(inputs, training, relu):
    x, gamma, beta, rm, rv, dy = inputs
    f = R.forward(x, gamma, beta, rm, rv, training, relu)
    b = R.backward(dy, f, gamma, training, relu)
    return dict(inputs=inputs, out=f["y"], run_mean=f["run_mean"], run_var=f["run_var"], mean=f["mean"], invstd=f["invstd"], **b)


_REF = {}


def reference(case, training, relu, mean=1.0, spread=0.7, seed=0):
    """float64 on the CPU, computed once per case, mode and input and shared"""
    key = (case, training, relu, mean, spread, seed)
    if key not in _REF:
        if relu:
            inputs, taken = R.draw_clear(case, training, seed, mean, spread)
            print("\n%s %s: seed %d taken" % (case, "train" if training else "eval", taken))
        else:
            inputs = R.draw(case, seed, mean, spread)
        _REF[key] = reference_of(inputs, training, relu)
    return _REF[key]


def within_the_bar(what, got, stk, ref, training, kinds=KINDS):
    bad, ratios = {}, {}
    for kind in kinds:
        if kind.startswith("run_") and not training:
            assert torch.equal(got[kind].cpu().double(), ref[kind]), "%s: eval mode touched %s" % (what, kind)
            continue
        e_new, e_stock = rel_err(got[kind], ref[kind]), rel_err(stk[kind], ref[kind])
        ratios[kind] = e_new / max(e_stock, FLOOR)
        print("BAR %s %-8s chain %.2e  stock %.2e  ratio %.2f" % (what, kind, e_new, e_stock, ratios[kind]))
        if not e_new <= 4.0 * max(e_stock, FLOOR):
            bad[kind] = (e_new, e_stock)
    assert not bad, "%s: over 4 x max(stock error, 2^-23): %s" % (what, bad)
    return ratios


def statistics_within_rounding(what, got, ref):
    """the saved statistics against one fp32 rounding of the float64 ones (module docstring), in units of 2^-23"""
    mean, invstd = got["mean"].double().cpu(), got["invstd"].double().cpu()
    std = 1.0 / ref["invstd"]
    e_i = float(((invstd - ref["invstd"]).abs() / ref["invstd"]).max()) / FLOOR
    e_m = float(((mean - ref["mean"]).abs() / torch.maximum(ref["mean"].abs(), std)).max()) / FLOOR
    print("STAT %s invstd %.3g  mean %.3g  (x 2^-23, the bar being 1)" % (what, e_i, e_m))
    assert e_i <= 1.0 and e_m <= 1.0, "%s: saved statistics off by (invstd %.3g, mean %.3g) x 2^-23" % (what, e_i, e_m)


def _mode(training):
    return "train" if training else "eval"


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", R.PLANE_CASES, ids=_ID)
def test_planes_against_float64(case, training):
    ref = reference(case, training, True)
    got, stk = run_ops(ref["inputs"], training, True), stock(ref["inputs"], training, True)
    print()
    within_the_bar("%s %s" % (case, _mode(training)), got, stk, ref, training)
    if got["y_slot"] is not None:
        assert _slot_bits(got["y_slot"]) == _bits_of_max_finite(got["out"]) and _slot_bits(got["dx_slot"]) == _bits_of_max_finite(got["dx"])


@pytest.mark.parametrize("case", R.PLANE_CASES, ids=_ID)
def test_plane_saved_statistics(case):
    ref = reference(case, True, True)
    got = run_abi(case, ref["inputs"], True, True)
    print()
    statistics_within_rounding("%s" % (case,), got, ref)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", R.UNALIGNED_CASES, ids=_ID)
def test_unaligned_planes_take_the_scalar_sweep(case, training):
    """x, y, dy, dx one float off a 16-byte boundary: the float4 sweeps would fault or read the wrong floats"""
    ref = reference(case, training, True)
    got, stk = run_abi(case, ref["inputs"], training, True, off=1), stock(ref["inputs"], training, True)
    print()
    within_the_bar("%s +1 %s" % (case, _mode(training)), got, stk, ref, training)
    if training:
        statistics_within_rounding("%s +1" % (case,), got, ref)


_ROW_PARAMS = [(c, t, r) for c in R.ROW_CASES for t in (True, False) for r in (True, False) if not (r and c in R.NO_RELU_CASES)]


@pytest.mark.parametrize("case,training,relu", _ROW_PARAMS, ids=lambda v: _ID(v) if isinstance(v, tuple) else str(int(v)))
def test_rows_against_float64(case, training, relu):
    ref = reference(case, training, relu)
    got, stk = run_abi(case, ref["inputs"], training, relu), stock(ref["inputs"], training, relu)
    what = "rows %s %s relu %d" % (case, _mode(training), relu)
    print()
    within_the_bar(what, got, stk, ref, training)
    if training:
        statistics_within_rounding(what, got, ref)
    else:
        assert torch.equal(got["mean"], got["run_mean"]), "eval mode: the saved mean is the running mean"


@pytest.mark.parametrize("mean", R.LARGE_MEANS, ids=lambda m: "mean%d" % m)
@pytest.mark.parametrize("case", R.LARGE_MEAN_CASES, ids=_ID)
def test_large_mean_input(case, mean):
    """x = mean + N(0, 1), train mode, no ReLU: the variance must not lose its digits to the mean.  Both bars."""
    ref = reference(case, True, False, mean, 1.0, 1)
    stk = stock(ref["inputs"], True, False)
    abi = run_abi(case, ref["inputs"], True, False)
    got = abi if len(case) == 2 else run_ops(ref["inputs"], True, False)
    what = "%s mean %d" % (case, mean)
    print()
    failed = []
    for check in (lambda: within_the_bar(what, got, stk, ref, True), lambda: statistics_within_rounding(what, abi, ref)):
        try:
            check()
        except AssertionError as e:          # (both bars are measured and printed before either fails the test)
            failed.append(str(e))
    assert not failed, failed


@pytest.mark.parametrize("case", [(2, 8, 784), (2, 4, 8196), (129, 64)], ids=_ID)
def test_constant_channel(case):
    """channel 2 is 1.5 throughout: the sums are exact, the variance is exactly 0 and invstd = 1 / sqrt(eps): finite outputs and dx, and
    y = relu(beta) there (beta = 0.75 on channel 2; a second input with beta = -0.75 gives 0)"""
    for b in (0.75, -0.75):
        inputs = R.draw(case, 2)
        inputs[0][:, 2] = 1.5          # (rows [M, C] and planes [N, C, S]: the channel is dimension 1 in both)
        inputs[2][2] = b
        got = run_abi(case, inputs, True, True)
        for kind in KINDS + ("mean", "invstd"):
            assert bool(torch.isfinite(got[kind]).all()), kind
        ch = got["out"][:, 2] if len(case) == 2 else got["out"][:, 2, :]
        assert bool((ch == max(b, 0.0)).all())
        assert float(got["mean"][2]) == 1.5
        want = (1.0 / torch.sqrt(torch.tensor(R.EPS, dtype=torch.float32).double())).float()
        assert float(got["invstd"][2]) == float(want), (float(got["invstd"][2]), float(want))
        if len(case) == 3:
            ops_got = run_ops(inputs, True, True)
            for kind in KINDS:
                assert torch.equal(ops_got[kind], got[kind]), kind         # (the same kernels on the same aligned inputs)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("case", [(3, 12, 49), (9, 8, 12), (2, 4, 8196), (129, 64)], ids=_ID)
def test_nan_in_one_plane_follows_the_reference(case, relu):
    """one NaN in channel 1: the NaN pattern of every output equals the float64 reference's, whatever it is; the other channels are finite"""
    inputs = R.draw(case, 3)
    x = inputs[0]
    if len(case) == 2:
        x[case[0] // 2, 1] = float("nan")
    else:
        x[case[0] - 1, 1, case[2] // 2] = float("nan")
    ref = reference_of(inputs, True, relu)
    got = run_abi(case, inputs, True, relu) if len(case) == 2 else run_ops(inputs, True, relu)
    poisoned = 0
    for kind in KINDS:
        g, r = got[kind].cpu(), ref[kind]
        assert torch.equal(torch.isnan(g), torch.isnan(r)), kind
        assert bool(torch.isfinite(g[~torch.isnan(g)]).all()), kind
        poisoned += int(torch.isnan(r).any())
        others = g.clone()
        if g.dim() == 1:
            others[1] = 0.0
        else:
            others[:, 1] = 0.0          # (rows [M, C] and planes [N, C, S]: the channel is dimension 1 in both)
        assert bool(torch.isfinite(others).all()), "%s: a NaN left channel 1" % kind
    # not vacuous: the reference has NaN in out, dx, dgamma and both running statistics -- and a finite dbeta (a plain sum of dy, masked or not)
    assert bool(torch.isnan(ref["out"]).any()) and bool(torch.isnan(ref["dx"]).any()) and bool(torch.isnan(ref["dgamma"][1]))
    assert bool(torch.isnan(ref["run_mean"][1])) and bool(torch.isnan(ref["run_var"][1]))
    assert poisoned == 5 and not bool(torch.isnan(ref["dbeta"]).any())
    if got.get("y_slot") is not None:
        assert _slot_bits(got["y_slot"]) == _bits_of_max_finite(got["out"]) and _slot_bits(got["dx_slot"]) == _bits_of_max_finite(got["dx"])


@pytest.mark.parametrize("case", [(70, 8, 16), (33, 4, 8196), (16400, 8)], ids=_ID)
def test_two_runs_are_bit_identical(case):
    ref = reference(case, True, True)
    run = (lambda: run_abi(case, ref["inputs"], True, True)) if len(case) == 2 else (lambda: run_ops(ref["inputs"], True, True))
    a, b = run(), run()
    for kind in KINDS:
        assert torch.equal(a[kind], b[kind]), kind


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("case", [(70, 8, 16), (2, 4, 8196)], ids=_ID)
def test_slots_hold_the_largest_finite_magnitude(case, relu):
    """with ops.TRANSPOSE_IMAGES[0] on, the slot handed out with y and with dx (ops._grad_slot(dx)) holds the bits of the largest finite
    magnitude -- the next convolution's operand scale"""
    from m3t import ops
    assert ops.TRANSPOSE_IMAGES[0], "the suite runs with the default switches"
    ref = reference(case, True, relu)
    got = run_ops(ref["inputs"], True, relu)
    assert _slot_bits(got["y_slot"]) == _bits_of_max_finite(got["out"])
    assert _slot_bits(got["dx_slot"]) == _bits_of_max_finite(got["dx"])
