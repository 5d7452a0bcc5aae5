"""Host side of the BatchNorm float64 bar (tests/test_gpu_bn_fp64.py): no GPU.

  * tests/bn_ref.py -- the float64 restatement the GPU tests compare csrc/bn.hip's kernels with -- agrees with torch's float64 autograd on the
    CPU to 1e-12 relative: planes and rows, train and eval mode, with and without the ReLU, running statistics included;
  * clear_of_flips rejects an input with one pre-activation planted at exactly 0, and its margin grows with the input's own magnitude;
  * every case of the GPU test finds an input clear of ReLU flips within 8 seeds, from the float64 values alone (the one case that runs
    without the ReLU, bn_ref.NO_RELU_CASES, is shown not to)."""
import pytest
import torch

import bn_ref as R

_ID = lambda c: "x".join(map(str, c))


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape, (tuple(a.shape), tuple(b.shape))
    top = float(b.abs().max())
    return float((a - b).abs().max()) <= tol * max(top, 1e-300)


@pytest.mark.parametrize("relu", [True, False], ids=["relu", "plain"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", [(5, 8, 3), (3, 12, 49), (129, 64)], ids=_ID)
def test_reference_agrees_with_torch_float64(case, training, relu):
    x, gamma, beta, rm, rv, dy = R.draw(case, 5)
    f = R.forward(x, gamma, beta, rm, rv, training, relu)
    b = R.backward(dy, f, gamma, training, relu)
    t = R.torch_autograd(x, gamma, beta, rm, rv, training, relu, dy)
    assert _close(f["y"], t["out"])
    for kind in ("dx", "dgamma", "dbeta"):
        assert _close(b[kind], t[kind]), kind
    assert _close(f["run_mean"], t["run_mean"]) and _close(f["run_var"], t["run_var"])
    if training:
        assert not torch.equal(f["run_mean"], rm) and not torch.equal(f["run_var"], rv)
    else:
        assert torch.equal(f["run_mean"], rm) and torch.equal(f["run_var"], rv)
    assert f["mean"].shape == (case[1],) and f["invstd"].shape == (case[1],)


def test_rows_are_planes_transposed():
    x, gamma, beta, rm, rv, dy = R.draw((37, 6), 2)
    f2 = R.forward(x, gamma, beta, rm, rv, True)
    f3 = R.forward(x.t()[None].contiguous(), gamma, beta, rm, rv, True)
    # (the same formulas over another memory order: torch's sums may differ in their last bits)
    assert _close(f2["y"], f3["y"][0].t(), 1e-14) and _close(f2["mean"], f3["mean"], 1e-14) and _close(f2["run_var"], f3["run_var"], 1e-14)
    b2, b3 = R.backward(dy, f2, gamma, True), R.backward(dy.t()[None].contiguous(), f3, gamma, True)
    assert _close(b2["dx"], b3["dx"][0].t(), 1e-13) and _close(b2["dgamma"], b3["dgamma"], 1e-13)


def test_draw_is_fp32_representable_and_centred():
    x, gamma, beta, rm, rv, dy = R.draw((6, 8, 784), 1, 1000.0, 1.0)
    for t in (x, gamma, beta, rm, rv, dy):
        assert t.dtype == torch.float64 and torch.equal(t.float().double(), t)
    assert abs(float(x.mean()) - 1000.0) < 0.1 and abs(float(x.std()) - 1.0) < 0.05 and bool((rv > 0).all())


@pytest.mark.parametrize("case", [(3, 12, 49), (129, 64)], ids=_ID)
def test_clear_of_flips_rejects_a_planted_zero(case):
    (x, gamma, beta, rm, rv, dy), _ = R.draw_clear(case, False)
    assert R.clear_of_flips(x, gamma, beta, rm, rv, False)
    beta = beta.clone()
    x = x.clone()
    beta[3] = 0.0
    if x.dim() == 3:
        x[1, 3, 7] = rm[3]
    else:
        x[7, 3] = rm[3]
    assert float(R.forward(x, gamma, beta, rm, rv, False)["pre"].abs().min()) == 0.0
    assert not R.clear_of_flips(x, gamma, beta, rm, rv, False)


def test_margin_grows_with_the_input_magnitude():
    """the same deviations around 1000 instead of 1: the fp32 mean's own rounding moves every pre-activation by ~ 1000 x 2^-24 invstd gamma"""
    case = (6, 8, 784)
    lo, hi = R.draw(case, 1, 1.0, 1.0), R.draw(case, 1, 1000.0, 1.0)
    m = lambda i: R.margin(i[0], R.forward(*i[:5], True), i[1], i[2])
    ratio = float(m(hi).median() / m(lo).median())
    assert 100.0 < ratio < 2000.0, ratio


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("case", [c for c in R.PLANE_CASES + R.ROW_CASES if c not in R.NO_RELU_CASES], ids=_ID)
def test_cases_find_a_clear_draw_within_the_cap(case, training):
    inputs, taken = R.draw_clear(case, training)
    print("\n%s %s: seed %d taken" % (case, "train" if training else "eval", taken))
    assert taken < 8000


def test_the_case_without_relu_cannot_clear():
    """4.2 M pre-activations: some lie within fp32 rounding of zero in every one of the 8 draws, so the GPU test runs this case without the
    ReLU rather than with more tries (train mode shown here; the GPU test drops the ReLU in both modes)"""
    for case in R.NO_RELU_CASES:
        with pytest.raises(AssertionError, match="no input clear"):
            R.draw_clear(case, True)
