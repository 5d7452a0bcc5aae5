"""The float64 reference of the optimizer tests (tests/optim_ref.py) pinned against torch, and the single-step error bounds
of tests/test_gpu_optim_fp64.py evaluated on the fp32 yardstick instead of the GPU.  No GPU needed."""
import numpy as np
import pytest
import torch

import optim_ref as R

# exactly representable in fp32, so that the reference's "round every hyperparameter to fp32 first" changes nothing
LR, B1, B2, EPS, WD, MOM = 2.0 ** -10, 0.875, 0.9990234375, 2.0 ** -27, 2.0 ** -13, 0.875


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _grads(n, steps, seed):
    rs = np.random.RandomState(seed)
    return [rs.standard_normal(n) * 10.0 ** rs.uniform(-3, 0, n) for _ in range(steps)]


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_reference_is_torch_optim_in_float64(kind):
    n = 1001
    p0 = np.random.RandomState(0).standard_normal(n)
    q = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    if kind == "adam":
        opt = torch.optim.Adam([q], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
        st = [np.zeros(n), np.zeros(n)]
    else:
        opt = torch.optim.SGD([q], lr=LR, momentum=MOM, weight_decay=WD)
        st = [np.zeros(n)]
    p = p0
    for t, g in enumerate(_grads(n, 20, 1), 1):
        q.grad = torch.from_numpy(g.copy())
        opt.step()
        out = R.adam_step(p, g, st[0], st[1], t, LR, B1, B2, EPS, WD) if kind == "adam" else R.sgd_step(p, g, st[0], t, LR, MOM, WD)
        p, st = out[0], list(out[1:])
        assert _rel(p, q.detach().numpy()) <= 1e-14, (t, _rel(p, q.detach().numpy()))
    state = opt.state[q]
    if kind == "adam":
        assert _rel(st[0], state["exp_avg"].numpy()) <= 1e-14 and _rel(st[1], state["exp_avg_sq"].numpy()) <= 1e-14
    else:
        assert _rel(st[0], state["momentum_buffer"].numpy()) <= 1e-14
    assert _rel(p, p0) > 1e-3           # (the parameters really moved)


@pytest.mark.parametrize("world", [1, 2, 8])
@pytest.mark.parametrize("max_norm,scale", [(1.0, 3.0), (1.0, 0.01), (0.125, 1.0), (0.0, 5.0)])
def test_reference_clip_is_torch_clip_grad_norm(world, max_norm, scale):
    g = np.random.RandomState(world).standard_normal(4099) * scale
    q = torch.nn.Parameter(torch.zeros(4099, dtype=torch.float64))
    q.grad = torch.from_numpy(g / world)
    norm = float(np.linalg.norm(g / world))
    if max_norm > 0:
        tn = torch.nn.utils.clip_grad_norm_([q], max_norm)
        assert abs(float(tn) - norm) <= 1e-14 * norm
    out, got_norm = R.norm_scale(g, world, max_norm)
    assert abs(float(got_norm) - norm) <= 1e-14 * norm
    assert _rel(out, q.grad.numpy()) <= 1e-14
    clipped = max_norm > 0 and norm + 1e-6 > max_norm
    assert (abs(float(np.linalg.norm(out)) - max_norm) <= 2e-6 * max_norm) == clipped


def test_hyperparameters_are_rounded_to_fp32_once():
    """float(0.999) = 0.99900001287...: the reference runs on that value, as the library does, not on the decimal one"""
    p, g, z = np.ones(4), np.full(4, 0.5), np.zeros(4)
    a = R.adam_step(p, g, z, z, 7, 5e-5, 0.9, 0.999, 1e-8, 1e-4)
    b = R.adam_step(p, g, z, z, 7, R.f32(5e-5), R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(1e-4))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    v_dec = (1 - 0.999) * (0.5 + 1e-4) ** 2
    assert 1e-6 < abs(a[2][0] - v_dec) / v_dec < 1e-4


def _worst(kind, cases):
    worst = (0.0, "")
    for c in cases:
        p, g, st = R.make_state(kind, c["n"], c["g_scale"], c["state"], c["hyper"], c["seed"])
        got = R.step_ref(kind, p, g, st, c["t"], c["hyper"], dtype=np.float32)
        assert all(a.dtype == np.float32 for a in got)
        w, msg = R.check_step(kind, got, p, g, st, c["t"], c["hyper"])
        assert w <= 1.0, "the fp32 yardstick leaves the single-step bound: %s %s (%.3g x)" % (c["name"], msg, w)
        worst = max(worst, (w, c["name"] + " " + msg))
    return worst


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_fp32_yardstick_stays_inside_the_single_step_bound_grid(kind):
    """step number x hyperparameters x gradient magnitude x state at n = 4099: 300 cases.  The bound (optim_ref docstring) is
    not tighter than fp32 arithmetic allows; the final rounding of p' alone uses up to 1.0 of it."""
    w, where = _worst(kind, R.grid_cases(kind))
    assert w > 0.25, "the bound is more than 4x away from what fp32 arithmetic does: %s" % where


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_fp32_yardstick_stays_inside_the_single_step_bound_sizes(kind):
    # (the two multi-sweep sizes once each: on the CPU a later step of a large buffer costs seconds and exercises nothing new)
    _worst(kind, [c for c in R.size_cases(kind) if c["n"] < 3000000 or c["t"] == 1])


def test_bounds_follow_the_terms_not_the_result():
    """cancellation in b1*m + (1-b1)*g~ (and in g + wd*p) must not make a bound vanish"""
    h = R.ADAM_DEFAULT
    m = np.array([1.0], np.float32)
    g = np.array([-9.0], np.float32)                 # 0.9*1 + 0.1*(-9 + 1e-4*0) = 0
    p = np.zeros(1, np.float32)
    e_m, e_v, e_p = R.adam_bounds(p, g, m, np.ones(1, np.float32), 10, **h)
    assert e_m[0] >= R.C_M * R.U * 1.8 * 0.999 and e_p[0] > 0
    e_b, e_p = R.sgd_bounds(np.array([1.0], np.float32), np.array([-5e-4], np.float32), np.zeros(1, np.float32), 1, **R.SGD_DEFAULT)
    assert e_b[0] >= R.C_BUF * R.U * 1e-3 * 0.999
