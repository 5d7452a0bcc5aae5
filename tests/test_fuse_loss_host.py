"""tests/fuse_loss_ref.py without a GPU: the float64 reference of the VA loss and the attention fusion against torch's own float64
autograd of the literal composition, the goldens and the existing oracle; the arithmetic of the three loss forms, restated in numpy,
against the bound the GPU tests assert (it must hold half of it, so that the bound is not tighter than that arithmetic allows); and
the comparison helper against results that are deliberately off."""
import numpy as np
import pytest
import torch

import fuse_loss_ref as R
from conftest import load_golden
from oracle import m3t_oracle as O

SEEDS = 20
EMU_ROWS = {"one": (1, 2, 65, 1024, 2500), "fused": (1025, 4097), "three": (33000,)}


def _rel(a, b, what, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=what)
    ok = ~np.isnan(b)
    if ok.any():
        scale = float(np.abs(b[ok]).max())
        assert float(np.abs(a[ok] - b[ok]).max()) <= tol * max(scale, 1e-300), "%s: %.3e of %.3e" % (what, np.abs(a[ok] - b[ok]).max(), scale)


# ------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("rows", [1, 2, 65, 300])
def test_va_reference_equals_torch_float64_autograd(rows):
    """the whole option matrix (layouts x use_mse x weights, label classes, statistics classes): the eight scalars and dy to 1e-12
    of each tensor's largest value.  rows == 1: the composition with the library's max(n - 1, 1) divisor."""
    cases = R.option_cases(rows)
    assert len(cases) > 50
    for c in cases:
        out, dy = R.va_loss(*R.case_args(c))
        t_out, t_dy = R.va_loss_torch(*R.case_args(c), dtype=torch.float64)
        for k, nm in enumerate(R.OUT_NAMES):
            _rel(out[k], t_out[k], c["name"] + " " + nm)
        groups, free = R.dy_groups(dy.shape[1], c["iv"], c["ia"], c["n_expr"], R.f32(c["w_v"]), R.f32(c["w_a"]))
        for nm, sl in groups:
            _rel(dy[:, sl], t_dy[:, sl], c["name"] + " " + nm)
        assert not np.count_nonzero(dy[:, free]) and not np.count_nonzero(t_dy[:, free])


def test_va_reference_zero_weight_skips_its_term():
    c = R.make_case(65, "gaps12", (0.0, 1.0, 0.8))
    c["y"][3, c["iv"]] = np.nan
    out, dy = R.va_loss(*R.case_args(c))
    assert np.isfinite(out[[0, 1, 2, 3]]).all() and np.isfinite(dy).all() and np.isnan(out[6]) and not np.count_nonzero(dy[:, c["iv"]])
    c = R.make_case(65, "mtl9", (0.5, 0.5, 0.0))
    c["y"][3, 2] = np.nan
    out, dy = R.va_loss(*R.case_args(c))
    assert np.isfinite(out[[0, 1, 2]]).all() and np.isfinite(dy).all() and not np.count_nonzero(dy[:, :7])


def test_va_reference_one_row_rule():
    c = R.make_case(1, "va2")
    out, dy = R.va_loss(*R.case_args(c))
    assert out[6] == 0 and out[7] == 0 and out[1] == 1 and out[2] == 1 and out[0] == 1 and not np.count_nonzero(dy)
    c["y"][0, 0] = c["valence"][0]                                     # prediction == target: 0 / 0
    out, dy = R.va_loss(*R.case_args(c))
    assert np.isnan(out[6]) and np.isnan(dy[0, 0]) and out[7] == 0 and dy[0, 1] == 0


@pytest.mark.parametrize("rows,D", [(1, 1), (5, 3), (2, 64), (7, 65), (3, 260)])
def test_att_reference_equals_torch_float64_autograd(rows, D):
    df, sv, sa, xv, xa = R.make_att(rows, D, seed=rows + D, score_scale=3.0)
    t = R.att_fuse_torch(df, sv, sa, xv, xa, dtype=torch.float64)
    _rel(R.att_fuse_fwd(sv, sa, xv, xa), t["f"], "f")
    for got, nm in zip(R.att_fuse_bwd(df, sv, sa, xv, xa), ("ds_v", "ds_a", "dx_v", "dx_a")):
        _rel(got, t[nm], nm)


def test_att_reference_saturated_scores():
    s = np.array([0.0, 30.0, -30.0, 100.0, -100.0, np.inf, -np.inf], np.float32)
    df, _, _, xv, xa = R.make_att(s.size, 5, seed=3)
    hv, ha, w0, w1 = R.att_weights(s, s[::-1].copy())
    e = np.e
    assert (w0 >= 1 / (1 + e) - 1e-16).all() and (w0 <= e / (1 + e) + 1e-16).all() and np.allclose(w0 + w1, 1, atol=1e-15)
    ds_v = R.att_fuse_bwd(df, s, s[::-1].copy(), xv, xa)[0]
    assert np.isfinite(ds_v).all() and (ds_v[[3, 5, 6]] == 0).all()           # float64: 1 - h is 0 from s = 37 on, h is 0 only at -inf
    t = R.att_fuse_torch(df, s, s[::-1].copy(), xv, xa, dtype=torch.float64)
    _rel(ds_v, t["ds_v"], "ds_v", tol=1e-9)
    sn = s.copy()
    sn[2] = np.nan
    f = R.att_fuse_fwd(sn, s, xv, xa)
    assert np.isnan(f[2]).all() and np.isfinite(np.delete(f, 2, axis=0)).all()


# ------------------------------------------------------------------------------------------------- goldens and the oracle
def test_reference_reproduces_the_losses_golden():
    """fp32 torch results of the reference's own training_step: 1e-6 of each tensor's largest value (a dozen fp32 roundings)"""
    g = load_golden("losses")
    yh = g["y_hat"].reshape(-1, 9)
    out, dy = R.va_loss(yh, g["valence"], g["arousal"], g["class_expr"], g["expr_valid"], 7, 8, 7, 0.5, 0.5, 0.8, 0)
    for k, nm in ((0, "loss"), (1, "loss_v"), (2, "loss_a"), (3, "loss_expr"), (6, "ccc_v")):
        _rel(out[k], g[nm], nm, tol=1e-6)
    _rel(dy.reshape(g["dy_hat"].shape), g["dy_hat"], "dy_hat", tol=1e-6)
    assert out[4] == g["expr_valid"].sum()


@pytest.mark.parametrize("name", ["attfusion_same", "attfusion_proj"])
def test_reference_reproduces_the_attfusion_goldens(name):
    """AttFusion of the reference with the oracle's GRU scorers around this file's reduction (in place of the oracle's own)"""
    g = load_golden(name)
    p = {k[2:]: v.astype(np.float64) for k, v in g.items() if k.startswith("p.")}
    x_a, x_v = g["x_a"].astype(np.float64), g["x_v"].astype(np.float64)
    xv_in = x_v
    if "proj_v.weight" in p:
        x_v = O.linear_fwd(x_v, p["proj_v.weight"], p["proj_v.bias"])
    pv = {k[len("scorer_v."):]: v for k, v in p.items() if k.startswith("scorer_v.")}
    pa = {k[len("scorer_a."):]: v for k, v in p.items() if k.startswith("scorer_a.")}
    s_v, _, cv = O.gru_module_fwd(x_v, pv, 1, 1, 1)
    s_a, _, ca = O.gru_module_fwd(x_a, pa, 1, 1, 1)
    B, T, D = x_a.shape
    flat = lambda a: a.reshape(B * T, -1)
    f = R.att_fuse_fwd(s_v.reshape(-1), s_a.reshape(-1), flat(x_v), flat(x_a)).reshape(B, T, D)
    _rel(f, g["y"], "y", tol=2e-5)
    ds_v, ds_a, dx_v, dx_a = R.att_fuse_bwd(flat(g["ct"].astype(np.float64)), s_v.reshape(-1), s_a.reshape(-1), flat(x_v), flat(x_a))
    dx_v = dx_v.reshape(B, T, D) + O.gru_module_bwd(ds_v.reshape(B, T, 1), cv, pv, 1)[0]
    dx_a = dx_a.reshape(B, T, D) + O.gru_module_bwd(ds_a.reshape(B, T, 1), ca, pa, 1)[0]
    if "proj_v.weight" in p:
        dx_v = O.linear_bwd(dx_v, xv_in, p["proj_v.weight"])[0]
    _rel(dx_a, g["dx_a"], "dx_a", tol=2e-5)
    _rel(dx_v, g["dx_v"], "dx_v", tol=2e-5)


def test_reference_equals_the_oracle_where_they_overlap():
    """oracle/m3t_oracle.py has the ccc / ccc_mtl objective at the default weights and the fusion core; no mse, no other layout"""
    for lam in (0.5, 0.25):                                            # (weights that fp32 holds exactly)
        c = R.make_case(150, "mtl9", (lam, 1 - lam, 0.8), seed=5)
        out, dy = R.va_loss(*R.case_args(c))
        d = lambda a: a.astype(np.float64)
        l, parts, dy_o = O.training_loss_fwd_bwd(d(c["y"]), d(c["valence"]), d(c["arousal"]), c["class_expr"], c["expr_valid"].astype(bool),
                                                 loss_lambda=lam)
        k = R.f32(0.8) / 0.8                                           # the oracle's 0.8 is the decimal, the library's the fp32 value
        _rel(out[0], l + (k - 1) * 0.8 * parts["loss_expr"], "loss"); _rel(out[1], parts["loss_v"], "loss_v")
        _rel(out[2], parts["loss_a"], "loss_a"); _rel(out[3], parts["loss_expr"], "loss_expr")
        _rel(dy[:, 7:], dy_o[:, 7:], "dy"); _rel(dy[:, :7], k * dy_o[:, :7], "dy[ce]")
    c = R.make_case(150, "va2", seed=6)
    out, dy = R.va_loss(*R.case_args(c))
    l, parts, dy_o = O.training_loss_fwd_bwd(c["y"].astype(np.float64), c["valence"].astype(np.float64), c["arousal"].astype(np.float64), mtl=False)
    _rel(out[0], l, "loss (ccc)"); _rel(dy, dy_o, "dy (ccc)")
    _rel(out[6], O.concordance_cc2(c["y"][:, 0].astype(np.float64), c["valence"].astype(np.float64)), "ccc_v")
    c = R.make_case(150, "ce7", seed=7)
    out, dy = R.va_loss(*R.case_args(c))
    l, dl = O.masked_ce_fwd_bwd(c["y"].astype(np.float64), c["class_expr"], c["expr_valid"])
    _rel(out[0], l, "ce_loss"); _rel(dy, dl, "d ce_loss")
    df, sv, sa, xv, xa = (a.astype(np.float64) for a in R.make_att(9, 33, seed=8))
    f_o, cache = O.att_fuse_core_fwd(sv[:, None], sa[:, None], xv, xa)
    _rel(R.att_fuse_fwd(sv, sa, xv, xa), f_o, "f")
    for got, want, nm in zip(R.att_fuse_bwd(df, sv, sa, xv, xa), O.att_fuse_core_bwd(df, cache), ("ds_v", "ds_a", "dx_v", "dx_a")):
        _rel(got, want.reshape(got.shape), nm)


def test_workspace_size_covers_the_fp64_partials():
    """16 doubles per 256-row block: what the one-launch form writes (it used to be promised 16 floats) and the three-launch form's
    two 8-double parts"""
    from m3t import _lib
    lib = _lib.load()
    for rows in (1, 256, 257, 1025, 32768, 33000):
        assert lib.m3t_va_loss_ws_bytes(rows) == -(-rows // 256) * 16 * 8
    assert lib.m3t_va_loss_ws_bytes(0) == 0


# ------------------------------------------------------------------------------------------------- the forms' arithmetic
def _emu_classes():
    out = [(s, m, "mixed") for s in R.STATS for m in (0, 1)]
    return out + [("normal", 0, lb) for lb in R.LABELS[1:]]


@pytest.mark.parametrize("form", ["one", "fused", "three"])
def test_emulated_forms_hold_half_the_bound(form):
    """numpy restatements of the three forms' arithmetic (fuse_loss_ref.va_loss_emulated) stay within HALF the bound (ratio <= 2) on
    every input class the GPU file uses, 20 seeds each, at the ends of each form's row range: the bound is not tighter than the
    arithmetic allows, and the GPU (other expf / logf, contraction) keeps a factor 2 of room.  Measured: 0.50 on every regression
    output (they are correctly rounded), up to 1.84 on the fp32 cross-entropy gradient, 1.66 on the loss.  R.admitted() would take a
    (form, class) pair out of the GPU file if its emulation could not hold this; none is out."""
    worst = (0.0, "")
    for rows in EMU_ROWS[form]:
        for stats, use_mse, labels in _emu_classes():
            assert R.admitted(form, stats, use_mse)
            for seed in range(SEEDS):
                c = R.make_case(rows, "mtl9", (0.3, 0.7, 0.8), use_mse, stats=stats, labels=labels, seed=seed)
                out, dy = R.va_loss_emulated(form, *R.case_args(c))
                r = R.check_va(out, dy, c)
                assert r[0] <= R.BOUND / 2, "%s %s seed %d: %s" % (form, c["name"], seed, r[1])
                worst = max(worst, r)
    print("%s: worst error / max(E32, floor) of the emulation = %.3f (half the bound: 2)  %s" % (form, worst[0], worst[1]))


def test_fp32_sums_would_break_the_bound():
    """why the forms sum in fp64: their former arithmetic -- fp32 block partials added in block order (three launches), fp32 strided
    sums and an fp32 closed form (one workgroup) -- restated in numpy, exceeds the bound itself on classes the GPU file runs"""
    c = R.make_case(33000, "mtl9", (0.3, 0.7, 0.8), stats="const", seed=0)
    r3 = R.check_va(*R.va_loss_emulated_fp32("three", *R.case_args(c)), c)
    r1 = (0.0, "")
    for seed in range(SEEDS):
        c = R.make_case(2, "mtl9", (0.3, 0.7, 0.8), stats="offset", seed=seed)
        r1 = max(r1, R.check_va(*R.va_loss_emulated_fp32("one", *R.case_args(c)), c))
    print("fp32 three-launch arithmetic, constant column, 33 000 rows: %.1f x;  fp32 one-workgroup, 0.8 + 1e-3 N, 2 rows: %.1f x" % (r3[0], r1[0]))
    assert r3[0] > R.BOUND and r1[0] > R.BOUND


# ------------------------------------------------------------------------------------------------- the helper can fail
def test_helper_rejects_a_result_that_is_off():
    c = R.make_case(300, "gaps12", (0.3, 0.7, 0.8), seed=11)
    a = R.case_args(c)
    out, dy, f_out, f_dy = R.va_loss(*a, floors=True)
    y_out, y_dy = R.va_loss_torch(*a)
    assert R.check_va(out, dy, c)[0] == 0.0
    assert R.check_va(*R.va_loss_emulated("one", *a), c)[0] <= 2.0
    for col in (0, c["iv"], c["ia"]):                                  # one element of each dy tensor moved by 8 units
        sl = slice(0, c["n_expr"]) if col == 0 else slice(col, col + 1)
        e32 = np.abs(y_dy[:, sl] - dy[:, sl]).max()
        bad = dy.copy()
        bad[17, col] += 8 * max(e32, R.ulp32(f_dy[17, col]))
        r = R.check_va(out, bad, c)
        assert 7.9 <= r[0] <= 8.1, r
    for k in (0, 1, 3, 6):                                             # ... of a scalar
        bad = out.copy()
        bad[k] += 8 * max(abs(y_out[k] - out[k]), R.ulp32(f_out[k]))
        assert 7.9 <= R.check_va(bad, dy, c)[0] <= 8.1
    bad = out.copy()
    bad[5] += 1                                                        # counts are exact or wrong
    assert R.check_va(bad, dy, c)[0] == float("inf")
    bad = dy.copy()
    bad[3, 8] = 1e-30                                                  # a column no term owns
    assert R.check_va(out, bad, c)[0] == float("inf")
    bad = dy.copy()
    bad[3, c["iv"]] = np.nan
    assert R.check_va(out, bad, c)[0] == float("inf")
    bad = dy.copy()
    bad[:, c["iv"]] *= 1.01                                            # the 1 % error the old absolute bars let through
    assert R.check_va(out, bad, c)[0] > 1000


def test_helper_rejects_an_att_fuse_result_that_is_off():
    df, sv, sa, xv, xa = R.make_att(5, 65, seed=12)
    ds_v, ds_a, dx_v, dx_a, fl_v, fl_a = R.att_fuse_bwd(df, sv, sa, xv, xa, floors=True)
    good = dict(f=R.att_fuse_fwd(sv, sa, xv, xa), ds_v=ds_v, ds_a=ds_a, dx_v=dx_v, dx_a=dx_a)
    yard = R.att_fuse_torch(df, sv, sa, xv, xa)
    assert R.check_att(good, df, sv, sa, xv, xa)[0] == 0.0
    assert R.check_att({k: v.astype(np.float32) for k, v in good.items()}, df, sv, sa, xv, xa)[0] <= 1.0      # rounding the reference
    for k, fl in (("f", None), ("dx_a", None), ("ds_v", fl_v), ("ds_a", fl_a)):
        bad = {n: v.copy() for n, v in good.items()}
        i = (2, 7) if bad[k].ndim == 2 else (2,)
        unit = max(np.abs(yard[k] - good[k]).max(), R.ulp32((good[k] if fl is None else fl)[i]))
        bad[k][i] += 8 * unit
        r = R.check_att(bad, df, sv, sa, xv, xa)
        assert 7.9 <= r[0] <= 8.1, (k, r)
    bad = {n: v.copy() for n, v in good.items()}
    _, _, w0, w1 = R.att_weights(sv, sa)
    bad["ds_v"] = ds_v * w1 / w0                                       # w1 for w0 in front of ds_v
    assert R.check_att(bad, df, sv, sa, xv, xa)[0] > R.BOUND
