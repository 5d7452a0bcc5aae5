"""csrc/fuse_loss.hip on the MI355X: every form and option of the VA loss (m3t_va_loss) and the attention fusion (m3t_att_fuse_fwd /
_bwd) against the float64 reference of tests/fuse_loss_ref.py.

Bound (fuse_loss_ref's docstring): an element may be off by 4 max(E32, floor) -- E32 the largest error of torch's own float32 CPU
autograd of the same composition on the same inputs, floor one fp32 ulp of the reference value or, where the closed form subtracts, of
the sum of the magnitudes of its terms.  Every test prints the worst ratio error / max(E32, floor) it saw (bound: 4).
tests/test_fuse_loss_host.py shows on the CPU that the forms' arithmetic holds half of that bound on every input class used here.

The loss has three forms behind one entry point; the row count selects them (include/m3t_hip.h):
  one workgroup    rows <= 1024 (ops.va_loss), or any row count without a workspace (C ABI, ws = NULL: several rows per thread)
  one launch       1025 .. 32768 rows: fp64 raw moments, the blocks meet once inside the kernel
  three launches   more rows: fp64 block partials, centred moments in a second pass
"""
import argparse
import ctypes as C

import numpy as np
import pytest
import torch

import fuse_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORST = {}


def _lib():
    from m3t import _lib
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _note(key, r, what=""):
    WORST[key] = max(WORST.get(key, 0.0), r[0])
    assert r[0] <= R.BOUND, "%s %s: %s" % (key, what, r[1])
    return r


# =============================================================================================== VA loss
def _form_of(rows, nows=False):
    return "one" if nows or rows <= 1024 else ("fused" if rows <= 32768 else "three")


def _va_ops(c):
    """through m3t.ops.va_loss and autograd (the library's own workspace) -> (out[8], dy) as numpy"""
    from m3t import ops
    y = _dev(c["y"]).requires_grad_(True)
    cls = _dev(c["class_expr"]) if c["n_expr"] > 0 else None
    vld = _dev(c["expr_valid"]) if c["n_expr"] > 0 else None
    loss, stats = ops.va_loss(y, _dev(c["valence"]), _dev(c["arousal"]), cls, vld, iv=c["iv"], ia=c["ia"], n_expr=c["n_expr"],
                              w_v=c["w_v"], w_a=c["w_a"], expr_w=c["expr_w"], use_mse=bool(c["use_mse"]))
    loss.backward()
    out = stats.cpu().numpy()
    assert out[0] == float(loss.detach()) or (np.isnan(out[0]) and np.isnan(float(loss.detach())))
    return out, y.grad.cpu().numpy()


def _va_abi(c, ws_floats=None):
    """through the C ABI.  ws_floats None: ws = NULL (one workgroup at any row count); else a workspace of exactly
    m3t_va_loss_ws_bytes(rows) inside an allocation twice that size, whose second half must come back untouched"""
    rows, Cc = c["y"].shape
    y, val, aro = _dev(c["y"]), _dev(c["valence"]), _dev(c["arousal"])
    cls = _dev(c["class_expr"]) if c["n_expr"] > 0 else None
    vld = _dev(c["expr_valid"]) if c["n_expr"] > 0 else None
    out = torch.full((8,), float("nan"), dtype=torch.float32, device=DEV)
    dy = torch.full((rows, Cc), float("nan"), dtype=torch.float32, device=DEV)
    ws, nbytes = None, 0
    if ws_floats is not None:
        nbytes = int(_lib().m3t_va_loss_ws_bytes(rows))
        assert nbytes == 4 * ws_floats
        ws = torch.full((2 * ws_floats,), -7.0, dtype=torch.float32, device=DEV)
        assert ws.data_ptr() % 8 == 0
    rc = _lib().m3t_va_loss(_ptr(y), rows, Cc, c["iv"], c["ia"], _ptr(val), _ptr(aro), _ptr(cls), _ptr(vld), c["n_expr"],
                            c["w_v"], c["w_a"], c["expr_w"], c["use_mse"], _ptr(out), _ptr(dy), _ptr(ws), nbytes, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    if ws is not None:
        assert bool((ws[ws_floats:] == -7.0).all()), "the loss wrote past m3t_va_loss_ws_bytes(rows)"
    return out.cpu().numpy(), dy.cpu().numpy()


def _va(c, form):
    rows = c["y"].shape[0]
    if form == "one_nows":
        return _va_abi(c)
    assert _form_of(rows) == form, (rows, form)
    return _va_ops(c)


def _check_case(c, form, skip_out=()):
    """one case on one form: two runs bit-identical, counts exact, free columns exactly zero, everything else within the bound"""
    out, dy = _va(c, form)
    out2, dy2 = _va(c, form)
    assert out.tobytes() == out2.tobytes() and dy.tobytes() == dy2.tobytes(), "%s %s: reruns differ" % (form, c["name"])
    return _note("va_loss " + R.emu_form(form), R.check_va(out, dy, c, skip_out=skip_out), c["name"])


@pytest.mark.parametrize("form", ["one", "one_nows", "fused", "three"])
def test_va_loss_option_matrix(form):
    """layouts (9 columns mtl; 2 columns; 12 columns with five that belong to no term; the ce_loss call, n_expr == C with zero regression
    weights; the ccc_loss / mse_loss call, C == 1) x use_mse x weights (0.5, 0.5, 0.8), (0.3, 0.7, 0.8), (1, 0, 0), (0, 1, 0.8); the label
    classes (no valid row, one valid row -- the last, in the ragged block --, all valid, logits of +-80 and +-1e4, tied maxima) and
    the statistics classes (predictions within 1e-3 of the targets, 0.8 + 1e-3 N, 1e-4 N, a constant column) -- all eight scalars and
    the full dy of each."""
    rows = R.OPTION_ROWS[form]
    worst = (0.0, "")
    for c in R.option_cases(rows):
        stats = c["name"].split("-")[-2]
        if not R.admitted(R.emu_form(form), stats, c["use_mse"]):
            continue
        worst = max(worst, _check_case(c, form))
    print("%s at %d rows: worst error / max(E32, floor) = %.3f (bound 4)  %s" % (form, rows, worst[0], worst[1]))


@pytest.mark.parametrize("form", ["one", "one_nows", "fused", "three"])
def test_va_loss_row_counts(form):
    """the row counts at which each form's indexing can go wrong: 1, 2, one wavefront +- 1, the workgroup's 1024 threads - 1 and full;
    2500 rows without a workspace (ragged third sweep); 1025 and 32769 (the last block holds one row), 4097, the 128-block limit"""
    worst = (0.0, "")
    for rows in R.FORM_ROWS[form]:
        for c in (R.make_case(rows, "mtl9", (0.3, 0.7, 0.8), seed=rows), R.make_case(rows, "gaps12", use_mse=1, labels="last", seed=rows),
                  R.make_case(rows, "one1", seed=rows)):
            worst = max(worst, _check_case(c, form))
    print("%s: worst error / max(E32, floor) = %.3f (bound 4)  %s" % (form, worst[0], worst[1]))


@pytest.mark.parametrize("form", ["one", "one_nows", "fused", "three"])
def test_va_loss_constant_prediction_column(form):
    """A constant prediction column against varying targets: cov = 0 exactly, so ccc = 0 and loss = 1, and the gradient is
    -w 2 (t - m_t) / (n den) (the cov / den^2 term vanishes; the gradient itself does not, ccc rises as soon as the column follows the
    targets).  fp64 sums of a constant are exact up to 2^-53 n, so the emulation (test_fuse_loss_host.py, class 'const') holds
    0.5 x the unit on dy and the loss scalars here are exact to one fp32 rounding: asserted as |ccc| <= 2^-40."""
    rows = R.OPTION_ROWS[form]
    c = R.make_case(rows, "va2", (0.3, 0.7, 0.8), stats="const", seed=3)
    out, dy = _va(c, form)
    assert abs(out[6]) <= 2.0 ** -40 and abs(out[7]) <= 2.0 ** -40 and out[1] == 1.0 and out[2] == 1.0
    r = _note("va_loss " + R.emu_form(form), R.check_va(out, dy, c), c["name"])
    print("%s: worst error / max(E32, floor) = %.3f (bound 4)" % (form, r[0]))


@pytest.mark.parametrize("form", ["one", "one_nows", "fused", "three"])
def test_va_loss_zero_weight_skips_its_term(form):
    """include/m3t_hip.h: a zero weight skips its term entirely.  A NaN in that term's prediction column leaves the loss and all of dy
    finite (the skipped term's own statistic, ccc_v / ccc_a / loss_expr, may be NaN), and everything else within the bound."""
    rows = R.OPTION_ROWS[form]
    for w, col_of, skip in (((1.0, 0.0, 0.0), "ia", (7,)), ((0.0, 1.0, 0.8), "iv", (6,))):
        for layout in ("mtl9", "gaps12"):
            c = R.make_case(rows, layout, w, seed=5)
            c["y"][rows // 2, c[col_of]] = np.nan
            out, dy = _va(c, form)
            assert np.isfinite(out[:6]).all() and np.isfinite(dy).all() and np.isnan(out[skip[0]]), (form, c["name"], out)
            assert not np.count_nonzero(dy[:, c[col_of]])
            _note("va_loss " + R.emu_form(form), R.check_va(out, dy, c, skip_out=skip), c["name"])
    c = R.make_case(rows, "mtl9", (0.5, 0.5, 0.0), labels="all", seed=6)
    clean = _va(c, form)
    c["y"][rows // 2, 3] = np.nan                                          # a logit of a valid row, expr_w == 0
    out, dy = _va(c, form)
    assert np.isfinite(out[:3]).all() and np.isfinite(dy).all() and not np.count_nonzero(dy[:, :7])
    assert out[:3].tobytes() == clean[0][:3].tobytes() and dy.tobytes() == clean[1].tobytes()


@pytest.mark.parametrize("form", ["one", "one_nows", "fused", "three"])
def test_va_loss_labels(form):
    """Markers of missing labels (-1, 255) on invalid rows give the bits of label 0; no valid row: the CE columns are exactly zero and
    loss_expr is not added; one valid row in the last block; the first of tied maxima counts; +-80 and +-1e4 stay finite."""
    rows = R.OPTION_ROWS[form]
    c = R.make_case(rows, "mtl9", seed=7)
    base = _va(c, form)
    for marker in (-1, 255):
        m = dict(c, class_expr=np.where(c["expr_valid"].astype(bool), c["class_expr"], marker).astype(np.int64))
        got = _va(m, form)
        assert got[0].tobytes() == base[0].tobytes() and got[1].tobytes() == base[1].tobytes(), marker
    c = R.make_case(rows, "mtl9", (0.3, 0.7, 0.8), labels="none", seed=8)
    out, dy = _va(c, form)
    ref = R.va_loss(*R.case_args(c))[0]
    assert out[4] == 0 and out[3] == 0 and not np.count_nonzero(dy[:, :7]) and abs(out[0] - (ref[0])) <= 4 * R.ulp32(1.0)
    c = R.make_case(rows, "mtl9", labels="last", seed=9)
    out, dy = _va(c, form)
    assert out[4] == 1 and np.count_nonzero(dy[:-1, :7]) == 0 and np.count_nonzero(dy[-1, :7]) == 7
    # ties: every logit of a row equal -> class 0 is the prediction; two equal maxima -> the lower index
    c = R.make_case(rows, "ce7", labels="all", seed=10)
    c["y"][:] = 0.25
    c["y"][1::2, 4] = c["y"][1::2, 2] = 1.5
    c["class_expr"][:] = np.tile(np.array([0, 2, 0, 4], np.int64), rows // 4 + 1)[:rows]
    out, dy = _va(c, form)
    expect = sum(1 for i in range(rows) if (i % 2 == 0 and c["class_expr"][i] == 0) or (i % 2 == 1 and c["class_expr"][i] == 2))
    assert out[5] == expect == R.va_loss(*R.case_args(c))[0][5] and out[4] == rows
    for labels in ("big80", "big1e4"):
        c = R.make_case(rows, "mtl9", labels=labels, seed=11)
        out, dy = _va(c, form)
        assert np.isfinite(out).all() and np.isfinite(dy).all()
        _note("va_loss " + R.emu_form(form), R.check_va(out, dy, c), c["name"])


def test_va_loss_one_row_rule():
    """rows == 1 (include/m3t_hip.h): the variances divide by max(rows - 1, 1) = 1, so var = cov = 0: ccc = 0, loss_v = 1, dL/dy = 0 for a
    prediction that differs from its target; 0 / 0 = NaN where they are equal.  mse and the CE term are ordinary."""
    c = R.make_case(1, "mtl9", (0.3, 0.7, 0.8), labels="all", seed=12)
    for run in (_va_ops, _va_abi):
        out, dy = run(c)
        assert out[6] == 0 and out[7] == 0 and out[1] == 1 and out[2] == 1 and dy[0, 7] == 0 and dy[0, 8] == 0 and out[4] == 1
        _note("va_loss one", R.check_va(out, dy, c), c["name"])
        m = dict(c, use_mse=1)
        _note("va_loss one", R.check_va(*run(m), m), "mse")
    e = dict(c, y=c["y"].copy())
    e["y"][0, 7] = e["valence"][0]
    out, dy = _va_ops(e)
    assert np.isnan(out[6]) and np.isnan(dy[0, 7]) and out[7] == 0 and dy[0, 8] == 0 and np.isfinite(dy[0, :7]).all()


@pytest.mark.parametrize("rows", [1025, 32768, 32769])
def test_va_loss_stays_inside_its_workspace(rows):
    """m3t_va_loss_ws_bytes(rows) is what the grid-wide forms may write: 16 doubles per 256-row block (the one-launch form's raw
    moments were promised 16 FLOATS per block and wrote twice that).  A workspace of exactly that size, then a guard band."""
    c = R.make_case(rows, "mtl9", (0.3, 0.7, 0.8), seed=13)
    out, dy = _va_abi(c, ws_floats=-(-rows // 256) * 32)
    ops_out, ops_dy = _va_ops(c)
    assert out.tobytes() == ops_out.tobytes() and dy.tobytes() == ops_dy.tobytes()          # the same form as through m3t.ops
    _note("va_loss " + _form_of(rows), R.check_va(out, dy, c), c["name"])


# ----------------------------------------------------------------------------------------------- model wiring
def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


@pytest.mark.parametrize("loss", ["ccc", "ccc_mtl", "mse", "mse_mtl"])
def test_model_va_objective_equals_the_reference(loss):
    """AffWild2VA.va_objective at --loss_lambda 0.3: hparams.loss picks the columns (7 / 8 with 'mtl', the last two without), the CE
    term and use_mse; the weights are (lambda, 1 - lambda, 0.8)"""
    from models.model import AffWild2VA
    m = AffWild2VA(_hp(modality="audio", loss=loss, loss_lambda=0.3))
    B, T = 3, 7
    mtl = "mtl" in loss
    c = R.make_case(B * T, "mtl9", (0.3, 1 - 0.3, 0.8), int("mse" in loss), seed=21)
    if not mtl:
        c.update(n_expr=0, iv=7, ia=8)
    y = _dev(c["y"].reshape(B, T, 9)).requires_grad_(True)
    batch = {"label_valence": _dev(c["valence"].reshape(B, T)), "label_arousal": _dev(c["arousal"].reshape(B, T)),
             "class_expr": _dev(c["class_expr"].reshape(B, T)), "expr_valid": _dev(c["expr_valid"].astype(bool).reshape(B, T))}
    l, stats = m.va_objective(y, batch)
    l.backward()
    r = _note("model", R.check_va(stats.cpu().numpy(), y.grad.reshape(B * T, 9).cpu().numpy(), c), loss)
    print("%s: worst error / max(E32, floor) = %.3f (bound 4)" % (loss, r[0]))


def test_model_loss_helpers_equal_the_reference():
    """mse_loss, ccc_loss (C == 1, w_a = expr_w = 0) and ce_loss (n_expr == C, zero regression weights): loss and gradient"""
    from models.model import AffWild2VA
    m = AffWild2VA(_hp(modality="audio"))
    B, T = 4, 9
    for name, use_mse in (("ccc_loss", 0), ("mse_loss", 1)):
        c = R.make_case(B * T, "one1", use_mse=use_mse, seed=22)
        y = _dev(c["y"].reshape(B, T)).requires_grad_(True)
        l = getattr(m, name)(y, _dev(c["valence"].reshape(B, T)))
        l.backward()
        ref, ref_dy, f_out, f_dy = R.va_loss(*R.case_args(c), floors=True)
        yo, ydy = R.va_loss_torch(*R.case_args(c))
        _note("model", R.compare(float(l), ref[0], yo[0], f_out[0], name))
        _note("model", R.compare(y.grad.reshape(-1, 1).cpu().numpy(), ref_dy, ydy, f_dy, "d " + name))
    c = R.make_case(B * T, "ce7", seed=23)
    y = _dev(c["y"].reshape(B, T, 7)).requires_grad_(True)
    l = m.ce_loss(y, _dev(c["class_expr"].reshape(B, T)), _dev(c["expr_valid"].astype(bool).reshape(B, T)))
    l.backward()
    ref, ref_dy, f_out, f_dy = R.va_loss(*R.case_args(c), floors=True)
    yo, ydy = R.va_loss_torch(*R.case_args(c))
    _note("model", R.compare(float(l), ref[0], yo[0], f_out[0], "ce_loss"))
    _note("model", R.compare(y.grad.reshape(-1, 7).cpu().numpy(), ref_dy, ydy, f_dy, "d ce_loss"))
    print("helpers: worst error / max(E32, floor) = %.3f (bound 4)" % WORST["model"])


# =============================================================================================== attention fusion
def _att_ops(df, s_v, s_a, x_v, x_a):
    from m3t import ops
    t = [_dev(a).requires_grad_(True) for a in (s_v, s_a, x_v, x_a)]
    f = ops.att_fuse(*t)
    f.backward(_dev(df))
    return dict(f=f.detach().cpu().numpy(), ds_v=t[0].grad.cpu().numpy(), ds_a=t[1].grad.cpu().numpy(), dx_v=t[2].grad.cpu().numpy(),
                dx_a=t[3].grad.cpu().numpy())


def _off(a, off):
    """a device copy of `a` whose base is `off` floats past a 16-byte boundary"""
    base = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 16 == 0
    t = base[off:off + a.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(a).reshape(-1)))
    return t


def _att_abi(df, s_v, s_a, x_v, x_a, off=0):
    """through the C ABI with x_v `off` floats past a 16-byte boundary (off != 0: the scalar path also where D % 4 == 0)"""
    rows, D = x_v.shape
    d = dict(df=_off(df, 0), s_v=_off(s_v, 0), s_a=_off(s_a, 0), x_v=_off(x_v, off), x_a=_off(x_a, 0))
    o = {k: torch.full((n + 8,), float("nan"), dtype=torch.float32, device=DEV)[:n]
         for k, n in (("f", rows * D), ("dx_v", rows * D), ("dx_a", rows * D), ("ds_v", rows), ("ds_a", rows))}
    assert d["x_v"].data_ptr() % 16 == 4 * off and all(o[k].data_ptr() % 16 == 0 for k in o)
    rc = _lib().m3t_att_fuse_fwd(_ptr(d["s_v"]), _ptr(d["s_a"]), _ptr(d["x_v"]), _ptr(d["x_a"]), _ptr(o["f"]), rows, D, _stream())
    assert rc == 0, rc
    rc = _lib().m3t_att_fuse_bwd(_ptr(d["df"]), _ptr(d["s_v"]), _ptr(d["s_a"]), _ptr(d["x_v"]), _ptr(d["x_a"]), _ptr(o["ds_v"]),
                                 _ptr(o["ds_a"]), _ptr(o["dx_v"]), _ptr(o["dx_a"]), rows, D, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().reshape((rows, D) if k in ("f", "dx_v", "dx_a") else (rows,)) for k, v in o.items()}


ATT_D = (1, 3, 4, 63, 64, 65, 260, 512, 1025)
ATT_ROWS = (1, 2, 5, 1000)


@pytest.mark.parametrize("rows", ATT_ROWS)
def test_att_fuse_shapes(rows):
    """D below a float4, below / at / above a wavefront's 64 lanes, several sweeps, odd (scalar path) and % 4 == 0 (vector path);
    rows % 4 != 0: the last workgroup is ragged.  f, dx_v, dx_a, ds_v, ds_a of each."""
    worst = (0.0, "")
    for D in ATT_D:
        a = R.make_att(rows, D, seed=1, score_scale=2.0)
        got = _att_ops(*a)
        worst = max(worst, _note("att_fuse", R.check_att(got, *a), "rows %d D %d" % (rows, D)))
    print("rows %d: worst error / max(E32, floor) = %.3f (bound 4)  %s" % (rows, worst[0], worst[1]))


@pytest.mark.parametrize("D", [4, 64, 260, 512])
def test_att_fuse_misaligned_operand_takes_the_scalar_path(D):
    """x_v 4, 8 and 12 bytes past a 16-byte boundary with D % 4 == 0: no float4 access.  f, dx_v, dx_a carry the vector path's bits
    (the same expression per element); ds_v, ds_a sum in another order and go through the bound."""
    a = R.make_att(5, D, seed=2)
    vec = _att_abi(*a, off=0)
    _note("att_fuse", R.check_att(vec, *a), "aligned D %d" % D)
    for off in (1, 2, 3):
        got = _att_abi(*a, off=off)
        for k in ("f", "dx_v", "dx_a"):
            assert got[k].tobytes() == vec[k].tobytes(), (k, off)
        r = _note("att_fuse", R.check_att(got, *a), "off %d D %d" % (off, D))
    print("D %d: worst error / max(E32, floor) = %.3f (bound 4)" % (D, WORST["att_fuse"]))


def test_att_fuse_saturated_scores():
    """Scores of 0, +-30, +-100, +-inf in every pairing.  fp32 sigmoid: 1 + expf(-30) rounds to 1 and expf(100) overflows, so the
    gate is exactly 1 at +30, +100, +inf and exactly 0 at -100, -inf, and h (1 - h) = 0 gives ds = 0 exactly there; at -30 the gate is
    9.4e-14 and ds is small, not zero.  The mixing weights stay in [1 / (1 + e), e / (1 + e)] (to one fp32 rounding)."""
    vals = np.array([0.0, 30.0, -30.0, 100.0, -100.0, np.inf, -np.inf], np.float32)
    s_v, s_a = np.repeat(vals, vals.size), np.tile(vals, vals.size)
    rows, D = s_v.size, 5
    df, _, _, x_v, x_a = R.make_att(rows, D, seed=3)
    got = _att_ops(df, s_v, s_a, x_v, x_a)
    assert all(np.isfinite(got[k]).all() for k in got)
    sat = lambda s: np.isin(s, vals[[1, 3, 4, 5, 6]])
    assert (got["ds_v"][sat(s_v)] == 0).all() and (got["ds_a"][sat(s_a)] == 0).all()
    assert (got["ds_v"][~sat(s_v) & (s_v != s_a)] != 0).all()
    r = _note("att_fuse", R.check_att(got, df, s_v, s_a, x_v, x_a), "saturated")
    w0 = _att_ops(df, s_v, s_a, np.ones_like(x_v), np.zeros_like(x_a))["f"][:, 0].astype(np.float64)
    lo, hi = 1 / (1 + np.e), np.e / (1 + np.e)
    assert (w0 >= lo - R.ulp32(lo)).all() and (w0 <= hi + R.ulp32(hi)).all()
    assert w0[(s_v == np.inf) & (s_a == -np.inf)] == pytest.approx(hi, abs=R.ulp32(hi)) and w0[s_v == s_a] == pytest.approx(0.5, abs=1e-7)
    print("saturated scores: worst error / max(E32, floor) = %.3f (bound 4)" % r[0])


def test_att_fuse_equal_inputs_cancel_in_ds():
    """x_v == x_a: ds = w0 w1 h (1 - h) (sum df x_v - sum df x_a) is exactly 0; what the kernel's d0 - (w0 d0 + w1 d1) leaves is bounded
    by the absolute-sum floor"""
    df, s_v, s_a, x_v, _ = R.make_att(37, 260, seed=4)
    got = _att_ops(df, s_v, s_a, x_v, x_v.copy())
    r = _note("att_fuse", R.check_att(got, df, s_v, s_a, x_v, x_v), "x_v == x_a")
    print("x_v == x_a: worst error / max(E32, floor) = %.3f (bound 4), largest |ds| %.3e" % (r[0], np.abs(got["ds_v"]).max()))


def test_att_fuse_nan_score_poisons_exactly_its_row():
    a = R.make_att(9, 65, seed=5)
    clean = _att_ops(*a)
    df, s_v, s_a, x_v, x_a = a
    s_v = s_v.copy()
    s_v[6] = np.nan
    got = _att_ops(df, s_v, s_a, x_v, x_a)
    for k, v in got.items():
        assert np.isnan(v[6]).all(), k
        keep = np.arange(9) != 6
        assert v[keep].tobytes() == clean[k][keep].tobytes(), k
    _note("att_fuse", R.check_att(got, df, s_v, s_a, x_v, x_a), "NaN score")


def test_zz_report_worst_ratios():
    """the figures NOTEBOOK.md records: worst error / max(E32, floor) per loss form and per operator over this run"""
    for k in sorted(WORST):
        print("%-18s worst error / max(E32, floor) = %.3f (bound 4)" % (k, WORST[k]))
    assert all(v <= R.BOUND for v in WORST.values())
