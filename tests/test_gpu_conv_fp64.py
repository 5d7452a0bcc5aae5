"""The 3-D convolutions of the visual front-ends against float64 at an fp32-rounding bar (tests/conv_ref.py: reference, yardsticks, bound, ONE
case table; tests/test_conv_ref_host.py checks those on the CPU): ops.conv3d, ops.conv2d and ops.conv3d_cl forward + backward under the
case's switches and precision.  Every case asserts the path it reached (ops.CONV3D_CALLS, ops.STOCK_FALLBACKS) and the split-K / tile plan
of its walks for the workspace the process really has, synchronises and compares y, dx, dw, db per tensor:
rel_err <= BOUND max(E32, E_emu, 2^-24), exact zeros where no tap reaches.  Run with -s for one line per case."""
import contextlib

import numpy as np
import pytest
import torch

import conv_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_F = np.float32


def _dev(a, grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a, _F)).to(DEV)
    return t.requires_grad_(True) if grad else t


def _np(t):
    return t.detach().double().cpu().numpy()


def _rows(a):
    """[N,C,T,H,W] -> channels-last rows [N T H W, C]"""
    return R.to_rows(a).reshape(-1, a.shape[1])


def _planes(t, N, grid):
    """channels-last rows [N T H W, C] on the device -> [N,C,T,H,W] float64 numpy"""
    return R.to_planes(_np(t).reshape((N,) + tuple(grid) + (t.shape[-1],)))


def _run(c):
    """one forward + backward through the public operator -> tensor_names(c) in torch's layouts, float64 numpy"""
    from m3t import ops
    d = R.data(c)
    Ci, Co, k, st, pd, N, T, H, W = c.geo
    og = R.grids(c)[0]
    asked = bool(c.dx)
    if c.op == "conv3d":
        x, w, b = _dev(d["x"], asked), _dev(d["w"], True), _dev(d["b"], True)
        y = ops.conv3d(x, w, b, st, pd)
        y.backward(_dev(d["ct"]))
        out = {"y": _np(y), "dw": _np(w.grad), "dx": _np(x.grad) if asked else None}
    elif c.op == "conv2d":
        assert T == 1 and k[0] == 1 and st[0] == 1 and pd[0] == 0
        x, w, b = _dev(d["x"][:, :, 0], asked), _dev(d["w"][:, :, 0], True), _dev(d["b"], True)
        y = ops.conv2d(x, w, b, st[1:], pd[1:])
        y.backward(_dev(d["ct"][:, :, 0]))
        out = {"y": _np(y)[:, :, None], "dw": _np(w.grad)[:, :, None], "dx": _np(x.grad)[:, :, None] if asked else None}
    else:
        two = c.op == "conv3d_cl2"
        assert c.op == "conv3d_cl" or (two and k[0] == 1 and st[0] == 1 and pd[0] == 0)
        w, b = _dev(d["w"][:, :, 0] if two else d["w"], True), _dev(d["b"], True)
        if asked:
            x = _dev(_rows(d["x"]), True)
            xin = ops.CLTensor(x, N, T, H, W, None)
        else:                                              # a first layer takes the video planes
            x = xin = _dev(d["x"])
        assert ops.conv3d_cl_ok(xin, w, st[1:] if two else st, pd[1:] if two else pd, 1, (1,) * (w.dim() - 2), "zeros")
        y = ops.conv3d_cl(xin, w, b, st[1:] if two else st, pd[1:] if two else pd)
        assert (y.N, y.T, y.H, y.W) == (N,) + og
        y.data.backward(_dev(_rows(d["ct"])))
        out = {"y": _planes(y.data, N, og), "dw": _np(w.grad).reshape(d["w"].shape), "dx": _planes(x.grad, N, (T, H, W)) if asked else None}
    out["db"] = _np(b.grad)
    if not asked:
        del out["dx"]
    return out


@pytest.mark.parametrize("c", R.CASES, ids=[R.case_id(c) for c in R.CASES])
def test_convolution_against_float64(c):
    from m3t import ops
    assert R.flops(c) <= R.MAX_FLOP
    # the path-selection rules for the workspace this process really has: the plans the table was built for (host file) hold here too
    ws_bytes = ops.workspace(DEV).numel() * 4
    assert ws_bytes >= R.WS_MIN and R.plans(c, ws_bytes) == R.plans(c), (ws_bytes, R.plans(c, ws_bytes))
    if c.id == "T1":
        assert all(not narrow and splits > 1 for ts in R.plans(c, ws_bytes).values() for splits, _, narrow in ts)
    saved = {s: getattr(ops, s)[0] for s in c.off}
    calls0, stock0 = dict(ops.CONV3D_CALLS), sum(ops.STOCK_FALLBACKS.values())
    try:
        for s in c.off:
            getattr(ops, s)[0] = False
        with (ops.precision("x6") if c.prec == "x6" else contextlib.nullcontext()):
            got = _run(c)
            torch.cuda.synchronize()
    finally:
        for s, v in saved.items():
            getattr(ops, s)[0] = v
    # the path reached
    key = "walk" if c.fwd == "walk4" else c.fwd
    moved = {n: ops.CONV3D_CALLS[n] - calls0[n] for n in calls0}
    assert moved == {n: int(n == key) for n in calls0}, (c.id, moved)
    assert sum(ops.STOCK_FALLBACKS.values()) - stock0 == R.stock_calls(c), (c.id, ops.STOCK_FALLBACKS)
    ratio, name, fails = R.check(got, c)
    assert not fails, "%s: %s" % (c.id, "; ".join(fails))
    assert ratio <= R.BOUND
