"""The temporal convolutions against float64 at an fp32-rounding bar (tests/tcn_ref.py: reference, yardsticks, bound, ONE case table;
tests/test_tcn_ref_host.py checks those on the CPU): m3t_conv1d_fwd_scaled on both of its kernels in every fused form,
m3t_conv1d_wgrad_scaled, the weight-norm and mask kernels directly, and TemporalConvNet forward + backward with the nine magnitude slots of
every block.  Every case asserts the kernel it reached, synchronises and compares per tensor: rel_err <= BOUND max(E32, E_emu, 2^-24).
Run with -s for one line per case."""
import numpy as np
import pytest
import torch

import tcn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_F = np.float32


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, _F)).to(DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


def _bits(x):
    """fp32 value(s) -> the 32-bit patterns a magnitude slot holds in its low word"""
    return np.asarray(x, _F).view(np.uint32)


def _slot_val(slots):
    return (slots.cpu().numpy().astype(np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _amax_bits(t):
    return _bits(t.detach().abs().max().cpu().numpy())


def _offset_view(a, guard=None):
    """a copy of `a` that starts 4 bytes into a larger buffer (so it is not 16-byte aligned) -> (view, whole buffer)"""
    n = a.numel()
    buf = torch.full((n + 8,), float(guard) if guard is not None else 0.0, dtype=torch.float32, device=DEV)
    v = buf[1:1 + n]
    if guard is None:
        v.copy_(a.reshape(-1))
    assert v.data_ptr() % 16 == 4
    return v, buf


def _conv(x, w_t, bias, res, mask, shape, lead, act, anti, flags, drop=(0.0, 0), amax=(None, None), want_pre=False, arm=None, unaligned=False):
    """one m3t_conv1d_fwd_scaled call -> (y, pre or None, whole y buffer or None)"""
    from m3t import ops, _lib
    B, T, Ci, Co, K, dil = shape
    assert x.numel() == B * T * Ci and w_t.numel() == K * Co * Ci
    assert res is None or res.numel() == B * T * Co
    assert mask is None or mask.numel() == B * T * Co
    assert bias is None or bias.numel() == Co
    ybuf = None
    if unaligned:
        x, _kx = _offset_view(x)
        w_t, _kw = _offset_view(w_t)
        y, ybuf = _offset_view(torch.empty(B * T * Co, device=DEV), guard=12345.0)
    else:
        y = torch.empty(B * T * Co, dtype=torch.float32, device=DEV)
    pre = torch.empty(B * T * Co, dtype=torch.float32, device=DEV) if want_pre else None
    ops.amax_out(arm)
    rc = ops.lib().m3t_conv1d_fwd_scaled(ops._p(x), ops._p(w_t), ops._p(bias), ops._p(res), ops._p(mask), ops._p(y), ops._p(pre), B, T, Ci, Co, K, dil,
                                         lead, act, anti, float(drop[0]), int(drop[1]), flags, amax[0], amax[1], ops._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return y.view(B, T, Co), (pre.view(B, T, Co) if want_pre else None), ybuf


def _flags(prec):
    from m3t import _lib
    return _lib.M3T_GEMM_F16X3 if prec == "f16x3" else 0


def _run_op(c, amax=(None, None), arm=None):
    x, w_t, bias, res, mask_t, _ = R.op_operands(c)
    act, anti = R.op_args(c)
    y, pre, ybuf = _conv(_dev(x), _dev(w_t), _dev(bias), _dev(res), _dev(mask_t), (c.B, c.T, c.Ci, c.Co, c.K, c.dil), c.lead, act, anti,
                         _flags(c.prec), drop=(R.DROP_P, R.SEED) if c.form == "drop" else (0.0, 0), amax=amax, want_pre=c.form == "pre",
                         arm=arm, unaligned=c.id == "E6")
    if ybuf is not None:                                   # the guard bytes around an unaligned y are untouched
        g = ybuf.cpu().numpy()
        assert g[0] == 12345.0 and (g[1 + y.numel():] == 12345.0).all()
    out = {"y": y}
    if pre is not None:
        out["pre"] = pre
    return out


@pytest.mark.parametrize("c", R.OPS, ids=[R.case_id(c) for c in R.OPS])
def test_conv_forward_and_data_gradient_against_float64(c):
    from m3t import ops
    assert (c.kernel == "conv") == R.interior(c.B, c.T, c.Ci, c.Co, aligned=c.id != "E6")       # the kernel the call reaches
    arm = c.form in ("res", "drop") and c.id in ("I1", "E1")
    slot_y = torch.zeros(1, dtype=torch.int64, device=DEV) if arm else None
    got = _run_op(c, arm=slot_y.data_ptr() if arm else None)
    ratio, name, fails = R.check_op({n: _np(t) for n, t in got.items()}, c)
    assert not fails, "%s: %s" % (R.case_id(c), "; ".join(fails))
    assert ratio <= R.BOUND
    if arm:                                                # the armed slot holds max |y| of the returned tensor, bit for bit
        assert _slot_val(slot_y)[0] == _amax_bits(got["y"])
    if c.kernel == "conv" and c.prec == "f16x3":
        x, w_t = R.op_operands(c)[:2]
        xd, wd = _dev(x), _dev(w_t)
        slots = torch.zeros(2, dtype=torch.int64, device=DEV)
        assert ops.measure_amax([(xd.view(c.B * c.T, c.Ci), slots.data_ptr()), (wd.view(-1, wd.shape[-1]), slots.data_ptr() + 8)])
        torch.cuda.synchronize()
        assert _slot_val(slots)[0] == _bits(np.abs(x).max()) and _slot_val(slots)[1] == _bits(np.abs(w_t).max())
        exact = _run_op(c, amax=(slots.data_ptr(), slots.data_ptr() + 8))
        for n in got:                                      # exact caller slots: the very bits of the library's own measurement
            assert torch.equal(exact[n], got[n]), n
        big = torch.from_numpy(np.array([int(_bits(np.abs(x).max() * _F(64.0))), int(_bits(np.abs(w_t).max() * _F(64.0)))], np.int64)).to(DEV)
        loose = _run_op(c, amax=(big.data_ptr(), big.data_ptr() + 8))
        r6, n6, f6 = R.check_op({n: _np(t) for n, t in loose.items()}, c, quiet=True)
        assert not f6 and r6 <= R.BOUND, ("slots 2^6 too large", r6, n6)


@pytest.mark.parametrize("id_", ["I1", "E1"])
def test_power_of_two_statistics_scale_the_output_exactly(id_):
    """act 0, no bias: x scaled by a power of two scales y by the same power of two bit for bit -- the fp16x3 scales are exponents only, so
    a stale or mis-read slot breaks this"""
    c = [c for c in R.OPS if c.id == id_ and c.form == "pre" and c.prec == "f16x3"][0]
    x, w_t = R.op_operands(c)[:2]
    shape = (c.B, c.T, c.Ci, c.Co, c.K, c.dil)
    base = _conv(_dev(x), _dev(w_t), None, None, None, shape, c.lead, 0, 0, _flags("f16x3"))[0]
    assert torch.isfinite(base).all() and base.abs().max() > 0
    for k in (-20, 10):
        s = _F(2.0 ** k)
        y = _conv(_dev(x * s), _dev(w_t), None, None, None, shape, c.lead, 0, 0, _flags("f16x3"))[0]
        assert torch.equal(y, base * float(s)), k


@pytest.mark.parametrize("c", R.WGS, ids=[R.case_id(c) for c in R.WGS])
def test_conv_weight_gradient_against_float64(c):
    from m3t import ops
    d = R.wg_data(c)
    dy, x = _dev(d["dy"]), _dev(d["x"])
    flags = _flags(c.prec)
    ws = ops.workspace(torch.device(DEV))
    for use_ws in ((True, False) if c.id == "W4" else (True,)):
        for j in range(c.K):                               # the route of every tap
            r = R.wgrad_route(c.B, c.T, c.Ci, c.Co, c.K, c.dil, c.lead, c.prec, j)
            if r is not None:
                kern, _ = ops.sgemm_plan(1, c.Co, c.Ci, r[1], seg_len=r[2], prec=flags, ws_bytes=ws.numel() * 4 if use_ws else 0)
                assert kern == (0 if r[0] == "fp32" else 1), (j, r, kern)
        if c.id == "W4":
            assert all(R.wgrad_route(c.B, c.T, c.Ci, c.Co, c.K, c.dil, c.lead, c.prec, j)[0] == c.prec for j in range(c.K))
        dw = torch.full((c.K, c.Co, c.Ci), float("nan"), dtype=torch.float32, device=DEV)
        rc = ops.lib().m3t_conv1d_wgrad_scaled(ops._p(dy), ops._p(x), ops._p(dw), c.B, c.T, c.Ci, c.Co, c.K, c.dil, c.lead,
                                               ops._p(ws) if use_ws else None, ws.numel() * 4 if use_ws else 0, flags, None, None, ops._stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        ratio, name, fails = R.check_taps(_np(dw), c)
        assert not fails, "%s (workspace %s): %s" % (R.case_id(c), use_ws, "; ".join(fails))
        assert ratio <= R.BOUND


@pytest.mark.parametrize("Co,Ci,K", [(36, 20, 3), (130, 7, 2), (128, 64, 3)])
def test_weight_norm_kernels_against_float64(Co, Ci, K):
    from m3t import ops
    from oracle import m3t_oracle as O
    rs = np.random.RandomState(Co + Ci + K)
    v = rs.standard_normal((Co, Ci, K)).astype(_F)
    g = rs.uniform(0.5, 1.5, (Co, 1, 1)).astype(_F)
    dw_t = rs.standard_normal((K, Co, Ci)).astype(_F)
    w64, n64 = O.weight_norm_fwd(v.astype(np.float64), g.astype(np.float64))
    dv64, dg64 = O.weight_norm_bwd(dw_t.transpose(1, 2, 0).astype(np.float64), v.astype(np.float64), g.astype(np.float64), n64)
    ref = {"w_t": w64.transpose(2, 0, 1), "norm": n64.reshape(-1), "dv": dv64, "dg": dg64.reshape(-1)}
    # yardstick A: torch float32 autograd of g v / ||v||; yardstick B: the kernels' formulas in numpy float32
    tv, tg = torch.from_numpy(v).requires_grad_(True), torch.from_numpy(g).requires_grad_(True)
    nrm = tv.norm(2, dim=(1, 2), keepdim=True)
    tw = tg * tv / nrm
    tw.backward(torch.from_numpy(np.ascontiguousarray(dw_t.transpose(1, 2, 0))))
    yard = {"w_t": tw.detach().permute(2, 0, 1).numpy(), "norm": nrm.detach().reshape(-1).numpy(), "dv": tv.grad.numpy(), "dg": tg.grad.reshape(-1).numpy()}
    ew, en = R.emu_weight_norm(v, g)
    edv, edg = R.emu_weight_norm_bwd(dw_t, v, g, en)
    emu = {"w_t": ew, "norm": en, "dv": edv, "dg": edg.reshape(-1)}
    vd, gd, dwd = _dev(v), _dev(g), _dev(dw_t)
    w_t = torch.empty(K, Co, Ci, dtype=torch.float32, device=DEV)
    norm = torch.empty(Co, dtype=torch.float32, device=DEV)
    dv, dg = torch.empty(Co, Ci, K, dtype=torch.float32, device=DEV), torch.empty(Co, dtype=torch.float32, device=DEV)
    slot = torch.zeros(1, dtype=torch.int64, device=DEV)
    ops.amax_out(slot.data_ptr())
    assert ops.lib().m3t_weight_norm_fwd(ops._p(vd), ops._p(gd), ops._p(w_t), ops._p(norm), Co, Ci, K, ops._stream()) == 0
    assert ops.lib().m3t_weight_norm_bwd(ops._p(dwd), ops._p(vd), ops._p(gd), ops._p(norm), ops._p(dv), ops._p(dg), Co, Ci, K, ops._stream()) == 0
    torch.cuda.synchronize()
    assert _slot_val(slot)[0] == _amax_bits(w_t)
    got = {"w_t": w_t, "norm": norm, "dv": dv, "dg": dg}
    for n in ref:
        yd = max(R.rel_err(yard[n], ref[n]), R.rel_err(emu[n], ref[n]), R.FLOOR)
        ratio = R.rel_err(_np(got[n]), ref[n]) / yd
        print("weight_norm (%d, %d, %d) %-5s %5.2f x" % (Co, Ci, K, n, ratio))
        assert ratio <= R.BOUND, (n, ratio)


@pytest.mark.parametrize("rows,Cc", [(111, 36), (384, 128)])
def test_mask_kernels_are_exact_selections(rows, Cc):
    from m3t import ops
    rs = np.random.RandomState(rows + Cc)
    s, dy, mul = (rs.standard_normal((rows, Cc)).astype(_F) for _ in range(3))
    mk = R.drop_mask(rows, Cc, R.SEED).astype(_F)
    want = {"plain": np.where(s > 0, dy, _F(0)), "mul": np.where(s > 0, dy * mul, _F(0)), "drop": np.where(s > 0, dy * mk, _F(0))}
    sd, dyd, muld = _dev(s), _dev(dy), _dev(mul)
    for kind in ("plain", "mul", "drop"):
        out = torch.full((rows, Cc), float("nan"), dtype=torch.float32, device=DEV)
        slot = torch.zeros(1, dtype=torch.int64, device=DEV)
        ops.amax_out(slot.data_ptr())
        if kind == "drop":
            rc = ops.lib().m3t_mask_pos_drop(ops._p(sd), ops._p(dyd), ops._p(out), rows, Cc, float(R.DROP_P), int(R.SEED), ops._stream())
        else:
            rc = ops.lib().m3t_mask_pos(ops._p(sd), ops._p(dyd), ops._p(muld) if kind == "mul" else None, ops._p(out), rows * Cc, ops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want[kind]), kind
        assert (want[kind] == 0).mean() > 0.3 and np.abs(want[kind]).max() > 0
        assert _slot_val(slot)[0] == _bits(np.abs(want[kind]).max()), kind


# ================================================================================================= blocks
def _net(c, d):
    from models.tcn import TemporalConvNet
    m = TemporalConvNet(c.Cin, list(c.widths), c.K, dropout=R.DROP_P).to(DEV)
    names = sorted(n for n, _ in m.named_parameters())
    assert names == sorted(d["p"]), (names, sorted(d["p"]))
    with torch.no_grad():
        for n, t in m.named_parameters():
            t.copy_(torch.from_numpy(d["p"][n]))
    m.train(c.train)
    return m


def _run_net(c, m, d):
    """forward block by block (explicit seeds) + backward -> (tensors name -> device tensor, per-block outputs, the input tensor)"""
    from m3t import ops
    for p in m.parameters():
        p.grad = None
    x = _dev(d["x"]).requires_grad_(True)
    ys, cur = [], x
    with ops.precision("x6" if c.prec == "x6" else "fp32"):
        for i, blk in enumerate(m.network):
            cur = blk.forward_btc(cur, seeds=R.block_seeds(i) if c.train else None)
            ys.append(cur)
        (cur * _dev(d["ct"])).sum().backward()
    ops.join_wgrad()
    torch.cuda.synchronize()
    got = {"y": cur, "dx": x.grad}
    got.update({n: p.grad for n, p in m.named_parameters()})
    return got, ys, x


def _check_slots(c, m, d, ys, x):
    """the nine magnitude slots of every block of an interior network after backward"""
    from m3t import ops
    _, e_emu = R.emulated(c)
    for i, (blk, (ci, co, dil)) in enumerate(zip(m.network, R.levels(c))):
        pre = "network.%d." % i
        tag = ys[i]._m3t_amax
        assert tag[0][1] == 8 and tag[1] == ys[i]._version
        val = _slot_val(tag[0][0])
        assert len(val) == 9
        for k, conv, cin in ((1, blk.conv1, ci), (2, blk.conv2, co)):          # the weight-norm kernel is deterministic: recompute w_t
            w_t = torch.empty(c.K, co, cin, dtype=torch.float32, device=DEV)
            nrm = torch.empty(co, dtype=torch.float32, device=DEV)
            assert ops.lib().m3t_weight_norm_fwd(ops._p(conv.weight_v.detach()), ops._p(conv.weight_g.detach()), ops._p(w_t), ops._p(nrm), co, cin, c.K,
                                                 ops._stream()) == 0
            torch.cuda.synchronize()
            assert val[k] == _amax_bits(w_t), (i, k)
        assert val[8] == _amax_bits(ys[i]), i
        if i == 0:
            assert getattr(x, "_m3t_amax", None) is None and val[0] == _amax_bits(x)          # an input without a slot: measured by the block
        else:
            assert ops._tagged_amax(ys[i - 1]) is not None and val[0] == 0       # the block found the slot on its input and measured nothing
        if blk.downsample is not None:
            assert val[3] == _amax_bits(blk.downsample.weight)
        else:
            assert val[3] == 0
        for k, nm in ((4, "h1"), (5, "ds"), (6, "da2"), (7, "da1")):
            top = float(np.abs(d["ref"][pre + nm]).max())
            yd = max(d["e32"][pre + nm], e_emu[pre + nm], R.FLOOR)
            got = float(val[k:k + 1].view(_F)[0])
            assert abs(got - top) / top <= R.BOUND * yd, (i, nm, got, top, yd)


@pytest.mark.parametrize("c", R.BLOCKS, ids=[R.case_id(c) for c in R.BLOCKS])
def test_temporal_blocks_against_float64(c):
    d = R.data(c)
    m = _net(c, d)
    # ---- the kernels the case reaches
    inner = [R.interior(c.B, c.T, ci, co) and R.interior(c.B, c.T, co, co) for ci, co, _ in R.levels(c)]
    assert all(inner) == (c.id != "C3" and c.id != "C3t") and (all(inner) or not any(inner))
    got, ys, x = _run_net(c, m, d)
    ratio, name, fails = R.check({n: _np(t) for n, t in got.items()}, c)
    assert not fails, "%s: %s" % (R.case_id(c), "; ".join(fails))
    assert ratio <= R.BOUND
    if all(inner) and c.prec == "f16x3":
        _check_slots(c, m, d, ys, x)
    else:
        assert all(getattr(y, "_m3t_amax", None) is None for y in ys)


def test_weight_gradient_stream_path_with_gradient_sinks():
    """C7: C1 with every parameter holding a gradient sink -- the weight gradients are written on the weight-gradient streams straight into the
    sinks; after join_wgrad they are held to the same bar, and dx is bit-identical to the plain path's"""
    from m3t import ops
    c = [c for c in R.BLOCKS if c.id == "C1"][0]
    d = R.data(c)
    m = _net(c, d)
    plain, _, _ = _run_net(c, m, d)
    dx_plain = plain["dx"].clone()
    params = list(m.named_parameters())
    flat = torch.zeros(sum((p.numel() + 3) // 4 * 4 for _, p in params), dtype=torch.float32, device=DEV)
    try:
        off = 0
        for _, p in params:
            view = flat[off:off + p.numel()].view(p.shape)
            off += (p.numel() + 3) // 4 * 4
            p.grad = view
            ops.register_grad_sink(p, view)
        ops.arm_grad_sinks()
        x = _dev(d["x"]).requires_grad_(True)
        cur = x
        for blk in m.network:
            cur = blk.forward_btc(cur)
        (cur * _dev(d["ct"])).sum().backward()
        assert not any(e[2] for e in ops._GRAD_SINKS.values()), "a sink was not taken: the stream path did not run"
        ops.join_wgrad()
        torch.cuda.synchronize()
        got = {"y": cur, "dx": x.grad}
        off = 0
        for n, p in params:
            assert p.grad.data_ptr() == flat.data_ptr() + 4 * off
            got[n] = flat[off:off + p.numel()].view(p.shape)
            off += (p.numel() + 3) // 4 * 4
    finally:
        ops.clear_grad_sinks()
    assert torch.equal(got["dx"], dx_plain)
    ratio, name, fails = R.check({n: _np(t) for n, t in got.items()}, c)
    assert not fails, "; ".join(fails)
    assert ratio <= R.BOUND
