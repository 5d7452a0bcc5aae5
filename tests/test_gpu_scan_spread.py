"""M3T_SCAN_SPREAD (include/m3t_hip.h): the fp16x3 forward scans and the wide producer-split backward scan with row blocks of 8 clips,
through m3t_gru_scan_fwd / _bwd directly, one forward and one reverse scan per call (n = 2), T = 6.

Forward: flag on equals flag off bit for bit (rows are independent; the W_hh slice scales do not depend on the row block).
Backward: a producer workgroup's scale is taken over 8 rows instead of 16, so results move at rounding level.  They are held to the
float64 recurrence on the same fp32 inputs at the bar of tests/gru_ref.py (NOTEBOOK.md R11): rel_err <= BOUND max(E32, E_emu, 2^-24)
per tensor, E32 = the same recurrence in numpy float32, E_emu = the 16-row kernel's arithmetic restated in float32 (gru_ref._BwdProduct,
gru_ref.cell_bwd) -- nothing fitted to GPU output.  Flag on and flag off each lie within the bar of the reference, hence within twice
the bar of each other.  The magnitude slot equals the largest stored |dr|, |dz|, |dn| and is no smaller than (1 - bar) x the float64
maximum.  Clips whose values would be NaN if rows 8..15 of a block leaked into rows 0..7 do not change the other clips' bits.
Run with -s for one line per case."""
import ctypes as C

import numpy as np
import pytest
import torch

import gru_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = 6
SHAPES = [(H, B) for H in (256, 512) for B in (8, 12, 20, 32)]
_F = np.float32


def _lib():
    from m3t import _lib
    return _lib


def _call(fn, descs, cls, B, flags):
    """one scan call with the exchange arena of the stream (the 8-clip geometry needs it); -> persistent launches issued"""
    from m3t import ops
    lib = _lib().load()
    dev = torch.device(DEV)
    ws = ops.workspace(dev)
    ops._scan_arena(dev)
    n0 = lib.m3t_gru_persist_count()
    rc = fn((cls * len(descs))(*descs), len(descs), B, T, C.c_void_p(ws.data_ptr()), ws.numel() * 4, flags,
            C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    ops.poll_scan_error()
    return lib.m3t_gru_persist_count() - n0


_IN = {}


def _inputs(H, B, n=2):
    """fp32 inputs of a case, drawn once: (n / 2) bidirectional pairs"""
    k = (H, B, n)
    if k not in _IN:
        g = torch.Generator().manual_seed(1000 * H + 10 * B + n)
        rn = lambda *s: torch.randn(*s, generator=g)
        _IN[k] = dict(xproj=[(rn(B, T, 6 * H) * 0.7).to(DEV) for _ in range(n // 2)],
                      w=[(rn(3 * H, H) / H ** 0.5).to(DEV) for _ in range(n)], b=[(rn(3 * H) * 0.1).to(DEV) for _ in range(n)],
                      dout=[(rn(B, T, 2 * H) * 0.2).to(DEV) for _ in range(n // 2)], dhn=(rn(n, B, H) * 0.2).to(DEV))
    return _IN[k]


def _fwd(H, B, flags, n=2, xproj=None):
    Lb = _lib()
    d = _inputs(H, B, n)
    xp = xproj if xproj is not None else d["xproj"]
    out = [torch.full((B, T, 2 * H), 7.0, device=DEV) for _ in range(n // 2)]
    gates, hn = torch.full((n, B, T, 4 * H), 7.0, device=DEV), torch.full((n, B, H), 7.0, device=DEV)
    descs = [Lb.GruFwdDesc(xp[i // 2].data_ptr(), d["w"][i].data_ptr(), d["b"][i].data_ptr(), out[i // 2].data_ptr(), gates[i].data_ptr(),
                           hn[i].data_ptr(), H, i % 2, 6 * H, (i % 2) * 3 * H, 2 * H, (i % 2) * H) for i in range(n)]
    launches = _call(Lb.load().m3t_gru_scan_fwd, descs, Lb.GruFwdDesc, B, flags)
    return (torch.stack(out), gates, hn), launches


_ACT = {}


def _acts(H, B, n=2):
    """the activations the backward cases read: the 16-row forward launch's, computed once"""
    k = (H, B, n)
    if k not in _ACT:
        _ACT[k] = _fwd(H, B, _lib().M3T_GEMM_F16X3, n)[0]
    return _ACT[k]


def _bwd(H, B, flags, n=2, dout=None):
    Lb = _lib()
    d = _inputs(H, B, n)
    out, gates, _ = _acts(H, B, n)
    do = dout if dout is not None else d["dout"]
    dgx = [torch.full((B, T, 6 * H), 7.0, device=DEV) for _ in range(n // 2)]
    dgh, dh = torch.full((n, B, T, 3 * H), 7.0, device=DEV), torch.full((n, B, H), 7.0, device=DEV)
    dbp, dbi, dbh = torch.full((n, B, 4, H), 7.0, device=DEV), torch.zeros(n, 3 * H, device=DEV), torch.zeros(n, 3 * H, device=DEV)
    amax = torch.zeros(n, 8, dtype=torch.int64, device=DEV)
    descs = [Lb.GruBwdDesc(do[i // 2].data_ptr(), out[i // 2].data_ptr(), gates[i].data_ptr(), d["w"][i].data_ptr(), d["dhn"][i].data_ptr(),
                           dgx[i // 2].data_ptr(), dgh[i].data_ptr(), dh[i].data_ptr(), dbp[i].data_ptr(), dbi[i].data_ptr(), dbh[i].data_ptr(),
                           H, i % 2, 2 * H, (i % 2) * H, 6 * H, (i % 2) * 3 * H, amax[i].data_ptr(), None) for i in range(n)]
    launches = _call(Lb.load().m3t_gru_scan_bwd, descs, Lb.GruBwdDesc, B, flags | Lb.M3T_SCAN_WHH)
    return dict(dgx=torch.stack(dgx), dgh=dgh, dh=dh, dbp=dbp, db_ih=dbi, db_hh=dbh, amax=amax), launches


def _cdiv(a, b):
    return (a + b - 1) // b


def _expect_wgs(n, H, B, members, spread):
    """level_shape in csrc/gru_persist.hip: 8-clip row blocks while n ceil(B / 8) H / 16 fits the CUs"""
    rb = 8 if (spread and n * _cdiv(B, 8) * (H // 16) <= R.CUS) else 16
    return n * _cdiv(B, rb) * members


# ================================================================================================= geometry
@pytest.mark.parametrize("H,B", SHAPES + [(512, 32)], ids=lambda v: str(v))
def test_workgroup_counts(H, B):
    Lb = _lib()
    lib = Lb.load()
    f16, wide, spread = Lb.M3T_GEMM_F16X3, Lb.M3T_SCAN_WIDE, Lb.M3T_SCAN_SPREAD
    for n in (2, 4):
        for fl, members, bwd in ((f16, H // 16, 0), (f16 | wide, H // 32, 0), (f16 | wide, H // 32, 1)):
            off, on = lib.m3t_gru_scan_workgroups(n, H, B, T, fl, bwd), lib.m3t_gru_scan_workgroups(n, H, B, T, fl | spread, bwd)
            assert off == _expect_wgs(n, H, B, members, False), (n, fl, bwd, off)
            assert on == _expect_wgs(n, H, B, members, True), (n, fl, bwd, on)
    # the fusion level's launches: twice the count; four scans of H = 512 would need 512 workgroups at 8-clip rows: unchanged
    if (H, B) == (512, 32):
        assert lib.m3t_gru_scan_workgroups(2, H, B, T, f16 | spread, 0) == 256 == 2 * lib.m3t_gru_scan_workgroups(2, H, B, T, f16, 0)
        assert lib.m3t_gru_scan_workgroups(2, H, B, T, f16 | wide | spread, 1) == 128 == 2 * lib.m3t_gru_scan_workgroups(2, H, B, T, f16 | wide, 1)
        for fl, bwd in ((f16, 0), (f16 | wide, 0), (f16 | wide, 1)):
            assert lib.m3t_gru_scan_workgroups(4, H, B, T, fl | spread, bwd) == lib.m3t_gru_scan_workgroups(4, H, B, T, fl, bwd)
    # a launch that is not one of the two kernels ignores the flag: fp32 MFMAs, the bf16 mode, the launch-per-step path
    for fl in (0, Lb.M3T_SCAN_FP32 | f16, Lb.M3T_BF16, Lb.M3T_SCAN_NO_PERSIST | f16):
        for bwd in (0, 1):
            assert lib.m3t_gru_scan_workgroups(2, H, B, T, fl | spread, bwd) == lib.m3t_gru_scan_workgroups(2, H, B, T, fl, bwd)


# ================================================================================================= forward
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("H,B", SHAPES, ids=lambda v: str(v))
def test_forward_is_bit_identical(H, B, wide):
    Lb = _lib()
    fl = Lb.M3T_GEMM_F16X3 | (Lb.M3T_SCAN_WIDE if wide else 0)
    off, n_off = (_acts(H, B), 1) if not wide else _fwd(H, B, fl)
    on, n_on = _fwd(H, B, fl | Lb.M3T_SCAN_SPREAD)
    assert n_off == 1 and n_on == 1
    for a, b, name in zip(on, off, ("out", "gates", "h_n")):
        assert torch.equal(a, b), name
        assert bool(torch.isfinite(a).all()), name


# ================================================================================================= backward against float64
def _bwd_recurrence(dout, dhn, out, gates, w_hh, reverse, dtype, prod=None):
    """the backward scan of one direction in `dtype` (float64: the reference; float32: yardstick A) or, with `prod` (gru_ref._BwdProduct),
    the 16-row kernel's float32 arithmetic (yardstick B).  gates [B, T, H, 4] as stored (r, z, n, W_hn h + b_hn).
    -> dgx, dgh [B, T, 3H], dh [B, H], db_ih, db_hh [3H]"""
    B, _, H = out.shape
    cast = lambda a: np.asarray(a, dtype)
    dout, dhn, out, gates, w = cast(dout), cast(dhn), cast(out), cast(gates), cast(w_hh)
    dgx, dgh = np.zeros((B, T, 3 * H), dtype), np.zeros((B, T, 3 * H), dtype)
    carry, z_next, prev, bnd = dhn, np.zeros((B, H), dtype), None, None
    for step in range(T):
        t = step if reverse else T - 1 - step
        tp = t + 1 if reverse else t - 1
        hprev = out[:, tp] if 0 <= tp < T else np.zeros((B, H), dtype)
        gr, gz, gn, ghn = (gates[:, t, :, k] for k in range(4))
        if prod is not None:
            mm = prod(prev, bnd) if step > 0 else np.zeros((B, H), _F)
            dht, dr, dz, dn, dnr = R.cell_bwd(dout[:, t], carry, z_next, mm, step > 0, gr, gz, gn, ghn, hprev)
            bnd = (np.abs(dht) * np.maximum(_F(1), _F(0.25) * np.abs(ghn))).astype(_F)
        else:
            dht = dout[:, t] + (carry * z_next + prev @ w if step > 0 else carry)
            dn = dht * (1 - gz) * (1 - gn * gn)
            dz = dht * (hprev - gn) * gz * (1 - gz)
            dr = dn * ghn * gr * (1 - gr)
            dnr = dn * gr
        dgx[:, t], dgh[:, t] = np.concatenate([dr, dz, dn], 1), np.concatenate([dr, dz, dnr], 1)
        prev, carry, z_next = dgh[:, t], dht, gz
    return dict(dgx=dgx, dgh=dgh, dh=carry, db_ih=dgx.sum((0, 1), dtype=dtype), db_hh=dgh.sum((0, 1), dtype=dtype))


NAMES = ("dgx", "dgh", "dh", "db_ih", "db_hh")
_REF = {}


def _reference(H, B):
    """per direction: (float64 reference, bar per tensor), computed once per shape and left unchanged"""
    k = (H, B)
    if k not in _REF:
        d = _inputs(H, B)
        out, gates, _ = _acts(H, B)
        res = []
        for i in (0, 1):
            a = (d["dout"][0][..., i * H:(i + 1) * H].cpu().numpy(), d["dhn"][i].cpu().numpy(), out[0][..., i * H:(i + 1) * H].cpu().numpy(),
                 gates[i].view(B, T, H, 4).cpu().numpy(), d["w"][i].cpu().numpy(), bool(i))
            ref = _bwd_recurrence(*a, np.float64)
            y32 = _bwd_recurrence(*a, np.float32)
            emu = _bwd_recurrence(*a, np.float32, prod=R._BwdProduct(a[4], "f16x3"))
            bar = {n: R.BOUND * max(R.rel_err(y32[n], ref[n]), R.rel_err(emu[n], ref[n]), R.FLOOR) for n in NAMES}
            res.append((ref, bar))
        _REF[k] = res
    return _REF[k]


def _direction(got, i, H, B):
    return dict(dgx=got["dgx"][0][..., i * 3 * H:(i + 1) * 3 * H].double().cpu().numpy(), dgh=got["dgh"][i].double().cpu().numpy(),
                dh=got["dh"][i].double().cpu().numpy(), db_ih=got["db_ih"][i].double().cpu().numpy(), db_hh=got["db_hh"][i].double().cpu().numpy())


@pytest.mark.parametrize("H,B", SHAPES, ids=lambda v: str(v))
def test_backward_against_float64_and_flag_off(H, B):
    Lb = _lib()
    fl = Lb.M3T_GEMM_F16X3 | Lb.M3T_SCAN_WIDE
    off, n_off = _bwd(H, B, fl)
    on, n_on = _bwd(H, B, fl | Lb.M3T_SCAN_SPREAD)
    assert n_off == 1 and n_on == 1
    fails = []
    for i in (0, 1):
        ref, bar = _reference(H, B)[i]
        g_on, g_off = _direction(on, i, H, B), _direction(off, i, H, B)
        for n in NAMES:
            e_on, e_off, e_pair = R.rel_err(g_on[n], ref[n]), R.rel_err(g_off[n], ref[n]), R.rel_err(g_on[n], g_off[n])
            print("H%d B%d dir%d %-6s rel_err on %.3g off %.3g on-vs-off %.3g bar %.3g" % (H, B, i, n, e_on, e_off, e_pair, bar[n]))
            if not e_on <= bar[n]:
                fails.append("dir %d %s: rel_err %.3g > %.3g" % (i, n, e_on, bar[n]))
            if not e_pair <= 2 * bar[n]:
                fails.append("dir %d %s: flag on vs off %.3g > %.3g" % (i, n, e_pair, 2 * bar[n]))
        # the magnitude slot: exactly the largest stored |dr|, |dz|, |dn| (|dn r| <= |dn|), and no smaller than the bar allows
        for name, g, raw in (("on", g_on, on), ("off", g_off, off)):
            slot = float(np.array([int(raw["amax"][i, 0]) & 0xffffffff], np.uint32).view(np.float32)[0])
            top, top_ref = float(np.abs(g["dgx"]).max()), float(np.abs(ref["dgx"]).max())
            print("H%d B%d dir%d amax %s %.9g stored max %.9g float64 max %.9g" % (H, B, i, name, slot, top, top_ref))
            if slot != top:
                fails.append("dir %d amax (%s) %.9g != the largest stored magnitude %.9g" % (i, name, slot, top))
            if not slot >= top_ref * (1 - bar["dgx"]):
                fails.append("dir %d amax (%s) %.9g below the float64 maximum %.9g by more than the bar" % (i, name, slot, top_ref))
    assert not fails, "\n".join(fails)


# ================================================================================================= where the flag changes nothing
def test_four_scans_and_per_step_path_ignore_the_flag():
    """n = 4 at H = 512, B = 32 would need 512 workgroups at 8-clip rows; M3T_SCAN_NO_PERSIST takes the launch-per-step kernels"""
    Lb = _lib()
    f16, wide, spread = Lb.M3T_GEMM_F16X3, Lb.M3T_SCAN_WIDE, Lb.M3T_SCAN_SPREAD
    H, B = 512, 32
    for n, base, launches in ((4, f16, 1), (4, f16 | wide, 1), (2, f16 | Lb.M3T_SCAN_NO_PERSIST, 0)):
        off, n_off = _fwd(H, B, base, n)
        on, n_on = _fwd(H, B, base | spread, n)
        assert n_off == launches and n_on == launches
        for a, b, name in zip(on, off, ("out", "gates", "h_n")):
            assert torch.equal(a, b), (n, base, name)
    for n, base, launches in ((4, f16 | wide, 1), (2, f16 | wide | Lb.M3T_SCAN_NO_PERSIST, 0)):
        off, n_off = _bwd(H, B, base, n)
        on, n_on = _bwd(H, B, base | spread, n)
        assert n_off == launches and n_on == launches
        for name in off:
            assert torch.equal(on[name], off[name]), (n, base, name)


# ================================================================================================= garbage rows
@pytest.mark.parametrize("H,B", [(256, 20), (512, 32)], ids=lambda v: str(v))
def test_nan_clips_do_not_reach_their_neighbours(H, B):
    """clips 8..15 NaN: with 8-clip row blocks they are the clips whose values sit where rows 8..15 of block 0 would be read from if a
    masked row leaked (the hand-over's rows, the gather's upper lanes); every other clip must come out bit for bit as in the finite batch"""
    Lb = _lib()
    f16, wide, spread = Lb.M3T_GEMM_F16X3, Lb.M3T_SCAN_WIDE, Lb.M3T_SCAN_SPREAD
    d = _inputs(H, B)
    bad = torch.zeros(B, dtype=torch.bool, device=DEV)
    bad[8:16] = True
    keep = ~bad
    xp = d["xproj"][0].clone()
    xp[bad] = float("nan")
    for fl in (f16, f16 | wide):
        fin, _ = _fwd(H, B, fl | spread)
        nan, n_l = _fwd(H, B, fl | spread, xproj=[xp])
        assert n_l == 1
        for a, b, name in ((nan[0][0], fin[0][0], "out"), (nan[1].transpose(0, 1), fin[1].transpose(0, 1), "gates"),
                           (nan[2].transpose(0, 1), fin[2].transpose(0, 1), "h_n")):
            assert torch.equal(a[keep], b[keep]), (fl, name)
            assert bool(torch.isnan(a[bad]).any()), (fl, name)      # (the NaN clips did diverge; their first-step W_hn h + b_hn is b_hn)
    do = d["dout"][0].clone()
    do[bad] = float("nan")
    fin, _ = _bwd(H, B, f16 | wide | spread)
    nan, n_l = _bwd(H, B, f16 | wide | spread, dout=[do])
    assert n_l == 1
    for name, clip_dim in (("dgx", 1), ("dgh", 1), ("dh", 1), ("dbp", 1)):
        a, b = nan[name].transpose(0, clip_dim), fin[name].transpose(0, clip_dim)
        assert torch.equal(a[keep], b[keep]), name
        assert bool(torch.isnan(a[bad]).any()), name
