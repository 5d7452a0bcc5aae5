"""m3t_adam_step, m3t_sgd_step and m3t_grad_norm_scale through the C ABI, on plain device buffers, against the float64
reference of tests/optim_ref.py (GPU).

Every asserted bar is either derived (optim_ref's docstring: the forward error analysis behind the single-step bounds,
c_m = 5, c_v = 8, c_p = 16 for Adam, c_buf = 3, c_p = 4 for SGD, in units of 2^-24 of the TERM magnitudes) or a stated
multiple of a yardstick computed without the code under test: the same operation sequence in fp32 numpy on the CPU.
tests/test_optim_reference_host.py shows without a GPU that the yardstick stays inside the derived bounds, i.e. that they
are not tighter than fp32 arithmetic allows.  Division and sqrtf are taken as correctly rounded.  Checked in the gfx950
assembly of adam_kernel (plain -O3, no fast-math): every division is the v_div_scale / v_rcp / v_div_fmas / v_div_fixup
sequence and every sqrtf is v_sqrt_f32 followed by its fma correction with input scaling, both correctly rounded; the
kernels run with fp32 denormals kept (float_denorm_mode_32 = 3); the compiler contracts most products and sums into
v_fma_f32 / v_pk_fma_f32, which only removes roundings.
"""
import ctypes as C
import os
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = R.U


def _lib():
    from m3t import _lib
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev(a, off=0):
    """a device copy of `a` whose base is `off` floats past a 16-byte boundary"""
    base = torch.zeros(a.size + 8, dtype=torch.float32, device=DEV)
    assert base.data_ptr() % 16 == 0
    t = base[off:off + a.size]
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def _launch(kind, bufs, t, hyper, guard=None):
    """bufs: device (p, g, state...).  Returns the C ABI's return code."""
    n = bufs[0].numel()
    if kind == "adam":
        p, g, m, v = bufs
        return _lib().m3t_adam_step(_ptr(p), _ptr(g), _ptr(m), _ptr(v), n, hyper["lr"], hyper["b1"], hyper["b2"], hyper["eps"],
                                    hyper["wd"], t, _ptr(guard), _stream())
    p, g, b = bufs
    return _lib().m3t_sgd_step(_ptr(p), _ptr(g), _ptr(b), n, hyper["lr"], hyper["momentum"], hyper["wd"], t, _ptr(guard), _stream())


def _step_gpu(kind, p, g, st, t, hyper, guard=None, off=0):
    bufs = [_dev(a, off) for a in [p, g] + list(st)]
    rc = _launch(kind, bufs, t, hyper, guard)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert np.array_equal(bufs[1].cpu().numpy(), g), "the gradient buffer was written"
    return [bufs[0].cpu().numpy()] + [b.cpu().numpy() for b in bufs[2:]]


def _run_cases(kind, cases):
    worst = (0.0, "")
    for c in cases:
        p, g, st = R.make_state(kind, c["n"], c["g_scale"], c["state"], c["hyper"], c["seed"])
        got = _step_gpu(kind, p, g, st, c["t"], c["hyper"])
        w, msg = R.check_step(kind, got, p, g, st, c["t"], c["hyper"])
        assert w <= 1.0, "%s %s: %s (%.3g x the bound)" % (kind, c["name"], msg, w)
        worst = max(worst, (w, c["name"] + " " + msg))
    print("%s: worst |error| / bound = %.3f at %s" % (kind, worst[0], worst[1]))
    return worst


# ------------------------------------------------------------------------------------------------- single step, element-wise
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_single_step_within_derived_bound_grid(kind):
    """step number (1 .. 1e5) x hyperparameters x gradient magnitude (squares that underflow .. 1e8) x state (first step, 50
    steps of history, zero gradient) at n = 4099 (16 float4 blocks + a 3-element tail for Adam): per element
    |m' - m'_64| <= 5u (|b1 m| + (1-b1) G), |v' - v'_64| <= 8u (b2 v + (1-b2) G^2), |p' - p'_64| <= u |p'_64| + 16u U,
    G = |g| + |wd p|, u = 2^-24 (optim_ref docstring); zero padding stays exactly zero."""
    _run_cases(kind, R.grid_cases(kind))


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_single_step_within_derived_bound_sizes(kind):
    """1 .. 5 (tail loop only / one float4 + tail), one full grid sweep +/- 3, three sweeps + 1, the C3 model's 26 397 707"""
    _run_cases(kind, R.size_cases(kind))


@pytest.mark.parametrize("n", [4099, R.SGD_SWEEP + 1])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_sgd_takes_any_base_alignment(n, off):
    h = R.SGD_DEFAULT
    p, g, st = R.make_state("sgd", n, 3e-3, "warm", h, 77 + off)
    got = _step_gpu("sgd", p, g, st, 5, h, off=off)
    w, msg = R.check_step("sgd", got, p, g, st, 5, h)
    assert w <= 1.0, msg


def test_refused_calls_return_einval_and_launch_nothing():
    """m3t_adam_step demands 16-byte aligned buffers (float4 accesses) and both kernels step >= 1: M3T_EINVAL before any
    launch -- the buffers are as they were."""
    from m3t import _lib
    n = 4099
    h = R.ADAM_DEFAULT
    p, g, st = R.make_state("adam", n, 3e-3, "warm", h, 5)
    host = [p, g] + st
    for which in range(4):
        for off in (1, 2, 3):
            bufs = [_dev(a, off if i == which else 0) for i, a in enumerate(host)]
            assert _launch("adam", bufs, 3, h) == _lib.M3T_EINVAL, (which, off)
            torch.cuda.synchronize()
            assert all(np.array_equal(b.cpu().numpy(), a) for a, b in zip(host, bufs))
    for step in (0, -1):
        bufs = [_dev(a) for a in host]
        assert _launch("adam", bufs, step, h) == _lib.M3T_EINVAL
        sb = [_dev(a) for a in host[:3]]
        assert _launch("sgd", sb, step, R.SGD_DEFAULT) == _lib.M3T_EINVAL
        torch.cuda.synchronize()
        assert all(np.array_equal(b.cpu().numpy(), a) for a, b in zip(host, bufs))
        assert all(np.array_equal(b.cpu().numpy(), a) for a, b in zip(host, sb))


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_guard_on_the_bare_kernel_at_a_multi_sweep_size(kind):
    """guard = NULL or a finite scalar: the step is taken; NaN, +inf, -inf: p and the state are bit-identical afterwards"""
    n = 3 * (R.ADAM_SWEEP if kind == "adam" else R.SGD_SWEEP) + 1
    h = R.hypers(kind)[0]
    p, g, st = R.make_state(kind, n, 3e-3, "warm", h, 31)
    ref_bits = None
    for val in (None, 0.37):
        guard = None if val is None else torch.tensor([val], dtype=torch.float32, device=DEV)
        got = _step_gpu(kind, p, g, st, 4, h, guard=guard)
        w, msg = R.check_step(kind, got, p, g, st, 4, h)
        assert w <= 1.0, (val, msg)
        assert not np.array_equal(got[0], p)
        if ref_bits is None:
            ref_bits = got
        assert all(np.array_equal(a, b) for a, b in zip(got, ref_bits)), "a finite guard changed the result"
    for val in (float("nan"), float("inf"), float("-inf")):
        guard = torch.tensor([val], dtype=torch.float32, device=DEV)
        got = _step_gpu(kind, p, g, st, 4, h, guard=guard)
        for a, b in zip(got, [p] + st):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "guard %r: a skipped step wrote something" % val


# ------------------------------------------------------------------------------------------------- skipped steps, pinned
def _flat_opt(kind, p, h):
    """FlatAdam / FlatSGD over bare buffers: the three attributes of FlatGradDDP they use"""
    from m3t.optim import FlatAdam, FlatSGD
    ddp = types.SimpleNamespace(flat_params=_dev(p), flat=_dev(np.zeros_like(p)), last_norm=None)
    if kind == "adam":
        return ddp, FlatAdam(ddp, lr=h["lr"], betas=(h["b1"], h["b2"]), eps=h["eps"], weight_decay=h["wd"])
    return ddp, FlatSGD(ddp, lr=h["lr"], momentum=h["momentum"], weight_decay=h["wd"])


def _state(kind, ddp, opt):
    torch.cuda.synchronize()
    st = [opt.m, opt.v] if kind == "adam" else [opt.buf]
    return ddp.flat_params.cpu().numpy().copy(), [s.cpu().numpy().copy() for s in st]


def test_adam_skipped_step_still_advances_the_step_count():
    """The rule (include/m3t_hip.h, `guard`): FlatAdam.step() counts a step the device skipped -- the host cannot know without
    synchronising -- so `clean, skipped, clean` is the reference called with t = 1, (nothing), t = 3."""
    n, h = 4099, dict(R.ADAM_DEFAULT, lr=1e-3)
    p0, g1, _ = R.make_state("adam", n, 3e-3, "zero", h, 11)
    _, g2, _ = R.make_state("adam", n, 3e-3, "zero", h, 12)
    _, g3, _ = R.make_state("adam", n, 3e-3, "zero", h, 13)
    ddp, opt = _flat_opt("adam", p0, h)
    norm = lambda x: torch.tensor([x], dtype=torch.float32, device=DEV)
    ddp.flat.copy_(torch.from_numpy(g1)); ddp.last_norm = norm(1.0); opt.step()
    p1, st1 = _state("adam", ddp, opt)
    w, msg = R.check_step("adam", [p1] + st1, p0, g1, [np.zeros_like(p0)] * 2, 1, h)
    assert w <= 1.0, msg
    ddp.flat.copy_(torch.from_numpy(g2)); ddp.last_norm = norm(float("nan")); opt.step()
    p2, st2 = _state("adam", ddp, opt)
    assert np.array_equal(p2, p1) and all(np.array_equal(a, b) for a, b in zip(st2, st1)) and opt.t == 2
    ddp.flat.copy_(torch.from_numpy(g3)); ddp.last_norm = norm(1.0); opt.step()
    p3, st3 = _state("adam", ddp, opt)
    assert opt.t == 3
    w, msg = R.check_step("adam", [p3] + st3, p1, g3, st1, 3, h)
    assert w <= 1.0, "not the reference's step with t = 3: " + msg
    w2, _ = R.check_step("adam", [p3] + st3, p1, g3, st1, 2, h)
    assert w2 > 100.0, "t = 2 and t = 3 are not told apart by this check (%.3g)" % w2


def test_sgd_skipped_first_step_then_clean_step_is_the_first_step():
    """skipped at t = 1, clean at t = 2: buf = 0 makes momentum*buf + g~ the reference's first step (buf' = g~), bit for bit"""
    n, h = 4099, R.SGD_DEFAULT
    p0, g1, _ = R.make_state("sgd", n, 3e-3, "zero", h, 21)
    _, g2, _ = R.make_state("sgd", n, 3e-3, "zero", h, 22)
    ddp, opt = _flat_opt("sgd", p0, h)
    ddp.flat.copy_(torch.from_numpy(g1)); ddp.last_norm = torch.tensor([float("inf")], device=DEV); opt.step()
    p1, st1 = _state("sgd", ddp, opt)
    assert np.array_equal(p1, p0) and not st1[0].any() and opt.t == 1
    ddp.flat.copy_(torch.from_numpy(g2)); ddp.last_norm = torch.tensor([0.5], device=DEV); opt.step()
    p2, st2 = _state("sgd", ddp, opt)
    assert opt.t == 2
    w, msg = R.check_step("sgd", [p2] + st2, p0, g2, [np.zeros_like(p0)], 1, h)
    assert w <= 1.0, msg
    first = _step_gpu("sgd", p0, g2, [np.zeros_like(p0)], 1, h)
    assert np.array_equal(first[0], p2) and np.array_equal(first[1], st2[0])


# ------------------------------------------------------------------------------------------------- many steps, yardstick
REGIMES = [(1e-4, 5e-5, 3e-3), (0.0, 1e-3, 1.0), (1e-4, 1e-3, 1e-9)]        # (weight decay, lr, gradient scale)
MANY_STEPS = 200
MANY_RATIOS = []


@pytest.mark.parametrize("regime", range(3))
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_many_steps_against_the_fp32_yardstick(kind, big, regime):
    """200 steps, a fresh gradient per step, the same fp32 gradients for three chains: float64, fp32 numpy (the yardstick),
    the kernel.  E_x = ||p_x - p_64|| / ||p_64 - p_0|| (and the moments' / the buffer's error relative to their own norm):
    E_gpu <= 4 E_f32.  Both are fp32 chains of the same length that differ in contraction and nothing else, so the
    expectation is a ratio near 1; a wrong constant anywhere moves E_gpu to 1e-3 .. 1, 20x .. 1e6x the yardstick."""
    wd, lr, gs = REGIMES[regime]
    n = (3 * (R.ADAM_SWEEP if kind == "adam" else R.SGD_SWEEP) + 1) if big else 4099
    h = dict(R.hypers(kind)[0], wd=wd, lr=lr)
    ns = 3 if kind == "adam" else 2
    p0, _, _ = R.make_state(kind, n, gs, "zero", h, 40 + regime)
    c64 = [p0.astype(np.float64)] + [np.zeros(n) for _ in range(ns - 1)]
    c32 = [p0.copy()] + [np.zeros(n, np.float32) for _ in range(ns - 1)]
    g = np.zeros(n, np.float32)
    bufs = [_dev(p0), _dev(g)] + [_dev(np.zeros(n, np.float32)) for _ in range(ns - 1)]
    # the CPU chains in independent chunks on a few threads (numpy releases the GIL): the buffers are element-wise
    nchunk = 16 if big else 1
    edges = np.linspace(0, n, nchunk + 1).astype(np.int64)
    rngs = [np.random.default_rng([regime, int(big), i]) for i in range(nchunk)]
    pad = R.pad_slice(n)

    def work(i, t):
        s = slice(int(edges[i]), int(edges[i + 1]))
        gi = R.draw_grad(rngs[i], s.stop - s.start, gs)
        lo, hi = max(pad.start, s.start), min(pad.stop, s.stop)
        if lo < hi:
            gi[lo - s.start:hi - s.start] = 0             # the padding stretch: p = g = 0 throughout
        g[s] = gi
        for chain, dt in ((c64, np.float64), (c32, np.float32)):
            out = R.step_ref(kind, chain[0][s], gi, [a[s] for a in chain[1:]], t, h, dtype=dt)
            for a, o in zip(chain, out):
                a[s] = o

    with ThreadPoolExecutor(max_workers=min(nchunk, 16, os.cpu_count() or 1)) as pool:
        for t in range(1, MANY_STEPS + 1):
            list(pool.map(lambda i: work(i, t), range(nchunk)))
            bufs[1].copy_(torch.from_numpy(g))
            assert _launch(kind, bufs, t, h) == 0
    torch.cuda.synchronize()
    got = [bufs[0].cpu().numpy()] + [b.cpu().numpy() for b in bufs[2:]]
    names = ("p", "m", "v") if kind == "adam" else ("p", "buf")
    msgs, ok = [], True
    for i, nm in enumerate(names):
        den = np.linalg.norm(c64[0] - p0) if i == 0 else np.linalg.norm(c64[i])
        assert den > 0
        e_gpu = np.linalg.norm(got[i].astype(np.float64) - c64[i]) / den
        e_f32 = np.linalg.norm(c32[i].astype(np.float64) - c64[i]) / den
        assert e_f32 > 0, "a yardstick of zero makes the assertion vacuous"
        msgs.append("%s: E_gpu %.3e E_f32 %.3e ratio %.2f" % (nm, e_gpu, e_f32, e_gpu / e_f32))
        ok = ok and e_gpu <= 4 * e_f32
    line = "%s n=%d wd=%g lr=%g g=%g  " % (kind, n, wd, lr, gs) + "; ".join(msgs)
    print(line)
    MANY_RATIOS.append(line)
    assert ok, line
    assert not got[0][pad].any() and all(not a[pad].any() for a in got[1:]), "the zero padding moved"


# ------------------------------------------------------------------------------------------------- the clip kernel
CLIP_SWEEP = 1024 * 256 * 4          # elements one pass of m3t_grad_norm_scale's grid covers
WS = []
NORM_RATIO = [0.0, ""]


def _clip_gpu(flat, world, max_norm):
    if not WS:
        WS.append(torch.zeros(1024 + 8, dtype=torch.float32, device=DEV))
    buf = _dev(flat)
    norm = torch.full((1,), -1.0, dtype=torch.float32, device=DEV)
    rc = _lib().m3t_grad_norm_scale(_ptr(buf), buf.numel(), 1.0 / world, max_norm, _ptr(norm), _ptr(WS[0]), WS[0].numel() * 4, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return buf.cpu().numpy(), float(norm.cpu()[0]), norm


_DRAWN = {}


def _drawn(n):
    if n not in _DRAWN:
        _DRAWN.clear()                                    # (one large vector at a time)
        _DRAWN[n] = R.draw_grad(np.random.default_rng(n), n, 1.0).astype(np.float64)
        _DRAWN[n][0] = 1.0                                # (n = 1: never a zero vector)
    return _DRAWN[n]


def _check_clip(flat, world, max_norm, what):
    """the norm against float64 within max(8 e_f32, 4u norm); the buffer: bit-identical (world 1) or the exact fp32 product
    g * (1/world) where the float64 coefficient is 1 by more than the norm's tolerance, else within 4u |ref| (the roundings of
    norm + 1e-6, the division, inv_world * coef, the product) plus the coefficient's relative error, which is the norm's"""
    ref, n64 = R.norm_scale(flat, world, max_norm)
    _, n32 = R.norm_scale(flat, world, max_norm, np.float32)
    got, ngpu, _ = _clip_gpu(flat, world, max_norm)
    e_f32 = abs(float(n32) - n64)
    tol = max(8 * e_f32, 4 * U * n64)
    err = abs(ngpu - n64)
    assert err <= tol, "%s: norm %.9g, float64 %.9g: error %.3g > max(8 x %.3g, 4u norm = %.3g)" % (what, ngpu, n64, err, e_f32, 4 * U * n64)
    if tol > 0 and err / tol > NORM_RATIO[0]:
        NORM_RATIO[:] = [err / tol, what]
    rel = tol / n64 if n64 > 0 else 0.0
    mx = R.f32(max_norm)
    coef64 = mx / (n64 + 1e-6) if mx > 0 else np.inf
    if coef64 >= 1 + 2 * rel + 4 * U:
        want = flat if world == 1 else flat * np.float32(1.0 / world)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: an unclipped buffer is not g * (1/world) bit for bit" % what
    bound = (4 * U + rel) * np.abs(ref) + 4 * R.TINY
    bad = np.abs(got.astype(np.float64) - ref) > bound
    assert not bad.any(), "%s: %d elements outside 4u + the norm's error, first at %d: %.9g vs %.9g" % (
        what, int(bad.sum()), int(np.argmax(bad)), got[np.argmax(bad)], ref[np.argmax(bad)])
    return ngpu, n64


WORLDS, MAX_NORMS = (1, 2, 8), (0.0, 1.0, 0.1, 1e9)
PLACES = (0.5, 0.9999, 0.999999, 1.000001, 2.0)      # norm / max_norm.  0.999999 is AT Lightning's threshold norm + 1e-6 = max_norm
                                                     # for max_norm = 1 and above it for 0.1; 0.9999 is a place strictly below


def _placed(n, world, max_norm, place):
    """a drawn vector scaled in float64 so that ||flat / world|| = place * max_norm (max_norm 0: place * 1), then rounded"""
    d = _drawn(n)
    target = place * (max_norm if max_norm > 0 else 1.0)
    return (d * (target * world / np.linalg.norm(d))).astype(np.float32)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 4099, CLIP_SWEEP + 1])
def test_clip_matches_float64_every_combination(n):
    for world in WORLDS:
        for max_norm in MAX_NORMS:
            for place in PLACES:
                _check_clip(_placed(n, world, max_norm, place), world, max_norm, "n=%d world=%d max_norm=%g place=%g" % (n, world, max_norm, place))
    print("worst norm error / tolerance so far: %.3f at %s" % tuple(NORM_RATIO))


@pytest.mark.parametrize("n", [CLIP_SWEEP - 3, CLIP_SWEEP - 2, CLIP_SWEEP - 1, CLIP_SWEEP, CLIP_SWEEP + 2, CLIP_SWEEP + 3,
                               3 * CLIP_SWEEP + 1, R.ADAM_SWEEP - 3, R.ADAM_SWEEP + 3, 3 * R.ADAM_SWEEP + 1, R.C3_PARAMS])
def test_clip_matches_float64_large_sizes(n):
    """every world, max_norm and place occurs at every size; the combinations rotate (the float64 side is the cost)"""
    for k in range(len(WORLDS) * len(PLACES)):
        world, place = WORLDS[k % 3], PLACES[k % 5]
        max_norm = MAX_NORMS[(k + n) % 4]
        _check_clip(_placed(n, world, max_norm, place), world, max_norm, "n=%d world=%d max_norm=%g place=%g" % (n, world, max_norm, place))
    print("worst norm error / tolerance so far: %.3f at %s" % tuple(NORM_RATIO))


@pytest.mark.parametrize("max_norm", [1.0, 1e9])
def test_clip_on_a_buffer_laid_out_like_the_real_one(max_norm):
    """FlatGradDDP's layout: slices of very different magnitude (1e-8 .. 1e2), each padded with zeros to a multiple of 32
    floats.  The padding is still exactly zero afterwards and the norm matches."""
    rng = np.random.default_rng(9)
    sizes = [9, 1, 33, 512 * 384, 384, 7, 1536 * 512, 1536, 100003, 2, 31, 64, 3 * 128 * 128, 129]
    scales = 10.0 ** np.linspace(-8, 2, len(sizes))
    rng.shuffle(scales)
    parts, mask = [], []
    for k, s in zip(sizes, scales):
        padded = (k + 31) // 32 * 32
        a = np.zeros(padded, np.float32)
        a[:k] = rng.standard_normal(k, dtype=np.float32) * np.float32(s)
        parts.append(a)
        mask.append(np.arange(padded) >= k)
    flat, mask = np.concatenate(parts), np.concatenate(mask)
    ref, n64 = R.norm_scale(flat, 1, max_norm)
    assert (n64 > 1.0) and mask.sum() > 100
    _check_clip(flat, 1, max_norm, "layout max_norm=%g" % max_norm)
    got, _, _ = _clip_gpu(flat, 1, max_norm)
    assert not got[mask].any(), "padding is not zero after the clip"


def _guarded_step_is_skipped(norm_dev):
    h = R.SGD_DEFAULT
    p, g, st = R.make_state("sgd", 4099, 1.0, "warm", h, 3)
    got = _step_gpu("sgd", p, g, st, 2, h, guard=norm_dev)
    return np.array_equal(got[0], p) and np.array_equal(got[1], st[0])


def test_clip_edges():
    """Documented in include/m3t_hip.h at m3t_grad_norm_scale."""
    n = 4099
    # all zeros: norm 0, buffer untouched, no NaN from 0 / 1e-6
    for world in (1, 8):
        got, norm, _ = _clip_gpu(np.zeros(n, np.float32), world, 1.0)
        assert norm == 0.0 and not got.any() and not np.signbit(got).any()
    # elements whose squares underflow: the norm reads 0, nothing is clipped, the buffer is untouched
    tiny = np.full(n, 1e-25, np.float32)
    got, norm, nd = _clip_gpu(tiny, 1, 1.0)
    assert norm == 0.0 and np.array_equal(got, tiny) and not _guarded_step_is_skipped(nd)
    # one NaN / one inf element: the norm is not finite and the guarded optimizer step is skipped
    for bad in (np.nan, np.inf, -np.inf):
        for max_norm in (1.0, 0.0):
            a = _placed(n, 1, 1.0, 0.5)
            a[n // 2] = bad
            _, norm, nd = _clip_gpu(a, 1, max_norm)
            assert not np.isfinite(norm), (bad, max_norm, norm)
            assert _guarded_step_is_skipped(nd)
    # every element 1e20: the true norm 6.4e21 is finite in fp32, the fp32 sum of squares is not.  The norm is not finite,
    # so the guarded optimizer step is skipped (the buffer's contents are not pinned)
    big = np.full(n, 1e20, np.float32)
    assert np.isfinite(np.float32(R.norm_scale(big, 1, 1.0)[1]))
    for max_norm in (1.0, 0.0):
        _, norm, nd = _clip_gpu(big, 1, max_norm)
        assert not np.isfinite(norm), norm
        assert _guarded_step_is_skipped(nd)
