"""Float64 reference of what runs after backward: the 1/world average + global-norm clip, Adam, SGD.  Plain numpy.

Semantics
  adam_step   torch.optim.Adam: L2 weight decay added to the gradient, m' = b1 m + (1-b1) g~, v' = b2 v + (1-b2) g~^2,
              denom = sqrt(v')/sqrt(bc2) + eps, p' = p - (lr/bc1) m'/denom, bc_i = 1 - b_i^t, t counts from 1.
  sgd_step    torch.optim.SGD(momentum, weight_decay), dampening 0, no Nesterov: buf' = g~ on the first step (t == 1),
              momentum buf + g~ afterwards; p' = p - lr buf'.
  norm_scale  Lightning's clip after the data-parallel average: a = flat/world, norm = ||a||_2,
              coef = min(1, max_norm / (norm + 1e-6)), out = a coef; max_norm <= 0: no clipping.

The hyperparameters are fp32 values.  The C ABI (include/m3t_hip.h) takes lr, beta1, beta2, eps, weight_decay, momentum,
inv_world and max_norm as `float`, and the kernels form `1 - beta` from what they were passed: float(0.999) is
0.99900001287..., so the library runs Adam with THAT beta2 (consistently: the host computes the bias corrections from the
same rounded value, in double).  A reference that used the decimal 0.999 would differ by 1.3e-5 relative in v, far above
the rounding-level bounds of the tests.  So every hyperparameter is rounded to fp32 first, exactly once, and everything
after that is computed in `dtype`.  (1e-6 in the clip coefficient stays the decimal constant: its fp32 rounding moves the
coefficient by 2.5e-15 / norm.)

dtype = np.float64 is the reference.  dtype = np.float32 is the YARDSTICK: the same operation sequence carried out in fp32
on the CPU, one rounding per operation, no contraction.  It is what "an fp32 implementation of this update" deviates from
float64 by, and it is independent of the code under test.

Single-step error bounds (adam_bounds, sgd_bounds), u = 2^-24, every operation rounded once, G = |g| + |wd p| the
magnitude of the TERMS of g~ = g + wd p.  Forward error analysis of
      gg = g + wd*p;  mm = b1*m + (1-b1)*gg;  vv = b2*v + ((1-b2)*gg)*gg;  p -= ((lr*ibc1)*mm) / (sqrt(vv)*isb2 + eps)
  gg    2 roundings (product, sum)                                              |gg - g~| <= 2u G
  1-b   exact for b in [0.5, 1] (Sterbenz), else 1 rounding
  m'    term b1*m: product + sum = 2;   term (1-b1)*gg: (1-b1) 1 + gg 2 + product 1 + sum 1 = 5      ->  c_m = 5
  v'    term b2*v: 2;   term: (1-b2) 1 + gg 2 + product 1 + gg 2 + product 1 + sum 1 = 8             ->  c_v = 8
  p'    numerator: ibc1 = (float)(1/bc1) 1 + product 1 + mm 5 (of its term magnitudes) + product 1 = 8;
        denominator: sqrt halves v's 8 -> 4, sqrt 1, isb2 = (float)(1/sqrt(bc2)) 1, product 1, + eps 1 = 8;
        division 1: 17 in general, and 16 = 15.5 rounded up for betas in [0.5, 1] where 1-b is exact (one rounding
        less in mm, one less in vv, i.e. half of one in the denominator): every beta the tests use   ->  c_p = 16
        plus the final subtraction, u |p'|.
  SGD   buf' = momentum*buf + gg: term momentum*buf 2, term gg 2 + 1 = 3                             ->  c_buf = 3
        p' = p - lr*buf': product 1 + buf' 3 = 4, plus the final subtraction u |p'|                  ->  c_p = 4
Fused multiply-adds on the device only remove roundings.  Products that underflow are rounded absolutely, not relatively:
every bound carries a floor of a few denormal steps (2^-149), and p' the effect of v's floor through the square root.

Where g and wd p cancel (g~ much smaller than G) v' = (1-b2) g~^2 + ... is known only to 8u (1-b2) G^2 in ANY fp32
evaluation, which may be many times v' itself; the linear bound on p' then does not hold for any fp32 implementation.
adam_bounds therefore bounds the denominator by interval: sqrt(v' +- E_v), which equals the linear term wherever E_v is small
against v' and stays valid where it is not.
"""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
C_M, C_V, C_P_ADAM, C_BUF, C_P_SGD = 5, 8, 16, 3, 4

ADAM_DEFAULT = dict(lr=5e-5, b1=0.9, b2=0.999, eps=1e-8, wd=1e-4)
SGD_DEFAULT = dict(lr=1e-2, momentum=0.9, wd=5e-4)


def f32(x):
    """the value the C ABI receives"""
    return float(np.float32(x))


def adam_step(p, g, m, v, t, lr, b1, b2, eps, wd, dtype=np.float64):
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    d = dtype
    p, g, m, v = (np.asarray(a, dtype=d) for a in (p, g, m, v))
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t                       # (double on the host, from the rounded betas)
    gt = g + d(wd) * p
    m2 = d(b1) * m + (d(1) - d(b1)) * gt
    v2 = d(b2) * v + ((d(1) - d(b2)) * gt) * gt
    den = np.sqrt(v2) * d(1.0 / np.sqrt(bc2)) + d(eps)
    p2 = p - ((d(lr) * d(1.0 / bc1)) * m2) / den
    return p2, m2, v2


def sgd_step(p, g, buf, t, lr, momentum, wd, dtype=np.float64):
    lr, momentum, wd = f32(lr), f32(momentum), f32(wd)
    d = dtype
    p, g, buf = (np.asarray(a, dtype=d) for a in (p, g, buf))
    gt = g + d(wd) * p
    b2 = gt if t == 1 else d(momentum) * buf + gt
    return p - d(lr) * b2, b2


def norm_scale(flat, world, max_norm, dtype=np.float64):
    """-> (averaged and clipped buffer, norm of the averaged buffer before the clip)"""
    d = dtype
    a = np.asarray(flat, dtype=d) * d(f32(1.0 / world))
    with np.errstate(over="ignore", invalid="ignore"):
        norm = np.sqrt(np.sum(a * a, dtype=d))                    # (numpy: pairwise summation in `dtype`)
        mx = f32(max_norm)
        if mx > 0:
            coef = min(d(1), d(mx) / (norm + d(1e-6))) if np.isfinite(norm) else d(mx) / (norm + d(1e-6))
            a = a * d(coef)
    return a, norm


def adam_bounds(p, g, m, v, t, lr, b1, b2, eps, wd, ref=None):
    """(E_m, E_v, E_p): per-element bounds on |fp32 result - float64 result| of one step from the fp32 state (p, m, v);
    ref: adam_step's float64 result of the same arguments, if the caller has it already"""
    lr, b1, b2, eps, wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    assert 0.5 <= b1 <= 1 and 0.5 <= b2 <= 1, "c_p = 16 counts 1 - beta as exact"
    p64, _, v64 = ref if ref is not None else adam_step(p, g, m, v, t, lr, b1, b2, eps, wd)
    G = np.abs(g) + np.abs(wd * p)
    M = np.abs(b1 * m) + (1 - b1) * G                              # term magnitudes of m'
    V = b2 * v + (1 - b2) * G * G                                  # ... of v'
    e_m = C_M * U * M + 4 * TINY
    e_v = C_V * U * V + 4 * TINY
    isb2, step = 1.0 / np.sqrt(1.0 - b2 ** t), lr / (1.0 - b1 ** t)
    den = np.sqrt(v64) * isb2 + eps
    # the denominator an fp32 evaluation may see: v' anywhere in [v' - E_v, v' + E_v], then sqrt, two products / sums, + eps
    den_lo = (np.sqrt(np.maximum(v64 - e_v, 0.0)) * isb2 + eps) * (1 - 4 * U)
    den_hi = (np.sqrt(v64 + e_v) * isb2 + eps) * (1 + 4 * U)
    rel_den = np.maximum(den / den_lo - 1, 1 - den / den_hi)       # |den/den_f32 - 1|: 8u where E_v << v', more where g~ cancels
    upd = step * M / den
    e_p = U * np.abs(p64) + upd * (8 * U + rel_den * (1 + 8 * U)) + 4 * TINY     # 8 + 8 = 16 where rel_den is at its linear value 8u
    return e_m, e_v, e_p


def sgd_bounds(p, g, buf, t, lr, momentum, wd, ref=None):
    lr, momentum, wd = f32(lr), f32(momentum), f32(wd)
    p, g, buf = (np.asarray(a, dtype=np.float64) for a in (p, g, buf))
    p64, _ = ref if ref is not None else sgd_step(p, g, buf, t, lr, momentum, wd)
    G = np.abs(g) + np.abs(wd * p)
    B = G if t == 1 else np.abs(momentum * buf) + G
    e_b = C_BUF * U * B + 4 * TINY
    e_p = U * np.abs(p64) + C_P_SGD * U * lr * B + 4 * TINY
    return e_b, e_p


# --------------------------------------------------------------------------------------------- the cases of the kernel tests
ADAM_SWEEP = 2048 * 256 * 4          # elements one pass of m3t_adam_step's grid covers (float4 per thread)
SGD_SWEEP = 4096 * 256               # ... of m3t_sgd_step's
C3_PARAMS = 26397707                 # the benchmark's model


def sizes(kind):
    s = ADAM_SWEEP if kind == "adam" else SGD_SWEEP
    return [1, 3, 4, 5, 1023, 4099, s - 3, s - 2, s - 1, s, s + 1, s + 2, s + 3, 3 * s + 1, C3_PARAMS]


STEPS = (1, 2, 10, 1000, 100000)
G_SCALES = (1e-20, 1e-9, 3e-3, 1.0, 1e4)
STATES = ("zero", "warm", "pad")


def hypers(kind):
    if kind == "adam":
        return [dict(ADAM_DEFAULT), dict(ADAM_DEFAULT, wd=0.0), dict(ADAM_DEFAULT, lr=1.0), dict(ADAM_DEFAULT, eps=1e-3)]
    return [dict(SGD_DEFAULT), dict(SGD_DEFAULT, wd=0.0), dict(SGD_DEFAULT, lr=1.0), dict(SGD_DEFAULT, momentum=0.0)]


def draw_grad(rng, n, scale):
    """N(0,1) times 10**U(-3,0) per element, times `scale`, as fp32"""
    g = rng.standard_normal(n, dtype=np.float32) * np.exp2(np.float32(-3.0 * np.log2(10.0)) * rng.random(n, dtype=np.float32))
    return (g.astype(np.float64) * scale).astype(np.float32)


def pad_slice(n):
    """a stretch that plays FlatGradDDP's padding: p = g = state = 0 there"""
    k = min(37, n // 4)
    return slice(n // 3, n // 3 + k)


def make_state(kind, n, g_scale, state, hyper, seed, warm_steps=None):
    """fp32 (p, g, state...) of one case.  'zero': first-step state; 'warm': moments from `warm_steps` earlier float32 steps
    with fresh gradients of the same magnitude (50 for small buffers, 1 for the large ones: the cost is the CPU's);
    'pad': as 'zero' and the gradient is 0 everywhere, p = 0 on the padding stretch.  Every state carries the padding
    stretch, where the update must be exactly 0."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n, dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    pad = pad_slice(n)
    p[pad] = 0
    st = [np.zeros(n, np.float32) for _ in range(2 if kind == "adam" else 1)]
    if state == "warm":
        k = warm_steps if warm_steps is not None else (50 if n <= 5000 else 1)
        for t in range(1, k + 1):
            g = draw_grad(rng, n, g_scale)
            g[pad] = 0
            out = adam_step(p, g, st[0], st[1], t, dtype=np.float32, **hyper) if kind == "adam" else \
                sgd_step(p, g, st[0], t, dtype=np.float32, **hyper)
            p, st = out[0], list(out[1:])
    g = draw_grad(rng, n, g_scale)
    g[pad] = 0
    if state == "pad":
        g[:] = 0
    assert all(a.dtype == np.float32 for a in [p, g] + st)
    return p, g, st


def step_ref(kind, p, g, st, t, hyper, dtype=np.float64):
    if kind == "adam":
        return adam_step(p, g, st[0], st[1], t, dtype=dtype, **hyper)
    return sgd_step(p, g, st[0], t, dtype=dtype, **hyper)


def step_bounds(kind, p, g, st, t, hyper, ref=None):
    """bounds in the order of step_ref's results: (E_p, E_m, E_v) or (E_p, E_buf)"""
    if kind == "adam":
        e_m, e_v, e_p = adam_bounds(p, g, st[0], st[1], t, ref=ref, **hyper)
        return e_p, e_m, e_v
    e_b, e_p = sgd_bounds(p, g, st[0], t, ref=ref, **hyper)
    return e_p, e_b


def grid_cases(kind):
    """the full product step x hyperparameters x gradient magnitude x state at n = 4099"""
    out = []
    for t in STEPS:
        for hi, h in enumerate(hypers(kind)):
            for gs in G_SCALES:
                for st in STATES:
                    out.append(dict(n=4099, t=t, hyper=h, g_scale=gs, state=st, seed=len(out) + 1,
                                    name="n4099-t%d-h%d-g%g-%s" % (t, hi, gs, st)))
    return out


def size_cases(kind):
    """every size, default hyperparameters, ordinary gradients: the first step (t = 1, zero state) and a later one"""
    out = []
    for n in sizes(kind):
        for t, st in ((1, "zero"), (10, "warm")):
            out.append(dict(n=n, t=t, hyper=hypers(kind)[0], g_scale=3e-3, state=st, seed=1000 + len(out),
                            name="n%d-t%d-%s" % (n, t, st)))
    return out


def check_step(kind, got, p, g, st, t, hyper):
    """got: (p', state'...) of some fp32 implementation.  -> (worst |error| / bound over all outputs, message).  The padding
    stretch and every element with g~ = 0 and zero state must not have moved at all."""
    ref = step_ref(kind, p, g, st, t, hyper)
    bnd = step_bounds(kind, p, g, st, t, hyper, ref=ref)
    worst, msg = 0.0, ""
    names = ("p", "m", "v") if kind == "adam" else ("p", "buf")
    for nm, a, r, b in zip(names, got, ref, bnd):
        a = np.asarray(a, dtype=np.float64)
        if not np.all(np.isfinite(a)):
            return float("inf"), "%s not finite" % nm
        ratio = np.abs(a - r) / b                                  # (every bound has a positive floor)
        i = int(np.argmax(ratio))
        if ratio[i] > worst:
            worst, msg = float(ratio[i]), "%s[%d]: got %.9g ref %.9g bound %.3g" % (nm, i, a[i], r[i], b[i])
    pad = pad_slice(len(p))
    for nm, a, a0 in zip(names, got, [p] + list(st)):
        if not np.array_equal(np.asarray(a)[pad], np.asarray(a0)[pad]):
            return float("inf"), "%s moved on the zero padding" % nm
    return worst, msg
