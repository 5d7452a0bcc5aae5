"""The float64 statement of GroupNorm (+ReLU) (+max pooling) forward and backward, as csrc/gn_cl.hip computes it -- written out by formula,
not by autograd, so that the fused form (pooled output, winner byte, gradient routed through the winner) has a reference of its own.
tests/test_gn_stem_host.py checks it against torch's float64 autograd on the CPU; the GPU tests compare the kernels with it.

Tensors are planes [N, C, T, H, W] (float64 torch tensors); to_rows / from_rows convert to and from the channels-last rows of the kernels."""
import torch


def to_rows(x5):
    """[N, C, T, H, W] -> [N T H W, C]"""
    return x5.permute(0, 2, 3, 4, 1).reshape(-1, x5.shape[1]).contiguous()


def from_rows(rows, N, T, H, W):
    """[N T H W, C] -> [N, C, T, H, W]"""
    return rows.reshape(N, T, H, W, -1).permute(0, 4, 1, 2, 3).contiguous()


def stats(x, G, eps):
    """mean, rstd [N, G]: one mean and one biased variance per (clip, group)"""
    N = x.shape[0]
    xg = x.reshape(N, G, -1)
    mean = xg.mean(2)
    var = ((xg - mean[:, :, None]) ** 2).mean(2)
    return mean, 1.0 / torch.sqrt(var + eps)


def _per_channel(v, C):
    """[N, G] -> [N, C, 1, 1, 1]"""
    return v.repeat_interleave(C // v.shape[1], dim=1)[:, :, None, None, None]


def xhat_of(x, G, eps):
    mean, rstd = stats(x, G, eps)
    C = x.shape[1]
    return (x - _per_channel(mean, C)) * _per_channel(rstd, C), mean, rstd


def _windows(y, k):
    """[N, C, T, H, W] -> [N, C, T, Ho, Wo, k k] in window order (dh k + dw); positions no window covers are left out"""
    N, C, T, H, W = y.shape
    Ho, Wo = H // k, W // k
    return y[:, :, :, :Ho * k, :Wo * k].reshape(N, C, T, Ho, k, Wo, k).permute(0, 1, 2, 3, 5, 4, 6).reshape(N, C, T, Ho, Wo, k * k)


def pool(y, k):
    """max pooling (1, k, k) / stride k / no padding -> (yp, win): ties go to the first maximum in window order, NaN wins (the first NaN)"""
    w = _windows(y, k)
    nan = torch.isnan(w)
    first_nan = nan.to(torch.int8).argmax(-1)
    top = torch.where(nan, torch.full_like(w, float("-inf")), w).max(-1, keepdim=True).values
    first_max = (w == top).to(torch.int8).argmax(-1)
    win = torch.where(nan.any(-1), first_nan, first_max)
    return w.gather(-1, win[..., None])[..., 0], win.to(torch.uint8)


def forward(x, G, gamma, beta, eps, relu=True, k=0):
    """-> dict(y: the full-resolution map, yp / win: the pooled map and the winner bytes if k, mean, rstd, xhat)"""
    C = x.shape[1]
    xh, mean, rstd = xhat_of(x, G, eps)
    y = xh * gamma.view(1, C, 1, 1, 1) + beta.view(1, C, 1, 1, 1)
    if relu:
        y = torch.relu(y)
    out = dict(y=y, mean=mean, rstd=rstd, xhat=xh)
    if k:
        out["yp"], out["win"] = pool(y, k)
    return out


def backward(dout, x, G, gamma, eps, fwd, relu=True, k=0):
    """dout: d(y) [N, C, T, H, W], or d(yp) if k.  g = dout masked by the ReLU (0 where y <= 0, as torch's threshold_backward), in the fused
    form taken at the window's winner.  Per (clip, group), M = (C / G) R: s1 = sum gamma g, s2 = sum gamma g xhat,
    dx = rstd (gamma g - s1 / M - xhat s2 / M); dgamma = sum g xhat, dbeta = sum g.  -> dict(dx, dgamma, dbeta, colsum: dx's column sums, g)"""
    N, C, T, H, W = x.shape
    xh, rstd = fwd["xhat"], fwd["rstd"]
    if k:
        yp, win = fwd["yp"], fwd["win"].long()
        gp = torch.where(yp <= 0, torch.zeros_like(dout), dout) if relu else dout
        Ho, Wo = H // k, W // k
        gw = torch.zeros(N, C, T, Ho, Wo, k * k, dtype=x.dtype)
        gw.scatter_(-1, win[..., None], gp[..., None])
        g = torch.zeros_like(x)
        g[:, :, :, :Ho * k, :Wo * k] = gw.reshape(N, C, T, Ho, Wo, k, k).permute(0, 1, 2, 3, 5, 4, 6).reshape(N, C, T, Ho * k, Wo * k)
    else:
        g = torch.where(fwd["y"] <= 0, torch.zeros_like(dout), dout) if relu else dout
    gam = gamma.view(1, C, 1, 1, 1)
    M = (C // G) * T * H * W
    s1 = (gam * g).reshape(N, G, -1).sum(2)
    s2 = (gam * g * xh).reshape(N, G, -1).sum(2)
    dx = _per_channel(rstd, C) * (gam * g - _per_channel(s1, C) / M - xh * _per_channel(s2, C) / M)
    return dict(dx=dx, dgamma=(g * xh).sum((0, 2, 3, 4)), dbeta=g.sum((0, 2, 3, 4)), colsum=dx.sum((0, 2, 3, 4)), g=g)


def torch_autograd(x, G, gamma, beta, eps, dout, k=0):
    """the same quantities from torch's own operators and autograd (F.group_norm -> relu -> max_pool3d), any dtype / device"""
    import torch.nn.functional as F
    x, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    y = torch.relu(F.group_norm(x, G, gamma, beta, eps))
    out = F.max_pool3d(y, (1, k, k), (1, k, k)) if k else y
    out.backward(dout)
    return dict(out=out.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, colsum=x.grad.sum((0, 2, 3, 4)))


# the operator cases of tests/test_gpu_gn_cl.py: (N, C, G, T, H, W, k), k = 0 for no pooling
CASES = [
    (3, 64, 32, 2, 5, 5, 2),        # a thread's quad straddles groups, odd frame with uncovered positions, 50 rows a clip
    (2, 128, 32, 3, 7, 6, 0),       # one quad per group
    (2, 256, 32, 1, 4, 4, 2),       # two quads per group, tiny R
    (2, 64, 32, 2, 27, 27, 2),      # 1 458 rows a clip: several chunks, none crossing a clip
    (1, 512, 32, 2, 3, 3, 0),       # the deep stem layers
    (2, 64, 4, 1, 6, 6, 3),         # another G, k = 3
]
EPS = 1e-5


def clear_of_flips(x, G, gamma, beta, eps, k):
    """True if no float32 evaluation of this input can take another branch than float64 does: a ReLU or a pooling is discontinuous in its
    gradient, so a pre-activation within rounding of 0, or two window values within rounding of each other, sends d(out) to another place and
    shows as an error of the size of the gradient itself -- in ANY fp32 route, the stock one included.  Decided from the float64 values alone.
    The margin per element is 8 x 2^-24 x (|mean| rstd |gamma| + |xhat gamma| + |beta|): the rounding of an fp32 mean, of the scaled
    difference and of the sum, with a factor 8 to spare.  Values that are both <= 0 tie at exactly 0 after the ReLU in every route."""
    C = x.shape[1]
    xh, mean, rstd = xhat_of(x, G, eps)
    gam, bet = gamma.view(1, C, 1, 1, 1), beta.view(1, C, 1, 1, 1)
    pre = xh * gam + bet
    margin = 8 * 2.0 ** -24 * ((_per_channel(mean, C) * _per_channel(rstd, C) * gam).abs() + (xh * gam).abs() + bet.abs())
    if not k:
        return bool((pre.abs() > margin).all())
    pw, mw = _windows(pre, k), _windows(margin, k)
    top, at = pw.max(-1)
    m_top = mw.gather(-1, at[..., None])[..., 0]
    if not bool((top.abs() > m_top).all()):             # the winner's own ReLU
        return False
    rest = pw.clone()
    rest.scatter_(-1, at[..., None], float("-inf"))
    second, at2 = rest.max(-1)
    gap_ok = (top - second > m_top + mw.gather(-1, at2[..., None])[..., 0]) | (top <= -m_top)
    return bool(gap_ok.all())


def draw_clear(case, seed=0, mean=3.0, spread=0.7, tries=8):
    """draw(case, seed + 1000 j, ...) for the first j whose input is clear_of_flips -> (inputs, seed taken)"""
    for j in range(tries):
        inputs = draw(case, seed + 1000 * j, mean, spread)
        if clear_of_flips(inputs[0], case[2], inputs[1], inputs[2], EPS, case[6]):
            return inputs, seed + 1000 * j
    raise AssertionError("no input clear of ReLU / pooling flips among %d seeds from %d" % (tries, seed))


def draw(case, seed=0, mean=3.0, spread=0.7):
    """x = spread N(0, 1) + mean (the mean is not small against the spread), gamma, beta ~ N(0, 1), d(out) ~ N(0, 1): fp32 values as float64"""
    N, C, G, T, H, W, k = case
    gen = torch.Generator().manual_seed(1000 * seed + sum(case))
    x = (spread * torch.randn(N, C, T, H, W, generator=gen) + mean).float().double()
    gamma, beta = torch.randn(C, generator=gen).float().double(), torch.randn(C, generator=gen).float().double()
    shape = (N, C, T, H // k, W // k) if k else (N, C, T, H, W)
    return x, gamma, beta, torch.randn(*shape, generator=gen).float().double()
