"""The float64 statement of the operator that puts the per-frame ResNet v2 (pre-activation) on the channels-last chain (csrc/stem_cl.hip
m3t_add_bn_relu_cl_*), written out by formula, not by autograd: s = a + b and z = relu(bn(s)) over rows [M, C], forward and backward in train and
eval mode, with and without the gradient ds_out that reaches s through its second use (the next identity).  tests/test_resnet_v2_cl_host.py
checks it against torch's float64 autograd on the CPU; the GPU tests compare the kernels with it.  Also here: the draws of the operator cases and
the decision whether an input is clear of ReLU flips, taken from the float64 values and the precision of fp32 alone."""
import torch
import torch.nn.functional as F

import resnet_ref as R

EPS, MOMENTUM, ULP = R.EPS, R.MOMENTUM, R.ULP

# (M, C): fewer rows than row groups; a ragged last chunk over several blocks; eight row groups; four row groups and five chunks; the narrowest C
# with M = 2 (256 row groups, two of them busy); the widest C (one row group) with a ragged second chunk
CASES = [(3, 64), (4099, 64), (24, 512), (1030, 256), (2, 4), (257, 1024)]


def forward(a, b, gamma, beta, run_mean, run_var, training, momentum=MOMENTUM, eps=EPS):
    """s = a + b, z = relu(gamma xhat + beta) with xhat from s -> dict(s, z, pre, xhat, mean, rstd, run_mean, run_var: the running statistics
    AFTER the call)"""
    s = a + b
    mean, rstd = R.stats(s, run_mean, run_var, training, eps)
    xhat = (s - mean) * rstd
    pre = xhat * gamma + beta
    out = dict(s=s, z=torch.relu(pre), pre=pre, xhat=xhat, mean=mean, rstd=rstd, run_mean=run_mean, run_var=run_var)
    if training:
        M = s.shape[0]
        var = ((s - mean) ** 2).mean(0)
        out["run_mean"] = (1 - momentum) * run_mean + momentum * mean
        out["run_var"] = (1 - momentum) * run_var + momentum * (var * M / (M - 1) if M > 1 else var)
    return out


def backward(dz, ds_out, fwd, gamma, training):
    """g = dz (z > 0); dbeta = sum g; dgamma = sum g xhat; ds = (training: gamma rstd (g - mean(g) - xhat mean(g xhat)), eval: g gamma rstd)
    + ds_out (None: nothing to add) -- the gradient of a and of b alike.  -> dict(ds, dgamma, dbeta, colsum: ds's column sums)"""
    g = torch.where(fwd["z"] > 0, dz, torch.zeros_like(dz))
    xhat, rstd = fwd["xhat"], fwd["rstd"]
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    if training:
        M = dz.shape[0]
        ds = gamma * rstd * (g - dbeta / M - xhat * (dgamma / M))
    else:
        ds = g * (gamma * rstd)
    if ds_out is not None:
        ds = ds + ds_out
    return dict(ds=ds, dgamma=dgamma, dbeta=dbeta, colsum=ds.sum(0))


def torch_autograd(a, b, gamma, beta, run_mean, run_var, training, dz, ds_out=None, momentum=MOMENTUM, eps=EPS):
    """the same quantities from torch's own operators and autograd (add -> F.batch_norm -> relu, with a second use of s that carries ds_out), any
    dtype / device.  ds is a's gradient, ds_b is b's: the same values"""
    a, b, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (a, b, gamma, beta))
    rm, rv = run_mean.detach().clone(), run_var.detach().clone()
    s = a + b
    z = torch.relu(F.batch_norm(s, rm, rv, gamma, beta, training, momentum, eps))
    if ds_out is None:
        z.backward(dz)
    else:
        torch.autograd.backward([z, s * 1.0], [dz, ds_out])
    return dict(s=s.detach(), z=z.detach(), ds=a.grad, ds_b=b.grad, dgamma=gamma.grad, dbeta=beta.grad, colsum=a.grad.sum(0), run_mean=rm, run_var=rv)


def margin(fwd, gamma, beta):
    """what fp32 rounding can move a pre-activation by: resnet_ref.tail_margin's BatchNorm terms plus the rounding of the fp32 sum s = a + b
    (half an ulp of s) as it reaches the pre-activation, |s| rstd |gamma| -- with the same factor 8 to spare"""
    return 8 * ULP * ((fwd["mean"] * fwd["rstd"] * gamma).abs() + (fwd["xhat"] * gamma).abs() + beta.abs()
                      + fwd["s"].abs() * fwd["rstd"] * gamma.abs())


def clear_of_flips(a, b, gamma, beta, run_mean, run_var, training):
    """True if no float32 evaluation of this input can take another ReLU branch than float64 does.  Decided from the float64 values alone."""
    f = forward(a, b, gamma, beta, run_mean, run_var, training)
    return bool((f["pre"].abs() > margin(f, gamma, beta)).all())


def draw(case, seed=0):
    """resnet_ref.draw with (a, b) = (x, s) and dz = dy, and ds_out ~ N(0, 1) as the next draw of the same generator -> (a, b, gamma, beta,
    run_mean, run_var, dz, ds_out): fp32 values as float64"""
    M, C = case
    base = R.draw(case, seed)
    gen = torch.Generator().manual_seed(1000 * seed + M + C)      # resnet_ref.draw's generator, advanced past resnet_ref.draw's own draws
    r = lambda *shape: torch.randn(*shape, generator=gen)
    replay = (0.7 * r(M, C) + 1.0, r(M, C), r(M, C), r(C), r(C), 1.0 + 0.1 * r(C), 0.3 + 0.7 * torch.rand(C, generator=gen))
    x, s, dy, gam, bet, rm, rv = (t.float().double() for t in replay)
    for got, want in zip((x, s, gam, bet, rm, rv, dy), base):
        assert torch.equal(got, want), "resnet_ref.draw no longer draws in the order replayed here"
    return base + (r(M, C).float().double(),)


def draw_clear(case, training, seed=0, tries=8):
    """draw(case, seed + 1000 j) for the first j whose input is clear_of_flips -> (inputs, seed taken)"""
    for j in range(tries):
        inputs = draw(case, seed + 1000 * j)
        if clear_of_flips(*inputs[:6], training):
            return inputs, seed + 1000 * j
    raise AssertionError("no input clear of ReLU flips among %d seeds from %d" % (tries, seed))
