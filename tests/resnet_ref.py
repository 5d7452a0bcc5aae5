"""The float64 statement of the two operators that put the per-frame ResNet (v1) on the channels-last chain (csrc/stem_cl.hip
m3t_bn_add_relu_cl_* / m3t_mean_cl_*), written out by formula, not by autograd: the block tail relu(bn(x) + s) over rows [M, C], forward and
backward in train and eval mode, and the spatial mean [P, HW, C] -> [P, C].  tests/test_resnet_cl_host.py checks it against torch's float64
autograd on the CPU; the GPU tests compare the kernels with it.  Also here: the draws of the operator cases, the decision whether an input is
clear of ReLU (and pooling) flips -- taken from the float64 values and the precision of fp32 alone -- for one operator and for a whole
float64 front-end."""
import torch
import torch.nn.functional as F

EPS = 1e-5
MOMENTUM = 0.1
ULP = 2.0 ** -24

# (M, C) of the block-tail cases, (P, HW, C) of the mean's
TAIL_CASES = [(3, 64), (4099, 64), (24, 512), (1030, 256)]
MEAN_CASES = [(5, 1, 512), (5, 12, 512), (6, 49, 64), (1, 16, 256)]


def stats(x, run_mean, run_var, training, eps=EPS):
    """mean, rstd [C]: batch statistics (biased variance) when training, the running ones otherwise"""
    if training:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)
    else:
        mean, var = run_mean, run_var
    return mean, 1.0 / torch.sqrt(var + eps)


def forward(x, s, gamma, beta, run_mean, run_var, training, momentum=MOMENTUM, eps=EPS):
    """y = relu(gamma xhat + beta + s) -> dict(y, pre, xhat, mean, rstd, run_mean, run_var: the running statistics AFTER the call)"""
    mean, rstd = stats(x, run_mean, run_var, training, eps)
    xhat = (x - mean) * rstd
    pre = xhat * gamma + beta + s
    out = dict(y=torch.relu(pre), pre=pre, xhat=xhat, mean=mean, rstd=rstd, run_mean=run_mean, run_var=run_var)
    if training:
        M = x.shape[0]
        var = ((x - mean) ** 2).mean(0)
        out["run_mean"] = (1 - momentum) * run_mean + momentum * mean
        out["run_var"] = (1 - momentum) * run_var + momentum * (var * M / (M - 1) if M > 1 else var)
    return out


def backward(dy, fwd, gamma, training):
    """g = dy (y > 0); ds = g; dbeta = sum g; dgamma = sum g xhat; training: dx = gamma rstd (g - mean(g) - xhat mean(g xhat)), eval: dx = g gamma
    rstd.  -> dict(dx, ds, dgamma, dbeta, colsum: dx's column sums)"""
    g = torch.where(fwd["y"] > 0, dy, torch.zeros_like(dy))
    xhat, rstd = fwd["xhat"], fwd["rstd"]
    dbeta, dgamma = g.sum(0), (g * xhat).sum(0)
    if training:
        M = dy.shape[0]
        dx = gamma * rstd * (g - dbeta / M - xhat * (dgamma / M))
    else:
        dx = g * (gamma * rstd)
    return dict(dx=dx, ds=g, dgamma=dgamma, dbeta=dbeta, colsum=dx.sum(0))


def torch_autograd(x, s, gamma, beta, run_mean, run_var, training, dy, momentum=MOMENTUM, eps=EPS):
    """the same quantities from torch's own operators and autograd (F.batch_norm -> add -> relu), any dtype / device"""
    x, s, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (x, s, gamma, beta))
    rm, rv = run_mean.detach().clone(), run_var.detach().clone()
    y = torch.relu(F.batch_norm(x, rm, rv, gamma, beta, training, momentum, eps) + s)
    y.backward(dy)
    return dict(out=y.detach(), dx=x.grad, ds=s.grad, dgamma=gamma.grad, dbeta=beta.grad, colsum=x.grad.sum(0), run_mean=rm, run_var=rv)


def mean_forward(x):
    """[P, HW, C] -> [P, C]"""
    return x.mean(1)


def mean_backward(dy, HW):
    """[P, C] -> [P, HW, C]"""
    return (dy / HW)[:, None, :].expand(-1, HW, -1).contiguous()


def tail_margin(fwd, s, gamma, beta):
    """what fp32 rounding can move a pre-activation by: 8 x 2^-24 x (|mean| rstd |gamma| + |xhat gamma| + |beta| + |s|) -- the rounding of an fp32
    mean, of the scaled difference and of the two sums, with a factor 8 to spare (as tests/gn_ref.py, plus the shortcut's term)"""
    return 8 * ULP * ((fwd["mean"] * fwd["rstd"] * gamma).abs() + (fwd["xhat"] * gamma).abs() + beta.abs() + s.abs())


def clear_of_flips(x, s, gamma, beta, run_mean, run_var, training):
    """True if no float32 evaluation of this input can take another ReLU branch than float64 does (a pre-activation within rounding of 0 flips
    its mask in ANY fp32 route, the stock one included, and is no error of the operator).  Decided from the float64 values alone."""
    f = forward(x, s, gamma, beta, run_mean, run_var, training)
    return bool((f["pre"].abs() > tail_margin(f, s, gamma, beta)).all())


def draw(case, seed=0, zero_gamma=False):
    """x = 0.7 N(0, 1) + 1, s, dy ~ N(0, 1), gamma, beta ~ N(0, 1), running mean ~ 1 + 0.1 N, running variance in [0.3, 1]: fp32 values as float64"""
    M, C = case
    gen = torch.Generator().manual_seed(1000 * seed + M + C)
    r = lambda *shape: torch.randn(*shape, generator=gen)
    x, s, dy = 0.7 * r(M, C) + 1.0, r(M, C), r(M, C)
    gamma, beta = r(C), r(C)
    run_mean, run_var = 1.0 + 0.1 * r(C), 0.3 + 0.7 * torch.rand(C, generator=gen)
    if zero_gamma:
        gamma, beta = torch.zeros(C), torch.zeros(C)
    return tuple(t.float().double() for t in (x, s, gamma, beta, run_mean, run_var, dy))


def draw_clear(case, training, seed=0, tries=8):
    """draw(case, seed + 1000 j) for the first j whose input is clear_of_flips -> (inputs, seed taken)"""
    for j in range(tries):
        inputs = draw(case, seed + 1000 * j)
        if clear_of_flips(*inputs[:6], training):
            return inputs, seed + 1000 * j
    raise AssertionError("no input clear of ReLU flips among %d seeds from %d" % (tries, seed))


def draw_mean(case, seed=0):
    P, HW, C = case
    gen = torch.Generator().manual_seed(1000 * seed + P + HW + C)
    return (torch.randn(P, HW, C, generator=gen) + 0.5).float().double(), torch.randn(P, C, generator=gen).float().double()


# ---- a whole float64 front-end (models.backbone.VA_3DResNet, resnet_ver='v1', on the CPU: every module takes its stock operator) ----------------
VIDEO_SHAPE = (2, 3, 3, 52, 44)


def draw_video(seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(*VIDEO_SHAPE, generator=gen).float().double()


def _bn_pre(m, x):
    """the BatchNorm's output (before any ReLU) and its rounding margin, from the module's parameters -- nothing of the module is updated"""
    if m.training:
        dims = [0] + list(range(2, x.dim()))
        mean, var = x.mean(dims), x.var(dims, unbiased=False)
    else:
        mean, var = m.running_mean, m.running_var
    shape = [1, -1] + [1] * (x.dim() - 2)
    rstd = 1.0 / torch.sqrt(var + m.eps)
    mean, rstd, gam, bet = (t.view(shape) for t in (mean, rstd, m.weight, m.bias))
    xg = (x - mean) * rstd * gam
    return xg + bet, 8 * ULP * ((mean * rstd * gam).abs() + xg.abs() + bet.abs())


def _pool_clear(y, margin, k, s, p):
    """max pooling of frames [P, C, H, W]: in every window the largest value leads the second by more than both margins -- or the window is
    all zero behind the ReLU (values <= 0 tie at exactly 0 in every route and the first of them wins everywhere)"""
    P, C, H, W = y.shape
    yw = F.unfold(F.pad(y, (p, p, p, p), value=float("-inf")), k, stride=s).view(P, C, k * k, -1)
    mw = F.unfold(F.pad(margin, (p, p, p, p), value=0.0), k, stride=s).view(P, C, k * k, -1)
    top2, at = yw.topk(2, dim=2)
    m2 = mw.gather(2, at)
    ok = (top2[:, :, 0] - top2[:, :, 1] > m2[:, :, 0] + m2[:, :, 1]) | (top2[:, :, 0] == 0)
    return bool(ok.all())


def model_clear_of_flips(model, video):
    """run the float64 CPU module once (grad off) and decide, from its values and the precision of fp32 alone, whether any ReLU or the stem's
    pooling could go the other way in an fp32 route: every BatchNorm + ReLU, every block tail relu(bn2(.) + shortcut), the pooling's windows.
    (Margins are the rounding of the operator that makes the decision, as for one operator above.)  The module's buffers are put back."""
    from models.resnet import BasicBlock, PlaneBatchNorm2d
    from models.backbone import BatchNorm3dReLU, SpatialMaxPool3d
    import copy
    state = copy.deepcopy(model.state_dict())
    verdict, hooks, stem = [], [], {}

    def bn_relu(m, inp, out):
        pre, margin = _bn_pre(m, inp[0])
        verdict.append(bool((pre.abs() > margin).all()))
        if isinstance(m, BatchNorm3dReLU):
            stem["margin"] = margin.expand_as(pre)

    def pool(m, inp, out):
        y = inp[0]
        fr = lambda t: t.transpose(1, 2).reshape(-1, t.size(1), t.size(3), t.size(4))
        verdict.append(_pool_clear(fr(y), fr(stem["margin"].contiguous()), m.kernel_size[1], m.stride[1], m.padding[1]))

    def tail(m, inp, out):
        x = inp[0]
        shortcut = x if m.downsample is None else m.downsample(x)
        z = m.conv2(m.bn1(m.conv1(x)))
        pre, margin = _bn_pre(m.bn2, z)
        verdict.append(bool(((pre + shortcut).abs() > margin + 8 * ULP * shortcut.abs()).all()))

    for m in model.modules():
        if isinstance(m, (BatchNorm3dReLU,)) or (isinstance(m, PlaneBatchNorm2d) and m.fuse_relu):
            hooks.append(m.register_forward_hook(bn_relu))
        elif isinstance(m, SpatialMaxPool3d):
            hooks.append(m.register_forward_hook(pool))
        elif isinstance(m, BasicBlock):
            hooks.append(m.register_forward_hook(tail))
    try:
        with torch.no_grad():
            model(video)
    finally:
        for h in hooks:
            h.remove()
        model.load_state_dict(state)
    return all(verdict)


def pick_video(model, seed, tries=8):
    """the first of draw_video(seed + 1000 j) that is model_clear_of_flips -> (video, seed taken)"""
    for j in range(tries):
        v = draw_video(seed + 1000 * j)
        if model_clear_of_flips(model, v):
            return v, seed + 1000 * j
    raise AssertionError("no video clear of ReLU / pooling flips among %d seeds from %d" % (tries, seed))
