"""The float64 statement of BatchNorm (+ReLU) forward and backward, as csrc/bn.hip computes it in its three families (the row kernels behind
`tcn_simple`, the chunked channel-plane kernels of the 3-D stems, the small-plane kernels of the per-frame ResNet) -- written out by formula,
not by autograd.  tests/test_bn_ref_host.py checks it against torch's float64 autograd on the CPU; tests/test_gpu_bn_fp64.py compares the
kernels with it.

One core over planes [N, C, S] (a channel is N planes of S values); rows [M, C] are the same thing with N = 1, S = M, transposed: every
function here takes either layout and answers in the layout it was given.  Also here: the cases, their draws, and the decision whether an
input is clear of ReLU flips -- taken from the float64 values and the precision of fp32 alone."""
import torch
import torch.nn.functional as F

EPS = 1e-5
MOMENTUM = 0.1
ULP = 2.0 ** -24

# (N, C, S) of the plane cases: the smallest that reach each branch of m3t_bn_planes_* (PL_SMALL = 1024, PL_CHUNK = 8192)
PLANE_CASES = [
    (7, 4, 1),          # small, scalar, one lane per plane, 64 planes per wave, 28 planes (ragged workgroup)
    (5, 8, 3),          # small, scalar, four lanes per plane, one idle
    (9, 8, 12),         # small, float4, 3 units on 4 lanes
    (70, 8, 16),        # small, float4, 560 planes = 8.75 workgroups (the ResNet 4 x 4 form)
    (3, 12, 49),        # small, scalar, 49 units on 64 lanes
    (2, 8, 784),        # small, float4, 196 units: four passes, ragged last
    (2, 4, 1023),       # upper edge of PL_SMALL, scalar
    (2, 4, 1024),       # upper edge of PL_SMALL, float4
    (2, 4, 1025),       # first chunked size, scalar
    (2, 4, 1028),       # first chunked size, float4
    (2, 4, 8192),       # exactly one chunk
    (2, 4, 8196),       # a second chunk of one float4
    (2, 4, 8193),       # a second chunk of one float
    (33, 4, 8196),      # 66 partials per channel: the second trip of the final kernel's 64-lane loop
]
UNALIGNED_CASES = [(2, 8, 784), (2, 4, 8192)]      # S % 4 == 0 with every pointer one float off: the scalar sweep
# (M, C) of the row cases (m3t_bn_rows_*)
ROW_CASES = [
    (2, 64),            # smallest train-mode input
    (3, 70),            # C not a multiple of the 64-column workgroup
    (129, 64),          # two chunks, uneven
    (16400, 8),         # the chunk count clamped at 128, short last chunk
    (8200, 512),        # 4 198 400 elements > 4096 x 1024: the grid-stride loops' second trip
]
LARGE_MEAN_CASES = [(6, 8, 784), (70, 8, 16), (2, 4, 8196), (129, 64)]
LARGE_MEANS = [30.0, 1000.0]
# cases whose 1 M to 4 M pre-activations cannot all stay clear of zero within 8 draws (tests/test_bn_ref_host.py): these run without the ReLU
NO_RELU_CASES = [(8200, 512)]


def _planes(t):
    """rows [M, C] -> planes [1, C, M] (a view); planes pass through"""
    return t.t().unsqueeze(0) if t.dim() == 2 else t


def _like(t3, x):
    """planes [1, C, M] back to rows [M, C] if `x` was given as rows"""
    return t3[0].t() if x.dim() == 2 else t3


def stats(x, run_mean, run_var, training, eps=EPS):
    """mean, invstd [C] (and the biased variance): batch statistics over the N S values of a channel when training, the running ones otherwise"""
    if training:
        x3 = _planes(x)
        mean = x3.mean((0, 2))
        var = ((x3 - mean[None, :, None]) ** 2).mean((0, 2))
    else:
        mean, var = run_mean, run_var
    return mean, 1.0 / torch.sqrt(var + eps), var


def forward(x, gamma, beta, run_mean, run_var, training, relu=True, momentum=MOMENTUM, eps=EPS):
    """pre = gamma xhat + beta, y = relu(pre) if relu else pre -> dict(pre, y, xhat, mean, invstd, run_mean, run_var: the running statistics
    AFTER the call -- updated with the unbiased variance, as torch does, when training; the objects given otherwise)"""
    x3 = _planes(x)
    mean, invstd, var = stats(x, run_mean, run_var, training, eps)
    col = lambda v: v[None, :, None]
    xhat = (x3 - col(mean)) * col(invstd)
    pre = xhat * col(gamma) + col(beta)
    y = torch.relu(pre) if relu else pre
    out = dict(pre=_like(pre, x), y=_like(y, x), xhat=_like(xhat, x), mean=mean, invstd=invstd, run_mean=run_mean, run_var=run_var)
    if training:
        count = x3.shape[0] * x3.shape[2]
        out["run_mean"] = (1 - momentum) * run_mean + momentum * mean
        out["run_var"] = (1 - momentum) * run_var + momentum * (var * count / (count - 1) if count > 1 else var)
    return out


def backward(dy, fwd, gamma, training, relu=True):
    """g = dy (y > 0) if relu else dy; dbeta = sum g; dgamma = sum g xhat; training: dx = gamma invstd (g - mean(g) - xhat mean(g xhat)), eval:
    dx = g gamma invstd.  -> dict(dx, dgamma, dbeta)"""
    d3, y3, xh = _planes(dy), _planes(fwd["y"]), _planes(fwd["xhat"])
    g = torch.where(y3 > 0, d3, torch.zeros_like(d3)) if relu else d3
    dbeta, dgamma = g.sum((0, 2)), (g * xh).sum((0, 2))
    col = lambda v: v[None, :, None]
    w = col(gamma * fwd["invstd"])
    if training:
        count = d3.shape[0] * d3.shape[2]
        dx = w * (g - col(dbeta) / count - xh * col(dgamma / count))
    else:
        dx = g * w
    return dict(dx=_like(dx, dy), dgamma=dgamma, dbeta=dbeta)


def torch_autograd(x, gamma, beta, run_mean, run_var, training, relu, dy, momentum=MOMENTUM, eps=EPS):
    """the same quantities from torch's own operators and autograd (F.batch_norm -> relu), in whatever dtype and on whatever device it is
    given.  x: planes [N, C, S] or rows [M, C] (F.batch_norm takes both)"""
    x, gamma, beta = (t.detach().clone().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = run_mean.detach().clone(), run_var.detach().clone()
    y = F.batch_norm(x, rm, rv, gamma, beta, training, momentum, eps)
    if relu:
        y = torch.relu(y)
    y.backward(dy)
    return dict(out=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, run_mean=rm, run_var=rv)


def margin(x, fwd, gamma, beta):
    """what fp32 rounding can move a pre-activation by: 8 x 2^-24 x ((|x| + |mean|) |gamma invstd| + |xhat gamma| + |beta|) -- the rounding of
    an fp32 mean against the input it is taken from (the term that grows with the input's own size: at mean 1000 it is 3e-5 invstd gamma,
    whatever xhat is), of the scaled difference and of the sum, with a factor 8 to spare (as tests/gn_ref.py, tests/resnet_ref.py)"""
    col = lambda v: v[None, :, None]
    w = col((gamma * fwd["invstd"]).abs())
    m = 8 * ULP * ((_planes(x).abs() + col(fwd["mean"].abs())) * w + (_planes(fwd["xhat"]) * col(gamma)).abs() + col(beta.abs()))
    return _like(m, x)


def clear_of_flips(x, gamma, beta, run_mean, run_var, training):
    """True if no float32 evaluation of this input can take another ReLU branch than float64 does (a pre-activation within rounding of 0 flips
    its mask in ANY fp32 route, the stock one included, and is no error of the operator).  Decided from the float64 values alone."""
    f = forward(x, gamma, beta, run_mean, run_var, training, relu=True)
    return bool((f["pre"].abs() > margin(x, f, gamma, beta)).all())


def draw(case, seed=0, mean=1.0, spread=0.7):
    """x = spread N(0, 1) + mean, dy ~ N(0, 1), gamma, beta ~ N(0, 1), running mean ~ mean + 0.1 spread N, running variance in spread^2 [0.3, 1]:
    fp32 values as float64.  case: (N, C, S) -> planes, (M, C) -> rows.  -> (x, gamma, beta, run_mean, run_var, dy)"""
    C = case[1]
    shape = tuple(case)
    gen = torch.Generator().manual_seed(1000 * seed + sum(case))
    r = lambda *s: torch.randn(*s, generator=gen)
    x, dy = spread * r(*shape) + mean, r(*shape)
    gamma, beta = r(C), r(C)
    run_mean, run_var = mean + 0.1 * spread * r(C), spread * spread * (0.3 + 0.7 * torch.rand(C, generator=gen))
    return tuple(t.float().double() for t in (x, gamma, beta, run_mean, run_var, dy))


def draw_clear(case, training, seed=0, mean=1.0, spread=0.7, tries=8):
    """draw(case, seed + 1000 j, ...) for the first j whose input is clear_of_flips -> (inputs, seed taken)"""
    for j in range(tries):
        inputs = draw(case, seed + 1000 * j, mean, spread)
        if clear_of_flips(*inputs[:5], training):
            return inputs, seed + 1000 * j
    raise AssertionError("no input clear of ReLU flips among %d seeds from %d" % (tries, seed))
