"""Several real training steps of the benchmark's C3 graph -- make_c3_step (forward, loss, backward, 1/world, clip) + the
fused optimizer: line for line what bench.py times, plus the optimizer -- with the PARAMETERS compared against float64 (GPU).

Three runs of the same S steps from the same initial parameters (golden.recipe.fill_module) on the same batch:
  truth      oracle.torch_ref.RefAVFeatureGraph.double(), mtl_loss, clip_grad_norm_, torch.optim in float64 (CPU)
  yardstick  the same in float32: stock torch on the CPU, what the reference project itself would compute
  under test m3t.workloads.AVFeatureGraph + make_c3_step + FlatAdam / FlatSGD on the GPU
D_r(G) = ||(p_S^r - p_S^truth) on G|| / ||(p_S^truth - p_0) on G|| for a set of parameters G; asserted: D_gpu(G) <= 4 D_f32(G).
The margin rests on the project's own accuracy claim -- the fp16x3 products are "no less accurate than a sequential fp32 chain"
(tests/test_fp16x3_model.py) -- so the GPU run is one more fp32-accurate implementation and should land near the yardstick; 4
allows for a different summation order amplified over S steps.  A wrong clip coefficient, 1/world, weight decay, stale lr or
a gradient slice written to the wrong offset gives D of 1e-2 .. 1 against a yardstick of 1e-6 .. 5e-4.

G = everything and each top-level group for both optimizers; each single tensor for SGD only: Adam's first updates are
lr * sign(g)-like, so an element whose gradient is of the size of its own rounding error moves by a full lr in either
direction in ANY fp32 implementation (stock fp32 against float64: the worst single tensor is 25x above the global figure
for Adam, 3-4x for SGD).  Per-tensor L2 under SGD is linear in the gradient error and has no such tail.

The Adam cases' max_norm lies inside the range of the truth run's norms (measured once, fixed here) and the test asserts on
the truth run that at least 2 steps are clipped and at least 2 are not; the SGD cases clip every step.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GROUPS = ("audio.", "visual.gru_v.", "visual.gru_a.", "proj_v.", "att_fuse.", "fusion.")
D_A, D_V = 40, 48

CASES = {
    # solo scans (H 128), persistent audio scans (H 256), small slices and their padding
    "a": dict(H=128, B=5, T=20, opt="adam", max_norm=0.5, steps=12),
    # wide H 512 scans, producer-split backward, 20 M+ parameters: multi-sweep optimizer and clip kernels on real gradients
    "b": dict(H=512, B=4, T=12, opt="adam", max_norm=1.5, steps=8),
    "c": dict(H=128, B=5, T=20, opt="sgd", max_norm=0.1, steps=12),             # every step clipped, per-tensor check
    "d": dict(H=512, B=19, T=9, opt="sgd", max_norm=0.1, steps=8),              # ragged row block, full widths
    # lr and momentum change between launches: CyclicLR on a shadow optimizer, copied in as Trainer._sync_hyper does
    "e": dict(H=128, B=5, T=20, opt="sgd", max_norm=0.1, steps=12, cyclic=True),
}
ADAM = dict(lr=1e-3, weight_decay=1e-4)
SGD = dict(lr=1e-2, momentum=0.9, weight_decay=5e-4)
CYCLIC = dict(base_lr=1e-4, max_lr=1e-2, step_size_up=4, cycle_momentum=True)
SEED = 20240
TABLE = []


def _batch(c):
    """features N(0,1); labels smooth functions of the inputs; expression classes uniform, 70 % valid"""
    rs = np.random.RandomState(SEED + c["B"] * 100 + c["T"])
    B, T = c["B"], c["T"]
    xa = rs.standard_normal((B, T, D_A)).astype(np.float32)
    xv = rs.standard_normal((B, T, D_V)).astype(np.float32)
    t = torch.from_numpy
    return dict(x_a=t(xa), x_v=t(xv), valence=t(np.tanh(3 * xa[..., :8].mean(-1)).astype(np.float32)),
                arousal=t(np.tanh(3 * xv[..., :8].mean(-1)).astype(np.float32)),
                class_expr=t(rs.randint(0, 7, (B, T)).astype(np.int64)), expr_valid=t(rs.uniform(size=(B, T)) < 0.7))


def _cpu_run(c, dtype):
    """-> (final parameters as float64 numpy by name, losses, pre-clip norms)"""
    from golden.recipe import fill_module
    from oracle import torch_ref as R
    model = fill_module(R.RefAVFeatureGraph(D_A, D_V, c["H"]), SEED).to(dtype)
    b = _batch(c)
    f = lambda k: b[k].to(dtype)
    params = list(model.parameters())
    sched = None
    if c["opt"] == "adam":
        opt = torch.optim.Adam(params, **ADAM)
    else:
        opt = torch.optim.SGD(params, **SGD)
        if c.get("cyclic"):
            sched = torch.optim.lr_scheduler.CyclicLR(opt, **CYCLIC)
    losses, norms = [], []
    for _ in range(c["steps"]):
        opt.zero_grad()
        loss = R.mtl_loss(model(f("x_a"), f("x_v")), f("valence"), f("arousal"), b["class_expr"], b["expr_valid"])
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_(params, c["max_norm"])))
        opt.step()
        if sched is not None:
            sched.step()
        losses.append(float(loss.detach()))
    return {n: p.detach().double().numpy().copy() for n, p in model.named_parameters()}, np.array(losses), np.array(norms)


def _gpu_run(c):
    from golden.recipe import fill_module
    from m3t import _lib
    from m3t.optim import FlatAdam, FlatSGD
    from m3t.workloads import AVFeatureGraph, make_c3_step
    model = fill_module(AVFeatureGraph(D_A, D_V, c["H"]), SEED).to(DEV)
    batch = {k: v.to(DEV) for k, v in _batch(c).items()}
    ddp, step = make_c3_step(model, batch, max_norm=c["max_norm"], flatten_params=True)
    shadow = sched = None
    if c["opt"] == "adam":
        opt = FlatAdam(ddp, **ADAM)
    else:
        opt = FlatSGD(ddp, **SGD)
        if c.get("cyclic"):
            shadow = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], **SGD)
            sched = torch.optim.lr_scheduler.CyclicLR(shadow, **CYCLIC)
    n0 = _lib.load().m3t_gru_persist_count()
    losses, norms = [], []
    for _ in range(c["steps"]):
        if sched is not None:                                     # Trainer._sync_hyper
            opt.lr, opt.momentum = float(shadow.param_groups[0]["lr"]), float(shadow.param_groups[0]["momentum"])
        loss, _, _ = step()
        opt.step()
        if sched is not None:
            shadow.step()
            sched.step()
        losses.append(float(loss.detach()))
        norms.append(float(ddp.last_norm))
    torch.cuda.synchronize()
    from m3t import ops
    ops.poll_scan_error()
    assert _lib.load().m3t_gru_persist_count() > n0, "the persistent scans did not run"
    # what lies between the parameter slices is exactly zero: gradients, parameters, optimizer state
    covered = torch.zeros(ddp.flat.numel(), dtype=torch.bool, device=DEV)
    for p in model.parameters():
        o = ddp.offsets[id(p)]
        covered[o:o + p.numel()] = True
    assert int((~covered).sum()) > 0
    state = [opt.m, opt.v] if c["opt"] == "adam" else [opt.buf]
    for name, t in [("ddp.flat", ddp.flat), ("flat_params", ddp.flat_params)] + list(zip(("state0", "state1"), state)):
        assert not bool(t[~covered].any()), "%s is not zero on the padding between the slices" % name
    assert opt.t == c["steps"]
    got = {n: p.detach().double().cpu().numpy() for n, p in model.named_parameters()}
    ddp.close()
    return got, np.array(losses), np.array(norms)


def _dist(names, a, b):
    return float(np.sqrt(sum(float(((a[n] - b[n]) ** 2).sum()) for n in names)))


@pytest.mark.parametrize("case", sorted(CASES))
def test_parameters_follow_the_float64_trajectory(case):
    from golden.recipe import fill_module
    from oracle import torch_ref as R
    c = CASES[case]
    p0 = {n: p.detach().double().numpy().copy()
          for n, p in fill_module(R.RefAVFeatureGraph(D_A, D_V, c["H"]), SEED).named_parameters()}
    truth, l64, n64 = _cpu_run(c, torch.float64)
    yard, l32, n32 = _cpu_run(c, torch.float32)
    names = sorted(truth)
    # the truth run exercises what the case is for
    clipped = n64 + 1e-6 > c["max_norm"]
    if c["opt"] == "adam":
        assert clipped.sum() >= 2 and (~clipped).sum() >= 2, "max_norm %g is outside the truth run's norms %s" % (c["max_norm"], n64)
    else:
        assert clipped.all(), n64
    for n in names:
        assert np.linalg.norm(truth[n] - p0[n]) > 0, "%s never moved in the truth run" % n
    assert _dist(names, yard, truth) / _dist(names, truth, p0) > 1e-8, "a yardstick of zero makes the assertion vacuous"

    got, lg, ng = _gpu_run(c)
    assert sorted(got) == names
    sets = [("all", names)] + [(g, [n for n in names if n.startswith(g)]) for g in GROUPS]
    if c["opt"] == "sgd":
        sets += [(n, [n]) for n in names]
    rows, bad = [], []
    for label, G in sets:
        assert G, label
        moved = _dist(G, truth, p0)
        d_gpu, d_f32 = _dist(G, got, truth) / moved, _dist(G, yard, truth) / moved
        rows.append("%-44s D_gpu %.3e  D_f32 %.3e  ratio %.2f" % (label, d_gpu, d_f32, d_gpu / d_f32 if d_f32 > 0 else np.inf))
        if not d_gpu <= 4 * d_f32:
            bad.append(rows[-1])
    # the loss of every step; floor 2e-6: the fp32 resolution of a loss near 2 after a 2-moment CCC
    l_bar = max(4 * float(np.abs(l32 - l64).max()), 2e-6)
    l_err = float(np.abs(lg - l64).max())
    rows.append("loss: max |gpu - truth| %.3e, bar %.3e (yardstick max %.3e)" % (l_err, l_bar, float(np.abs(l32 - l64).max())))
    if not l_err <= l_bar:
        bad.append(rows[-1])
    # the clip norm of every step, relative; floor 1e-6
    n_bar = max(4 * float((np.abs(n32 - n64) / n64).max()), 1e-6)
    n_err = float((np.abs(ng - n64) / n64).max())
    rows.append("norm: max rel |gpu - truth| %.3e, bar %.3e; truth norms %.3f .. %.3f, %d of %d steps clipped" % (
        n_err, n_bar, n64.min(), n64.max(), int(clipped.sum()), len(n64)))
    if not n_err <= n_bar:
        bad.append(rows[-1])
    head = "case %s (H %d, B %d, T %d, %s%s, max_norm %g, %d steps)" % (
        case, c["H"], c["B"], c["T"], c["opt"], " + CyclicLR" if c.get("cyclic") else "", c["max_norm"], c["steps"])
    nset = 1 + len(GROUPS)
    per_tensor = rows[nset:-2]
    shown = rows[:nset] + (["worst single tensor: " + max(per_tensor, key=lambda r: float(r.split()[-1]))] if per_tensor else []) + rows[-2:]
    print("\n".join([head] + shown))
    TABLE.append((head, rows))
    assert not bad, head + ": above 4x the float32 yardstick:\n" + "\n".join(bad) + "\n-- all:\n" + "\n".join(rows)
