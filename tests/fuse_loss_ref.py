"""Float64 reference, fp32 yardstick and error bound for the two operators of csrc/fuse_loss.hip that every training step runs:
the attention-fusion reduction (m3t_att_fuse_fwd / _bwd) and the AffWild2VA loss with its gradient (m3t_va_loss).  Written from
the definitions in include/m3t_hip.h and the reference's models/att_fusion.py:21-25, models/model.py:132-182, models/utils.py:6-17,
not from the kernels.  tests/test_fuse_loss_host.py checks it against torch's float64 autograd; tests/test_gpu_fuse_loss.py uses it.

Definitions (n rows, x a prediction column, t its target)
  ccc      2 cov / (var_x + var_t + (m_x - m_t)^2), cov = sum((x - m_x)(t - m_t)) / n (BIASED), var = sum((x - m)^2) / max(n - 1, 1)
           (UNBIASED; n = 1: the divisor is 1, so both variances and cov are 0, ccc = 0 / (m_x - m_t)^2 -- see `rows == 1` below)
  loss_v   1 - ccc, or mean((x - t)^2) with use_mse; 0 when its weight is 0 (the term is skipped: its column is not read into the loss
           and dy of that column is not touched)
  loss_e   sum over VALID rows of (logsumexp(l[:n_expr]) - l[label]) / n: the mean over ALL rows; added (x expr_w) only when at least
           one row is valid and expr_w != 0
  n_correct  valid rows whose FIRST maximum of l[:n_expr] is the label
  out      {loss, loss_v, loss_a, loss_e, n_valid, n_correct, ccc_v, ccc_a};  dy = dL/dy, zero in every column no term reads
The weights cross the C ABI as `float`: they are rounded to fp32 once, here as there (float(0.3) is 0.300000012: a reference at the
decimal 0.3 would be off by 4e-8 relative, a third of the bound).

rows == 1.  torch's unbiased variance of one element is NaN, so the reference's ccc_loss is NaN on a one-frame batch.  The library
divides by max(n - 1, 1) instead: var = cov = 0, ccc = 0 / (x - t)^2 = 0, loss = 1 and dL/dx = 0 for x != t (NaN for x == t, where the
quotient is 0 / 0).  The mse form and the CE term are unaffected.  This file pins that rule; the yardstick follows it at n = 1.

Yardstick and bound.  E32 of a tensor = the largest error, against float64, of torch's own float32 CPU autograd of the literal
composition (`1 - 2 cov / (x.var() + t.var() + (m1 - m2)^2)`, F.mse_loss, F.cross_entropy(reduction='none') * mask averaged over all
rows, softmax(sigmoid) mixing) on the same inputs.  An element may be off by 4 max(E32, floor): the factor 4 is the project's
allowance for another summation order (tests/test_gpu_pretrain.py).  `floor` is one fp32 ulp of
  * the reference value: f, dx_v, dx_a, the CE columns of dy, the mse gradient;
  * the sum of the absolute values of the terms where the closed form subtracts:
      dy[iv], dy[ia] (ccc)   w (|2 (t - m_t) / (n den)| + |2 cov / den^2| |2 (x - m_x) / (n - 1) + 2 (m_x - m_t) / n|)
      ds_v, ds_a             w0 w1 h (1 - h) (sum |df x_v| + sum |df x_a|)
      loss scalars           max(1, |ref|), since 1 - ccc is formed in fp32
  * never less than the smallest normal fp32 (2^-126): denormal results may be flushed.
The three tensors of dy -- the CE block, the valence column, the arousal column -- have magnitudes apart by orders, so each gets
its own E32.
"""
import numpy as np
import torch
import torch.nn.functional as F

BOUND = 4.0
TINY = 2.0 ** -126
LB = 256              # rows per block of the grid-wide forms
NT = 1024             # threads of the one-workgroup form
OUT_NAMES = ("loss", "loss_v", "loss_a", "loss_expr", "n_valid", "n_correct", "ccc_v", "ccc_a")


def f32(x):
    """the value the C ABI receives"""
    return float(np.float32(x))


def ulp32(a):
    """one fp32 ulp of |a| (elementwise), at least the smallest normal"""
    a = np.minimum(np.abs(np.asarray(a, np.float64)), 3.0e38)
    return np.maximum(np.spacing(a.astype(np.float32)).astype(np.float64), TINY)


# ================================================================================================= VA loss: float64
def _ccc_parts(x, t):
    n = x.size
    mx, mt = x.sum() / n, t.sum() / n
    cov = ((x - mx) * (t - mt)).sum() / n
    nm1 = max(n - 1, 1)
    vx, vt = ((x - mx) ** 2).sum() / nm1, ((t - mt) ** 2).sum() / nm1
    den = vx + vt + (mx - mt) ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        ccc = 2 * cov / den
        t1 = 2 * (t - mt) / (n * den)                                        # d ccc / dx = t1 - t2
        t2 = (2 * cov / den ** 2) * (2 * (x - mx) / nm1 + 2 * (mx - mt) / n)
    return ccc, t1, t2


def va_loss(y, valence, arousal, class_expr, expr_valid, iv, ia, n_expr, w_v, w_a, expr_w, use_mse, floors=False):
    """-> (out[8], dy [rows, C]) in float64; with floors=True also (floor_out[8], floor_dy [rows, C]): the magnitudes whose fp32 ulp
    is the floor of the bound (module docstring)"""
    y = np.asarray(y, np.float64)
    rows, C = y.shape
    w_v, w_a, expr_w = f32(w_v), f32(w_a), f32(expr_w)
    val, aro = np.asarray(valence, np.float64).reshape(rows), np.asarray(arousal, np.float64).reshape(rows)
    out, dy, fdy = np.zeros(8), np.zeros((rows, C)), np.zeros((rows, C))
    for k, (col, t, w) in enumerate(((iv, val, w_v), (ia, aro, w_a))):
        x = y[:, col]
        ccc, t1, t2 = _ccc_parts(x, t)
        out[6 + k] = ccc
        if w == 0.0:
            continue                                                         # skipped entirely: x may hold anything
        if use_mse:
            out[1 + k] = ((x - t) ** 2).sum() / rows
            g = 2 * (x - t) / rows
            mag = np.abs(g)
        else:
            out[1 + k] = 1 - ccc
            g = -(t1 - t2)
            mag = np.abs(t1) + np.abs(t2)
        dy[:, col] += w * g
        fdy[:, col] += w * mag
    out[0] = w_v * out[1] + w_a * out[2]
    if n_expr > 0:
        valid = np.asarray(expr_valid).reshape(rows).astype(bool)
        lab = np.where(valid, np.asarray(class_expr, np.int64).reshape(rows), 0)     # invalid rows: the label is never read
        l = y[:, :n_expr]
        m = l.max(axis=1, keepdims=True)
        e = np.exp(l - m)
        s = e.sum(axis=1, keepdims=True)
        ce = (m[:, 0] + np.log(s[:, 0])) - l[np.arange(rows), lab]
        out[3] = ce[valid].sum() / rows
        out[4] = valid.sum()
        out[5] = (valid & (np.argmax(l, axis=1) == lab)).sum()               # np.argmax: the first maximum
        if out[4] > 0 and expr_w != 0.0:
            out[0] += expr_w * out[3]
            onehot = np.zeros((rows, n_expr))
            onehot[np.arange(rows), lab] = 1.0
            g = (expr_w / rows) * (e / s - onehot) * valid[:, None]
            dy[:, :n_expr] += g
            fdy[:, :n_expr] += np.abs(g)
    if not floors:
        return out, dy
    fout = np.maximum(1.0, np.abs(np.where(np.isfinite(out), out, 1.0)))
    return out, dy, fout, fdy


# ================================================================================================= VA loss: torch composition
class _one_thread:
    """torch's CPU reductions split their input by thread count: one thread makes the yardstick the same number on every machine
    (and 33 000-element reductions are faster without the pool)"""

    def __enter__(self):
        self.n = torch.get_num_threads()
        torch.set_num_threads(1)

    def __exit__(self, *exc):
        torch.set_num_threads(self.n)


def va_loss_torch(*args, **kw):
    with _one_thread():
        return _va_loss_torch(*args, **kw)


def _va_loss_torch(y, valence, arousal, class_expr, expr_valid, iv, ia, n_expr, w_v, w_a, expr_w, use_mse, dtype=torch.float32):
    """the literal composition of the reference's training_step under torch autograd in `dtype` on the CPU -> (out[8], dy) as float64
    numpy.  dtype=torch.float32: the yardstick.  dtype=torch.float64: what tests/test_fuse_loss_host.py holds va_loss against."""
    w_v, w_a, expr_w = f32(w_v), f32(w_a), f32(expr_w)
    yt = torch.from_numpy(np.asarray(y, np.float32)).to(dtype).requires_grad_(True)
    rows = yt.shape[0]
    out = [torch.zeros((), dtype=dtype) for _ in range(8)]
    loss = torch.zeros((), dtype=dtype)
    for k, (col, t, w) in enumerate(((iv, valence, w_v), (ia, arousal, w_a))):
        x = yt[:, col]
        t = torch.from_numpy(np.asarray(t, np.float32).reshape(rows)).to(dtype)
        m1, m2 = x.mean(), t.mean()
        cov = ((x - m1) * (t - m2)).mean()
        if rows > 1:
            ccc = 2 * cov / (x.var() + t.var() + (m1 - m2) ** 2)
        else:                                                                # the library's rule at n = 1 (module docstring)
            ccc = 2 * cov / (((x - m1) ** 2).sum() + ((t - m2) ** 2).sum() + (m1 - m2) ** 2)
        out[6 + k] = ccc.detach()
        if w == 0.0:
            continue
        lk = F.mse_loss(x, t) if use_mse else 1 - ccc
        out[1 + k] = lk.detach()
        loss = loss + w * lk
    if n_expr > 0:
        valid = torch.from_numpy(np.asarray(expr_valid).reshape(rows).astype(bool))
        lab = torch.from_numpy(np.asarray(class_expr, np.int64).reshape(rows))
        lab = torch.where(valid, lab, torch.zeros_like(lab))                 # (F.cross_entropy refuses the markers of missing labels)
        lg = yt[:, :n_expr]
        le = (F.cross_entropy(lg, lab, reduction="none") * valid.to(dtype)).mean()
        out[3], out[4] = le.detach(), valid.sum().to(dtype)
        out[5] = (valid & (torch.argmax(lg.detach(), dim=-1) == lab)).sum().to(dtype)
        if int(valid.sum()) > 0 and expr_w != 0.0:
            loss = loss + expr_w * le
    out[0] = loss.detach()
    if loss.requires_grad:
        loss.backward()
    dy = yt.grad.double().numpy() if yt.grad is not None else np.zeros(tuple(yt.shape))
    return np.array([float(o) for o in out]), dy


# ================================================================================================= the comparison helper
def compare(got, ref, yard, floor_of=None, what=""):
    """worst |got - ref| / max(E32, floor) over the tensor and a message naming the element.  E32 = max |yard - ref|; floor = one fp32
    ulp of `floor_of` (default: the reference value), at least 2^-126.  Where ref is NaN, got must be NaN (else the ratio is inf) and
    the element counts for nothing else.  A non-finite got where ref is finite gives inf."""
    got, ref, yard = (np.asarray(a, np.float64) for a in (got, ref, yard))
    if got.shape != ref.shape:
        return float("inf"), "%s: shape %s, reference %s" % (what, got.shape, ref.shape)
    if ref.size == 0:
        return 0.0, ""
    ok = np.isfinite(ref)
    if not np.array_equal(np.isnan(got), np.isnan(ref)) or not np.isfinite(got[ok]).all():
        return float("inf"), "%s: non-finite values are not where the reference has them" % what
    assert np.isfinite(yard[ok]).all(), "%s: the fp32 yardstick is not finite where the reference is" % what
    e32 = float(np.abs(yard[ok] - ref[ok]).max()) if ok.any() else 0.0
    mag = np.broadcast_to(ref if floor_of is None else np.asarray(floor_of, np.float64), ref.shape)
    floor = ulp32(np.where(ok & np.isfinite(mag), mag, 0.0))
    ratio = np.where(ok, np.abs(np.where(ok, got - ref, 0.0)) / np.maximum(e32, floor), 0.0)
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[i]), "%s%s: got %.9g ref %.9g, E32 %.3g, floor %.3g -> %.2f x" % (
        what, list(i), got[i], ref[i], e32, floor[i], ratio[i])


def dy_groups(C, iv, ia, n_expr, w_v, w_a):
    """the tensors dy consists of: [(name, column index or slice)], and the columns that belong to no term"""
    groups, used = [], set()
    if n_expr > 0:
        groups.append(("dy[ce]", slice(0, n_expr)))
        used.update(range(n_expr))
    if w_v != 0.0:
        groups.append(("dy[iv]", slice(iv, iv + 1)))
        used.add(iv)
    if w_a != 0.0 and not (ia == iv and w_v != 0.0):
        groups.append(("dy[ia]", slice(ia, ia + 1)))
        used.add(ia)
    return groups, [c for c in range(C) if c not in used]


def check_va(got_out, got_dy, case, skip_out=(), detail=None):
    """got: the eight scalars and dy of some fp32 implementation on `case` (a dict of va_loss's arguments).  -> (worst ratio, message).
    n_valid and n_correct must be exact and every dy column outside the terms exactly zero (ratio inf otherwise)."""
    a = case_args(case)
    ref_out, ref_dy, f_out, f_dy = va_loss(*a, floors=True)
    y_out, y_dy = va_loss_torch(*a)
    got_out, got_dy = np.asarray(got_out, np.float64), np.asarray(got_dy, np.float64)
    worst = (0.0, "")
    for k in (4, 5):
        if got_out[k] != ref_out[k]:
            return float("inf"), "%s: got %r, reference %r" % (OUT_NAMES[k], got_out[k], ref_out[k])
    for k in (0, 1, 2, 3, 6, 7):
        if k in skip_out:
            continue
        r = compare(got_out[k], ref_out[k], y_out[k], f_out[k], OUT_NAMES[k])
        worst = max(worst, r)
        if detail is not None:
            detail[OUT_NAMES[k]] = max(detail.get(OUT_NAMES[k], 0.0), r[0])
    groups, free = dy_groups(ref_dy.shape[1], case["iv"], case["ia"], case["n_expr"], f32(case["w_v"]), f32(case["w_a"]))
    for name, sl in groups:
        r = compare(got_dy[:, sl], ref_dy[:, sl], y_dy[:, sl], f_dy[:, sl], name)
        worst = max(worst, r)
        if detail is not None:
            detail[name] = max(detail.get(name, 0.0), r[0])
    if free and np.count_nonzero(got_dy[:, free]):
        return float("inf"), "dy is not zero in a column that belongs to no term"
    return worst


# ================================================================================================= VA loss: the cases
LAYOUTS = {                                    # C, n_expr, iv, ia and the weights a layout fixes (None: the case's)
    "mtl9": dict(C=9, n_expr=7, iv=7, ia=8),
    "va2": dict(C=2, n_expr=0, iv=0, ia=1),
    "gaps12": dict(C=12, n_expr=5, iv=10, ia=6),                    # columns 5, 7, 8, 9, 11 belong to no term
    "ce7": dict(C=7, n_expr=7, iv=0, ia=0, w=(0.0, 0.0, 1.0)),      # AffWild2VA.ce_loss
    "one1": dict(C=1, n_expr=0, iv=0, ia=0, w=(1.0, 0.0, 0.0)),     # AffWild2VA.ccc_loss / mse_loss
}
WEIGHTS = ((0.5, 0.5, 0.8), (0.3, 0.7, 0.8), (1.0, 0.0, 0.0), (0.0, 1.0, 0.8))
STATS = ("normal", "near", "offset", "tiny", "const")
LABELS = ("mixed", "none", "last", "all", "big80", "big1e4", "ties")


def make_case(rows, layout="mtl9", weights=(0.5, 0.5, 0.8), use_mse=0, stats="normal", labels="mixed", seed=0):
    """fp32 inputs of one case.
    stats   normal: predictions N(0, 0.7^2), targets U(-1, 1);  near: predictions = targets + 1e-3 N;  offset: predictions
            0.8 + 1e-3 N;  tiny: predictions 1e-4 N;  const: both prediction columns constant (0.3 and -0.6)
    labels  mixed: 70 % of the rows valid;  none;  last: only the last row;  all;  big80 / big1e4: every logit +-80 / +-1e4 (ties
            everywhere);  ties: logits on a grid of 0.5.  Invalid rows carry label 0 (test_gpu_fuse_loss swaps in -1 and 255)."""
    L = LAYOUTS[layout]
    rs = np.random.RandomState((1000003 * seed + 17 * rows + sum(map(ord, layout + stats + labels)) + 2 * int(use_mse)) % 2 ** 32)
    C, n_expr, iv, ia = L["C"], L["n_expr"], L["iv"], L["ia"]
    w = L.get("w", weights)
    y = (rs.standard_normal((rows, C)) * 0.7).astype(np.float32)
    val, aro = (rs.uniform(-1, 1, rows).astype(np.float32) for _ in range(2))
    noise = rs.standard_normal((rows, 2)).astype(np.float32)
    if layout != "ce7":                                                   # (ce_loss passes zero targets and reads column 0 as a logit)
        for k, (col, t) in enumerate(((iv, val), (ia, aro))):
            if stats == "near":
                y[:, col] = t + np.float32(1e-3) * noise[:, k]
            elif stats == "offset":
                y[:, col] = np.float32(0.8) + np.float32(1e-3) * noise[:, k]
            elif stats == "tiny":
                y[:, col] = np.float32(1e-4) * noise[:, k]
            elif stats == "const":
                y[:, col] = np.float32((0.3, -0.6)[k])
    else:
        val[:] = 0
        aro[:] = 0
    cls = rs.randint(0, max(n_expr, 1), rows).astype(np.int64)
    valid = rs.uniform(size=rows) < 0.7
    if n_expr > 0:
        if labels == "none":
            valid[:] = False
        elif labels == "last":
            valid[:] = False
            valid[-1] = True
        elif labels == "all":
            valid[:] = True
        elif labels in ("big80", "big1e4"):
            mag = 80.0 if labels == "big80" else 1e4
            y[:, :n_expr] = np.where(rs.uniform(size=(rows, n_expr)) < 0.5, -mag, mag).astype(np.float32)
        elif labels == "ties":
            y[:, :n_expr] = np.round(y[:, :n_expr] * 2) / 2
    cls[~valid] = 0
    return dict(y=y, valence=val, arousal=aro, class_expr=cls, expr_valid=valid.astype(np.uint8), iv=iv, ia=ia, n_expr=n_expr,
                w_v=w[0], w_a=w[1], expr_w=w[2], use_mse=int(use_mse),
                name="%s-r%d-w%g_%g_%g-%s-%s-%s" % (layout, rows, w[0], w[1], w[2], "mse" if use_mse else "ccc", stats, labels))


def case_args(c):
    return (c["y"], c["valence"], c["arousal"], c["class_expr"], c["expr_valid"], c["iv"], c["ia"], c["n_expr"], c["w_v"], c["w_a"],
            c["expr_w"], c["use_mse"])


FORM_ROWS = {                                   # the row counts at which each form is run
    "one": (1, 2, 63, 64, 65, 1023, 1024),      # ops.va_loss
    "one_nows": (1025, 2500),                   # C ABI, ws = NULL: several rows per thread, ragged
    "fused": (1025, 4097, 32768),               # five blocks, the last holds one row .. the 128-block limit
    "three": (32769, 33000),                    # 129 blocks, the last holds one row
}
OPTION_ROWS = {"one": 65, "one_nows": 1025, "fused": 1025, "three": 32769}      # where the option matrix runs on each form


def emu_form(form):
    return {"one": "one", "one_nows": "one", "fused": "fused", "three": "three"}[form]


def admitted(form, stats, use_mse):
    """Which (form, statistics class) pairs run on the GPU.  tests/test_fuse_loss_host.py measures each form's emulation against the
    bound on every class over 20 seeds; a form whose emulation cannot hold half the bound (ratio 2) on a class is not run on that
    class (no wider bound instead).  With the sums and the closed form in fp64 every form holds it on every class -- 'offset'
    (predictions 0.8 + 1e-3 N) included, where the fp32 three-launch arithmetic gave 3 - 6 x the unit at 33 000 rows and the fp32
    one-workgroup arithmetic 16.7 x at two rows -- so nothing is excluded; the hook stays for the day a form changes."""
    return True


def option_cases(rows):
    """the option matrix at one row count: layouts x use_mse x weights (on the layouts that take weights), then the label and
    statistics classes on the 9-column layout"""
    out = []
    for layout in LAYOUTS:
        for use_mse in (0, 1):
            ws = (None,) if "w" in LAYOUTS[layout] else WEIGHTS
            if layout == "ce7" and use_mse:
                continue
            for w in ws:
                out.append(make_case(rows, layout, w or (0.5, 0.5, 0.8), use_mse, seed=len(out)))
    for labels in LABELS[1:]:
        out.append(make_case(rows, "mtl9", labels=labels, seed=len(out)))
        out.append(make_case(rows, "ce7", labels=labels, seed=len(out)))
    for stats in STATS[1:]:
        for use_mse in (0, 1):
            out.append(make_case(rows, "mtl9", (0.3, 0.7, 0.8), use_mse, stats=stats, seed=len(out)))
        out.append(make_case(rows, "one1", stats=stats, seed=len(out)))
    return out


# ================================================================================================= VA loss: fp32 emulations of the forms
_F = np.float32


def _tree64(v):
    """the xor butterfly of wave_sum over the last axis (64 lanes): every lane ends with the same sum; lane 0 is returned"""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _serial(v, axis=0):
    """left-to-right fp32 sum along `axis`"""
    v = np.moveaxis(np.asarray(v, _F), axis, 0)
    acc = np.zeros(v.shape[1:], _F)
    for r in v:
        acc = acc + r
    return acc


def _sum_one(terms):
    """one workgroup of 1024 threads: thread t adds rows t, t + 1024, ... in order; wave butterflies; the 16 wave sums in order"""
    terms = np.asarray(terms, _F)
    pad = (-terms.size) % NT
    per_thread = _serial(np.concatenate([terms, np.zeros(pad, _F)]).reshape(-1, NT))
    return _serial(_tree64(per_thread.reshape(NT // 64, 64)))


def _sum_blocks(terms):
    """256-row blocks, one row per thread: wave butterflies, the 4 wave sums in order; then the block sums in block order"""
    terms = np.asarray(terms, _F)
    pad = (-terms.size) % LB
    blocks = np.concatenate([terms, np.zeros(pad, _F)]).reshape(-1, LB // 64, 64)
    return _serial(_serial(_tree64(blocks), axis=1))


def _ce_rows32(l, lab, valid, legacy=False):
    """per-row CE terms of the valid rows (0 elsewhere), fp32 exp(l - m) and their fp32 sums.  CE = fp32 log(sum) + (m - l[label]), the
    sum exact (fp64); `legacy`: (m + log(sum)) - l[label] in fp32 as the kernels had it, which rounds at the magnitude of the logits
    (2e-6 at +-80)"""
    m = l.max(axis=1)
    e = np.exp(l - m[:, None])                                               # float32 in, float32 out
    se = _serial(e, axis=1)
    ll = l[np.arange(l.shape[0]), lab]
    ce = ((m + np.log(se)) - ll).astype(_F) if legacy else np.log(se).astype(np.float64) + (m.astype(np.float64) - ll)
    return np.where(valid, ce, 0), e, se


def va_loss_emulated_fp32(form, y, valence, arousal, class_expr, expr_valid, iv, ia, n_expr, w_v, w_a, expr_w, use_mse):
    """numpy restatement of the arithmetic the three forms had BEFORE they moved their sums and closed form to fp64: 'one' (strided
    per-thread fp32 sums plus tree), 'three' (256-row block trees summed in block order in fp32, two passes), 'fused' (fp64 raw
    moments, rounded to fp32 before an fp32 closed form).  One rounding per operation, no contraction.  Kept as the record of why they
    moved (tests/test_fuse_loss_host.py: it breaks the bound), not as a model of the library.  -> (out[8], dy) as float32"""
    y = np.asarray(y, _F)
    rows, C = y.shape
    val, aro = np.asarray(valence, _F).reshape(rows), np.asarray(arousal, _F).reshape(rows)
    wv, wa, ew = _F(w_v), _F(w_a), _F(expr_w)
    invn = _F(1) / _F(rows)
    nm1 = _F(1) / _F(max(rows - 1, 1))
    S = _sum_one if form == "one" else _sum_blocks
    st = []
    for col, t in ((iv, val), (ia, aro)):
        x = y[:, col]
        if form == "fused":
            xd, td, n = x.astype(np.float64), t.astype(np.float64), float(rows)
            mxd, mtd = xd.sum() / n, td.sum() / n
            cvd, xvd, tvd = (xd * td).sum() - n * mxd * mtd, (xd * xd).sum() - n * mxd * mxd, (td * td).sum() - n * mtd * mtd
            n1 = 1.0 / max(rows - 1, 1)
            with np.errstate(invalid="ignore"):
                mx, mt, cov = _F(mxd), _F(mtd), _F(cvd / n)
                den = _F(xvd * n1 + tvd * n1 + (mxd - mtd) * (mxd - mtd))
                mse = _F(((xd - td) ** 2).sum() / n)
        else:
            mx, mt = S(x) * invn, S(t) * invn
            cov = S((x - mx) * (t - mt)) * invn
            den = S((x - mx) * (x - mx)) * nm1 + S((t - mt) * (t - mt)) * nm1 + (mx - mt) * (mx - mt)
            mse = S((x - t) * (x - t)) * invn
        st.append((x, t, mx, mt, cov, den, mse))
    out, dy = np.zeros(8, _F), np.zeros((rows, C), _F)
    use_e = False
    if n_expr > 0:
        valid = np.asarray(expr_valid).reshape(rows).astype(bool)
        lab = np.where(valid, np.asarray(class_expr, np.int64).reshape(rows), 0)
        l = y[:, :n_expr]
        ce, e, se = _ce_rows32(l, lab, valid, legacy=True)
        out[3] = _F(ce.astype(np.float64).sum() / rows) if form == "fused" else S(ce) * invn
        out[4] = valid.sum()
        out[5] = (valid & (np.argmax(l, axis=1) == lab)).sum()
        use_e = out[4] > 0 and ew != 0
        if use_e:
            onehot = np.zeros((rows, n_expr), _F)
            onehot[np.arange(rows), lab] = 1
            dy[:, :n_expr] = np.where(valid[:, None], (ew * invn) * (e / se[:, None] - onehot), _F(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, ((x, t, mx, mt, cov, den, mse), w, col) in enumerate(zip(st, (wv, wa), (iv, ia))):
            ccc = _F(2) * cov / den
            out[6 + k] = ccc
            if w == 0:
                continue
            if use_mse:
                out[1 + k] = mse
                g = _F(2) * (x - t) * invn
            else:
                out[1 + k] = _F(1) - ccc
                g = -(_F(2) * (t - mt) * invn / den - (_F(2) * cov / (den * den)) * (_F(2) * (x - mx) * nm1 + _F(2) * (mx - mt) * invn))
            dy[:, col] = dy[:, col] + w * g
        out[0] = wv * out[1] + wa * out[2] + (ew * out[3] if use_e else _F(0))
    assert out.dtype == _F and dy.dtype == _F
    return out, dy


def va_loss_emulated(form, y, valence, arousal, class_expr, expr_valid, iv, ia, n_expr, w_v, w_a, expr_w, use_mse):
    """numpy restatement of one form's ARITHMETIC as csrc/fuse_loss.hip has it: every sum over rows in fp64 (their order is then
    immaterial at the bound's scale), 'one' and 'three' from moments centred in a second pass, 'fused' from raw moments; the closed
    form and each row's regression gradient in fp64, rounded to fp32 once; of the cross entropy l - max, exp, their sum over the
    classes and its log are fp32 (numpy's float32 exp / log, one rounding per operation), what combines them is fp64.
    -> (out[8], dy) as float32"""
    y = np.asarray(y, _F)
    rows, C = y.shape
    val, aro = np.asarray(valence, _F).reshape(rows), np.asarray(arousal, _F).reshape(rows)
    wv, wa, ew = _F(w_v), _F(w_a), _F(expr_w)
    n = float(rows)
    invn, nm1 = 1.0 / n, 1.0 / max(rows - 1, 1)
    out64, dy = np.zeros(8), np.zeros((rows, C), _F)
    use_e = False
    if n_expr > 0:
        valid = np.asarray(expr_valid).reshape(rows).astype(bool)
        lab = np.where(valid, np.asarray(class_expr, np.int64).reshape(rows), 0)
        l = y[:, :n_expr]
        ce, e, se = _ce_rows32(l, lab, valid)
        out64[3] = ce.astype(np.float64).sum() * invn
        out64[4] = valid.sum()
        out64[5] = (valid & (np.argmax(l, axis=1) == lab)).sum()
        use_e = out64[4] > 0 and ew != 0
        if use_e:
            onehot = np.zeros((rows, n_expr), _F)
            onehot[np.arange(rows), lab] = 1
            sc = float(ew) * invn
            g = e.astype(np.float64) * (sc / se.astype(np.float64))[:, None] - sc * onehot
            dy[:, :n_expr] = np.where(valid[:, None], g, 0.0).astype(_F)
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, (col, t, w) in enumerate(((iv, val, wv), (ia, aro, wa))):
            x, t = y[:, col].astype(np.float64), t.astype(np.float64)
            mx, mt = x.sum() * invn, t.sum() * invn
            if form == "fused":
                cv, xv, tv = (x * t).sum() - n * mx * mt, (x * x).sum() - n * mx * mx, (t * t).sum() - n * mt * mt
            else:
                cv, xv, tv = ((x - mx) * (t - mt)).sum(), ((x - mx) * (x - mx)).sum(), ((t - mt) * (t - mt)).sum()
            cov, den = cv * invn, xv * nm1 + tv * nm1 + (mx - mt) * (mx - mt)
            ccc, q = 2.0 * cov / den, 2.0 * cov / (den * den)
            out64[6 + k] = ccc
            if w == 0:
                continue
            if use_mse:
                out64[1 + k] = ((x - t) * (x - t)).sum() * invn
                g = 2.0 * (x - t) * invn
            else:
                out64[1 + k] = 1.0 - ccc
                g = -((2.0 * invn / den) * (t - mt) - (q * 2.0 * nm1) * (x - mx) - q * 2.0 * (mx - mt) * invn)
            dy[:, col] = dy[:, col] + (float(w) * g).astype(_F)
    out64[0] = float(wv) * out64[1] + float(wa) * out64[2] + (float(ew) * out64[3] if use_e else 0.0)
    return out64.astype(_F), dy


# ================================================================================================= attention fusion
def _sigmoid(s):
    with np.errstate(over="ignore"):
        e = np.exp(-np.abs(s))
    return np.where(np.isnan(s), s, np.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e)))        # (a NaN score stays NaN)


def att_weights(s_v, s_a):
    """h_v, h_a = sigmoid(s); (w0, w1) = softmax([h_v, h_a]), index 0 = VIDEO"""
    hv, ha = _sigmoid(np.asarray(s_v, np.float64)), _sigmoid(np.asarray(s_a, np.float64))
    m = np.maximum(hv, ha)
    ev, ea = np.exp(hv - m), np.exp(ha - m)
    return hv, ha, ev / (ev + ea), ea / (ev + ea)


def att_fuse_fwd(s_v, s_a, x_v, x_a):
    """s [rows], x [rows, D] -> f [rows, D]"""
    _, _, w0, w1 = att_weights(s_v, s_a)
    return w0[:, None] * np.asarray(x_v, np.float64) + w1[:, None] * np.asarray(x_a, np.float64)


def att_fuse_bwd(df, s_v, s_a, x_v, x_a, floors=False):
    """-> (ds_v, ds_a, dx_v, dx_a); with floors=True also the magnitude whose ulp floors ds_v and ds_a:
    w0 w1 h (1 - h) (sum |df x_v| + sum |df x_a|) -- ds_v = w0 w1 h_v (1 - h_v) (sum df x_v - sum df x_a), and ds_a likewise"""
    df, x_v, x_a = (np.asarray(a, np.float64) for a in (df, x_v, x_a))
    hv, ha, w0, w1 = att_weights(s_v, s_a)
    d0, d1 = (df * x_v).sum(-1), (df * x_a).sum(-1)
    dot = w0 * d0 + w1 * d1
    ds_v, ds_a = w0 * (d0 - dot) * hv * (1 - hv), w1 * (d1 - dot) * ha * (1 - ha)
    res = (ds_v, ds_a, w0[:, None] * df, w1[:, None] * df)
    if not floors:
        return res
    mag = np.abs(df * x_v).sum(-1) + np.abs(df * x_a).sum(-1)
    with np.errstate(invalid="ignore"):
        return res + (w0 * w1 * hv * (1 - hv) * mag, w0 * w1 * ha * (1 - ha) * mag)


def att_fuse_torch(*args, **kw):
    with _one_thread():
        return _att_fuse_torch(*args, **kw)


def _att_fuse_torch(df, s_v, s_a, x_v, x_a, dtype=torch.float32):
    """models/att_fusion.py:21-25 under torch autograd on the CPU -> dict(f, ds_v, ds_a, dx_v, dx_a) as float64 numpy"""
    t = [torch.from_numpy(np.asarray(a, np.float32)).to(dtype).requires_grad_(True) for a in (s_v, s_a, x_v, x_a)]
    sv, sa, xv, xa = t
    h = torch.cat((torch.sigmoid(sv).unsqueeze(-1), torch.sigmoid(sa).unsqueeze(-1)), dim=-1)
    h = F.softmax(h, dim=-1)
    f = h[..., 0].unsqueeze(-1) * xv + h[..., 1].unsqueeze(-1) * xa
    f.backward(torch.from_numpy(np.asarray(df, np.float32)).to(dtype))
    names = ("ds_v", "ds_a", "dx_v", "dx_a")
    res = {n: a.grad.double().numpy() for n, a in zip(names, t)}
    res["f"] = f.detach().double().numpy()
    return res


def check_att(got, df, s_v, s_a, x_v, x_a, only=None):
    """got: dict with any of f, ds_v, ds_a, dx_v, dx_a from an fp32 implementation -> (worst ratio, message)"""
    ref = dict(zip(("ds_v", "ds_a", "dx_v", "dx_a", "fl_v", "fl_a"), att_fuse_bwd(df, s_v, s_a, x_v, x_a, floors=True)))
    ref["f"] = att_fuse_fwd(s_v, s_a, x_v, x_a)
    yard = att_fuse_torch(df, s_v, s_a, x_v, x_a)
    worst = (0.0, "")
    for k in only or ("f", "ds_v", "ds_a", "dx_v", "dx_a"):
        fl = {"ds_v": ref["fl_v"], "ds_a": ref["fl_a"]}.get(k)
        worst = max(worst, compare(got[k], ref[k], yard[k], fl, k))
    return worst


def make_att(rows, D, seed=0, score_scale=1.0):
    rs = np.random.RandomState(7919 * seed + 31 * rows + D)
    s_v, s_a = ((rs.standard_normal(rows) * score_scale).astype(np.float32) for _ in range(2))
    x_v, x_a, df = (rs.standard_normal((rows, D)).astype(np.float32) for _ in range(3))
    return df, s_v, s_a, x_v, x_a
