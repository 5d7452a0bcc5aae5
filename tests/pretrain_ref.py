"""Float64 numpy restatement of the loss end of the pre-training tasks (m3t.ops.temporal_pool / cls_loss / pooled_cls_loss,
csrc/cls_loss.hip), written from the definitions -- reference models/vox2_model.py:58-67 (F.cross_entropy, argmax == label),
models/audioset_model.py:34-49 (temporal max, F.binary_cross_entropy_with_logits, target at the argmax) -- and not from the kernels.
tests/test_pretrain_host.py checks it against torch's own float64 autograd; the GPU tests use it as their reference."""
import numpy as np

MAX, MEAN = 0, 1
CE, BCE = 0, 1


def _first_argmax(a, axis):
    """index of the first maximum along `axis`, a NaN above every number (np.argmax: the first NaN wins, as in torch)"""
    return np.argmax(a, axis=axis)


def tpool_fwd(z, mode):
    """z [B,T,C] -> (pooled [B,C], arg [B,C] int or None)"""
    z = np.asarray(z, np.float64)
    if mode == MEAN:
        return z.sum(axis=1) / z.shape[1], None
    arg = _first_argmax(z, 1)
    return np.take_along_axis(z, arg[:, None, :], axis=1)[:, 0, :], arg


def tpool_bwd(dpooled, arg, T, mode):
    """dL/dz [B,T,C]: the pooled gradient at the frame of the maximum (zero elsewhere), or a T-th of it at every frame"""
    dpooled = np.asarray(dpooled, np.float64)
    B, C = dpooled.shape
    if mode == MEAN:
        return np.repeat((dpooled / T)[:, None, :], T, axis=1)
    dz = np.zeros((B, T, C))
    np.put_along_axis(dz, arg[:, None, :], dpooled[:, None, :], axis=1)
    return dz


def cls_loss(x, target, kind):
    """per-clip logits x [B,C] -> (loss, n_correct, correct [B], dL/dx [B,C])"""
    x = np.asarray(x, np.float64)
    B, C = x.shape
    top = _first_argmax(x, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        if kind == CE:
            y = np.asarray(target, np.int64)
            m = x.max(axis=1, keepdims=True)
            e = np.exp(x - m)
            s = e.sum(axis=1, keepdims=True)
            lse = np.log(s[:, 0]) + m[:, 0]
            loss = (lse - x[np.arange(B), y]).sum() / B
            onehot = np.zeros((B, C))
            onehot[np.arange(B), y] = 1.0
            dx = (e / s - onehot) / B
            correct = (top == y).astype(np.float64)
        else:
            y = np.asarray(target, np.float64)
            e = np.exp(-np.abs(x))
            loss = (np.where(x > 0, x, 0.0) - x * y + np.log1p(e)).sum() / (B * C)
            sig = np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
            sig = np.where(np.isnan(x), x, sig)
            dx = (sig - y) / (B * C)
            correct = y[np.arange(B), top]
    return loss, correct.sum(), correct, dx


def pooled_cls_loss(z, target, mode, kind):
    """per-frame logits z [B,T,C] -> dict(pooled, arg, loss, n_correct, correct, dpooled, dz)"""
    pooled, arg = tpool_fwd(z, mode)
    loss, n_correct, correct, dpooled = cls_loss(pooled, target, kind)
    return dict(pooled=pooled, arg=arg, loss=loss, n_correct=n_correct, correct=correct, dpooled=dpooled,
                dz=tpool_bwd(dpooled, arg, np.shape(z)[1], mode))
