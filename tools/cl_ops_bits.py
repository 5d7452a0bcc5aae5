#!/usr/bin/env python3
"""Run every entry point of csrc/stem_cl.hip, csrc/gn_cl.hip and csrc/vggface.hip once on seeded inputs and save every output as raw bits.

    python tools/cl_ops_bits.py OUT.npz

One process, one library (M3T_LIB_PATH picks another build), a few seconds.  Two libraries compute the same thing when every array of their
files is equal as a bit pattern: run this once per library in a fresh process each and compare the arrays (they are saved as uint32 / uint8
views: numpy.array_equal on floats would fail on the NaN inputs).  The kernels have no float atomics and the magnitude slot is an integer max, so
a second run of one library is equal to its first.

The operators go through m3t.ops as the models drive them (CLTensor, lazy norm + pool_cl, the armed magnitude slots, the dx hand-over with its
column sums); what ops does not expose -- a backward without dx_colsum -- goes through ops.lib().  Saved: y / yp / s / z, what each forward
keeps for its backward (winner bytes, saved mean / inv-std), the running statistics after the step, dx / ds, dgamma, dbeta, the column sums
and the slot words.

Shapes: the smallest at which these kernels can go wrong, not the workload's.  Rows operators at 2 clips x 3 x 7 x 9 (R = 189 rows a clip:
two BatchNorm chunks that end ragged, two blocks in the map pass, two clips on GroupNorm's grid) with C = 64, G = 32 (a quad straddles two
groups), the same rows at C = 4 (C / 4 = 1: 256 row groups) and 6 rows at C = 1024 (one row group, four turns of the per-channel loops); C = 96
for the two VGGFace rows operators (C / 4 = 24 does not divide 256).  Pooling on 6 frames of 7 x 9 x 64: k = 2 (both edges odd), k = 3 (a row
left over), the plain pooling with and without padding, the ReLU pooling with ceil_mode on and off.  Every input also as a second copy with
an exact tie inside a window, one NaN and one +inf."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))

DEV = "cuda:0"
OUT = {}
HAND = []          # (dx, slot, column sums) of every dx hand-over since the last take


def keep(name, t):
    if t is None:
        return
    assert name not in OUT, name
    a = t.detach().contiguous().cpu().numpy()
    OUT[name] = a if a.dtype == np.uint8 else a.view(np.uint32)


def rnd(*shape):
    return 0.7 * torch.randn(*shape, device=DEV) + 3.0 if len(shape) == 2 else torch.randn(*shape, device=DEV)


def spiked(x, W, C):
    """a copy of rows [.., C] on a grid W wide: positions (0, 0) and (0, 1) of the first frame tie exactly in channel 1, a NaN and a +inf"""
    x, rows = x.clone(), x.shape[0]
    x[1, 1] = x[0, 1] = 7.25
    x[(W + 2) % rows, 3 % C] = float("nan")
    x[(2 * W + 5) % rows, 2 % C] = float("inf")
    return x


def affine(C):
    return (torch.randn(C, device=DEV).requires_grad_(True), torch.randn(C, device=DEV).requires_grad_(True),
            0.1 * torch.randn(C, device=DEV), 1.0 + 0.1 * torch.rand(C, device=DEV))


def finish(tag, outs, leaves, douts):
    """save the outputs, what the forward kept, then backward from `douts` and save every gradient and hand-over"""
    for i, o in enumerate(outs):
        keep("%s.out%d" % (tag, i), o.data if o is not None else None)
        keep("%s.out%d.slot" % (tag, i), o.slot if o is not None else None)
    fn = next(o.data.grad_fn for o in outs if o is not None and o.data.grad_fn is not None)
    for i, t in enumerate(fn.saved_tensors):
        keep("%s.saved%d" % (tag, i), t)
    del HAND[:]
    torch.autograd.backward([o.data for o, d in zip(outs, douts) if d is not None], [d for d in douts if d is not None])
    for name, t in leaves.items():
        keep("%s.grad_%s" % (tag, name), t.grad)
        t.grad = None
    for i, (dx, slot, csum) in enumerate(HAND):
        keep("%s.hand%d.dx" % (tag, i), dx)
        keep("%s.hand%d.slot" % (tag, i), slot)
        keep("%s.hand%d.colsum" % (tag, i), csum)


def rows_ops(ops, tag, N, T, H, W, C, G):
    M = N * T * H * W
    base = rnd(M, C)
    for kind, x0 in (("plain", base), ("spiked", spiked(base, W, C))):
        for training in (True, False):
            for relu in (True, False):
                t = "%s.%s.%s.relu%d" % (tag, kind, "train" if training else "eval", relu)
                x = x0.clone().requires_grad_(True)
                gamma, beta, rm, rv = affine(C)
                y = ops.bn_cl(ops.CLTensor(x, N, T, H, W), gamma, beta, rm, rv, training, 0.1, 1e-5, relu)
                finish(t + ".bn_cl", [y], {"x": x, "gamma": gamma, "beta": beta}, [rnd(M, C)])
                keep(t + ".bn_cl.run_mean", rm)
                keep(t + ".bn_cl.run_var", rv)
            t = "%s.%s.%s" % (tag, kind, "train" if training else "eval")
            x, sc = x0.clone().requires_grad_(True), rnd(M, C).requires_grad_(True)
            gamma, beta, rm, rv = affine(C)
            y = ops.bn_add_relu_cl(ops.CLTensor(x, N, T, H, W), ops.CLTensor(sc, N, T, H, W), gamma, beta, rm, rv, training, 0.1, 1e-5)
            finish(t + ".bn_add_relu_cl", [y], {"x": x, "shortcut": sc, "gamma": gamma, "beta": beta}, [rnd(M, C)])
            keep(t + ".bn_add_relu_cl.run_mean", rm)
            keep(t + ".bn_add_relu_cl.run_var", rv)
            for ds_out in (True, False):
                a, b = x0.clone().requires_grad_(True), rnd(M, C).requires_grad_(True)
                gamma, beta, rm, rv = affine(C)
                s, z = ops.add_bn_relu_cl(ops.CLTensor(a, N, T, H, W), ops.CLTensor(b, N, T, H, W), gamma, beta, rm, rv, training, 0.1, 1e-5)
                finish("%s.add_bn_relu_cl.ds_out%d" % (t, ds_out), [s, z], {"a": a, "b": b, "gamma": gamma, "beta": beta},
                       [rnd(M, C) if ds_out else None, rnd(M, C)])
                keep("%s.add_bn_relu_cl.ds_out%d.run_mean" % (t, ds_out), rm)
                keep("%s.add_bn_relu_cl.ds_out%d.run_var" % (t, ds_out), rv)
        with torch.no_grad():      # eval with the sum not written
            gamma, beta, rm, rv = affine(C)
            s, z = ops.add_bn_relu_cl(ops.CLTensor(x0, N, T, H, W), ops.CLTensor(rnd(M, C), N, T, H, W), gamma, beta, rm, rv, False, 0.1, 1e-5,
                                      need_s=False)
            assert s is None
            keep("%s.%s.add_bn_relu_cl.no_s.z" % (tag, kind), z.data)
            keep("%s.%s.add_bn_relu_cl.no_s.slot" % (tag, kind), z.slot)
        if C % G == 0:
            for relu in (True, False):
                t = "%s.%s.gn_cl.relu%d" % (tag, kind, relu)
                x = x0.clone().requires_grad_(True)
                gamma, beta, _, _ = affine(C)
                y = ops.gn_cl(ops.CLTensor(x, N, T, H, W), G, gamma, beta, 1e-5, relu)
                finish(t, [y], {"x": x, "gamma": gamma, "beta": beta}, [rnd(M, C)])
        relu_rows(ops, "%s.%s" % (tag, kind), x0, N, T, H, W)
        no_colsum(ops, "%s.%s" % (tag, kind), x0, N, T * H * W, C, G)


def relu_rows(ops, tag, x0, N, T, H, W):
    x = x0.clone().requires_grad_(True)
    y = ops.relu_cl(ops.CLTensor(x, N, T, H, W))
    finish(tag + ".relu_cl", [y], {"x": x}, [rnd(*x0.shape)])
    mean = ops.mean_cl(ops.CLTensor(x, N, T, H, W))
    keep(tag + ".mean_cl.y", mean)
    mean.backward(torch.randn_like(mean))
    keep(tag + ".mean_cl.dx", x.grad)


def no_colsum(ops, tag, x0, N, R, C, G):
    """the backward entry points without dx_colsum (ops always asks for it): through the library, slot armed"""
    lib, p, M = ops.lib(), ops._p, N * R
    dy, y = rnd(M, C), torch.relu(x0)
    gamma = torch.randn(C, device=DEV)
    stat = torch.stack([x0.mean(0), 1.0 / torch.sqrt(x0.var(0, unbiased=False) + 1e-5)]).contiguous()
    stat = torch.nan_to_num(stat, nan=0.5, posinf=0.5)
    ws = ops.workspace(torch.device(DEV), max(int(lib.m3t_bn_cl_ws_bytes(M, C)), int(lib.m3t_gn_cl_ws_bytes(N, R, C)), 8))
    dx, ds = torch.empty(M, C, device=DEV), torch.empty(M, C, device=DEV)
    dgb = torch.empty(2, C, device=DEV)
    calls = [("bn_cl", "m3t_bn_cl_bwd", (p(dy), p(x0), p(y), p(gamma), p(stat[0]), p(stat[1]), M, C, 1, 1, p(dx), p(dgb[0]), p(dgb[1]), None)),
             ("bn_add_relu_cl", "m3t_bn_add_relu_cl_bwd", (p(dy), p(x0), p(y), p(gamma), p(stat[0]), p(stat[1]), M, C, 1, p(dx), p(ds), p(dgb[0]),
                                                          p(dgb[1]), None)),
             ("add_bn_relu_cl", "m3t_add_bn_relu_cl_bwd", (p(dy), None, p(x0), p(y), p(gamma), p(stat[0]), p(stat[1]), M, C, 1, p(dx), p(dgb[0]),
                                                          p(dgb[1]), None)),
             ("relu_cl", "m3t_relu_cl_bwd", (p(dy), p(y), M, C, p(dx), None))]
    if C % G == 0:
        gst = torch.stack([torch.full((N * G,), 3.0, device=DEV), torch.full((N * G,), 1.4, device=DEV)]).contiguous()
        calls.append(("gn_cl", "m3t_gn_cl_bwd", (p(dy), p(x0), p(y), p(gamma), p(gst[0]), p(gst[1]), N, R, C, G, 1, p(dx), p(dgb[0]), p(dgb[1]), None)))
    for name, entry, args in calls:
        slot = ops.amax_slots(1, torch.device(DEV))
        dx.zero_(); ds.zero_(); dgb.zero_()
        ops._armed_call(p(slot), entry, *args, p(ws), ws.numel() * 4, ops._stream())
        t = "%s.%s.no_colsum" % (tag, name)
        keep(t + ".dx", dx)
        keep(t + ".ds", ds)
        keep(t + ".dgb", dgb)
        keep(t + ".slot", slot)


def pool_no_colsum(ops, tag, entry, y, dyp, geo):
    """a fused pooling's backward without dx_colsum, on what its forward kept: through the library, slot armed"""
    lib, p = ops.lib(), ops._p
    saved = y.data.grad_fn.saved_tensors
    win = next(t for t in saved if t.dtype == torch.uint8)
    slot = ops.amax_slots(1, torch.device(DEV))
    ws = ops.workspace(torch.device(DEV), 1 << 22)
    if entry == "m3t_relu_pool_cl_bwd":
        P, H, W, C, ceil_mode = geo
        dx = torch.zeros(P * H * W, C, device=DEV)
        ops._armed_call(p(slot), entry, p(dyp), p(saved[0]), win.data_ptr(), P, H, W, C, ceil_mode, p(dx), None, p(ws), ws.numel() * 4, ops._stream())
    else:
        x, yp, _, gamma, stats = saved
        dx, dgb = torch.zeros_like(x), torch.zeros(2, x.shape[1], device=DEV)
        ops._armed_call(p(slot), entry, p(dyp), p(x), p(yp), win.data_ptr(), p(gamma), p(stats[0]), p(stats[1]), *geo, p(dx), p(dgb[0]), p(dgb[1]), None,
                        p(ws), ws.numel() * 4, ops._stream())
        keep(tag + ".no_colsum.dgb", dgb)
    keep(tag + ".no_colsum.dx", dx)
    keep(tag + ".no_colsum.slot", slot)


def pool_ops(ops, N, T, H, W, C, G):
    P = N * T
    base = rnd(P * H * W, C)
    for kind, x0 in (("plain", base), ("spiked", spiked(base, W, C))):
        for k in (2, 3):
            Mp = P * (H // k) * (W // k)
            for training in (True, False):
                t = "pool.%s.bn_pool_cl.k%d.%s" % (kind, k, "train" if training else "eval")
                x = x0.clone().requires_grad_(True)
                gamma, beta, rm, rv = affine(C)
                y = ops.pool_cl(ops.bn_cl(ops.CLTensor(x, N, T, H, W), gamma, beta, rm, rv, training, 0.1, 1e-5, True, lazy=True), (k, k), (k, k), (0, 0))
                assert y.data.shape[0] == Mp and type(y.data.grad_fn).__name__.startswith("_BNPoolCL")
                if training:
                    pool_no_colsum(ops, t, "m3t_bn_pool_cl_bwd", y, rnd(Mp, C), (P, H, W, C, k, 1))
                finish(t, [y], {"x": x, "gamma": gamma, "beta": beta}, [rnd(Mp, C)])
                keep(t + ".run_mean", rm)
                keep(t + ".run_var", rv)
            t = "pool.%s.gn_pool_cl.k%d" % (kind, k)
            x = x0.clone().requires_grad_(True)
            gamma, beta, _, _ = affine(C)
            y = ops.pool_cl(ops.gn_cl(ops.CLTensor(x, N, T, H, W), G, gamma, beta, 1e-5, True, lazy=True), (k, k), (k, k), (0, 0))
            assert type(y.data.grad_fn).__name__.startswith("_GNPoolCL")
            pool_no_colsum(ops, t, "m3t_gn_pool_cl_bwd", y, rnd(Mp, C), (N, T, H, W, C, G, k))
            finish(t, [y], {"x": x, "gamma": gamma, "beta": beta}, [rnd(Mp, C)])
        for k, s, p in (((3, 3), (2, 2), (1, 1)), ((2, 2), (2, 2), (0, 0))):
            x = x0.clone().requires_grad_(True)
            y = ops.pool_cl(ops.CLTensor(x, N, T, H, W), k, s, p)
            finish("pool.%s.pool_cl.k%d.p%d" % (kind, k[0], p[0]), [y], {"x": x}, [rnd(y.data.shape[0], C)])
        for ceil_mode in (True, False):
            x = x0.clone().requires_grad_(True)
            y = ops.relu_pool_cl(ops.CLTensor(x, N, T, H, W), ceil_mode)
            pool_no_colsum(ops, "pool.%s.relu_pool_cl.ceil%d" % (kind, ceil_mode), "m3t_relu_pool_cl_bwd", y, rnd(y.data.shape[0], C),
                           (P, H, W, C, int(ceil_mode)))
            finish("pool.%s.relu_pool_cl.ceil%d" % (kind, ceil_mode), [y], {"x": x}, [rnd(y.data.shape[0], C)])


def main():
    if len(sys.argv) != 2:
        print(__doc__)
        return 2
    from m3t import ops
    torch.manual_seed(1234)
    handover = ops._dx_handover

    def recording(dx):
        slot, csum = handover(dx)
        HAND.append((dx, slot, csum))
        return slot, csum

    ops._dx_handover = recording
    rows_ops(ops, "rows64", 2, 3, 7, 9, 64, 32)
    rows_ops(ops, "rows4", 2, 3, 7, 9, 4, 2)
    rows_ops(ops, "rows1024", 1, 1, 2, 3, 1024, 32)
    x96 = rnd(378, 96)
    for kind, x0 in (("plain", x96), ("spiked", spiked(x96, 9, 96))):
        relu_rows(ops, "rows96." + kind, x0, 2, 3, 7, 9)
    pool_ops(ops, 2, 3, 7, 9, 64, 32)
    torch.cuda.synchronize()
    np.savez(sys.argv[1], **OUT)
    print("cl_ops_bits: %d arrays -> %s" % (len(OUT), sys.argv[1]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
