"""Child process of tests/test_gpu_gemm_tr.py: runs a fixed list of products with a row-contiguous operand under the M3T_GEMM_TR of its
environment and saves every result.   usage: python tests/gemm_tr_child.py gemm|conv FLAGS OUT.pt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p_ in (ROOT, os.path.join(ROOT, "m3f.pytorch_amd"), os.path.join(ROOT, "tests")):
    if p_ not in sys.path:
        sys.path.insert(0, p_)
import numpy as np
import torch
from m3t import ops, _lib

DEV = "cuda:0"
F16X3, X6 = _lib.M3T_GEMM_F16X3, 0

# (name, tA, tB, M, N, K, seg, use_ws, bias, act, accumulate, fill, prec)
#   128-column tiles need splits > 1 or more than 384 tiles; N % 128 == 64 or a small one-pass grid takes the 64-column tile
GEMM_CASES = [
    ("tn_128_split", 1, 0, 256, 256, 1536, None, True, False, 0, False, "normal", F16X3),
    ("tn_128_one", 1, 0, 2560, 2560, 64, None, False, False, 0, False, "normal", F16X3),
    ("tn_64_one", 1, 0, 256, 256, 1024, None, False, False, 0, False, "normal", F16X3),
    ("tn_64_split", 1, 0, 256, 192, 1536, None, True, False, 0, False, "normal", F16X3),
    ("tn_acc_split", 1, 0, 384, 256, 1536, None, True, False, 0, True, "normal", F16X3),
    ("tn_acc_one", 1, 0, 2560, 2560, 96, None, False, False, 0, True, "normal", F16X3),
    ("tn_range", 1, 0, 256, 256, 1536, None, True, False, 0, False, "range", F16X3),
    ("tn_zeros", 1, 0, 256, 256, 1024, None, False, False, 0, False, "zeros", F16X3),
    ("tn_nan", 1, 0, 256, 256, 1536, None, True, False, 0, False, "nan", F16X3),
    ("tn_inf", 1, 0, 256, 256, 1024, None, False, False, 0, False, "inf", F16X3),
    ("tt_128_split", 1, 1, 256, 256, 1536, None, True, False, 0, False, "normal", F16X3),
    ("seg_128_split", 1, 0, 256, 256, 1536, (96, 100, 1, 0), True, False, 0, False, "normal", F16X3),
    ("seg_128_one", 1, 0, 2560, 2560, 64, (32, 40, 2, 1), False, False, 0, False, "normal", F16X3),
    ("seg_64_one", 1, 0, 256, 128, 512, (64, 65, 1, 0), False, False, 0, False, "normal", F16X3),
    ("seg_ragged_504", 1, 0, 384, 128, 504, (63, 64, 1, 0), True, False, 0, False, "normal", F16X3),
    ("seg_ragged_504_acc", 1, 0, 384, 192, 504, (63, 64, 1, 0), False, False, 0, True, "range", F16X3),
    ("seg_dwhh", 1, 0, 1536, 512, 9568, (299, 300, 1, 0), True, False, 0, False, "normal", F16X3),
    ("nn_128_split", 0, 0, 256, 256, 1536, None, True, True, 1, False, "normal", F16X3),
    ("nn_128_one", 0, 0, 2560, 2560, 64, None, False, True, 1, False, "normal", F16X3),
    ("nn_64_one", 0, 0, 256, 192, 1024, None, False, True, 0, True, "normal", F16X3),
    ("nn_64_split", 0, 0, 256, 192, 1536, None, True, True, 1, True, "normal", F16X3),
    ("nn_range", 0, 0, 256, 512, 1536, None, True, False, 0, False, "range", F16X3),
    ("nn_nan_inf", 0, 0, 256, 256, 1024, None, False, True, 1, False, "naninf", F16X3),
    ("nn_step", 0, 0, 9600, 1024, 1536, None, True, False, 0, False, "normal", F16X3),
    ("tn_step", 1, 0, 1536, 1024, 9600, None, True, False, 0, False, "normal", F16X3),
    ("tn_x6", 1, 0, 256, 256, 1536, None, True, False, 0, False, "normal", X6),
    ("nn_x6", 0, 0, 256, 192, 1024, None, False, True, 1, False, "range", X6),
]


def fill(gen, shape, kind):
    t = torch.randn(shape, generator=gen, dtype=torch.float32)
    if kind in ("range",):      # magnitudes over 2^-30 .. 2^10
        e = torch.randint(-30, 11, shape, generator=gen).to(torch.float32)
        t = t * torch.exp2(e)
    if kind == "zeros":
        t[::3] = 0.0
        t[:, 5:70] = 0.0
    if kind in ("nan", "naninf"):
        t[3, 7] = float("nan")
    if kind in ("inf", "naninf"):
        t[5, 11] = float("-inf")
    return t


def run_gemm(flags, out):
    gen = torch.Generator().manual_seed(1234)
    res, plans = {}, {}
    for name, tA, tB, m, n, k, seg, use_ws, bias, act, acc, kind, prec in GEMM_CASES:
        if seg:
            rows = (k // seg[0] - 1) * seg[1] + seg[0] + max(seg[2], seg[3])
            A = fill(gen, (rows, m), kind).to(DEV); Bm = fill(gen, (rows, 2 * n), "normal").to(DEV)
        else:
            A = fill(gen, (k, m) if tA else (m, k), "normal" if tA == 0 else kind).to(DEV)
            Bm = fill(gen, (n, k) if tB else (k, n), kind if tA == 0 else "normal").to(DEV)
        bv = torch.randn(n, generator=gen).to(DEV) if bias else None
        Cm = torch.randn(m, n, generator=gen).to(DEV)
        ops.sgemm(tA, tB, m, n, k, A, 0, A.shape[1], Bm, 0, Bm.shape[1], Cm, 0, n, bias=bv, act=act, accumulate=acc,
                  seg=seg or (0, 0, 0, 0), use_ws=use_ws, prec=prec | flags)
        torch.cuda.synchronize()
        res[name] = Cm.cpu()
        plans[name] = ops.sgemm_plan(tA, m, n, k, seg[0] if seg else 0, prec=prec | flags, ws_bytes=ops._WS_MIN if use_ws else 0)[1]
    torch.save({"res": res, "splits": plans}, out)


def run_conv(out):
    """the convolutions' weight gradient (the C3 = 2 walk) through ops.conv3d_cl's backward: a 64-column and a 128-column grid"""
    from golden.recipe import draw
    res = {}
    for name, (Ci, Co, k, stride, pad, N, T, H, W) in (("stem_64", (64, 128, (3, 3, 3), (1, 1, 1), (1, 0, 0), 2, 4, 9, 9)),
                                                      ("stem_128", (64, 256, (3, 3, 3), (1, 1, 1), (1, 0, 0), 2, 8, 18, 18))):
        rs = np.random.RandomState(Ci + Co + H)
        xn, wn = draw(rs, (N * T * H * W, Ci)), draw(rs, (Co, Ci) + k) * 0.2
        x = torch.from_numpy(xn).to(DEV).requires_grad_(True)
        w = torch.from_numpy(wn).to(DEV).requires_grad_(True)
        y = ops.conv3d_cl(ops.CLTensor(x, N, T, H, W, None), w, None, stride, pad)
        ct = torch.from_numpy(draw(rs, tuple(y.data.shape))).to(DEV)
        (y.data * ct).sum().backward()
        ops.join_wgrad()
        torch.cuda.synchronize()
        res[name + "_dw"] = w.grad.cpu()
        res[name + "_dx"] = x.grad.cpu()
        res[name + "_y"] = y.data.detach().cpu()
    torch.save({"res": res, "splits": {}}, out)


if __name__ == "__main__":
    if sys.argv[1] == "gemm":
        run_gemm(int(sys.argv[2]), sys.argv[3])
    else:
        run_conv(sys.argv[3])
