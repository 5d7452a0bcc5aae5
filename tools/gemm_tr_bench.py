#!/usr/bin/env python3
"""The row-contiguous-operand GEMM shapes of a C3 step, one launch timed at a time (magnitude slots given: the tile kernel and its slab
reduce alone).  Prints `name median min max` in us per case; M3T_GEMM_TR / M3T_LIB_PATH select what runs, so two processes make an A/B.
usage: python tools/gemm_tr_bench.py [--reps N] [--only substring] [--digest]"""
import argparse
import hashlib
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))
import torch
from m3t import ops, _lib

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--only", default="")
ap.add_argument("--digest", action="store_true")
a = ap.parse_args()
dev = "cuda:0"
BESIDE, BACK = _lib.M3T_GEMM_BESIDE_SCAN, 1      # (M3T_GEMM_BACKGROUND, include/m3t_hip.h)
# (name, tA, tB, M, N, K, seg, use_ws, extra flags)
CASES = [
    ("NT 9600x1536x1024", 0, 1, 9600, 1536, 1024, None, True, 0),
    ("NN 9600x1024x1536", 0, 0, 9600, 1024, 1536, None, True, 0),
    ("NN 9600x2048x512", 0, 0, 9600, 2048, 512, None, True, 0),
    ("NN 9600x512x1024", 0, 0, 9600, 512, 1024, None, True, 0),
    ("TN 1536x1024x9600", 1, 0, 1536, 1024, 9600, None, True, 0),
    ("TN 1536x1024x9600 splits=1", 1, 0, 1536, 1024, 9600, None, False, 0),
    ("TN 1536x512x9568 seg", 1, 0, 1536, 512, 9568, (299, 300, 1, 0), True, 0),
    ("NN 9600x1024x1536 beside", 0, 0, 9600, 1024, 1536, None, True, BESIDE),
    ("TN 1536x1024x9600 beside", 1, 0, 1536, 1024, 9600, None, True, BESIDE),
    ("TN 1536x512x9568 seg beside", 1, 0, 1536, 512, 9568, (299, 300, 1, 0), True, BESIDE),
    ("TN 1536x1024x9600 background", 1, 0, 1536, 1024, 9600, None, True, BACK),
    ("TN 768x256x9568 seg", 1, 0, 768, 256, 9568, (299, 300, 1, 0), True, 0),
    ("TN 1536x256x9600", 1, 0, 1536, 256, 9600, None, True, 0),
]
torch.manual_seed(0)
for name, tA, tB, m, n, k, seg, use_ws, fl in CASES:
    if a.only and a.only not in name:
        continue
    if seg:
        A = torch.randn(9600, m, device=dev); Bm = torch.randn(9600, 2 * n, device=dev)
    else:
        A = torch.randn((k, m) if tA else (m, k), device=dev)
        Bm = torch.randn((n, k) if tB else (k, n), device=dev)
    Cm = torch.empty(m, n, device=dev)
    sl = ops.amax_slots(2, A.device)
    ops.measure_amax([(A, sl.data_ptr()), (Bm, sl.data_ptr() + 8)])
    kw = dict(use_ws=use_ws, prec=ops._PREC[0] | fl, amax=(sl.data_ptr(), sl.data_ptr() + 8))
    if seg:
        run = lambda: ops.sgemm(1, 0, m, n, k, A, 0, m, Bm, 0, 2 * n, Cm, 0, n, seg=seg, **kw)
    else:
        run = lambda: ops.sgemm(tA, tB, m, n, k, A, 0, A.shape[1], Bm, 0, Bm.shape[1], Cm, 0, n, **kw)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); run(); e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    ts.sort()
    dg = "  digest " + hashlib.sha256(Cm.cpu().numpy().tobytes()).hexdigest()[:12] if a.digest else ""
    print("%-30s %8.1f %8.1f %8.1f%s" % (name, ts[len(ts) // 2], ts[0], ts[-1], dg), flush=True)
