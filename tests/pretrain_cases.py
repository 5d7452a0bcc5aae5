"""Seeded inputs of the operator tests of the pre-training loss end, shared by the host test (which checks on the CPU that every case
has a clear top-1 class) and the GPU test (which runs them).  Every value of B in {1, 3, 257}, T in {1, 2, 5} and C in
{1, 7, 63, 64, 65, 527, 1000, 1025} appears, and so do the pairs (T=1, C=527), (B=257, C=1000) and (B=1, C=1)."""
import numpy as np

SHAPES = [(1, 1, 1), (3, 2, 7), (3, 5, 63), (1, 5, 64), (3, 2, 65), (3, 1, 527), (257, 2, 1000), (3, 5, 1025), (257, 5, 7)]
MARGIN = 1e-3       # least float64 gap between the two largest per-clip logits of a row: the top-1 class cannot depend on fp32 rounding


def make_case(B, T, C, mode, kind):
    """float32 z [B,T,C] ~ 3 N(0,1) and the target of `kind` (0: int64 labels, about half of them the clip's own top-1 class so that
    `correct` is not all zeros; 1: float32 multi-hot targets with ~30 % ones)"""
    rs = np.random.RandomState(10007 * B + 101 * T + C + 7 * mode + 3 * kind)
    z = (rs.standard_normal((B, T, C)) * 3).astype(np.float32)
    if kind == 0:
        pooled = z.astype(np.float64).mean(axis=1) if mode else z.max(axis=1)
        own = rs.uniform(size=B) < 0.5
        target = np.where(own, pooled.argmax(axis=1), rs.randint(0, C, (B,))).astype(np.int64)
    else:
        target = (rs.uniform(size=(B, C)) < 0.3).astype(np.float32)
    return z, target


def top2_margin(pooled):
    """least gap between the largest and the second largest entry over the rows of pooled [B,C] (inf for C = 1)"""
    if pooled.shape[1] < 2:
        return np.inf
    s = np.sort(np.asarray(pooled, np.float64), axis=1)
    return float((s[:, -1] - s[:, -2]).min())
