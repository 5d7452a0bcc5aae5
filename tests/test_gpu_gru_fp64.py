"""The bidirectional GRU scans against float64, family by family, at an fp32-rounding bar (tests/gru_ref.py: reference, yardsticks,
bound; tests/test_gru_ref_host.py checks those on the CPU).  Every (B, T, H, L) is one tests/test_gpu_parity.py already runs under the
same switches.  Each case asserts the kernel family it reached, synchronises, polls the scan error word, and compares 3 + 8 L tensors:
rel_err <= BOUND max(E32, E_emu, 2^-24) per tensor; on the `small` class the tensors the absolute error of fast_tanh reaches are held
to the bound derived from it and must exceed the fp32 bar (csrc/gru_common.h, NOTEBOOK.md R11).  Run with -s for one line per case."""
import pytest
import torch

import gru_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _run(c, m, d, switch, prec):
    """one forward + backward under the switches -> (the 3 + 8 L tensors as float64 numpy, one-launch scans counted)"""
    from m3t import ops, _lib
    lib = _lib.load()
    keep = (ops.SCAN_PER_STEP[0], ops.SCAN_FP32[0], ops.FORCE_WIDE_FWD[0], ops._PREC[0])
    try:
        ops.SCAN_PER_STEP[0], ops.SCAN_FP32[0], ops.FORCE_WIDE_FWD[0] = switch == "per_step", switch == "fp32", switch == "wide"
        m.zero_grad()
        x = torch.from_numpy(d["x"]).to(DEV).requires_grad_(True)
        n0 = lib.m3t_gru_persist_count()
        with ops.precision("x6" if prec == "x6" else "fp32"):          # ("fp32" is the default mode: fp16x3 products)
            y, h = m(x)
            ((y * torch.from_numpy(d["ct"]).to(DEV)).sum() + (h * torch.from_numpy(d["cth"]).to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        ops.poll_scan_error()
        launches = lib.m3t_gru_persist_count() - n0
        got = {"y": y, "h_n": h, "dx": x.grad}
        got.update({n: p.grad for n, p in m.named_parameters()})
        return {n: t.detach().double().cpu().numpy() for n, t in got.items()}, launches
    finally:
        ops.SCAN_PER_STEP[0], ops.SCAN_FP32[0], ops.FORCE_WIDE_FWD[0], ops._PREC[0] = keep


@pytest.mark.parametrize("c", R.CASES, ids=[R.case_id(c) + ("-" + c.switch if c.switch else "") for c in R.CASES])
def test_gru_scans_against_float64(c):
    from models.rnn import GRU
    from m3t import _lib
    lib = _lib.load()
    d = R.data(c)
    m = GRU(c.I, c.H, c.L, -1, return_h=True).to(DEV)
    with torch.no_grad():
        for n, t in m.named_parameters():
            t.copy_(torch.from_numpy(d["p"][n]))
    assert sorted(n for n, _ in m.named_parameters()) == sorted(d["p"])
    got, launches = _run(c, m, d, c.switch, c.prec)

    # ---- the family the case reached
    B, T, H, L = c.B, c.T, c.H, c.L
    f16 = _lib.M3T_GEMM_F16X3 if c.prec == "f16x3" else 0
    wg16, wg32 = 2 * ((B + 15) // 16) * (H // 16), 2 * ((B + 31) // 32) * (H // 16)
    model = R.scan_model(c)
    if "per-step" in c.family:
        assert launches == 0 and model == "fp32", launches
        assert (H % 16 != 0) == c.family.startswith("generic")
    elif c.family == "solo":
        assert launches == 2 * L and H == 128 and model == "fp32", launches
        assert lib.m3t_gru_scan_workgroups(2, H, B, T, f16, 0) == 0                       # no grid of exchanging workgroups: one per clip
    elif c.family.startswith("persistent fp32"):
        assert launches == 2 * L and model == "fp32", launches
        flags = f16 | (_lib.M3T_SCAN_FP32 if c.switch == "fp32" else 0)
        if "32 rows" in c.family:
            assert wg16 > R.CUS and lib.m3t_gru_scan_workgroups(2, H, B, T, flags, 0) == wg32 != wg16
        else:
            assert lib.m3t_gru_scan_workgroups(2, H, B, T, flags, 0) == wg16
        if c.switch == "fp32":                                                           # the default is the other arithmetic
            other, n_other = _run(c, m, d, "", c.prec)
            assert n_other == 2 * L and not (other["y"] == got["y"]).all()
    else:
        assert launches == 2 * L and model == c.prec and H in (256, 512), launches
        wide = _lib.M3T_SCAN_WIDE if c.switch == "wide" else 0
        assert lib.m3t_gru_scan_workgroups(2, H, B, T, f16 | wide, 0) == (wg16 // 2 if wide else wg16)
        assert lib.m3t_gru_scan_workgroups(2, H, B, T, f16 | _lib.M3T_SCAN_WIDE, 1) == (wg16 // 2 if f16 else wg16)      # backward: every level asks for the wide form
        other, n_other = _run(c, m, d, "fp32", c.prec)                                    # it is not the fp32-MFMA arithmetic ...
        assert n_other == 2 * L and not (other["y"] == got["y"]).all() and not (other["dx"] == got["dx"]).all()
        if c.prec == "x6":                                                               # ... and six bf16 products are not three fp16 products
            other, _ = _run(c, m, d, c.switch, "f16x3")
            assert not (other["y"] == got["y"]).all() and not (other["dx"] == got["dx"]).all()

    ratio, name, fails = R.check(got, c)
    assert not fails, "%s [%s]: %s" % (R.case_id(c), c.family, "; ".join(fails))
    assert ratio <= R.BOUND
