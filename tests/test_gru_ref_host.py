"""CPU checks of tests/gru_ref.py, the yardsticks tests/test_gpu_gru_fp64.py holds the GRU scans to: the float64 oracle against
torch's float64 nn.GRU, the fp32 restatement of the kernels' arithmetic against the reference, and whether the comparison helper
notices six planted errors -- next to what the old `close()` bars of tests/test_gpu_parity.py make of the same six.  Run with -s
for the figures (NOTEBOOK.md R11)."""
import numpy as np
import pytest

import gru_ref as R

SENSITIVITY_CASES = tuple(c for c in R.CASES if c.stats == "normal" and (c.B, c.T, c.H, c.L, c.switch, c.prec) in (
    (33, 5, 256, 2, "", "f16x3"), (5, 2, 256, 1, "", "f16x3"), (21, 11, 128, 2, "", "f16x3"), (2, 50, 256, 1, "", "f16x3"),
    (33, 5, 256, 2, "", "x6")))


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if R._data_key(c) not in seen:
            seen.add(R._data_key(c))
            out.append(c)
    return out


def test_the_case_table_has_every_family_and_no_filter():
    assert len(SENSITIVITY_CASES) == 5
    assert {R.scan_model(c) for c in R.CASES} == {"fp32", "f16x3", "x6"}
    assert {c.stats for c in R.CASES} == {"normal", "saturated", "small", "one_hot_time"}
    assert not hasattr(R, "admitted")
    assert len({R.case_id(c) + c.switch for c in R.CASES}) == len(R.CASES)
    for c in R.CASES:                                                  # what the families stand on
        if c.family.startswith("persistent split") or c.family == "long chain":
            assert R.scan_model(c) == c.prec and not R.rows32(c), c
        else:
            assert R.scan_model(c) == "fp32", c
    assert [c for c in R.CASES if R.rows32(c)] == [c for c in R.CASES if "32 rows" in c.family]
    assert {c.T for c in R.CASES if c.stats == "one_hot_time"} == {23, 50}


def test_oracle_equals_float64_torch_gru():
    """oracle.m3t_oracle.bigru_fwd / bigru_bwd against torch.nn.GRU in float64, to 1e-13 of each tensor's own maximum: every case with
    H <= 256 and one at H = 512"""
    cases = _unique([c for c in R.CASES if c.H <= 256] + [c for c in R.CASES if (c.B, c.T, c.H) == (19, 23, 512)][:1])
    assert any(c.H == 512 for c in cases) and len(cases) >= 20
    worst = 0.0
    for c in cases:
        d = R.data(c)
        t64 = R.torch_gru(d["p"], d["x"], d["ct"], d["cth"], c.L, dtype=R.torch.float64)
        for n in R.tensor_names(c.L):
            e = R.rel_err(t64[n], d["ref"][n])
            worst = max(worst, e)
            assert e <= 1e-13, (R.case_id(c), n, e)
    print("\noracle vs float64 nn.GRU: worst %.2g of a tensor's maximum over %d cases" % (worst, len(cases)))


def test_emulation_stays_at_fp32_rounding_on_normal_statistics():
    """yardstick B within BOUND max(E32, 2^-24) of the reference on the normal-statistics cases of all three product models; the figures
    of every case and class are printed"""
    models = set()
    print()
    for c in R.CASES:
        d, (_, e_emu) = R.data(c), R.emulated(c)
        names = R.tensor_names(c.L)
        ratio = {n: e_emu[n] / max(d["e32"][n], R.FLOOR) for n in names}
        wn = max(names, key=lambda n: ratio[n])
        print("%-72s %-5s E32 %.1e .. %.1e  E_emu %.1e .. %.1e  worst E_emu / E32 %7.2f  %s" % (
            R.case_id(c), R.scan_model(c), min(d["e32"].values()), max(d["e32"].values()), min(e_emu.values()), max(e_emu.values()),
            ratio[wn], wn))
        if c.stats == "normal":
            models.add(R.scan_model(c))
            assert ratio[wn] <= R.BOUND, (R.case_id(c), wn, ratio[wn])
    assert models == {"fp32", "f16x3", "x6"}


def test_the_small_class_shows_the_stated_limit_of_fast_tanh_and_nothing_else():
    """inputs and biases x 1e-3: the absolute error of the subtractive tanh form reaches y, h_n and the weight gradients that read a
    hidden state (E_emu > BOUND E32 there, by two orders), stays under the bound derived from it, and leaves dx, the bias gradients
    and the first layer's dW_ih at fp32 rounding"""
    small = [c for c in R.CASES if c.stats == "small"]
    assert len(small) >= 8
    print()
    for c in small:
        d, (_, e_emu), lim = R.data(c), R.emulated(c), R.limits(c)
        reached = [n for n in R.tensor_names(c.L) if lim[n][1] is not None]
        assert {"y", "h_n", "gru.weight_hh_l0", "gru.weight_hh_l0_reverse"} <= set(reached), (R.case_id(c), reached)
        for n in R.tensor_names(c.L):
            hi, lo = lim[n]
            assert e_emu[n] <= hi, (R.case_id(c), n, e_emu[n], hi)
            if lo is not None:
                assert e_emu[n] > 10 * lo, (R.case_id(c), n, e_emu[n], lo)       # far over, not marginally: the GPU test asserts > lo
            else:
                assert "bias" in n or n == "dx" or "weight_ih_l0" in n, (R.case_id(c), n)
        print("%-72s limit %.1e reaches %d tensors: E_emu %.1e .. %.1e = %3.0f .. %3.0f x E32" % (
            R.case_id(c), R.BOUND * R.TANH_ABS / d["scale"], len(reached), min(e_emu[n] for n in reached), max(e_emu[n] for n in reached),
            min(e_emu[n] / max(d["e32"][n], R.FLOOR) for n in reached), max(e_emu[n] / max(d["e32"][n], R.FLOOR) for n in reached)))


def _old_bars_pass(got, ref, L):
    """close() of tests/test_gpu_parity.py: err <= tol max(1, max |ref|), tol 1e-4 (y, h_n, dx), 2e-4 (parameter gradients)"""
    for n in R.tensor_names(L):
        tol = 1e-4 if n in ("y", "h_n", "dx") else 2e-4
        if float(np.abs(np.asarray(got[n], np.float64) - ref[n]).max()) > tol * max(1.0, float(np.abs(ref[n]).max())):
            return False
    return True


@pytest.mark.parametrize("plant", R.PLANTS[1:])
def test_the_helper_flags_a_planted_error_on_every_case(plant):
    print()
    old = []
    for c in SENSITIVITY_CASES:
        if plant == "a" and R.scan_model(c) != "f16x3":
            continue                                                   # (there is no fp16 term to drop in the other families)
        d = R.data(c)
        got = R.emulate(c, d["p"], d["x"], d["ct"], d["cth"], plant=plant)
        ratio, name, fails = R.check(got, c, quiet=True)
        passes_old = _old_bars_pass(got, d["ref"], c.L)
        old.append(passes_old)
        print("(%s) %-62s on %-58s %10.1f x  %-26s old bars: %s" % (plant, R.PLANT_TEXT[plant], R.case_id(c), ratio, name,
                                                                     "PASS" if passes_old else "fail"))
        assert ratio > R.BOUND and fails, (plant, R.case_id(c), ratio, name)
    assert old
    print("(%s) the old close() bars accept it on %d of %d cases" % (plant, sum(old), len(old)))


def test_the_clean_emulation_passes_its_own_check():
    for c in SENSITIVITY_CASES:
        ratio, name, fails = R.check(R.emulated(c)[0], c, quiet=True)
        assert ratio <= R.BOUND and not fails, (R.case_id(c), ratio, name, fails)
