"""tests/tcn_ref.py checked on the CPU: the float64 reference against torch's float64 autograd of the literal composition (and the general
tap rule against the oracle's causal / same-padding convolutions), the three product models against the reference, the admission of every
block-level case by draw_clear, the coverage of the case table, and the sensitivity of the new bar to six planted errors next to what
close() of tests/test_gpu_parity.py makes of them.  Run with -s for the figures."""
import numpy as np
import pytest
import torch

import tcn_ref as R
from oracle import m3t_oracle as O

TIGHT = 1e-13


def _uniq(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


def test_tap_rule_against_the_oracle():
    rs = np.random.RandomState(1)
    for B, T, Ci, Co, K, dil in ((2, 9, 3, 5, 3, 2), (2, 5, 4, 6, 3, 8), (3, 7, 5, 4, 5, 1)):
        x, w, dy = rs.standard_normal((B, T, Ci)), rs.standard_normal((Co, Ci, K)), rs.standard_normal((B, T, Co))
        w_t = np.ascontiguousarray(w.transpose(2, 0, 1))
        y = R.conv_taps(x, w_t, K, dil)
        assert np.abs(y - R._cf(O.causal_conv1d_fwd(R._cf(x), w, None, dil))).max() <= TIGHT * np.abs(y).max()
        dx, dw, _ = O.causal_conv1d_bwd(R._cf(dy), R._cf(x), w, dil)
        got_dx = R.conv_taps(dy, w_t, K, dil, 0, True)                     # the forward layout [K][Co][Ci] IS the time-flipped form's [K][Ci'][Co']
        assert np.abs(got_dx - R._cf(dx)).max() <= TIGHT * np.abs(dx).max()
        got_dw = R.wgrad_ref(dy, x, K, dil)
        assert np.abs(got_dw - dw.transpose(2, 0, 1)).max() <= TIGHT * np.abs(dw).max()
        for j in range(K):
            assert ((K - 1 - j) * dil >= T) == (not got_dw[j].any())
        if dil == 1 and K % 2 == 1:
            pad = (K - 1) // 2
            y = R.conv_taps(x, w_t, K, 1, pad)
            assert np.abs(y - R._cf(O.conv1d_same_fwd(R._cf(x), w, None, pad))).max() <= TIGHT * np.abs(y).max()
            dx, dw, _ = O.conv1d_same_bwd(R._cf(dy), R._cf(x), w, pad)
            assert np.abs(R.conv_taps(dy, w_t, K, 1, pad, True) - R._cf(dx)).max() <= TIGHT * np.abs(dx).max()
            assert np.abs(R.wgrad_ref(dy, x, K, 1, pad) - dw.transpose(2, 0, 1)).max() <= TIGHT * np.abs(dw).max()


def test_reference_against_torch_float64():
    worst = 0.0
    for c in _uniq(R.OPS, R._op_key):
        x, w_t, bias, res, _, mk = R.op_operands(c)
        yard, ref = R._torch_op(c, x, w_t, bias, res, mk, torch.float64), R.op_data(c)["ref"]
        for n in ref:
            e = R.rel_err(yard[n], ref[n])
            worst = max(worst, e)
            assert e <= TIGHT, (R.case_id(c), n, e)
    for c in _uniq(R.WGS, lambda c: c[:8]):
        d = R.wg_data(c)
        B, T, Ci, Co, K, dil = c.B, c.T, c.Ci, c.Co, c.K, c.dil
        w = torch.zeros(Co, Ci, K, dtype=torch.float64, requires_grad=True)
        out = torch.nn.functional.conv1d(torch.nn.functional.pad(torch.from_numpy(d["x"]).double().permute(0, 2, 1), ((K - 1) * dil - c.lead, c.lead)),
                                         w, None, dilation=dil)
        g, = torch.autograd.grad(out, w, torch.from_numpy(d["dy"]).double().permute(0, 2, 1))
        e = R.rel_err(g.permute(2, 0, 1).numpy(), d["ref"])
        worst = max(worst, e)
        assert e <= TIGHT, (R.case_id(c), e)
    for c in _uniq(R.BLOCKS, R._blk_key):
        d = R.data(c)
        yard = R.torch_net(c, d["p"], d["x"], d["ct"], d["masks"], torch.float64)
        for n in R.tensor_names(c) + R.inner_names(c):
            if n in d["zero"]:
                assert not yard[n].any(), (c.id, n)
                continue
            e = R.rel_err(yard[n].reshape(d["ref"][n].shape), d["ref"][n])
            worst = max(worst, e)
            assert e <= TIGHT, (c.id, n, e)
    print("reference vs float64 torch: worst rel_err %.3g" % worst)


def test_emulation_within_the_bound_of_the_reference():
    """yardstick B is an fp32 computation: on normal statistics all three product models sit within BOUND max(E32, 2^-24) of float64"""
    worst = {}
    for c in R.OPS:
        d, e = R.op_data(c), R.op_emulated(c)
        m = c.prec if c.kernel == "conv" else "fp32"
        for n in e:
            r = e[n] / max(d["e32"][n], R.FLOOR)
            worst[m] = max(worst.get(m, (0, "")), (r, R.case_id(c) + ":" + n))
            assert r <= R.BOUND, (R.case_id(c), n, e[n], d["e32"][n])
    for c in R.WGS:
        d, emu = R.wg_data(c), R.wg_emulated(c)
        for j in range(c.K):
            if d["ref"][j].any():
                r = R.rel_err(emu[j], d["ref"][j]) / max(R.rel_err(d["yard"][j], d["ref"][j]), R.FLOOR)
                m = "wgrad " + R.wgrad_route(c.B, c.T, c.Ci, c.Co, c.K, c.dil, c.lead, c.prec, j)[0]
                worst[m] = max(worst.get(m, (0, "")), (r, R.case_id(c) + ":tap%d" % j))
                assert r <= R.BOUND, (R.case_id(c), j, r)
            else:
                assert not emu[j].any()
    for c in R.BLOCKS:
        if c.stats != "normal":
            continue
        d, (_, e) = R.data(c), R.emulated(c)
        for n in e:
            r = e[n] / max(d["e32"][n], R.FLOOR)
            worst["blocks " + c.prec] = max(worst.get("blocks " + c.prec, (0, "")), (r, c.id + ":" + n))
            assert r <= R.BOUND, (c.id, n, e[n], d["e32"][n])
    for m, (r, where) in sorted(worst.items()):
        print("emulation %-14s worst E_emu / max(E32, 2^-24) = %5.2f  (%s)" % (m, r, where))


def test_every_block_case_is_admitted_and_the_table_covers_what_it_names():
    for c in R.BLOCKS:
        d = R.data(c)
        assert R.is_clear(d["clear"]) and d["seed"] < 8, (c.id, d["clear"])
        assert len(d["clear"]) == 3 * len(c.widths)
        for name, n_in, pos in d["clear"]:
            assert n_in == 0 and 0.25 <= pos <= 0.75, (c.id, name, n_in, pos)
        print("%-5s admitted at seed %d; positive fractions %.2f .. %.2f" % (c.id, d["seed"], min(p for _, _, p in d["clear"]),
                                                                         max(p for _, _, p in d["clear"])))
    # every kernel with every form, both precisions on the interior kernel, lead and the time-flipped form together
    for kern, prec in (("fp32", "f16x3"), ("conv", "f16x3"), ("conv", "x6")):
        assert {c.form for c in R.OPS if c.kernel == kern and c.prec == prec} == set(R.FORMS), (kern, prec)
        assert any(c.lead > 0 and c.form == "anti" for c in R.OPS if c.kernel == kern and c.prec == prec)
    for c in R.OPS:
        assert (c.kernel == "conv") == R.interior(c.B, c.T, c.Ci, c.Co, aligned=c.id != "E6"), c
        assert c.B * c.T <= 1024 and c.Ci * c.K <= 640
    assert {c.id for c in R.OPS} == {"E1", "E2", "E3", "E4", "E5a", "E5b", "E6", "I1", "I2", "I2b", "I3", "I4"}
    assert {(c.id, c.prec) for c in R.WGS} == {("W1", "f16x3"), ("W1", "x6"), ("W2", "f16x3"), ("W3", "f16x3"), ("W4", "f16x3"), ("W4", "x6"),
                                               ("W5", "f16x3"), ("W5", "x6")}
    w1 = [c for c in R.WGS if c.id == "W1"][0]
    assert [R.wgrad_route(*w1[1:8], "f16x3", j) for j in range(3)] == [("fp32", 64, 16), ("f16x3", 224, 56), ("f16x3", 384, 96)]
    w2 = [c for c in R.WGS if c.id == "W2"][0]
    assert [R.wgrad_route(*w2[1:8], "f16x3", j) for j in range(3)][:2] == [None, None]
    c6b = [c for c in R.BLOCKS if c.id == "C6b"][0]
    assert R.levels(c6b)[-1][2] >= c6b.T            # the last level's first two taps read nothing: a zero dw_t under its weight_v gradient
    assert len(R.CASES) == len(R.OPS) + len(R.WGS) + len(R.BLOCKS)


def _pick(id_, form, prec="f16x3"):
    return [c for c in R.OPS if (c.id, c.form, c.prec) == (id_, form, prec)][0]


SENSITIVITY = (          # (planted error, case id, form)
    ("lo_hi", "I1", "pre"), ("lo_hi", "I1", "anti"), ("slot", "I1", "pre"), ("slot20", "I1", "pre"), ("leak", "I1", "pre"), ("leak", "E1", "pre"), ("slab", "E1", "pre"),
    ("drop_row", "I1", "drop"), ("drop_row", "E1", "drop"), ("res_first", "I1", "res"), ("res_first", "E1", "res"),
)


def test_planted_errors_are_rejected_by_the_new_bar():
    """each planted error in the emulation of one interior (I1) and one edge (E1) case: the new bar rejects it; printed beside it what
    close() of tests/test_gpu_parity.py makes of the same tensors at its tolerances: 1e-4 max(1, max |ref|) on outputs, 2e-4 on gradients.
    A slot 2^8 too large turns out to be no error at all at these statistics: scaled to 2^6 instead of 2^14 the low fp16 term still holds
    its eleven bits (fp16 is normal down to 2^-14), the result stays AT the yardstick (ratio 1.0; the GPU file asserts the same for 2^6),
    and the bar starts to notice a slot from 2^18 on -- 2^20 is rejected here and passes close().  A dropped lo hi product costs 1.4e-4 .. 1.9e-4 of the
    maximum, AT the old bar -- rejected at 1e-4, passed at the gradient tolerance (the time-flipped form is a data gradient).  A whole
    leaked row is a gross error on values of order one, which close() does reject; it passes close() at gradient-like magnitudes (the same
    tensors x 2^-20, the statistics of C5), where max(1, .) makes the old bar absolute -- as does every other plant.  The relative bar
    rejects each at any magnitude."""
    seen = set()
    for plant, id_, form in SENSITIVITY:
        c = _pick(id_, form)
        ref = R.op_data(c)["ref"]
        got = R.op_emulate(c, plant=plant)
        ratio, name, fails = R.check_op(got, c, quiet=True)
        old = R.close_verdict(got["y"], ref["y"], 2e-4 if form == "anti" else 1e-4)
        old_small = R.close_verdict(got["y"] * 2.0 ** -20, ref["y"] * 2.0 ** -20)
        print("%-9s %-12s new bar: %10.1f x the yardstick   close(): %s   close() at x 2^-20: %s   -- %s"
              % (plant, R.case_id(c), ratio, "passes" if old else "rejects", "passes" if old_small else "rejects", R.PLANT_TEXT[plant]))
        if plant == "slot":
            assert not fails and ratio <= R.BOUND, (plant, ratio)
            continue
        assert fails and ratio > R.BOUND, (plant, R.case_id(c), ratio)
        clean = R.check_op(R.op_emulate(c), c, quiet=True)
        assert not clean[2] and clean[0] <= R.BOUND
        if plant == "slot20" or (plant == "lo_hi" and form == "anti"):
            assert old, (plant, "the old bar was expected to miss this")
        assert old_small, (plant, "max(1, .) makes the old bar absolute at small magnitudes")
        seen.add(plant)
    seen.add("slot")
    assert seen == set(R.PLANTS) - {""}
