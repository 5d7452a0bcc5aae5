"""tests/conv_ref.py checked on the CPU: the tap rule and the parity-class decomposition against torch's float64 autograd, the restated
dispatch against the case table (and the class plan against ops._dgrad_plan), the product models against the reference, the admission of
every case, the coverage of the table -- every path, every edge, both sides of every path-selection rule -- and the sensitivity of the new
bar to seven planted errors next to what close() of tests/test_gpu_parity.py makes of them.  Run with -s for the figures."""
import numpy as np
import torch

import conv_ref as R

TIGHT = 1e-13


def _uniq(cases, key):
    seen, out = set(), []
    for c in cases:
        if key(c) not in seen:
            seen.add(key(c))
            out.append(c)
    return out


def test_tap_rule_and_parity_classes_against_float64_autograd():
    worst = 0.0
    for c in _uniq(R.CASES, lambda c: c.geo):
        if R.flops(c) > 2e8:                      # (the rules do not depend on the size: the largest geometries are left to the reference itself)
            continue
        Ci, Co, k, st, pd, N, T, H, W = c.geo
        x, w, b, ct = (a.astype(np.float64) for a in R.draw(c.geo, "normal"))
        ref = R.torch_conv(x, w, b, ct, st, pd, torch.float64)
        got = dict(zip(("y", "dx", "dw", "db"), R.conv3d_taps_ref(x, w, b, st, pd, ct)))
        got["dx (classes)"] = R.dgrad_classes_ref(ct, w, st, pd, (T, H, W))
        for n, g in got.items():
            e = R.rel_err(g, ref[n[:2]])
            worst = max(worst, e)
            assert e <= TIGHT, (c.id, n, e)
        z = R.zero_mask(c)
        assert not got["dx (classes)"][z].any() and not ref["dx"][z].any()
    print("tap rule / parity classes vs float64 autograd: worst rel_err %.3g" % worst)


def test_class_plan_and_dispatch_restate_ops():
    from m3t import ops
    for c in R.CASES:
        Ci, Co, k, st, pd, N, T, H, W = c.geo
        mine = [(cls, list(r), list(sub), list(size), list(base)) for cls, r, sub, size, base in R.dgrad_plan(k, st, pd, (T, H, W))]
        assert mine == ops._dgrad_plan(k, st, pd, (T, H, W)), c.id
        assert R.route(c) == (c.fwd, c.dx, c.dw), (c.id, R.route(c))
        assert set(c.off) <= set(R.SWITCHES) and all(hasattr(ops, s) for s in c.off)
    assert R.WS_MIN == ops._WS_MIN


def test_every_case_is_admitted():
    for c in R.CASES:
        d = R.data(c)
        assert R.flops(c) <= R.MAX_FLOP, c.id
        assert set(R.tensor_names(c)) <= set(d["ref"])
        for n in R.tensor_names(c):
            top = np.abs(d["ref"][n]).max()
            assert np.isfinite(top) and top > 0, (c.id, n)
        z = R.zero_mask(c)
        assert not d["ref"]["dx"][z].any(), c.id                     # the stated zero regions really are zero in the reference
        assert np.count_nonzero(d["ref"]["dx"][~z]) > 0.99 * (~z).sum(), c.id
    w5 = R.BY_ID["W5"]
    assert R.zero_mask(w5).mean() == 0.75 and len(R.dgrad_plan(*w5.geo[2:5], w5.geo[6:])) == 1
    assert {c.id for c in R.CASES if R.zero_mask(c).any()} == {"W5", "P3"}       # (P3: the last time step lies behind the last window)


def test_emulation_within_the_bound_of_the_reference():
    """yardstick B is an fp32 computation: on normal statistics every product model sits within BOUND max(E32, 2^-24) of float64"""
    worst = {}
    for c in R.CASES:
        if c.stats != "normal":
            continue
        d, e = R.data(c), R.emulated(c)
        for n, m in zip(R.tensor_names(c), [c.fwd] + (["dx " + c.dx] if c.dx else []) + ["dw " + c.dw, "db"]):
            m = "%s %s" % (c.prec, m)
            r = e[n] / max(d["e32"][n], R.FLOOR)
            worst[m] = max(worst.get(m, (0, "")), (r, c.id + ":" + n))
            assert r <= R.BOUND, (c.id, n, e[n], d["e32"][n])
    for m, (r, where) in sorted(worst.items()):
        print("emulation %-22s worst E_emu / max(E32, 2^-24) = %5.2f  (%s)" % (m, r, where))


def test_decades_limits_come_from_the_emulation_alone():
    for c in R.CASES:
        if c.stats != "decades":
            continue
        d, e, lim = R.data(c), R.emulated(c), R.limits(c)
        for n in R.tensor_names(c):
            fp32_bar = R.BOUND * max(d["e32"][n], R.FLOOR)
            hi, lo = lim[n]
            if e[n] > fp32_bar:
                assert (hi, lo) == (R.BOUND * e[n], fp32_bar)
            else:
                assert lo is None and hi == R.BOUND * max(d["e32"][n], e[n], R.FLOOR)
            print("%s %-2s E32 %.3g  E_emu %.3g  %s" % (c.id, n, d["e32"][n], e[n], "normwise limit reached" if lo else "within the fp32 bar"))


def test_the_table_covers_what_it_names():
    ids = [c.id for c in R.CASES]
    assert len(set(ids)) == len(ids)
    assert set(ids) == {"W1", "W2", "W3", "W4", "W5", "W6", "W7", "W8", "F1", "F2", "F3", "P1", "P2", "P3", "P4", "X1", "X2", "S1", "S2", "T1",
                        "C1", "C2", "C3", "C4", "D1", "D2", "M1"}
    assert {c.op for c in R.CASES} == {"conv3d", "conv2d", "conv3d_cl", "conv3d_cl2"}
    assert {c.fwd for c in R.CASES} == {"walk", "walk4", "patch", "torch"}
    assert {c.dx for c in R.CASES} == {"walk", "walk_loop", "walk_x6", "stock", ""}
    assert {c.dw for c in R.CASES} == {"walk", "dyTP", "PTdy", "ceil4"}
    assert {c.stats for c in R.CASES} == {"normal", "small", "decades"}
    assert {c.off for c in R.CASES} == {(), ("CONV3D_IMPLICIT",), ("CONV3D_PRESPLIT",), ("WGRAD_IMAGES",)}
    assert {(c.prec, c.fwd) for c in R.CASES if c.prec == "x6"} == {("x6", "patch")}
    # the edges by name
    g = lambda id_: R.grids(R.BY_ID[id_])
    assert g("W1")[1] == 75 and R.BY_ID["W1"].geo[0] * g("W1")[3] == 288
    assert R.plans(R.BY_ID["W1"])["fwd"] == [(1, 288, True)] and R.plans(R.BY_ID["W1"])["dw"][0][0] == 1          # no slabs, ragged last k tile
    w2 = R.plans(R.BY_ID["W2"])
    assert w2["fwd"][0][0] > 1 and w2["dx"][0][0] > 1 and w2["dw"][0][0] > 1 and g("W2")[1] == 512
    sizes = lambda id_: sorted(tuple(s[3]) for s in R.dgrad_plan(*R.BY_ID[id_].geo[2:5], R.BY_ID[id_].geo[6:]))
    assert g("W3")[1] == 192 and sizes("W3") == [(1, 7, 7), (1, 7, 8), (1, 8, 7), (1, 8, 8)]
    assert len(sizes("W4")) == 8 and len(set(sizes("W4"))) == 8 and g("W4")[1] % 128 != 0
    assert len(sizes("W6")) == 2 and R.BY_ID["W6"].geo[3] == (2, 1, 1)
    assert 96 * 9 == 864 and 864 % 128 != 0 and 128 > 96                                                            # W7
    assert R.BY_ID["W8"].geo[8] % 4 != 0
    for id_, kw in (("F1", 3), ("F2", 7), ("F3", 8)):
        assert R.BY_ID[id_].geo[2][2] == kw and R.channel_width(R.BY_ID[id_]) == 4
    assert R.BY_ID["F3"].geo[:2] == (1, 128)
    assert g("P1")[1] == 128 and 8 * 27 == 216 and g("P2")[1] == 128 and 16 * 4 == 64
    # both sides of every path-selection rule, for the stated workspace size; no plan of the table depends on that size (the cap on the
    # number of slabs binds nowhere), so a larger workspace plans the same
    every = [(c, p, t) for c in R.CASES for p, ts in R.plans(c).items() for t in ts]
    for p in ("fwd", "dx"):
        assert {t[0] > 1 for c, q, t in every if q == p} == {True, False}, "slabs and none: " + p
    assert {t[0] > 1 for c, q, t in every if q == "dw"} == {True, False}, "row split and none"
    for p in ("fwd", "dx", "dw"):
        assert {t[2] for c, q, t in every if q == p} == {True, False}, "narrow and wide: " + p
    for c in R.CASES:
        assert R.plans(c) == R.plans(c, 1 << 30), c.id
    # T1: the smallest number of row tiles at which the forward walk of its layer takes the 128 x 128 tile with slabs
    t1 = R.BY_ID["T1"]
    Ci, Co, k = t1.geo[:3]
    rows = g("T1")[1]
    assert rows == 17 * 128 and R.walk_plan(rows, Co, 27 * Ci) == (12, 288, False)
    assert all(R.walk_plan(r, Co, 27 * Ci)[2] for r in range(128, rows - 127, 128))
    assert all(not t[2] and t[0] > 1 for ts in R.plans(t1).values() for t in ts)
    assert max(R.flops(c) for c in R.CASES) == R.flops(t1) == R.MAX_FLOP


SENSITIVITY = (          # (planted error, case, the tensor it reaches, does close() let it through?)
    ("lo_hi_tap", "W2", "y", True), ("lo_last_tile", "W1", "dw", True), ("bias_f16", "W1", "y", None), ("clamp", "W2", "y", False),
    ("class_r", "W3", "dx", False), ("tap8", "F1", "y", False), ("lo_hi", "W2", "dx", None), ("lo_hi", "M1", "dx", True),
)


def test_planted_errors_are_rejected_by_the_new_bar():
    """each planted error in the emulation of the case built for it: the new bar rejects it; printed beside it what close() of
    tests/test_gpu_parity.py makes of the same tensor at its tolerance (1e-4 max(1, max |ref|) on y, 2e-4 on gradients).  The two
    partial-precision plants -- one tap of 27, the ragged last k tile -- pass close() by a wide margin; a lost cross product everywhere sits on
    its edge at values of order one and is invisible to it at gradient-like magnitudes (M1), where max(1, .) makes the old bar absolute."""
    seen, passed_old = set(), 0
    for plant, id_, name, old_passes in SENSITIVITY:
        c = R.BY_ID[id_]
        ref = R.data(c)["ref"]
        clean = R.emulate(c)
        r0, _, f0 = R.check(clean, c, quiet=True)
        assert not f0 and r0 <= R.BOUND
        got = R.emulate(c, plant=plant)
        for n in R.tensor_names(c):               # the plant reaches the tensor it is meant for, and only that
            assert (n == name) != np.array_equal(got[n], clean[n]), (plant, id_, n)
        ratio, worst, fails = R.check(got, c, quiet=True)
        old = R.close_verdict(got[name], ref[name], R.CLOSE_TOL[name])
        print("%-13s %-3s %-3s rel_err %.2e  new bar: %9.1f x the yardstick   close(): %s   -- %s"
              % (plant, id_, name, R.rel_err(got[name], ref[name]), ratio, "passes" if old else "rejects", R.PLANT_TEXT[plant]))
        assert fails and ratio > R.BOUND and worst == name, (plant, id_, ratio)
        if old_passes is not None:
            assert old == old_passes, (plant, id_, "close() was expected to %s this" % ("miss" if old_passes else "reject"))
        passed_old += bool(old)
        seen.add(plant)
    assert seen == set(R.PLANTS) - {""} and len(seen) >= 6
    assert passed_old >= 2
