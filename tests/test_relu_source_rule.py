"""Every fused ReLU in the HIP sources keeps NaN as torch.relu does (CPU).

fmaxf(NaN, 0.f) is 0: a ReLU written that way hides a diverged input from the loss and from the optimizer's non-finite guard.
csrc/common.h defines m3t_relu for that purpose; this rule keeps fmaxf(<expr>, 0.f) out of every other line of the kernels."""
import glob
import os
import re

from conftest import PKG

CSRC = os.path.join(PKG, "csrc")
_ZERO = re.compile(r"^\s*(?:0|0\.|0\.0*|\.0+)(?:f|F)?\s*$")


def _fmaxf_with_zero(line):
    """the fmaxf(a, b) calls of `line` (nested ones included) whose second argument is a zero literal"""
    hits = []
    for m in re.finditer(r"\bfmaxf\s*\(", line):
        depth, i, comma = 1, m.end(), None
        while i < len(line) and depth:
            c = line[i]
            if c == "(":
                depth += 1
            elif c == ")":
                depth -= 1
            elif c == "," and depth == 1:
                comma = i
            i += 1
        if depth == 0 and comma is not None and (_ZERO.match(line[comma + 1:i - 1]) or _ZERO.match(line[m.end():comma])):
            hits.append(line[m.start():i])
    return hits


def test_the_rule_catches_a_nan_dropping_relu():
    assert _fmaxf_with_zero("v = fmaxf(v, 0.f);")
    assert _fmaxf_with_zero("o = fmaxf(fmaxf(a + b[i], 0.0f) * mk + r, 0.f);")
    assert _fmaxf_with_zero("s.x = fmaxf(0.f, s.x);")
    assert not _fmaxf_with_zero("mx = fmaxf(mx, m3t_fin_abs(r));")
    assert not _fmaxf_with_zero("v = m3t_relu(v);")


def test_no_fmaxf_relu_outside_m3t_relu():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.inc")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert any(f.endswith("common.h") for f in files) and len(files) > 10
    bad, defined = [], False
    for f in files:
        with open(f) as fh:
            for n, line in enumerate(fh, 1):
                code = line.split("//", 1)[0]
                if re.search(r"\bfloat\s+m3t_relu\s*\(", code):
                    defined = True
                    continue
                for h in _fmaxf_with_zero(code):
                    bad.append("%s:%d: %s" % (os.path.basename(f), n, h))
    assert defined, "csrc/common.h no longer defines m3t_relu"
    assert not bad, "ReLU written as fmaxf(x, 0) drops NaN; use m3t_relu:\n" + "\n".join(bad)
