"""M3T_GEMM_TR: the fp16x3 tile kernels stage a row-contiguous operand (A of a TN product, B of an NN one) in LDS as it lies in memory and
read the MFMA operands with transposed LDS reads, instead of transposing 4 x 4 blocks across lanes into 16-byte records.  Every lane ends
up with the same eight halves in the same order, so every MFMA sees the operands it saw: the results are the SAME BITS, on every kernel
(gemm_x6d.hip alone, gemm_x6.hip beside a scan / in the background, gemm_x6w.hip where the planner takes the 128 x 256 tile), tile
width, split-K count, epilogue and operand content.  M3T_GEMM_TR = 1 against 0 in fresh child processes (tests/gemm_tr_child.py)."""
import os
import subprocess
import sys

import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

BESIDE_SCAN, BACKGROUND = 512, 1      # include/m3t_hip.h


def _child(tmp_path, what, flags, tr, extra_env=None):
    out = os.path.join(str(tmp_path), "%s_%d_tr%s.pt" % (what, flags, tr))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["M3T_GEMM_TR"] = tr
    env["M3T_SCAN_LOCK"] = "0"
    env.update(extra_env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gemm_tr_child.py"), what, str(flags), out], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return torch.load(out)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), \
        "%s: %d of %d values differ" % (what, int((a.view(torch.int32) != b.view(torch.int32)).sum()), a.numel())


@pytest.mark.parametrize("flags", [0, BESIDE_SCAN, BACKGROUND], ids=["alone_x6d", "beside_scan_x6", "background_x6"])
def test_products_are_bit_identical(tmp_path, flags):
    on, off = _child(tmp_path, "gemm", flags, "1"), _child(tmp_path, "gemm", flags, "0")
    assert set(on["res"]) == set(off["res"]) and len(on["res"]) >= 27
    assert on["splits"] == off["splits"]                       # the switch changes no split-K count
    sp = on["splits"]
    assert sp["tn_128_one"] == 1 and sp["tn_64_one"] == 1 and sp["nn_128_one"] == 1 and sp["seg_128_one"] == 1
    if flags != BESIDE_SCAN:                                     # (beside a scan the slab count follows the free CUs: checked by the values alone)
        assert sp["tn_128_split"] > 1 and sp["nn_128_split"] > 1 and sp["seg_128_split"] > 1 and sp["tn_64_split"] > 1
    for name in sorted(on["res"]):
        _same_bits(on["res"][name], off["res"][name], name)
    # the results are products, not leftovers: a finite case against float64 would be test_gpu_parity's job; here: not all zero, non-finite where fed
    assert float(on["res"]["tn_128_split"].abs().max()) > 1.0
    # (an infinite operand splits into inf + (inf - inf): its products are non-finite, not necessarily infinite)
    assert bool(torch.isnan(on["res"]["tn_nan"]).any()) and not bool(torch.isfinite(on["res"]["tn_inf"]).all())


@pytest.mark.parametrize("images", ["1", "0"], ids=["conv_images", "conv_split_in_loop"])
def test_conv_weight_gradient_is_bit_identical(tmp_path, images):
    env = {"M3T_WGRAD_IMAGES": images}
    on, off = _child(tmp_path, "conv", 0, "1", env), _child(tmp_path, "conv", 0, "0", env)
    assert set(on["res"]) == set(off["res"]) and len(on["res"]) == 6
    for name in sorted(on["res"]):
        _same_bits(on["res"][name], off["res"][name], name + " images=" + images)
    assert float(on["res"]["stem_128_dw"].abs().max()) > 0.0
