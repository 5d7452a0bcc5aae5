"""m3t.ops._armed_call on the MI355X: a call that ctypes refuses before the C side runs leaves no magnitude-slot pointer parked for the
next kernel (tests/test_amax_arm_rule.py keeps every arm site of m3t/ops.py on this helper)."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def test_a_refused_call_leaves_nothing_armed():
    from m3t import ops
    x = torch.tensor([[-1.0, 2.0, float("nan"), -0.5]] * 4, dtype=torch.float32, device=DEV)
    y = torch.empty_like(x)
    S = torch.zeros(1, dtype=torch.int64, device=DEV)
    with pytest.raises(ctypes.ArgumentError):      # "four" stands where size_t M belongs: the C function is never entered
        ops._armed_call(S.data_ptr(), "m3t_relu_cl_fwd", ops._p(x), "four", 4, ops._p(y), ops._stream())
    # the next producing call, unarmed: were the pointer still parked, this kernel would raise S to the bits of max |y|
    assert ops.lib().m3t_relu_cl_fwd(ops._p(x), 4, 4, ops._p(y), ops._stream()) == 0
    torch.cuda.synchronize()
    assert int(S.item()) == 0
    ref = torch.relu(x)
    assert bool(torch.isnan(y[:, 2]).all()) and torch.equal(torch.nan_to_num(y, nan=-7.0), torch.nan_to_num(ref, nan=-7.0))
