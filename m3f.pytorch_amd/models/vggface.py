"""models.vggface -- the VGGFace per-frame front-end (reference models/vggface.py), as a channels-last chain on the HIP library.

Names, constructor signatures, parameter creation order and state_dict keys are the reference's (`conv{1..5}.convs.{i}.weight/bias` as
nn.Conv2d parameters [Co, Ci, 3, 3], `fc1`): a reference checkpoint loads strictly, `torch.manual_seed` + construction draws the same values.

On the chain (m3t.ops.vggface_ok: an fp32 device input, the fp16x3 mode, the chain's switches on) the thirteen Conv2d(3x3, pad 1) are the tap
walks of m3t.ops.conv3d_cl with a unit time tap (bias in the walk), the inner ReLUs m3t.ops.relu_cl (in place on the convolution's output),
each block's last ReLU + max_pool2d(2, 2, 0, ceil_mode=True) one operator (m3t.ops.relu_pool_cl), `fc1` + ReLU the GEMM and the dropout an
in-kernel Philox mask (m3t.ops.relu_dropout).  Nothing between the video and `fc1` is transposed except the [P, 16, 512] -> [P, 512, 16] turn
that gives `x.view(P, -1)` the reference's (c, h, w) order.  Off the chain the convolutions go through m3t.ops.conv2d (stock on the CPU) and
F.relu / F.max_pool2d are the stock ops; that exit is announced once on stderr (m3t.ops.stock_fallback).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from m3t import ops


# channel counts of the five blocks: block i holds len(units) - 1 convolutions, units[j] -> units[j + 1] channels
_BLOCK_UNITS = ((3, 64, 64), (64, 128, 128), (128, 256, 256, 256), (256, 512, 512, 512), (512, 512, 512, 512))


class VGGFace(nn.Module):
    """five convolution blocks `conv1` .. `conv5`, then `fc1` on the 4 x 4 x 512 map a 112 x 112 frame leaves (7 -> 4 by the last ceil-mode
    pooling), ReLU and Dropout(0.5)"""

    def __init__(self):
        super().__init__()
        for i, units in enumerate(_BLOCK_UNITS, 1):          # (creation order = the reference's: the RNG draws line up)
            setattr(self, "conv%d" % i, _ConvBlock(*units))
        self.dropout = nn.Dropout(0.5)
        self.fc1 = nn.Linear(4 * 4 * _BLOCK_UNITS[-1][-1], 4096)

    def _blocks(self, x):
        for blk in (self.conv1, self.conv2, self.conv3, self.conv4, self.conv5):
            x = blk(x)
        return x

    def forward(self, x):
        """x: frames [P, 3, H, W]; or, from VA_VGGFace, clips [B, 3, T, H, W] / a VideoCL (P = B T frames, clip-major) -> [P, 4096]"""
        if ops.vggface_ok(x):
            if not isinstance(x, ops.CLTensor) and x.dim() == 4:
                x = x.unsqueeze(2)                                     # [P, 3, 1, H, W]: every frame a clip of one
            x = self._blocks(x)
            P, hw, Cc = x.N * x.T, x.H * x.W, x.C
            flat = ops.btc_to_bct(x.data.view(P, hw, Cc)).view(P, Cc * hw)      # the reference's x.view(P, -1): (c, h, w)
        else:
            ops.stock_fallback("models.vggface.VGGFace", "CPU / non-fp32 input, a precision mode or a switch the channels-last chain does not cover")
            if isinstance(x, ops.CLTensor):
                x = x.planes()
            if x.dim() == 5:                                           # fold T into the batch (reference backbone.py:38-39)
                x = x.transpose(1, 2).reshape(-1, x.size(1), x.size(3), x.size(4))
            x = self._blocks(x)
            flat = x.reshape(x.size(0), -1)
        if flat.is_cuda and flat.dtype == torch.float32:
            h = ops.linear(flat, self.fc1.weight, self.fc1.bias, 1)    # ReLU in the GEMM's epilogue
            if self.training:
                # nn.Dropout(0.5) (reference vggface.py:27) as the GRU heads': a Philox mask made in the kernel, forward and backward;
                # self.drop_seed overrides the seed (tests)
                h = ops.relu_dropout(h, self.dropout.p, getattr(self, "drop_seed", None))
            return h
        return self.dropout(F.relu(self.fc1(flat)))


class _ConvBlock(nn.Module):
    """`convs`: Conv2d(3 x 3, stride 1, padding 1) from units[j] to units[j + 1] channels for every neighbouring pair of `units`; forward applies
    each with a ReLU and closes with the 2 x 2 ceil-mode max pooling"""

    def __init__(self, *units):
        super().__init__()
        self.convs = nn.ModuleList(nn.Conv2d(cin, cout, kernel_size=3, stride=1, padding=1) for cin, cout in zip(units, units[1:]))

    def forward(self, x):
        # reference vggface.py:45-50
        if isinstance(x, ops.CLTensor) or (x.dim() == 5 and ops.vggface_ok(x)):
            last = len(self.convs) - 1
            for i, c in enumerate(self.convs):
                if not ops.conv3d_cl_ok(x, c.weight, c.stride, c.padding, c.groups, c.dilation, c.padding_mode):
                    raise ops.M3THipError("models.vggface: the channels-last chain does not cover Conv2d(%d, %d)" % (c.in_channels, c.out_channels))
                x = ops.conv3d_cl(x, c.weight, c.bias, c.stride, c.padding)
                x = ops.relu_pool_cl(x, ceil_mode=True) if i == last else ops.relu_cl(x, inplace=True)
            return x
        for c in self.convs:
            if x.is_cuda and x.dtype == torch.float32:
                x = F.relu(ops.conv2d(x, c.weight, c.bias, c.stride, c.padding))
            else:
                x = F.relu(c(x))
        return F.max_pool2d(x, 2, 2, 0, ceil_mode=True)
