"""models.rnn -- BiGRU stack + per-timestep FC head, MI355X-native.

Drop-in for the reference's models/rnn.py:11-81 (`GRU`): same constructor, same
forward contract ([B,T,I] -> [B,T,2H] | [B,T,nC] | (out, h[2L,B,H])), same parameter
names/shapes (`gru.weight_ih_l{k}[_reverse]`, `gru.weight_hh_...`, `gru.bias_..`,
`fc.*`), same initialisation recipe (rnn.py:57-69) drawn in the same RNG order.
The arithmetic runs in libm3t_hip.so: input projections and FC layers on the fp32-MFMA
GEMM, the recurrence in the grouped per-step scan kernels (m3t.ops.multi_bigru).
`Attention`, `Decoder`, `AttEncDec` (rnn.py:84-165, --fusion_type att_dec): same constructors, attribute names
and init order; the decoder loop runs in csrc/attdec.hip (m3t.ops.att_decode), greedy or teacher-forced with the
reference's `random.random()` draws (m3t.ops.teacher_forcing_mask).  One decoder layer, input and output width 2.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from m3t import ops


class BiGRUParameters(nn.Module):
    """Parameter holder with nn.GRU's names, shapes, registration order and default init
    (bidirectional unless told otherwise, batch_first).  No forward: the scan lives in m3t.ops."""

    def __init__(self, input_size, hidden_size, num_layers, bidirectional=True):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.bidirectional = bidirectional
        H = hidden_size
        for layer in range(num_layers):
            in_l = input_size if layer == 0 else (2 if bidirectional else 1) * H
            for suffix in ("", "_reverse") if bidirectional else ("",):
                tag = "l%d%s" % (layer, suffix)
                self.register_parameter("weight_ih_" + tag, nn.Parameter(torch.empty(3 * H, in_l)))
                self.register_parameter("weight_hh_" + tag, nn.Parameter(torch.empty(3 * H, H)))
                self.register_parameter("bias_ih_" + tag, nn.Parameter(torch.empty(3 * H)))
                self.register_parameter("bias_hh_" + tag, nn.Parameter(torch.empty(3 * H)))
        bound = 1.0 / math.sqrt(H) if H > 0 else 0.0
        for p in self.parameters():
            nn.init.uniform_(p, -bound, bound)

    def flatten_parameters(self):   # reference calls it every forward (rnn.py:72); nothing to do here
        return None

    def flat(self):
        """[w_ih, w_hh, b_ih, b_hh] for (layer 0 fwd, layer 0 rev, layer 1 fwd, ...)."""
        out = []
        for layer in range(self.num_layers):
            for suffix in ("", "_reverse"):
                tag = "l%d%s" % (layer, suffix)
                out += [getattr(self, "weight_ih_" + tag), getattr(self, "weight_hh_" + tag),
                        getattr(self, "bias_ih_" + tag), getattr(self, "bias_hh_" + tag)]
        return out


def _build_head(hidden_size, num_classes, num_fcs, dropout):
    """FC head with the reference's child indices (rnn.py:20-55) so state_dict keys match."""
    H = hidden_size
    if num_fcs == 1:
        return nn.Linear(2 * H, num_classes)
    widths = [2 * H] + [H] * (num_fcs - 1) + [num_classes]
    mods = []
    for i in range(num_fcs):
        mods.append(nn.Linear(widths[i], widths[i + 1]))
        if i != num_fcs - 1:
            mods.append(nn.ReLU(True))
            if dropout:
                mods.append(nn.Dropout(0.5))
    return nn.Sequential(*mods)


class GRU(nn.Module):
    def __init__(self, input_size, hidden_size, num_layers, num_classes, num_fcs=1, dropout=False, return_h=False):
        super().__init__()
        self.hidden_size = hidden_size
        self.num_layers = num_layers
        self.num_classes = num_classes
        self.return_h = return_h
        self.gru = BiGRUParameters(input_size, hidden_size, num_layers)
        if num_classes > 0:
            if num_fcs not in (1, 2, 3):
                raise ValueError("num_fcs must be 1, 2 or 3")
            self.fc = _build_head(hidden_size, num_classes, num_fcs, dropout)
        self._init_gru(input_size, hidden_size)

    def _init_gru(self, input_size, hidden_size):
        # rnn.py:57-69: per-gate U(+-sqrt(3)*sqrt(2/(I+H))) for every weight_ih (layer-1 also uses the
        # layer-0 I), per-gate orthogonal weight_hh, zero biases.
        H = hidden_size
        lim = math.sqrt(3.0) * math.sqrt(2.0 / (input_size + hidden_size))
        with torch.no_grad():
            for name, p in self.gru.named_parameters():
                for g0 in range(0, 3 * H, H):
                    if "weight_ih" in name:
                        nn.init.uniform_(p[g0:g0 + H], -lim, lim)
                    elif "weight_hh" in name:
                        nn.init.orthogonal_(p[g0:g0 + H])
                    elif "bias" in name:
                        nn.init.constant_(p[g0:g0 + H], 0.0)

    # -- pieces exposed so that callers can advance several independent GRUs in one grouped scan
    def stack(self, x):
        return (x, self.gru.flat(), self.num_layers)

    def head(self, out):
        if self.num_classes <= 0:
            return out
        if isinstance(self.fc, nn.Linear):
            return ops.linear(out, self.fc.weight, self.fc.bias, 0)
        layers = [m for m in self.fc if isinstance(m, nn.Linear)]
        drops = [m for m in self.fc if isinstance(m, nn.Dropout)]
        for i, lin in enumerate(layers):
            last = i == len(layers) - 1
            out = ops.linear(out, lin.weight, lin.bias, 0 if last else 1)     # ReLU fused in the GEMM epilogue
            if not last and drops and self.training:
                # nn.Dropout(0.5) of the `dropout=True` heads (reference rnn.py:24-28,40-49): Philox mask generated inside
                # the kernel, forward and backward (no mask tensor, no torch RNG kernel); self.drop_seeds overrides the seeds (tests)
                seeds = getattr(self, "drop_seeds", None)
                out = ops.relu_dropout(out, drops[0].p, None if seeds is None else seeds[i])
        return out

    def forward(self, x):
        self.gru.flatten_parameters()
        ((out, h_n),) = ops.multi_bigru([self.stack(x)])
        out = self.head(out)
        if self.return_h:
            return out, h_n
        return out


def run_grus(modules, inputs):
    """Advance several independent `GRU` modules (same batch, length and depth) together:
    one grouped scan per layer level instead of one per module.  Returns the per-module
    outputs after their FC heads (and ignores return_h)."""
    res = ops.multi_bigru([m.stack(x) for m, x in zip(modules, inputs)])
    return [m.head(o) for m, (o, _) in zip(modules, res)]


def run_grus_cat(modules, inputs, lo, hi):
    """`run_grus` followed by `torch.cat(outputs[lo:hi], dim=-1)` (the visual towers' gru_v | gru_a features, reference
    models/model.py:111-112 / models/backbone.py:281-283): the list of outputs with the concatenation in place of the group.
    When the grouped modules end without an FC head (num_classes <= 0) their scans write straight into the concatenated buffer
    (m3t.ops.multi_bigru(cat=...)): no cat copy forward, no slice copies backward."""
    if hi - lo >= 2 and all(m.num_classes <= 0 for m in modules[lo:hi]):
        res = ops.multi_bigru([m.stack(x) for m, x in zip(modules, inputs)], cat=(lo, hi))
        outs = [m.head(o) if not (lo < i < hi) else None for i, (m, (o, _)) in enumerate(zip(modules, res))]
        return outs[:lo + 1] + outs[hi:]
    outs = run_grus(modules, inputs)
    return outs[:lo] + [torch.cat(outs[lo:hi], dim=-1)] + outs[hi:]


class Attention(nn.Module):
    """Reference models/rnn.py:84-111: additive attention over the encoder frames."""

    def __init__(self, hidden_size):
        super().__init__()
        self.hidden_size = hidden_size
        self.attn = nn.Linear(self.hidden_size * 2, hidden_size)
        self.v = nn.Parameter(torch.rand(hidden_size))
        stdv = 1. / math.sqrt(self.v.size(0))
        self.v.data.uniform_(-stdv, stdv)

    def forward(self, hidden, encoder_outputs):
        """hidden [B,H], encoder_outputs [B,T,H] -> softmax weights [B,1,T]"""
        return ops.attention_weights(hidden, encoder_outputs, self.attn.weight, self.attn.bias, self.v).unsqueeze(1)


class Decoder(nn.Module):
    """Reference models/rnn.py:114-142: one attention + GRU-cell + output step.  The kernels fix the input and output width at 2
    (AttEncDec's) and the depth at one layer."""

    def __init__(self, embed_size=128, hidden_size=512, output_size=2, n_layers=1):
        super().__init__()
        if n_layers != 1:
            raise NotImplementedError("Decoder: only n_layers = 1 (the reference's AttEncDec) runs on the HIP decoder")
        if embed_size != 2 or output_size != 2:
            raise NotImplementedError("Decoder: the HIP decoder feeds its 2 outputs back as its 2 inputs (embed_size = output_size = 2)")
        self.embed_size = embed_size
        self.hidden_size = hidden_size
        self.output_size = output_size
        self.n_layers = n_layers
        self.attention = Attention(hidden_size)
        self.gru = BiGRUParameters(hidden_size + embed_size, hidden_size, n_layers, bidirectional=False)
        self.out = nn.Linear(hidden_size * 2, output_size)

    def weights(self):
        g = self.gru
        return (self.attention.attn.weight, self.attention.attn.bias, self.attention.v, g.weight_ih_l0, g.weight_hh_l0,
                g.bias_ih_l0, g.bias_hh_l0, self.out.weight, self.out.bias)

    def forward(self, inputs, last_hidden, encoder_outputs):
        """inputs [B,2], last_hidden [1,B,H], encoder_outputs [B,T,H] -> (output [B,2], hidden [1,B,H], attn_weights [B,1,T])"""
        out, h, _ = ops.att_decode(encoder_outputs, last_hidden[-1], *self.weights(), y0=inputs, L=2)
        # the weights the step used, as a differentiable output of their own (att_decode's copy carries no gradient)
        attn_weights = self.attention(last_hidden[-1], encoder_outputs)
        return out[:, 1], h.unsqueeze(0), attn_weights


class AttEncDec(nn.Module):
    """Reference models/rnn.py:145-165: BiGRU encoder, directions summed, attention decoder over T-1 steps (greedy, or teacher-forced
    with probability teacher_forcing_ratio per step when a target is given)."""

    def __init__(self):
        super().__init__()
        self.encoder = GRU(1024, 512, 2, -1, return_h=True)
        self.decoder = Decoder(2, 512, 2, 1)

    def forward(self, src, trg=None, teacher_forcing_ratio=0.5):
        max_len = trg.size(1) if trg is not None else src.size(1)
        encoder_output, hidden = self.encoder(src)
        encoder_output = ops.sum_halves(encoder_output)
        hidden = hidden[: self.decoder.n_layers]
        tf = ops.teacher_forcing_mask(max_len, teacher_forcing_ratio) if trg is not None else None
        outputs, _, _ = ops.att_decode(encoder_output, hidden[-1], *self.decoder.weights(), trg=trg, tf_mask=tf, L=max_len)
        return outputs
