"""att_dec on the MI355X: the HIP attention decoder (csrc/attdec.hip via m3t.ops.att_decode) against the reference's own outputs
and gradients (tests/golden/attdec_*.npz, float64 runs of the reference written by gen_golden_attdec.py) and against an fp64
restatement of the decoder equations written here.

Bars: outputs 1e-4 absolute; gradients 2e-4 relative to the largest entry of the reference gradient (a digest's entries: to its
L2 norm).  The recurrence is fp32 over up to 299 fed-back steps."""
import argparse
import random

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _encdec(seed):
    from models.rnn import AttEncDec
    from golden.recipe import fill_module
    return fill_module(AttEncDec(), seed + 1).to(DEV)


def _inputs(g, with_trg=False):
    from golden.recipe import draw
    B, T = (int(x) for x in g["dims"])
    rs = np.random.RandomState(int(g["seed"]))
    src = torch.from_numpy(draw(rs, (B, T, 1024))).to(DEV).requires_grad_(True)
    trg = torch.from_numpy(draw(rs, (B, T, 2), "uniform_pm1")).to(DEV) if with_trg else None
    return src, trg, torch.from_numpy(g["ct"]).to(DEV)


def _check_grad(name, got, ref, tol=2e-4):
    got = np.asarray(got, np.float64)
    scale = max(float(np.abs(ref).max()), 1e-6)
    err = float(np.abs(got - ref).max()) / scale
    assert err <= tol, "%s: relative error %.2e" % (name, err)


def _check_digest(name, got, ref, tol=2e-4):
    """digest = (L2 norm, sum, first 8 entries): every entry to tol of the norm, except the sum of n entries, whose error is
    bounded by sqrt(n) times the L2 norm of the error (Cauchy-Schwarz): tol * sqrt(n) of the norm"""
    from golden.recipe import grad_digest
    d = grad_digest(got)
    scale = np.full(d.shape, max(float(ref[0]), 1e-6))
    scale[1] *= np.sqrt(np.asarray(got).size)
    err = float((np.abs(d - ref) / scale).max())
    assert err <= tol, "%s: digest error %.2e of the norm" % (name, err)


def _run_golden(name, with_trg):
    g = load_golden(name)
    m = _encdec(int(g["seed"]))
    src, trg, ct = _inputs(g, with_trg)
    if with_trg:
        random.seed(int(g["trg_seed"]))
        y = m(src, trg, float(g["ratio"]))
    else:
        y = m(src)
    (y * ct).sum().backward()
    torch.cuda.synchronize()
    e_y = float(np.abs(y.detach().cpu().numpy() - g["y"]).max())
    assert e_y <= 1e-4, "outputs: %.2e" % e_y
    for n, p in m.named_parameters():
        gr = p.grad.cpu().numpy()
        _check_digest(n, gr, g["gd." + n])
        if "g." + n in g:
            _check_grad(n, gr, g["g." + n])
    if g["dx"].ndim == 1:
        _check_digest("src", src.grad.cpu().numpy(), g["dx"])
    else:
        _check_grad("src", src.grad.cpu().numpy(), g["dx"])
    return m, y


def test_encdec_b2_t12_matches_reference():
    _run_golden("attdec_b2_t12", False)


def test_encdec_teacher_forcing_matches_reference():
    from m3t import ops
    g = load_golden("attdec_b2_t12_tf")
    random.seed(int(g["trg_seed"]))
    assert ops.teacher_forcing_mask(int(g["dims"][1]), float(g["ratio"])) == list(g["tf"])
    assert 0 < int(g["tf"].sum()) < len(g["tf"]) - 1          # both kinds of step occur
    _run_golden("attdec_b2_t12_tf", True)


def test_encdec_b2_t300_matches_reference():
    _run_golden("attdec_b2_t300", False)


def test_small_decoder_and_attention_single_step():
    from models.rnn import Decoder, Attention
    g = load_golden("attdec_small_h64")
    B, T, H = (int(x) for x in g["dims"])
    t = lambda k: torch.from_numpy(np.ascontiguousarray(g[k]).astype(np.float32)).to(DEV)      # noqa: E731
    dec = Decoder(2, H, 2, 1).to(DEV)
    with torch.no_grad():
        for n, p in dec.named_parameters():
            p.copy_(t("p." + n))
    inp, hid, enc = (t(k).requires_grad_(True) for k in ("inp", "hid", "enc"))
    out, h, aw = dec(inp, hid, enc)
    assert out.shape == (B, 2) and h.shape == (1, B, H) and aw.shape == (B, 1, T)
    ((out * t("c_out")).sum() + (h * t("c_h")).sum() + (aw * t("c_aw")).sum()).backward()
    for k, v in (("out", out), ("h", h), ("aw", aw)):
        assert float(np.abs(v.detach().cpu().numpy() - g[k]).max()) <= 1e-5, k
    for k, v in (("d_inp", inp), ("d_hid", hid), ("d_enc", enc)):
        _check_grad(k, v.grad.cpu().numpy(), g[k])
    for n, p in dec.named_parameters():
        _check_digest(n, p.grad.cpu().numpy(), g["gd." + n])
    att = Attention(H).to(DEV)
    with torch.no_grad():
        for n, p in att.named_parameters():
            p.copy_(t("att.p." + n))
    hid2, enc2 = t("att.hid").requires_grad_(True), t("att.enc").requires_grad_(True)
    w = att(hid2, enc2)
    (w * t("att.c_w")).sum().backward()
    assert float(np.abs(w.detach().cpu().numpy() - g["att.w"]).max()) <= 1e-5
    _check_grad("att.d_hid", hid2.grad.cpu().numpy(), g["att.d_hid"])
    _check_grad("att.d_enc", enc2.grad.cpu().numpy(), g["att.d_enc"])
    for n, p in att.named_parameters():
        _check_grad("att." + n, p.grad.cpu().numpy(), g["att.g." + n])


def _decoder_h64(seed):
    from models.rnn import Decoder
    from golden.recipe import fill_module
    return fill_module(Decoder(2, 64, 2, 1), seed).to(DEV)


def _decode(dec, enc, h0, **kw):
    from m3t import ops
    return ops.att_decode(enc, h0, *dec.weights(), **kw)


def test_t1_is_all_zero_without_graph_and_t2():
    m = _encdec(3)
    src = torch.randn(2, 1, 1024, device=DEV, requires_grad=True)
    y = m(src)
    assert y.shape == (2, 1, 2) and not y.requires_grad and float(y.abs().max()) == 0.0
    # T = 2: one decoder step, against the fp64 restatement
    dec = _decoder_h64(11)
    enc = torch.randn(3, 2, 64, device=DEV)
    h0 = 0.5 * torch.randn(3, 64, device=DEV)
    y, _, _ = _decode(dec, enc, h0)
    ref, _ = _restated(dec, enc, h0)
    assert float(y[:, 0].detach().abs().max()) == 0.0
    assert float((y.double().cpu() - ref.detach()).abs().max()) <= 1e-5


def _restated(dec, enc, h0, trg=None, tf=None):
    """fp64 decoder on the CPU from the equations: a = W_ah h, s = v.relu(P + a), alpha = softmax(s), c = alpha enc,
    h = GRUCell([y_in, c], h), y = W_o [h, c] + b_o; y_in of the next step = trg[:, t] where tf[t] else y"""
    ps = {n: p.detach().double().cpu().requires_grad_(True) for n, p in dec.named_parameters()}
    enc = enc.detach().double().cpu().requires_grad_(True)
    h = h0.detach().double().cpu().requires_grad_(True)
    inputs = (enc, h)
    B, T, H = enc.shape
    W_a, b_a, v = ps["attention.attn.weight"], ps["attention.attn.bias"], ps["attention.v"]
    W_ih, W_hh, b_ih, b_hh = ps["gru.weight_ih_l0"], ps["gru.weight_hh_l0"], ps["gru.bias_ih_l0"], ps["gru.bias_hh_l0"]
    W_o, b_o = ps["out.weight"], ps["out.bias"]
    P = enc @ W_a[:, H:].T + b_a
    y_in = torch.zeros(B, 2, dtype=torch.float64)
    outs = [torch.zeros(B, 2, dtype=torch.float64)]
    for t in range(1, T):
        a = h @ W_a[:, :H].T
        s = (torch.relu(P + a[:, None, :]) * v).sum(-1)
        alpha = torch.softmax(s, dim=1)
        c = (alpha[:, :, None] * enc).sum(1)
        gi = torch.cat([y_in, c], 1) @ W_ih.T + b_ih
        gh = h @ W_hh.T + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * h
        y = torch.cat([h, c], 1) @ W_o.T + b_o
        outs.append(y)
        y_in = trg[:, t].double().cpu() if (tf is not None and tf[t]) else y
    return torch.stack(outs, 1), (ps, inputs)


def test_b5_t300_against_fp64_restatement():
    dec = _decoder_h64(21)
    torch.manual_seed(5)
    B, T, H = 5, 300, 64
    enc = torch.randn(B, T, H, device=DEV, requires_grad=True)
    h0 = (0.5 * torch.randn(B, H, device=DEV)).requires_grad_(True)
    ct = torch.randn(B, T, 2, device=DEV)
    y, _, _ = _decode(dec, enc, h0)
    (y * ct).sum().backward()
    ref, (ps, (enc64, h64)) = _restated(dec, enc, h0)
    (ref * ct.double().cpu()).sum().backward()
    e_y = float((y.detach().double().cpu() - ref.detach()).abs().max())
    assert e_y <= 1e-4, "outputs %.2e" % e_y
    for n, p in dec.named_parameters():
        _check_grad(n, p.grad.cpu().numpy(), ps[n].grad.numpy())
    _check_grad("enc", enc.grad.cpu().numpy(), enc64.grad.numpy())
    _check_grad("h0", h0.grad.cpu().numpy(), h64.grad.numpy())


def test_teacher_forcing_against_fp64_restatement():
    from m3t import ops
    dec = _decoder_h64(31)
    torch.manual_seed(6)
    B, T, H = 3, 40, 64
    enc = torch.randn(B, T, H, device=DEV, requires_grad=True)
    h0 = (0.5 * torch.randn(B, H, device=DEV)).requires_grad_(True)
    trg = torch.rand(B, T, 2, device=DEV) * 2 - 1
    ct = torch.randn(B, T, 2, device=DEV)
    random.seed(3)
    tf = ops.teacher_forcing_mask(T, 0.5)
    y, _, _ = _decode(dec, enc, h0, trg=trg, tf_mask=tf)
    (y * ct).sum().backward()
    ref, (ps, (enc64, h64)) = _restated(dec, enc, h0, trg, tf)
    (ref * ct.double().cpu()).sum().backward()
    assert float((y.detach().double().cpu() - ref.detach()).abs().max()) <= 1e-4
    for n, p in dec.named_parameters():
        _check_grad(n, p.grad.cpu().numpy(), ps[n].grad.numpy())
    _check_grad("enc", enc.grad.cpu().numpy(), enc64.grad.numpy())
    _check_grad("h0", h0.grad.cpu().numpy(), h64.grad.numpy())


def test_no_grad_equals_train_and_runs_are_bit_identical():
    dec = _decoder_h64(41)
    torch.manual_seed(7)
    enc = torch.randn(4, 50, 64, device=DEV, requires_grad=True)
    h0 = torch.randn(4, 64, device=DEV).tanh()
    ct = torch.randn(4, 50, 2, device=DEV)
    with torch.no_grad():
        y_ng, _, _ = _decode(dec, enc, h0)
    runs = []
    for _ in range(2):
        dec.zero_grad(set_to_none=True)
        enc.grad = None
        y, _, _ = _decode(dec, enc, h0)
        (y * ct).sum().backward()
        runs.append([y.detach().clone(), enc.grad.clone()] + [p.grad.clone() for p in dec.parameters()])
    assert torch.equal(y_ng, runs[0][0])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _hp(**kw):
    from models.model import AffWild2VA
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    for k, v in kw.items():
        setattr(ns, k, v)
    return ns


def _affwild_batch(g):
    from golden.recipe import draw
    B, T = (int(x) for x in g["dims"])
    rs = np.random.RandomState(int(g["seed"]))
    f = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
    return {"video": f(rs.randint(0, 256, (B, 3, T, 112, 112)).astype(np.float32)), "se_features": f(draw(rs, (B, 512, T))),
            "audio": f(draw(rs, (B, T, 200))), "label_valence": f(draw(rs, (B, T), "uniform_pm1")),
            "label_arousal": f(draw(rs, (B, T), "uniform_pm1"))}


def test_affwild_att_dec_training_step_matches_reference():
    from models.model import AffWild2VA
    from golden.recipe import fill_module
    g = load_golden("attdec_affwild_t16_train")
    m = fill_module(AffWild2VA(_hp(modality="audiovisual", backbone="v2p_split", fusion_type="att_dec", loss="ccc", window=16)),
                    int(g["seed"]) + 1).to(DEV).train()
    batch = _affwild_batch(g)
    ys = {}
    fwd = m.forward

    def tap(b):
        o = fwd(b)
        ys["y"] = o.detach().cpu().numpy()
        return o
    m.forward = tap
    out = m.training_step(batch, 0)
    del m.forward
    out["loss"].backward()
    torch.cuda.synchronize()
    assert ys["y"].shape == g["y"].shape
    e_y = float(np.abs(ys["y"] - g["y"]).max())
    assert e_y <= 1e-4, "outputs %.2e" % e_y
    assert abs(float(out["loss"]) - float(g["loss"])) <= 1e-4
    # the whole model in fp32 on both sides: digests compared as the C5 golden tests do (test_gpu_parity.check_digests: absolute with a
    # floor of 1, norm and first entries) -- the conv biases in front of BatchNorm have gradients that are zero up to rounding
    from golden.recipe import grad_digest
    for n, p in m.named_parameters():
        ref, got = g["gd." + n], grad_digest(p.grad.cpu().numpy())
        assert abs(got[0] - ref[0]) <= 1e-3 * max(1.0, ref[0]), (n, got[0], ref[0])
        assert float(np.abs(got[2:] - ref[2:]).max()) <= 1e-3 * max(1.0, float(np.abs(ref[2:]).max())), n


def test_trainer_step_with_flat_grad_clip():
    from models.model import AffWild2VA
    from m3t.trainer import Trainer
    g = load_golden("attdec_affwild_t16_train")
    torch.manual_seed(12345)
    model = AffWild2VA(_hp(modality="audiovisual", backbone="v2p_split", fusion_type="att_dec", loss="ccc", window=16,
                           learning_rate=1e-4)).to(DEV)
    tr = Trainer.from_hparams(model, model.hparams)
    before = {n: p.detach().clone() for n, p in model.fusion.decoder.named_parameters()}
    out = tr.step(_affwild_batch(g))
    torch.cuda.synchronize()
    assert np.isfinite(float(out["loss"])) and np.isfinite(float(out["grad_norm"])) and float(out["grad_norm"]) > 0
    moved = [n for n, p in model.fusion.decoder.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert len(moved) == len(before), "every decoder parameter takes the optimizer step"
