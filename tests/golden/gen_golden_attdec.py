#!/usr/bin/env python3
"""Generate tests/golden/attdec_*.npz: the reference's attention encoder-decoder (--fusion_type att_dec; models/rnn.py:84-165,
models/model.py:96-97,119-126) run by the REFERENCE itself, imported read-only, on CPU.  Like gen_golden.py it runs only in the
build container; the fixtures are data (inputs, outputs, gradients or their digests; weights come from the frozen recipe seed).

The decoder cases run in float64 (model.double()): the target is then the exact recurrence, and the tests' bars measure the
HIP path's fp32 error alone.  The AffWild2VA case runs in float32 like the other C5 fixtures.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_attdec.py
"""
import os
import random
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import gen_golden as G                                       # noqa: E402  (sets up the reference import path and stubs)
from models import rnn as ref_rnn                            # noqa: E402  (reference)
from models.rnn import AttEncDec, Decoder, Attention          # noqa: E402
from recipe import fill_module, draw, grad_digest             # noqa: E402

save, hp = G.save, G.hp
_ORIG_RANDOM = random.random


def _grads(m, digest):
    """every gradient as a digest ("gd."); with digest=False the decoder's vectors also in full as float32 ("g.")"""
    out = {}
    for n, p in m.named_parameters():
        if p.grad is None:
            continue
        g = p.grad.detach().double().numpy()
        out["gd." + n] = grad_digest(g)
        if not digest and not n.startswith("encoder.") and g.size <= 4096:
            out["g." + n] = g.astype(np.float32)
    return out


def _recording_random(log):
    """wraps the reference module's `random.random` so the draws of a forward are recorded (order and value)"""
    orig = random.random

    def rec():
        x = orig()
        log.append(x)
        return x
    return rec


def case_encdec(name, seed, B, T, digest, trg_seed=None, ratio=0.5):
    rs = np.random.RandomState(seed)
    m = fill_module(AttEncDec(), seed + 1).double()
    src = torch.from_numpy(draw(rs, (B, T, 1024))).double().requires_grad_(True)
    trg = None
    if trg_seed is not None:
        trg = torch.from_numpy(draw(rs, (B, T, 2), "uniform_pm1")).double()
    ct = torch.from_numpy(draw(rs, (B, T, 2))).double()
    draws = []
    if trg is not None:
        random.seed(trg_seed)
        ref_rnn.random.random = _recording_random(draws)
    try:
        y = m(src, trg, ratio) if trg is not None else m(src)
    finally:
        ref_rnn.random.random = _ORIG_RANDOM
    (y * ct).sum().backward()
    extra = {}
    if trg is not None:
        extra = dict(trg=trg.numpy().astype(np.float32), trg_seed=np.array(trg_seed), ratio=np.array(ratio),
                     draws=np.array(draws), tf=np.array([0] + [int(d < ratio) for d in draws], np.int32))
    dx = src.grad.numpy()
    save(name, seed=np.array(seed), dims=np.array([B, T]), y=y.detach().numpy(), ct=ct.numpy().astype(np.float32),
         dx=grad_digest(dx) if digest else dx, **_grads(m, digest), **extra)


def case_small_decoder(name, seed, B=3, T=7, H=64):
    """Decoder(2, H, 2, 1) and Attention(H) single steps: everything stored"""
    rs = np.random.RandomState(seed)
    dec = fill_module(Decoder(2, H, 2, 1), seed + 1).double()
    inp = torch.from_numpy(draw(rs, (B, 2))).double().requires_grad_(True)
    hid = torch.from_numpy(0.5 * draw(rs, (1, B, H))).double().requires_grad_(True)
    enc = torch.from_numpy(draw(rs, (B, T, H))).double().requires_grad_(True)
    out, h, aw = dec(inp, hid, enc)
    c_out, c_h, c_aw = (torch.from_numpy(draw(rs, tuple(t.shape))).double() for t in (out, h, aw))
    ((out * c_out).sum() + (h * c_h).sum() + (aw * c_aw).sum()).backward()
    arrs = dict(inp=inp.detach().numpy(), hid=hid.detach().numpy(), enc=enc.detach().numpy(), out=out.detach().numpy(),
                h=h.detach().numpy(), aw=aw.detach().numpy(), c_out=c_out.numpy(), c_h=c_h.numpy(), c_aw=c_aw.numpy(),
                d_inp=inp.grad.numpy(), d_hid=hid.grad.numpy(), d_enc=enc.grad.numpy())
    arrs.update({"p." + n: p.detach().numpy() for n, p in dec.named_parameters()})
    arrs.update(_grads(dec, False))
    att = fill_module(Attention(H), seed + 2).double()
    hid2 = torch.from_numpy(draw(rs, (B, H))).double().requires_grad_(True)
    enc2 = torch.from_numpy(draw(rs, (B, T, H))).double().requires_grad_(True)
    w = att(hid2, enc2)
    c_w = torch.from_numpy(draw(rs, tuple(w.shape))).double()
    (w * c_w).sum().backward()
    arrs.update({"att.hid": hid2.detach().numpy(), "att.enc": enc2.detach().numpy(), "att.w": w.detach().numpy(),
                 "att.c_w": c_w.numpy(), "att.d_hid": hid2.grad.numpy(), "att.d_enc": enc2.grad.numpy()})
    arrs.update({"att.p." + n: p.detach().numpy() for n, p in att.named_parameters()})
    arrs.update({"att.g." + n: p.grad.numpy() for n, p in att.named_parameters()})
    save(name, seed=np.array(seed), dims=np.array([B, T, H]), **arrs)


def case_affwild_att_dec(name, seed, B=2, T=16):
    """AffWild2VA(audiovisual, v2p_split, att_dec, ccc) training_step in train mode: the reference's batch has no 'valence' /
    'arousal' keys, so its decoder runs greedy (model.py:121)"""
    rs = np.random.RandomState(seed)
    m = fill_module(G.AffWild2VA(hp(modality="audiovisual", backbone="v2p_split", fusion_type="att_dec", loss="ccc", window=T)),
                    seed + 1).train()
    batch = {
        "video": torch.from_numpy(rs.randint(0, 256, (B, 3, T, 112, 112)).astype(np.float32)),
        "se_features": torch.from_numpy(draw(rs, (B, 512, T))),
        "audio": torch.from_numpy(draw(rs, (B, T, 200))),
        "label_valence": torch.from_numpy(draw(rs, (B, T), "uniform_pm1")),
        "label_arousal": torch.from_numpy(draw(rs, (B, T), "uniform_pm1")),
    }
    ys = {}
    fwd = m.forward

    def tap(b):
        o = fwd(b)
        ys["y"] = o.detach().numpy().copy()
        return o
    m.forward = tap
    out = m.training_step(batch, 0)
    del m.forward
    out["loss"].backward()
    sd = m.state_dict()
    save(name, seed=np.array(seed), dims=np.array([B, T]), y=ys["y"], loss=out["loss"].detach().numpy(),
         keys=np.array(list(sd.keys())), shapes=np.array([",".join(map(str, v.shape)) for v in sd.values()]), **_grads(m, True))


def case_init(name):
    """initial weights under torch.manual_seed(12345) (the reference's default --seed) as digests, and the state_dict contract"""
    out = {}
    for tag, ctor in {"encdec": AttEncDec, "dec64": lambda: Decoder(2, 64, 2, 1), "att64": lambda: Attention(64)}.items():
        torch.manual_seed(12345)
        m = ctor()
        for n, p in m.state_dict().items():
            out["%s.%s" % (tag, n)] = grad_digest(p.detach().numpy())
        out["%s.keys" % tag] = np.array(list(m.state_dict().keys()))
        out["%s.shapes" % tag] = np.array([",".join(map(str, v.shape)) for v in m.state_dict().values()])
    # teacher-forcing draws: random.seed(k), one random.random() per step of an L-frame target, as AttEncDec.forward makes them
    for k in (0, 7):
        draws = []
        random.seed(k)
        ref_rnn.random.random = _recording_random(draws)
        try:
            m = AttEncDec()
            with torch.no_grad():
                m(torch.zeros(1, 5, 1024), torch.zeros(1, 9, 2), 0.5)
        finally:
            ref_rnn.random.random = _ORIG_RANDOM
        out["tf_draws.%d" % k] = np.array(draws)
    save(name, **out)


def main():
    torch.set_num_threads(8)
    case_init("attdec_init")
    case_small_decoder("attdec_small_h64", 1200)
    case_encdec("attdec_b2_t12", 1210, 2, 12, digest=False)
    case_encdec("attdec_b2_t12_tf", 1220, 2, 12, digest=False, trg_seed=5)
    case_encdec("attdec_b2_t300", 1230, 2, 300, digest=True)
    case_affwild_att_dec("attdec_affwild_t16_train", 1240)


if __name__ == "__main__":
    main()
