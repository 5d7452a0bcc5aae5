"""att_dec on the host side (no GPU): the module contract of models/rnn.py's Attention / Decoder / AttEncDec against the reference
(tests/golden/attdec_init.npz, written by gen_golden_attdec.py) and the teacher-forcing draws of m3t.ops.teacher_forcing_mask."""
import argparse
import random

import numpy as np
import pytest
import torch

from conftest import load_golden


def _ctors():
    from models.rnn import AttEncDec, Decoder, Attention
    return {"encdec": AttEncDec, "dec64": lambda: Decoder(2, 64, 2, 1), "att64": lambda: Attention(64)}


def test_state_dict_keys_and_shapes_match_reference():
    g = load_golden("attdec_init")
    for tag, ctor in _ctors().items():
        sd = ctor().state_dict()
        assert list(sd.keys()) == list(g["%s.keys" % tag]), tag
        assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["%s.shapes" % tag]), tag


def test_init_digests_match_reference_rng_order():
    from golden.recipe import grad_digest
    g = load_golden("attdec_init")
    for tag, ctor in _ctors().items():
        torch.manual_seed(12345)
        m = ctor()
        for n, p in m.state_dict().items():
            # per-gate orthogonal weight_hh of the encoder: LAPACK QR rounding depends on the host BLAS (see test_host_api.py)
            atol = 4e-6 if "weight_hh" in n and n.startswith("encoder") else 1e-7
            np.testing.assert_allclose(grad_digest(p.detach().numpy()), g["%s.%s" % (tag, n)], rtol=1e-6, atol=atol,
                                       err_msg="%s.%s" % (tag, n))


@pytest.mark.parametrize("seed", [0, 7])
def test_teacher_forcing_mask_follows_reference_draws(seed):
    from m3t import ops
    draws = load_golden("attdec_init")["tf_draws.%d" % seed]
    random.seed(seed)
    mask = ops.teacher_forcing_mask(len(draws) + 1, 0.5)
    assert mask == [0] + [int(d < 0.5) for d in draws]
    random.seed(seed)
    for _ in draws:
        random.random()
    after = random.random()
    random.seed(seed)
    ops.teacher_forcing_mask(len(draws) + 1, 0.5)
    assert random.random() == after, "one draw per decoder step, no more, no less"


def test_decoder_rejects_what_the_kernels_do_not_run():
    from models.rnn import Decoder
    with pytest.raises(NotImplementedError):
        Decoder(2, 64, 2, 2)
    with pytest.raises(NotImplementedError):
        Decoder(128, 64, 2, 1)


def test_att_dec_model_builds_and_mtl_loss_is_refused():
    from models.model import AffWild2VA
    from models.rnn import AttEncDec
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    ns.modality, ns.fusion_type, ns.loss, ns.window = "audiovisual", "att_dec", "ccc_mtl", 16
    m = AffWild2VA(ns)
    assert isinstance(m.fusion, AttEncDec)
    keys = list(m.state_dict().keys())
    assert "fusion.decoder.attention.v" in keys and "fusion.encoder.gru.weight_ih_l0" in keys
    y = torch.zeros(2, 16, 2)
    batch = {"label_valence": torch.zeros(2, 16), "label_arousal": torch.zeros(2, 16), "class_expr": torch.zeros(2, 16, dtype=torch.long),
             "expr_valid": torch.ones(2, 16, dtype=torch.bool)}
    with pytest.raises(ValueError, match="att_dec"):
        m.va_objective(y, batch)


def test_affwild_att_dec_state_dict_matches_reference():
    from models.model import AffWild2VA
    g = load_golden("attdec_affwild_t16_train")
    ns = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
    ns.modality, ns.backbone, ns.fusion_type, ns.loss, ns.window = "audiovisual", "v2p_split", "att_dec", "ccc", 16
    sd = AffWild2VA(ns).state_dict()
    assert list(sd.keys()) == list(g["keys"])
    assert [",".join(map(str, v.shape)) for v in sd.values()] == list(g["shapes"])
