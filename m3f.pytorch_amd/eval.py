#!/usr/bin/env python3
"""Test AffWild2VA from a dataset folder: the reference's eval.py (its flags, `eval.py:26-36`, on top of
`AffWild2VA.add_model_specific_args`).  `--checkpoint` is loaded strictly from its 'state_dict'; the test feed (m3t/feed.py; the val feed
at half-window stride under `--test_on_val`) goes through Trainer.evaluate(test=True), which overlap-adds the windows on the device and
writes predictions_test.pt (predictions_val.pt and the metrics under `--test_on_val`) into the directory it runs in.

    python eval.py --checkpoint best.ckpt --dataset_path /data/Aff-Wild2 --modality audiovisual --fusion_type attention --window 64 --batch_size 8
"""
import os
import sys
from argparse import ArgumentParser

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from models.model import AffWild2VA  # noqa: E402
from train import add_driver_args, join_world  # noqa: E402


def main(hparams):
    from m3t.trainer import Trainer
    pg = join_world(hparams)
    model = AffWild2VA(hparams)
    checkpoint = torch.load(hparams.checkpoint, map_location='cpu')
    model.load_state_dict(checkpoint['state_dict'])
    print('Loaded pretrained weights')
    model = model.to(torch.device('cuda', torch.cuda.current_device()))
    trainer = Trainer.from_hparams(model, hparams, gradient_clip_val=1.0, process_group=pg, checkpoint_path=None)
    res = trainer.evaluate(model.test_dataloader(), test=True)
    if res:
        print({k: float(v) for k, v in res['log'].items()}, flush=True)


if __name__ == '__main__':
    parser = ArgumentParser(add_help=False)
    add_driver_args(parser)
    parser = AffWild2VA.add_model_specific_args(parser)
    main(parser.parse_args())
