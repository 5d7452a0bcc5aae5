#!/usr/bin/env python3
"""Pre-train the audio BiGRU on AudioSet from a dataset folder (stage 2 of the reference's workflow): the reference's
pretrain_audioset.py (its flags, `pretrain_audioset.py:41-49`, on top of `AudioSet.add_model_specific_args`) on the Lightning-free loop of
m3t/trainer.py and the epoch feed of m3t/audioset.py.

    python pretrain_audioset.py --dataset_path /data/AudioSet_16k --window 32 --batch_size 128
    python -m m3t.checkpoints merge audioset/best.ckpt video_checkpoint.pt fused_av.pt

  * the four seeds (`pretrain_audioset.py:18-21`); `--checkpoint` restores model, optimizer and schedule through Trainer.load_checkpoint;
  * Trainer.from_hparams(model, hparams, gradient_clip_val=1.0); `--max_nb_epochs` epochs of fit over the train feed; after every epoch the
    val feed goes through Trainer.validate, and end_epoch keeps `<checkpoint_path>/best.ckpt` by the best val_loss;
  * `--dataset_path` holds class_labels_indices.csv, balanced_train_segments.csv, eval_segments.csv and the two folders of 16 kHz, 16-bit,
    mono .wav clips of the same names; both splits are uploaded to the device once, before the first step;
  * `--convert_audio` takes the folder as the reference's loader does: clips of any rate, channel count and sample kind (m3t/wav.py's wider
    reader), down-mixed and resampled to 16 kHz on the device when the store is built (m3t.audio.decode_waves); without it such a clip is refused;
  * `--eval_on_device` sends the epoch's validation through Trainer.evaluate_cls (m3t/cls_evaluate.py): the epoch line also gives mean average
    precision, mean ROC-AUC and d' over the classes, scored on the device; `best.ckpt` is still chosen by val_loss.  Without it nothing changes;
  * `--spec_augment` masks every training clip's dB spectrogram with the reference's own `spec_augment` (`audioset_dataset.py:17-55`;
    `--freq_mask_para` / `--time_mask_para`, default 20, `--freq_mask_num` / `--time_mask_num`, default 1, at most 4), and `--mixup_alpha A`
    mixes each training batch with a permutation of itself, weights from Beta(A, A), audio and labels alike; both run inside the ingest's
    own launches and never touch validation;
  * `--gpus` / `--nodes` are accepted and ignored: start one process per GPU with torchrun and pass `--distributed`; the world is torchrun's;
  * `--workers` is accepted and ignored: there is no host-side decoding left to spread;
  * `--test_lr` (the LR range finder) is out of scope and raises.
"""
import os
import random
import sys
from argparse import SUPPRESS, ArgumentParser

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from models.audioset_model import AudioSet  # noqa: E402
from train import join_world  # noqa: E402


def make_parser():
    parser = ArgumentParser(add_help=False)
    parser.add_argument('--gpus', type=str, default='2')
    parser.add_argument('--nodes', type=int, default=1)
    parser.add_argument('--seed', type=int, default=12345)
    parser.add_argument('--checkpoint', type=str, default='')
    parser.add_argument('--convert_audio', action='store_true', default=SUPPRESS)    # (absent unless given: the reference has no such flag)
    parser.add_argument('--eval_on_device', action='store_true', default=SUPPRESS)   # (absent unless given, as --convert_audio)
    # training-time augmentation of the train feed (m3t/audioset.py); every flag absent unless given: no flag, no change
    parser.add_argument('--spec_augment', action='store_true', default=SUPPRESS)
    parser.add_argument('--freq_mask_para', type=float, default=SUPPRESS)
    parser.add_argument('--time_mask_para', type=float, default=SUPPRESS)
    parser.add_argument('--freq_mask_num', type=int, default=SUPPRESS)
    parser.add_argument('--time_mask_num', type=int, default=SUPPRESS)
    parser.add_argument('--mixup_alpha', type=float, default=SUPPRESS)
    return AudioSet.add_model_specific_args(parser)


def main(hparams):
    from m3t.trainer import Trainer
    if hparams.test_lr:
        raise NotImplementedError("LR range finder (models/lr_finder.py) is out of scope")
    random.seed(hparams.seed)
    torch.manual_seed(hparams.seed)
    torch.cuda.manual_seed(hparams.seed)
    np.random.seed(hparams.seed)
    pg = join_world(hparams)

    model = AudioSet(hparams).to(torch.device('cuda', torch.cuda.current_device()))
    trainer = Trainer.from_hparams(model, hparams, gradient_clip_val=1.0, process_group=pg)
    if hparams.checkpoint:
        trainer.load_checkpoint(hparams.checkpoint)
        print('Restored %s (epoch %d, step %d)' % (hparams.checkpoint, trainer.epoch, trainer.global_step))

    train_feed, val_feed = model.train_dataloader(), model.val_dataloader()
    for feed in (train_feed, val_feed):
        feed.build_store()
        print('Loaded partition {}: {} samples'.format(feed.split, len(feed.files)))        # (the reference's line, audioset_dataset.py:121)
        print('  %.1f MB of PCM and labels resident on the device' % (feed.store.nbytes / 1e6))
    while trainer.epoch < hparams.max_nb_epochs:
        epoch = trainer.epoch
        train_feed.set_epoch(epoch)
        val_feed.set_epoch(epoch)
        best = trainer.best_val_loss
        on_device = bool(getattr(hparams, 'eval_on_device', False))
        trainer.fit(train_feed, val_batches=val_feed, max_epochs=1,     # (validate and end_epoch are fit's own)
                    val_fn=trainer.evaluate_cls if on_device else None)
        if trainer.rank == 0:
            ranking = ''
            if on_device:
                m = trainer.last_eval.metrics
                ranking = ", mAP %.4f, AUC %.4f, d' %.3f" % (m['val_map'], m['val_auc'], m['val_dprime'])
            print('epoch %d: lr %.3g, best val_loss %.6f%s%s' % (epoch, trainer.lr, trainer.best_val_loss,
                                                                 ' (improved)' if trainer.best_val_loss < best else '', ranking), flush=True)


if __name__ == '__main__':
    main(make_parser().parse_args())
