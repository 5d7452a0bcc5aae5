#!/usr/bin/env python3
"""Train AffWild2VA from a dataset folder: the reference's train.py (its flags, `train.py:45-59`, on top of
`AffWild2VA.add_model_specific_args`) on the Lightning-free loop of m3t/trainer.py and the epoch feed of m3t/feed.py.

    python train.py --dataset_path /data/Aff-Wild2 --modality audiovisual --fusion_type attention --window 64 --batch_size 8 --cutout

  * the four seeds (`train.py:18-21`); `--fusion_checkpoint` is loaded with strict=False, `--checkpoint` restores model, optimizer and
    schedule through Trainer.load_checkpoint;
  * Trainer.from_hparams(model, hparams, gradient_clip_val=1.0); `--max_nb_epochs` epochs of fit over the train feed; after every epoch the
    val feed goes through Trainer.validate -- or, with `--eval_on_device`, through Trainer.evaluate (no read-back per batch) -- and
    end_epoch keeps `<checkpoint_path>/best.ckpt` by the best val_loss;
  * `--splits_dir`: where frames_fps.csv, {train,val,test}.csv and expr.csv lie (the reference reads ./splits);
  * `--gpus` / `--nodes` are accepted and ignored: start one process per GPU with torchrun and pass `--distributed`; the world is torchrun's;
  * `--test_lr` (the LR range finder) is out of scope and raises.
"""
import os
import random
import sys
from argparse import ArgumentParser

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from models.model import AffWild2VA  # noqa: E402


def add_driver_args(parser):
    parser.add_argument('--gpus', type=str, default='2')
    parser.add_argument('--nodes', type=int, default=1)
    parser.add_argument('--checkpoint', type=str, default='')
    parser.add_argument('--splits_dir', type=str, default='splits')
    parser.add_argument('--eval_on_device', action='store_true', default=False)
    return parser


def join_world(hparams):
    """the process group torchrun describes (under --distributed), or None"""
    print('--gpus / --nodes are ignored: the world is torchrun\'s (one process per GPU, --distributed)')
    if hparams.distributed and int(os.environ.get('WORLD_SIZE', '1')) > 1:
        import torch.distributed as dist
        local = int(os.environ.get('LOCAL_RANK', '0'))
        torch.cuda.set_device(local)
        dist.init_process_group('nccl', device_id=torch.device('cuda', local))
        return dist.group.WORLD
    return None


def main(hparams):
    from m3t.trainer import Trainer
    if hparams.test_lr:
        raise NotImplementedError("LR range finder (models/lr_finder.py) is out of scope")
    random.seed(hparams.seed)
    torch.manual_seed(hparams.seed)
    torch.cuda.manual_seed(hparams.seed)
    np.random.seed(hparams.seed)
    pg = join_world(hparams)

    model = AffWild2VA(hparams)
    if hparams.fusion_checkpoint:
        checkpoint = torch.load(hparams.fusion_checkpoint, map_location='cpu')
        model.load_state_dict(checkpoint['state_dict'], strict=False)
        print('Loaded pretrained weights for individual streams')
    model = model.to(torch.device('cuda', torch.cuda.current_device()))
    trainer = Trainer.from_hparams(model, hparams, gradient_clip_val=1.0, process_group=pg)
    if hparams.checkpoint and not hparams.fusion_checkpoint:
        trainer.load_checkpoint(hparams.checkpoint)
        print('Restored %s (epoch %d, step %d)' % (hparams.checkpoint, trainer.epoch, trainer.global_step))

    train_feed, val_feed = model.train_dataloader(), model.val_dataloader()
    print('Loaded partition train: %d files, %d windows' % (len(train_feed.names), len(train_feed.sample_src)))
    print('Loaded partition val: %d files, %d windows' % (len(val_feed.names), len(val_feed.sample_src)))
    while trainer.epoch < hparams.max_nb_epochs:
        epoch = trainer.epoch
        train_feed.set_epoch(epoch)
        val_feed.set_epoch(epoch)
        best = trainer.best_val_loss
        if hparams.eval_on_device:
            _one_epoch(trainer, train_feed)
            trainer.end_epoch(float(trainer.evaluate(val_feed)['val_loss']))
        else:
            trainer.fit(train_feed, val_batches=val_feed, max_epochs=1)     # (validate and end_epoch are fit's own)
        if trainer.rank == 0:
            print('epoch %d: lr %.3g, best val_loss %.6f%s' % (epoch, trainer.lr, trainer.best_val_loss,
                                                               ' (improved)' if trainer.best_val_loss < best else ''), flush=True)


def _one_epoch(trainer, feed):
    """fit()'s hot loop for one epoch without its validate / end_epoch: under --eval_on_device the epoch is scored by Trainer.evaluate"""
    import gc
    for batch in feed:
        trainer.step(batch)
        if trainer.global_step == 1 and trainer.freeze_gc:
            gc.collect()
            gc.freeze()
    trainer.ddp.agree_on_scan_error()


if __name__ == '__main__':
    parser = ArgumentParser(add_help=False)
    add_driver_args(parser)
    parser.add_argument('--seed', type=int, default=12345)
    parser.add_argument('--fusion_checkpoint', type=str, default='')
    parser = AffWild2VA.add_model_specific_args(parser)
    main(parser.parse_args())
