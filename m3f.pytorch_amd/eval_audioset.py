#!/usr/bin/env python3
"""Score an AudioSet checkpoint on the val split (eval_segments) with the figures published AudioSet results are given in: mean average
precision, mean ROC-AUC and d' over the 527 classes, computed on the device (m3t/cls_evaluate.py, Trainer.evaluate_cls).

    python eval_audioset.py --checkpoint audioset/best.ckpt --dataset_path /data/AudioSet_16k

Prints val_loss, val_acc, the three ranking figures and the classes with the lowest and highest AP (names from the folder's
class_labels_indices.csv), and writes `<out>.json` (the metrics) and `<out>.csv` (AP, AUC, P, N per class); `--out` defaults to
audioset_eval.  The model's flags are pretrain_audioset.py's (`--num_hidden`, `--num_fc_layers`, `--window`, `--batch_size` must be the
checkpoint's); `--convert_audio` as there.
"""
import os
import sys
from argparse import SUPPRESS, ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def make_parser():
    from models.audioset_model import AudioSet
    parser = ArgumentParser(add_help=False)
    parser.add_argument('--checkpoint', type=str, required=True)
    parser.add_argument('--out', type=str, default='audioset_eval')
    parser.add_argument('--top', type=int, default=10)
    parser.add_argument('--convert_audio', action='store_true', default=SUPPRESS)
    return AudioSet.add_model_specific_args(parser)


def main(hparams):
    import torch
    from m3t.trainer import Trainer
    from models.audioset_model import AudioSet
    model = AudioSet(hparams).to(torch.device('cuda', torch.cuda.current_device()))
    trainer = Trainer.from_hparams(model, hparams, gradient_clip_val=1.0, checkpoint_path=None)
    trainer.load_checkpoint(hparams.checkpoint)
    feed = model.val_dataloader().build_store()
    print('Loaded partition {}: {} samples'.format(feed.split, len(feed.files)))
    res = trainer.evaluate_cls(feed)['log']
    print('val_loss %.6f, val_acc %.4f, mAP %.4f over %d classes, AUC %.4f over %d classes, d\' %.3f'
          % (res['val_loss'], res['val_acc'], res['val_map'], res['n_classes_ap'], res['val_auc'], res['n_classes_auc'], res['val_dprime']))
    names = os.path.join(hparams.dataset_path, 'class_labels_indices.csv')
    names = names if os.path.exists(names) else None
    trainer.last_eval.report(names, top=hparams.top)
    print('wrote %s and %s' % trainer.last_eval.save(hparams.out, names))


if __name__ == '__main__':
    main(make_parser().parse_args())
