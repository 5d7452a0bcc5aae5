"""models.audioset_model -- stage 2 of the reference's workflow: pre-training the audio BiGRU on AudioSet, 527-way multi-label.

Drop-in for the reference's models/audioset_model.py:24-175 (`AudioSet`): same `hparams` namespace and `add_model_specific_args`, same
sub-module name (`audio` = GRU(200, num_hidden, 2, 527, num_fc_layers, dropout=True)) and therefore the same state_dict keys
(`audio.gru.*`, `audio.fc.0.*`, `audio.fc.3.*`), same `forward(x)` (temporal max-pooling of the per-frame logits), `bce_loss`, step and
epoch-end dicts.  The loss end runs on csrc/cls_loss.hip: `forward` pools with m3t.ops.temporal_pool, `training_step` hands the
per-frame logits [B,T,527] to ONE operator (m3t.ops.pooled_cls_loss: pooling, BCE-with-logits, top-1 statistic and dL/dz from its forward
pass); `train_acc` stays on the device (M3T_STEP_SYNC=1: a Python float).  The head's Dropout(0.5) draws its mask inside the GEMM epilogue
(models/rnn.py, `drop_seeds`), so a train-mode step has no bit-parity with the reference's torch RNG; eval mode has.
m3t/checkpoints.py carries a trained checkpoint into AffWild2VA.  `batch['audio']` may be the audio as decoded -- 16 kHz PCM, int16 [N, S] or
float32 [N, S], with the loader's draws in `batch['audio_aug']` (m3t.audio.draw_audioset) and the clips' lengths in `batch['audio_len']`:
crop, spectrogram, power_to_db and the context stack of the reference's loader (audioset_dataset.py:58-87) then run on the device
(m3t.audio.ingest) in front of the BiGRU; a float32 [N, T, 200] batch takes the reference's route.  train_dataloader / val_dataloader
return the epoch feed of m3t/audioset.py (the clips of `--dataset_path` resident on the device, batches of {'audio', 'label'} as the
reference's loader yields them); pretrain_audioset.py drives it.  Out of scope: the LR range finder.
"""
from argparse import ArgumentParser

import torch

from m3t import audio, ops
from .model import _Base, _STEP_SYNC
from .rnn import GRU
from .vox2_model import _classification_epoch_end, _configure_optimizers


class AudioSet(_Base):

    def __init__(self, hparams):
        super().__init__()
        try:
            self.hparams = hparams
        except AttributeError:      # newer Lightning: hparams is a read-only property
            self.save_hyperparameters(hparams)
        self.audio = GRU(200, hparams.num_hidden, 2, 527, hparams.num_fc_layers, dropout=True)
        self.history = {'lr': [], 'loss': []}

    def _features(self, x, aug=None, lengths=None, mix=None):
        """[N, T, 200] rows; a waveform batch (int16, or 2-D float32 [N, S]) goes through m3t.audio.ingest with hparams.window frames
        (masks in the draws and mix = batch['audio_mix'] = (partner, lam) are applied there; the labels of such a batch come mixed)"""
        if x.dtype == torch.int16 or (x.dtype == torch.float32 and x.dim() == 2):
            return audio.ingest(x, aug, self.hparams.window, lengths, mix=mix)
        return x

    def forward(self, x, aug=None, lengths=None):
        return ops.temporal_pool(self.audio(self._features(x, aug, lengths)), 'max')          # temporal max-pooling (audioset_model.py:36)

    def bce_loss(self, y_hat, y):
        return ops.cls_loss(y_hat, y, 'bce')[0]

    def training_step(self, batch, batch_idx):
        x, y = self._features(batch['audio'], batch.get('audio_aug'), batch.get('audio_len'), batch.get('audio_mix')), batch['label']
        loss, stats, _ = ops.pooled_cls_loss(self.audio(x), y, 'max', 'bce')
        # top-1 accuracy: a 0-dim device tensor (the reference: `.item()`, one host sync per step, audioset_model.py:49)
        acc = float(stats[1]) / x.size(0) if _STEP_SYNC else stats[1] / x.size(0)
        if getattr(self.hparams, 'test_lr', False):
            raise NotImplementedError("LR range finder (models/lr_finder.py) is out of scope")
        return {'loss': loss, 'progress_bar': {'loss': loss, 'train_acc': acc}, 'log': {'loss': loss, 'train_acc': acc}}

    def on_batch_end(self):
        if getattr(self.hparams, 'scheduler', None) == 'cyclic' and hasattr(self, 'cyclic_scheduler'):
            self.cyclic_scheduler.step()

    def validation_step(self, batch, batch_idx):
        with torch.no_grad():
            x = self._features(batch['audio'], batch.get('audio_aug'), batch.get('audio_len'))
            loss, _, correct = ops.pooled_cls_loss(self.audio(x), batch['label'], 'max', 'bce')
        return {'val_loss': loss, 'correct': correct}

    def eval_scores(self, batch):
        """validation_step's own call with the pooled per-clip logits kept: (pooled [N, 527], val_loss, correct [N]), the input of the
        device-side evaluation epoch (m3t/cls_evaluate.py, Trainer.evaluate_cls)"""
        with torch.no_grad():
            x = self._features(batch['audio'], batch.get('audio_aug'), batch.get('audio_len'))
            loss, _, correct, pooled, _ = ops.pooled_cls_loss(self.audio(x), batch['label'], 'max', 'bce', return_pooled=True)
        return pooled, loss, correct

    def validation_end(self, outputs):
        return _classification_epoch_end(outputs)

    def configure_optimizers(self):
        return _configure_optimizers(self, step_size_up=480)

    # ------------------------------------------------------------------ data (audioset_model.py:129-145; m3t/audioset.py)
    def _feed(self, split):
        from m3t import audioset
        rank, world = 0, 1
        if getattr(self.hparams, 'distributed', False) and torch.distributed.is_available() and torch.distributed.is_initialized():
            rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
        return audioset.feed_from_hparams(self.hparams, split, rank, world)

    def train_dataloader(self):
        return self._feed('train')

    def val_dataloader(self):
        return self._feed('val')

    @staticmethod
    def add_model_specific_args(parent_parser):
        """The reference's flags with the reference's defaults (audioset_model.py:147-175)."""
        parser = ArgumentParser(parents=[parent_parser])
        flags = [
            ('--learning_rate', 0.3, float), ('--min_lr', 1e-3, float), ('--decay_factor', 0.5, float), ('--batch_size', 128, int),
            ('--optimizer', 'adam', str), ('--scheduler', 'plateau', str), ('--num_fc_layers', 2, int), ('--num_hidden', 256, int),
            ('--window', 32, int), ('--dataset_path', '/data/f/zhangyuanhang/Aff-Wild2/AudioSet_16k', str),
            ('--checkpoint_path', './audioset', str), ('--workers', 8, int), ('--max_nb_epochs', 80, int),
        ]
        for name, default, typ in flags:
            parser.add_argument(name, default=default, type=typ)
        for name in ('--test_lr', '--distributed'):
            parser.add_argument(name, action='store_true', default=False)
        return parser
