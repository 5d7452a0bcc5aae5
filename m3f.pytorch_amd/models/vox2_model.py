"""models.vox2_model -- stage 1 of the reference's workflow: pre-training the visual tower on VoxCeleb2, 1000-way identity.

Drop-in for the reference's models/vox2_model.py:25-194 (`VoxCeleb2_1k`): same `hparams` namespace and `add_model_specific_args`,
same sub-module name (`visual`) and therefore the same state_dict keys (`visual.v2p.*`, `visual.fc.0.*`, `visual.fc.2.*`), same
`forward(x)`, `ce_loss`, step and epoch-end dicts.  The loss end runs on csrc/cls_loss.hip: `training_step` hands the per-frame
logits [B,T,1000] to ONE operator (m3t.ops.pooled_cls_loss) that pools over T, evaluates the cross-entropy and the top-1 count and writes
dL/dz in its forward pass; `train_acc` stays on the device (M3T_STEP_SYNC=1: a Python float, as `acc_expr` of AffWild2VA).

The reference evaluates its loss only with `--backbone v2p --backend fc` (its defaults): the other two backbones return per-frame outputs
[B,T,1000] that the module never pools, and F.cross_entropy rejects them.  The constructor accepts `resnet` and `densenet` as the
reference's does; their steps raise here too (m3t.ops.cls_loss takes per-clip logits).  m3t/checkpoints.py carries a trained checkpoint
into AffWild2VA.  `batch['video']` may be uint8 frames as decoded with the draws in `batch['video_aug']` (m3t/video.py: crop, mirror, colour
jitter and normalisation in one kernel).  Out of scope: the dataloaders (VoxCeleb2, cv2) and the LR range finder.
"""
from argparse import ArgumentParser

import torch

from m3t import ops, video
from .backbone import VA_3DDenseNet, VA_3DResNet, VA_3DVGGM
from .model import _Base, _STEP_SYNC


class VoxCeleb2_1k(_Base):

    def __init__(self, hparams):
        super().__init__()
        try:
            self.hparams = hparams
        except AttributeError:      # newer Lightning: hparams is a read-only property
            self.save_hyperparameters(hparams)
        hp = hparams
        if hp.backbone == 'resnet':
            self.visual = VA_3DResNet(frameLen=hp.window, backend=hp.backend, resnet_ver='v1', nClasses=1000)
        elif hp.backbone == 'v2p':
            self.visual = VA_3DVGGM(frameLen=hp.window, backend=hp.backend, nClasses=1000, norm_layer=getattr(hp, 'norm_layer', 'bn'))
        elif hp.backbone == 'densenet':
            self.visual = VA_3DDenseNet(frameLen=hp.window, backend=hp.backend, nClasses=1000)
        self.history = {'lr': [], 'loss': []}

    def _frames(self):
        """the loss operator pools per-frame logits itself where the back-end ends in a temporal mean (v2p + fc)"""
        vis = getattr(self, 'visual', None)
        return isinstance(vis, VA_3DVGGM) and vis.backend == 'fc'

    def _normalised(self, x, aug=None, frame_idx=None):
        """to [-1, 1] (vox2_model.py:55); uint8 frames as decoded [N, Ts, Hs, Ws, 3] go through m3t.video (crop, mirror, jitter and this in one kernel)"""
        if x.dtype == torch.uint8:
            return video.ingest_for(self.visual, x, aug, frame_idx)
        return (x - 127.5) / 127.5

    def forward(self, x, aug=None, frame_idx=None):
        x = self._normalised(x, aug, frame_idx)
        if isinstance(x, torch.Tensor) and not x.is_cuda and self._frames():            # host input: the stock ops (the HIP back-end has no CPU path)
            return ops.temporal_pool(self.visual.forward_frames(x), 'mean')
        return self.visual(x)

    def ce_loss(self, y_hat, y):
        return ops.cls_loss(y_hat, y, 'ce')[0]

    def _loss_and_hits(self, x, y, aug=None, frame_idx=None):
        """(loss, stats = [loss, n_correct], correct [B]) of one batch"""
        if self._frames():
            z = self.visual.forward_frames(self._normalised(x, aug, frame_idx))
            return ops.pooled_cls_loss(z, y, 'mean', 'ce')
        return ops.cls_loss(self.forward(x, aug, frame_idx), y, 'ce')

    def training_step(self, batch, batch_idx):
        x, y = batch['video'], batch['label']
        loss, stats, _ = self._loss_and_hits(x, y, batch.get('video_aug'), batch.get('video_frame_idx'))
        # a 0-dim device tensor (the reference: `.item()`, one host sync per step, vox2_model.py:67)
        acc = float(stats[1]) / x.size(0) if _STEP_SYNC else stats[1] / x.size(0)
        if getattr(self.hparams, 'test_lr', False):
            raise NotImplementedError("LR range finder (models/lr_finder.py) is out of scope")
        return {'loss': loss, 'progress_bar': {'loss': loss, 'train_acc': acc}, 'log': {'loss': loss, 'train_acc': acc}}

    def on_batch_end(self):
        if getattr(self.hparams, 'scheduler', None) == 'cyclic' and hasattr(self, 'cyclic_scheduler'):
            self.cyclic_scheduler.step()

    def validation_step(self, batch, batch_idx):
        with torch.no_grad():
            loss, _, correct = self._loss_and_hits(batch['video'], batch['label'], batch.get('video_aug'), batch.get('video_frame_idx'))
        return {'val_loss': loss, 'correct': correct > 0}

    def validation_end(self, outputs):
        return _classification_epoch_end(outputs)

    def configure_optimizers(self):
        return _configure_optimizers(self, step_size_up=5000)

    @staticmethod
    def add_model_specific_args(parent_parser):
        """The reference's flags with the reference's defaults (vox2_model.py:165-194)."""
        parser = ArgumentParser(parents=[parent_parser])
        flags = [
            ('--backbone', 'v2p', str), ('--backend', 'fc', str), ('--learning_rate', 0.3, float), ('--min_lr', 1e-3, float),
            ('--decay_factor', 0.5, float), ('--batch_size', 128, int), ('--optimizer', 'sgd', str), ('--scheduler', 'plateau', str),
            ('--num_fc_layers', 2, int), ('--window', 16, int), ('--dataset_path', '/.data/zhangyuanhang/VoxCeleb2', str),
            ('--checkpoint_path', './vox2', str), ('--workers', 8, int), ('--max_nb_epochs', 80, int),
        ]
        for name, default, typ in flags:
            parser.add_argument(name, default=default, type=typ)
        for name in ('--test_lr', '--distributed'):
            parser.add_argument(name, action='store_true', default=False)
        return parser


def _classification_epoch_end(outputs):
    """validation_end of both pre-training modules (vox2_model.py:107-122, audioset_model.py:89-104)"""
    avg_loss = torch.stack([o['val_loss'] for o in outputs]).mean()
    hits = torch.cat([o['correct'] for o in outputs])
    val_acc = torch.sum(hits).item() / len(hits)
    return {'val_loss': avg_loss, 'progress_bar': {'val_loss': avg_loss, 'val_acc': val_acc},
            'log': {'val_loss': avg_loss, 'val_acc': val_acc}}


def _configure_optimizers(module, step_size_up):
    """configure_optimizers of both pre-training modules (vox2_model.py:124-145, audioset_model.py:106-127; the cyclic schedule's
    step_size_up is 5000 / 480)"""
    hp = module.hparams
    if getattr(hp, 'test_lr', False):
        raise NotImplementedError("LR range finder (models/lr_finder.py) is out of scope")
    if hp.optimizer == 'adam':
        opt = torch.optim.Adam(module.parameters(), lr=hp.learning_rate, weight_decay=1e-4)
    elif hp.optimizer == 'sgd':
        opt = torch.optim.SGD(module.parameters(), lr=hp.learning_rate, momentum=0.9, weight_decay=5e-4)
    else:
        raise ValueError(hp.optimizer)
    if hp.scheduler == 'cyclic':
        module.cyclic_scheduler = torch.optim.lr_scheduler.CyclicLR(opt, hp.min_lr, hp.learning_rate, step_size_up=step_size_up,
                                                                    cycle_momentum=hp.optimizer == 'sgd')
        return opt
    if hp.scheduler == 'exp':
        return [opt], [torch.optim.lr_scheduler.ExponentialLR(opt, hp.decay_factor)]
    if hp.scheduler == 'plateau':
        return [opt], [torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=hp.decay_factor, patience=3, min_lr=1e-6)]
    return opt
