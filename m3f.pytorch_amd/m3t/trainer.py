"""Lightning-free training loop for AffWild2VA-style modules: what the reference gets from
`pl.Trainer(gradient_clip_val=1.0, check_val_every_n_epoch=1, distributed_backend='ddp')` (reference train.py:32-42) and
`AffWild2VA.configure_optimizers` (reference models/model.py:375-407), reduced to the hot loop -- zero flat grads,
training_step, backward, RCCL all-reduce + clip, fused optimizer step -- plus:

  * `freeze_enc` (model.py:376-386): everything frozen except fusion / proj_v / att_fuse BEFORE the flat buffers are
    built, so frozen parameters are outside the gradient buffer, the all-reduce, the clip norm and the weight decay;
  * the three schedulers (model.py:399-407): `plateau` = ReduceLROnPlateau(factor decay_factor, patience 3, min_lr 1e-6)
    on the epoch's val_loss, `exp` = ExponentialLR(decay_factor) per epoch, `cyclic` = CyclicLR(min_lr, learning_rate,
    step_size_up 5000, cycle_momentum iff sgd) per batch (model.py:220-224).  The schedules ARE torch's scheduler
    classes, driven on a one-scalar shadow optimizer whose lr / momentum are copied into the fused optimizer before
    every step: host glue, identical traces by construction;
  * validation after every epoch through the module's own validation_step / validation_end (window stitching,
    SURVEY 8(f) f-1) and a best-`val_loss` checkpoint (Lightning's default ModelCheckpoint monitors val_loss, mode min);
    `evaluate()` is the same epoch without a read-back per batch (m3t/evaluate.py), beside `validate()`, which `fit()` calls;
    `evaluate_cls()` is the multi-label counterpart for the AudioSet stage (m3t/cls_evaluate.py: mAP, mean AUC, d');
  * `{'state_dict': ...}` checkpoints the reference's eval.py loads strictly (eval.py:14-15), with optimizer and
    scheduler state for resume.

A dead persistent scan cannot reach the parameters: see FlatGradDDP.finish() and include/m3t_hip.h (error model);
step() polls the error word after the optimizer step is queued and save_checkpoint() synchronises and polls first.
"""
import gc
import os

import torch
import torch.distributed as dist

from . import ops
from .ddp import FlatGradDDP
from .optim import FlatAdam, FlatSGD


def apply_freeze_enc(model, fusion_type="attention"):
    """reference models/model.py:376-386"""
    for p in model.parameters():
        p.requires_grad = False
    live = [model.fusion, model.proj_v] + ([model.att_fuse] if fusion_type == "attention" else [])
    for m in live:
        for p in m.parameters():
            p.requires_grad = True


class Trainer:
    def __init__(self, model, optimizer="adam", learning_rate=5e-5, gradient_clip_val=1.0, process_group=None,
                 scheduler=None, decay_factor=0.5, min_lr=1e-8, freeze_enc=False, fusion_type="attention",
                 checkpoint_path=None):
        self.model = model
        self.freeze_gc = os.environ.get("M3T_TRAINER_FREEZE_GC", "1") != "0"
        if freeze_enc:
            apply_freeze_enc(model, fusion_type)
        self.ddp = FlatGradDDP(model, max_norm=gradient_clip_val, process_group=process_group, flatten_params=True)
        if optimizer == "adam":
            self.opt = FlatAdam(self.ddp, lr=learning_rate, weight_decay=1e-4)
            shadow = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=learning_rate, weight_decay=1e-4)
        elif optimizer == "sgd":
            self.opt = FlatSGD(self.ddp, lr=learning_rate, momentum=0.9, weight_decay=5e-4)
            shadow = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=learning_rate, momentum=0.9, weight_decay=5e-4)
        else:
            raise ValueError(optimizer)
        self._shadow = shadow
        self.scheduler_name = scheduler
        self.scheduler = None
        if scheduler == "cyclic":
            self.scheduler = torch.optim.lr_scheduler.CyclicLR(shadow, min_lr, learning_rate, step_size_up=5000,
                                                               cycle_momentum=optimizer == "sgd")
        elif scheduler == "exp":
            self.scheduler = torch.optim.lr_scheduler.ExponentialLR(shadow, decay_factor)
        elif scheduler == "plateau":
            self.scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(shadow, factor=decay_factor, patience=3, min_lr=1e-6)
        elif scheduler not in (None, "none"):
            raise ValueError(scheduler)
        self.checkpoint_path = checkpoint_path
        self.global_step = 0
        self.epoch = 0
        self.best_val_loss = float("inf")
        self.lr_history = []

    @classmethod
    def from_hparams(cls, model, hparams, **kw):
        """the reference's flags (models/model.py:448-493): optimizer, learning_rate, scheduler, decay_factor, min_lr,
        freeze_enc, fusion_type, checkpoint_path"""
        g = lambda k, d: getattr(hparams, k, d)
        args = dict(optimizer=g("optimizer", "adam"), learning_rate=g("learning_rate", 5e-5), scheduler=g("scheduler", None),
                    decay_factor=g("decay_factor", 0.5), min_lr=g("min_lr", 1e-8), freeze_enc=g("freeze_enc", False),
                    fusion_type=g("fusion_type", "attention"), checkpoint_path=g("checkpoint_path", None))
        args.update(kw)
        return cls(model, **args)

    # ------------------------------------------------------------------ schedule plumbing
    def _sync_hyper(self):
        grp = self._shadow.param_groups[0]
        self.opt.lr = float(grp["lr"])
        if isinstance(self.opt, FlatSGD):
            self.opt.momentum = float(grp["momentum"])

    @property
    def lr(self):
        return float(self._shadow.param_groups[0]["lr"])

    # ------------------------------------------------------------------ the hot loop
    def step(self, batch):
        """One optimisation step; returns the dict of model.training_step (loss is a device scalar)."""
        self.model.train()
        self._sync_hyper()
        self.ddp.zero_grad()
        out = self.model.training_step(batch, self.global_step)
        out["loss"].backward()
        out["grad_norm"] = self.ddp.finish()         # all-reduce, 1/N, clip; raises if a scan has died
        self.opt.step()                              # skipped on the device when the norm is not finite
        self.lr_history.append(self.opt.lr)
        if self.scheduler_name == "cyclic":          # per batch (reference models/model.py:220-224)
            self._shadow.step()                      # (keeps torch's "optimizer.step() before lr_scheduler.step()" order)
            self.scheduler.step()
        self.global_step += 1
        return out

    def validate(self, batches):
        """the module's own validation_step / validation_end over `batches`; returns validation_end's dict"""
        self.model.eval()
        outputs = [self.model.validation_step(b, i) for i, b in enumerate(batches)]
        self.ddp.agree_on_scan_error()               # eval forwards end here: nothing else would report a dead scan (every rank raises or none)
        res = self.model.validation_end(outputs)
        return res

    def evaluate(self, batches, test=False, out_path=None, expr=False):
        """validate() without a read-back per batch (m3t/evaluate.py): the forward passes are queued back to back, the windows
        are stitched and scored on the device, and the epoch ends with one read-back of the five metrics.  Follows the module's
        hooks: validation_step / validation_end, or with test=True test_step / test_end -- predictions only, overlap-added,
        saved as predictions_test.pt, result {}; under hparams.test_on_val those are the validation hooks with overlap-add, as
        in the reference.  Same tracks bit for bit, same file layout (out_path: another file name); the result is
        validation_end's dict with Python floats.  Each rank scores its own shard, as in validate().
        expr=True (a 9-channel `mtl` model; batches with class_expr / expr_valid when labelled) also stitches and scores the
        expression head, which the reference trains and never validates: `log` gains val_acc_expr / val_f1_expr /
        val_score_expr, progress_bar val_acc_expr, the file expr_logits / expr_pred (/ expr_gt); still one read-back."""
        from .evaluate import Evaluator
        hp = self.model.hparams
        test_on_val = bool(getattr(hp, "test_on_val", False))
        with_gt = test_on_val or not test
        ev = Evaluator(hp.window, overlap=test_on_val or test, with_gt=with_gt, expr=expr)
        self.model.eval()
        with torch.no_grad():
            for b in batches:
                ev.add(self.model.forward(b), b)
        self.ddp.agree_on_scan_error()               # as in validate(): nothing else would report a dead scan
        res = self.last_eval = ev.finish()           # the tracks stay on the device: self.last_eval.smoothed_report()
        res.save(out_path or ("predictions_val.pt" if with_gt else "predictions_test.pt"))
        if not with_gt:
            return {}
        m = res.metrics
        bar = {"val_ccc_v": m["val_ccc_v"], "val_ccc_a": m["val_ccc_a"]}
        if expr:
            bar["val_acc_expr"] = m["val_acc_expr"]
        return {"val_loss": m["val_loss"], "progress_bar": bar, "log": dict(m)}

    def evaluate_cls(self, feed, lds_rows=None):
        """validate() of a multi-label module (AudioSet) with the ranking metrics every published AudioSet figure is given in, scored on
        the device (m3t/cls_evaluate.py): one append launch per batch, no read-back per batch, one at the end.  `feed`: an epoch feed
        with plans() / batch(plan) / files (m3t/audioset.py), which says which items a batch holds; the module needs eval_scores(batch).
        Returns validation_end's dict, val_loss and val_acc with validate()'s bits as Python floats, with val_map / val_auc / val_dprime
        (and the counts) added to `log` and the three to `progress_bar`; the result stays as self.last_eval (report(), save()).  With
        world > 1 every rank's scores, labels and items are gathered (one all_gather each) and absorbed, so every rank ranks the whole
        split and reports the same ranking figures; val_loss / val_acc stay the rank's own shard's, as in validate()."""
        from .cls_evaluate import ClsEvaluator
        self.model.eval()
        ev = None
        for plan in feed.plans():
            b = feed.batch(plan)
            pooled, loss, correct = self.model.eval_scores(b)
            if ev is None:
                ev = ClsEvaluator(len(feed.files), pooled.size(1), lds_rows=lds_rows)
            ev.add(pooled, b["label"], plan.items, loss, correct)
        self.ddp.agree_on_scan_error()               # as in validate(): nothing else would report a dead scan
        if ev is None:
            raise ValueError("evaluate_cls: the feed gave no batch")
        if self.ddp.world > 1:
            mine = ev.shard()
            shards = []
            for t in mine:                           # DistributedSampler pads: every rank holds the same number of rows
                parts = [torch.empty_like(t) for _ in range(self.ddp.world)]
                dist.all_gather(parts, t, group=self.ddp.pg)
                shards.append(parts)
            for r in range(self.ddp.world):
                if r != self.rank:
                    ev.absorb(shards[0][r], shards[1][r], shards[2][r])
        res = self.last_eval = ev.finish()
        m = res.metrics
        bar = {k: m[k] for k in ("val_loss", "val_acc", "val_map", "val_auc", "val_dprime")}
        return {"val_loss": m["val_loss"], "progress_bar": bar, "log": dict(m)}

    # ------------------------------------------------------------------ rank plumbing
    @property
    def rank(self):
        return dist.get_rank(self.ddp.pg) if self.ddp.world > 1 else 0

    def _mean_over_ranks(self, value):
        """every replica must take the same plateau / best-checkpoint decision: the epoch's val_loss is averaged over the
        process group first (each rank validates its own shard of the windows)"""
        if self.ddp.world <= 1:
            return value
        # (value, "I have one"): a rank without a validation loss must not leave the others waiting in the collective
        t = torch.tensor([0.0 if value is None else float(value), 0.0 if value is None else 1.0], dtype=torch.float64)
        if dist.get_backend(self.ddp.pg) == "nccl":
            t = t.to(self.ddp.flat.device)
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.ddp.pg)
        have = int(round(float(t[1].item())))
        if have not in (0, self.ddp.world):
            raise RuntimeError("val_loss is None on %d of %d ranks: every rank must validate (or none)" % (self.ddp.world - have, self.ddp.world))
        return None if have == 0 else float(t[0].item()) / self.ddp.world

    def end_epoch(self, val_loss=None):
        """epoch-level schedulers + best-val_loss checkpoint (Lightning: check_val_every_n_epoch=1, ModelCheckpoint on val_loss).
        Under DDP the val_loss is the mean over ranks (identical lr / best decisions on every replica) and only rank 0
        writes the checkpoint (as Lightning's ModelCheckpoint), behind a barrier for the others."""
        val_loss = self._mean_over_ranks(val_loss)
        if self.scheduler_name == "exp":
            self._shadow.step()
            self.scheduler.step()
        elif self.scheduler_name == "plateau" and val_loss is not None:
            self.scheduler.step(float(val_loss))
        self.epoch += 1
        improved = val_loss is not None and float(val_loss) < self.best_val_loss
        if improved:
            self.best_val_loss = float(val_loss)
            if self.checkpoint_path:
                if self.rank == 0:
                    os.makedirs(self.checkpoint_path, exist_ok=True)
                self.save_checkpoint(os.path.join(self.checkpoint_path, "best.ckpt"))
        return improved

    def fit(self, batches, max_steps=None, log_every=0, val_batches=None, max_epochs=1, val_fn=None):
        """`batches`: an iterable of batch dicts = one epoch (re-iterated per epoch when max_epochs > 1).  val_fn: what scores
        `val_batches` after an epoch instead of validate(), e.g. evaluate_cls; its dict's val_loss drives end_epoch as before."""
        history = []
        done = 0
        for _ in range(max_epochs):
            for i, batch in enumerate(batches):
                if max_steps is not None and done >= max_steps:
                    break
                out = self.step(batch)
                done += 1
                if done == 1 and self.freeze_gc:
                    # a generation-2 pass of Python's cyclic collector stops the host for 45-100 ms in a process of this size:
                    # longer than its lead over the GPU (a step is 4-5 ms of host work, ~17 ms of GPU work).  Everything
                    # alive after the first step is long-lived: take it out of the collector's sight.
                    gc.collect()
                    gc.freeze()
                if log_every and i % log_every == 0:
                    history.append(float(out["loss"].detach()))
            val_loss = None
            if val_batches is not None:
                val_loss = float((val_fn or self.validate)(val_batches)["val_loss"])
            self.end_epoch(val_loss)
            if max_steps is not None and done >= max_steps:
                break
        self.ddp.agree_on_scan_error()
        return history

    # ------------------------------------------------------------------ checkpoints
    def save_checkpoint(self, path):
        """Rank 0 writes (to a temporary file, then os.replace: a reader never sees a torn file); the other ranks wait at a
        barrier so that none of them runs ahead into a load of a checkpoint that is still being written.  Every rank polls
        the scan error state first: parameters behind an unreported dead scan are never persisted."""
        self.ddp.agree_on_scan_error()
        err = None
        if self.rank == 0:
            try:
                opt_state = {"t": self.opt.t}
                for k in ("m", "v", "buf"):
                    if hasattr(self.opt, k):
                        opt_state[k] = getattr(self.opt, k).detach().cpu().clone()
                tmp = "%s.tmp.%d" % (path, os.getpid())
                torch.save({"state_dict": {k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
                            "global_step": self.global_step, "epoch": self.epoch, "best_val_loss": self.best_val_loss,
                            "optimizer": opt_state, "shadow_optimizer": self._shadow.state_dict(),
                            "scheduler": self.scheduler.state_dict() if self.scheduler is not None else None}, tmp)
                os.replace(tmp, path)
            except Exception as e:  # noqa: BLE001  (disk full, permissions ...: the other ranks must not wait at a barrier forever)
                err = e
        if self.ddp.world > 1:
            # instead of a bare barrier: rank 0 tells everyone whether the write succeeded; every rank raises if it did not
            flag = torch.tensor([0.0 if err is None else 1.0], dtype=torch.float32)
            if dist.get_backend(self.ddp.pg) == "nccl":
                flag = flag.to(self.ddp.flat.device)
            dist.all_reduce(flag, op=dist.ReduceOp.MAX, group=self.ddp.pg)
            if float(flag.item()) != 0.0 and err is None:
                raise RuntimeError("rank 0 could not write the checkpoint %s" % path)
        if err is not None:
            raise err

    def load_checkpoint(self, path, strict=True):
        ck = torch.load(path, map_location="cpu")
        self.model.load_state_dict(ck["state_dict"], strict=strict)     # copies into the flat-parameter views in place
        self.global_step = ck.get("global_step", 0)
        self.epoch = ck.get("epoch", 0)
        self.best_val_loss = ck.get("best_val_loss", float("inf"))
        st = ck.get("optimizer")
        if st:
            self.opt.t = st["t"]
            for k in ("m", "v", "buf"):
                if k in st and hasattr(self.opt, k):
                    getattr(self.opt, k).copy_(st[k])
        if ck.get("shadow_optimizer"):
            self._shadow.load_state_dict(ck["shadow_optimizer"])
        if ck.get("scheduler") and self.scheduler is not None:
            self.scheduler.load_state_dict(ck["scheduler"])
        self.ddp.broadcast_state()
        ops.weights_changed()                        # (world size 1: broadcast_state returns before it writes anything)
        return ck
