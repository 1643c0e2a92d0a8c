"""
The training loop of ``python -m bonito_amd train`` (the reference's bonito/training.py: load_state, ClipGrad, Trainer), on the device:

    optimizer.zero_grad(set_to_none=True)
    optimizer.scale(model.loss(model.forward_train(x), targets, lengths)).backward()
    optimizer.step(max_norm)
    lr_scheduler.step()

``optimizer`` is bonito_amd.optim.AdamW: unscale, gradient norm, overflow check, clip, update and the loss-scale rule are three kinds
of kernel launch. The host reads the step's scalars (``optimizer.last()``) once per step, for the log and for the quantile clip.

The inference engine snapshots the weights when it is built and the update kernel changes them behind the module's back, so the engine
is dropped before every validation pass (and only there: forward_train does not use it). The model is any model whose forward_train
serves it: the LSTM and the transformer family of CRF models, and with norm="batch" the QuartzNet CTC models (bonito_amd.ctc). ``Trainer(norm="batch")`` trains convolutions that carry a
BatchNorm with batch statistics (forward_train's keyword): every sub-batch of a step rewrites the running statistics, as in the
reference, and the validation pass, which drops the engine, folds the new ones.
"""
import math
import os
import re
from collections import OrderedDict
from datetime import datetime
from glob import glob
from itertools import islice
from time import perf_counter

import numpy as np
import torch

from bonito_amd import optim
from bonito_amd.io import CSVLogger
from bonito_amd.schedule import linear_warmup_cosine_decay
from bonito_amd.util import accuracy, decode_ref, match_names

__all__ = ["load_state", "ClipGrad", "Trainer"]


def _numbers(dirname, name):
    return {int(m.group(1)) for m in (re.fullmatch(r".*_([0-9]+)\.tar", f) for f in glob(os.path.join(dirname, name + "_*.tar"))) if m}


def load_state(dirname, device, model, optim=None):
    """Load the newest weights_N.tar of `dirname` into `model`; with `optim`, the newest N that has both weights_N.tar and optim_N.tar,
    into both. -> N, the epoch to continue behind (0 = nothing found)."""
    model.to(device)
    weight_nos, optim_nos = _numbers(dirname, "weights"), _numbers(dirname, "optim")
    epoch = max(weight_nos & optim_nos if optim is not None else weight_nos, default=None)
    if not epoch:
        return 0
    print("[picking up %s state from epoch %s]" % ("weights, optim" if optim is not None else "weights", epoch))
    state = torch.load(os.path.join(dirname, "weights_%s.tar" % epoch), map_location=device)
    state = {k2: state[k1] for k1, k2 in match_names(state, model).items()}
    model.load_state_dict(OrderedDict((k.replace("module.", ""), v) for k, v in state.items()))
    if optim is not None:
        optim.load_state_dict(torch.load(os.path.join(dirname, "optim_%s.tar" % epoch), map_location=device))
    return epoch


class ClipGrad:
    """The quantile clip: max_norm = factor * quantile of the last `buffer_size` gradient norms (the buffer starts filled with 1e6, so
    the first steps are not clipped). ``max_norm()`` before the step, ``append(grad_norm)`` behind it; a NaN norm is not recorded."""

    def __init__(self, quantile=0.5, factor=2.0, buffer_size=100):
        self.buffer = np.full(buffer_size, fill_value=1e6)
        self.quantile, self.factor, self.i = quantile, factor, 0

    def max_norm(self):
        return float(self.factor * np.quantile(self.buffer, self.quantile))

    def append(self, grad_norm):
        if not math.isnan(grad_norm):
            self.buffer[self.i] = grad_norm
            self.i = (self.i + 1) % len(self.buffer)


class _FixedClip:
    def __init__(self, max_norm=2.0):
        self.value = max_norm

    def max_norm(self):
        return self.value

    def append(self, grad_norm):
        pass


class Trainer:
    def __init__(self, model, device, train_loader, valid_loader, criterion=None, use_amp=True, lr_scheduler_fn=None, restore_optim=False,
                 save_optim_every=10, grad_accum_split=1, quantile_grad_clip=False, chunks_per_epoch=None, batch_size=None, norm=None):
        if not use_amp:
            raise ValueError("Trainer: use_amp=False is not served: forward_train computes in fp16 and there is no fp32 path")
        if not hasattr(model, "forward_train"):
            raise ValueError("Trainer: %s has no forward_train (the LSTM and transformer families of CRF models and the QuartzNet CTC models train on the device)" % type(model).__name__)
        self.model = model.to(device)
        self.device = device
        self.train_loader, self.valid_loader = train_loader, valid_loader
        self.criterion = criterion or model.loss
        self.lr_scheduler_fn = lr_scheduler_fn or linear_warmup_cosine_decay()
        self.restore_optim, self.save_optim_every, self.grad_accum_split = restore_optim, save_optim_every, int(grad_accum_split)
        self.optimizer = None
        self.clip_grad = ClipGrad() if quantile_grad_clip else _FixedClip(2.0)
        self.batch_size, self.chunks_per_epoch = batch_size, chunks_per_epoch
        self.norm_kwargs = {} if norm is None else {"norm": norm}       # forward_train's keyword, passed only where it was asked for
        self.steps_per_epoch = chunks_per_epoch // batch_size

    def train_one_step(self, batch):
        """-> ({'loss': ...}, grad_norm, the loss scale the gradients carried). A step whose gradients overflowed leaves the weights
        alone and halves the scale; its grad_norm is inf or nan."""
        self.optimizer.zero_grad(set_to_none=True)
        losses = None
        for data, targets, lengths in zip(*(t.chunk(self.grad_accum_split, dim=0) for t in batch)):
            scores = self.model.forward_train(data.to(torch.float16).to(self.device), **self.norm_kwargs)
            losses_ = self.criterion(scores, targets, lengths)
            if not isinstance(losses_, dict):
                losses_ = {"loss": losses_}
            total = losses_.get("total_loss", losses_["loss"]) / self.grad_accum_split
            self.optimizer.scale(total).backward()
            losses = {k: v.item() / self.grad_accum_split + (0.0 if losses is None else losses[k]) for k, v in losses_.items()}
        self.optimizer.step(self.clip_grad.max_norm())
        grad_norm, scale, _ = self.optimizer.last()
        self.clip_grad.append(grad_norm)
        return losses, grad_norm, scale

    def train_one_epoch(self, loss_log, lr_scheduler):
        t0, chunks, smoothed = perf_counter(), 0, None
        self.model.train()
        for batch in islice(self.train_loader, self.steps_per_epoch):
            chunks += batch[0].shape[0]
            losses, grad_norm, scale = self.train_one_step(batch)
            smoothed = losses["loss"] if smoothed is None else 0.01 * losses["loss"] + 0.99 * smoothed
            if loss_log is not None:
                lr = lr_scheduler.get_last_lr() if lr_scheduler is not None else [g["lr"] for g in self.optimizer.param_groups]
                loss_log.append({"chunks": chunks, "time": perf_counter() - t0, "grad_norm": grad_norm,
                                 "lr": lr[0] if len(lr) == 1 else lr, "scale": scale, **losses})
            if lr_scheduler is not None:
                lr_scheduler.step()
        return smoothed, perf_counter() - t0

    def validate_one_step(self, batch):
        data, targets, lengths = batch
        scores = self.model(data.to(torch.float16).to(self.device))
        losses = self.criterion(scores, targets, lengths)
        losses = {k: v.item() for k, v in losses.items()} if isinstance(losses, dict) else losses.item()
        if hasattr(self.model, "decode_batch"):
            seqs = self.model.decode_batch(scores)
        else:                                 # bonito.ctc: the prefix beam search `evaluate` scores such a model with
            from bonito_amd.cli.evaluate import decode_batch
            seqs = decode_batch(self.model, scores)
        refs = [decode_ref(target, self.model.alphabet) for target in targets]
        n_pre, n_post = getattr(self.model, "n_pre_context_bases", 0), getattr(self.model, "n_post_context_bases", 0)
        if n_pre > 0 or n_post > 0:
            refs = [ref[n_pre:len(ref) - n_post] for ref in refs]
        accs = [accuracy(ref, seq, min_coverage=0.5) if len(seq) else 0.0 for ref, seq in zip(refs, seqs)]
        return seqs, refs, accs, losses

    def validate_one_epoch(self):
        """-> (mean of the batch losses, mean accuracy, median accuracy) over the validation set, with the CURRENT weights."""
        self.model.eval()
        self.model._drop_engine()             # the engine holds the weights of the moment it was built
        with torch.no_grad():
            seqs, refs, accs, losses = zip(*(self.validate_one_step(batch) for batch in self.valid_loader))
        accs = sum(accs, [])
        loss = np.mean([(x["loss"] if isinstance(x, dict) else x) for x in losses])
        return loss, np.mean(accs), np.median(accs)

    def init_optimizer(self, lr, **optim_kwargs):
        """AdamW over the trainable parameters. `lr`: a number, or a list of k of them (``--lr a,b``): the parameters, in the model's
        order, are then split into k groups of consecutive parameters of as equal a count as possible, one rate each (the first rate
        for the layers nearest the signal)."""
        if "package" in optim_kwargs:
            raise ValueError("Trainer: an [optim] package (%s.%s) is not served; the optimizer is bonito_amd.optim.AdamW"
                             % (optim_kwargs["package"], optim_kwargs.get("symbol")))
        print("[loading optim] - 'AdamW' with args: %s" % optim_kwargs)
        params = [p for p in self.model.parameters() if p.requires_grad]
        if isinstance(lr, (list, tuple)):
            if not 1 <= len(lr) <= len(params):
                raise ValueError("Trainer: %d learning rates for %d trainable parameters" % (len(lr), len(params)))
            bounds = [round(i * len(params) / len(lr)) for i in range(len(lr) + 1)]
            self.optimizer = optim.AdamW([{"params": params[lo:hi], "lr": v} for lo, hi, v in zip(bounds, bounds[1:], lr)], lr=lr[0],
                                         **optim_kwargs)
        else:
            self.optimizer = optim.AdamW(params, lr=lr, **optim_kwargs)

    def get_lr_scheduler(self, epochs, last_epoch=0):
        return self.lr_scheduler_fn(self.optimizer, self.steps_per_epoch, epochs, last_epoch)

    def fit(self, workdir, epochs=1, lr=2e-3, **optim_kwargs):
        if self.optimizer is None:
            self.init_optimizer(lr, **optim_kwargs)
        last_epoch = load_state(workdir, self.device, self.model, self.optimizer if self.restore_optim else None)
        if self.restore_optim:                # the command line's learning rate replaces the saved one
            for i, group in enumerate(self.optimizer.param_groups):
                group["initial_lr"] = group["lr"] = lr[i] if isinstance(lr, (list, tuple)) else lr
        lr_scheduler = self.get_lr_scheduler(epochs, last_epoch=last_epoch)
        for epoch in range(1 + last_epoch, epochs + 1):
            if hasattr(self.train_loader, "set_epoch"):
                self.train_loader.set_epoch(epoch)
            try:
                with CSVLogger(os.path.join(workdir, "losses_%s.csv" % epoch)) as loss_log:
                    train_loss, duration = self.train_one_epoch(loss_log, lr_scheduler)
                torch.save(self.model.state_dict(), os.path.join(workdir, "weights_%s.tar" % epoch))
                if epoch % self.save_optim_every == 0:
                    torch.save(self.optimizer.state_dict(), os.path.join(workdir, "optim_%s.tar" % epoch))
                val_loss, val_mean, val_median = self.validate_one_epoch()
            except KeyboardInterrupt:
                break
            print("[epoch {}] directory={} loss={:.4f} mean_acc={:.3f}% median_acc={:.3f}%".format(epoch, workdir, val_loss, val_mean, val_median))
            with CSVLogger(os.path.join(workdir, "training.csv")) as training_log:
                training_log.append({"time": datetime.today(), "duration": int(duration), "epoch": epoch, "train_loss": train_loss,
                                     "validation_loss": val_loss, "validation_mean": val_mean, "validation_median": val_median})
