"""Target entropy minimisation: beside the supervised loss on the labelled source batch (GTA5), an
unsupervised penalty on the network's own prediction of an unlabelled target batch (Cityscapes)
-- ADVENT's MinEnt (Vu et al. 2019), FDA's robust entropy (Yang & Soatto 2020) or Maximum Squares
(Chen et al. 2019).  The reference has none of them, so the protocol is this module's own, stated
in functional.entropy_loss: the penalty is taken on the low-resolution main head of the target batch
(csrc/entropy.hip); the auxiliary heads carry none.

``entmin_step`` is train.seg_step on the source batch plus that term on the target batch, ``train``
is train.train around it; both leave train.py untouched.
"""
import math

import torch

from . import functional as F
from . import train as _train
from . import utils
from .optim import begin_grad_phase
from .runtime import collect_cuts, dp_world
from .train import tqdm


class EntropyMinimiser:
    """The settings of the entropy term -- ``penalty`` (functional.ENTROPY_PENALTIES), ``eta`` (the
    robust penalty's exponent), ``weight`` of the term in the loss -- and the one iterator over the
    target loader that ``train`` draws from, epoch after epoch."""

    def __init__(self, penalty="entropy", eta=2.0, weight=0.001):
        if penalty not in F.ENTROPY_PENALTIES:
            raise ValueError(f"rtsds_amd.entmin: penalty must be one of {', '.join(F.ENTROPY_PENALTIES)}, got {penalty!r}")
        if not (float(eta) > 0.0 and math.isfinite(float(eta))):
            raise ValueError(f"rtsds_amd.entmin: eta must be positive, got {eta}")
        if not (float(weight) >= 0.0 and math.isfinite(float(weight))):
            raise ValueError(f"rtsds_amd.entmin: weight must not be negative, got {weight}")
        self.penalty, self.eta, self.weight = penalty, float(eta), float(weight)
        self._loader, self._it = None, None
        self.restarts = 0  # times the target loader ran out and was started again

    def next_target(self, loader):
        """The next target batch's images (its labels are dropped) from one persistent iterator over
        ``loader``, restarted when it runs out."""
        if self._loader is not loader:
            self._loader, self._it = loader, iter(loader)
        try:
            batch = next(self._it)
        except StopIteration:
            self._it = iter(loader)
            self.restarts += 1
            try:
                batch = next(self._it)
            except StopIteration:
                raise RuntimeError("rtsds_amd.entmin: the target loader is empty") from None
        return batch[0] if isinstance(batch, (tuple, list)) else batch


def entmin_step(model, em, criterion, optimizer, src_x, src_y, tgt_x):
    """train.seg_step on the source batch plus entropy minimisation on the target batch: loss =
    CE(main) + CE(aux1) + CE(aux2) on (src_x, src_y), with seg_step's fused heads and cross-entropy,
    + em.weight * entropy_loss(main low-resolution head of tgt_x).  The two backward passes are
    ordered as da_step orders its source and adversarial ones: the source loss plainly first, then
    the target forward inside collect_cuts and its backward in bucketed phases, so that under data
    parallelism no gradient arrives after its all-reduce has started; one optimizer step.  Returns
    device tensors (loss, correct, ent_loss, mean_entropy) -- no host sync: ent_loss the unweighted
    penalty, mean_entropy the target batch's mean normalised entropy."""
    optimizer.zero_grad()
    fused = _train._fused_heads(model, criterion, src_x)
    if fused is None:
        raise RuntimeError("rtsds_amd.entmin: the model needs forward_lowres and the CrossEntropy criterion "
                           "(the penalty is taken on its low-resolution main head)")
    heads, geo = fused
    if geo is None:
        raise RuntimeError("rtsds_amd.entmin: the model's heads must share one upsample geometry that the fused "
                           "cross-entropy covers")
    correct = torch.empty(1, dtype=torch.int64, device=src_x.device)  # (overwritten)
    ce = F.upsample_cross_entropy(heads, src_y, geo, criterion.ignore_index, correct, set_correct=True,
                                  weight=criterion.weight)
    ce.backward(_train._one(ce))

    split = dp_world() > 1 and hasattr(optimizer, "start_grad_allreduce")
    with collect_cuts(split) as cuts:
        (low, _), = model.forward_lowres(tgt_x, main_only=True)
    ent, mean_entropy = F.entropy_loss(low, em.penalty, em.eta)
    term = em.weight * ent
    _train._backward(term, optimizer, cuts, since=begin_grad_phase() if split else None)
    optimizer.step()
    return ce.detach() + term.detach(), correct, ent.detach(), mean_entropy


def train(epoch: int, model: torch.nn.Module, train_loader, criterion: torch.nn.Module,
          optimizer: torch.optim.Optimizer, init_lr: float, max_iter: int, power: float = 0.9,
          lr_decay_iter: float = 1.0, device: str = "cuda", callbacks: list = [], target_loader=None,
          minimiser: EntropyMinimiser = None):
    """train.train over the labelled source ``train_loader`` with the entropy term of ``minimiser``
    on batches of ``target_loader`` (both required; target labels are dropped): one host sync per
    iteration, and on_batch_end also receives ``entropy_loss`` (unweighted) and ``target_entropy``
    (the target batch's mean normalised entropy, in [0, 1])."""
    if minimiser is None or target_loader is None:
        raise RuntimeError("rtsds_amd.entmin.train needs target_loader= and minimiser=EntropyMinimiser(...)")
    for cb in callbacks:
        cb.on_train_begin()
    model.train()
    running_loss, running_ent, running_h, correct, total = 0.0, 0.0, 0.0, 0, 0
    for batch_idx, (inputs, targets) in tqdm(enumerate(train_loader), total=len(train_loader),
                                             desc=f"Epoch {epoch + 1}", leave=False):
        current_iter = epoch * len(train_loader) + batch_idx
        if current_iter % lr_decay_iter == 0 and current_iter <= max_iter:
            utils.poly_lr_scheduler(optimizer, init_lr, current_iter, lr_decay_iter, max_iter, power)
        inputs = inputs.to(device)
        targets = targets.to(device).squeeze(1)
        target_inputs = minimiser.next_target(target_loader).to(device)
        loss, corr, ent, h = entmin_step(model, minimiser, criterion, optimizer, inputs, targets, target_inputs)
        vals = _train._host_values([loss, corr[0], ent, h])
        running_loss += vals[0]
        running_ent += vals[2]
        running_h += vals[3]
        total += targets.size(0) * targets.size(1) * targets.size(2) * dp_world()
        correct += int(vals[1])
        for cb in callbacks:
            cb.on_batch_end(batch_idx, {"train_loss": vals[0], "train_accuracy": 100.0 * correct / total,
                                        "entropy_loss": vals[2], "target_entropy": vals[3]})
    batches = max(1, len(train_loader))
    train_loss = running_loss / batches
    train_accuracy = 100.0 * correct / max(1, total)
    print(f"Train Epoch: {epoch + 1} Loss: {train_loss:.6f} Acc: {train_accuracy:.2f}% "
          f"Entropy loss: {running_ent / batches:.6f} Target entropy: {running_h / batches:.4f}")
    for cb in callbacks:
        cb.on_epoch_end(epoch, {"train_loss": train_loss, "train_accuracy": train_accuracy,
                                "entropy_loss": running_ent / batches, "target_entropy": running_h / batches})
    return model


__all__ = ["EntropyMinimiser", "entmin_step", "train"]
