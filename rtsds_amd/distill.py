"""Knowledge distillation: a frozen teacher (DeepLabV2, or any model with forward_lowres) teaches
the network that will be deployed (BiSeNet) through its soft class distribution.  The reference has
no distillation, so the protocol is this module's own, stated in functional.distill_kl: the loss is
T^2 * KL(teacher || student) on the student's low-resolution main head, the teacher's head resampled
onto that grid inside the kernel (csrc/distill.hip); the auxiliary heads are not distilled.

``distill_step`` is train.seg_step with that term added, ``train`` is train.train around it; both
leave train.py untouched.
"""
import torch

from . import functional as F
from . import train as _train
from . import utils
from .runtime import collect_cuts, dp_world
from .train import tqdm


class Distiller:
    """A frozen teacher and the distillation term's settings.  The teacher's parameters stop
    requiring gradients and it is put in eval mode -- and kept there: it is no submodule of the
    student, and ``teacher_head`` puts it back should someone have switched it to training, so its
    BatchNorm statistics never move."""

    def __init__(self, teacher, temperature=1.0, weight=1.0):
        if not hasattr(teacher, "forward_lowres"):
            raise RuntimeError("rtsds_amd.distill: the teacher must expose forward_lowres (BiSeNet, DeepLabV2)")
        if not float(temperature) > 0.0:
            raise ValueError(f"rtsds_amd.distill: temperature must be positive, got {temperature}")
        if not float(weight) >= 0.0:
            raise ValueError(f"rtsds_amd.distill: weight must not be negative, got {weight}")
        self.teacher = teacher.requires_grad_(False).eval()
        self.temperature, self.weight = float(temperature), float(weight)
        self.low_pixels = 0  # pixels of the student's low-resolution head in the last distill_step (what `agree` counts over)

    def teacher_head(self, inputs):
        """The teacher's low-resolution main head of ``inputs`` (no resize, no gradient graph)."""
        if self.teacher.training:
            self.teacher.eval()
        with torch.no_grad():
            (head, _), = self.teacher.forward_lowres(inputs, main_only=True)
        return head


def distill_step(model, distiller, criterion, optimizer, inputs, targets):
    """train.seg_step plus distillation: loss = CE(main) + CE(aux1) + CE(aux2) + weight *
    distill_kl(main low-resolution head, teacher's), with the same fused heads, cross-entropy and
    backward as seg_step.  Returns device tensors (loss, correct, kd, agree) -- no host sync: kd the
    unweighted distillation loss, agree the pixels (of the low-resolution grid) on which student and
    teacher predict the same class."""
    optimizer.zero_grad()
    teacher_low = distiller.teacher_head(inputs)
    split = dp_world() > 1 and hasattr(optimizer, "start_grad_allreduce")
    with collect_cuts(split) as cuts:
        fused = _train._fused_heads(model, criterion, inputs)
    if fused is None:
        raise RuntimeError("rtsds_amd.distill: the student needs forward_lowres and the CrossEntropy criterion "
                           "(the loss is taken on its low-resolution main head)")
    heads, geo = fused
    if geo is None:
        raise RuntimeError("rtsds_amd.distill: the student's heads must share one upsample geometry that the fused "
                           "cross-entropy covers")
    correct = torch.empty(1, dtype=torch.int64, device=inputs.device)  # (overwritten)
    agree = torch.zeros(1, dtype=torch.int64, device=inputs.device)
    ce = F.upsample_cross_entropy(heads, targets, geo, criterion.ignore_index, correct, set_correct=True,
                                  weight=criterion.weight)
    main_low = heads[0]
    distiller.low_pixels = main_low.shape[0] * main_low.shape[2] * main_low.shape[3]
    kd = F.distill_kl(main_low, teacher_low, distiller.temperature, agree)
    loss = ce + distiller.weight * kd
    _train._backward(loss, optimizer, cuts)
    optimizer.step()
    return loss.detach(), correct, kd.detach(), agree


def train(epoch: int, model: torch.nn.Module, train_loader, criterion: torch.nn.Module,
          optimizer: torch.optim.Optimizer, init_lr: float, max_iter: int, power: float = 0.9,
          lr_decay_iter: float = 1.0, device: str = "cuda", callbacks: list = [], distiller: Distiller = None):
    """train.train with the distillation term of ``distiller`` (required): one host sync per
    iteration, and on_batch_end also receives ``distill_loss`` (unweighted) and
    ``teacher_agreement`` (running, in % of the low-resolution pixels)."""
    if distiller is None:
        raise RuntimeError("rtsds_amd.distill.train needs distiller=Distiller(teacher, ...)")
    for cb in callbacks:
        cb.on_train_begin()
    model.train()
    running_loss, running_kd, correct, total, agreed, low_total = 0.0, 0.0, 0, 0, 0, 0
    for batch_idx, (inputs, targets) in tqdm(enumerate(train_loader), total=len(train_loader),
                                             desc=f"Epoch {epoch + 1}", leave=False):
        current_iter = epoch * len(train_loader) + batch_idx
        if current_iter % lr_decay_iter == 0 and current_iter <= max_iter:
            utils.poly_lr_scheduler(optimizer, init_lr, current_iter, lr_decay_iter, max_iter, power)
        inputs = inputs.to(device)
        targets = targets.to(device).squeeze(1)
        loss, corr, kd, agree = distill_step(model, distiller, criterion, optimizer, inputs, targets)
        vals = _train._host_values([loss, corr[0], kd, agree[0]])
        running_loss += vals[0]
        running_kd += vals[2]
        total += targets.size(0) * targets.size(1) * targets.size(2) * dp_world()
        correct += int(vals[1])
        agreed += int(vals[3])
        low_total += distiller.low_pixels * dp_world()
        for cb in callbacks:
            cb.on_batch_end(batch_idx, {"train_loss": vals[0], "train_accuracy": 100.0 * correct / total,
                                        "distill_loss": vals[2], "teacher_agreement": 100.0 * agreed / low_total})
    train_loss = running_loss / len(train_loader)
    train_accuracy = 100.0 * correct / total
    print(f"Train Epoch: {epoch + 1} Loss: {train_loss:.6f} Acc: {train_accuracy:.2f}% "
          f"Distill: {running_kd / len(train_loader):.6f} Teacher agreement: {100.0 * agreed / max(1, low_total):.2f}%")
    for cb in callbacks:
        cb.on_epoch_end(epoch, {"train_loss": train_loss, "train_accuracy": train_accuracy,
                                "distill_loss": running_kd / len(train_loader),
                                "teacher_agreement": 100.0 * agreed / max(1, low_total)})
    return model


__all__ = ["Distiller", "distill_step", "train"]
