"""Loss modules on the HIP kernels: drop-ins for the nn.CrossEntropyLoss(ignore_index) and
nn.BCEWithLogitsLoss() built by the reference's optimzer_loss_loader (main.py:124-134)."""
import math

import numpy as np
import torch
from torch import nn

from . import functional as F
from .runtime import dp_world


WEIGHT_MODES = ("inverse_log", "median_frequency")


def _weight_tensor(weight):
    """A criterion's ``weight`` (sequence, ndarray or tensor) as a float32 CPU tensor, validated:
    one dimension, every entry finite and non-negative."""
    w = weight.detach().cpu() if isinstance(weight, torch.Tensor) else torch.as_tensor(np.asarray(weight))
    if w.dim() != 1 or w.numel() == 0:
        raise ValueError(f"rtsds_amd.CrossEntropyLoss: weight must be a 1-D sequence of class weights, got shape "
                         f"{tuple(w.shape)}")
    if w.dtype == torch.bool or w.is_complex():
        raise ValueError(f"rtsds_amd.CrossEntropyLoss: weight must be numeric, got {w.dtype}")
    w = w.to(torch.float64)
    for k, v in enumerate(w.tolist()):
        if not math.isfinite(v) or v < 0.0:
            raise ValueError(f"rtsds_amd.CrossEntropyLoss: weight[{k}] = {v} is not a finite, non-negative number")
    return w.to(torch.float32)


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight, ignore_index), mean reduction; logits [N, C, H, W] (NHWC or
    NCHW memory), target int64 [N, H, W] (or [N, 1, H, W]).  Unweighted: the mean over non-ignored
    pixels of -log softmax(x)[target].  ``weight`` (c finite, non-negative numbers: sequence,
    ndarray or tensor; kept as a float32 buffer, so ``.to(device)`` moves it): sum of
    w[t] * (-log softmax(x)[t]) over the non-ignored pixels divided by the sum of their w[t].
    Under data parallelism the mean runs over every rank's pixels (runtime.dp_world): the count --
    the weight sum of a weighted criterion -- is all-reduced, nothing else."""

    def __init__(self, weight=None, ignore_index=-100, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("rtsds_amd.CrossEntropyLoss: mean reduction only (main.py:130)")
        self.ignore_index = -100 if ignore_index is None else int(ignore_index)
        self.register_buffer("weight", None if weight is None else _weight_tensor(weight))

    def set_weight(self, weight):
        """Install (or, with None, remove) the class weights; the buffer keeps the module's device."""
        if weight is None:
            self.weight = None
            return
        w = _weight_tensor(weight)
        dev = next((b.device for b in self.buffers()), None)
        self.weight = w if dev is None else w.to(dev)

    def forward(self, input, target):
        w = self.weight
        if w is not None and w.numel() != input.shape[1]:
            raise ValueError(f"rtsds_amd.CrossEntropyLoss: {w.numel()} class weights for {input.shape[1]} classes")
        return F.cross_entropy(input, target, self.ignore_index, w)


def class_weights(count, support=None, mode="inverse_log", c=1.02):
    """Class weights from the exact integer label statistics (functional.label_stats), in float64
    on the host; returns a float64 ndarray.

    * ``"inverse_log"`` (ENet, Paszke et al. 2016): w_k = 1 / ln(c + p_k), p_k = count_k / sum(count),
      c = 1.02 (weights in about [1.4, 50]; an absent class gets the largest).
    * ``"median_frequency"`` (Eigen & Fergus 2015): f_k = count_k / support_k, with support_k the valid
      pixels of the images that contain class k; w_k = median(f over the present classes) / f_k, and 0
      for an absent class."""
    cnt = np.asarray(count, dtype=np.float64)
    if cnt.ndim != 1 or cnt.size == 0 or (cnt < 0).any():
        raise ValueError("rtsds_amd.class_weights: count must be a 1-D array of non-negative pixel counts")
    if cnt.sum() <= 0:
        raise ValueError("rtsds_amd.class_weights: no labelled pixel")
    if mode == "inverse_log":
        return 1.0 / np.log(float(c) + cnt / cnt.sum())
    if mode == "median_frequency":
        if support is None:
            raise ValueError("rtsds_amd.class_weights: median_frequency needs support")
        sup = np.asarray(support, dtype=np.float64)
        if sup.shape != cnt.shape:
            raise ValueError(f"rtsds_amd.class_weights: support has shape {sup.shape}, count {cnt.shape}")
        present = cnt > 0
        f = cnt[present] / sup[present]
        w = np.zeros_like(cnt)
        w[present] = np.median(f) / f
        return w
    raise ValueError(f"rtsds_amd.class_weights: unknown mode {mode!r} (one of {', '.join(WEIGHT_MODES)})")


def class_statistics(loader, num_classes, ignore_index, device="cuda"):
    """One sweep over ``loader`` (batches whose second item is the int64 label map; the images
    are not touched): (count, support) of functional.label_stats as int64 ndarrays, accumulated on
    the device and fetched once.  Under data parallelism both are summed over the ranks, so every
    rank derives the same weights."""
    count = torch.zeros(int(num_classes), dtype=torch.int64, device=device)
    support = torch.zeros_like(count)
    for batch in loader:
        F.label_stats(batch[1].to(device, non_blocking=True).long(), num_classes, ignore_index, count, support)
    if dp_world() > 1:
        import torch.distributed as dist
        both = torch.stack([count, support])
        dist.all_reduce(both)
        count, support = both[0], both[1]
    return count.cpu().numpy(), support.cpu().numpy()


class BCEWithLogitsLoss(nn.Module):
    """Mean of the logistic loss.  Under data parallelism the mean runs over every rank's
    elements: every eager call all-reduces the local element count (a one-element collective,
    issued by every rank on every call, so the collectives of the ranks always pair up) and
    scales this rank's mean by n / total on the device (no host sync).  Under hipGraph capture
    (runtime.GraphedStep) no collective may run inside the captured segment, so the call reuses
    the scale of the last eager call with the same local size (the warm-up iterations before
    capture); graph replays have static shapes, so that scale stays valid.  A capture that meets
    a local size no eager call has seen raises instead of guessing."""

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("rtsds_amd.BCEWithLogitsLoss: mean only (main.py:132)")
        self._scale = {}

    def forward(self, input, target):
        loss = F.bce_with_logits(input, target)
        if dp_world() == 1:
            return loss
        # global-batch mean under data parallelism (see runtime.dp_world): this rank's mean
        # weighted by its share of the all-reduced element count, so shards of unequal size
        # still sum to the gathered-batch mean
        import torch.distributed as dist
        n = int(input.numel())
        key = (n, dp_world())
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            scale = self._scale.get(key)
            if scale is None:
                raise RuntimeError("rtsds_amd.BCEWithLogitsLoss: run an eager iteration with this local "
                                   "batch size before graph capture")
            return loss * scale
        cnt = torch.full((1,), float(n), dtype=torch.float64, device=input.device)
        dist.all_reduce(cnt)
        # fp32(n / total): the rounding ATen applies to a Python-float multiplier
        scale = (n / cnt).to(loss.dtype).reshape(())
        self._scale[key] = scale
        return loss * scale


class DistillationLoss(nn.Module):
    """Soft-target loss T^2 * KL(softmax(teacher / T) || softmax(student / T)), averaged over the
    student's pixels, between two low-resolution heads [N, C, h, w] whose grids may differ: the
    teacher is resampled onto the student's inside the kernel (functional.distill_kl, which states
    the whole protocol).  The reference has no counterpart.  ``agree``: optional int64 device
    counter that receives the number of pixels on which the two argmaxes agree.  Under data
    parallelism the mean runs over world * local pixels (equal shards)."""

    def __init__(self, temperature=1.0):
        super().__init__()
        if not float(temperature) > 0.0:
            raise ValueError(f"rtsds_amd.DistillationLoss: temperature must be positive, got {temperature}")
        self.temperature = float(temperature)

    def forward(self, student_low, teacher_low, agree=None):
        return F.distill_kl(student_low, teacher_low, self.temperature, agree)


class EntropyLoss(nn.Module):
    """Entropy minimisation on a low-resolution head [N, C, h, w] (functional.entropy_loss, which
    states the whole protocol): the mean over the pixels of ``penalty`` -- ``"entropy"`` the
    normalised Shannon entropy h of the softmax (ADVENT MinEnt), ``"robust"`` (h^2 + 1e-8)^eta
    (FDA), ``"max_squares"`` minus half the sum of the squared probabilities (Maximum Squares).
    The reference has no counterpart.  ``last_entropy``: the mean normalised entropy of the last
    forward, a 0-dim device tensor without gradient.  Under data parallelism the mean runs over
    world * local pixels (equal shards)."""

    def __init__(self, penalty="entropy", eta=2.0):
        super().__init__()
        if penalty not in F.ENTROPY_PENALTIES:
            raise ValueError(f"rtsds_amd.EntropyLoss: penalty must be one of {', '.join(F.ENTROPY_PENALTIES)}, got {penalty!r}")
        if not float(eta) > 0.0:
            raise ValueError(f"rtsds_amd.EntropyLoss: eta must be positive, got {eta}")
        self.penalty, self.eta = penalty, float(eta)
        self.last_entropy = None

    def forward(self, low):
        loss, self.last_entropy = F.entropy_loss(low, self.penalty, self.eta)
        return loss
