"""Class-balanced self-training on the unlabelled target set (CBST; no reference counterpart:
its loops never train on target pixels).

    labels = generate(model, target_loader, num_classes)        # one sweep, everything on device
    tbin = class_thresholds(labels.hist, portion=0.2, cap=0.9)   # one host sync
    loader = PseudoLabelLoader(target_loader, labels, tbin, ignore_index=19)
    train.train(..., train_loader=loader, ...)                   # ordinary cross-entropy

``generate`` predicts every batch (validation.predict_multiscale), and the HIP kernel
rtsds_conf_hist turns the fp32 probability sum into a per-class confidence histogram plus, per
pixel, the predicted class (uint8) and its confidence bin (uint16): 3 B/pixel, 4.7 GB for the
Cityscapes train set at 512 x 1024.  ``class_thresholds`` picks, per class, the confidence above
which the wanted share of that class's pixels lies; ``PseudoLabelLoader`` applies the thresholds
per batch with rtsds_pseudo_select and yields the (inputs, labels) pairs train.train expects.

Quantisation.  Confidences are compared as bins of width 1 / bins: ``cbin >= tbin[k]`` is the
test ``conf >= tbin[k] / bins``.  A threshold is therefore a bin edge, and the pixels kept for
class k are exactly sum_{b >= tbin[k]} hist[k, b]: at least portion * N_k, and at most that
plus the population of bin tbin[k] (all of that bin is kept, not the part of it the exact
quantile would cut off).  With 1024 bins the confidence step is below 0.1 %.

Batch order.  The per-batch pred / cbin are recorded in the order the loader yielded them, so
the loader must replay the same batches in the same order on every iteration (main's
SyntheticLoader does; so does a non-shuffled, non-augmented transforms.DeviceLoader).  A
different batch count or batch shape is refused; different images of the same shape cannot be
detected.

ClassMix.  Trained on pseudo-labels alone the network sees no ground-truth pixel and its own
mistakes become its labels.  ``ClassMixLoader(target_loader, source_loader, labels, tbin,
ignore_index)`` replaces PseudoLabelLoader (config key training.self_training.mix: classmix):
every batch carries the pixels of half of the classes of a labelled source image, pasted into
target context, with their true labels (the HIP kernels rtsds_class_presence and
rtsds_classmix; the pseudo-label map of the target side is formed inside the mix and never
materialised).

Online form.  ``TeacherLoader(target_loader, teacher, threshold, ignore_index)`` needs none of the
above: an EMA teacher (ema.EMATeacher) labels every batch on the fly -- its low-resolution head
through one rtsds_upsample_pseudo launch -- so the target loader may be shuffled and augmented,
no sweep is run and nothing is stored (config key training.self_training.mode: online; ``mix:
classmix`` applies to it as well).
"""
import math

import numpy as np
import torch

from . import functional as F
from .validation import predict_multiscale


def _global_hist(hist):
    """``hist`` summed over the ranks of an initialised process group (a copy), else ``hist``."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        hist = hist.clone()
        dist.all_reduce(hist, op=dist.ReduceOp.SUM)
    return hist


def _check_tbin(tbin, c):
    t = np.asarray(tbin.cpu() if torch.is_tensor(tbin) else tbin).astype(np.int64).reshape(-1)
    if t.shape[0] != c:
        raise RuntimeError(f"rtsds_amd: selftrain: {t.shape[0]} thresholds for {c} classes")
    return t


def class_thresholds(hist, portion, cap=None):
    """Per-class confidence thresholds, as bin indices (int32 CPU tensor [c]), from the int64
    [c, bins] histogram of ``generate`` -- on the host (numpy), one sync per sweep.

    For class k with N_k = sum_b hist[k, b] pixels: need = max(1, ceil(portion * N_k)) (float64)
    and tbin[k] is the largest b whose tail sum_{b' >= b} hist[k, b'] reaches ``need``; an empty
    class gets ``bins`` (keeps nothing).  ``cap`` (a confidence in (0, 1]) limits every threshold
    to floor(cap * bins): no class demands more than ``cap``.  Without ``cap`` class k keeps
    exactly sum_{b >= tbin[k]} hist[k, b] pixels (see the module docstring for the bin
    quantisation).  Under an initialised process group of more than one rank the histogram is
    all-reduced (SUM) first, so every rank gets the same, global thresholds."""
    if not 0.0 < float(portion) <= 1.0:
        raise RuntimeError(f"rtsds_amd: class_thresholds: portion must be in (0, 1], got {portion}")
    if cap is not None and not 0.0 < float(cap) <= 1.0:
        raise RuntimeError(f"rtsds_amd: class_thresholds: cap must be in (0, 1], got {cap}")
    if hist.dim() != 2 or hist.dtype != torch.int64:
        raise RuntimeError(f"rtsds_amd: class_thresholds: hist must be int64 [c, bins], got {hist.dtype} "
                           f"{tuple(hist.shape)}")
    h = _global_hist(hist).cpu().numpy()
    c, bins = h.shape
    tail = np.cumsum(h[:, ::-1], axis=1)[:, ::-1]  # tail[k, b] = sum_{b' >= b} hist[k, b']
    tbin = np.full(c, bins, dtype=np.int32)
    for k in range(c):
        n_k = int(tail[k, 0])
        if n_k == 0:
            continue
        need = max(1, math.ceil(np.float64(portion) * np.float64(n_k)))
        tbin[k] = np.nonzero(tail[k] >= need)[0].max()  # the tail is non-increasing in b
    if cap is not None:
        tbin = np.minimum(tbin, np.int32(math.floor(float(cap) * bins)))
    return torch.from_numpy(tbin.astype(np.int32))


class PseudoLabels:
    """One sweep's result: ``hist`` (int64 [c, bins], on the sweep's device), the per-batch
    ``pred`` (uint8 [n, H, W]) and ``cbin`` (uint16 [n, H, W]) in loader order, and ``bins``."""

    def __init__(self, hist, pred, cbin, bins):
        self.hist, self.pred, self.cbin, self.bins = hist, pred, cbin, bins

    def __len__(self):
        return len(self.pred)

    @property
    def num_classes(self):
        return int(self.hist.shape[0])


def generate(model, loader, num_classes, bins=1024, scales=(1.0,), flip=False, device="cuda", store="device"):
    """One sweep over ``loader`` in its own order: every batch is predicted at the input size
    (predict_multiscale with ``scales`` / ``flip``) and reduced to (pred, cbin) plus the running
    histogram by functional.confidence_histogram.  The loader's own labels are ignored.
    ``store``: "device" keeps pred / cbin (3 B/pixel) in device memory, "cpu" copies each batch
    to the host.  Returns a PseudoLabels."""
    if store not in ("device", "cpu"):
        raise RuntimeError(f"rtsds_amd: selftrain.generate: store must be 'device' or 'cpu', got {store!r}")
    scales = tuple(float(s) for s in scales)
    passes = len(scales) * (2 if flip else 1)
    hist = None
    preds, cbins = [], []
    for inputs, _ in loader:
        inputs = inputs.to(device)
        acc, _ = predict_multiscale(model, inputs, inputs.shape[-2:], scales, flip)
        if acc.shape[-1] != num_classes:
            raise RuntimeError(f"rtsds_amd: selftrain.generate: the model predicts {acc.shape[-1]} classes, "
                               f"num_classes is {num_classes}")
        if hist is None:
            hist = torch.zeros((num_classes, bins), dtype=torch.int64, device=acc.device)
        pred = torch.empty(acc.shape[:3], dtype=torch.uint8, device=acc.device)
        cbin = torch.empty(acc.shape[:3], dtype=torch.uint16, device=acc.device)
        F.confidence_histogram(acc, hist, passes=passes, pred=pred, cbin=cbin)
        preds.append(pred.cpu() if store == "cpu" else pred)
        cbins.append(cbin.cpu() if store == "cpu" else cbin)
    if hist is None:
        raise RuntimeError("rtsds_amd: selftrain.generate: the loader yielded no batch")
    return PseudoLabels(hist, preds, cbins, bins)


class PseudoLabelLoader:
    """Iterates ``loader`` and yields ``(inputs, pseudo)`` with ``pseudo`` int64 [N, 1, H, W] --
    the format train.train expects -- made per batch by functional.pseudo_select from the
    recorded ``labels`` (a PseudoLabels) and the thresholds ``tbin`` (class_thresholds).
    ``len()`` is the loader's.

    The loader must replay the same batches in the same order on every iteration, the order
    ``generate`` saw: main's SyntheticLoader does, and so does a non-shuffled, non-augmented
    transforms.DeviceLoader.  A different number of batches or a batch of another shape raises
    RuntimeError.  ``set_thresholds`` replaces the thresholds between rounds without another
    sweep."""

    def __init__(self, loader, labels, tbin, ignore_index):
        self.loader, self.labels, self.ignore_index = loader, labels, int(ignore_index)
        if len(loader) != len(labels):
            raise RuntimeError(f"rtsds_amd: PseudoLabelLoader: the loader has {len(loader)} batches, "
                               f"{len(labels)} were recorded")
        self.set_thresholds(tbin)

    def set_thresholds(self, tbin):
        self.tbin = torch.from_numpy(_check_tbin(tbin, self.labels.num_classes).astype(np.int32))
        self._tbin_dev = {}

    def __len__(self):
        return len(self.loader)

    def _tbin_on(self, device):
        if device not in self._tbin_dev:
            self._tbin_dev[device] = self.tbin.to(device)
        return self._tbin_dev[device]

    def __iter__(self):
        n = 0
        for inputs, _ in self.loader:
            if n >= len(self.labels):
                raise RuntimeError(f"rtsds_amd: PseudoLabelLoader: the loader yielded more than the "
                                   f"{len(self.labels)} recorded batches")
            pred, cbin = self.labels.pred[n], self.labels.cbin[n]
            want = (inputs.shape[0], inputs.shape[2], inputs.shape[3])
            if tuple(pred.shape) != want:
                raise RuntimeError(f"rtsds_amd: PseudoLabelLoader: batch {n} has shape {want}, "
                                   f"{tuple(pred.shape)} was recorded")
            if not pred.is_cuda:  # store="cpu": back to the device of the sweep
                dev = self.labels.hist.device
                pred, cbin = pred.to(dev, non_blocking=True), cbin.to(dev, non_blocking=True)
            out = F.pseudo_select(pred, cbin, self._tbin_on(pred.device), self.ignore_index)
            yield inputs, out.unsqueeze(1)
            n += 1
        if n != len(self.labels):
            raise RuntimeError(f"rtsds_amd: PseudoLabelLoader: the loader yielded {n} batches, "
                               f"{len(self.labels)} were recorded")


class ClassMixLoader(PseudoLabelLoader):
    """PseudoLabelLoader with ClassMix (DACS): per target batch the next batch of the labelled
    ``source_loader`` is drawn and, per sample, the pixels of half of the classes present in a
    random target-sized window of the source image are pasted, image and label, onto the target
    image; every other pixel keeps the target image and its thresholded pseudo-label.  Yields
    ``(mixed_inputs, mixed_labels)`` -- inputs in the compute-dtype input form (pack_input),
    labels int64 [N, 1, H, W] -- which train.train consumes unchanged.  One pair of launches per
    batch (functional.class_presence + functional.classmix), no device -> host transfer.

    ``loader`` / ``labels`` / ``tbin``: PseudoLabelLoader's contract (same replay order, same
    refusals, ``set_thresholds``, ``len()``).  ``source_loader`` may be shuffled and augmented; it
    is restarted with a fresh iter() when exhausted.  Of a source batch the first N_target samples
    are used; one with fewer samples, or smaller than the target in H or W, raises RuntimeError.

    Random draws, per sample in order, from torch's default CPU generator:
    ``y0 = randint(0, Hs - H + 1, (1,))``, ``x0 = randint(0, Ws - W + 1, (1,))``,
    ``perm = randperm(c)``; the int32 [N, 2 + c] block goes to the device in one copy.
    ``last_chosen`` holds the last batch's chosen classes (uint32 bit masks [N], on the device)."""

    def __init__(self, loader, source_loader, labels, tbin, ignore_index):
        super().__init__(loader, labels, tbin, ignore_index)
        self.source_loader = source_loader
        self._source_iter = None
        self.last_chosen = None

    def _next_source(self):
        return _next_source(self)

    @staticmethod
    def draw(n, c, hs, ws, h, w):
        """The [n, 2 + c] int32 block of one batch's draws: rows (y0, x0, perm[0..c))."""
        blk = torch.empty((n, 2 + c), dtype=torch.int32)
        for i in range(n):
            blk[i, 0] = torch.randint(0, hs - h + 1, (1,))
            blk[i, 1] = torch.randint(0, ws - w + 1, (1,))
            blk[i, 2:] = torch.randperm(c)
        return blk

    def __iter__(self):
        n, c = 0, self.labels.num_classes
        for inputs, _ in self.loader:
            if n >= len(self.labels):
                raise RuntimeError(f"rtsds_amd: ClassMixLoader: the loader yielded more than the "
                                   f"{len(self.labels)} recorded batches")
            pred, cbin = self.labels.pred[n], self.labels.cbin[n]
            nt, h, w = inputs.shape[0], inputs.shape[2], inputs.shape[3]
            if tuple(pred.shape) != (nt, h, w):
                raise RuntimeError(f"rtsds_amd: ClassMixLoader: batch {n} has shape {(nt, h, w)}, "
                                   f"{tuple(pred.shape)} was recorded")
            dev = pred.device if pred.is_cuda else self.labels.hist.device
            mixed, mixed_labels = _mix_batch(self, inputs, pred, cbin, self._tbin_on(dev), c, dev)
            yield mixed, mixed_labels.unsqueeze(1)
            n += 1
        if n != len(self.labels):
            raise RuntimeError(f"rtsds_amd: ClassMixLoader: the loader yielded {n} batches, "
                               f"{len(self.labels)} were recorded")


def _next_source(ld):
    """The next batch of ``ld.source_loader``, restarted with a fresh iter() when exhausted."""
    for fresh in (False, True):
        if ld._source_iter is None or fresh:
            ld._source_iter = iter(ld.source_loader)
        try:
            return next(ld._source_iter)
        except StopIteration:
            continue
    raise RuntimeError(f"rtsds_amd: {type(ld).__name__}: the source loader yielded no batch")


def _mix_batch(ld, inputs, pred, cbin, tbin, c, dev):
    """One ClassMix batch, shared by ClassMixLoader (recorded pred / cbin) and TeacherLoader (the
    teacher's): draws the next source batch of ``ld`` and the per-sample window origins and class
    permutations (ClassMixLoader.draw), packs both images and runs functional.classmix with the
    target's ``pred`` / ``cbin`` thresholded by ``tbin``.  Sets ``ld.last_chosen``; returns
    (mixed inputs, mixed int64 labels [N, H, W])."""
    from .runtime import compute_dtype
    who = type(ld).__name__
    nt, h, w = inputs.shape[0], inputs.shape[2], inputs.shape[3]
    simg, slab = _next_source(ld)
    if simg.shape[0] < nt or simg.shape[2] < h or simg.shape[3] < w:
        raise RuntimeError(f"rtsds_amd: {who}: the source batch {tuple(simg.shape)} is smaller than "
                           f"the target batch {tuple(inputs.shape)} (samples, H or W)")
    if slab.shape[0] != simg.shape[0] or tuple(slab.shape[-2:]) != tuple(simg.shape[-2:]):
        raise RuntimeError(f"rtsds_amd: {who}: source labels {tuple(slab.shape)} do not match the "
                           f"source images {tuple(simg.shape)}")
    if not pred.is_cuda:  # store="cpu": back to the device of the sweep
        pred, cbin = pred.to(dev, non_blocking=True), cbin.to(dev, non_blocking=True)
    hs, ws = simg.shape[2], simg.shape[3]
    blk = ClassMixLoader.draw(nt, c, hs, ws, h, w).to(dev, non_blocking=True)
    dtype = compute_dtype()
    tgt = F.pack_input(inputs.to(dev), dtype)
    src = F.pack_input(simg[:nt].to(dev), dtype)
    slab = slab[:nt].to(dev).long().contiguous()
    chosen = torch.empty(nt, dtype=F._U32, device=dev)
    mixed, mixed_labels = F.classmix(src, slab, tgt, pred, cbin, tbin, blk[:, 2:], blk[:, :2], ld.ignore_index,
                                     chosen=chosen)
    ld.last_chosen = chosen
    return mixed, mixed_labels


class TeacherLoader:
    """Online (mean-teacher) pseudo-labels: iterates ``loader`` -- which may be shuffled and
    augmented, its own labels are ignored -- and labels every batch on the fly with ``teacher``
    (an ema.EMATeacher).  Per batch, under no_grad, the teacher's low-resolution main head
    (``teacher.model.forward_lowres(x, main_only=True)``) goes through ONE
    functional.upsample_pseudo launch to the input size, with the uniform threshold
    ``tbin = ceil(threshold * bins)`` for every class (a pixel is kept iff its confidence bin
    reaches it, i.e. conf >= tbin / bins).  Nothing is stored between batches and no sweep over
    the target set is needed.

    Without ``source_loader`` it yields ``(inputs, labels.unsqueeze(1))``, labels int64 with
    ``ignore_index`` -- the format train.train expects.  With ``source_loader`` (ClassMix) the
    kernel writes pred / cbin instead and the batch is mixed exactly as ClassMixLoader does (same
    draws from torch's default CPU generator, same functional.classmix call; ``last_chosen``).

    Update timing.  When iteration resumes after a ``yield`` the consumer has taken the
    student's step on that batch, so ``teacher.update()`` is called there: one update per yielded
    batch.  A consumer that abandons the iterator early (break) skips the update of its last
    batch.

    ``len()`` is the loader's.  ``last_kept`` is a device int64 scalar: the pixels of the last
    batch that were not ignored (for logging; reading it synchronises).  ``kept_sum`` (device
    int64) and ``pixels`` (host int) accumulate the same over the current iteration."""

    def __init__(self, loader, teacher, threshold=0.968, ignore_index=None, bins=1024, source_loader=None):
        if ignore_index is None:
            raise RuntimeError("rtsds_amd: TeacherLoader: ignore_index is required")
        bins = int(bins)
        if bins < 16 or bins > 1024 or bins & (bins - 1):
            raise RuntimeError(f"rtsds_amd: TeacherLoader: bins must be a power of two in [16, 1024], got {bins}")
        if not 0.0 <= float(threshold) <= 1.0:
            raise RuntimeError(f"rtsds_amd: TeacherLoader: threshold must be in [0, 1], got {threshold}")
        self.loader, self.teacher, self.ignore_index, self.bins = loader, teacher, int(ignore_index), bins
        self.threshold = float(threshold)
        self.tbin_value = int(math.ceil(self.threshold * bins))
        self.source_loader = source_loader
        self._source_iter = None
        self._tbin_dev = {}
        self.last_chosen = None
        self.last_kept = None
        self.kept_sum, self.pixels = None, 0

    def __len__(self):
        return len(self.loader)

    def _tbin_on(self, device, c):
        if (device, c) not in self._tbin_dev:
            self._tbin_dev[(device, c)] = torch.full((c,), self.tbin_value, dtype=torch.int32, device=device)
        return self._tbin_dev[(device, c)]

    def label(self, inputs):
        """(low, geo, tbin) of one batch: the teacher's low-resolution head, the geometry of its
        resize to the input size, and the thresholds on its device."""
        model = self.teacher.model
        if model.training:
            model.eval()
        dev = next(model.parameters()).device
        with torch.no_grad():
            (low, _), = model.forward_lowres(inputs.to(dev), main_only=True)
        return low, F.upsample_geometry(low, size=tuple(inputs.shape[-2:])), self._tbin_on(low.device, low.shape[1])

    def __iter__(self):
        self.kept_sum, self.pixels = None, 0
        for inputs, _ in self.loader:
            low, geo, tbin = self.label(inputs)
            with torch.no_grad():
                if self.source_loader is None:
                    _, _, labels = F.upsample_pseudo(low, geo, self.bins, tbin=tbin, ignore_index=self.ignore_index)
                    out = inputs
                else:
                    pred, cbin, _ = F.upsample_pseudo(low, geo, self.bins)
                    out, labels = _mix_batch(self, inputs, pred, cbin, tbin, low.shape[1], low.device)
                self.last_kept = (labels != self.ignore_index).sum()
                self.kept_sum = self.last_kept if self.kept_sum is None else self.kept_sum + self.last_kept
                self.pixels += labels.numel()
            yield out, labels.unsqueeze(1)
            self.teacher.update()  # the student's step on this batch has been taken


def kept_fraction(labels, tbin):
    """Per-class share of the predicted pixels that ``tbin`` keeps (float64 numpy [c]; NaN for a
    class nothing was predicted as), from the histogram alone -- for logging."""
    h = _global_hist(labels.hist).cpu().numpy()
    c, bins = h.shape
    t = _check_tbin(tbin, c)
    kept = np.array([h[k, min(int(t[k]), bins):].sum() for k in range(c)], dtype=np.float64)
    total = h.sum(axis=1).astype(np.float64)
    return np.where(total > 0, kept / np.maximum(total, 1), np.nan)


__all__ = ["class_thresholds", "generate", "PseudoLabels", "PseudoLabelLoader", "ClassMixLoader", "TeacherLoader", "kept_fraction"]
