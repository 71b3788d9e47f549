"""Validation loops (reference validation.py:12-148) with the argmax and the 19x19 confusion
histogram computed on the device (rtsds_argmax + rtsds_confusion); mIoU is
``utils.per_class_iou`` over the accumulated histogram exactly as the reference computes it.

Deviation (documented): ``val`` also accepts ``class_names`` / ``detailed_report`` -- the
reference's main.py:365-374 passes them and its ``val`` raises TypeError.
"""
import numpy as np
import torch

from . import functional as F
from . import utils


MAX_MULTISCALE_CLASSES = 32  # rtsds_upsoftmax_acc keeps one pixel's class row in registers


def scaled_size(size, scale, align=32):
    """(h, w) of an image rescaled by ``scale``, each side rounded to the nearest multiple of
    ``align`` (the networks' total stride) and never below ``align``."""
    return tuple(max(align, int(round(s * scale / align)) * align) for s in size)


def predict_multiscale(model, inputs, size, scales=(1.0,), flip=False, align=32):
    """Multi-scale / flip evaluation: summed class probabilities and their argmax.

    Protocol: for each scale, in the given order, the NCHW fp32 batch ``inputs`` is resized to
    ``scaled_size(inputs.shape[-2:], scale, align)`` (plain bilinear, align_corners=False, no
    antialias; skipped when the size is unchanged) and run through the model; its low-resolution
    head (``forward_lowres``) is resized straight to the label size ``size = (H, W)`` in ONE
    bilinear step, softmaxed over classes and added to an fp32 sum
    (functional.upsample_softmax_accumulate).  With ``flip`` the horizontally mirrored batch is
    evaluated as well and its probabilities are un-mirrored before the add.  At
    ``scales=(1.0,), flip=False`` and ``size`` = input size this is ``softmax(model(x))``.

    Returns ``(acc, pred)``: fp32 [n, H, W, c] probability sums and int64 [n, H, W] argmax."""
    if not hasattr(model, "forward_lowres"):
        raise RuntimeError("rtsds_amd: predict_multiscale needs a model with forward_lowres() "
                           "(BiSeNet, DeepLabV2); there is no fallback")
    scales = tuple(float(s) for s in scales)
    if not scales:
        raise RuntimeError("rtsds_amd: predict_multiscale needs at least one scale")
    H, W = int(size[0]), int(size[1])
    n = inputs.shape[0]
    passes = [(s, f) for s in scales for f in ((False, True) if flip else (False,))]
    acc = pred = None
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for i, (scale, mirrored) in enumerate(passes):
                if not mirrored:
                    hw = scaled_size(inputs.shape[-2:], scale, align)
                    x = inputs if hw == tuple(inputs.shape[-2:]) else F.interpolate_bilinear(inputs, size=hw)
                (low, _), = model.forward_lowres(torch.flip(x, dims=[3]) if mirrored else x, main_only=True)
                c = low.shape[1]
                if c > MAX_MULTISCALE_CLASSES:
                    raise RuntimeError(f"rtsds_amd: predict_multiscale covers at most {MAX_MULTISCALE_CLASSES} "
                                       f"classes, the model has {c}")
                if acc is None:
                    acc = torch.empty((n, H, W, c), dtype=torch.float32, device=low.device)
                    pred = torch.empty((n, H, W), dtype=torch.int64, device=low.device)
                F.upsample_softmax_accumulate(low, F.upsample_geometry(low, size=(H, W)), acc, flip=mirrored,
                                              accumulate=i > 0, pred=pred if i == len(passes) - 1 else None)
    finally:
        model.train(was_training)
    return acc, pred


def sliding_windows(size, window, stride=None):
    """The window origins [(y0, x0), ...] that cover ``size`` = (H, W) with ``window`` = (h, w)
    crops ``stride`` = (sy, sx) apart (default: half the window), row-major.  Per axis
    n = ceil((S - w) / s) + 1 origins o_i = min(i * s, S - w): the last window is pulled back
    inside, so every pixel is covered and no window leaves the image."""
    if stride is None:
        stride = tuple(max(1, int(w) // 2) for w in window)
    axes = []
    for S, w, s in zip(size, window, stride):
        S, w, s = int(S), int(w), int(s)
        if w < 1 or S < w:
            raise RuntimeError(f"rtsds_amd: sliding_windows: a window of {w} does not fit a side of {S}")
        if s < 1:
            raise RuntimeError(f"rtsds_amd: sliding_windows: the stride must be positive, got {s}")
        axes.append([min(i * s, S - w) for i in range(-(-(S - w) // s) + 1)])
    return [(y0, x0) for y0 in axes[0] for x0 in axes[1]]


def slide_table(size, window, stride=None, flip=False):
    """sliding_windows() as slide_paint's table [(y0, x0, flip), ...]; with ``flip`` each window is
    followed by its mirrored twin."""
    return [(y0, x0, m) for y0, x0 in sliding_windows(size, window, stride) for m in ((0, 1) if flip else (0,))]


def slide_chunks(table, nf, max_batch):
    """The table cut into chunks of max(1, max_batch // nf) windows (<= slide_paint's 64)."""
    per = min(F.MAX_SLIDE_WINDOWS, max(1, int(max_batch) // int(nf)))
    return [table[i:i + per] for i in range(0, len(table), per)]


def predict_sliding(model, inputs, window, stride=None, flip=False, max_batch=16, want_acc=False):
    """Sliding-window evaluation at native resolution: summed class probabilities of overlapping
    crops and their argmax.

    Protocol: the normalised NCHW batch ``inputs`` [n, 3, H, W] (any size >= ``window``) is cut
    into the crops of sliding_windows((H, W), window, stride) -- tensor slices, made contiguous;
    with ``flip`` each crop is followed by its copy mirrored along W -- which run through
    ``forward_lowres(main_only=True)`` in chunks of max(1, max_batch // n) windows (eval mode,
    no_grad; the training flag is restored).  Each chunk makes one functional.slide_paint call:
    every crop's low-resolution head is resized to the window size in ONE bilinear step and
    softmaxed as predict_multiscale does it, and a pixel's probabilities are summed over the
    windows covering it, in window order.  Chunks after the first accumulate onto an fp32 canvas,
    which exists only when there is more than one chunk or ``want_acc`` is set; only the last
    chunk writes the class map.

    Returns ``(acc or None, pred)``: fp32 [n, H, W, c] sums, int64 [n, H, W] argmax."""
    if not hasattr(model, "forward_lowres"):
        raise RuntimeError("rtsds_amd: predict_sliding needs a model with forward_lowres() "
                           "(BiSeNet, DeepLabV2); there is no fallback")
    if not inputs.is_cuda:
        raise RuntimeError("rtsds_amd: predict_sliding: inputs must be a HIP tensor; there is no CPU fallback")
    if inputs.dim() != 4:
        raise RuntimeError(f"rtsds_amd: predict_sliding: inputs must be [n, 3, H, W], got {tuple(inputs.shape)}")
    n, _, H, W = inputs.shape
    hw, ww = int(window[0]), int(window[1])
    chunks = slide_chunks(slide_table((H, W), (hw, ww), stride, flip), n, max_batch)
    acc = ids = None
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for i, chunk in enumerate(chunks):
                crops = [inputs[:, :, y0:y0 + hw, x0:x0 + ww] for y0, x0, _ in chunk]
                crops = [torch.flip(cr, dims=[3]) if m else cr for cr, (_, _, m) in zip(crops, chunk)]
                (low, _), = model.forward_lowres(torch.cat(crops).contiguous(), main_only=True)
                c = low.shape[1]
                if c > MAX_MULTISCALE_CLASSES:
                    raise RuntimeError(f"rtsds_amd: predict_sliding covers at most {MAX_MULTISCALE_CLASSES} "
                                       f"classes, the model has {c}")
                if acc is None and (len(chunks) > 1 or want_acc):
                    acc = torch.empty((n, H, W, c), dtype=torch.float32, device=low.device)
                ids, _ = F.slide_paint(low, F.upsample_geometry(low, size=(hw, ww)), chunk, (H, W), n, acc=acc,
                                       accumulate=i > 0, want_ids=i == len(chunks) - 1)
    finally:
        model.train(was_training)
    return acc, ids.long()


def _confusion_device(model, val_loader, num_classes, device, callbacks, scales=None, flip=False, window=None,
                      stride=None):
    hist = torch.zeros(num_classes * num_classes, dtype=torch.int64, device=device)
    for batch_idx, (inputs, targets) in enumerate(val_loader):
        inputs = inputs.to(device)
        targets = targets.to(device)
        if targets.dim() == 4:
            targets = targets.squeeze(1)
        if window is not None:
            _, pred = predict_sliding(model, inputs, window, stride=stride, flip=flip)
        elif scales is None and not flip:
            outputs = model(inputs)
            if isinstance(outputs, tuple):
                outputs = outputs[0]
            pred = F.argmax_channels(outputs)
        else:
            _, pred = predict_multiscale(model, inputs, targets.shape[-2:], scales=scales or (1.0,), flip=flip)
        F.confusion(targets.long(), pred, hist, num_classes)
        if callbacks:
            h = hist.view(num_classes, num_classes).cpu().numpy()
            tp = np.diag(h)
            loss = 1.0 - np.sum(tp) / max(np.sum(h), 1)
            for cb in callbacks:
                cb.on_validation_batch_end(batch_idx, loss)
    return hist.view(num_classes, num_classes).cpu().numpy()


def val(epoch, model, val_loader, num_classes, device="cuda", callbacks=[], class_names=None,
        detailed_report=False, scales=None, flip=False, window=None, stride=None):
    """``scales`` / ``flip`` (rtsds): multi-scale / flip evaluation (predict_multiscale); absent,
    the single pass of the reference.  ``window`` (h, w) / ``stride`` (rtsds): sliding-window
    evaluation at the loader's own resolution (predict_sliding; ``flip`` adds the mirrored
    twins); not together with ``scales``."""
    if window is not None and scales is not None:
        raise RuntimeError("rtsds_amd: val: window together with scales is not covered (a multi-scale slide); "
                           "pass one of them")
    for cb in callbacks:
        cb.on_validation_begin()
    model.eval()
    with torch.no_grad():
        hist = _confusion_device(model, val_loader, num_classes, device, callbacks, scales, flip, window, stride)
    ious = utils.per_class_iou(hist)
    mean_iou = np.nanmean(ious)
    print(f"Validation Mean IoU for Epoch {epoch + 1}: {mean_iou:.4f}")
    for cb in callbacks:
        cb.on_validation_end(mean_iou)
    return mean_iou


def val_GTA5(epoch, model, val_loader, num_classes, class_names, callbacks=[], device="cuda", scales=None,
             flip=False, window=None, stride=None):
    if window is not None and scales is not None:
        raise RuntimeError("rtsds_amd: val_GTA5: window together with scales is not covered (a multi-scale slide); "
                           "pass one of them")
    import pandas as pd
    model.eval()
    for cb in callbacks:
        cb.on_validation_begin()
    with torch.no_grad():
        hist = _confusion_device(model, val_loader, num_classes, device, callbacks, scales, flip, window, stride)
    ious = utils.per_class_iou(hist)
    total_miou = np.nanmean(ious)
    print(f"Validation mIoU for Epoch {epoch + 1}: {total_miou:.4f}")
    df = pd.DataFrame({"Class": class_names, "IoU": [f"{i:.4f}" for i in ious]})
    print(df)
    for cb in callbacks:
        cb.on_validation_end({"validation_mIoU": total_miou}, data=df)
    return total_miou, df
