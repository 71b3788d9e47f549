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


def _confusion_device(model, val_loader, num_classes, device, callbacks, scales=None, flip=False):
    hist = torch.zeros(num_classes * num_classes, dtype=torch.int64, device=device)
    for batch_idx, (inputs, targets) in enumerate(val_loader):
        inputs = inputs.to(device)
        targets = targets.to(device)
        if targets.dim() == 4:
            targets = targets.squeeze(1)
        if scales is None and not flip:
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
        detailed_report=False, scales=None, flip=False):
    """``scales`` / ``flip`` (rtsds): multi-scale / flip evaluation (predict_multiscale); absent,
    the single pass of the reference."""
    for cb in callbacks:
        cb.on_validation_begin()
    model.eval()
    with torch.no_grad():
        hist = _confusion_device(model, val_loader, num_classes, device, callbacks, scales, flip)
    ious = utils.per_class_iou(hist)
    mean_iou = np.nanmean(ious)
    print(f"Validation Mean IoU for Epoch {epoch + 1}: {mean_iou:.4f}")
    for cb in callbacks:
        cb.on_validation_end(mean_iou)
    return mean_iou


def val_GTA5(epoch, model, val_loader, num_classes, class_names, callbacks=[], device="cuda", scales=None,
             flip=False):
    import pandas as pd
    model.eval()
    for cb in callbacks:
        cb.on_validation_begin()
    with torch.no_grad():
        hist = _confusion_device(model, val_loader, num_classes, device, callbacks, scales, flip)
    ious = utils.per_class_iou(hist)
    total_miou = np.nanmean(ious)
    print(f"Validation mIoU for Epoch {epoch + 1}: {total_miou:.4f}")
    df = pd.DataFrame({"Class": class_names, "IoU": [f"{i:.4f}" for i in ious]})
    print(df)
    for cb in callbacks:
        cb.on_validation_end({"validation_mIoU": total_miou}, data=df)
    return total_miou, df
