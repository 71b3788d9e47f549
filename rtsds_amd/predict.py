"""Prediction: a trained checkpoint and camera frames in, class maps and painted frames out.

    python -m rtsds_amd.predict --weights CKPT.pth --input FRAME_OR_DIR --output DIR
                                [--config rtsds_amd/config.yaml] [--model bisenet|deeplab]
                                [--overlay A] [--label_ids] [--batch_size N]
                                [--stride SY,SX] [--flip] [--max_batch N]

No counterpart in the reference (its only consumers of a prediction are the validation histogram
and the losses).  Protocol, per call of a ``Predictor``: the uint8 frames, of any sizes, are
resized (antialiased) and normalised into one NHWC batch of the network size by
transforms.ImagePipeline, the model's low-resolution main head (``forward_lowres``, eval mode,
no_grad) is resized to each frame's own size in ONE bilinear step -- the rule of
validation.predict_multiscale -- and reduced to the arg-max class, which is what ``val`` takes;
functional.upsample_paint does resize, arg-max, id lookup, palette lookup and the blend over the
frame in one launch (rtsds_upsample_paint), one launch for all frames when they share a size.

Sliding windows (``Predictor(stride=...)``, ``--stride``): a frame at least as large as the network
size is not shrunk but cut into overlapping crops of the network size at its native resolution
(validation.sliding_windows; ``flip`` adds each crop's mirrored twin); the crops go through the
same pipeline (at equal size its resize is the identity) and model, and functional.slide_paint
(rtsds_slide_paint) sums the class probabilities of the crops covering each pixel -- the protocol
of validation.predict_sliding -- and paints the arg-max of the sum, one launch per chunk of
windows and no fp32 canvas when one chunk holds them all.  Smaller frames take the resize path.

Out of scope here: a hipGraph-replayed frame loop (the ops are capture-safe, so it can be added),
video decode, and multi-scale prediction (sliding windows at several scales included).
"""
import argparse
import os
import time

import torch

from . import functional as F
from .datasets.gta5 import TRAIN_ID_COLORS
from .runtime import compute_dtype, precision

# train id -> Cityscapes label id (the public cityscapesScripts table)
CITYSCAPES_LABEL_IDS = (7, 8, 11, 12, 13, 17, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 31, 32, 33)
MAX_CLASSES = 32  # rtsds_upsample_paint
IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg")


def default_palette():
    """TRAIN_ID_COLORS, the table rtsds_gta5_decode inverts, as a uint8 [19, 3] tensor."""
    return torch.tensor(TRAIN_ID_COLORS, dtype=torch.uint8)


class Predictor:
    """``model`` (on a HIP device, with ``forward_lowres``) applied to uint8 HWC frames.

    ``size``: the network input size (data.cityscapes.image_size).  ``palette``: [c][3] colours
    (default TRAIN_ID_COLORS); ``label_ids``: optional [c] ids written instead of the train ids
    (CITYSCAPES_LABEL_IDS); ``alpha`` in [0, 1]: weight of the colour over the frame (1.0: the
    mask alone); ``dtype``: compute dtype of the forward (default: the runtime's).  Palette and
    id table are moved to the device once.  ``stride`` = (sy, sx): sliding windows of ``size`` for
    every frame at least that large (None: every frame is resized, as before); ``flip`` adds the
    mirrored twin of each window; ``max_batch``: crops per forward."""

    def __init__(self, model, size, palette=None, label_ids=None, alpha=1.0, dtype=None, stride=None, flip=False,
                 max_batch=16):
        from . import transforms as T
        if not hasattr(model, "forward_lowres"):
            raise RuntimeError("rtsds_amd: Predictor needs a model with forward_lowres() (BiSeNet, DeepLabV2); "
                               "there is no fallback")
        param = next(model.parameters(), None)
        if param is None or not param.is_cuda:
            raise RuntimeError("rtsds_amd: Predictor needs a model on a HIP device; there is no CPU fallback "
                               "(move the model to 'cuda')")
        self.model, self.device = model, param.device
        self.alpha = float(alpha)
        if not 0.0 <= self.alpha <= 1.0:
            raise RuntimeError(f"rtsds_amd: Predictor: alpha must lie in [0, 1], got {alpha}")
        self.dtype = dtype
        pal = default_palette() if palette is None else torch.as_tensor(palette)
        if pal.dim() != 2 or pal.shape[1] != 3 or not 2 <= pal.shape[0] or pal.dtype not in (torch.uint8, torch.int64):
            raise RuntimeError(f"rtsds_amd: Predictor: palette must be [c][3] integers, got {tuple(pal.shape)} {pal.dtype}")
        if pal.shape[0] > MAX_CLASSES:
            raise RuntimeError(f"rtsds_amd: Predictor covers at most {MAX_CLASSES} classes, the palette has {pal.shape[0]}")
        if pal.min() < 0 or pal.max() > 255:
            raise RuntimeError("rtsds_amd: Predictor: palette entries must lie in 0..255")
        self.palette = pal.to(torch.uint8).contiguous().to(self.device)
        self.lut = None
        if label_ids is not None:
            lut = torch.as_tensor(label_ids)
            if tuple(lut.shape) != (pal.shape[0],) or lut.min() < 0 or lut.max() > 255:
                raise RuntimeError(f"rtsds_amd: Predictor: label_ids must be {pal.shape[0]} ids in 0..255")
            self.lut = lut.to(torch.uint8).contiguous().to(self.device)
        self.pipe = T.ImagePipeline(size)
        self.size = self.pipe.size
        self.stride = None if stride is None else (int(stride[0]), int(stride[1]))
        if self.stride is not None and min(self.stride) < 1:
            raise RuntimeError(f"rtsds_amd: Predictor: the stride must be positive, got {stride}")
        self.flip, self.max_batch = bool(flip), int(max_batch)
        if self.max_batch < 1:
            raise RuntimeError(f"rtsds_amd: Predictor: max_batch must be positive, got {max_batch}")

    def lowres(self, frames):
        """The main head [n, c, h/8, w/8] of the frames (uint8 HWC device tensors), resized and
        normalised to the network size."""
        was_training = self.model.training
        self.model.eval()
        try:
            with torch.no_grad(), precision(self.dtype or compute_dtype()):
                batch = self.pipe(frames)
                (low, _), = self.model.forward_lowres(batch, main_only=True)
        finally:
            self.model.train(was_training)
        if low.shape[1] > MAX_CLASSES:
            raise RuntimeError(f"rtsds_amd: Predictor covers at most {MAX_CLASSES} classes, the model has {low.shape[1]}")
        if low.shape[1] != self.palette.shape[0]:
            raise RuntimeError(f"rtsds_amd: Predictor: the model has {low.shape[1]} classes, the palette "
                               f"{self.palette.shape[0]}")
        return low

    def slide(self, frames, ids=True, rgb=True):
        """Sliding-window prediction of frames that share one size >= the network size: (ids, rgb)
        as uint8 [n, H, W] / [n, H, W, 3] tensors, None for one not asked for."""
        from .validation import slide_chunks, slide_table
        n, (H, W), (h, w) = len(frames), frames[0].shape[:2], self.size
        chunks = slide_chunks(slide_table((H, W), (h, w), self.stride, self.flip), n, self.max_batch)
        blend = rgb and self.alpha < 1.0
        acc = out_i = out_c = None
        for i, chunk in enumerate(chunks):
            crops = [f[y0:y0 + h, x0:x0 + w] for y0, x0, _ in chunk for f in frames]  # window-major
            crops = [(torch.flip(cr, dims=[1]) if chunk[j // n][2] else cr).contiguous() for j, cr in enumerate(crops)]
            low = self.lowres(crops)
            if acc is None and len(chunks) > 1:
                acc = torch.empty((n, H, W, low.shape[1]), dtype=torch.float32, device=self.device)
            last = i == len(chunks) - 1
            out_i, out_c = F.slide_paint(low, F.upsample_geometry(low, size=(h, w)), chunk, (H, W), n,
                                         palette=self.palette if rgb and last else None, alpha=self.alpha,
                                         frame=torch.stack(frames) if blend and last else None, lut=self.lut, acc=acc,
                                         accumulate=i > 0, want_ids=bool(ids) and last)
        return out_i, out_c

    def __call__(self, frames, ids=True, rgb=True):
        """``frames``: a list of uint8 HWC [H_i, W_i, 3] tensors (CPU ones are moved to the model's
        device).  Returns ``(ids, rgb)``: per frame a uint8 [H_i, W_i] id map and a uint8
        [H_i, W_i, 3] painted frame; None in place of a list not asked for."""
        if not (ids or rgb):
            raise RuntimeError("rtsds_amd: Predictor: nothing asked for (ids=False, rgb=False)")
        frames = [f.to(self.device) if f.device != self.device else f for f in frames]
        for f in frames:
            if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3:
                raise RuntimeError(f"rtsds_amd: Predictor takes uint8 HWC [H, W, 3] frames, got {f.dtype} {tuple(f.shape)}")
        frames = [f.contiguous() for f in frames]
        if self.stride is None:
            return self._resized(frames, ids, rgb)
        # frames of one size are batched: those at least as large as the network size slide, the rest are resized
        large = lambda f: f.shape[0] >= self.size[0] and f.shape[1] >= self.size[1]  # noqa: E731
        groups = {}
        for j, f in enumerate(frames):
            groups.setdefault((large(f),) + tuple(f.shape[:2]), []).append(j)
        out_i, out_c = [None] * len(frames), [None] * len(frames)
        for (slides, _, _), idx in groups.items():
            gi, gc = (self.slide if slides else self._resized)([frames[j] for j in idx], ids, rgb)
            for m, j in enumerate(idx):
                out_i[j] = gi[m] if ids else None
                out_c[j] = gc[m] if rgb else None
        return (out_i if ids else None), (out_c if rgb else None)

    def _resized(self, frames, ids, rgb):
        """The frames shrunk (or stretched) to the network size, the head painted at each frame's own size."""
        low = self.lowres(frames)
        blend = rgb and self.alpha < 1.0
        kw = dict(palette=self.palette if rgb else None, alpha=self.alpha, lut=self.lut, want_ids=bool(ids))
        sizes = {tuple(f.shape[:2]) for f in frames}
        if len(sizes) == 1:  # one launch
            geo = F.upsample_geometry(low, size=sizes.pop())
            i, c = F.upsample_paint(low, geo, frame=torch.stack(frames) if blend else None, **kw)
            return (list(i) if ids else None), (list(c) if rgb else None)
        out_i, out_c = [], []
        for n, f in enumerate(frames):
            one = low[n:n + 1]
            i, c = F.upsample_paint(one, F.upsample_geometry(one, size=f.shape[:2]), frame=f[None] if blend else None, **kw)
            out_i.append(i[0] if ids else None)
            out_c.append(c[0] if rgb else None)
        return (out_i if ids else None), (out_c if rgb else None)


def argument_parser(argv=None):
    p = argparse.ArgumentParser(description="Paint frames with a trained segmentation model (MI355X)")
    p.add_argument("--config", type=str, default=os.path.join(os.path.dirname(__file__), "config.yaml"))
    p.add_argument("--model", type=str, default="bisenet", choices=("bisenet", "deeplab"))
    p.add_argument("--weights", type=str, required=True, help="a state_dict (the reference's keys), read with weights_only=True")
    p.add_argument("--input", type=str, required=True, help="an image or a directory of .png / .jpg / .jpeg")
    p.add_argument("--output", type=str, required=True, help="directory for <stem>_color.png and <stem>_ids.png")
    p.add_argument("--overlay", type=float, default=1.0, help="weight of the colour over the frame (1.0: the mask alone)")
    p.add_argument("--label_ids", action="store_true", help="write Cityscapes label ids instead of train ids")
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--stride", type=str, default=None, help="SY,SX: sliding windows of the network size at the frame's own "
                                                            "resolution, this far apart (default: every frame is resized)")
    p.add_argument("--flip", action="store_true", help="with --stride: add the mirrored twin of every window")
    p.add_argument("--max_batch", type=int, default=16, help="with --stride: crops per forward")
    return p.parse_args(argv)


def input_paths(path):
    """The image itself, or the directory's images in sorted order."""
    if os.path.isdir(path):
        names = sorted(n for n in os.listdir(path) if n.lower().endswith(IMAGE_SUFFIXES))
        if not names:
            raise RuntimeError(f"rtsds_amd.predict: no {' / '.join(IMAGE_SUFFIXES)} image in {path}")
        return [os.path.join(path, n) for n in names]
    if not os.path.isfile(path):
        raise RuntimeError(f"rtsds_amd.predict: --input {path} does not exist")
    return [path]


def build_model(config, name, weights):
    """main._generator's model with the state_dict ``weights`` (no pretrained file is read: the
    weights come from --weights alone), on the configured device."""
    from .main import _generator
    from .utils import forModel
    cfg = {k: dict(v) for k, v in config.model.items() if k in ("bisenet", "deeplab")}
    cfg["deeplab"]["pretrain"] = False
    model = _generator(cfg, name)
    model.load_state_dict(torch.load(weights, map_location="cpu", weights_only=True))
    return forModel(model, config.device)


def main(argv=None):
    import numpy as np
    from PIL import Image

    from . import transforms as T
    from .main import load_config
    from .runtime import set_compute_dtype
    args = argument_parser(argv)
    if args.batch_size < 1:
        raise RuntimeError("rtsds_amd.predict: --batch_size must be positive")
    if args.max_batch < 1:
        raise RuntimeError("rtsds_amd.predict: --max_batch must be positive")
    if args.flip and args.stride is None:
        raise RuntimeError("rtsds_amd.predict: --flip needs --stride")
    config = load_config(args.config)
    set_compute_dtype(torch.bfloat16 if getattr(config, "precision", "fp32") == "bf16" else torch.float32)
    paths = input_paths(args.input)
    model = build_model(config, args.model, args.weights)
    predictor = Predictor(model, T.parse_size(config.data["cityscapes"]["image_size"]), alpha=args.overlay,
                          label_ids=CITYSCAPES_LABEL_IDS if args.label_ids else None,
                          stride=None if args.stride is None else T.parse_size(args.stride), flip=args.flip,
                          max_batch=args.max_batch)
    os.makedirs(args.output, exist_ok=True)
    t0 = time.perf_counter()
    for b in range(0, len(paths), args.batch_size):
        chunk = paths[b:b + args.batch_size]
        frames = [torch.from_numpy(np.array(Image.open(p).convert("RGB"))) for p in chunk]
        ids, rgb = predictor(frames)
        for p, i, c in zip(chunk, ids, rgb):
            stem = os.path.join(args.output, os.path.splitext(os.path.basename(p))[0])
            Image.fromarray(c.cpu().numpy()).save(stem + "_color.png")
            Image.fromarray(i.cpu().numpy()).save(stem + "_ids.png")
    dt = time.perf_counter() - t0  # the .cpu() copies above synchronise
    print(f"Predicted {len(paths)} frames in {dt:.3f} s ({len(paths) / dt:.1f} frames/s, decode and PNG encode "
          f"included) -> {args.output}")


__all__ = ["Predictor", "CITYSCAPES_LABEL_IDS", "default_palette", "main"]

if __name__ == "__main__":
    main()
