"""Mean teacher for online self-training (DACS-style; no reference counterpart: its loops
never train on target pixels).

    teacher = EMATeacher(student, model_loader(...)[0], optimizer, decay=0.99)
    loader = selftrain.TeacherLoader(target_loader, teacher, threshold=0.968, ignore_index=19)
    train.train(..., model=student, train_loader=loader, ...)   # teacher.update() after every step

The teacher is a second model of the student's architecture whose weights are the exponential
moving average of the student's,

    t = t + w * (s - t),   w = float32(1 - decay_t)

three separately rounded fp32 operations per element (rtsds_ema_step; never an FMA, so the
update can be restated exactly).  The student's parameters live in the optimizer's flat arenas
(optim._Arena); the teacher gets a flat fp32 buffer and a bf16 shadow per student arena with
the same offsets, so one launch per arena updates every parameter and writes the bf16 weights
the teacher's convs read in the same pass, as the optimizer kernels do for the student.  The
BatchNorm running statistics live outside the arenas and follow the student through one
rtsds_ema_many launch over a device pointer table; integer buffers (num_batches_tracked) are
copied.

Warm-up: with ``warmup`` the decay of update number ``updates`` (counted from 0) is
``min(decay, 1 - 1 / (updates + 1))``: the first update copies the student, the second averages
both, and the configured decay is reached after 1 / (1 - decay) updates.

Data parallelism: every rank's student is identical after the all-reduced optimizer step, and
every rank applies the same update with the same w, so the teachers stay identical on all ranks
without a collective.
"""
import numpy as np
import torch

from . import functional as F
from ._lib import lib
from .runtime import bump_params_epoch, stream


def decay_schedule(decay, updates, warmup=True):
    """The decay of update number ``updates`` (0 for the first): ``min(decay, 1 - 1 / (updates + 1))``
    with ``warmup``, else ``decay``."""
    return min(float(decay), 1.0 - 1.0 / (int(updates) + 1)) if warmup else float(decay)


def ema_weight(decay, updates, warmup=True):
    """w of that update as the kernels receive it: 1 - decay_t in float64, rounded to fp32."""
    return float(np.float32(1.0 - decay_schedule(decay, updates, warmup)))


class EMATeacher:
    """``student`` trained by ``optimizer`` (rtsds_amd.optim.Adam / SGD), ``teacher`` a second,
    freshly built model of the same architecture on the same device (not a deepcopy of the
    student: its parameters are arena views with hooks).  The teacher's parameters are rebound to
    views of this object's flat buffers, set to the student's values, frozen, and the model is
    put in eval mode; ``model`` is the teacher.

    ``update()`` -- after every optimizer step -- applies one EMA step to all parameters and
    floating buffers, copies the integer buffers and advances runtime's parameter epoch (the
    teacher's eval-mode BatchNorm folds are rebuilt).  It runs eagerly on the current stream and
    refuses a stream under capture.  ``updates`` counts the calls.

    ``state_dict()`` / ``load_state_dict()``: {"model": teacher.state_dict(), "updates": int,
    "decay": float}."""

    def __init__(self, student, teacher, optimizer, decay=0.99, warmup=True):
        if not 0.0 <= float(decay) < 1.0:
            raise RuntimeError(f"rtsds_amd: EMATeacher: decay must be in [0, 1), got {decay}")
        self.student, self.model, self.optimizer = student, teacher, optimizer
        self.decay, self.warmup, self.updates = float(decay), bool(warmup), 0
        where = {}
        for a in optimizer.arenas():
            for i, p in enumerate(a.params):
                where[id(p)] = (a, i)
        sp, tp = dict(student.named_parameters()), dict(teacher.named_parameters())
        if sp.keys() != tp.keys():
            raise RuntimeError("rtsds_amd: EMATeacher: the teacher's parameters do not match the student's "
                               f"({sorted(sp.keys() ^ tp.keys())[:4]} ...)")
        for name, p in sp.items():
            if id(p) not in where:
                raise RuntimeError(f"rtsds_amd: EMATeacher: the student's parameter {name} is in none of the "
                                   "optimizer's arenas")
            if tuple(tp[name].shape) != tuple(p.shape) or tp[name].device != p.device:
                raise RuntimeError(f"rtsds_amd: EMATeacher: parameter {name}: teacher {tuple(tp[name].shape)} on "
                                   f"{tp[name].device}, student {tuple(p.shape)} on {p.device}")
        # per student arena: the teacher's fp32 values and bf16 shadow at the same offsets
        self._store = {}
        with torch.no_grad():
            for name, p in sp.items():
                a, i = where[id(p)]
                if id(a) not in self._store:
                    self._store[id(a)] = (a, a.flat.clone(), torch.empty_like(a.shadow))
                _, flat, shadow = self._store[id(a)]
                q, off, n = tp[name], a.offsets[i], p.numel()
                q.data = flat[off:off + n].as_strided(p.shape, p.stride())
                q.requires_grad_(False)
                if q.dim() == 4:
                    q._rt_shadow = shadow[off:off + n].as_strided(p.shape, p.stride())
        self._refresh_shadows()
        # buffers: floating ones follow by EMA (one launch over a pointer table), the rest are copied
        sb, tb = dict(student.named_buffers()), dict(teacher.named_buffers())
        if sb.keys() != tb.keys():
            raise RuntimeError("rtsds_amd: EMATeacher: the teacher's buffers do not match the student's "
                               f"({sorted(sb.keys() ^ tb.keys())[:4]} ...)")
        self._float_buffers, self._int_buffers = [], []
        with torch.no_grad():
            for name, b in sb.items():
                if tuple(tb[name].shape) != tuple(b.shape) or tb[name].dtype != b.dtype:
                    raise RuntimeError(f"rtsds_amd: EMATeacher: buffer {name}: teacher {tb[name].dtype} "
                                       f"{tuple(tb[name].shape)}, student {b.dtype} {tuple(b.shape)}")
                tb[name].copy_(b)
                if b.dtype == torch.float32 and b.numel() > 0:
                    self._float_buffers.append((tb[name], b))
                elif b.is_floating_point() and b.numel() > 0:
                    raise RuntimeError(f"rtsds_amd: EMATeacher: buffer {name} is {b.dtype}; floating buffers must be fp32")
                else:
                    self._int_buffers.append((tb[name], b))
        self._table = None
        teacher.eval()
        bump_params_epoch()

    def _refresh_shadows(self):
        """bf16 shadows from the fp32 values, one rtsds_cast per arena; the 4-D weights' shadow
        keys follow (nn._shadow then uses the shadows as they are)."""
        for _, flat, shadow in self._store.values():
            lib.rtsds_cast(flat.data_ptr(), 0, shadow.data_ptr(), 1, flat.numel(), stream())
        for q in self.model.parameters():
            if q.dim() == 4 and getattr(q, "_rt_shadow", None) is not None:
                q._rt_shadow_key = (q.data_ptr(), q._version)

    def weight(self):
        """w of the next update (fp32-rounded)."""
        return ema_weight(self.decay, self.updates, self.warmup)

    @torch.no_grad()
    def update(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("rtsds_amd: EMATeacher.update() runs eagerly; call it outside a graph capture "
                               "(after the GraphedStep replay)")
        w = self.weight()
        for a, flat, shadow in self._store.values():
            F.ema_step(flat, a.flat, w, shadow)
        if self._float_buffers:
            if self._table is None or self._table.stale():
                self._table = F.EmaTable(self._float_buffers)
            F.ema_many(self._table, w)
        if self._int_buffers:  # copy_ of every integer buffer, batched
            torch._foreach_copy_([t for t, _ in self._int_buffers], [s for _, s in self._int_buffers])
        self.updates += 1
        bump_params_epoch()  # the kernels wrote through raw pointers: eval-mode BN folds are rebuilt

    def state_dict(self):
        return {"model": self.model.state_dict(), "updates": int(self.updates), "decay": float(self.decay)}

    @torch.no_grad()
    def load_state_dict(self, state):
        self.model.load_state_dict(state["model"])
        self.updates, self.decay = int(state["updates"]), float(state["decay"])
        self._refresh_shadows()
        bump_params_epoch()


__all__ = ["EMATeacher", "decay_schedule", "ema_weight"]
