"""Autograd functions over the C ABI (include/rtsds_hip.h).

Every forward and backward here is a call into librtsds_hip.so on the current HIP stream;
PyTorch supplies only memory (caching allocator), the stream and the autograd graph.
Activations are NHWC tensors of logical shape [N, C, H, W] (``torch.channels_last``) in the
runtime compute dtype; parameters, statistics and losses are fp32.
"""
import ctypes

import numpy as np
import torch

from ._lib import (ACT_RELU, ACT_SIGMOID, INPUT_PADDED, UPCE_SET_CORRECT, WEIGHT_PACKED, BnParams, ConvDesc,
                   SplitReduceDesc, lib)
from .runtime import (CL, bump_params_epoch, collective, dcode, dp_world, empty_nhwc, nhwc, params_epoch,
                      register_fold, require_hip, side_enabled, side_fork, stream, workspace)

_P = lambda t: None if t is None else t.data_ptr()  # noqa: E731

# Optional conv-kernel timing (bench.py's live roofline): when ``CONV_PROFILE`` is a list,
# every implicit-GEMM launch is bracketed by HIP events on the launch stream and
# (start, end, algorithmic_flops) is appended.
CONV_PROFILE = None


def _conv_flops(d):
    return 2.0 * d.n * d.ho * d.wo * d.k * d.c * d.kh * d.kw


class _Timed:
    def __init__(self, d, tag="fwd"):
        self.d, self.tag = d, tag

    def __enter__(self):
        if CONV_PROFILE is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e1 = torch.cuda.Event(enable_timing=True)
            self.e0.record()
        return self

    def __exit__(self, *exc):
        if CONV_PROFILE is not None:
            self.e1.record()
            CONV_PROFILE.append((self.e0, self.e1, _conv_flops(self.d), self.tag, self.d))


# ----------------------------------------------------------------------------- grad sinks
def _sink(p):
    """The flat-arena gradient view of parameter ``p`` if an rtsds optimizer owns it.
    Backward kernels then accumulate straight into it (accumulate flag) and the Function
    returns None for ``p``, so autograd's per-parameter AccumulateGrad add never runs."""
    ref = getattr(p, "_rt_arena", None) if p is not None else None
    if ref is None:
        return None
    arena, i = ref
    return arena.sink(i)


def _sinks(*params):
    """All-or-nothing: the sinks of every given (non-None) parameter, or None."""
    out = []
    for p in params:
        if p is None:
            out.append(None)
            continue
        s = _sink(p)
        if s is None:
            return None
        out.append(s)
    return out


def _bn_param_grads(ctx, c, device):
    """(dgamma, dbeta, accumulate) of a BatchNorm backward: the parameters' sinks (accumulate = 1, the
    Function then returns None for both), else fresh fp32 [c] tensors for the gradients wanted."""
    return _bn_grads_of(ctx.gamma, ctx.beta, ctx.needs_input_grad[1], ctx.needs_input_grad[2], c, device)


def _bn_grads_of(gamma, beta, need_g, need_b, c, device):
    """_bn_param_grads for the parameters given."""
    sinks = _sinks(gamma if need_g else None, beta if need_b else None) if (need_g or need_b) else None
    if sinks is not None:
        return sinks[0], sinks[1], 1
    dg = torch.empty(c, dtype=torch.float32, device=device) if need_g else None
    db = torch.empty(c, dtype=torch.float32, device=device) if need_b else None
    return dg, db, 0


# ----------------------------------------------------------------------------- conv
def _conv_desc(x, k, kh, kw, stride, padding, dilation):
    n, c, h, w = x.shape
    ho = (h + 2 * padding[0] - dilation[0] * (kh - 1) - 1) // stride[0] + 1
    wo = (w + 2 * padding[1] - dilation[1] * (kw - 1) - 1) // stride[1] + 1
    d = ConvDesc(n, h, w, c, ho, wo, k, kh, kw, stride[0], stride[1], padding[0], padding[1],
                 dilation[0], dilation[1], dcode(x))
    return d


def is_padded_input(x, d=None):
    """A tensor written with the padded channel pitch a conv gathers (upsample_softmax's class
    probabilities, pitch 32; pack_input's 3-channel images, pitch 4): [N, C, H, W] view of an
    NHWC [N, H, W, Cp] buffer, zero in C..Cp-1.  With a conv descriptor ``d``: and Cp is the
    pitch that conv reads (rtsds_conv2d_input_pitch)."""
    cp = getattr(x, "_rt_cpad", None)
    ok = cp is not None and x.dim() == 4 and x.stride(1) == 1 and x.stride(3) == cp and \
        x.stride(2) == cp * x.shape[3] and x.stride(0) == cp * x.shape[2] * x.shape[3]
    return ok and (d is None or lib.rtsds_conv2d_input_pitch(ctypes.byref(d)) == cp)


def detach_padded(x):
    """x.detach() keeping the padded-input marker (tensor attributes do not survive detach)."""
    y = x.detach()
    if getattr(x, "_rt_cpad", None) is not None:
        y._rt_cpad = x._rt_cpad
    return y


# ----------------------------------------------------------------------------- packed dgrad weights
# The data-gradient GEMMs read each conv weight transposed ([ci][tap][co], flipped / split per
# stride-2 phase by route).  For weights owned by an rtsds optimizer the transposed copy is
# refreshed by the optimizer right after its update -- every registered conv in one launch
# (optim._Arena.repack -> rtsds_conv2d_dgrad_pack_many) -- and the backward passes it with
# RTSDS_WEIGHT_PACKED instead of repacking per call.  A conv registers on its first backward;
# the copy is used once the optimizer has packed it from the current bf16 shadow.
_DPACK = {"on": True}


def set_dgrad_packs(on):
    """Use optimizer-maintained packed dgrad weights (default on; off: repack per call)."""
    _DPACK["on"] = bool(on)


class _DPack:
    __slots__ = ("arena", "key", "desc", "buf", "valid")


def _desc_key(d):
    return tuple(getattr(d, f) for f, _ in ConvDesc._fields_)


def _dgrad_weight(weight, wq, d):
    """(weight operand, flag) for a data-gradient launch of ``weight`` with descriptor ``d``."""
    if not _DPACK["on"] or wq.dtype != torch.bfloat16 or weight is None:
        return wq, 0
    ref = getattr(weight, "_rt_arena", None)
    if ref is None:
        return wq, 0
    pk = getattr(weight, "_rt_dpack", None)
    if pk is not None and pk.arena is ref[0]:
        if pk.key == _desc_key(d) and pk.buf is not None and pk.valid is not None and \
                pk.valid == getattr(weight, "_rt_shadow_key", None) and wq is getattr(weight, "_rt_shadow", None):
            return pk.buf, WEIGHT_PACKED
        return wq, 0
    pk = _DPack()
    pk.arena, pk.key, pk.valid = ref[0], _desc_key(d), None
    pk.desc = ConvDesc(*pk.key)
    nb = lib.rtsds_conv2d_dgrad_pack_bytes(ctypes.byref(d))
    pk.buf = torch.empty(nb // 2, dtype=torch.bfloat16, device=wq.device) if nb else None
    weight._rt_dpack = pk
    if nb:
        ref[0].dpacks.append(weight)
    return wq, 0


class GradJoin:
    """Gradient of a tensor read by ``n`` rtsds Functions -- a residual block's input, read by
    conv1 and by the identity (BatchNorm residual) or downsample branch
    (build_contextpath.py BasicBlock / Bottleneck; torchvision resnet.py semantics).

    Autograd would sum the ``n`` contributions with its own elementwise add over the whole
    activation.  Instead the first contribution's buffer is kept here and handed to the next
    producer, whose kernel accumulates into it (conv dgrad ``accumulate`` flag); the first
    ``n - 1`` backward calls return None for the tensor and the last returns the sum, so the
    engine sees one gradient.  Order-independent: whichever producer runs last returns.

    ``first_returns``: for a tensor whose readers need not all be reached by the backward (a
    model output the caller may leave out of the loss): the first contribution returns its
    buffer and later ones accumulate into it in place and return None -- the engine runs the
    tensor's producer only after every reached reader, so it sees the full sum either way."""

    __slots__ = ("left", "buf", "first")

    def __init__(self, n, first_returns=False):
        self.left = n
        self.buf = None
        self.first = first_returns

    def put(self, g):
        """Record this producer's finished contribution (``g`` already includes ``buf``)."""
        if self.first:
            if self.buf is None:
                self.buf = g
                return g
            return None  # accumulated into the returned buffer
        self.buf = g
        self.left -= 1
        return g if self.left == 0 else None


def _join_add(join, g):
    """Contribution ``g`` computed into its own buffer: fold any earlier one in, then put."""
    if join is None:
        return g
    if join.buf is not None:  # not reached in the residual blocks (the BN runs first)
        if join.first:
            join.buf.add_(g)
            return join.put(join.buf)
        g.add_(join.buf)
    return join.put(g)


# ----------------------------------------------------------------------------- deferred wgrad reduce
# The split-K weight gradients of one backward pass leave their fp32 partial slabs in workspace
# and are reduced into the optimizer's gradient arena together, by one rtsds_split_reduce_many
# launch at the end of the backward (an autograd engine callback, so .grad is complete when
# backward() returns) instead of one small launch per conv (~27 per BiSeNet step).  Same sums,
# same order.  Off while bench.py event-times each conv (CONV_PROFILE).
DEFER_WGRAD_REDUCE = True
# [(SplitReduceDesc, workspace tensor holding the slabs, stream of the wgrad, the weight, keep)]
# keep: the gradient must stay readable in .grad after the optimizer step (the image convs)
_deferred = []
# The optimizer step sums the slabs itself (optim.Adam, rtsds_adam_step_slabs): the reductions of a
# backward pass whose optimizer has opted in (fuse_wgrad_reduce_into; train.seg_step) are handed to
# it instead of launched, and the weight gradients never reach the arena.  False: always reduce
# at the end of the backward (A/B runs and tests).
FUSE_REDUCE_ADAM = True
_fuse_into = [None]  # the optimizer that opted in for the backward pass now running


def fuse_wgrad_reduce_into(optimizer):
    """Opt in for the next backward pass only: its deferred reductions onto ``optimizer``'s
    parameters go to optimizer.take_wgrad_reduces() at the end of the pass (None: opt out)."""
    _fuse_into[0] = optimizer if FUSE_REDUCE_ADAM and DEFER_WGRAD_REDUCE else None


def reduce_wgrads_now(items, cur):
    """rtsds_split_reduce_many over pending items on stream ``cur``: one launch per run of distinct
    targets (a parameter reduced twice keeps its order); the targets now hold their gradients."""
    batch, seen = [], set()
    for desc, *_ in list(items) + [(None,)]:
        if desc is None or desc.dw in seen or len(batch) == 16:
            if batch:
                arr = (SplitReduceDesc * len(batch))(*batch)
                lib.rtsds_split_reduce_many(len(batch), arr, cur.cuda_stream)
            batch, seen = [], set()
        if desc is not None:
            batch.append(desc)
            seen.add(desc.dw)
    for _desc, _ws, _st, weight, _keep in items:
        arena, i = weight._rt_arena
        arena.dirty[i] = True


def flush_wgrad_reduce():
    """Run the pending split-K reductions (every deferral also queues this as an end-of-backward
    callback; the first one of a backward pass does the work, optim.step() calls it too) -- or
    hand them to the optimizer that opted in for this pass."""
    global _deferred
    items, _deferred = _deferred, []
    owner, _fuse_into[0] = _fuse_into[0], None
    if not items:
        return
    cur = torch.cuda.current_stream(items[0][1].device)
    for st in {it[2] for it in items}:  # wgrads issued on branch streams
        if st != cur:
            cur.wait_stream(st)
    mine = []
    if owner is not None and FUSE_REDUCE_ADAM:
        own = owner.arenas()
        mine = [it for it in items if any(it[3]._rt_arena[0] is a for a in own)]
        owner.take_wgrad_reduces(mine)
    reduce_wgrads_now([it for it in items if not any(it is m for m in mine)], cur)
    for _desc, ws, st, *_ in items:
        if st != cur:
            ws.record_stream(cur)


def _defer(pend, ws, weight, keep=False):
    """Queue a pending reduction onto ``weight``'s arena gradient: the sink handed out for it has
    not been written."""
    arena, i = weight._rt_arena
    arena.sink_unwritten(i)
    _deferred.append((pend, ws, torch.cuda.current_stream(ws.device), weight, keep))
    torch.autograd.Variable._execution_engine.queue_callback(flush_wgrad_reduce)


def _wgrad_into_arena(d, x, g, sinks, xflag, ws, weight):
    """Weight gradient accumulated into the optimizer arena; its split-K reduction deferred to
    the end of the backward pass when allowed."""
    if DEFER_WGRAD_REDUCE and CONV_PROFILE is None and x.dtype == torch.bfloat16:
        pend = SplitReduceDesc()
        lib.rtsds_conv2d_wgrad_deferred(ctypes.byref(d), _P(x), _P(g), _P(sinks[0]), _P(sinks[1]), 1 | xflag,
                                        _P(ws), ws.numel(), ctypes.byref(pend), stream())
        if pend.nv > 0:
            _defer(pend, ws, weight)
        return
    with _Timed(d, "wgrad"):
        lib.rtsds_conv2d_wgrad(ctypes.byref(d), _P(x), _P(g), _P(sinks[0]), _P(sinks[1]), 1 | xflag,
                               _P(ws), ws.numel(), stream())


class ConvFn(torch.autograd.Function):
    """nn.Conv2d forward / backward (bias and LeakyReLU/ReLU epilogue optionally fused).

    ``wq`` is the weight in compute dtype and kernel layout [Cout][KH][KW][Cin] (the fp32
    parameter itself or its bf16 shadow); gradients are returned for ``weight``."""

    @staticmethod
    def forward(ctx, x, weight, bias, wq, stride, padding, dilation, act, stats, join=None, fold=(0, False),
                bn_link=None, wg_link=None):
        """``fold = (in_act, out_folded)``: ``in_act`` -- x is the output of a ReLU / LeakyReLU
        whose backward this conv's data gradient applies in its epilogue
        (rtsds_conv2d_dgrad_act); ``out_folded`` -- the single consumer of y does that for this
        conv's own ``act``, so the backward takes dy as the pre-activation gradient.  Set only
        by modules whose intermediate activations have exactly one reader (discriminators)."""
        require_hip(x, weight)
        k, _, kh, kw = weight.shape
        padded = hasattr(x, "_rt_cpad") and is_padded_input(x, _conv_desc(x, k, kh, kw, stride, padding, dilation))
        if not padded:
            x = nhwc(x)
        d = _conv_desc(x, k, kh, kw, stride, padding, dilation)
        y = empty_nhwc(d.n, k, d.ho, d.wo, x.dtype, x.device)
        ws = workspace(lib.rtsds_conv2d_fwd_workspace(ctypes.byref(d)), x.device)
        flag = INPUT_PADDED if padded else 0
        with _Timed(d, "fwd"):
            lib.rtsds_conv2d_fwd(ctypes.byref(d), _P(x), _P(wq), _P(bias), _P(y), act | flag, _P(stats), _P(ws),
                                        ws.numel(), stream())
        ctx.xflag = flag
        ctx.in_act, ctx.out_folded = fold
        ctx.bn_link = bn_link if join is None and not fold[0] else None
        if ctx.in_act and join is not None:
            raise RuntimeError("rtsds_amd: a conv whose input gradient is masked cannot join other readers")
        ctx.d, ctx.act, ctx.has_bias = d, act, bias is not None
        ctx.params = (weight, bias)
        # the following BatchNorm's backward apply fused into this conv's weight gradient
        # (ImgWgradLink): the input needs no gradient, no bias, no activation of our own, and the
        # geometry the kernel takes.  (With side-stream weight gradients on, this one still runs
        # on the backward's own stream, behind the BatchNorm statistics it depends on: the conv has
        # no data-gradient chain to overlap, and both schedules keep computing the same bits.)
        ctx.wg_link = None
        if wg_link is not None:
            wg_link.conv_ok = bool(
                IMG_WGRAD_LINK and not ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and bias is None and not act
                and not fold[0] and not fold[1]
                and lib.rtsds_imgconv_bn_wgrad_workspace(ctypes.byref(d)) > 0)
            if wg_link.conv_ok:
                ctx.wg_link = wg_link
        ctx.join = join
        ctx.save_for_backward(x, wq, y if act else None)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, wq, y = ctx.saved_tensors
        d = ctx.d
        dy = nhwc(dy)
        if dy.dtype != x.dtype:
            dy = cast(dy, x.dtype)
        link = ctx.wg_link
        if link is not None and link.bn is not None:
            # dy is the BatchNorm's incoming gradient: its dx is formed inside the weight gradient
            (bx, coef, bact), link.bn = link.bn, None
            return (None, _img_bn_wgrad(d, x, dy, bx, coef, bact, ctx.params[0], ctx.xflag)) + (None,) * 11
        if ctx.act and not ctx.out_folded:
            g = torch.empty_like(dy)
            lib.rtsds_act_bwd(_P(dy), _P(y), _P(g), dy.numel(), ctx.act, 1.0, dcode(dy), stream())
        else:
            g = dy  # (out_folded: the consumer's dgrad already applied act')
        dx = dw = db = None
        # weight gradient into the optimizer's arena: on the side stream, overlapping the
        # data-gradient chain (runtime.side_fork); forked before the dgrad launch
        wg_side = None
        if ctx.needs_input_grad[1] and side_enabled(d.n * d.ho * d.wo) and CONV_PROFILE is None:
            weight, bias = ctx.params
            sinks = _sinks(weight, bias if ctx.needs_input_grad[2] else None)
            if sinks is not None:
                ws = workspace(lib.rtsds_conv2d_wgrad_workspace(ctypes.byref(d)), x.device)
                side = side_fork(x, g, ws)
                lib.rtsds_conv2d_wgrad(ctypes.byref(d), _P(x), _P(g), _P(sinks[0]), _P(sinks[1]), 1 | ctx.xflag,
                                       _P(ws), ws.numel(), side.cuda_stream)
                wg_side = True
        if ctx.needs_input_grad[0]:
            join = ctx.join
            acc = join is not None and join.buf is not None  # accumulate onto the earlier contribution
            dx = join.buf if acc else empty_nhwc(d.n, d.c, d.h, d.w, x.dtype, x.device)
            ws = workspace(lib.rtsds_conv2d_dgrad_workspace(ctypes.byref(d)), x.device)
            link = ctx.bn_link
            wd, wpk = _dgrad_weight(ctx.params[0], wq, d)
            tiles = 0
            if link is not None and link.src is not None and not acc and g.dtype == torch.bfloat16:
                tiles = lib.rtsds_conv2d_dgrad_bnstats_tiles(ctypes.byref(d))
            with _Timed(d, "dgrad"):
                if tiles:
                    bx, bsm, bsi, bg, bb, bact = link.src
                    part = torch.empty(d.c * tiles * 2, dtype=torch.float32, device=x.device)
                    lib.rtsds_conv2d_dgrad_bnstats(ctypes.byref(d), _P(g), _P(wd), _P(dx), _P(bx), _P(bg), _P(bb),
                                                   _P(bsm), _P(bsi), bact | wpk, _P(part), _P(ws), ws.numel(), stream())
                    link.part, link.nrb = part, tiles
                elif ctx.in_act:
                    lib.rtsds_conv2d_dgrad_act(ctypes.byref(d), _P(g), _P(wd), _P(dx), _P(x), ctx.in_act | wpk,
                                               _P(ws), ws.numel(), stream())
                else:
                    lib.rtsds_conv2d_dgrad(ctypes.byref(d), _P(g), _P(wd), _P(dx), (1 if acc else 0) | wpk, _P(ws),
                                           ws.numel(), stream())
            if join is not None:
                dx = join.put(dx)
        if (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]) and not wg_side:
            weight, bias = ctx.params
            sinks = _sinks(weight, bias if ctx.needs_input_grad[2] else None) if ctx.needs_input_grad[1] else None
            ws = workspace(lib.rtsds_conv2d_wgrad_workspace(ctypes.byref(d)), x.device)
            if sinks is not None:
                _wgrad_into_arena(d, x, g, sinks, ctx.xflag, ws, weight)
                dw = None
                db = None
            else:
                dw = torch.empty((d.k, d.c, d.kh, d.kw), dtype=torch.float32, device=x.device,
                                 memory_format=CL)
                db = torch.empty(d.k, dtype=torch.float32, device=x.device) if ctx.has_bias else None
                with _Timed(d, "wgrad"):
                    lib.rtsds_conv2d_wgrad(ctypes.byref(d), _P(x), _P(g), _P(dw), _P(db), ctx.xflag, _P(ws),
                                                  ws.numel(), stream())
                if not ctx.needs_input_grad[1]:
                    dw = None
        return dx, dw, db, None, None, None, None, None, None, None, None, None, None


def _img_bn_wgrad(d, x, g, bx, coef, act, weight, xflag):
    """rtsds_imgconv_bn_wgrad into the optimizer arena (None returned; reduction deferred to the
    end of the backward pass when allowed) or into a fresh dw."""
    ws = workspace(lib.rtsds_imgconv_bn_wgrad_workspace(ctypes.byref(d)), x.device)
    sinks = _sinks(weight)
    if sinks is not None and DEFER_WGRAD_REDUCE and CONV_PROFILE is None:
        pend = SplitReduceDesc()
        lib.rtsds_imgconv_bn_wgrad_deferred(ctypes.byref(d), _P(x), _P(g), _P(bx), _P(coef), act, _P(sinks[0]),
                                            1 | xflag, _P(ws), ws.numel(), ctypes.byref(pend), stream())
        # keep: the image convs' gradients stay readable after the step (11 k floats; the fused
        # BatchNorm form is checked against them at model level)
        _defer(pend, ws, weight, keep=True)
        return None
    dw = sinks[0] if sinks is not None else torch.empty((d.k, d.c, d.kh, d.kw), dtype=torch.float32,
                                                         device=x.device, memory_format=CL)
    with _Timed(d, "wgrad"):
        lib.rtsds_imgconv_bn_wgrad(ctypes.byref(d), _P(x), _P(g), _P(bx), _P(coef), act, _P(dw),
                                   (1 if sinks is not None else 0) | xflag, _P(ws), ws.numel(), stream())
    return None if sinks is not None else dw


def conv2d(x, weight, bias, wq, stride=(1, 1), padding=(0, 0), dilation=(1, 1), act=0, bn_stats=False,
           join=None, in_act=0, fold_out=False, bn_link=None, wg_link=None):
    """bn_stats=True: the conv epilogue also emits the following BatchNorm's per-tile batch
    statistics, attached to the output as ``_rt_bn_stats`` and consumed by batch_norm().
    ``join``: GradJoin shared with the other readers of ``x``."""
    stats = nrb = None
    if bn_stats and act == 0:
        n, _, h, w = x.shape
        k, _, kh, kw = weight.shape
        d = _conv_desc(x, k, kh, kw, stride, padding, dilation)
        nrb = lib.rtsds_conv2d_fwd_stats_tiles(ctypes.byref(d))
        stats = torch.empty(nrb * k * 4, dtype=torch.float32, device=x.device)  # [k][nrb][4]
    y = ConvFn.apply(x, weight, bias, wq, tuple(stride), tuple(padding), tuple(dilation), act, stats, join,
                     (in_act, bool(fold_out and act in (1, 2))), bn_link, wg_link)
    if stats is not None:
        y._rt_bn_stats = (stats, nrb)
    return y


def _bn_fold(gamma, beta, running_mean, running_var, bias, eps, k):
    """Eval-mode BatchNorm folded with the conv bias into [scale | shift] (rtsds_bn_fold), cached
    on the running-mean tensor: recomputed -- in place, so captured graphs keep reading the
    same buffer -- only when a parameter / statistic changed (tensor versions for torch-side
    writes, runtime.params_epoch for the rtsds optimizer and train-mode BatchNorm, which write
    through raw pointers).  A GraphedForward capture registers the refresh, run before every
    replay."""
    ts = (gamma, beta, running_mean, running_var, bias)

    def key():
        return (params_epoch(), float(eps)) + tuple((t.data_ptr(), t._version) if t is not None else None for t in ts)

    ent = getattr(running_mean, "_rt_fold", None)
    if ent is None or ent[1].numel() != 2 * k or ent[1].device != running_mean.device:
        ent = [None, torch.empty(2 * k, dtype=torch.float32, device=running_mean.device)]
        running_mean._rt_fold = ent
    ss = ent[1]

    def refresh():
        kk = key()
        if ent[0] != kk:
            lib.rtsds_bn_fold(_P(gamma), _P(beta), _P(running_mean), _P(running_var), _P(bias), float(eps), k,
                              _P(ss), ss.data_ptr() + 4 * k, stream())
            ent[0] = kk

    refresh()
    register_fold(refresh)
    return ss


def conv_bn_eval(x, weight, bias, wq, stride, padding, dilation, gamma, beta, running_mean, running_var,
                 eps, act=0, residual=None, out=None):
    """Inference (no autograd) conv -> BatchNorm(running statistics) [-> + residual] [-> act]
    as ONE implicit-GEMM launch: the BN is folded into a per-channel scale / shift of the conv
    epilogue (rtsds_bn_fold + rtsds_conv2d_fwd_bn).  Same function as the unfused
    conv2d -> batch_norm(training=False) chain, with the BN applied to the fp32 accumulators.
    ``out = (buf, off)``: write y straight into channels [off, off + k) of the wider NHWC
    tensor ``buf`` (rtsds_conv2d_fwd_bn_ld) and return that slice as a view; where the kernel
    route does not support it, a plain y is returned (the caller copies)."""
    require_hip(x, weight)
    k, _, kh, kw = weight.shape
    flag = INPUT_PADDED if hasattr(x, "_rt_cpad") and \
        is_padded_input(x, _conv_desc(x, k, kh, kw, stride, padding, dilation)) else 0
    if not flag:
        x = nhwc(x)
    d = _conv_desc(x, k, kh, kw, stride, padding, dilation)
    ss = _bn_fold(gamma, beta, running_mean, running_var, bias, eps, k)
    if residual is not None:
        residual = nhwc(residual)
        if residual.dtype != x.dtype or tuple(residual.shape) != (d.n, k, d.ho, d.wo):
            raise RuntimeError("rtsds_amd.conv_bn_eval: residual must match the conv output")
    ws = workspace(lib.rtsds_conv2d_fwd_workspace(ctypes.byref(d)), x.device)
    if out is not None and residual is None:
        buf, off = out
        if _slice_target(buf, off, (d.n, k, d.ho, d.wo), x.dtype):  # the kernel route checks the 16-B chunks
            try:
                with _Timed(d, "fwd"):
                    lib.rtsds_conv2d_fwd_bn_ld(ctypes.byref(d), _P(x), _P(wq), _P(ss), ss.data_ptr() + 4 * k,
                                               buf.data_ptr() + off * buf.element_size(), buf.shape[1], act | flag,
                                               _P(ws), ws.numel(), stream())
                return buf[:, off:off + k]
            except RuntimeError as e:
                if "unsupported" not in str(e):
                    raise
    y = empty_nhwc(d.n, k, d.ho, d.wo, x.dtype, x.device)
    with _Timed(d, "fwd"):
        lib.rtsds_conv2d_fwd_bn(ctypes.byref(d), _P(x), _P(wq), _P(ss), ss.data_ptr() + 4 * k, _P(residual), _P(y),
                                act | flag, _P(ws), ws.numel(), stream())
    return y


def conv_bn_maxpool_eval(x, weight, bias, wq, stride, padding, dilation, gamma, beta, running_mean, running_var, eps,
                         act, pool_k, pool_s, pool_p, ceil_mode):
    """Inference stem: pool(act(bn(conv(x)))) with the BN folded and the 3x3 stride-2 pool in
    the conv's epilogue (rtsds_conv2d_fwd_bn_maxpool; the full-resolution activation is never
    written).  None where that route does not apply (the caller runs the separate ops)."""
    require_hip(x, weight)
    if pool_k != 3 or pool_s != 2 or x.dtype != torch.bfloat16:
        return None
    k, _, kh, kw = weight.shape
    flag = INPUT_PADDED if hasattr(x, "_rt_cpad") and \
        is_padded_input(x, _conv_desc(x, k, kh, kw, stride, padding, dilation)) else 0
    if not flag:
        x = nhwc(x)
    d = _conv_desc(x, k, kh, kw, stride, padding, dilation)
    hp, wp = pool_out(d.ho, 3, 2, pool_p, ceil_mode), pool_out(d.wo, 3, 2, pool_p, ceil_mode)
    ss = _bn_fold(gamma, beta, running_mean, running_var, bias, eps, k)
    y = empty_nhwc(d.n, k, hp, wp, x.dtype, x.device)
    ws = workspace(lib.rtsds_conv2d_fwd_workspace(ctypes.byref(d)), x.device)
    try:
        with _Timed(d, "fwd"):
            lib.rtsds_conv2d_fwd_bn_maxpool(ctypes.byref(d), _P(x), _P(wq), _P(ss), ss.data_ptr() + 4 * k, _P(y),
                                            act | flag, hp, wp, pool_p, _P(ws), ws.numel(), stream())
    except RuntimeError as e:
        if "unsupported" in str(e):  # not the stem geometry: the separate ops
            return None
        raise
    return y


class ConvSumFn(torch.autograd.Function):
    """sum_i conv_i(x) + bias_i over convs sharing x and output shape (ASPP,
    deeplabv2.py:62-66): one output buffer accumulated in the GEMM epilogue; the backward
    accumulates all dgrads into one dx."""

    @staticmethod
    def forward(ctx, x, geoms, *wb):
        require_hip(x)
        x = nhwc(x)
        m = len(geoms)
        weights, biases, wqs = wb[:m], wb[m:2 * m], wb[2 * m:]
        descs = []
        y = None
        for i, (stride, padding, dilation) in enumerate(geoms):
            k, _, kh, kw = weights[i].shape
            d = _conv_desc(x, k, kh, kw, stride, padding, dilation)
            if y is None:
                y = empty_nhwc(d.n, k, d.ho, d.wo, x.dtype, x.device)
            ws = workspace(lib.rtsds_conv2d_fwd_workspace(ctypes.byref(d)), x.device)
            with _Timed(d, "fwd"):
                lib.rtsds_conv2d_fwd(ctypes.byref(d), _P(x), _P(wqs[i]), _P(biases[i]), _P(y),
                                     0x100 if i else 0, None, _P(ws), ws.numel(), stream())
            descs.append(d)
        ctx.descs = descs
        ctx.params = tuple(weights) + tuple(biases)
        ctx.has_bias = [b is not None for b in biases]
        ctx.save_for_backward(x, *wqs)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, *wqs = ctx.saved_tensors
        dy = nhwc(dy)
        m = len(wqs)
        dx = None
        dws, dbs = [None] * m, [None] * m
        for i, d in enumerate(ctx.descs):
            if ctx.needs_input_grad[0]:
                if dx is None:
                    dx = empty_nhwc(d.n, d.c, d.h, d.w, x.dtype, x.device)
                ws = workspace(lib.rtsds_conv2d_dgrad_workspace(ctypes.byref(d)), x.device)
                wd, wpk = _dgrad_weight(ctx.params[i], wqs[i], d)
                with _Timed(d, "dgrad"):
                    lib.rtsds_conv2d_dgrad(ctypes.byref(d), _P(dy), _P(wd), _P(dx), (1 if i else 0) | wpk,
                                           _P(ws), ws.numel(), stream())
            if ctx.needs_input_grad[2 + i] or ctx.needs_input_grad[2 + m + i]:
                w_i, b_i = ctx.params[i], ctx.params[m + i]
                sinks = (_sinks(w_i, b_i if ctx.needs_input_grad[2 + m + i] else None)
                         if ctx.needs_input_grad[2 + i] else None)
                ws = workspace(lib.rtsds_conv2d_wgrad_workspace(ctypes.byref(d)), x.device)
                if sinks is not None:
                    with _Timed(d, "wgrad"):
                        lib.rtsds_conv2d_wgrad(ctypes.byref(d), _P(x), _P(dy), _P(sinks[0]), _P(sinks[1]),
                                               1, _P(ws), ws.numel(), stream())
                    continue
                dw = torch.empty((d.k, d.c, d.kh, d.kw), dtype=torch.float32, device=x.device,
                                 memory_format=CL)
                db = torch.empty(d.k, dtype=torch.float32, device=x.device) if ctx.has_bias[i] else None
                with _Timed(d, "wgrad"):
                    lib.rtsds_conv2d_wgrad(ctypes.byref(d), _P(x), _P(dy), _P(dw), _P(db), 0, _P(ws),
                                           ws.numel(), stream())
                dws[i] = dw if ctx.needs_input_grad[2 + i] else None
                dbs[i] = db
        return (dx, None, *dws, *dbs, *([None] * m))


# ----------------------------------------------------------------------------- batch norm
BN_BWD_LINK = True  # False: every BatchNorm backward computes its own statistics (A/B tests)


class BnBwdLink:
    """Hands a train-mode BatchNorm's backward statistics from the data gradient of the conv
    that reads its (activated) output to the BatchNorm's backward, which then skips its own
    statistics pass (rtsds_conv2d_dgrad_bnstats -> rtsds_bn_bwd_part).  Created by a module
    whose BatchNorm output has exactly that one reader (ResNet BasicBlock bn1 -> conv2,
    Bottleneck bn1 -> conv2 -> bn2 -> conv3); ignored wherever a route does not apply."""

    __slots__ = ("src", "part", "nrb")

    def __init__(self):
        self.src = None   # (bn input x, save_mean, save_invstd, gamma, beta, act), set by the BN forward
        self.part = None  # set by the conv backward, consumed by the BN backward
        self.nrb = 0


IMG_WGRAD_LINK = True  # False: the image convs' BatchNorms write dx and the conv reads it back (A/B tests)


class ImgWgradLink:
    """Joins a train-mode BatchNorm's backward to the weight gradient of the 3-channel image
    conv that produced its input (ResNet stem, spatial path's first block): the conv input needs
    no gradient, so the BatchNorm's dx has that weight gradient as its only reader.  The
    BatchNorm backward then runs its statistics and finalize only (rtsds_bn_bwd_coef), leaves
    ``(x, coef, act)`` here and returns its incoming gradient in place of dx; the conv backward
    forms dx per tile inside the weight-gradient kernel (rtsds_imgconv_bn_wgrad).  Created by
    nn.conv_bn / nn.conv_bn_relu_maxpool, whose conv output has the BatchNorm as its only
    reader; the conv forward arms it when its geometry and situation qualify, the BatchNorm
    forward accepts it when its own do.  Everything else runs the separate passes."""

    __slots__ = ("conv_ok", "bn")

    def __init__(self):
        self.conv_ok = False  # set by the conv forward
        self.bn = None        # (bn input x, coef, act), set by the BatchNorm backward

    def take(self, x, training, act):
        """The link, if armed and the BatchNorm on ``x`` qualifies (BatchNorm forward)."""
        if IMG_WGRAD_LINK and self.conv_ok and training and act in (0, 1, 2) and x.dtype == torch.bfloat16 \
                and not getattr(x, "_backward_hooks", None):
            return self
        return None


def _bn_bwd_coef(ctx_link, dy, x, dg, db, rows, c, gamma, beta, sm, si, training, act, acc):
    """Statistics + finalize of a linked BatchNorm backward; the coefficients go to the link."""
    coef = torch.empty(6 * c, dtype=torch.float32, device=x.device)
    ws = workspace(lib.rtsds_bn_workspace(rows, c), x.device)
    lib.rtsds_bn_bwd_coef(_P(dy), _P(x), _P(dg), _P(db), _P(coef), rows, c, _P(gamma), _P(beta), _P(sm), _P(si),
                          training, act, acc, dcode(x), _P(ws), ws.numel(), stream())
    ctx_link.bn = (x, coef, act)


# True: the two BatchNorms that end a residual block with a downsample branch run as one
# BatchNormPairFn (nn.res_block_tail); False: as two BatchNormFns (A/B tests)
RES_BN_PAIR = True
# True: every other training-mode residual BatchNorm + ReLU keeps mask bits for its backward instead
# of its output (rtsds_bn_fwd_bits / rtsds_bn_bwd_bits).  Off: on its own it measured no faster than
# keeping y.
RES_BN_BITS = False


def _res_bits_ok(x, res, training, act):
    """Whether a BatchNorm on NHWC ``x`` with residual ``res`` can keep mask bits instead of its output
    (rtsds_bn_fwd_bits, rtsds_bn_pair_fwd): training mode, ReLU, bf16 / fp32, whole 16-byte channel
    vectors, one shape."""
    return (training and res is not None and act == ACT_RELU and x.shape[1] % 8 == 0
            and x.dtype in (torch.bfloat16, torch.float32) and res.dtype == x.dtype and res.shape == x.shape)


class BatchNormFn(torch.autograd.Function):
    """BatchNorm2d (+ residual add) (+ ReLU/LeakyReLU) fused, train or eval statistics."""

    @staticmethod
    def forward(ctx, x, gamma, beta, res, running_mean, running_var, training, momentum, eps, act,
                stats, stats_nrb, nbt, res_join=None, link=None, out=None, wg_link=None):
        require_hip(x)
        x = nhwc(x)
        if res is not None:
            res = nhwc(res)
        n, c, h, w = x.shape
        rows = n * h * w
        keep_y = res is not None or act == ACT_SIGMOID
        ld = c
        if out is not None and not keep_y and x.dtype == torch.bfloat16 and \
                _slice_target(out[0], out[1], x.shape, x.dtype, vec16=True):
            # y written straight into channels [off, off + c) of out's NHWC buffer (a view)
            buf, off = out
            ld = buf.shape[1]
            y = buf[:, off:off + c]
        else:
            y = torch.empty_like(x, memory_format=CL)
        sm = torch.empty(c, dtype=torch.float32, device=x.device)
        si = torch.empty(c, dtype=torch.float32, device=x.device)
        ws = workspace(lib.rtsds_bn_workspace(rows, c), x.device)
        # A residual BatchNorm + ReLU whose backward wants both gradients keeps one mask bit per
        # element instead of y (the backward statistics pass then reads a byte per channel vector
        # in place of the y vector; same bits everywhere).
        bits = None
        if RES_BN_BITS and _res_bits_ok(x, res, training, act) and ctx.needs_input_grad[0] \
                and ctx.needs_input_grad[3]:
            bits = torch.empty(lib.rtsds_bn_bits_bytes(rows, c, dcode(x)), dtype=torch.uint8, device=x.device)
            lib.rtsds_bn_fwd_bits(_P(x), _P(res), _P(y), _P(bits), rows, c, _P(gamma), _P(beta), _P(running_mean),
                                  _P(running_var), _P(nbt), _P(sm), _P(si), float(momentum), float(eps), _P(stats),
                                  int(stats_nrb or 0), dcode(x), _P(ws), ws.numel(), stream())
        else:
            lib.rtsds_bn_fwd_ld(_P(x), _P(res), _P(y), ld, rows, c, _P(gamma), _P(beta), _P(running_mean),
                                _P(running_var), _P(nbt), _P(sm), _P(si), float(momentum), float(eps), int(training),
                                act, _P(stats) if training else None, int(stats_nrb or 0), dcode(x), _P(ws),
                                ws.numel(), stream())
        ctx.meta = (rows, c, int(training), act, res is not None)
        ctx.gamma, ctx.beta = gamma, beta
        ctx.res_join = res_join
        ctx.has_bits = bits is not None
        # Without a residual the ReLU/LeakyReLU mask is recomputed from x in the backward
        # (bit-identical pre-activation), so y is neither kept nor re-read.
        ctx.save_for_backward(x, bits if bits is not None else (y if keep_y else None), gamma, beta, sm, si)
        ctx.link = None
        if link is not None and BN_BWD_LINK and training and res is None and act in (0, 1, 2) \
                and x.dtype == torch.bfloat16 and c % 8 == 0:
            link.src, link.part = (x, sm, si, gamma, beta, act), None
            ctx.link = link
        ctx.wg_link = wg_link if res is None else None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, beta, sm, si = ctx.saved_tensors
        rows, c, training, act, has_res = ctx.meta
        ldy = _channel_slice_pitch(dy) if ctx.link is None else 0
        if not ldy:
            dy = nhwc(dy)
            ldy = c
        need_dx, need_r = ctx.needs_input_grad[0], ctx.needs_input_grad[3]
        if ctx.wg_link is not None and need_dx and ldy == c and dy.dtype == x.dtype:
            # dx is formed inside the image conv's weight gradient: hand it our incoming gradient
            dg, db, acc = _bn_param_grads(ctx, c, x.device)
            _bn_bwd_coef(ctx.wg_link, dy, x, dg, db, rows, c, gamma, beta, sm, si, training, act, acc)
            if acc:
                dg = db = None
            return (dy, dg, db) + (None,) * 14
        dx = torch.empty_like(x, memory_format=CL) if need_dx else None
        dres = torch.empty_like(x, memory_format=CL) if (has_res and need_r) else None
        dg, db, acc = _bn_param_grads(ctx, c, x.device)
        ws = workspace(lib.rtsds_bn_workspace(rows, c), x.device)
        link = ctx.link
        if ctx.has_bits:  # (y: the mask bits)
            lib.rtsds_bn_bwd_bits(_P(dy), ldy, _P(x), _P(y), _P(dx), _P(dres), _P(dg), _P(db), rows, c, _P(gamma),
                                  _P(beta), _P(sm), _P(si), acc, dcode(x), _P(ws), ws.numel(), stream())
        elif link is not None and link.part is not None and dy.dtype == x.dtype:
            # statistics from the reading conv's data-gradient epilogue
            lib.rtsds_bn_bwd_part(_P(dy), _P(x), _P(dx), _P(dg), _P(db), rows, c, _P(gamma), _P(beta), _P(sm),
                                  _P(si), training, act, acc, _P(link.part), link.nrb, dcode(x), _P(ws), ws.numel(),
                                  stream())
        else:
            lib.rtsds_bn_bwd_ld(_P(dy), ldy, _P(x), _P(y), _P(dx), _P(dres), _P(dg), _P(db), rows, c,
                                _P(gamma), _P(beta), _P(sm), _P(si), training, act, acc, dcode(x), _P(ws), ws.numel(),
                                stream())
        if link is not None:
            link.src = link.part = None
        if acc:
            dg = db = None
        if dres is not None:
            dres = _join_add(ctx.res_join, dres)
        return dx, dg, db, dres, None, None, None, None, None, None, None, None, None, None, None, None, None


def _nhwc_pitch(t):
    """Channel pitch of a 4-D [N, C, H, W] tensor or view stored NHWC with dense rows and images
    (its C channels may be a slice of a wider pixel), else 0."""
    n, c, h, w = t.shape
    ld = t.stride(3)
    if t.stride(1) != 1 or ld < c or (h > 1 and t.stride(2) != w * ld) or (n > 1 and t.stride(0) != h * w * ld):
        return 0
    return ld


def _slice_target(buf, off, shape, dtype, vec16=False):
    """Whether channels [off, off + c) of ``buf`` can take an [n, c, h, w] = ``shape`` result of
    ``dtype`` through a pitched NHWC store: same n, h, w and dtype, the slice inside buf's
    channels, buf dense NHWC.  ``vec16``: the kernel stores 16-byte vectors, so off, c and the
    pitch are multiples of the vector and the slice starts 16-byte aligned."""
    n, c, h, w = shape
    if buf.dim() != 4 or buf.dtype != dtype or (buf.shape[0], buf.shape[2], buf.shape[3]) != (n, h, w):
        return False
    ld = buf.shape[1]
    if off < 0 or off + c > ld or _nhwc_pitch(buf) != ld:
        return False
    if vec16:
        vec = 16 // buf.element_size()
        if off % vec or c % vec or ld % vec or (buf.data_ptr() + off * buf.element_size()) % 16:
            return False
    return True


def _channel_slice_pitch(t):
    """Row pitch of a bf16 [N, C, H, W] view that is a channel slice of a wider NHWC buffer
    (C % 8 == 0, pitch % 8 == 0, pitch > C), else 0."""
    if t.dim() != 4 or t.dtype != torch.bfloat16:
        return 0
    ld = _nhwc_pitch(t)
    if ld <= t.shape[1] or t.shape[1] % 8 or ld % 8 or t.data_ptr() % 16:
        return 0
    return ld


def _bn_epilogue_stats(x, training, running_mean):
    """(stats, nrb) a producing conv attached to ``x`` for a training-mode BatchNorm, else (None, None);
    also notes that the call is about to change the running statistics."""
    st = getattr(x, "_rt_bn_stats", None) if training else None
    if training and running_mean is not None:
        bump_params_epoch()  # running statistics change (raw-pointer write)
    return st if st is not None else (None, None)


def batch_norm(x, gamma, beta, running_mean, running_var, training, momentum, eps, act=0,
               residual=None, num_batches_tracked=None, res_join=None, link=None, out=None, wg_link=None):
    """``num_batches_tracked`` (int64, optional) is incremented by the finalize kernel.
    ``res_join``: GradJoin shared with the other readers of ``residual``.  ``out``: (NHWC
    buffer, channel offset) to write y into (a view of it is returned; bf16 without residual).
    ``wg_link``: ImgWgradLink of the image conv that produced ``x``."""
    stats, nrb = _bn_epilogue_stats(x, training, running_mean)
    if wg_link is not None:
        wg_link = wg_link.take(x, training and residual is None, act)
    return BatchNormFn.apply(x, gamma, beta, residual, running_mean, running_var, training,
                             momentum, eps, act, stats, nrb, num_batches_tracked, res_join, link, out, wg_link)


class BatchNormPairFn(torch.autograd.Function):
    """relu(bnA(xa) + bnB(xb)) for the end of a residual block with a downsample branch: xa the raw
    output of the block's last conv, xb of its downsample conv, both [N, C, H, W] of one shape.
    Stands for BatchNormFn(xb) -> BatchNormFn(xa, residual = that) in training mode with the same
    bits (rtsds_bn_pair_fwd / rtsds_bn_pair_bwd): three launches per direction instead of six, the
    skip tensor and its gradient never stored.  ``pa`` / ``pb``: (running_mean, running_var,
    num_batches_tracked, momentum, eps, stats, stats_nrb) of each BatchNorm."""

    @staticmethod
    def forward(ctx, xa, xb, ga, ba, gb, bb, pa, pb):
        require_hip(xa)
        xa, xb = nhwc(xa), nhwc(xb)
        n, c, h, w = xa.shape
        rows = n * h * w
        y = torch.empty_like(xa, memory_format=CL)
        bits = torch.empty(lib.rtsds_bn_bits_bytes(rows, c, dcode(xa)), dtype=torch.uint8, device=xa.device)
        sv = [torch.empty(c, dtype=torch.float32, device=xa.device) for _ in range(4)]
        ws = workspace(lib.rtsds_bn_pair_workspace(rows, c), xa.device)
        qa = BnParams(_P(ga), _P(ba), _P(pa[0]), _P(pa[1]), _P(pa[2]), _P(sv[0]), _P(sv[1]), float(pa[3]), float(pa[4]),
                      _P(pa[5]), int(pa[6] or 0), 0, None, None)
        qb = BnParams(_P(gb), _P(bb), _P(pb[0]), _P(pb[1]), _P(pb[2]), _P(sv[2]), _P(sv[3]), float(pb[3]), float(pb[4]),
                      _P(pb[5]), int(pb[6] or 0), 0, None, None)
        lib.rtsds_bn_pair_fwd(_P(xa), _P(xb), _P(y), _P(bits), rows, c, ctypes.byref(qa), ctypes.byref(qb), dcode(xa),
                              _P(ws), ws.numel(), stream())
        ctx.meta = (rows, c)
        ctx.params = (ga, ba, gb, bb)
        ctx.save_for_backward(xa, xb, bits, ga, ba, gb, bb, *sv)
        return y

    @staticmethod
    def backward(ctx, dy):
        xa, xb, bits, ga, ba, gb, bb, sma, sia, smb, sib = ctx.saved_tensors
        rows, c = ctx.meta
        ldy = _channel_slice_pitch(dy)
        if not ldy:
            dy = nhwc(dy)
            ldy = c
        need = ctx.needs_input_grad
        dxa = torch.empty_like(xa, memory_format=CL)
        dxb = torch.empty_like(xb, memory_format=CL)
        dga, dba, acca = _bn_grads_of(ctx.params[0], ctx.params[1], need[2], need[3], c, xa.device)
        dgb, dbb, accb = _bn_grads_of(ctx.params[2], ctx.params[3], need[4], need[5], c, xa.device)
        ws = workspace(lib.rtsds_bn_pair_workspace(rows, c), xa.device)
        qa = BnParams(_P(ga), _P(ba), None, None, None, _P(sma), _P(sia), 0.0, 0.0, None, 0, acca, _P(dga), _P(dba))
        qb = BnParams(_P(gb), _P(bb), None, None, None, _P(smb), _P(sib), 0.0, 0.0, None, 0, accb, _P(dgb), _P(dbb))
        lib.rtsds_bn_pair_bwd(_P(dy), ldy, _P(xa), _P(xb), _P(bits), _P(dxa), _P(dxb), rows, c, ctypes.byref(qa),
                              ctypes.byref(qb), dcode(xa), _P(ws), ws.numel(), stream())
        if acca:
            dga = dba = None
        if accb:
            dgb = dbb = None
        return dxa, dxb, dga, dba, dgb, dbb, None, None


def batch_norm_pair(xa, bn_a, xb, bn_b, training, act=ACT_RELU):
    """act(bnA(xa) + bnB(xb)), the two BatchNorms that end a residual block with a downsample
    branch.  ``bn_a`` / ``bn_b``: (gamma, beta, running_mean, running_var, momentum, eps,
    num_batches_tracked) of each.  Training mode with ReLU, bf16 / fp32, one shape, c % 8 == 0
    and gradients wanted for both inputs: one BatchNormPairFn; everything else runs the chain
    batch_norm(xb) -> batch_norm(xa, residual=...).  The results are the same bits either way."""
    ga, ba, rma, rva, moma, epsa, nbta = bn_a
    gb, bb, rmb, rvb, momb, epsb, nbtb = bn_b
    if RES_BN_PAIR and xa.dim() == 4 and _res_bits_ok(xa, xb, training, act) and torch.is_grad_enabled() \
            and xa.requires_grad and xb.requires_grad and xa.is_cuda:
        sa, na = _bn_epilogue_stats(xa, training, rma)
        sb, nb = _bn_epilogue_stats(xb, training, rmb)
        return BatchNormPairFn.apply(xa, xb, ga, ba, gb, bb, (rma, rva, nbta, moma, epsa, sa, na),
                                     (rmb, rvb, nbtb, momb, epsb, sb, nb))
    skip = batch_norm(xb, gb, bb, rmb, rvb, training, momb, epsb, 0, None, nbtb)
    return batch_norm(xa, ga, ba, rma, rva, training, moma, epsa, act, skip, nbta)


# ----------------------------------------------------------------------------- layout / dtype
def pack_input(x, dtype):
    """NCHW fp32 batch (reference loaders, reference-layout activations) -> NHWC compute dtype.
    Differentiable when ``x`` requires grad (discriminator / UpSampler inputs): the gradient
    goes back as the NHWC tensor cast to x's dtype (same logical NCHW shape)."""
    require_hip(x)
    if x.dtype == dtype and x.dim() == 4 and (x.is_contiguous(memory_format=CL) and x.shape[1] > 1 or is_padded_input(x)):
        return x
    if x.requires_grad and torch.is_grad_enabled():
        return PackInputFn.apply(x, dtype)
    return _pack(x, dtype)


class PackInputFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype):
        ctx.xdtype = x.dtype
        return _pack(x, dtype)

    @staticmethod
    def backward(ctx, dy):
        return cast(nhwc(dy), ctx.xdtype), None


def pack_input_into(x, y):
    """pack_input(x, y.dtype) written into the existing packed tensor ``y`` (same shape): a
    captured graph's input buffer refilled with one pass over x."""
    require_hip(x)
    xf = (x if x.dtype == torch.float32 else cast(x, torch.float32)).contiguous()
    n, c, h, w = xf.shape
    if tuple(y.shape) != (n, c, h, w):
        raise RuntimeError("rtsds_amd.pack_input_into: shape mismatch")
    if is_padded_input(y):
        lib.rtsds_nchw_to_nhwc_pad(_P(xf), _P(y), n, c, h, w, y._rt_cpad, 0 if y.dtype == torch.float32 else 1, stream())
    elif y.is_contiguous(memory_format=CL):
        lib.rtsds_nchw_to_nhwc(_P(xf), _P(y), n, c, h, w, 0 if y.dtype == torch.float32 else 1, stream())
    else:
        raise RuntimeError("rtsds_amd.pack_input_into: y is not a packed input")
    return y


def _pack(x, dtype):
    xf = x if x.dtype == torch.float32 else cast(x, torch.float32)
    xf = xf.contiguous()
    n, c, h, w = xf.shape
    if c == 3 and dtype == torch.bfloat16:
        # the image in the 4-channel pitch of its convs' superpixel gathers (stem / spatial
        # path, RTSDS_INPUT_PADDED): they skip their own pad pass; other readers see a
        # [N, 3, H, W] tensor (non-conv readers make an NHWC copy via nhwc())
        buf = torch.empty((n, h, w, 4), dtype=dtype, device=x.device)
        lib.rtsds_nchw_to_nhwc_pad(_P(xf), _P(buf), n, c, h, w, 4, 1, stream())
        y = buf.permute(0, 3, 1, 2)[:, :3]
        y._rt_cpad = 4
        return y
    y = empty_nhwc(n, c, h, w, dtype, x.device)
    lib.rtsds_nchw_to_nhwc(_P(xf), _P(y), n, c, h, w, 0 if dtype == torch.float32 else 1, stream())
    return y


def cast(t, dtype):
    """dtype conversion on device, preserving the memory layout."""
    if t.dtype == dtype:
        return t
    out = torch.empty_like(t, dtype=dtype)
    if not (t.is_contiguous() or t.is_contiguous(memory_format=CL)):
        raise RuntimeError("rtsds_amd.cast: dense tensor required")
    if out.stride() != t.stride():
        raise RuntimeError("rtsds_amd.cast: layout mismatch")
    lib.rtsds_cast(_P(t), dcode(t), _P(out), dcode(out), t.numel(), stream())
    return out


class CatFn(torch.autograd.Function):
    """torch.cat(dim=1) of NHWC tensors (build_bisenet.py:72,153).  ``joins[i]``: GradJoin of
    input i when it has other readers (the split slice is accumulated into their gradient)."""

    @staticmethod
    def forward(ctx, joins, *xs):
        xs = [nhwc(x) for x in xs]
        n, _, h, w = xs[0].shape
        ct = sum(x.shape[1] for x in xs)
        y = empty_nhwc(n, ct, h, w, xs[0].dtype, xs[0].device)
        off = 0
        for x in xs:
            c = x.shape[1]
            lib.rtsds_copy_channels(_P(x), c, 0, _P(y), ct, off, n * h * w, c, 0, dcode(x), stream())
            off += c
        ctx.split = [x.shape[1] for x in xs]
        ctx.joins = joins
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = nhwc(dy)
        n, ct, h, w = dy.shape
        outs, off = [None], 0
        for i, c in enumerate(ctx.split):
            if ctx.needs_input_grad[1 + i]:
                join = ctx.joins[i] if ctx.joins else None
                acc = join is not None and join.buf is not None
                g = join.buf if acc else empty_nhwc(n, c, h, w, dy.dtype, dy.device)
                lib.rtsds_copy_channels(_P(dy), ct, off, _P(g), c, 0, n * h * w, c, 1 if acc else 0, dcode(dy),
                                        stream())
                outs.append(join.put(g) if join is not None else g)
            else:
                outs.append(None)
            off += c
        return tuple(outs)


class CatResizeFn(torch.autograd.Function):
    """cat([x0] + [interpolate_bilinear(x, size) for x in xs], dim=1) (build_bisenet.py:151-153
    and the FFM's cat, :72) with each resize written straight into its channel slice of the
    output (rtsds_bilinear_fwd's output pitch / offset) and, backward, each resize's gradient
    read straight from its slice of dy (rtsds_bilinear_bwd's input pitch / offset): neither the
    resized maps nor their gradients exist on their own; x0 (already at ``size``) is the one
    copy each way.  ``joins[k]``: GradJoin of xs[k]'s readers (BiSeNet's cx1 / cx2 also feed the
    supervision convs, whose data gradients then accumulate into the resize adjoint's buffer)."""

    @staticmethod
    def forward(ctx, size, joins, into, x0, *xs):
        xs = [nhwc(x) for x in xs]
        ct = x0.shape[1] + sum(x.shape[1] for x in xs)
        # x0 already written as channels [0, c0) of ``into`` (its producer's pitched store): no copy
        ctx.x0_in_place = into is not None and tuple(into.shape[1:]) == (ct,) + tuple(x0.shape[2:]) and \
            x0.data_ptr() == into.data_ptr() and _channel_slice_pitch(x0) == ct
        if not ctx.x0_in_place:
            x0 = nhwc(x0)
        n, c0, h, w = x0.shape
        if (h, w) != (int(size[0]), int(size[1])):
            raise RuntimeError("rtsds_amd.concat_resized: x0 must have the target size")
        y = into if ctx.x0_in_place else empty_nhwc(n, ct, h, w, x0.dtype, x0.device)
        if not ctx.x0_in_place:
            lib.rtsds_copy_channels(_P(x0), c0, 0, _P(y), ct, 0, n * h * w, c0, 0, dcode(x0), stream())
        off, geos = c0, []
        for x in xs:
            _, c, hi, wi = x.shape
            ho, wo, sh, sw = upsample_geometry(x, size=size)
            lib.rtsds_bilinear_fwd(_P(x), _P(y), n, hi, wi, c, ho, wo, sh, sw, ct, off, dcode(x), stream())
            geos.append((off, c, hi, wi, ho, wo, sh, sw))
            off += c
        ctx.meta = (n, c0, h, w, ct, geos)
        ctx.joins = joins
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c0, h, w, ct, geos = ctx.meta
        dy = nhwc(dy)
        grads = [None, None, None, None]
        if ctx.needs_input_grad[3]:
            if ctx.x0_in_place:  # x0's producer reads its gradient from the slice in place
                grads[3] = dy[:, :c0]
            else:
                g0 = empty_nhwc(n, c0, h, w, dy.dtype, dy.device)
                lib.rtsds_copy_channels(_P(dy), ct, 0, _P(g0), c0, 0, n * h * w, c0, 0, dcode(dy), stream())
                grads[3] = g0
        for k, (off, c, hi, wi, ho, wo, sh, sw) in enumerate(geos):
            if not ctx.needs_input_grad[4 + k]:
                grads.append(None)
                continue
            dx = empty_nhwc(n, c, hi, wi, dy.dtype, dy.device)
            ws = workspace(lib.rtsds_bilinear_bwd_workspace(n, hi, wi, c, ho, wo), dy.device)
            lib.rtsds_bilinear_bwd(_P(dy), _P(dx), n, hi, wi, c, ho, wo, sh, sw, ct, off, dcode(dy), _P(ws),
                                   ws.numel(), stream())
            # first contribution: the other reader accumulates into dx (otherwise one add)
            grads.append(_join_add(ctx.joins[k], dx) if ctx.joins else dx)
        return tuple(grads)


def concat_resized(x0, xs, size, joins=None, into=None):
    """cat([x0] + [interpolate_bilinear(x, size) for x in xs], dim=1) without materialising the
    resized maps (CatResizeFn).  ``joins``: per-xs GradJoin (or None) for inputs with other readers.
    ``into``: the preallocated NHWC output; when x0 already is its leading channel slice (e.g.
    written there by nn.conv_bn(out=...)), x0 is neither copied in nor its gradient copied out."""
    return CatResizeFn.apply((int(size[0]), int(size[1])), tuple(joins) if joins else None, into, x0, *xs)


def concat_resized_scaled_eval(x0, parts, size, into=None):
    """Inference only: concat_resized(x0, [channel_scale(...channel_scale(x, s1)..., sk) for
    (x, (s1, ...)) in parts], size) with the (at most two) channel scales applied to the resize's
    taps (rtsds_bilinear_fwd_scaled; bit-identical to the separate ops).  None when a part's
    geometry is outside the fused kernel (the caller then runs the separate ops).  ``into``: the
    preallocated output; x0 is not copied when it already is its leading channel slice (the
    spatial path's conv wrote it there, conv_bn_eval(out=...))."""
    n, c0, h, w = x0.shape
    ps = []
    for x, scales in parts:
        x = nhwc(x)
        if len(scales) > 2 or x.shape[-2] > h or x.shape[-1] > w:
            return None
        ss = [(s if s.dtype == x.dtype else cast(s, x.dtype)).contiguous() for s in scales]
        ps.append((x, ss + [None] * (2 - len(ss))))
    ct = c0 + sum(x.shape[1] for x, _ in ps)
    if into is not None and _slice_target(into, 0, (n, ct, h, w), x0.dtype) and into.shape[1] == ct:
        y = into
        in_place = x0.data_ptr() == into.data_ptr() and x0.stride() == into.stride()
    else:
        y, in_place = empty_nhwc(n, ct, h, w, x0.dtype, x0.device), False
    if not in_place:
        x0 = nhwc(x0)
    off = c0
    for x, (s1, s2) in ps:
        _, c, hi, wi = x.shape
        ho, wo, sh, sw = upsample_geometry(x, size=size)
        try:
            lib.rtsds_bilinear_fwd_scaled(_P(x), _P(s1), _P(s2), _P(y), n, hi, wi, c, ho, wo, sh, sw, ct, off, dcode(x), stream())
        except RuntimeError as e:
            if "unsupported" in str(e):
                return None
            raise
        off += c
    if not in_place:
        lib.rtsds_copy_channels(_P(x0), c0, 0, _P(y), ct, 0, n * h * w, c0, 0, dcode(x0), stream())
    return y


def ffm_head_eval(feature, w1, b1, w2, b2, w3, b3):
    """Inference only: conv3(f * a + f) + b3 with a = sigmoid(conv2(relu(conv1(GAP(f)) + b1)) + b2)
    -- FeatureFusionModule's attention tail and BiSeNet's final 1x1 conv (build_bisenet.py:75-80,
    167) in one launch (rtsds_ffm_head_eval).  w*: [c, c, 1, 1] weights in the feature's dtype."""
    f = nhwc(feature)
    n, c, h, w = f.shape
    out = empty_nhwc(n, c, h, w, f.dtype, f.device)
    ws = [t.reshape(c, c).contiguous() for t in (w1, w2, w3)]
    bs = [None if b is None else b.float().contiguous() for b in (b1, b2, b3)]
    wk = workspace(lib.rtsds_ffm_head_eval_workspace(n, h * w, c), f.device)
    lib.rtsds_ffm_head_eval(_P(f), _P(ws[0]), _P(bs[0]), _P(ws[1]), _P(bs[1]), _P(ws[2]), _P(bs[2]), _P(out), n, h * w, c,
                            dcode(f), _P(wk), wk.numel(), stream())
    return out


def cat(xs, joins=None):
    """``joins``: per-input GradJoin (or None) for inputs that have other readers."""
    return CatFn.apply(joins, *xs)


# ----------------------------------------------------------------------------- pointwise
class ActFn(torch.autograd.Function):
    """ReLU (1) / LeakyReLU(0.2) (2) / sigmoid (3)."""

    @staticmethod
    def forward(ctx, x, act):
        require_hip(x)
        x = x.contiguous(memory_format=CL) if x.dim() == 4 else x.contiguous()
        y = torch.empty_like(x)
        lib.rtsds_act_fwd(_P(x), _P(y), x.numel(), act, dcode(x), stream())
        ctx.act = act
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = dy.contiguous(memory_format=CL) if dy.dim() == 4 else dy.contiguous()
        dx = torch.empty_like(y)
        lib.rtsds_act_bwd(_P(dy), _P(y), _P(dx), y.numel(), ctx.act, 1.0, dcode(y), stream())
        return dx, None


def relu(x):
    return ActFn.apply(x, 1)


def leaky_relu(x):
    return ActFn.apply(x, 2)


def sigmoid(x):
    return ActFn.apply(x, 3)


class GradReverseFn(torch.autograd.Function):
    """GradientReversalFunction (model.py:9-17): identity forward, -alpha * grad backward."""

    @staticmethod
    def forward(ctx, x, alpha):
        ctx.alpha = float(alpha)
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous(memory_format=CL) if dy.dim() == 4 else dy.contiguous()
        dx = torch.empty_like(dy)
        lib.rtsds_act_bwd(_P(dy), None, _P(dx), dy.numel(), 0, -ctx.alpha, dcode(dy), stream())
        return dx, None


# ----------------------------------------------------------------------------- pooling
def pool_out(size, k, s, p, ceil_mode):
    """ATen pooling_output_shape (dilation 1)."""
    num = size + 2 * p - (k - 1) - 1 + ((s - 1) if ceil_mode else 0)
    o = num // s + 1
    if ceil_mode and (o - 1) * s >= size + p:
        o -= 1
    return o


class MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p, ceil_mode):
        require_hip(x)
        x = nhwc(x)
        n, c, h, w = x.shape
        ho, wo = pool_out(h, k, s, p, ceil_mode), pool_out(w, k, s, p, ceil_mode)
        y = empty_nhwc(n, c, ho, wo, x.dtype, x.device)
        # inference (no gradient): the argmax bytes are not written where the kernel allows it
        need = ctx.needs_input_grad[0] or not (k == 3 and c % (8 if x.dtype == torch.bfloat16 else 4) == 0)
        idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device) if need else None
        lib.rtsds_maxpool_fwd(_P(x), _P(y), _P(idx), n, h, w, c, ho, wo, k, s, p, dcode(x), stream())
        ctx.geo = (n, h, w, c, ho, wo, k, s, p)
        ctx.dtype = x.dtype
        ctx.save_for_backward(idx)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        n, h, w, c, ho, wo, k, s, p = ctx.geo
        dy = nhwc(dy)
        dx = empty_nhwc(n, c, h, w, dy.dtype, dy.device)
        lib.rtsds_maxpool_bwd(_P(dy), _P(idx), _P(dx), n, h, w, c, ho, wo, k, s, p, dcode(dy), stream())
        return dx, None, None, None, None


def max_pool2d(x, k, s, p, ceil_mode=False):
    return MaxPoolFn.apply(x, k, s, p, ceil_mode)


class BnReluMaxPoolFn(torch.autograd.Function):
    """BatchNorm2d + ReLU + MaxPool2d(3, 2, p) (the ResNet stem bn1 -> relu -> maxpool,
    build_contextpath.py:15-18 via torchvision resnet.py; deeplabv2.py:106-110): the forward
    is one pass that never writes the full-resolution activation (bn.hip)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, stats, stats_nrb, nbt,
                p, ceil_mode, wg_link=None):
        require_hip(x)
        x = nhwc(x)
        n, c, h, w = x.shape
        ho, wo = pool_out(h, 3, 2, p, ceil_mode), pool_out(w, 3, 2, p, ceil_mode)
        y = empty_nhwc(n, c, ho, wo, x.dtype, x.device)
        idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
        sm = torch.empty(c, dtype=torch.float32, device=x.device)
        si = torch.empty(c, dtype=torch.float32, device=x.device)
        ws = workspace(lib.rtsds_bn_workspace(n * h * w, c), x.device)
        lib.rtsds_bn_relu_maxpool_fwd(_P(x), _P(y), _P(idx), n, h, w, c, ho, wo, p, _P(gamma), _P(beta),
                                      _P(running_mean), _P(running_var), _P(nbt), _P(sm), _P(si), float(momentum),
                                      float(eps), int(training), _P(stats) if training else None,
                                      int(stats_nrb or 0), dcode(x), _P(ws), ws.numel(), stream())
        ctx.meta = (n, c, h, w, ho, wo, p, int(training))
        ctx.gamma, ctx.beta = gamma, beta
        ctx.save_for_backward(x, idx, gamma, beta, sm, si)
        ctx.wg_link = wg_link
        return y

    @staticmethod
    def backward(ctx, dy):
        x, idx, gamma, beta, sm, si = ctx.saved_tensors
        n, c, h, w, ho, wo, p, training = ctx.meta
        dy = nhwc(dy)
        if dy.dtype != x.dtype:
            dy = cast(dy, x.dtype)
        dx = torch.empty_like(x, memory_format=CL) if ctx.needs_input_grad[0] else None
        dg, db, acc = _bn_param_grads(ctx, c, x.device)
        # backward unfused: the pool gradient is materialised once (16-B scatter-free gather,
        # rtsds_maxpool_bwd) and the BatchNorm backward reads it directly -- measured faster
        # than gathering it inside both BatchNorm passes (rtsds_bn_relu_maxpool_bwd: 94 + 108
        # vs 66 + 45 + 60 us at the BiSeNet stem, the gather's 4-window compare is VALU-bound)
        g = empty_nhwc(n, c, h, w, dy.dtype, dy.device)
        lib.rtsds_maxpool_bwd(_P(dy), _P(idx), _P(g), n, h, w, c, ho, wo, 3, 2, p, dcode(dy), stream())
        if ctx.wg_link is not None and dx is not None:
            # dx is formed inside the stem conv's weight gradient, from the pool gradient g
            _bn_bwd_coef(ctx.wg_link, g, x, dg, db, n * h * w, c, gamma, beta, sm, si, training, ACT_RELU, acc)
            dx = g
        else:
            ws = workspace(lib.rtsds_bn_workspace(n * h * w, c), x.device)
            lib.rtsds_bn_bwd(_P(g), _P(x), None, _P(dx), None, _P(dg), _P(db), n * h * w, c, _P(gamma), _P(beta),
                             _P(sm), _P(si), training, ACT_RELU, acc, dcode(x), _P(ws), ws.numel(), stream())
        if acc:
            dg = db = None
        return dx, dg, db, None, None, None, None, None, None, None, None, None, None, None


def bn_relu_maxpool_ok(x, k, s, p):
    """Shapes the fused stem kernels take: bf16 NHWC, channels % 8, MaxPool2d(3, 2, p <= 1)."""
    return x.dtype == torch.bfloat16 and x.shape[1] % 8 == 0 and k == 3 and s == 2 and p in (0, 1)


def bn_relu_maxpool(x, gamma, beta, running_mean, running_var, training, momentum, eps, p, ceil_mode,
                    num_batches_tracked=None, wg_link=None):
    stats, nrb = _bn_epilogue_stats(x, training, running_mean)
    if wg_link is not None:
        wg_link = wg_link.take(x, training, ACT_RELU)
    return BnReluMaxPoolFn.apply(x, gamma, beta, running_mean, running_var, training, momentum, eps, stats, nrb,
                                 num_batches_tracked, p, ceil_mode, wg_link)


class PooledMlpFn(torch.autograd.Function):
    """sigmoid(conv2(relu(conv1(p)))) on pooled [N, C, 1, 1] vectors -- the FFM attention
    (build_bisenet.py:67-70) -- forward as one launch (rtsds_pooled_mlp_fwd) bit-identical to the
    two pooled conv launches, backward as one launch (rtsds_pooled_mlp_bwd) bit-identical to the
    six of the per-conv chain."""

    @staticmethod
    def forward(ctx, p, w1, b1, wq1, w2, b2, wq2):
        p = nhwc(p)
        n, c0 = p.shape[0], p.shape[1]
        c1, c2 = w1.shape[0], w2.shape[0]
        h = empty_nhwc(n, c1, 1, 1, p.dtype, p.device)
        a = empty_nhwc(n, c2, 1, 1, p.dtype, p.device)
        lib.rtsds_pooled_mlp_fwd(_P(p), _P(wq1), _P(b1), _P(wq2), _P(b2), _P(h), _P(a), n, c0, c1, c2, dcode(p), stream())
        ctx.params = (w1, b1, w2, b2)
        ctx.dims = (n, c0, c1, c2)
        ctx.save_for_backward(p, h, a, wq1, wq2)
        return a

    @staticmethod
    def backward(ctx, da):
        p, h, a, wq1, wq2 = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        n, c0, c1, c2 = ctx.dims
        da = nhwc(da)
        if da.dtype != a.dtype:
            da = cast(da, a.dtype)
        sinks = _sinks(w1, b1, w2, b2)
        if sinks is not None:
            dw1, db1, dw2, db2 = sinks
            acc = 1
        else:
            dw1 = torch.empty(c1, c0, 1, 1, dtype=torch.float32, device=p.device)
            dw2 = torch.empty(c2, c1, 1, 1, dtype=torch.float32, device=p.device)
            db1 = torch.empty(c1, dtype=torch.float32, device=p.device) if b1 is not None else None
            db2 = torch.empty(c2, dtype=torch.float32, device=p.device) if b2 is not None else None
            acc = 0
        dp = empty_nhwc(n, c0, 1, 1, p.dtype, p.device)
        lib.rtsds_pooled_mlp_bwd(_P(da), _P(a), _P(h), _P(p), _P(wq1), _P(wq2), _P(dw1), _P(db1), _P(dw2), _P(db2),
                                 _P(dp), n, c0, c1, c2, acc, dcode(p), stream())
        if acc:
            dw1 = db1 = dw2 = db2 = None
        return dp, dw1, db1, None, dw2, db2, None


def pooled_mlp_ok(p, c1, c2):
    """Shapes rtsds_pooled_mlp_bwd reproduces bit for bit: N <= 8 pooled rows, <= 64 channels,
    channel counts off the vector kernels' multiples."""
    n, c0 = p.shape[0], p.shape[1]
    v = 8 if p.dtype == torch.bfloat16 else 4
    return p.dim() == 4 and p.shape[2] == p.shape[3] == 1 and n <= 8 and max(c0, c1, c2) <= 64 and \
        all(c % v for c in (c0, c1, c2)) and p.dtype in (torch.bfloat16, torch.float32)


def pooled_mlp(p, w1, b1, wq1, w2, b2, wq2):
    return PooledMlpFn.apply(p, w1, b1, wq1, w2, b2, wq2)


class FfmTailFn(torch.autograd.Function):
    """Training-mode tail of the FeatureFusionModule after its 3x3 conv (build_bisenet.py:75-80):
    feature = relu(bn(x)), att = sigmoid(conv2(relu(conv1(GAP(feature))))), r = feature * att +
    feature -- BatchNormFn, GapFn, PooledMlpFn and ChScaleFn (mode 1) as one Function.

    Forward: the BatchNorm apply also leaves the pool's slice partials (rtsds_bn_fwd_gap), then one
    launch sums them, runs the two pooled convs and scales (rtsds_ffm_att_scale): 2 launches after
    the finalize for the chain's 5.  Backward: the attention gradient's slice partials and one
    launch for their sum + the pooled convs' backward (rtsds_ffm_att_bwd), then the BatchNorm
    backward reading round(round(dr * (att + 1)) + round(dpooled / hw)) per element
    (rtsds_bn_bwd_ffm) instead of the joined feature gradient the channel scale and the pool
    would have written: 5 launches for the chain's 8.  Every result equals the chain's bit for
    bit (each reduction keeps its partition and order)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, stats, stats_nrb, nbt,
                w1, b1, wq1, w2, b2, wq2, pitch=0):
        require_hip(x)
        x = nhwc(x)
        n, c, h, w = x.shape
        hw = h * w
        feature = torch.empty_like(x, memory_format=CL)
        if pitch > c:  # r in the zero-padded pixel pitch its reader gathers (is_padded_input)
            r = torch.empty((n, h, w, pitch), dtype=x.dtype, device=x.device).permute(0, 3, 1, 2)[:, :c]
        else:
            pitch = c
            r = torch.empty_like(x, memory_format=CL)
        sm = torch.empty(c, dtype=torch.float32, device=x.device)
        si = torch.empty(c, dtype=torch.float32, device=x.device)
        pooled, hid, att = (empty_nhwc(n, c, 1, 1, x.dtype, x.device) for _ in range(3))
        ws = workspace(lib.rtsds_bn_workspace(n * hw, c), x.device)
        part = workspace(lib.rtsds_gap_workspace(n, hw, c), x.device)
        lib.rtsds_bn_fwd_gap(_P(x), _P(feature), _P(part), n, hw, c, _P(gamma), _P(beta), _P(running_mean),
                             _P(running_var), _P(nbt), _P(sm), _P(si), float(momentum), float(eps), ACT_RELU,
                             _P(stats), int(stats_nrb or 0), dcode(x), _P(ws), ws.numel(), stream())
        lib.rtsds_ffm_att_scale(_P(part), _P(feature), _P(wq1), _P(b1), _P(wq2), _P(b2), _P(pooled), _P(hid), _P(att),
                                _P(r), pitch, n, hw, c, dcode(x), stream())
        ctx.gamma, ctx.beta = gamma, beta
        ctx.params = (w1, b1, w2, b2)
        ctx.save_for_backward(x, feature, pooled, hid, att, wq1, wq2, gamma, beta, sm, si)
        return r

    @staticmethod
    def backward(ctx, dr):
        x, feature, pooled, hid, att, wq1, wq2, gamma, beta, sm, si = ctx.saved_tensors
        w1, b1, w2, b2 = ctx.params
        n, c, h, w = x.shape
        hw = h * w
        dr = nhwc(dr)
        if dr.dtype != x.dtype:
            dr = cast(dr, x.dtype)
        sinks = _sinks(w1, b1, w2, b2)
        if sinks is not None:
            dw1, db1, dw2, db2 = sinks
            acc = 1
        else:
            dw1 = torch.empty(c, c, 1, 1, dtype=torch.float32, device=x.device)
            dw2 = torch.empty(c, c, 1, 1, dtype=torch.float32, device=x.device)
            db1 = torch.empty(c, dtype=torch.float32, device=x.device) if b1 is not None else None
            db2 = torch.empty(c, dtype=torch.float32, device=x.device) if b2 is not None else None
            acc = 0
        dp = empty_nhwc(n, c, 1, 1, x.dtype, x.device)
        part = workspace(lib.rtsds_gap_workspace(n, hw, c), x.device)
        lib.rtsds_ffm_att_bwd(_P(dr), _P(feature), _P(att), _P(hid), _P(pooled), _P(wq1), _P(wq2), _P(dw1), _P(db1),
                              _P(dw2), _P(db2), _P(dp), n, hw, c, acc, dcode(x), _P(part), part.numel(), stream())
        if acc:
            dw1 = db1 = dw2 = db2 = None
        dx = torch.empty_like(x, memory_format=CL) if ctx.needs_input_grad[0] else None
        dg, db, bacc = _bn_param_grads(ctx, c, x.device)
        ws = workspace(lib.rtsds_bn_workspace(n * hw, c), x.device)
        lib.rtsds_bn_bwd_ffm(_P(dr), _P(att), _P(dp), n, hw, _P(x), _P(dx), _P(dg), _P(db), c, _P(gamma), _P(beta),
                             _P(sm), _P(si), 1, ACT_RELU, bacc, dcode(x), _P(ws), ws.numel(), stream())
        if bacc:
            dg = db = None
        return dx, dg, db, None, None, None, None, None, None, None, dw1, db1, None, dw2, db2, None, None


def ffm_tail_ok(x, convs):
    """Whether FfmTailFn takes ``x`` (the fusion module's conv output) with the 1x1 ``convs``: the
    shapes its kernels are instantiated for and reproduce bit for bit -- 19-channel maps, N <= 8
    (pooled_mlp_ok), hw a multiple of the 16-byte vector, square 1x1 convs of that width."""
    if x.dim() != 4 or not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float32):
        return False
    n, c, h, w = x.shape
    v = 8 if x.dtype == torch.bfloat16 else 4
    return c == 19 and n <= 8 and (h * w) % v == 0 and \
        all(m.kernel_size == (1, 1) and m.in_channels == m.out_channels == c and m.stride == (1, 1)
            and m.padding == (0, 0) and m.groups == 1 for m in convs)


def ffm_tail(x, gamma, beta, running_mean, running_var, momentum, eps, nbt, w1, b1, wq1, w2, b2, wq2, reader=None):
    """``x``: the conv output, carrying its epilogue's BatchNorm statistics when it has them.
    ``reader``: the conv module that alone reads the result (BiSeNet's final 1x1 conv): the result
    is then written in the zero-padded pixel pitch that conv gathers (is_padded_input), which
    saves its channel-pad launch; any other reader sees an ordinary [N, C, H, W] view."""
    stats, nrb = _bn_epilogue_stats(x, True, running_mean)
    pitch = 0
    if reader is not None:
        k, _, kh, kw = reader.weight.shape
        d = _conv_desc(x, k, kh, kw, reader.stride, reader.padding, reader.dilation)
        pitch = lib.rtsds_conv2d_input_pitch(ctypes.byref(d))
        pitch = pitch if x.shape[1] < pitch <= 64 else 0
    r = FfmTailFn.apply(x, gamma, beta, running_mean, running_var, momentum, eps, stats, nrb, nbt,
                        w1, b1, wq1, w2, b2, wq2, pitch)
    if pitch:
        r._rt_cpad = pitch
    return r


class GapFn(torch.autograd.Function):
    """Mean over H, W keeping dims -> [N, C, 1, 1].  ``join``: GradJoin shared with the other
    reader of x (the attention modules' channel scale): the backward adds its broadcast into
    that reader's gradient buffer instead of autograd summing two full-size gradients."""

    @staticmethod
    def forward(ctx, x, join=None):
        require_hip(x)
        x = nhwc(x)
        n, c, h, w = x.shape
        y = empty_nhwc(n, c, 1, 1, x.dtype, x.device)
        ws = workspace(lib.rtsds_gap_workspace(n, h * w, c), x.device)
        lib.rtsds_gap_fwd(_P(x), _P(y), n, h * w, c, dcode(x), _P(ws), ws.numel(), stream())
        ctx.shape = (n, c, h, w)
        ctx.join = join
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c, h, w = ctx.shape
        dy = dy.contiguous()
        join = ctx.join
        acc = join is not None and join.buf is not None
        dx = join.buf if acc else empty_nhwc(n, c, h, w, dy.dtype, dy.device)
        lib.rtsds_gap_bwd(_P(dy), _P(dx), n, h * w, c, 1 if acc else 0, dcode(dy), stream())
        return (join.put(dx) if join is not None else dx), None


def global_avg_pool(x, join=None):
    """``join``: GradJoin shared with x's other reader (see GapFn)."""
    return GapFn.apply(x, join)


class ChScaleFn(torch.autograd.Function):
    """x * a[N,C,1,1] (mode 0) or x * a + x (mode 1).  ``join``: GradJoin shared with x's
    other reader (GapFn); ``join_a``: the same for a's other reader.  ``fused``: the backward's
    dx and da from one rtsds_chscale_bwd call (one pixel pass where the library has it); False:
    one call each, the separate passes (for A/B tests; the same bits)."""

    @staticmethod
    def forward(ctx, x, a, mode, join=None, join_a=None, fused=True):
        require_hip(x, a)
        x = nhwc(x)
        a = a.contiguous()
        n, c, h, w = x.shape
        if a.dtype != x.dtype:
            a = cast(a, x.dtype)
        y = torch.empty_like(x, memory_format=CL)
        lib.rtsds_chscale_fwd(_P(x), _P(a), _P(y), n, h * w, c, mode, dcode(x), stream())
        ctx.mode = mode
        ctx.join, ctx.join_a, ctx.fused = join, join_a, fused
        ctx.save_for_backward(x, a)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, a = ctx.saved_tensors
        n, c, h, w = x.shape
        dy = nhwc(dy)
        dx = torch.empty_like(x, memory_format=CL) if ctx.needs_input_grad[0] else None
        da = torch.empty_like(a) if ctx.needs_input_grad[1] else None
        ws = workspace(lib.rtsds_gap_workspace(n, h * w, c) if da is not None else 0, x.device)
        for gx, ga in ((dx, da),) if ctx.fused else ((dx, None), (None, da)):
            if gx is not None or ga is not None:
                lib.rtsds_chscale_bwd(_P(dy), _P(x), _P(a), _P(gx), _P(ga), n, h * w, c, ctx.mode,
                                      dcode(x), _P(ws), ws.numel(), stream())
        if dx is not None and ctx.join is not None:
            dx = _join_add(ctx.join, dx)
        if da is not None and ctx.join_a is not None:
            da = _join_add(ctx.join_a, da)
        return dx, da, None, None, None, None


def channel_scale(x, a, residual=False, join=None, join_a=None, fused=True):
    """``join`` / ``join_a``: GradJoin shared with x's / a's other reader (see GapFn)."""
    return ChScaleFn.apply(x, a, 1 if residual else 0, join, join_a, fused)


class ChScale2Fn(torch.autograd.Function):
    """(x * a) * b with a, b [N,C,1,1] -- BiSeNet's cx2 = ARM2(f4) * tail (build_bisenet.py:52,
    149) -- as one Function: two ChScaleFn (mode 0) without the intermediate tensor written, read
    back and saved.  Forward one launch (rtsds_chscale2_fwd) for two; backward one pixel pass and
    one final launch (rtsds_chscale2_bwd) for the chain's four passes and two finals.  Bit-identical
    to the chain: the intermediate and its gradient are rounded per element as the chain stores
    them, each reduction keeps its partition and order.  ``join`` / ``join_b``: GradJoin shared
    with x's / b's other reader, fed in the chain's order."""

    @staticmethod
    def forward(ctx, x, a, b, join=None, join_b=None):
        require_hip(x, a, b)
        x = nhwc(x)
        n, c, h, w = x.shape
        a, b = (cast(t.contiguous(), x.dtype) for t in (a, b))
        y = torch.empty_like(x, memory_format=CL)
        lib.rtsds_chscale2_fwd(_P(x), _P(a), _P(b), _P(y), n, h * w, c, dcode(x), stream())
        ctx.join, ctx.join_b = join, join_b
        ctx.save_for_backward(x, a, b)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, a, b = ctx.saved_tensors
        n, c, h, w = x.shape
        dy = nhwc(dy)
        if dy.dtype != x.dtype:
            dy = cast(dy, x.dtype)
        dx = torch.empty_like(x, memory_format=CL)
        da, db = torch.empty_like(a), torch.empty_like(b)
        ws = workspace(2 * lib.rtsds_gap_workspace(n, h * w, c), x.device)
        lib.rtsds_chscale2_bwd(_P(dy), _P(x), _P(a), _P(b), _P(dx), _P(da), _P(db), n, h * w, c, dcode(x),
                               _P(ws), ws.numel(), stream())
        # the chain's order: the outer scale's db, then the inner scale's dx
        db = _join_add(ctx.join_b, db) if ctx.needs_input_grad[2] else None
        dx = _join_add(ctx.join, dx) if ctx.needs_input_grad[0] else None
        return dx, (da if ctx.needs_input_grad[1] else None), db, None, None


def channel_scale2_ok(x, a, b):
    """Whether ChScale2Fn takes (x * a) * b: HIP tensors of one bf16 / fp32 dtype, whole 16-byte
    channel vectors (what rtsds_chscale2_fwd / _bwd are written for)."""
    if x.dim() != 4 or not x.is_cuda or x.dtype not in (torch.bfloat16, torch.float32):
        return False
    n, c = x.shape[0], x.shape[1]
    return c % (8 if x.dtype == torch.bfloat16 else 4) == 0 and n <= 65535 and \
        all(t.dtype == x.dtype and tuple(t.shape) == (n, c, 1, 1) for t in (a, b))


def channel_scale2(x, a, b, join=None, join_b=None):
    """``join`` / ``join_b``: GradJoin shared with x's / b's other reader (see GapFn)."""
    return ChScale2Fn.apply(x, a, b, join, join_b)


# ----------------------------------------------------------------------------- bilinear
def _src_scale(in_size, out_size, scale_factor):
    """ATen area_pixel_compute_scale (align_corners=False), fp32."""
    if scale_factor is not None and scale_factor > 0:
        return float(np.float32(1.0 / scale_factor))
    return float(np.float32(in_size) / np.float32(out_size))


class BilinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ho, wo, sh, sw):
        require_hip(x)
        x = nhwc(x)
        n, c, hi, wi = x.shape
        y = empty_nhwc(n, c, ho, wo, x.dtype, x.device)
        lib.rtsds_bilinear_fwd(_P(x), _P(y), n, hi, wi, c, ho, wo, sh, sw, c, 0, dcode(x), stream())
        ctx.geo = (n, hi, wi, c, ho, wo, sh, sw)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, hi, wi, c, ho, wo, sh, sw = ctx.geo
        dy = nhwc(dy)
        dx = empty_nhwc(n, c, hi, wi, dy.dtype, dy.device)
        ws = workspace(lib.rtsds_bilinear_bwd_workspace(n, hi, wi, c, ho, wo), dy.device)
        lib.rtsds_bilinear_bwd(_P(dy), _P(dx), n, hi, wi, c, ho, wo, sh, sw, c, 0, dcode(dy), _P(ws),
                               ws.numel(), stream())
        return dx, None, None, None, None


def interpolate_bilinear(x, size=None, scale_factor=None):
    """F.interpolate(x, size | scale_factor, mode='bilinear', align_corners=False)."""
    hi, wi = x.shape[-2:]
    if size is not None:
        ho, wo = int(size[0]), int(size[1])
        sh, sw = _src_scale(hi, ho, None), _src_scale(wi, wo, None)
    else:
        ho, wo = int(np.floor(hi * scale_factor)), int(np.floor(wi * scale_factor))
        sh = sw = _src_scale(hi, ho, scale_factor)
    return BilinearFn.apply(x, ho, wo, sh, sw)


# ----------------------------------------------------------------------------- softmax / losses
def _pix_strides(x):
    """(sn, sc, shw) element strides of a [N, C, H, W] tensor whose H, W flatten."""
    sn, sc, s_h, s_w = x.stride()
    if x.shape[2] > 1 and s_h != x.shape[3] * s_w:
        raise RuntimeError("rtsds_amd: logits must have flattenable H, W")
    return sn, sc, s_w


class SoftmaxFn(torch.autograd.Function):
    """F.softmax(x, dim=1) (train.py:225,245,256); output NHWC."""

    @staticmethod
    def forward(ctx, x):
        require_hip(x)
        n, c, h, w = x.shape
        sn, sc, shw = _pix_strides(x)
        y = empty_nhwc(n, c, h, w, x.dtype, x.device)
        lib.rtsds_softmax_fwd(_P(x), sn, sc, shw, _P(y), c, n, h * w, c, dcode(x), stream())
        ctx.save_for_backward(y)
        ctx.xlayout = (x.stride(), x.dtype)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        n, c, h, w = y.shape
        dy = nhwc(dy)
        if dy.dtype != y.dtype:
            dy = cast(dy, y.dtype)
        dx = empty_nhwc(n, c, h, w, y.dtype, y.device)
        sn, sc, shw = _pix_strides(dx)
        lib.rtsds_softmax_bwd(_P(dy), _P(y), c, _P(dx), sn, sc, shw, n, h * w, c, dcode(y), stream())
        return dx


def softmax(x, dim=1):
    if dim != 1:
        raise NotImplementedError("rtsds_amd.softmax: only dim=1 (channels) is on the hot path")
    return SoftmaxFn.apply(x)


def _class_weight(weight, c, device):
    """``weight`` of a weighted cross-entropy as the kernels take it: float32, c elements,
    contiguous, on ``device`` (a static device tensor -- no copy, no host sync on the hot path)."""
    if not (isinstance(weight, torch.Tensor) and weight.dtype == torch.float32 and weight.device == device
            and tuple(weight.shape) == (c,)):
        got = (tuple(weight.shape), weight.dtype, weight.device) if isinstance(weight, torch.Tensor) else type(weight)
        raise RuntimeError(f"rtsds_amd: class weight must be a float32 tensor of {c} elements on {device}, got {got}")
    return weight.contiguous()


class CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target, ignore_index, weight=None):
        require_hip(x, target)
        if target.dim() == 4:
            target = target.squeeze(1)
        target = target.contiguous()
        if target.dtype != torch.int64:
            target = target.long()
        n, c, h, w = x.shape
        if tuple(target.shape) != (n, h, w):
            raise RuntimeError(f"rtsds_amd: target shape {tuple(target.shape)} != {(n, h, w)}")
        sn, sc, shw = _pix_strides(x)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ws = workspace(lib.rtsds_ce_workspace(), x.device)
        if weight is None:
            lib.rtsds_ce_fwd(_P(x), sn, sc, shw, _P(target), _P(loss), n, h * w, c, ignore_index,
                             dcode(x), _P(ws), ws.numel(), stream())
        else:
            weight = _class_weight(weight, c, x.device)
            lib.rtsds_ce_weighted_fwd(_P(x), sn, sc, shw, _P(target), _P(weight), _P(loss), n, h * w, c, ignore_index,
                                      dcode(x), _P(ws), ws.numel(), stream())
        if dp_world() > 1:  # global-batch mean: local loss sum over the all-reduced count (weight sum)
            import torch.distributed as dist
            cnt = ws.view(torch.float32)[2048:2049]
            collective(lambda: dist.all_reduce(cnt))
            lib.rtsds_ce_finish(_P(ws), _P(loss), stream())
        ctx.ignore = ignore_index
        ctx.weight = weight
        ctx.save_for_backward(x, target, ws)
        return loss

    @staticmethod
    def backward(ctx, g):
        x, target, ws = ctx.saved_tensors
        n, c, h, w = x.shape
        sn, sc, shw = _pix_strides(x)
        dx = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
        g = g.contiguous().float()
        count = ws.view(torch.float32)[2048:2049]
        if ctx.weight is None:
            lib.rtsds_ce_bwd(_P(x), sn, sc, shw, _P(target), _P(g), _P(count), _P(dx), n, h * w, c,
                             ctx.ignore, dcode(x), stream())
        else:
            lib.rtsds_ce_weighted_bwd(_P(x), sn, sc, shw, _P(target), _P(ctx.weight), _P(g), _P(count), _P(dx), n, h * w,
                                      c, ctx.ignore, dcode(x), stream())
        return dx, None, None, None


def cross_entropy(x, target, ignore_index=-100, weight=None):
    """nn.CrossEntropyLoss(weight, ignore_index) mean.  ``weight``: None (today's unweighted calls,
    untouched) or a float32 device tensor of c class weights: loss = sum w[t] (lse - x[t]) / sum w[t]
    over the valid pixels.  Under data parallelism nothing else changes: the slot that held the
    local valid count holds the local weight sum, and the same one-element all-reduce makes it the
    global one."""
    if weight is None:
        return CrossEntropyFn.apply(x, target, ignore_index)
    return CrossEntropyFn.apply(x, target, ignore_index, weight)


class AdaptiveAvgPoolFn(torch.autograd.Function):
    """F.adaptive_avg_pool2d(x, (ho, wo)) (train.py:410,438,445), NHWC."""

    @staticmethod
    def forward(ctx, x, ho, wo):
        require_hip(x)
        x = nhwc(x)
        n, c, hi, wi = x.shape
        y = empty_nhwc(n, c, ho, wo, x.dtype, x.device)
        lib.rtsds_adaptive_avgpool_fwd(_P(x), _P(y), n, hi, wi, c, ho, wo, dcode(x), stream())
        ctx.geo = (n, c, hi, wi, ho, wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        n, c, hi, wi, ho, wo = ctx.geo
        dy = nhwc(dy)
        dx = empty_nhwc(n, c, hi, wi, dy.dtype, dy.device)
        lib.rtsds_adaptive_avgpool_bwd(_P(dy), _P(dx), n, hi, wi, c, ho, wo, dcode(dy), stream())
        return dx, None, None


def adaptive_avg_pool2d(x, output_size):
    """Identity (same tensor, as ATen's values) when the size already matches."""
    ho, wo = (output_size, output_size) if isinstance(output_size, int) else output_size
    if tuple(x.shape[-2:]) == (int(ho), int(wo)):
        return x
    return AdaptiveAvgPoolFn.apply(x, int(ho), int(wo))


class UpsampleCrossEntropyFn(torch.autograd.Function):
    """sum_h CrossEntropy(interpolate_bilinear(head_h, (H, W)), target) without materialising
    the full-resolution logits (rtsds_upce_*; the chain it replaces is cited in the header).
    Also adds head 0's argmax==target pixel count into ``correct`` when given."""

    @staticmethod
    def forward(ctx, target, geo, ignore_index, correct, set_correct, *heads):
        return UpsampleCrossEntropyFn.run(ctx, target, geo, ignore_index, correct, set_correct, None, heads, 5)

    @staticmethod
    def run(ctx, target, geo, ignore_index, correct, set_correct, weight, heads, first):
        n, c, hl, wl, H, W, sh, sw = geo
        xs = [nhwc(h) for h in heads]
        k = len(xs)
        dt = dcode(xs[0])
        nbytes = lib.rtsds_upce_workspace(k, n, hl, wl, c, H, W, sh, sw)
        ws = workspace(nbytes, xs[0].device)
        ptrs = (ctypes.c_void_p * k)(*[x.data_ptr() for x in xs])
        per_head = torch.empty(k, dtype=torch.float32, device=xs[0].device)
        total = torch.empty((), dtype=torch.float32, device=xs[0].device)
        want = any(ctx.needs_input_grad[first:])
        flags = int(want) | (UPCE_SET_CORRECT if set_correct else 0)
        if weight is None:
            lib.rtsds_upce_fwd(k, ptrs, _P(target), n, hl, wl, c, H, W, sh, sw, ignore_index, _P(per_head),
                               _P(total), _P(correct), flags, dt, _P(ws), ws.numel(), stream())
        else:
            lib.rtsds_upce_weighted_fwd(k, ptrs, _P(target), _P(weight), n, hl, wl, c, H, W, sh, sw, ignore_index,
                                        _P(per_head), _P(total), _P(correct), flags, dt, _P(ws), ws.numel(), stream())
        if dp_world() > 1:
            # global-batch mean: this rank's loss sums over the all-reduced valid-pixel count (the
            # weight sum of a weighted call: stat[0] either way)
            # (its contribution; the ranks' losses and gradients then SUM to the single-device
            # values, see runtime.dp_world)
            import torch.distributed as dist
            cnt = ws.view(torch.float32)[:1]
            collective(lambda: dist.all_reduce(cnt))
            lib.rtsds_upce_finish(k, _P(ws), _P(per_head), _P(total), stream())
        ctx.geo, ctx.k, ctx.dt, ctx.dtype = geo, k, dt, xs[0].dtype
        ctx.ws = ws
        ctx.per_head = per_head
        return total

    @staticmethod
    def backward(ctx, g):
        n, c, hl, wl, H, W, sh, sw = ctx.geo
        ws = ctx.ws
        dxs = [empty_nhwc(n, c, hl, wl, ctx.dtype, ws.device) for _ in range(ctx.k)]
        ptrs = (ctypes.c_void_p * ctx.k)(*[d.data_ptr() for d in dxs])
        g = g.contiguous().float()
        lib.rtsds_upce_bwd(ctx.k, _P(g), 0, ptrs, n, hl, wl, c, H, W, sh, sw, ctx.dt, _P(ws), ws.numel(),
                           stream())
        ctx.ws = None
        return (None, None, None, None, None, *dxs)


class WeightedUpsampleCrossEntropyFn(torch.autograd.Function):
    """UpsampleCrossEntropyFn with class weights (rtsds_upce_weighted_fwd): the same workspace plan
    and the same backward, which divides by stat[0] -- the weight sum here."""

    @staticmethod
    def forward(ctx, target, geo, ignore_index, correct, set_correct, weight, *heads):
        return UpsampleCrossEntropyFn.run(ctx, target, geo, ignore_index, correct, set_correct, weight, heads, 6)

    @staticmethod
    def backward(ctx, g):
        return (None, *UpsampleCrossEntropyFn.backward(ctx, g))


def interpolate_geometry(x, geo):
    """interpolate_bilinear with a precomputed upsample_geometry()."""
    ho, wo, sh, sw = geo
    return BilinearFn.apply(x, ho, wo, sh, sw)


def upsample_geometry(x, size=None, scale_factor=None):
    """(H, W, scale_h, scale_w) of interpolate_bilinear(x, size | scale_factor)."""
    hi, wi = x.shape[-2:]
    if size is not None:
        ho, wo = int(size[0]), int(size[1])
        return ho, wo, _src_scale(hi, ho, None), _src_scale(wi, wo, None)
    ho, wo = int(np.floor(hi * scale_factor)), int(np.floor(wi * scale_factor))
    s = _src_scale(hi, ho, scale_factor)
    return ho, wo, s, s


def upsample_cross_entropy_supported(heads, geo, ignore_index, weight=None):
    """Whether the fused upsample + CE covers these heads.  ``weight`` does not change the answer:
    the weighted kernel keeps its weights in registers and runs the unweighted call's plan, so every
    covered geometry is covered weighted too."""
    h0 = heads[0]
    n, c, hl, wl = h0.shape
    ho, wo, sh, sw = geo
    if len(heads) > 4 or any(tuple(h.shape) != tuple(h0.shape) or h.dtype != h0.dtype for h in heads):
        return False
    return lib.rtsds_upce_workspace(len(heads), n, hl, wl, c, ho, wo, sh, sw) > 0


def upsample_cross_entropy(heads, target, geo, ignore_index=-100, correct=None, set_correct=False, weight=None):
    """Sum over heads (in order) of cross_entropy(interpolate_bilinear(head, ...), target),
    fused; ``geo`` from upsample_geometry().  ``correct``: optional int64 device counter that
    receives head 0's pixel-accuracy matches (added; ``set_correct``: overwritten, so the
    caller need not zero it).  ``weight``: None, or a float32 device tensor of c class weights
    (nn.CrossEntropyLoss(weight=)): each head's loss is sum w[t] (lse - z[t]) / sum w[t]; ``correct``
    stays the unweighted count.  Under data parallelism nothing new is needed: stat[0] is the local
    weight sum and the existing one-element all-reduce makes it the global one.  Returns the total
    loss."""
    require_hip(target, *heads)
    t = target.squeeze(1) if target.dim() == 4 else target
    t = t.contiguous()
    if t.dtype != torch.int64:
        t = t.long()
    n, c, hl, wl = heads[0].shape
    ho, wo, sh, sw = geo
    if tuple(t.shape) != (n, ho, wo):
        raise RuntimeError(f"rtsds_amd: target shape {tuple(t.shape)} != {(n, ho, wo)}")
    if not upsample_cross_entropy_supported(heads, geo, ignore_index, weight):
        raise RuntimeError("rtsds_amd: fused upsample+CE does not cover this geometry")
    full = (n, c, hl, wl, ho, wo, sh, sw)
    if weight is not None:
        weight = _class_weight(weight, c, heads[0].device)
        return WeightedUpsampleCrossEntropyFn.apply(t, full, int(ignore_index), correct, bool(set_correct), weight, *heads)
    fn = UpsampleCrossEntropyFn
    total = fn.apply(t, full, int(ignore_index), correct, bool(set_correct), *heads)
    return total


def label_stats(labels, num_classes, ignore_index, count, support):
    """Label statistics for class weighting (rtsds_label_stats): adds to ``count[k]`` the pixels of
    ``labels`` (int64 [n, h, w] or [n, 1, h, w], on the device) labelled k, and to ``support[k]``
    the valid pixels (label in [0, num_classes)) of the images that contain class k.  ``count`` /
    ``support``: int64 device tensors of ``num_classes`` elements, accumulated into over calls.
    Labels equal to ``ignore_index`` or outside the classes enter neither.  Exact; no host sync."""
    require_hip(labels, count, support)
    t = labels.squeeze(1) if labels.dim() == 4 else labels
    if t.dim() != 3 or t.dtype != torch.int64:
        raise RuntimeError(f"rtsds_amd: label_stats takes int64 [n, h, w] labels, got {tuple(labels.shape)} {labels.dtype}")
    t = t.contiguous()
    c = int(num_classes)
    for name, v in (("count", count), ("support", support)):
        if v.dtype != torch.int64 or tuple(v.shape) != (c,) or not v.is_contiguous():
            raise RuntimeError(f"rtsds_amd: label_stats: {name} must be a contiguous int64 tensor of {c} elements")
    n, h, w = t.shape
    ws = workspace(lib.rtsds_label_stats_workspace(n, c), t.device)
    lib.rtsds_label_stats(_P(t), n, h, w, c, int(ignore_index), _P(count), _P(support), _P(ws), ws.numel(), stream())


class DistillKLFn(torch.autograd.Function):
    """distill_kl: rtsds_distill_fwd + rtsds_distill_finish, backward rtsds_distill_bwd from the
    residual q - p the forward left in its workspace.  A gradient for the student only."""

    @staticmethod
    def forward(ctx, student, teacher, temperature, agree, nbytes):
        s, t = nhwc(student), nhwc(teacher)
        n, c, hs, ws = s.shape
        ht, wt = t.shape[2:]
        buf = workspace(nbytes, s.device)
        loss = torch.empty((), dtype=torch.float32, device=s.device)
        want = bool(ctx.needs_input_grad[0])
        pixels = float(n * hs * ws * dp_world())
        lib.rtsds_distill_fwd(_P(s), dcode(s), _P(t), dcode(t), n, hs, ws, c, ht, wt, _src_scale(ht, hs, None),
                              _src_scale(wt, ws, None), float(np.float32(1.0 / temperature)), int(want), _P(agree),
                              _P(buf), buf.numel(), stream())
        lib.rtsds_distill_finish(_P(buf), buf.numel(), n, hs, ws, temperature * temperature / pixels, _P(loss), stream())
        if want:
            ctx.buf, ctx.coef_g, ctx.geo, ctx.dtype = buf, temperature / pixels, (n, c, hs, ws), s.dtype
        return loss

    @staticmethod
    def backward(ctx, g):
        n, c, hs, ws = ctx.geo
        dx = empty_nhwc(n, c, hs, ws, ctx.dtype, ctx.buf.device)
        g = g.contiguous().float()
        lib.rtsds_distill_bwd(_P(ctx.buf), ctx.buf.numel(), _P(g), ctx.coef_g, _P(dx), dcode(dx), n, hs, ws, c, stream())
        return dx, None, None, None, None


def distill_kl(student_low, teacher_low, temperature=1.0, agree=None):
    """Knowledge-distillation loss (Hinton et al., 2015) between two low-resolution class maps, in
    one fused pass (csrc/distill.hip).  The reference has no distillation; the protocol is this:

    * ``student_low`` [n, c, hs, ws] and ``teacher_low`` [n, c, ht, wt] are the models' main heads
      before their final resize (forward_lowres), fp32 or bf16 each, NHWC or NCHW memory.  The loss
      lives on the student's grid, where the student's own gradient does: no bilinear adjoint, and
      64x fewer pixels than at the label size.
    * The teacher is resampled onto that grid inside the kernel: bilinear, align_corners=False, not
      antialiased, any ratio up or down (BiSeNet's 64x128 head from DeepLab's 65x129), blended in
      fp32 and not rounded to the storage type; equal sizes give the identity.
    * Per student pixel, a = s/T, b = u/T (u the resampled teacher row), q = softmax(a), p = softmax(b):
      KL = sum_k p_k (log p_k - log q_k), a term with p_k == 0 counting 0 (torch's xlogy rule);
      loss = T^2 * sum_pixels KL / (n hs ws world), dloss/ds = g T (q - p) / (n hs ws world) --
      F.kl_div(log_softmax(s/T), softmax(u/T), 'sum') * T^2 / pixels.  ``world`` is
      runtime.dp_world(): the ranks' losses and gradients sum to the global batch's, assuming equal
      shards (BCE's world * local batch rule).
    * ``agree``: an optional one-element int64 (or uint64) device counter; the number of pixels whose
      argmax of s equals that of u is added to it.
    * The teacher gets no gradient.  Two runs give the same bits; no host sync (graph-capture safe)."""
    require_hip(student_low, teacher_low, agree)
    if student_low.dim() != 4 or teacher_low.dim() != 4:
        raise RuntimeError("rtsds_amd.distill_kl: student and teacher must be [n, c, h, w]")
    if student_low.shape[1] != teacher_low.shape[1]:
        raise RuntimeError(f"rtsds_amd.distill_kl: student has {student_low.shape[1]} classes, teacher {teacher_low.shape[1]}")
    if not 2 <= student_low.shape[1] <= 32:
        raise RuntimeError(f"rtsds_amd.distill_kl: the class count must lie in [2, 32], got {student_low.shape[1]}")
    if student_low.shape[0] != teacher_low.shape[0]:
        raise RuntimeError(f"rtsds_amd.distill_kl: batch sizes differ ({student_low.shape[0]} and {teacher_low.shape[0]})")
    temperature = float(temperature)
    if not (temperature > 0.0 and np.isfinite(temperature)):
        raise RuntimeError(f"rtsds_amd.distill_kl: temperature must be positive, got {temperature}")
    if agree is not None and (agree.numel() != 1 or agree.dtype not in (torch.int64, torch.uint64)):
        raise RuntimeError("rtsds_amd.distill_kl: agree must be a one-element int64 / uint64 tensor")
    n, c, hs, ws = student_low.shape
    nbytes = lib.rtsds_distill_workspace(n, hs, ws, c, *teacher_low.shape[2:])
    if not nbytes:
        raise RuntimeError("rtsds_amd.distill_kl: the kernel does not cover these sizes")
    return DistillKLFn.apply(student_low, teacher_low.detach(), temperature, agree, nbytes)


ENTROPY_PENALTIES = {"entropy": 0, "robust": 1, "max_squares": 2}  # include/rtsds_hip.h RTSDS_ENTROPY_*


class EntropyLossFn(torch.autograd.Function):
    """entropy_loss: rtsds_entropy_fwd + rtsds_entropy_finish, backward rtsds_entropy_bwd from the
    gradient term the forward left in its workspace.  Returns (loss, mean_entropy); the second
    carries no gradient."""

    @staticmethod
    def forward(ctx, x, penalty, eta, hmap, nbytes):
        x = nhwc(x)
        n, c, h, w = x.shape
        buf = workspace(nbytes, x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        ment = torch.empty((), dtype=torch.float32, device=x.device)
        want = bool(ctx.needs_input_grad[0])
        coef = 1.0 / float(n * h * w * dp_world())
        lib.rtsds_entropy_fwd(_P(x), dcode(x), n, h, w, c, penalty, eta, int(want), _P(hmap), _P(buf), buf.numel(), stream())
        lib.rtsds_entropy_finish(_P(buf), buf.numel(), n, h, w, coef, _P(loss), _P(ment), stream())
        if want:
            ctx.buf, ctx.coef_g, ctx.geo, ctx.dtype = buf, coef, (n, c, h, w), x.dtype
        ctx.mark_non_differentiable(ment)
        return loss, ment

    @staticmethod
    def backward(ctx, g, _):
        n, c, h, w = ctx.geo
        dx = empty_nhwc(n, c, h, w, ctx.dtype, ctx.buf.device)
        g = g.contiguous().float()
        lib.rtsds_entropy_bwd(_P(ctx.buf), ctx.buf.numel(), _P(g), ctx.coef_g, _P(dx), dcode(dx), n, h, w, c, stream())
        return dx, None, None, None, None


def entropy_loss(low, penalty="entropy", eta=2.0, entropy_map=None):
    """Entropy minimisation on a low-resolution class map, in one fused pass (csrc/entropy.hip):
    the direct unsupervised loss on a target prediction.  The reference has none; the protocol is this:

    * ``low`` [n, c, h, w] is the model's main head before its final resize (forward_lowres(x,
      main_only=True)), fp32 or bf16, NHWC or NCHW memory, 2 <= c <= 32.  The loss lives on that
      grid, where the head's own gradient does: no bilinear adjoint, and 64x fewer pixels than at
      the label size.
    * Per pixel, with logits z: d = z - max z, e = exp d, Z = sum e (a fixed order), p = e / Z,
      log p = d - log Z; H = -sum_k p_k log p_k, a term with p_k == 0 counting 0 (torch's xlogy
      rule: a masked class at -inf gives 0, not NaN); h = H / ln c in [0, 1]; S = sum_k p_k^2.
    * ``penalty``: ``"entropy"`` (ADVENT MinEnt, Vu et al. 2019) phi = h, dphi/dz_j =
      -(1 / ln c) p_j (log p_j + H); ``"robust"`` (FDA, Yang & Soatto 2020) phi = (h^2 + 1e-8)^eta,
      dphi/dz_j = 2 eta h (h^2 + 1e-8)^(eta - 1) times the former, eta > 0 (eta == 2 is formed as a
      product, any other with powf); ``"max_squares"`` (Chen et al. 2019) phi = -S / 2, dphi/dz_j =
      -p_j (p_j - S).  The gradient term of a class with p_j == 0 is 0.
    * loss = sum_pixels phi / (n h w world), dloss/dz = g dphi/dz / (n h w world); ``world`` is
      runtime.dp_world(): the ranks' losses and gradients sum to the global batch's, assuming equal
      shards (distill_kl's and BCE's rule).
    * Returns (loss, mean_entropy), both 0-dim fp32: ``loss`` carries the gradient, ``mean_entropy``
      = sum_pixels h / (n h w world) is for logs and carries none, whatever the penalty.
    * ``entropy_map``: an optional contiguous fp32 [n, h, w] device tensor that receives h per pixel.
    * Two runs give the same bits; no host sync, no memset (graph-capture safe)."""
    require_hip(low, entropy_map)
    if low.dim() != 4:
        raise RuntimeError("rtsds_amd.entropy_loss: the class map must be [n, c, h, w]")
    if not 2 <= low.shape[1] <= 32:
        raise RuntimeError(f"rtsds_amd.entropy_loss: the class count must lie in [2, 32], got {low.shape[1]}")
    if penalty not in ENTROPY_PENALTIES:
        raise RuntimeError(f"rtsds_amd.entropy_loss: penalty must be one of {', '.join(repr(p) for p in ENTROPY_PENALTIES)}, "
                           f"got {penalty!r}")
    eta = float(eta)
    if not (eta > 0.0 and np.isfinite(eta)):
        raise RuntimeError(f"rtsds_amd.entropy_loss: eta must be positive, got {eta}")
    dcode(low)
    n, c, h, w = low.shape
    if entropy_map is not None and (entropy_map.dtype != torch.float32 or tuple(entropy_map.shape) != (n, h, w)
                                    or not entropy_map.is_contiguous()):
        raise RuntimeError(f"rtsds_amd.entropy_loss: entropy_map must be a contiguous fp32 tensor of shape {(n, h, w)}")
    nbytes = lib.rtsds_entropy_workspace(n, h, w, c)
    if not nbytes:
        raise RuntimeError("rtsds_amd.entropy_loss: the kernel does not cover these sizes")
    return EntropyLossFn.apply(low, ENTROPY_PENALTIES[penalty], float(np.float32(eta)), entropy_map, nbytes)


class UpsampleSoftmaxFn(torch.autograd.Function):
    """softmax(interpolate_bilinear(x, geo), dim=1) in one pass (rtsds_upsoftmax_fwd), written
    zero-padded to 32 channels so the discriminator's first conv reads it directly
    (RTSDS_INPUT_PADDED); backward = softmax backward + resize adjoint in one pass plus the
    vertical adjoint (rtsds_upsoftmax_bwd).  Bit-identical to interpolate -> softmax."""

    @staticmethod
    def forward(ctx, x, geo):
        require_hip(x)
        x = nhwc(x)
        n, c, hi, wi = x.shape
        ho, wo, sh, sw = geo
        cp = 32
        buf = torch.empty((n, ho, wo, cp), dtype=x.dtype, device=x.device)
        lib.rtsds_upsoftmax_fwd(_P(x), _P(buf), n, hi, wi, c, ho, wo, sh, sw, cp, dcode(x), stream())
        ctx.geo, ctx.shape, ctx.cp = geo, (n, c, hi, wi), cp
        ctx.save_for_backward(buf)
        return buf.permute(0, 3, 1, 2)[:, :c]

    @staticmethod
    def backward(ctx, dy):
        buf, = ctx.saved_tensors
        n, c, hi, wi = ctx.shape
        ho, wo, sh, sw = ctx.geo
        dy = nhwc(dy)
        if dy.dtype != buf.dtype:
            dy = cast(dy, buf.dtype)
        dx = empty_nhwc(n, c, hi, wi, buf.dtype, buf.device)
        ws = workspace(lib.rtsds_upsoftmax_bwd_workspace(n, hi, wi, c, ho, wo), buf.device)
        lib.rtsds_upsoftmax_bwd(_P(dy), c, _P(buf), ctx.cp, _P(dx), n, hi, wi, c, ho, wo, sh, sw, dcode(buf),
                                       _P(ws), ws.numel(), stream())
        return dx, None


def upsample_softmax(x, geo):
    """softmax over classes of the resized head (train.py:225,245,256), as the discriminator's
    zero-padded input (functional.is_padded_input)."""
    y = UpsampleSoftmaxFn.apply(x, geo)
    y._rt_cpad = 32
    return y


class UpsampleSelfInformationFn(torch.autograd.Function):
    """ADVENT's weighted self-information maps -p log p / log c of the resized head in one pass
    (rtsds_upselfinfo_fwd), in UpsampleSoftmaxFn's padded layout.  -p log p does not determine p,
    so the backward (rtsds_upselfinfo_bwd) forms p again from the saved low-resolution head with
    the forward's own code instead of reading the full-resolution output."""

    @staticmethod
    def forward(ctx, x, geo):
        require_hip(x)
        x = nhwc(x)
        n, c, hi, wi = x.shape
        if not 2 <= c <= 32:
            raise RuntimeError(f"rtsds_amd.upsample_self_information: the class count must lie in [2, 32], got {c}")
        ho, wo, sh, sw = geo
        cp = 32
        buf = torch.empty((n, ho, wo, cp), dtype=x.dtype, device=x.device)
        lib.rtsds_upselfinfo_fwd(_P(x), _P(buf), n, hi, wi, c, ho, wo, sh, sw, cp, dcode(x), stream())
        ctx.geo = geo
        ctx.save_for_backward(x)
        return buf.permute(0, 3, 1, 2)[:, :c]

    @staticmethod
    def backward(ctx, dy):
        x, = ctx.saved_tensors
        n, c, hi, wi = x.shape
        ho, wo, sh, sw = ctx.geo
        dy = nhwc(dy)
        if dy.dtype != x.dtype:
            dy = cast(dy, x.dtype)
        dx = empty_nhwc(n, c, hi, wi, x.dtype, x.device)
        ws = workspace(lib.rtsds_upselfinfo_bwd_workspace(n, hi, wi, c, ho, wo), x.device)
        lib.rtsds_upselfinfo_bwd(_P(dy), c, _P(x), _P(dx), n, hi, wi, c, ho, wo, sh, sw, dcode(x), _P(ws), ws.numel(), stream())
        return dx, None


def upsample_self_information(x, geo):
    """The discriminator input of AdvEnt (Vu et al., CVPR 2019): I_k = -p_k log p_k / log c with
    p = softmax over classes of the resized head, as upsample_softmax's zero-padded tensor
    (functional.is_padded_input).  x [n, c, hi, wi], 2 <= c <= 32, fp32 or bf16, NHWC or NCHW memory;
    include/rtsds_hip.h states the arithmetic.  HIP only, no CPU fallback."""
    y = UpsampleSelfInformationFn.apply(x, geo)
    y._rt_cpad = 32
    return y


def upsample_softmax_accumulate(x, geo, acc, flip=False, accumulate=True, pred=None):
    """One pass of multi-scale / flip evaluation (rtsds_upsoftmax_acc): the fp32 probabilities
    softmax(interpolate_bilinear(x, geo), dim=1) are stored into (``accumulate=False``) or added
    onto the fp32 NHWC sum ``acc`` [n, ho, wo, c]; ``flip`` stores them mirrored along W (the
    prediction of a mirrored image, un-mirrored).  ``pred`` (int64 [n, ho, wo]) receives the
    argmax of the updated sum.  Inference only (no autograd node).  Returns ``acc``."""
    require_hip(x)
    x = nhwc(x.detach())
    n, c, hi, wi = x.shape
    ho, wo, sh, sw = geo
    if not acc.is_cuda or acc.device != x.device:
        raise RuntimeError("rtsds_amd: upsample_softmax_accumulate: acc must be on the input's HIP device")
    if acc.dtype != torch.float32 or tuple(acc.shape) != (n, ho, wo, c) or not acc.is_contiguous():
        raise RuntimeError(f"rtsds_amd: upsample_softmax_accumulate: acc must be contiguous fp32 {(n, ho, wo, c)}, "
                           f"got {acc.dtype} {tuple(acc.shape)}")
    if pred is not None and (pred.dtype != torch.int64 or tuple(pred.shape) != (n, ho, wo) or not pred.is_contiguous()
                             or pred.device != x.device):
        raise RuntimeError(f"rtsds_amd: upsample_softmax_accumulate: pred must be contiguous int64 {(n, ho, wo)} "
                           f"on the input's device, got {pred.dtype} {tuple(pred.shape)}")
    lib.rtsds_upsoftmax_acc(_P(x), _P(acc), _P(pred), n, hi, wi, c, ho, wo, sh, sw, int(bool(flip)),
                            int(bool(accumulate)), dcode(x), stream())
    return acc


def _pseudo_arg(fn, name, t, dtype, shape, device):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != device:
        raise RuntimeError(f"rtsds_amd: {fn}: {name} must be contiguous {dtype} {tuple(shape)} on {device}, "
                           f"got {t.dtype} {tuple(t.shape)} on {t.device}")


def confidence_histogram(acc, hist, passes=1, pred=None, cbin=None):
    """Per-class confidence histogram of a probability sum (rtsds_conf_hist).  ``acc``: fp32
    [n, H, W, c] as predict_multiscale / upsample_softmax_accumulate leave it, summed over
    ``passes`` passes.  Per pixel: k = argmax over classes (first maximum wins), conf =
    acc[k] * float32(1 / passes), b = floor(conf * bins) clamped to [0, bins - 1].  ``hist``
    (int64 [c, bins], bins a power of two in [16, 1024]) is ADDED to: it accumulates over
    batches.  ``pred`` (uint8 [n, H, W]) receives k, ``cbin`` (uint16 [n, H, W]) receives b;
    either may be None.  No host sync.  Returns ``hist``."""
    fn = "confidence_histogram"
    if not (acc.is_cuda and hist.is_cuda):
        raise RuntimeError(f"rtsds_amd: {fn}: acc and hist must be HIP tensors; there is no CPU fallback")
    if acc.dim() != 4 or acc.dtype != torch.float32 or not acc.is_contiguous():
        raise RuntimeError(f"rtsds_amd: {fn}: acc must be contiguous fp32 [n, H, W, c], got {acc.dtype} "
                           f"{tuple(acc.shape)}")
    n, h, w, c = acc.shape
    if acc.numel() == 0 or not 2 <= c <= 32:
        raise RuntimeError(f"rtsds_amd: {fn}: acc needs pixels and 2..32 classes, got {tuple(acc.shape)}")
    if hist.dim() != 2 or hist.shape[0] != c:
        raise RuntimeError(f"rtsds_amd: {fn}: hist must be int64 [{c}, bins], got {tuple(hist.shape)}")
    bins = int(hist.shape[1])
    if bins < 16 or bins > 1024 or bins & (bins - 1):
        raise RuntimeError(f"rtsds_amd: {fn}: bins must be a power of two in [16, 1024], got {bins}")
    _pseudo_arg(fn, "hist", hist, torch.int64, (c, bins), acc.device)
    if pred is not None:
        _pseudo_arg(fn, "pred", pred, torch.uint8, (n, h, w), acc.device)
    if cbin is not None:
        _pseudo_arg(fn, "cbin", cbin, torch.uint16, (n, h, w), acc.device)
    if int(passes) != passes or passes < 1:
        raise RuntimeError(f"rtsds_amd: {fn}: passes must be a positive integer, got {passes}")
    inv = float(np.float32(1.0) / np.float32(int(passes)))
    lib.rtsds_conf_hist(_P(acc), _P(hist), _P(pred), _P(cbin), n * h * w, c, bins, inv, stream())
    return hist


def pseudo_select(pred, cbin, tbin, ignore_index, out=None):
    """Thresholded pseudo-labels (rtsds_pseudo_select): int64 ``out`` (same shape as ``pred``)
    = pred where cbin >= tbin[pred], else ``ignore_index``.  ``pred`` uint8 / ``cbin`` uint16 as
    confidence_histogram wrote them, ``tbin`` int32 [c] on the same device (a value >= bins keeps
    nothing of that class).  No host sync.  Returns ``out``."""
    fn = "pseudo_select"
    if not (pred.is_cuda and cbin.is_cuda and tbin.is_cuda):
        raise RuntimeError(f"rtsds_amd: {fn}: pred, cbin and tbin must be HIP tensors; there is no CPU fallback")
    if pred.numel() == 0:
        raise RuntimeError(f"rtsds_amd: {fn}: pred is empty")
    _pseudo_arg(fn, "pred", pred, torch.uint8, pred.shape, pred.device)
    _pseudo_arg(fn, "cbin", cbin, torch.uint16, pred.shape, pred.device)
    if tbin.dim() != 1 or not 2 <= tbin.numel() <= 32:
        raise RuntimeError(f"rtsds_amd: {fn}: tbin must be int32 [c] with 2..32 classes, got {tuple(tbin.shape)}")
    _pseudo_arg(fn, "tbin", tbin, torch.int32, tbin.shape, pred.device)
    if out is None:
        out = torch.empty(pred.shape, dtype=torch.int64, device=pred.device)
    else:
        _pseudo_arg(fn, "out", out, torch.int64, pred.shape, pred.device)
    lib.rtsds_pseudo_select(_P(pred), _P(cbin), _P(tbin), _P(out), pred.numel(), tbin.numel(), int(ignore_index),
                            stream())
    return out


def upsample_pseudo(x, geo, bins=1024, tbin=None, ignore_index=None, pred=None, cbin=None, labels=None):
    """Pseudo-labels straight from a low-resolution head (rtsds_upsample_pseudo): the chain
    upsample_softmax_accumulate(accumulate=False) -> confidence_histogram(passes=1, pred, cbin)
    -> pseudo_select in one pass, bit for bit, without the fp32 probability tensor.  ``x``: the
    head [n, c, hi, wi] (2..32 classes), ``geo`` from upsample_geometry(); ``bins`` a power of two
    in [16, 1024].  With ``tbin`` (int32 [c] on the device) and ``ignore_index`` the int64 label
    map [n, H, W] is produced (allocated unless ``labels`` is given); without ``tbin`` the
    uint8 ``pred`` and uint16 ``cbin`` maps are (allocated unless given).  Outputs passed in are
    filled whichever mode.  Inference only, no host sync.  Returns (pred, cbin, labels), None for
    an output not produced."""
    fn = "upsample_pseudo"
    if not x.is_cuda or (tbin is not None and not tbin.is_cuda):
        raise RuntimeError(f"rtsds_amd: {fn}: x and tbin must be HIP tensors; there is no CPU fallback")
    if x.dim() != 4 or x.numel() == 0 or not 2 <= x.shape[1] <= 32:
        raise RuntimeError(f"rtsds_amd: {fn}: x must be [n, c, hi, wi] with 2..32 classes, got {tuple(x.shape)}")
    bins = int(bins)
    if bins < 16 or bins > 1024 or bins & (bins - 1):
        raise RuntimeError(f"rtsds_amd: {fn}: bins must be a power of two in [16, 1024], got {bins}")
    x = nhwc(x.detach())
    n, c, hi, wi = x.shape
    ho, wo, sh, sw = geo
    dev = x.device
    if labels is not None and tbin is None:
        raise RuntimeError(f"rtsds_amd: {fn}: labels need the thresholds tbin")
    if tbin is not None:
        if ignore_index is None:
            raise RuntimeError(f"rtsds_amd: {fn}: tbin needs ignore_index")
        _pseudo_arg(fn, "tbin", tbin, torch.int32, (c,), dev)
        if labels is None:
            labels = torch.empty((n, ho, wo), dtype=torch.int64, device=dev)
    else:
        if pred is None:
            pred = torch.empty((n, ho, wo), dtype=torch.uint8, device=dev)
        if cbin is None:
            cbin = torch.empty((n, ho, wo), dtype=torch.uint16, device=dev)
    for name, t, dt in (("pred", pred, torch.uint8), ("cbin", cbin, torch.uint16), ("labels", labels, torch.int64)):
        if t is not None:
            _pseudo_arg(fn, name, t, dt, (n, ho, wo), dev)
    lib.rtsds_upsample_pseudo(_P(x), _P(pred), _P(cbin), _P(tbin), _P(labels), n, hi, wi, c, ho, wo, sh, sw, bins,
                              int(ignore_index) if ignore_index is not None else 0, dcode(x), stream())
    return pred, cbin, labels


def upsample_paint(x, geo, palette=None, alpha=1.0, frame=None, lut=None, ids=None, rgb=None, want_ids=True):
    """A class map and a painted frame straight from a low-resolution head (rtsds_upsample_paint):
    k = argmax_channels(interpolate_geometry(x, geo)) bit for bit, in one pass, without the
    full-resolution logits.  ``x``: the head [n, c, hi, wi] (2..32 classes), ``geo`` from
    upsample_geometry().  ``ids`` (uint8 [n, H, W]; allocated when ``want_ids`` and not given)
    receives lut[k], or k without ``lut`` (uint8 [c] on the device).  With ``palette`` (uint8
    [c, 3] on the device) ``rgb`` (uint8 [n, H, W, 3]; allocated unless given) receives
    palette[k], blended over ``frame`` (uint8 [n, H, W, 3]) when ``alpha`` < 1:
    (A * palette[k] + (256 - A) * frame + 128) >> 8 with A = floor(alpha * 256 + 0.5), in integers.
    Inference only, no host sync.  Returns (ids, rgb), None for an output not produced."""
    fn = "upsample_paint"
    given = [t for t in (palette, frame, lut, ids, rgb) if t is not None]
    if not x.is_cuda or not all(t.is_cuda for t in given):
        raise RuntimeError(f"rtsds_amd: {fn}: x and every buffer must be HIP tensors; there is no CPU fallback")
    if x.dim() != 4 or x.numel() == 0 or not 2 <= x.shape[1] <= 32:
        raise RuntimeError(f"rtsds_amd: {fn}: x must be [n, c, hi, wi] with 2..32 classes, got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"rtsds_amd: {fn}: x must be fp32 or bf16, got {x.dtype}")
    from .transforms import _strength_q8  # (transforms imports this module)
    try:
        a = _strength_q8(float(alpha))
    except RuntimeError:
        raise RuntimeError(f"rtsds_amd: {fn}: alpha must lie in [0, 1], got {alpha}") from None
    x = nhwc(x.detach())
    n, c, hi, wi = x.shape
    ho, wo, sh, sw = geo
    dev = x.device
    if palette is None and rgb is not None:
        raise RuntimeError(f"rtsds_amd: {fn}: rgb needs a palette")
    if palette is None and not (want_ids or ids is not None):
        raise RuntimeError(f"rtsds_amd: {fn}: nothing to produce (no palette and no ids)")
    if palette is not None:
        _pseudo_arg(fn, "palette", palette, torch.uint8, (c, 3), dev)
        if a < 256 and frame is None:
            raise RuntimeError(f"rtsds_amd: {fn}: alpha < 1 needs the frame to blend over")
        if rgb is None:
            rgb = torch.empty((n, ho, wo, 3), dtype=torch.uint8, device=dev)
    if ids is None and want_ids:
        ids = torch.empty((n, ho, wo), dtype=torch.uint8, device=dev)
    for name, t, shape in (("frame", frame, (n, ho, wo, 3)), ("lut", lut, (c,)), ("ids", ids, (n, ho, wo)),
                           ("rgb", rgb, (n, ho, wo, 3))):
        if t is not None:
            _pseudo_arg(fn, name, t, torch.uint8, shape, dev)
    lib.rtsds_upsample_paint(_P(x), _P(frame), _P(palette), _P(lut), _P(ids), _P(rgb), n, hi, wi, c, ho, wo, sh, sw, a,
                             dcode(x), stream())
    return ids, rgb


MAX_SLIDE_WINDOWS = 64  # rtsds_slide_paint: the window table travels in the kernel's arguments


def slide_paint(x, geo, windows, canvas, nf, palette=None, alpha=1.0, frame=None, lut=None, acc=None, accumulate=False,
                ids=None, rgb=None, want_ids=True):
    """Sliding-window prediction (rtsds_slide_paint): the heads of overlapping crops -> the class
    map and painted frame of the whole canvas in one pass.  ``x``: the heads [nwin * nf, c, hi, wi]
    (2..32 classes), window-major (window k of frame f at index k * nf + f); ``geo`` from
    upsample_geometry(): one head -> one window (hw, ww).  ``windows``: 1..64 entries (y0, x0) or
    (y0, x0, flip), each window inside ``canvas`` = (H, W); ``flip`` marks the head of a mirrored
    crop.  Per canvas pixel the probabilities upsample_softmax_accumulate forms for each covering
    window are summed in fp32 in window order (onto ``acc`` when ``accumulate``), and the first-max
    class of the sum gives ``ids`` (uint8 [nf, H, W]; lut[k] with ``lut``; allocated when
    ``want_ids`` and not given) and ``rgb`` (uint8 [nf, H, W, 3], with ``palette``; blended over
    ``frame`` when ``alpha`` < 1) exactly as upsample_paint writes them.  ``acc`` (fp32
    [nf, H, W, c], optional) receives the sum; without it no fp32 canvas exists.  Bit-identical to
    upsample_softmax_accumulate per window + a slice add per window.  Inference only, no host
    sync.  Returns (ids, rgb), None for an output not produced."""
    fn = "slide_paint"
    given = [t for t in (palette, frame, lut, acc, ids, rgb) if t is not None]
    if not x.is_cuda or not all(t.is_cuda for t in given):
        raise RuntimeError(f"rtsds_amd: {fn}: x and every buffer must be HIP tensors; there is no CPU fallback")
    if x.dim() != 4 or x.numel() == 0 or not 2 <= x.shape[1] <= 32:
        raise RuntimeError(f"rtsds_amd: {fn}: x must be [nwin * nf, c, hi, wi] with 2..32 classes, got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f"rtsds_amd: {fn}: x must be fp32 or bf16, got {x.dtype}")
    from .transforms import _strength_q8  # (transforms imports this module)
    try:
        a = _strength_q8(float(alpha))
    except RuntimeError:
        raise RuntimeError(f"rtsds_amd: {fn}: alpha must lie in [0, 1], got {alpha}") from None
    hw, ww, sh, sw = geo
    H, W = int(canvas[0]), int(canvas[1])
    nf = int(nf)
    table = [(int(w[0]), int(w[1]), int(bool(w[2])) if len(w) > 2 else 0) for w in windows]
    nwin = len(table)
    if not 1 <= nwin <= MAX_SLIDE_WINDOWS:
        raise RuntimeError(f"rtsds_amd: {fn}: 1..{MAX_SLIDE_WINDOWS} windows per call, got {nwin} (chunk them: accumulate)")
    if nf < 1 or x.shape[0] != nwin * nf:
        raise RuntimeError(f"rtsds_amd: {fn}: x must hold nwin * nf = {nwin} * {nf} heads, got {x.shape[0]}")
    if hw > H or ww > W or any(not (0 <= y0 <= H - hw and 0 <= x0 <= W - ww) for y0, x0, _ in table):
        raise RuntimeError(f"rtsds_amd: {fn}: every {hw} x {ww} window must lie inside the {H} x {W} canvas")
    x = nhwc(x.detach())
    _, c, hi, wi = x.shape
    dev = x.device
    if palette is None and rgb is not None:
        raise RuntimeError(f"rtsds_amd: {fn}: rgb needs a palette")
    if accumulate and acc is None:
        raise RuntimeError(f"rtsds_amd: {fn}: accumulate needs acc")
    if palette is None and acc is None and not (want_ids or ids is not None):
        raise RuntimeError(f"rtsds_amd: {fn}: nothing to produce (no palette, no ids and no acc)")
    if palette is not None:
        _pseudo_arg(fn, "palette", palette, torch.uint8, (c, 3), dev)
        if a < 256 and frame is None:
            raise RuntimeError(f"rtsds_amd: {fn}: alpha < 1 needs the frame to blend over")
        if rgb is None:
            rgb = torch.empty((nf, H, W, 3), dtype=torch.uint8, device=dev)
    if ids is None and want_ids:
        ids = torch.empty((nf, H, W), dtype=torch.uint8, device=dev)
    for name, t, shape in (("frame", frame, (nf, H, W, 3)), ("lut", lut, (c,)), ("ids", ids, (nf, H, W)),
                           ("rgb", rgb, (nf, H, W, 3))):
        if t is not None:
            _pseudo_arg(fn, name, t, torch.uint8, shape, dev)
    if acc is not None:
        _pseudo_arg(fn, "acc", acc, torch.float32, (nf, H, W, c), dev)
    win = (ctypes.c_int * (3 * nwin))(*[v for w in table for v in w])
    lib.rtsds_slide_paint(_P(x), win, nwin, _P(frame), _P(palette), _P(lut), _P(acc), _P(ids), _P(rgb), nf, hi, wi, c,
                          int(hw), int(ww), H, W, sh, sw, int(bool(accumulate)), a, dcode(x), stream())
    return ids, rgb


def ema_step(teacher, student, w, shadow=None):
    """Mean-teacher update of one flat fp32 buffer (rtsds_ema_step): teacher += w * (student -
    teacher) as three separately rounded fp32 operations, ``w`` rounded to fp32 here; ``shadow``
    (bf16, same length) receives the updated values rounded to nearest even in the same pass.
    All tensors 1-D contiguous on one HIP device.  No host sync.  Returns ``teacher``."""
    fn = "ema_step"
    if not (teacher.is_cuda and student.is_cuda and (shadow is None or shadow.is_cuda)):
        raise RuntimeError(f"rtsds_amd: {fn}: teacher, student and shadow must be HIP tensors; there is no CPU fallback")
    if teacher.dim() != 1 or teacher.numel() == 0:
        raise RuntimeError(f"rtsds_amd: {fn}: teacher must be a non-empty flat tensor, got {tuple(teacher.shape)}")
    _pseudo_arg(fn, "teacher", teacher, torch.float32, teacher.shape, teacher.device)
    _pseudo_arg(fn, "student", student, torch.float32, teacher.shape, teacher.device)
    if shadow is not None:
        _pseudo_arg(fn, "shadow", shadow, torch.bfloat16, teacher.shape, teacher.device)
    lib.rtsds_ema_step(_P(teacher), _P(student), _P(shadow), teacher.numel(), float(np.float32(w)), stream())
    return teacher


class EmaTable:
    """The device tables of rtsds_ema_many for (teacher, student) pairs of contiguous fp32 HIP
    tensors of equal size; ``stale()`` tells (on the host, no sync) whether a tensor has moved."""

    def __init__(self, pairs):
        fn = "EmaTable"
        if not pairs:
            raise RuntimeError(f"rtsds_amd: {fn}: no segments")
        dev = pairs[0][0].device
        for t, s in pairs:
            if not (t.is_cuda and s.is_cuda):
                raise RuntimeError(f"rtsds_amd: {fn}: segments must be HIP tensors; there is no CPU fallback")
            _pseudo_arg(fn, "teacher segment", t, torch.float32, t.shape, dev)
            _pseudo_arg(fn, "student segment", s, torch.float32, t.shape, dev)
        self.pairs = [(t, s) for t, s in pairs if t.numel() > 0]
        self.count = len(self.pairs)
        self.ptrs = self._ptrs()
        rows = [[p[0] for p in self.ptrs], [p[1] for p in self.ptrs], [t.numel() for t, _ in self.pairs]]
        self.table = torch.tensor(rows, dtype=torch.int64).to(dev)  # [3, count]: teacher, student, numel

    def _ptrs(self):
        return [(t.data_ptr(), s.data_ptr()) for t, s in self.pairs]

    def stale(self):
        return self._ptrs() != self.ptrs


def ema_many(table, w):
    """The ema_step update over every segment of an EmaTable in one launch (rtsds_ema_many)."""
    if not isinstance(table, EmaTable):
        raise RuntimeError("rtsds_amd: ema_many: table must be a functional.EmaTable")
    if table.stale():
        raise RuntimeError("rtsds_amd: ema_many: a segment has moved since the table was built; rebuild it")
    if table.count:
        t = table.table
        lib.rtsds_ema_many(table.count, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), float(np.float32(w)), stream())


_U32 = getattr(torch, "uint32", torch.int32)  # a torch without uint32: int32 holding the same bits


def _mix_labels(fn, slab):
    """Source labels as contiguous int64 [N, Hs, Ws] (from [N, 1, Hs, Ws] or [N, Hs, Ws])."""
    if slab.dim() == 4 and slab.shape[1] == 1:
        slab = slab[:, 0]
    if slab.dim() != 3 or slab.dtype != torch.int64 or not slab.is_contiguous() or slab.numel() == 0:
        raise RuntimeError(f"rtsds_amd: {fn}: slab must be contiguous int64 [N, Hs, Ws] or [N, 1, Hs, Ws], got "
                           f"{slab.dtype} {tuple(slab.shape)}")
    return slab


def _mix_rows(fn, name, t, n, cols, device):
    """int32 [n, cols] on ``device`` with unit column stride (a column slice of one wider block is
    fine: the kernels take the row pitch).  Returns the pitch in elements."""
    if t.dtype != torch.int32 or tuple(t.shape) != (n, cols) or t.device != device or t.stride(1) != 1 or \
            (n > 1 and t.stride(0) < cols):
        raise RuntimeError(f"rtsds_amd: {fn}: {name} must be int32 {(n, cols)} on {device} with unit column stride, "
                           f"got {t.dtype} {tuple(t.shape)} strides {tuple(t.stride())} on {t.device}")
    return int(t.stride(0)) if n > 1 else cols


def _mix_image(fn, name, x):
    """(n, h, w, pitch) of an image batch in one of the two input forms of the networks: NHWC
    (channels-last [N, 3, H, W]: pitch 3) or the 4-element pixel pitch of _pack (``_rt_cpad`` = 4)."""
    if x.dim() != 4 or x.shape[1] != 3 or x.dtype not in (torch.bfloat16, torch.float32) or x.numel() == 0:
        raise RuntimeError(f"rtsds_amd: {fn}: {name} must be a bf16 or fp32 [N, 3, H, W] batch, got {x.dtype} "
                           f"{tuple(x.shape)}")
    n, _, h, w = x.shape
    if getattr(x, "_rt_cpad", None) == 4 and is_padded_input(x):
        return n, h, w, 4
    if getattr(x, "_rt_cpad", None) is None and x.is_contiguous(memory_format=CL):
        return n, h, w, 3
    raise RuntimeError(f"rtsds_amd: {fn}: {name} must be in an input form (pack_input): NHWC, or the 4-channel pitch "
                       f"marked _rt_cpad = 4; got strides {tuple(x.stride())}")


def _mix_empty_image(n, h, w, pitch, dtype, device):
    if pitch == 3:
        return empty_nhwc(n, 3, h, w, dtype, device)
    y = torch.empty((n, h, w, 4), dtype=dtype, device=device).permute(0, 3, 1, 2)[:, :3]
    y._rt_cpad = 4
    return y


def class_presence(slab, size, origins, num_classes=32):
    """Classes present in a window of each source label map (rtsds_class_presence): ``slab``
    int64 [N, Hs, Ws] (or [N, 1, Hs, Ws]), ``size`` = (H, W) of the window, ``origins`` int32
    [N, 2] on the device, rows (y0, x0) with 0 <= y0 <= Hs - H and 0 <= x0 <= Ws - W.  Returns
    uint32 [N]: bit k set iff some window pixel equals k, 0 <= k < ``num_classes`` (2..32; any
    other label value sets no bit).  No host sync."""
    fn = "class_presence"
    if not (slab.is_cuda and origins.is_cuda):
        raise RuntimeError(f"rtsds_amd: {fn}: slab and origins must be HIP tensors; there is no CPU fallback")
    slab = _mix_labels(fn, slab)
    n, hs, ws = slab.shape
    h, w = int(size[0]), int(size[1])
    if not (0 < h <= hs and 0 < w <= ws):
        raise RuntimeError(f"rtsds_amd: {fn}: the window {(h, w)} does not fit the source {(hs, ws)}")
    if not 2 <= int(num_classes) <= 32:
        raise RuntimeError(f"rtsds_amd: {fn}: num_classes must be in 2..32, got {num_classes}")
    opitch = _mix_rows(fn, "origins", origins, n, 2, slab.device)
    present = torch.empty(n, dtype=_U32, device=slab.device)
    lib.rtsds_class_presence(_P(slab), _P(origins), opitch, _P(present), n, hs, ws, h, w, int(num_classes), stream())
    return present


def classmix(src, slab, tgt, pred, cbin, tbin, perm, origins, ignore_index, present=None, out=None, out_labels=None,
             mask=None, chosen=None):
    """ClassMix of a labelled source batch onto a target batch (rtsds_classmix), fused with the
    target's thresholded pseudo-labels.  Per sample n the classes present in the source window at
    ``origins[n]`` = (y0, x0) are ranked by their keys ``perm[n, k]`` (ties: lower class first)
    and the first (count + 1) >> 1 are chosen; a window pixel whose source label s is a chosen
    class takes the source pixel and the label s, every other pixel keeps the target pixel and
    gets pred where cbin >= tbin[pred], else ``ignore_index`` (pseudo_select's rule).

    ``src`` / ``tgt``: [N, 3, Hs, Ws] / [N, 3, H, W] image batches of one input form (bf16 or
    fp32; NHWC, or the 4-channel pitch of pack_input marked ``_rt_cpad``) -- pixels are copied bit
    for bit.  ``slab``: int64 [N, Hs, Ws] or [N, 1, Hs, Ws]; ``pred`` uint8 / ``cbin`` uint16
    [N, H, W]; ``tbin`` int32 [c], 2 <= c <= 32; ``perm`` int32 [N, c] and ``origins`` int32
    [N, 2] on the device (column slices of one block are fine).  ``present`` (uint32 [N]): the
    result of class_presence for the same window, computed here when None.  Optional outputs:
    ``out`` (an image batch of the inputs' form, [N, 3, H, W]), ``out_labels`` (int64 [N, H, W]),
    ``mask`` (uint8 [N, H, W]: 1 where the source was pasted), ``chosen`` (uint32 [N]: the chosen
    classes as a bit mask).  No host sync.  Returns ``(out, out_labels)``; ``out`` keeps the
    ``_rt_cpad`` marker of the inputs, so the model's pack_input passes it through."""
    fn = "classmix"
    tensors = (src, slab, tgt, pred, cbin, tbin, perm, origins)
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"rtsds_amd: {fn}: src, slab, tgt, pred, cbin, tbin, perm and origins must be HIP tensors; "
                           "there is no CPU fallback")
    dev = tgt.device
    n, h, w, pitch = _mix_image(fn, "tgt", tgt)
    ns, hs, ws, spitch = _mix_image(fn, "src", src)
    if src.dtype != tgt.dtype or spitch != pitch or ns != n or src.device != dev:
        raise RuntimeError(f"rtsds_amd: {fn}: src and tgt must share the batch size, the dtype, the image form and the "
                           f"device, got {src.dtype} pitch {spitch} x{ns} on {src.device} and {tgt.dtype} pitch {pitch} "
                           f"x{n} on {dev}")
    if hs < h or ws < w:
        raise RuntimeError(f"rtsds_amd: {fn}: the window {(h, w)} does not fit the source {(hs, ws)}")
    slab = _mix_labels(fn, slab)
    _pseudo_arg(fn, "slab", slab, torch.int64, (n, hs, ws), dev)
    _pseudo_arg(fn, "pred", pred, torch.uint8, (n, h, w), dev)
    _pseudo_arg(fn, "cbin", cbin, torch.uint16, (n, h, w), dev)
    if tbin.dim() != 1 or not 2 <= tbin.numel() <= 32:
        raise RuntimeError(f"rtsds_amd: {fn}: tbin must be int32 [c] with 2..32 classes, got {tuple(tbin.shape)}")
    c = tbin.numel()
    _pseudo_arg(fn, "tbin", tbin, torch.int32, (c,), dev)
    ppitch = _mix_rows(fn, "perm", perm, n, c, dev)
    opitch = _mix_rows(fn, "origins", origins, n, 2, dev)
    if present is None:
        present = class_presence(slab, (h, w), origins, c)
    elif present.dtype not in (_U32, torch.int32):
        raise RuntimeError(f"rtsds_amd: {fn}: present must be uint32 (or int32) [N], got {present.dtype}")
    else:
        _pseudo_arg(fn, "present", present, present.dtype, (n,), dev)
    if out is None:
        out = _mix_empty_image(n, h, w, pitch, tgt.dtype, dev)
    else:
        on, oh, ow, opx = _mix_image(fn, "out", out)
        if (on, oh, ow, opx) != (n, h, w, pitch) or out.dtype != tgt.dtype or out.device != dev:
            raise RuntimeError(f"rtsds_amd: {fn}: out must be a {tgt.dtype} {(n, 3, h, w)} batch of the inputs' image "
                               f"form on {dev}, got {out.dtype} {tuple(out.shape)} pitch {opx} on {out.device}")
    if out_labels is None:
        out_labels = torch.empty((n, h, w), dtype=torch.int64, device=dev)
    else:
        _pseudo_arg(fn, "out_labels", out_labels, torch.int64, (n, h, w), dev)
    if mask is not None:
        _pseudo_arg(fn, "mask", mask, torch.uint8, (n, h, w), dev)
    if chosen is not None:
        if chosen.dtype not in (_U32, torch.int32):
            raise RuntimeError(f"rtsds_amd: {fn}: chosen must be uint32 (or int32) [N], got {chosen.dtype}")
        _pseudo_arg(fn, "chosen", chosen, chosen.dtype, (n,), dev)
    lib.rtsds_classmix(_P(src), _P(slab), _P(tgt), _P(pred), _P(cbin), _P(tbin), _P(present), _P(perm), ppitch,
                       _P(origins), opitch, _P(out), _P(out_labels), _P(mask), _P(chosen), n, hs, ws, h, w, c,
                       pitch * tgt.element_size(), int(ignore_index), stream())
    return out, out_labels


class BCEWithLogitsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, target):
        require_hip(x, target)
        xf = cast(x.contiguous(), torch.float32)
        tf = cast(target.contiguous(), torch.float32) if target.dtype != torch.float32 else target.contiguous()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        lib.rtsds_bce_fwd(_P(xf), _P(tf), _P(loss), xf.numel(), stream())
        ctx.xdtype = x.dtype
        ctx.save_for_backward(xf, tf)
        return loss

    @staticmethod
    def backward(ctx, g):
        xf, tf = ctx.saved_tensors
        dx = torch.empty_like(xf)
        lib.rtsds_bce_bwd(_P(xf), _P(tf), _P(g.contiguous().float()), _P(dx), xf.numel(), stream())
        return cast(dx, ctx.xdtype), None


def bce_with_logits(x, target):
    return BCEWithLogitsFn.apply(x, target)


# ----------------------------------------------------------------------------- metrics
def argmax_channels(x, target=None, correct=None, want_map=True):
    """argmax over dim 1 (first max wins) -> int64 [N, H, W]; optionally adds the number of
    pixels equal to ``target`` into the device counter ``correct`` (uint64 view)."""
    require_hip(x)
    n, c, h, w = x.shape
    sn, sc, shw = _pix_strides(x)
    out = torch.empty((n, h, w), dtype=torch.int64, device=x.device) if want_map else None
    t = None
    if target is not None:
        t = target.squeeze(1) if target.dim() == 4 else target
        t = t.contiguous().long()
    lib.rtsds_argmax(_P(x), sn, sc, shw, _P(out), _P(t), _P(correct), n, h * w, c, dcode(x), stream())
    return out


def confusion(label, pred, hist, nc):
    lib.rtsds_confusion(_P(label.contiguous()), _P(pred.contiguous()), _P(hist), label.numel(), nc,
                        stream())
