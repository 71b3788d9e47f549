"""The channel-vector routes of tests/chan_bits_cases.py stated as formulas (include/rtsds_hip.h: softmax /
losses, metrics, pooling, channel attention): ``reference(case, inputs, dtype)`` returns every output the
driver pins, by the same names, as tests/route_compare.Out.  float64 is the reference; float32 serves the
tolerance alone.  A pitched or sliced output is stated whole: the columns the kernel must not touch hold
UNWRITTEN, the padding columns of a pitched softmax hold zeros, and both must match exactly.

Intermediate roundings (bf16 cases), each where the unfused chain stores a tensor:
  rtsds_gap_bwd, accumulate: dx = round(dx + round(dy / hw)) ("same roundings as a separate elementwise
    add", include/rtsds_hip.h at rtsds_gap_bwd; dy * (1 / hw) in fp32, rtsds_amd/csrc/chan.hip gap_bwd_kernel).
  rtsds_ffm_head_eval: the pooled mean, the hidden vector, the attention vector and r = f * a + f are each
    "rounded to T where the unfused chain stores it" (rtsds_amd/csrc/chan.hip above ffm_head_apply_kernel).
"""
import numpy as np
import torch

from .bn_bits_cases import BF16, UNWRITTEN
from .chan_bits_cases import CE_RB, IGNORE, SLICE_C, SLICE_OFF
from .route_compare import Out, bf16_ulp, host, round_mid, round_op


def _logits(a, k, dt, dtype):
    """The case's logits as [n][hw][c] (a view of the whole input tensor in its layout)."""
    n, hw, c = k["n"], k["hw"], k["c"]
    t = host(a, dt, dtype)
    if k["lay"] == "nchw":
        return t.view(n, c, hw).permute(0, 2, 1)
    if k["lay"] == "slice":
        return t[SLICE_OFF:].view(n, hw, SLICE_C)[:, :, :c]   # the pointer is moved, the allocation SLICE_OFF longer
    return t[k.get("off", 0):].view(n, hw, c)


def _place(v, k, dtype, M=None):
    """v [n][hw][c] laid out as the kernel writes it into the whole output tensor; (values, fixed, M):
    elements outside the layout keep UNWRITTEN exactly."""
    n, hw, c = k["n"], k["hw"], k["c"]
    if k["lay"] == "nchw":
        return v.permute(0, 2, 1).contiguous(), None, None if M is None else M.permute(0, 2, 1).contiguous()
    if k["lay"] == "slice":
        full = torch.full((n, hw, SLICE_C), UNWRITTEN, dtype=dtype)
        fixed = torch.ones((n, hw, SLICE_C), dtype=torch.bool)
        full[:, :, SLICE_OFF:SLICE_OFF + c] = v
        fixed[:, :, SLICE_OFF:SLICE_OFF + c] = False
        Mf = None
        if M is not None:
            Mf = torch.zeros((n, hw, SLICE_C), dtype=torch.float64)
            Mf[:, :, SLICE_OFF:SLICE_OFF + c] = M
        return full, fixed, Mf
    return v.contiguous(), None, M


def smf(k, h, dtype, tols=None):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    x = _logits(h["x"], k, dt, dtype)
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    ld = k["ld"] or c
    y = torch.zeros((n, hw, ld), dtype=dtype)
    y[:, :, :c] = p
    fixed = torch.zeros((n, hw, ld), dtype=torch.bool)
    fixed[:, :, c:] = True
    less = y.clone()
    less[:, :, 1:c] = e[:, :, 1:] / (e.sum(-1, keepdim=True) - e[:, :, :1])   # class 0 left out of the sum
    return dict(y=Out(y, None, c, bf16=dt == BF16, fixed=fixed, dropped=less))


def smb(k, h, dtype, tols=None):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    ld, io = k["ld"] or c, k["off"]
    dy = host(h["dy"], dt, dtype)[io:].view(n, hw, ld)[:, :, :c]
    y = host(h["y"], dt, dtype)[io:].view(n, hw, ld)[:, :, :c]
    dot = (dy * y).sum(-1, keepdim=True)
    dx = y * (dy - dot)
    M = y.abs() * (dy.abs() + (dy * y).abs().sum(-1, keepdim=True))
    v, fixed, Mf = _place(dx, k, dtype, M.double())
    less = _place(y * (dy - dot + (dy * y)[:, :, :1]), k, dtype)[0]               # class 0 left out of the sum
    return dict(dx=Out(v, Mf, c, bf16=dt == BF16, fixed=fixed, dropped=less))


def ce(k, h, dtype, tols=None):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    x = _logits(h["x"], k, dt, dtype)
    t = torch.from_numpy(h["tgt"]).view(n, hw)
    valid, inb = t != IGNORE, (t >= 0) & (t < c)
    m = x.max(-1).values
    e = torch.exp(x - m[..., None])
    z = e.sum(-1)
    xt = x.gather(-1, t.clamp(0, c - 1)[..., None])[..., 0]
    xt = torch.where(inb, xt, torch.full_like(xt, float("nan")))   # a target outside [0, c): NaN
    loss_px = torch.log(z) + m - xt
    zero = torch.zeros_like(loss_px)
    S = torch.where(valid, loss_px, zero).sum()
    MS = torch.where(valid, torch.log(z).abs() + m.abs() + xt.abs(), zero).sum()
    C = valid.sum().to(dtype)
    pix = n * hw
    g = float(h["gl"][0]) / C                                        # upstream gradient / valid count
    onehot = torch.zeros_like(x).scatter_(-1, t.clamp(0, c - 1)[..., None], 1.0) * inb[..., None]
    dx = torch.where(valid[..., None], g * (e / z[..., None] - onehot), torch.zeros_like(x))
    v, fixed, _ = _place(dx, k, dtype)
    sel = torch.tensor([2 * CE_RB, 2 * CE_RB + 1])
    CF = torch.tensor(123.0, dtype=dtype)
    return dict(ws=Out(torch.stack([C, S]), torch.stack([C, MS]), pix, sel=sel), loss=Out(S / C, MS / C, pix, dropped=(S - torch.where(valid & inb, loss_px, zero).max()) / C),
                dx=Out(v, None, c, bf16=dt == BF16, fixed=fixed),
                ws_finish=Out(torch.stack([CF, S]), torch.stack([CF, MS]), pix, sel=sel), loss_finish=Out(S / CF, MS / CF, pix))


def am(k, h, dtype, tols=None):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    x = host(h["x"], dt, dtype)
    x = x.view(n, c, hw).permute(0, 2, 1) if k["lay"] == "nchw" else x.view(n, hw, c)
    key = torch.where(torch.isnan(x), torch.full_like(x, float("inf")), x)   # a NaN is a maximum; the first wins
    out = key.argmax(-1).reshape(-1)                                         # torch.argmax: the first of equal values
    outs = {}
    if k["null"] != "out":
        outs["out"] = Out(out, exact=True)
    if k["null"] != "correct":
        hits = int((out == torch.from_numpy(h["tgt"])).sum()) if h["tgt"] is not None else 0
        outs["correct"] = Out(torch.tensor([5 + hits]), exact=True)
    return outs


def bce(k, h, dtype, tols=None):
    n = k["n"]
    x, t = host(h["x"], 0, dtype), host(h["t"], 0, dtype)
    terms = (x.clamp_min(0), x * t, torch.log1p(torch.exp(-x.abs())))
    loss = (terms[0] - terms[1] + terms[2]).sum() / n
    M = sum(v.abs() for v in terms).sum() / n
    dx = float(h["gl"][0]) / n * (1 / (1 + torch.exp(-x)) - t)
    less = loss - (terms[0] - terms[1] + terms[2])[0] / n
    return dict(loss=Out(loss.reshape(1), M, n, dropped=less.reshape(1)), dx=Out(dx))


def conf(k, h, dtype, tols=None):
    nc = k["nc"]
    label, pred = torch.from_numpy(h["label"]), torch.from_numpy(h["pred"])
    ok = (label >= 0) & (label < nc)
    hist = torch.from_numpy(h["hist0"]).clone()
    hist.index_add_(0, (nc * label + pred)[ok], torch.ones(int(ok.sum()), dtype=torch.int64))
    return dict(hist=Out(hist, exact=True))


def gapf(k, h, dtype, tols=None):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    x = host(h["x"], dt, dtype).view(n, hw, c)
    return dict(y=Out(x.sum(1) / hw, x.abs().sum(1) / hw, hw, bf16=dt == BF16, dropped=(x.sum(1) - x[:, 0]) / hw))


def gapb(k, h, dtype, tols=None):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    dy = host(h["dy"], dt, dtype).view(n, 1, c)
    inv = float(np.float32(1.0) / np.float32(hw))        # the kernel multiplies by the fp32 reciprocal
    g = (dy * inv).expand(n, hw, c)
    if not k["acc"]:
        return dict(dx=Out(g.contiguous(), bf16=dt == BF16))
    return dict(dx=Out(host(h["dx0"], dt, dtype).view(n, hw, c) + round_op(g, dt), bf16=dt == BF16))


def csf(k, h, dtype, tols=None):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    x, a = host(h["x"], dt, dtype).view(n, hw, c), host(h["a"], dt, dtype).view(n, 1, c)
    return dict(y=Out(x * a + x if k["mode"] else x * a, bf16=dt == BF16))


def csb(k, h, dtype, tols=None):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    dy, x = host(h["dy"], dt, dtype).view(n, hw, c), host(h["x"], dt, dtype).view(n, hw, c)
    a = host(h["a"], dt, dtype).view(n, 1, c)
    if k["outs"] == "dx":
        return dict(dx=Out(dy * (a + k["mode"]), bf16=dt == BF16))
    return dict(da=Out((dy * x).sum(1), (dy * x).abs().sum(1), hw, bf16=dt == BF16, dropped=(dy * x).sum(1) - (dy * x)[:, 0]))


def ffm(k, h, dtype, tols=None):
    n, hw, c, dt = k["n"], k["hw"], k["c"], k["dt"]
    f = host(h["f"], dt, dtype).view(n, hw, c)
    w = [host(v, dt, dtype).view(c, c) for v in h["w"]]           # [out][in]
    b = [host(v, 0, dtype) for v in h["b"]]
    outs = {}

    def mid(name, v, M, N, f=lambda t: t, extra=0.0):
        """The stored vector and, per element, one bf16 step where its rounding is in doubt (else 0)."""
        outs[name] = Out(v, M, N, private=True)
        r, near = round_mid(v, dt, tols, name, f, extra)
        return r, near * bf16_ulp(r)

    # A doubtful rounding moves the next vector by at most one step times the weights; where that vector then
    # still rounds one way, the doubt ends there.  Only a doubtful attention value reaches the output.
    gap, dgap = mid("_gap", f.sum(1) / hw, f.abs().sum(1) / hw, hw)
    pre1 = gap @ w[0].T + b[0]
    hid, dhid = mid("_hid", pre1, gap.abs() @ w[0].abs().T + b[0].abs(), c + 1, lambda t: t.clamp_min(0),
                    dgap @ w[0].abs().double().T)
    pre2 = hid @ w[1].T + b[1]
    att, datt = mid("_att", 1 / (1 + torch.exp(-pre2)), hid.abs() @ w[1].abs().T + b[1].abs(), c + 1,
                    extra=dhid @ w[1].abs().double().T / 4)    # |sigmoid'| <= 1 / 4
    doubt = (datt > 0).any(1)
    r = round_op(f * att[:, None, :] + f, dt)                     # one fma
    out = r @ w[2].T + b[2]
    M = r.abs() @ w[2].abs().T + b[2].abs()
    # an image whose pooled chain has a value on a rounding boundary: every element of it is excluded
    slack = doubt.to(torch.float64)[:, None, None].expand(n, hw, c) * 1e30
    outs["out"] = Out(out, M, c + 1, bf16=dt == BF16, slack=slack if bool(doubt.any()) else None,
                      dropped=out - r[..., :1] * w[2][:, 0])
    return outs


_REF = {"smf": smf, "smb": smb, "ce": ce, "am": am, "bce": bce, "conf": conf, "gapf": gapf, "gapb": gapb, "csf": csf,
        "csb": csb, "ffm": ffm}


def reference(case, inputs, dtype=torch.float64, tols=None, got=None):
    """{output name: Out} of one case.  tols: the case's recorded tolerances (None while they are being
    recorded: no intermediate is rounded on a doubtful boundary then)."""
    return _REF[case["kind"]](case, inputs, dtype, tols)
