"""The BatchNorm routes of tests/bn_bits_cases.py stated as formulas (include/rtsds_hip.h, "batch norm"):
``reference(case, inputs, dtype)`` returns every output the driver pins, by the same names, as
tests/route_compare.Out.  float64 is the reference; float32 serves the tolerance alone.  Nothing here goes
through autograd or a torch module: the backward cases use save_mean / save_invstd / y as given, and those
are not consistent with x.

Intermediate roundings (bf16 cases): rtsds_bn_relu_maxpool_fwd compares the window values "rounded to the
storage dtype, exactly the value the separate bn_apply would have stored" (rtsds_amd/csrc/bn.hip, the
comment above bn_relu_pool_fwd_kernel), so idx is the first maximum of the rounded values.
"""
import numpy as np
import torch

from .bn_bits_cases import EPS, LEAKY, MOMENTUM, RELU, SIGMOID, pool_geo
from .route_compare import Out, bf16r, host

MOM, EPSF, SLOPE = float(np.float32(MOMENTUM)), float(np.float32(EPS)), float(np.float32(0.2))  # as the kernels receive them


def _f(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _act(v, act):
    if act == RELU:
        return v.clamp_min(0)
    if act == LEAKY:
        return torch.where(v > 0, v, SLOPE * v)
    if act == SIGMOID:
        return 1 / (1 + torch.exp(-v))
    return v


def batch_stats(x):
    """mean, M2 = sum (x - mean)^2 and their term magnitudes over the rows of x [rows][c]."""
    mean = x.mean(0)
    d = x - mean
    return mean, (d * d).sum(0), x.abs().mean(0), x[0] / x.shape[0]


def merged_stats(st, rows):
    """The same from [c][nrb][count, mean, M2, 0] partials (Chan's merge, stated in one step)."""
    cnt, mi, m2 = st[:, :, 0], st[:, :, 1], st[:, :, 2]
    mean = (cnt * mi).sum(1) / rows
    d = mi - mean[:, None]
    return mean, m2.sum(1) + (cnt * d * d).sum(1), (cnt * mi).abs().sum(1) / rows, cnt[:, 0] * mi[:, 0] / rows


def forward_stats(k, h, x, rows, dtype):
    """mean, invstd and the five statistics outputs of a forward over ``rows`` rows."""
    rmean, rvar = _f(h["rmean"], dtype), _f(h["rvar"], dtype)
    if k.get("training", 1):
        mean, M2, Mmean, term = merged_stats(_f(h["stats"], dtype), rows) if k.get("nrb") else batch_stats(x)
        N = k.get("nrb") or rows
        var = M2 / rows
        invstd = 1 / torch.sqrt(var + EPSF)
        unb = M2 / (rows - 1)
        outs = dict(save_mean=Out(mean, Mmean, N, dropped=mean - term), save_invstd=Out(invstd, invstd.abs(), N),
                    running_mean=Out((1 - MOM) * rmean + MOM * mean, (1 - MOM) * rmean.abs() + MOM * Mmean, N),
                    running_var=Out((1 - MOM) * rvar + MOM * unb, (1 - MOM) * rvar.abs() + MOM * unb, N),
                    num_batches_tracked=Out(torch.tensor([6]), exact=True))
        return mean, invstd, Mmean, N, outs
    mean, invstd = rmean, 1 / torch.sqrt(rvar + EPSF)
    outs = dict(save_mean=Out(mean), save_invstd=Out(invstd), running_mean=Out(rmean), running_var=Out(rvar),
                num_batches_tracked=Out(torch.tensor([5]), exact=True))
    return mean, invstd, mean.abs(), 4, outs


def fwd(k, h, dtype, tols=None, got=None):
    rows, c, dt = k["rows"], k["c"], k["dt"]
    x = host(h["x"], dt, dtype).view(rows, c)
    gamma, beta = _f(h["gamma"], dtype), _f(h["beta"], dtype)
    mean, invstd, Mmean, N, outs = forward_stats(k, h, x, rows, dtype)
    sc = gamma * invstd
    pre = sc * (x - mean) + beta
    M = sc.abs() * (x.abs() + Mmean) + beta.abs()
    if k["res"]:
        res = host(h["res"], dt, dtype).view(rows, c)
        pre, M = pre + res, M + res.abs()
    outs["y"] = Out(_act(pre, k["act"]), M, N, bf16=dt == 1)
    return outs


def _mask(k, x, y, gamma, beta, mean, invstd, act):
    """act'(.) per element and the number of elements whose mask an fp32 evaluation could give otherwise."""
    if not act:
        return torch.ones_like(x), 0
    if y is not None:
        if act == SIGMOID:
            return y * (1 - y), 0
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE if act == LEAKY else 0.0)), 0
    sc = gamma * invstd
    sh = beta - mean * sc
    pre = x * sc + sh
    doubt = pre.abs() <= 8 * 2.0 ** -23 * ((x * sc).abs() + (mean * sc).abs() + beta.abs())
    return torch.where(pre > 0, torch.ones_like(x), torch.full_like(x, SLOPE if act == LEAKY else 0.0)), int(doubt.sum())


def _bwd_core(k, g, x, gamma, mean, invstd, rows, training, sums, dtype, h, bf):
    """dx, dgamma, dbeta from the masked gradient g; sums = (sg, sgx, |sg| terms, |sgx| terms, N)."""
    sg, sgx, Msg, Msgx, N, term = sums
    a = gamma * invstd
    d = x - mean
    outs = {}
    dgam, dbet, Mg, Mb = sgx * invstd, sg, Msgx * invstd, Msg
    if k.get("acc"):
        g0, b0 = _f(h["dgamma0"], dtype), _f(h["dbeta0"], dtype)
        dgam, dbet, Mg, Mb = g0 + dgam, b0 + dbet, g0.abs() + Mg, b0.abs() + Mb
    outs["dgamma"], outs["dbeta"] = Out(dgam, Mg, N), Out(dbet, Mb, N, dropped=dbet - term)
    if training:
        dx = a * g - a * invstd * invstd * sgx / rows * d - a * sg / rows
        M = a.abs() * (g.abs() + invstd * invstd * Msgx / rows * d.abs() + Msg / rows)
    else:
        dx, M, N = a * g, None, 1
    outs["dx"] = Out(dx, M, N, bf16=bf)
    return outs


def _row_sums(g, d, rows):
    return g.sum(0), (g * d).sum(0), g.abs().sum(0), (g * d).abs().sum(0), rows, g.gather(0, g.abs().argmax(0)[None])[0]


def bwd(k, h, dtype, tols=None, got=None):
    rows, c, dt = k["rows"], k["c"], k["dt"]
    x, dy = host(h["x"], dt, dtype).view(rows, c), host(h["dy"], dt, dtype).view(rows, c)
    y = host(h["y"], dt, dtype).view(rows, c) if h.get("y") is not None else None
    gamma, beta, mean, invstd = (_f(h[n], dtype) for n in ("gamma", "beta", "mean", "invstd"))
    f, doubt = _mask(k, x, y, gamma, beta, mean, invstd, k["act"])
    g = dy * f
    if k["kind"] == "part":
        part = _f(h["part"], dtype).view(c, k["nrb"], 2)
        sums = (part[:, :, 0].sum(1), part[:, :, 1].sum(1), part[:, :, 0].abs().sum(1), part[:, :, 1].abs().sum(1), k["nrb"], part[:, 0, 0])
    else:
        sums = _row_sums(g, x - mean, rows)
    outs = _bwd_core(k, g, x, gamma, mean, invstd, rows, k.get("training", 1), sums, dtype, h, dt == 1)
    if not k.get("dx", True):
        del outs["dx"]
    if k.get("dres"):
        outs["dres"] = Out(g, bf16=dt == 1)
    outs["_doubtful_masks"] = Out(torch.tensor([doubt]), exact=True, private=True)
    return outs


def _windows(v, k, fill):
    """The nine window taps of v [n][h][w][c] per pooled element: [9][n][ho][wo][c], ``fill`` outside the image."""
    n, hh, ww, c, p = k["n"], k["h"], k["w"], k["c"], k["p"]
    ho, wo, _, _ = pool_geo(k)
    pad = torch.full((n, hh + 2 * p + 2, ww + 2 * p + 2, c), fill, dtype=v.dtype)
    pad[:, p:p + hh, p:p + ww] = v
    return torch.stack([pad[:, t // 3:t // 3 + 2 * ho:2, t % 3:t % 3 + 2 * wo:2] for t in range(9)])


def pool(k, h, dtype, tols=None, got=None):
    n, hh, ww, c, p = k["n"], k["h"], k["w"], k["c"], k["p"]
    ho, wo, rows, npool = pool_geo(k)
    x = host(h["x"], 1, dtype).view(rows, c)
    gamma, beta = _f(h["gamma"], dtype), _f(h["beta"], dtype)
    mean, invstd, Mmean, N, outs = forward_stats(k, h, x, rows, dtype)
    sc = gamma * invstd
    pre = sc * (x - mean) + beta
    Mpre = sc.abs() * (x.abs() + Mmean) + beta.abs()
    outs["_act"] = Out(pre.clamp_min(0), Mpre, N, private=True)
    inf = float("inf")
    win = _windows(bf16r(pre.clamp_min(0)).view(n, hh, ww, c), k, -inf)
    idx = win.argmax(0)            # the first maximum in window order (torch.argmax: first of equal values)
    accept = None
    if tols is not None:           # a tap within tol of a bf16 rounding boundary may round either way
        t = tols["_act"]
        lo = _windows(bf16r((pre - t).clamp_min(0)).view(n, hh, ww, c), k, -inf)
        hi = _windows(bf16r((pre + t).clamp_min(0)).view(n, hh, ww, c), k, -inf)
        may = hi >= lo.max(0).values               # taps that can hold the maximum
        sure = ((lo == hi) | ~may).all(0)          # each of them rounds one way: the first of them is idx
        onehot = torch.zeros_like(may).scatter_(0, idx[None], True)
        accept = torch.where(sure[None], onehot, may).permute(1, 2, 3, 4, 0).reshape(-1, 9)
    outs["idx"] = Out(idx, exact=True, accept=accept)
    outs["y"] = Out(_windows(pre.clamp_min(0).view(n, hh, ww, c), k, -inf).max(0).values,
                    _windows(Mpre.expand(rows, c).reshape(n, hh, ww, c), k, 0.0).max(0).values, N, bf16=True)
    # backward: the pooled gradient gathered through idx (the kernel's once it has been checked), then
    # BatchNorm + ReLU backward with the mask from x and the statistics as given
    use = idx if got is None else got["idx"].view(n, ho, wo, c).to(torch.int64)
    dyp = host(h["dyp"], 1, dtype).view(n, ho, wo, c)
    g = torch.zeros((n, hh + 2 * p + 2, ww + 2 * p + 2, c), dtype=dtype)
    for t in range(9):
        g[:, t // 3:t // 3 + 2 * ho:2, t % 3:t % 3 + 2 * wo:2] += torch.where(use == t, dyp, torch.zeros_like(dyp))
    g = g[:, p:p + hh, p:p + ww].reshape(rows, c)
    smean, sinv = _f(h["mean"], dtype), _f(h["invstd"], dtype)
    f, doubt = _mask(k, x, None, gamma, beta, smean, sinv, RELU)
    g = g * f
    outs.update(_bwd_core(k, g, x, gamma, smean, sinv, rows, 1, _row_sums(g, x - smean, rows), dtype, h, True))
    outs["_doubtful_masks"] = Out(torch.tensor([doubt]), exact=True, private=True)
    return outs


_REF = {"fwd": fwd, "bwd": bwd, "part": bwd, "pool": pool}


def reference(case, inputs, dtype=torch.float64, tols=None, got=None):
    """{output name: Out} of one case.  tols: the case's recorded tolerances (None while they are being
    recorded: no exclusions then); got: the kernel's outputs, of which only the pool case's idx is used, by
    its backward."""
    return _REF[case["kind"]](case, inputs, dtype, tols, got)
