"""What the three route-reference suites share (tests/test_{bn,chan,resize}_route_ref_gpu.py,
tests/test_route_refs_cpu.py, tools/record_route_tol.py): the description of one reference output, its
tolerance, and the comparison of what a kernel wrote with it.  No device and no library here.

A reference (tests/{bn,chan,resize}_route_ref.py) is a function of a case's host inputs that runs in a
given dtype: in float64 it is the statement of the operation, in float32 its only use is the tolerance

    tol = m * max(E32, U),   E32 = max |reference in float32 - reference in float64|,   U = 2^-23 * M,
    m = max(8, ceil(log2(N) / 2))

with M = max |reference| for an elementwise output and, for an output that is a sum of N terms, the float64
sum of the absolute values of its terms (the reference hands it back as ``Out.M``).  A blocked or pairwise
fp32 sum is off by at most log2(N) * 2^-24 * sum |t| in any order; 8 is the margin of
tests/pinned/entropy_tol.json over a float32 restatement (summation order, the hardware's expf / logf).  An
output stored as bf16 gets 2^-8 |ref_i| per element on top (its rounding and one boundary flip).  The
tolerances are recorded once, on the CPU, into tests/pinned/route_ref_tol.json; the GPU tests read them.

Elements on a discontinuity (a mask, an argmax, the bf16 rounding of a stored intermediate that lies within
its tolerance of a rounding boundary in float64) are excluded from the bound above and held to the weaker
statement the discontinuity allows: ``Out.slack`` is one ulp of the intermediate carried through to the
output, ``Out.accept`` the set of classes a near tie allows.  At most MAX_EXCLUDED of an output's elements
may be excluded; tests/test_route_refs_cpu.py shows from the references alone that every case keeps to it.
"""
import json
import math
import os

import numpy as np
import torch

from .bn_bits_cases import BF16, UNWRITTEN

TOL_PATH = os.path.join(os.path.dirname(__file__), "pinned", "route_ref_tol.json")
MARGIN = 8
EPS32 = 2.0 ** -23
BF16_OUT = 2.0 ** -8
MAX_EXCLUDED = 1e-3
TINY = 2.0 ** -149   # the smallest positive fp32: the tolerance of an output that is exactly zero (or all NaN)
EXACT = "exact"      # the tolerance entry of an integer output


class Out:
    """One output of a reference.  val: its elements (any shape; compared flat).  M / N: see the module
    docstring (M a scalar or a tensor like val; None = elementwise).  bf16: stored as bf16.  exact: an
    integer output.  sel: the flat indices of the kernel's output that val states (None = all of it).
    slack: per element, what an excluded element may be off by on top of the bound (0 = not excluded).
    accept: for an integer output, bool [elements][values]: an element whose row has more than one True is
    excluded and may hold any of them.  private: an intermediate; recorded with a tolerance, compared with
    nothing.  fixed: bool like val, True where the kernel must leave exactly val (untouched or zeroed columns).
    dropped (outputs that are sums): val with one term of the sum left out, which the comparison must not accept
    (tests/test_route_refs_cpu.py)."""

    def __init__(self, val, M=None, N=1, bf16=False, exact=False, sel=None, slack=None, accept=None, private=False,
                 fixed=None, dropped=None):
        self.val, self.M, self.N, self.bf16, self.exact, self.dropped = val, M, N, bf16, exact, dropped
        self.sel, self.slack, self.accept, self.private, self.fixed = sel, slack, accept, private, fixed

    def excluded(self):
        """The fraction of this output's elements that are excluded."""
        if self.accept is not None:
            return float((self.accept.sum(-1) > 1).double().mean())
        if self.slack is not None:
            return float((self.slack.flatten() > 0).double().mean())
        return 0.0


def tdt(dt):
    return torch.bfloat16 if dt == BF16 else torch.float32


def host(a, dt, dtype):
    """A host input as the kernel sees it (rounded to bf16 in a bf16 case), in the computation's dtype.  The
    drivers' inputs are fp32 arrays; a float64 array (a test's consistent statistics) is taken as it is."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(torch.bfloat16) if dt == BF16 else t).to(dtype)


def bf16r(t):
    """t rounded to bf16 (nearest even), in its own dtype."""
    return t.to(torch.bfloat16).to(t.dtype) if t.dtype != torch.float64 else _bf16r64(t)


def _bf16r64(t):
    # float64 -> bf16 in one rounding (through float32 it would round twice): scale to the exponent
    m, e = torch.frexp(t)                      # t = m * 2^e, 0.5 <= |m| < 1; bf16 keeps 8 significant bits
    r = torch.ldexp(torch.round(m * 256.0), e - 8)   # torch.round: half to even
    return torch.where(torch.isfinite(t), r, t)


def bf16_ulp(t):
    """The spacing of bf16 at |t| (of the binade t lies in)."""
    _, e = torch.frexp(t.double())
    return torch.ldexp(torch.ones_like(t, dtype=torch.float64), e - 8)


def near_bf16_boundary(t, tol):
    """True where t lies within tol of a point at which its bf16 rounding changes."""
    lo, hi = bf16r(t.double() - tol), bf16r(t.double() + tol)
    return lo != hi


def round_op(v, dt):
    """An intermediate that one correctly rounded fp32 operation on fp32 operands forms and a bf16 case then
    stores: v is that operation's exact result, so the stored value is bf16(fp32(v)) with no doubt about it.
    (An fp32 case stores the fp32 value; its rounding is within every tolerance.)"""
    return bf16r(v.float()).to(v.dtype) if dt == BF16 else v


def round_mid(v, dt, tols, name, f=lambda t: t, extra=0.0):
    """A stored intermediate f(v) of several operations (f monotone, exact: the identity or a ReLU):
    (f(v) rounded to bf16 in a bf16 case, bool: v within ``tols[name]`` + extra of a point where that rounded
    value changes; extra: per element, what doubtful roundings upstream can move v by).  While the tolerances
    are being recorded (tols None) nothing is rounded: the float32 and float64 evaluations would part at
    every boundary between them."""
    if dt != BF16 or tols is None:
        return f(v), torch.zeros_like(v, dtype=torch.bool)
    t = tols[name] + extra
    return bf16r(f(v)), bf16r(f(v.double() - t)) != bf16r(f(v.double() + t))


def margin(N):
    return max(MARGIN, math.ceil(math.log2(max(N, 1)) / 2))


def tolerance(o64, o32):
    """tol of one float output from its float64 and float32 evaluations (module docstring)."""
    v64, v32 = o64.val.double().flatten(), o32.val.double().flatten()
    ok = torch.isfinite(v64) & torch.isfinite(v32)
    e32 = float((v32 - v64).abs()[ok].max()) if ok.any() else 0.0
    if o64.M is None:
        M = float(v64.abs()[ok].max()) if ok.any() else 0.0
    else:
        Mt = torch.as_tensor(o64.M, dtype=torch.float64).flatten()
        Mt = Mt[torch.isfinite(Mt)]
        M = float(Mt.max()) if Mt.numel() else 0.0
    return margin(o64.N) * max(e32, EPS32 * M, TINY)


def load_tol():
    with open(TOL_PATH) as f:
        return json.load(f)


def floats(t):
    """A kernel output as numbers: raw 32-bit words (the cross-entropy workspace and losses) are fp32."""
    return t.view(torch.float32) if t.dtype == torch.int32 else t


def check(cid, name, got, o, tol):
    """Assert that ``got`` (the kernel's output, a host tensor) is ``o`` within ``tol``; returns the largest
    error-to-allowance ratio (0 for an integer output).  A failure names the case, the output, the worst
    element's index, got, want and tol."""
    assert o.excluded() <= MAX_EXCLUDED, f"{cid} {name}: {o.excluded():.2e} of the elements excluded"
    g = got.flatten()
    if o.sel is not None:
        g = g[o.sel]
    want = o.val.flatten()
    assert g.numel() == want.numel(), f"{cid} {name}: {g.numel()} elements, the reference has {want.numel()}"
    if o.exact:
        assert tol == EXACT
        g, want = g.to(torch.int64), want.to(torch.int64)
        bad = g != want
        if o.accept is not None:
            acc = o.accept.reshape(want.numel(), -1)
            inside = (g >= 0) & (g < acc.shape[1])
            bad = ~(inside & acc[torch.arange(want.numel()), g.clamp(0, acc.shape[1] - 1)])
        if bad.any():
            i = int(bad.nonzero()[0])
            raise AssertionError(f"{cid} {name}: element {i} got {int(g[i])} want {int(want[i])} (exact); {int(bad.sum())} differ")
        return 0.0
    g, want = floats(g).double(), want.double()
    allow = torch.full_like(want, float(tol))
    if o.bf16:
        allow = allow + BF16_OUT * want.abs()
    if o.slack is not None:
        allow = allow + o.slack.flatten().double()
    if o.fixed is not None:
        allow = torch.where(o.fixed.flatten(), torch.zeros_like(allow), allow)
    nan = torch.isnan(want)
    err = (g - want).abs()
    err = torch.where(nan, torch.where(torch.isnan(g), torch.zeros_like(err), torch.full_like(err, math.inf)), err)
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    err = torch.where((g == want) & ~nan, torch.zeros_like(err), err)   # equal infinities
    ratio = torch.where(err == 0, torch.zeros_like(err), err / torch.where(nan, torch.ones_like(allow), allow))
    i = int(ratio.argmax())
    if not bool(ratio[i] <= 1.0):
        raise AssertionError(f"{cid} {name}: element {i} got {float(g[i])!r} want {float(want[i])!r} off by {float(err[i]):.3e}, "
                             f"tol {float(tol):.3e} (allowed there {float(allow[i]):.3e}); {int((ratio > 1).sum())} of "
                             f"{want.numel()} elements out of bounds")
    return float(ratio[i])


def check_case(cid, ref, got, tols):
    """Every public output of one case; returns {output name: worst ratio}."""
    names = [n for n, o in ref.items() if not o.private]
    assert sorted(names) == sorted(got), f"{cid}: outputs {sorted(got)}, the reference states {sorted(names)}"
    return {n: check(cid, n, got[n], ref[n], tols[n]) for n in names}


def unwritten(got):
    """True when a float output still holds UNWRITTEN everywhere."""
    return bool((got.float() == UNWRITTEN).all())
