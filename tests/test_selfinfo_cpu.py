"""AdvEnt's discriminator input without a GPU: the float64 statement of tests/selfinfo_ref.py against torch's float64
autograd of ADVENT's literal formula, the pinned tolerances (tests/pinned/selfinfo_tol.json), that the comparison
rejects the wrong kernels it must, the entry points' refusals (all ahead of any launch) and the config key."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import yaml

from rtsds_amd import _lib
from rtsds_amd import main as rmain
from rtsds_amd import train

from tests import route_compare as RC
from tests import selfinfo_ref as R
from tests.bn_bits_cases import BF16, F32
from tests.resize_bits_cases import _scale

F64 = torch.float64
PINNED = R.pinned()
ALL = list(range(len(R.CASES)))


def advent(p, c):
    """ADVENT's prob_2_entropy (ADVENT/advent/utils/func.py), literally."""
    return -p * torch.log2(p + 1e-30) / math.log2(c)


def _torch_scale(s):
    """The float for which ATen's 1 / scale is the driver's fp32 scale s exactly (ATen takes the reciprocal of the
    scale factor it is handed), or the nearest it gets to."""
    best = 1.0 / s
    for cand in (best, np.nextafter(best, 0), np.nextafter(best, 4), np.nextafter(np.nextafter(best, 0), 0),
                 np.nextafter(np.nextafter(best, 4), 4)):
        if 1.0 / float(cand) == s:
            return float(cand)
    return float(best)


def torch_self_information(x, size, dy):
    """(I, dI/dx . dy) by torch in float64: x [n][hi][wi][c] -> softmax(interpolate) -> ADVENT's formula.  The resize is
    the op F.interpolate(mode="bilinear", align_corners=False) calls, handed the output size together with the fp32
    scales the driver passes (F.interpolate itself takes one or the other)."""
    n, hi, wi, c = x.shape
    xt = x.permute(0, 3, 1, 2).clone().requires_grad_()
    z = torch._C._nn.upsample_bilinear2d(xt, list(size), False, _torch_scale(_scale(hi, size[0])), _torch_scale(_scale(wi, size[1])))
    info = advent(torch.softmax(z, 1), c).permute(0, 2, 3, 1)
    (info * dy).sum().backward()
    return info.detach(), xt.grad.permute(0, 2, 3, 1)


def _off(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()), float(b.abs().max())


# ------------------------------------------------------------------ the yardstick
@pytest.mark.parametrize("i", [i for i in ALL if R.CASES[i]["dt"] == F32], ids=lambda i: R.IDS[i])
def test_the_float64_statement_is_torchs_autograd_of_advents_formula(i):
    k = R.CASES[i]
    h, r64 = R.case(i)
    n, hi, wi, c, ho, wo = (k[a] for a in ("n", "hi", "wi", "c", "ho", "wo"))
    x = torch.from_numpy(h["x"]).double().view(n, hi, wi, c)
    dy = torch.from_numpy(h["dy"]).double().view(n, ho, wo, k["dyld"])[..., :c]
    info, grad = torch_self_information(x, (ho, wo), dy)
    (ev, mv), (eg, mg) = _off(r64["y"].val[..., :c], info), _off(r64["dx"].val, grad)
    print(f"{R.IDS[i]}: I off by {ev:.1e} of {mv:.3e}, gradient off by {eg:.1e} of {mg:.3e}")
    assert ev <= 1e-12 * mv and eg <= 1e-12 * mg
    assert 0.0 <= float(r64["y"].val.min()) and mv <= 1.0 / (math.e * math.log(c)) + 1e-15
    assert not bool(r64["y"].val[..., c:].any())


@pytest.mark.parametrize("c", [19, 7])
def test_the_special_rows_are_torchs_too(c):
    k = R.special_case(c, F32)
    dy = torch.from_numpy(R.host_inputs(k)["dy"]).double().view(4, c)
    y, dx = R.special_reference(c, dy)
    info, grad = torch_self_information(torch.from_numpy(R.special_head(c)).double(), (1, 4), dy.view(1, 1, 4, c))
    (ev, mv), (eg, mg) = _off(y, info[0, 0]), _off(dx, grad)
    print(f"c = {c}: I off by {ev:.1e} of {mv:.3e}, gradient off by {eg:.1e} of {mg:.3e}")
    assert ev <= 1e-12 * mv and eg <= 1e-12 * mg
    dx = dx[0, 0, ::2]                                                            # one pixel of each block
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all())
    assert float(y[0].abs().max()) < 1e-80                                        # one logit at 200 (exp(-200) is no zero in float64)
    assert float((y[1] - 1.0 / c).abs().max()) <= 1e-15                           # a constant row: I = 1 / c
    assert not bool(y[2, [1, 4, c - 1]].any()) and not bool(dx[2, [1, 4, c - 1]].any()) and bool(y[2].any())   # classes at -inf
    assert float(y[3, 2]) == float(y[3, 9 % c])                                   # two equal maxima


# ------------------------------------------------------------------ the case table and the pinned file
def test_the_geometries_of_the_issue_are_all_there_in_both_dtypes():
    table = [((2, 19, 16, 32), (128, 256)), ((1, 19, 13, 17), (97, 129)), ((1, 19, 9, 17), (64, 128)), ((2, 7, 9, 40), (64, 96)),
             ((1, 19, 8, 40), (24, 300)), ((1, 2, 4, 4), (8, 8)), ((1, 32, 4, 4), (8, 8)), ((1, 19, 8, 8), (8, 8)),
             ((1, 19, 2, 4200), (4, 256)), ((1, 19, 3, 70), (6, 140))]
    for (n, c, hi, wi), (ho, wo) in table:
        for dt in (F32, BF16):
            assert any((k["n"], k["c"], k["hi"], k["wi"], k["ho"], k["wo"], k["dt"]) == (n, c, hi, wi, ho, wo, dt) for k in R.CASES)
    # the last geometry of the issue's table stands for "each tile width the planner can return": one case per width below 64
    assert sum(1 for g in R.GEOS if g[0][1] == 32 and g[1] == (4, 384)) == 6
    assert any(k["yld"] == 32 for k in R.CASES) and any(k["yld"] == k["c"] for k in R.CASES) and any(k["dyld"] > k["c"] for k in R.CASES)


def test_the_pinned_file_is_a_fresh_recording():
    assert R.record() == PINNED
    assert sorted(PINNED) == sorted(R.IDS)


@pytest.mark.parametrize("i", ALL, ids=lambda i: R.IDS[i])
def test_no_element_is_excluded(i):
    for o in R.case(i)[1].values():
        assert o.excluded() == 0.0 and o.slack is None and o.accept is None and not o.private


# ------------------------------------------------------------------ the comparison notices what it must
def _stored(v, k):
    """Values as the kernel would have stored them."""
    return v.contiguous().to(torch.bfloat16) if k["dt"] == BF16 else v.contiguous().float()


def _rejects(cid, name, got, o, tol):
    with pytest.raises(AssertionError, match=cid[:20]):
        RC.check(cid, name, got, o, tol)
    return True


@pytest.mark.parametrize("i", ALL, ids=lambda i: R.IDS[i])
def test_the_comparison_accepts_the_float32_evaluation_and_rejects_wrong_kernels(i):
    k, cid, tols = R.CASES[i], R.IDS[i], PINNED[R.IDS[i]]
    h, r64 = R.case(i)
    r32 = R.reference(k, h, torch.float32)
    for name in ("y", "dx"):
        assert RC.check(cid, name, _stored(r32[name].val, k), r64[name], tols[name]) <= 1.0
        assert _rejects(cid, name, _stored(r32[name].dropped, k), r64[name], tols[name])      # one term of the sum left out
    for wrong in ("no_minus_one", "short_dot"):    # a_k without its - 1; class 0 left out of sum_k p_k u_k
        bad = R.reference(k, h, torch.float32, wrong=wrong)["dx"].val
        assert _rejects(cid, "dx", _stored(bad, k), r64["dx"], tols["dx"])
    # a pad column that is not exactly zero
    if k["yld"] > k["c"]:
        bad = _stored(r32["y"].val, k).clone()
        bad.view(-1, k["yld"])[0, k["c"]] = 1e-30
        assert _rejects(cid, "y", bad, r64["y"], tols["y"])


# ------------------------------------------------------------------ the entry points' refusals (no device: all ahead of any launch)
def _fwd(n=1, hi=4, wi=4, c=19, ho=8, wo=8, yld=32, dtype=_lib.F32):
    return _lib.load().rtsds_upselfinfo_fwd(1 << 20, 1 << 21, n, hi, wi, c, ho, wo, 0.5, 0.5, yld, dtype, None)


def _bwd(n=1, hi=4, wi=4, c=19, ho=8, wo=8, dyld=None, dtype=_lib.F32, ws=None):
    lib = _lib.load()
    need = lib.rtsds_upselfinfo_bwd_workspace(n, hi, wi, c, ho, wo)
    return lib.rtsds_upselfinfo_bwd(1 << 20, c if dyld is None else dyld, 1 << 21, 1 << 22, n, hi, wi, c, ho, wo, _scale(hi, max(ho, 1)),
                                    _scale(wi, max(wo, 1)), dtype, 1 << 23, need if ws is None else ws, None)


def test_the_entries_refuse_what_the_softmax_entries_refuse():
    SHAPE, UNSUPPORTED, WORKSPACE = 1, 2, 4
    assert _fwd(c=33) == SHAPE and _fwd(c=1) == SHAPE and _fwd(n=0) == SHAPE and _fwd(wo=0) == SHAPE
    assert _fwd(yld=18) == SHAPE and _fwd(yld=33) == SHAPE and _fwd(c=7, yld=6) == SHAPE
    assert _fwd(dtype=7) == UNSUPPORTED
    assert _bwd(c=33) == SHAPE and _bwd(c=1) == SHAPE and _bwd(n=0) == SHAPE and _bwd(ho=0) == SHAPE and _bwd(dyld=18) == SHAPE
    assert _bwd(ws=7) == WORKSPACE
    assert _bwd(dtype=7) == UNSUPPORTED
    (n, c, hi, wi), (ho, wo) = R.UNSUPPORTED_BWD      # no tile of the backward fits its LDS
    assert _bwd(n, hi, wi, c, ho, wo) == UNSUPPORTED


def test_the_entries_are_bound():
    for name, nargs in (("rtsds_upselfinfo_fwd", 13), ("rtsds_upselfinfo_bwd_workspace", 6), ("rtsds_upselfinfo_bwd", 16)):
        res, args = _lib.SIGNATURES[name]
        assert len(args) == nargs and res is (ctypes.c_size_t if name.endswith("workspace") else ctypes.c_int)
    lib = _lib.load()
    assert lib.rtsds_upselfinfo_bwd_workspace(2, 16, 32, 19, 128, 256) == lib.rtsds_upsoftmax_bwd_workspace(2, 16, 32, 19, 128, 256) > 0
    assert _lib.ABI_VERSION >= 28 and lib.rtsds_abi_version() == _lib.ABI_VERSION


# ------------------------------------------------------------------ the config key and da_step's keyword
def _config(value=None, **extra):
    cfg = yaml.safe_load(open(os.path.join(os.path.dirname(rmain.__file__), "config.yaml")))
    if value is not None:
        cfg["training"]["domain_adaptation"]["discriminator_input"] = value
    cfg["training"]["domain_adaptation"].update(extra)
    return rmain.namedtuple("Config", cfg.keys())(*cfg.values())


def test_the_config_key_is_parsed_and_an_unknown_value_is_refused():
    assert rmain.discriminator_input_config(_config()) == "softmax"                       # absent in the shipped file
    assert rmain.discriminator_input_config(_config("softmax")) == "softmax"
    assert rmain.discriminator_input_config(_config("self_information")) == "self_information"
    for bad in ("entropy", "Softmax", "", 1, True, ["softmax"]):
        with pytest.raises(RuntimeError, match="discriminator_input"):
            rmain.discriminator_input_config(_config(bad))
    assert sorted(train.D_INPUTS) == ["self_information", "softmax"]


def test_da_step_refuses_an_unknown_input_before_it_touches_anything():
    with pytest.raises(ValueError, match="d_input"):
        train.da_step(None, None, None, None, None, None, None, None, None, 0.1, 1, d_input="entropy")
