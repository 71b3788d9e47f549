"""rtsds_color_jitter (csrc/data.hip) and its place in the image pipeline against the fp64
restatement of torchvision's ColorJitter (tests/colorjitter_ref.py).

Tolerance: the map is continuous (sector and tie switches of the hue do not jump), so an
absolute bound is meaningful.  It is 4 x e32, e32 = the largest |fp32 restatement - fp64
restatement| over the cases of the test at hand, computed here on the CPU: what fp32 arithmetic
alone costs, times 4 for fma contraction, the device's division and floor-mod, and another
summation order in the grey mean.  Every test prints the error the GPU shows next to e32.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

from oracle import transforms as OT  # noqa: E402
from rtsds_amd import transforms as T  # noqa: E402
from tests import colorjitter_ref as R  # noqa: E402

DEV = "cuda"
MEAN, STD = T.IMAGENET_MEAN, T.IMAGENET_STD
GTA5 = (1052, 1914, 1)  # (h, w, seed)
ORDER = (2, 0, 1, 3)    # contrast in the middle


@functools.lru_cache(maxsize=None)
def _image(key):
    """'I' -> the parity image; (h, w, seed) -> seeded noise.  uint8 [3, H, W], never modified."""
    return R.parity_image() if key == "I" else R.random_image(*key)


@functools.lru_cache(maxsize=None)
def _refs(key, order, factors, bound=255.0):
    img = _image(key)  # on another scale: the fp32 image the kernel is given, taken as exact
    return R.refs(img if bound == 255.0 else (img.double() / 255.0 * bound).float(), order, factors, bound)


def _e32(cases):
    return max(_refs(*c)[1] for c in cases)


def _run(key, order, factors, src="u8", bound=255.0, inplace=False):
    """The kernel on image `key`: [3, H, W] fp32 on the CPU."""
    hwc = _image(key).permute(1, 2, 0).contiguous()
    if src == "f32":
        hwc = hwc.float() if bound == 255.0 else (hwc.double() / 255.0 * bound).float()
    x = hwc.to(DEV)
    out = T.color_jitter(x, order, *factors, value_range=bound, out=x if inplace else None)
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and out.shape == hwc.shape
    assert (out.data_ptr() == x.data_ptr()) == inplace
    return out.cpu().permute(2, 0, 1)


def _check(got, case, e32, what, scale=1.0):
    ref = _refs(*case)[0]
    err = (got.double() - ref).abs().max().item()
    print(f"{what}: gpu err {err:.3e}, e32 {e32:.3e}, bound {4 * e32 * scale:.3e}")
    assert e32 > 0
    assert err <= 4 * e32 * scale, (what, err, e32)


# ------------------------------------------------------------------ single ops
# each op alone, at both ends of a range (brightness / contrast / saturation 0.2 .. 1.8, hue the
# whole circle), from a uint8 and from an fp32 source
SINGLE = [(k, f) for k, ends in enumerate([(0.2, 1.8), (0.2, 1.8), (0.2, 1.8), (-0.5, 0.5)]) for f in ends]


def _single_case(k, f):
    return ("I", (0, 1, 2, 3), tuple(f if j == k else None for j in range(4)))


@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("k,f", SINGLE)
def test_single_op(k, f, src):
    e32 = _e32([_single_case(*c) for c in SINGLE])
    case = _single_case(k, f)
    _check(_run("I", case[1], case[2], src=src), case, e32, f"op {k} factor {f} {src}")


# ------------------------------------------------------------------ orders
ALL_SETS = dict(R.SETS, saturating=R.SATURATING)


@pytest.mark.parametrize("name", sorted(ALL_SETS))
def test_all_orders(name):
    factors = ALL_SETS[name]
    cases = [("I", order, factors) for order in R.ORDERS]
    e32 = _e32(cases)
    worst = 0.0
    for case in cases:
        ref = _refs(*case)[0]
        share = ((ref <= 0) | (ref >= 255.0)).double().mean().item()
        if name != "saturating":  # the clamp must not hide errors
            assert share <= 0.25, (case, share)
        got = _run(*case)
        worst = max(worst, (got.double() - ref).abs().max().item())
        assert worst <= 4 * e32, (case, worst, e32)
    print(f"{name}: 24 orders, gpu err {worst:.3e}, e32 {e32:.3e}")


SUBSETS = {"hue": (3,), "contrast": (1,), "brightness+saturation": (0, 2)}


@pytest.mark.parametrize("order", [(0, 1, 2, 3), (3, 2, 1, 0), ORDER])
@pytest.mark.parametrize("name", sorted(R.SETS))
@pytest.mark.parametrize("subset", sorted(SUBSETS))
def test_subsets_with_ops_off(subset, name, order):
    def case(sub, nm, od):
        return ("I", od, tuple(f if k in SUBSETS[sub] else None for k, f in enumerate(R.SETS[nm])))
    e32 = _e32([case(s, n, o) for s in SUBSETS for n in R.SETS for o in [(0, 1, 2, 3), (3, 2, 1, 0), ORDER]])
    c = case(subset, name, order)
    _check(_run(*c), c, e32, f"{subset} {name} {order}")


# ------------------------------------------------------------------ shapes
SHAPES = [(1, 1, 1), (1, 5, 1), (3, 64, 1), (64, 96, 1), GTA5]


@pytest.mark.parametrize("src", ["u8", "f32"])
@pytest.mark.parametrize("key", SHAPES, ids=lambda k: f"{k[0]}x{k[1]}")
def test_shapes(key, src):
    """A single pixel, a vector tail, exact multiples, and GTA5's size (more pixels than one pass
    of the capped reduction grid covers, every partial in use, contrast in the middle)."""
    e32 = _e32([(k, ORDER, R.SETS["set1"]) for k in SHAPES])
    case = (key, ORDER, R.SETS["set1"])
    _check(_run(*case, src=src), case, e32, f"{key} {src}")


def test_unaligned_views_take_the_scalar_path():
    """A source / destination whose base is not 16-byte (fp32) or 4-byte (uint8) aligned."""
    case = ((64, 96, 1), ORDER, R.SETS["set1"])
    e32 = _e32([case])
    hwc = _image(case[0]).permute(1, 2, 0).contiguous()
    n = hwc.numel()
    for src in (hwc, hwc.float()):
        flat = torch.empty(n + 1, dtype=src.dtype, device=DEV)
        flat[1:] = src.reshape(-1).to(DEV)
        oflat = torch.empty(n + 1, dtype=torch.float32, device=DEV)
        out = T.color_jitter(flat[1:].view(hwc.shape), case[1], *case[2], out=oflat[1:].view(hwc.shape))
        torch.cuda.synchronize()
        _check(out.cpu().permute(2, 0, 1), case, e32, f"offset {src.dtype}")


def test_bound_one():
    """I / 255 as fp32 with value_range 1: torchvision's literal float-image result."""
    e32 = _e32([("I", order, R.SETS["set1"]) for order in R.ORDERS])
    case = ("I", ORDER, R.SETS["set1"], 1.0)
    _check(_run("I", ORDER, R.SETS["set1"], src="f32", bound=1.0), case, e32, "bound 1", scale=1.0 / 255.0)


def test_in_place_is_bit_identical():
    for key in ["I", (64, 96, 1)]:
        a = _run(key, ORDER, R.SETS["set1"], src="f32")
        b = _run(key, ORDER, R.SETS["set1"], src="f32", inplace=True)
        assert torch.equal(a, b)


def test_uint8_and_fp32_sources_agree_bitwise():
    assert torch.equal(_run("I", ORDER, R.SETS["set2"], src="u8"), _run("I", ORDER, R.SETS["set2"], src="f32"))


def test_deterministic():
    a = _run(GTA5, ORDER, R.SETS["set1"])
    b = _run(GTA5, ORDER, R.SETS["set1"])
    assert torch.equal(a, b)


def test_python_layer_refuses_what_the_kernel_does_not_take():
    x = torch.zeros((4, 4, 3), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError):
        T.color_jitter(x.permute(2, 0, 1), (0, 1, 2, 3), 1.2, None, None, None)      # not contiguous HWC
    with pytest.raises(RuntimeError):
        T.color_jitter(x.half(), (0, 1, 2, 3), 1.2, None, None, None)                 # dtype
    with pytest.raises(RuntimeError):
        T.color_jitter(x.to(torch.uint8), (0, 1, 2, 3), 1.2, None, None, None, out=x.to(torch.uint8))
    with pytest.raises(RuntimeError):
        T.color_jitter(x, (0, 1, 2, 2), 1.2, None, None, None)                        # not a permutation


# ------------------------------------------------------------------ pipeline, end to end
def _pipeline_case(jitter_first):
    """Seeded RandomApply([GaussianBlur, RandomHorizontalFlip(1.0), ColorJitter], p=1.0) (or with
    the jitter listed first) into ImagePipeline((60, 100)), against blur -> flip -> jitter ->
    resize -> normalize with the draws replayed here.  Returns (fp32 output, bf16 output, ref,
    bound): bound = 1e-4 max|ref| (the blur test's bound) + 4 e32 / min(STD) -- the blur and the
    resize are convex combinations, so they do not amplify the jitter's absolute error, and
    Normalize divides by std."""
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (120, 200, 3), generator=g, dtype=torch.uint8)
    blur = T.GaussianBlur((5, 9), (0.1, 5.0))
    cj = T.ColorJitter(0.4, 0.4, 0.4, 0.2)
    flip = T.RandomHorizontalFlip(1.0)
    pipe = T.ImagePipeline((60, 100), augment=T.RandomApply([cj, blur, flip] if jitter_first else [blur, flip, cj],
                                                            p=1.0))
    torch.manual_seed(123)
    out = pipe([img.to(DEV)], dtype=torch.float32)[0].cpu()
    torch.manual_seed(123)
    out16 = pipe([img.to(DEV)], dtype=torch.bfloat16)[0].float().cpu()

    def draw_jitter():
        order = tuple(torch.randperm(4).tolist())
        return order, [float(torch.empty(1).uniform_(lo, hi)) for lo, hi in
                       [(0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.2, 0.2)]]

    def jitter(x, order, factors):
        r64 = R.color_jitter(x.double(), order, *factors)
        e32 = (R.color_jitter(x.float(), order, *factors).double() - r64).abs().max().item()
        return r64.float(), e32

    torch.manual_seed(123)
    torch.rand(1)  # RandomApply's coin
    x = img.permute(2, 0, 1).float()
    if jitter_first:
        order, factors = draw_jitter()
        sigma = torch.empty(1).uniform_(0.1, 5.0).item()
        torch.rand(1)  # the flip's coin
        x, e32 = jitter(x, order, factors)
        x = OT.gaussian_blur(x, (5, 9), (sigma, sigma)).flip(-1)
    else:
        sigma = torch.empty(1).uniform_(0.1, 5.0).item()
        torch.rand(1)
        order, factors = draw_jitter()
        x, e32 = jitter(OT.gaussian_blur(x, (5, 9), (sigma, sigma)).flip(-1), order, factors)
    ref = OT.normalize(OT.resize(x, (60, 100)), MEAN, STD)
    return out, out16, ref, 1e-4 * ref.abs().max().item() + 4 * e32 / min(STD), e32


@pytest.mark.parametrize("jitter_first", [False, True], ids=["blur-flip-jitter", "jitter-blur-flip"])
def test_pipeline_end_to_end(jitter_first):
    out, out16, ref, bound, e32 = _pipeline_case(jitter_first)
    err = (out - ref).abs().max().item()
    print(f"pipeline jitter_first={jitter_first}: gpu err {err:.3e}, e32 {e32:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    # bf16: the fp32 output rounded once
    assert torch.equal(out16, out.to(torch.bfloat16).float()) or \
        ((out16 - ref).abs() <= 8e-3 * ref.abs() + 1e-2).all()


def test_pipeline_without_color_jitter_is_unchanged_by_a_switched_off_one():
    """A ColorJitter with every op off draws its permutation but leaves the pixels alone."""
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (120, 200, 3), generator=g, dtype=torch.uint8).to(DEV)
    blur = T.GaussianBlur((5, 9), (0.1, 5.0))
    torch.manual_seed(7)
    a = T.ImagePipeline((60, 100), augment=T.RandomApply([blur], p=1.0))([img], dtype=torch.float32)
    torch.manual_seed(7)
    b = T.ImagePipeline((60, 100), augment=T.RandomApply([blur, T.ColorJitter()], p=1.0))([img], dtype=torch.float32)
    assert torch.equal(a, b)
