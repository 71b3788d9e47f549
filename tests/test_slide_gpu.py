"""Sliding-window prediction on the device (rtsds_slide_paint, functional.slide_paint,
validation.predict_sliding, val(window=), predict.Predictor(stride=), python -m rtsds_amd.predict
--stride).

Every comparison in this file is EXACT.  The oracle is the chain of existing entries: per window,
in order, functional.upsample_softmax_accumulate (rtsds_upsoftmax_acc, accumulate=False, the
window's flip) into a scratch tensor, then a torch slice add onto a zero fp32 canvas; the arg-max
is taken on the host (first maximum), ids and colours follow tests/paint_ref.py.  The fp32 sums are
compared through an int32 view; byte outputs are pre-filled with a sentinel and sit, at odd byte
offsets, inside larger buffers of guard bytes."""
import functools
import itertools

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle.weights import recipe_state_dict, synthetic_images, synthetic_labels  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import predict, utils, validation  # noqa: E402
from rtsds_amd import transforms as T  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from tests import paint_ref as R  # noqa: E402
from tests import slide_ref as S  # noqa: E402

DEV = torch.device("cuda", 0)
CL = torch.channels_last
GUARD = 0xA5  # no id (< 200) and no class takes this value
# name -> (head (hi, wi), window, canvas, stride)
SHAPES = {
    "base": ((4, 6), (32, 48), (40, 80), (8, 16)),         # x8: 6 windows, 12 with flip
    "nonint": ((5, 7), (32, 48), (40, 80), (8, 16)),       # x6.4 / x6.86, a size= resize
    "tiles": ((4, 12), (32, 96), (40, 300), (8, 68)),      # two column tiles; window edges at 68, 96, 136, 164, 204,
                                                           # 232 inside them, the tile boundary 256 inside the last window
    "unstaged": ((2, 4200), (4, 256), (6, 300), (2, 44)),  # 2 x 4191 x c x 4 B of taps > 48 KiB: rows read from memory
}
# the kernel's routes, named: (shape, c).  staged-cc19 / staged-rt: source rows through LDS with the
# compile-time / run-time class count; unstaged-rt: rows from memory (run-time count only, c = 19 too)
ROUTES = {"staged-cc19": ("base", 19), "staged-rt7": ("base", 7), "unstaged-rt19": ("unstaged", 19),
          "unstaged-rt7": ("unstaged", 7)}
DTS = [torch.float32, torch.bfloat16]
dts = pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])
flips = pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])


def _heads(nwin, nf, c, hi, wi, dt, seed=0):
    g = torch.Generator().manual_seed(nwin * 7 + hi + 1000 * seed)
    x = torch.randn(nwin * nf, c, hi, wi, generator=g, dtype=torch.float64) * 3
    return x.to(DEV, dt).contiguous(memory_format=CL)


def _chain(x, geo, table, nf, canvas, start=None):
    """The oracle: (fp32 sums [nf, H, W, c] on the host, the windows' own probability tensors)."""
    hw, ww = geo[:2]
    c = x.shape[1]
    acc = torch.zeros((nf, canvas[0], canvas[1], c), dtype=torch.float32, device=DEV) if start is None else start.clone()
    probs = []
    for k, (y0, x0, m) in enumerate(table):
        tmp = torch.full((nf, hw, ww, c), float("nan"), dtype=torch.float32, device=DEV)
        F.upsample_softmax_accumulate(x[k * nf:(k + 1) * nf], geo, tmp, flip=bool(m), accumulate=False)
        acc[:, y0:y0 + hw, x0:x0 + ww] += tmp
        probs.append(tmp.cpu().numpy())
    return acc.cpu().numpy(), probs


@functools.lru_cache(maxsize=None)
def _case(shape, c, dt, nf, flip):
    """(x, geometry, table, canvas, oracle sums, oracle classes, palette, lut, frame) -- computed
    once, shared by the tests, never written to."""
    (hi, wi), window, canvas, stride = SHAPES[shape]
    table = validation.slide_table(canvas, window, stride, flip)
    x = _heads(len(table), nf, c, hi, wi, dt)
    geo = F.upsample_geometry(x, size=window)
    want, probs = _chain(x, geo, table, nf, canvas)
    assert np.array_equal(S.covering_sum(probs, table, canvas).view(np.int32), want.view(np.int32))  # the restatement
    g = torch.Generator().manual_seed(100 + c)
    pal = predict.default_palette() if c == 19 else torch.randint(0, 256, (c, 3), generator=g, dtype=torch.uint8)
    lut = torch.randperm(200, generator=g)[:c].to(torch.uint8)  # distinct ids, not the identity
    frame = torch.randint(0, 256, (nf, canvas[0], canvas[1], 3), generator=g, dtype=torch.uint8)
    frame[:, : canvas[0] // 2, : canvas[1] // 3] = 0
    frame[:, canvas[0] // 2:, canvas[1] // 2:] = 255
    return x, geo, table, canvas, want, S.argmax_first(want), pal, lut, frame


def _guarded(shape, off):
    numel = int(np.prod(shape))
    buf = torch.full((numel + off + 61,), GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[off:off + numel].view(shape)


def _guards_intact(buf, view, off):
    b = buf.cpu()
    return bool((b[:off] == GUARD).all()) and bool((b[off + view.numel():] == GUARD).all())


def _placed(t, off):
    _, v = _guarded(tuple(t.shape), off)
    v.copy_(t)
    return v


def _nan_acc(nf, canvas, c):
    return torch.full((nf, canvas[0], canvas[1], c), float("nan"), dtype=torch.float32, device=DEV)


def _same_bits(acc, want):
    return np.array_equal(acc.cpu().numpy().view(np.int32), want.view(np.int32))


def _check(shape, c, dt, nf, flip):
    x, geo, table, canvas, want, cls, pal, lut, frame = _case(shape, c, dt, nf, flip)
    H, W = canvas
    assert len(np.unique(cls)) > 1  # the map is not constant
    pal_d, lut_d, frame_d = pal.to(DEV), lut.to(DEV), _placed(frame, 7)
    # everything at once: sums, ids through the lut, a blend
    acc = _nan_acc(nf, canvas, c)
    ibuf, ids = _guarded((nf, H, W), 13)
    cbuf, rgb = _guarded((nf, H, W, 3), 5)
    out = F.slide_paint(x, geo, table, canvas, nf, palette=pal_d, alpha=0.5, frame=frame_d, lut=lut_d, acc=acc, ids=ids, rgb=rgb)
    assert out[0] is ids and out[1] is rgb
    torch.cuda.synchronize()
    assert _same_bits(acc, want)
    assert np.array_equal(ids.cpu().numpy(), R.ids_ref(cls, lut.numpy()))
    assert np.array_equal(rgb.cpu().numpy(), R.paint_ref(cls, pal.numpy(), 128, frame.numpy()))
    assert _guards_intact(ibuf, ids, 13) and _guards_intact(cbuf, rgb, 5)
    assert np.array_equal(frame_d.cpu().numpy(), frame.numpy())  # the frame is only read
    # the common path: no fp32 canvas, the mask alone
    ibuf, ids = _guarded((nf, H, W), 3)
    cbuf, rgb = _guarded((nf, H, W, 3), 11)
    F.slide_paint(x, geo, table, canvas, nf, palette=pal_d, ids=ids, rgb=rgb)
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy(), cls.astype(np.uint8))
    assert np.array_equal(rgb.cpu().numpy(), pal.numpy()[cls])
    assert _guards_intact(ibuf, ids, 3) and _guards_intact(cbuf, rgb, 11)


# ----------------------------------------------------------------------------- chain identity
@flips
@pytest.mark.parametrize("nf", [1, 2])
@dts
@pytest.mark.parametrize("c", [19, 7, 2, 32])
def test_base_case_equals_the_chain(c, dt, nf, flip):
    assert len(_case("base", c, dt, nf, flip)[2]) == (12 if flip else 6)
    _check("base", c, dt, nf, flip)


@flips
@dts
def test_non_integer_geometry(dt, flip):
    _check("nonint", 19, dt, 2, flip)


@flips
@dts
def test_two_tiles_per_row_with_window_edges_inside(dt, flip):
    table = _case("tiles", 19, dt, 1, flip)[2]
    assert sorted({x0 for _, x0, _ in table}) == [0, 68, 136, 204]
    _check("tiles", 19, dt, 1, flip)


@flips
@dts
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route(route, dt, flip):
    shape, c = ROUTES[route]
    _check(shape, c, dt, 2 if shape == "base" else 1, flip)


# ----------------------------------------------------------------------------- accumulate
@flips
@dts
def test_split_calls_equal_the_single_call(dt, flip):
    x, geo, table, canvas, want, cls, pal, lut, frame = _case("tiles", 19, dt, 1, flip)
    nf, pal_d, frame_d = 1, pal.to(DEV), frame.to(DEV)
    for m in (1, len(table) // 2, len(table) - 1):
        acc = _nan_acc(nf, canvas, 19)
        none = F.slide_paint(x[:m * nf], geo, table[:m], canvas, nf, acc=acc, want_ids=False)  # acc alone
        assert none == (None, None)
        ids, rgb = F.slide_paint(x[m * nf:], geo, table[m:], canvas, nf, palette=pal_d, alpha=0.25, frame=frame_d, acc=acc,
                                 accumulate=True)
        torch.cuda.synchronize()
        assert _same_bits(acc, want), m
        assert np.array_equal(ids.cpu().numpy(), cls.astype(np.uint8)), m
        assert np.array_equal(rgb.cpu().numpy(), R.paint_ref(cls, pal.numpy(), 64, frame.numpy())), m


# ----------------------------------------------------------------------------- uncovered pixels
@dts
def test_uncovered_pixels(dt):
    (hi, wi), window, _, _ = SHAPES["base"]
    canvas, nf, c = (50, 300), 2, 19
    x = _heads(1, nf, c, hi, wi, dt, seed=3)
    geo = F.upsample_geometry(x, size=window)
    g = torch.Generator().manual_seed(5)
    lut, pal = torch.randperm(200, generator=g)[:c].to(torch.uint8), predict.default_palette()
    for y0, x0 in ((0, 0), (18, 252)):  # the corners; the second window spans the tile boundary
        table = [(y0, x0, 1)]
        want, _ = _chain(x, geo, table, nf, canvas)
        inside = np.zeros(canvas, bool)
        inside[y0:y0 + window[0], x0:x0 + window[1]] = True
        acc = _nan_acc(nf, canvas, c)
        ids, rgb = F.slide_paint(x, geo, table, canvas, nf, palette=pal.to(DEV), lut=lut.to(DEV), acc=acc)
        torch.cuda.synchronize()
        assert _same_bits(acc, want) and not acc[:, torch.from_numpy(~inside).to(DEV)].any()  # zeros, none of the NaNs left
        assert (ids.cpu().numpy()[:, ~inside] == int(lut[0])).all()
        assert (rgb.cpu().numpy()[:, ~inside] == pal.numpy()[0]).all()
        cls = S.argmax_first(want)
        assert np.array_equal(ids.cpu().numpy(), R.ids_ref(cls, lut.numpy())) and len(np.unique(cls[:, inside])) > 1
        # accumulate: the old sums are kept there, and decide the class
        old = torch.rand((nf,) + canvas + (c,), generator=g, dtype=torch.float32).to(DEV)
        want2, _ = _chain(x, geo, table, nf, canvas, start=old)
        acc = old.clone()
        ids, _ = F.slide_paint(x, geo, table, canvas, nf, acc=acc, accumulate=True)
        torch.cuda.synchronize()
        assert _same_bits(acc, want2)
        out = torch.from_numpy(~inside).to(DEV)
        assert torch.equal(acc[:, out], old[:, out])
        assert np.array_equal(ids.cpu().numpy(), S.argmax_first(want2).astype(np.uint8))


# ----------------------------------------------------------------------------- ties
@dts
def test_ties_keep_the_first_class(dt):
    (hi, wi), window, canvas, stride = SHAPES["base"]
    table = validation.slide_table(canvas, window, stride)
    geo = F.upsample_geometry(torch.empty(1, 19, hi, wi), size=window)
    flat = torch.full((len(table), 19, hi, wi), 1.25, dtype=dt, device=DEV).contiguous(memory_format=CL)
    acc = _nan_acc(1, canvas, 19)
    ids, _ = F.slide_paint(flat, geo, table, canvas, 1, acc=acc)
    assert int(ids.max()) == 0  # uniform sums: the first class
    assert all(torch.equal(acc[..., k], acc[..., 0]) for k in range(19)) and _same_bits(acc, _chain(flat, geo, table, 1, canvas)[0])
    # two classes equal only after the summation: small integers through a x8 resize are exact, window 0
    # holds (3, 1, 0), window 1 (1, 3, 0) -- each prefers another class, their probabilities are each
    # other's mirror image, and the fp32 add commutes: where both cover a pixel classes 0 and 1 tie
    two = [(0, 0, 0), (8, 16, 0)]
    x = torch.zeros(2, 3, hi, wi, dtype=dt, device=DEV)
    x[0, 0], x[0, 1], x[1, 0], x[1, 1] = 3.0, 1.0, 1.0, 3.0
    x = x.contiguous(memory_format=CL)
    acc = _nan_acc(1, canvas, 3)
    ids, _ = F.slide_paint(x, geo, two, canvas, 1, acc=acc)
    torch.cuda.synchronize()
    assert _same_bits(acc, _chain(x, geo, two, 1, canvas)[0])
    a, i = acc.cpu().numpy()[0], ids.cpu().numpy()[0]
    assert np.array_equal(a[8:32, 16:48, 0].view(np.int32), a[8:32, 16:48, 1].view(np.int32)) and a[8, 16, 0] > a[8, 16, 2]
    assert (i[8:32, 16:48] == 0).all()                        # the tie: the first of the two
    assert (i[:8, :48] == 0).all() and (i[32:, 16:64] == 1).all()  # one window alone: its own class
    assert (i[:, 64:] == 0).all() and (i[32:, :16] == 0).all()   # no window: zeros, class 0
    swapped, _ = F.slide_paint(x.flip(0).contiguous(memory_format=CL), geo, two, canvas, 1)
    assert (swapped[0, 8:32, 16:48] == 0).all() and (swapped[0, :8, :48] == 1).all()


# ----------------------------------------------------------------------------- optional outputs
@pytest.mark.parametrize("alpha_q8", [0, 128, 256])
def test_optional_outputs(alpha_q8):
    x, geo, table, canvas, want, cls, pal, lut, frame = _case("base", 19, torch.bfloat16, 2, True)
    nf, (H, W) = 2, canvas
    pal_d, lut_d, frame_d = pal.to(DEV), lut.to(DEV), _placed(frame, 9)
    for use_acc, use_ids, use_rgb, use_lut in itertools.product((False, True), repeat=4):
        if not (use_acc or use_ids or use_rgb):
            continue
        acc = _nan_acc(nf, canvas, 19) if use_acc else None
        ids, rgb = F.slide_paint(x, geo, table, canvas, nf, palette=pal_d if use_rgb else None, alpha=alpha_q8 / 256.0,
                                 frame=frame_d if use_rgb else None, lut=lut_d if use_lut else None, acc=acc, want_ids=use_ids)
        torch.cuda.synchronize()
        key = (use_acc, use_ids, use_rgb, use_lut)
        assert (ids is not None) == use_ids and (rgb is not None) == use_rgb, key
        if use_acc:
            assert _same_bits(acc, want), key
        if use_ids:
            assert np.array_equal(ids.cpu().numpy(), R.ids_ref(cls, lut.numpy() if use_lut else None)), key
        if use_rgb:
            assert np.array_equal(rgb.cpu().numpy(), R.paint_ref(cls, pal.numpy(), alpha_q8, frame.numpy())), key


def test_refusals():
    x, geo, table, canvas, _, _, pal, lut, frame = _case("base", 19, torch.float32, 2, False)
    nf, (H, W) = 2, canvas
    good_i = torch.zeros((nf, H, W), dtype=torch.uint8, device=DEV)
    good_c = torch.zeros((nf, H, W, 3), dtype=torch.uint8, device=DEV)
    good_a = torch.zeros((nf, H, W, 19), dtype=torch.float32, device=DEV)
    pal_d, frame_d = pal.to(DEV), frame.to(DEV)
    bad = [{"ids": good_i.to(torch.int8)}, {"ids": good_i[:, :, :-1]}, {"ids": good_i.cpu()}, {"rgb": good_c[:1]},
           {"acc": good_a.double()}, {"acc": good_a[..., :7]}, {"acc": good_a.cpu()}, {"acc": None, "accumulate": True},
           {"frame": frame_d[:, :-1], "alpha": 0.5}, {"alpha": 0.5}, {"alpha": 1.5}, {"palette": pal_d[:5]}, {"palette": None},
           {"lut": lut.to(DEV)[:7]}, {"lut": lut}]
    for kw in bad:
        with pytest.raises(RuntimeError, match="^rtsds_amd: slide_paint"):
            F.slide_paint(x, geo, table, canvas, nf, **dict({"palette": pal_d, "ids": good_i, "rgb": good_c, "acc": good_a}, **kw))
    for args in ((x, geo, table + [(9, 0, 0)], canvas, nf), (x, geo, table, (40, 79), nf), (x, geo, table, canvas, 1),
                 (x, geo, table[:5], canvas, nf), (x[:, :1], geo, table, canvas, nf), (x.double(), geo, table, canvas, nf),
                 (x[:0], geo, [], canvas, nf), (x.repeat(11, 1, 1, 1), geo, table * 11, canvas, nf)):
        with pytest.raises(RuntimeError, match="^rtsds_amd: slide_paint"):
            F.slide_paint(*args)
    with pytest.raises(RuntimeError, match="^rtsds_amd: slide_paint"):
        F.slide_paint(x, geo, table, canvas, nf, want_ids=False)  # nothing to produce
    torch.cuda.synchronize()
    assert int(good_i.max()) == 0 and int(good_c.max()) == 0 and float(good_a.max()) == 0.0  # nothing was launched


# ----------------------------------------------------------------------------- the model paths
SIZE = (64, 128)  # the smallest BiSeNet-R18 input of the model tests


def _net(seed=1):
    net = BiSeNet(19, "resnet18")
    sd = net.state_dict()
    net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed))
    return net


def _frames(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]


@pytest.mark.parametrize("max_batch", [8, 4, 2], ids=["one-chunk", "two-chunks", "nwin-chunks"])
def test_predict_sliding_equals_the_chain(max_batch):
    """The same crops through the same forwards, chunk by chunk, then the oracle chain over all heads."""
    net = _net().to(DEV).train()
    n, (H, W), stride = 2, (96, 192), (32, 64)
    inputs = synthetic_images(n, H, W, seed=7).to(DEV)
    with rtsds_amd.precision(torch.float32):
        acc, pred = validation.predict_sliding(net, inputs, SIZE, stride=stride, max_batch=max_batch, want_acc=True)
        assert net.training  # restored
        table = validation.slide_table((H, W), SIZE, stride)
        chunks = validation.slide_chunks(table, n, max_batch)
        assert len(table) == 4 and len(chunks) == {8: 1, 4: 2, 2: 4}[max_batch]
        net.eval()
        lows = []
        with torch.no_grad():
            for chunk in chunks:
                crops = torch.cat([inputs[:, :, y0:y0 + SIZE[0], x0:x0 + SIZE[1]] for y0, x0, _ in chunk]).contiguous()
                lows.append(net.forward_lowres(crops, main_only=True)[0][0])
        low = torch.cat(lows)
        want, _ = _chain(low, F.upsample_geometry(low, size=SIZE), table, n, (H, W))
        assert _same_bits(acc, want) and pred.dtype == torch.int64 and tuple(pred.shape) == (n, H, W)
        assert np.array_equal(pred.cpu().numpy(), S.argmax_first(want)) and len(np.unique(S.argmax_first(want))) > 1
        if max_batch == 8:  # one chunk: no fp32 canvas unless asked for, the same classes
            none, pred2 = validation.predict_sliding(net, inputs, SIZE, stride=stride, max_batch=max_batch)
            assert none is None and torch.equal(pred2, pred)


@flips
def test_one_window_equal_to_the_canvas_is_predict_multiscale(flip):
    net = _net().to(DEV).eval()
    n = 2
    inputs = synthetic_images(n, *SIZE, seed=11).to(DEV)
    with rtsds_amd.precision(torch.float32):
        acc, pred = validation.predict_sliding(net, inputs, SIZE, flip=flip, max_batch=n, want_acc=True)  # a window per forward
        acc2, pred2 = validation.predict_multiscale(net, inputs, SIZE, scales=(1.0,), flip=flip)
    assert torch.equal(acc.view(torch.int32), acc2.view(torch.int32)) and torch.equal(pred, pred2)


def _by_hand(net, big, table, per, dt, **paint):
    """Slices, ImagePipeline, forward_lowres (``per`` windows per forward), one slide_paint call."""
    n, lows = len(big), []
    net.eval()
    with torch.no_grad(), rtsds_amd.precision(dt):
        for i in range(0, len(table), per):
            chunk = table[i:i + per]
            crops = [f[y0:y0 + SIZE[0], x0:x0 + SIZE[1]] for y0, x0, _ in chunk for f in big]
            crops = [(torch.flip(cr, dims=[1]) if chunk[j // n][2] else cr).contiguous() for j, cr in enumerate(crops)]
            lows.append(net.forward_lowres(T.ImagePipeline(SIZE)(crops), main_only=True)[0][0])
    low = torch.cat(lows)
    geo = F.upsample_geometry(low, size=SIZE)
    canvas = tuple(big[0].shape[:2])
    return F.slide_paint(low, geo, table, canvas, n, **paint), S.argmax_first(_chain(low, geo, table, n, canvas)[0])


@dts
def test_predictor_stride_equals_the_op_chain(dt):
    net = _net().to(DEV).train()
    frames = _frames(((96, 192), (48, 160), (96, 192)), 5)  # two frames slide as one batch, one is too small
    kw = dict(label_ids=predict.CITYSCAPES_LABEL_IDS, alpha=0.5, dtype=dt)
    ids, rgb = predict.Predictor(net, SIZE, stride=(32, 64), flip=True, **kw)(frames)
    assert net.training and len(ids) == len(rgb) == 3
    plain_i, plain_c = predict.Predictor(net, SIZE, **kw)(frames[1:2])  # the smaller frame: the resize path
    assert torch.equal(ids[1], plain_i[0]) and torch.equal(rgb[1], plain_c[0])
    big = [frames[0].to(DEV), frames[2].to(DEV)]
    table = validation.slide_table((96, 192), SIZE, (32, 64), flip=True)
    assert len(table) == 8
    pal, lut = predict.default_palette(), torch.tensor(predict.CITYSCAPES_LABEL_IDS, dtype=torch.uint8)
    paint = dict(palette=pal.to(DEV), alpha=0.5, frame=torch.stack(big), lut=lut.to(DEV))
    (want_i, want_c), cls = _by_hand(net, big, table, 8, dt, **paint)  # max_batch 16, two frames: one chunk
    assert torch.equal(ids[0], want_i[0]) and torch.equal(ids[2], want_i[1])
    assert torch.equal(rgb[0], want_c[0]) and torch.equal(rgb[2], want_c[1])
    # ... and those against the oracle chain of the same heads
    assert np.array_equal(want_i.cpu().numpy(), R.ids_ref(cls, lut.numpy())) and len(np.unique(cls)) > 1
    assert np.array_equal(want_c.cpu().numpy(), R.paint_ref(cls, pal.numpy(), 128, torch.stack(big).cpu().numpy()))
    # four chunks of two windows (an fp32 canvas in between), one output alone
    net.train()
    ids2, none = predict.Predictor(net, SIZE, stride=(32, 64), flip=True, max_batch=4, **kw)(big, rgb=False)
    assert none is None and net.training
    (want_i, _), cls = _by_hand(net, big, table, 2, dt, lut=lut.to(DEV))
    assert torch.equal(torch.stack(list(ids2)), want_i) and np.array_equal(want_i.cpu().numpy(), R.ids_ref(cls, lut.numpy()))


def test_cli_with_stride(tmp_path, capsys):
    from PIL import Image
    cfg = yaml.safe_load(open(predict.__file__.replace("predict.py", "config.yaml")))
    cfg["data"]["cityscapes"]["image_size"] = "64, 128"
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    net = _net()
    torch.save(net.state_dict(), tmp_path / "weights.pth")
    src = tmp_path / "frames"
    src.mkdir()
    sizes = {"a": (96, 192), "b": (48, 160)}
    frames = dict(zip(sizes, _frames(sizes.values(), 9)))
    for stem, f in frames.items():
        Image.fromarray(f.numpy()).save(src / f"{stem}.png")
    base = ["--config", str(tmp_path / "cfg.yaml"), "--weights", str(tmp_path / "weights.pth"), "--input", str(src)]
    with rtsds_amd.precision(torch.float32):  # main() sets the configured compute dtype: put it back afterwards
        predict.main(base + ["--output", str(tmp_path / "out"), "--stride", "32,64", "--flip", "--max_batch", "4"])
        dt = rtsds_amd.runtime.compute_dtype()
        p = predict.Predictor(net.to(DEV), SIZE, stride=(32, 64), flip=True, max_batch=4, dtype=dt)
        for stem, f in frames.items():
            want_i, want_c = p([f])
            assert np.array_equal(np.array(Image.open(tmp_path / "out" / f"{stem}_ids.png")), want_i[0].cpu().numpy()), stem
            assert np.array_equal(np.array(Image.open(tmp_path / "out" / f"{stem}_color.png")), want_c[0].cpu().numpy()), stem
    assert "Predicted 2 frames" in capsys.readouterr().out
    assert sorted(q.name for q in (tmp_path / "out").iterdir()) == ["a_color.png", "a_ids.png", "b_color.png", "b_ids.png"]


def test_val_window_equals_fast_hist_of_predict_sliding(capsys):
    net = _net().to(DEV).eval()
    loader = [(synthetic_images(1, 96, 192, seed=20 + b), synthetic_labels(1, 96, 192, seed=30 + b)) for b in range(2)]
    with rtsds_amd.precision(torch.float32):
        miou = validation.val(0, net, loader, 19, device=DEV, window=SIZE, stride=(32, 64), flip=True)
        hist = np.zeros((19, 19), np.int64)
        for x, y in loader:
            _, pred = validation.predict_sliding(net, x.to(DEV), SIZE, stride=(32, 64), flip=True)
            hist += utils.fast_hist(y.numpy().ravel(), pred.cpu().numpy().ravel(), 19)
    assert miou == np.nanmean(utils.per_class_iou(hist)) and 0.0 < miou < 1.0
    assert "Validation Mean IoU" in capsys.readouterr().out
