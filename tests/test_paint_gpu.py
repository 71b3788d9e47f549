"""Prediction path on the device (rtsds_upsample_paint, functional.upsample_paint,
predict.Predictor, python -m rtsds_amd.predict).

Every comparison in this file is EXACT: the class map against the chain
functional.interpolate_geometry -> functional.argmax_channels (rtsds_bilinear_fwd ->
rtsds_argmax) it fuses, ids and colours against the numpy restatement tests/paint_ref.py of that
map.  Outputs are pre-filled with a sentinel and sit, at odd byte offsets, inside larger buffers
of guard bytes, so a byte the kernel did not write -- or wrote next to its range -- shows."""
import functools

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle.weights import recipe_state_dict  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import predict  # noqa: E402
from rtsds_amd import transforms as T  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from tests import paint_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)
CL = torch.channels_last
GUARD = 0xA5  # no id (< 34) and no class takes this value
GEOS = [
    ((2, 19, 16, 32), (128, 256)),   # x8, compile-time 19 classes
    ((1, 19, 13, 17), (97, 129)),    # odd sizes: 387-B rows, every byte phase of the 3-byte pixels
    ((2, 7, 9, 40), (64, 96)),       # run-time class count
    ((1, 19, 8, 40), (24, 300)),     # two column tiles, ragged last tile
    ((1, 2, 4, 4), (8, 8)),          # c = 2
    ((1, 32, 4, 4), (8, 8)),         # c = 32
    ((1, 19, 2, 4200), (4, 256)),    # 2 x 4202 x 19 x 4 B of rows > 64 KiB: the unstaged kernel
]
DTS = [torch.float32, torch.bfloat16]
ALPHAS = (0, 1, 128, 255, 256)
geos = pytest.mark.parametrize("gi", range(len(GEOS)),
                               ids=["x".join(map(str, g[0])) + "-" + "x".join(map(str, g[1])) for g in GEOS])
dts = pytest.mark.parametrize("dt", DTS, ids=["fp32", "bf16"])


def _logits(geo, dt):
    """Random x 3, as tests/test_mseval_gpu.py::_logits; NHWC memory on the device."""
    (n, c, h, w), _ = geo
    g = torch.Generator().manual_seed(n * 7 + h)
    x = torch.randn(n, c, h, w, generator=g, dtype=torch.float64) * 3
    return x.to(DEV, dt).contiguous(memory_format=CL)


def _chain(x, gm):
    """The unfused reference: resize, then argmax over classes; uint8 [n, ho, wo]."""
    return F.argmax_channels(F.interpolate_geometry(x, gm)).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _case(gi, dt):
    """(x, geometry, chain class map on the host, palette, lut, frame) of one geometry -- computed
    once, shared by the tests, never written to."""
    geo = GEOS[gi]
    (n, c, _, _), (ho, wo) = geo
    x = _logits(geo, dt)
    gm = F.upsample_geometry(x, size=geo[1])
    g = torch.Generator().manual_seed(100 + gi)
    pal = predict.default_palette() if c == 19 else torch.randint(0, 256, (c, 3), generator=g, dtype=torch.uint8)
    lut = torch.randperm(200, generator=g)[:c].to(torch.uint8)  # distinct ids, not the identity
    frame = torch.randint(0, 256, (n, ho, wo, 3), generator=g, dtype=torch.uint8)
    frame[:, : ho // 2, : wo // 3] = 0      # frames that hold 0 ...
    frame[:, ho // 2:, wo // 2:] = 255      # ... and 255
    want = _chain(x, gm)
    torch.cuda.synchronize()
    return x, gm, want.cpu().numpy(), pal, lut, frame


def _guarded(shape, off):
    """(buffer, view): a contiguous uint8 view of ``shape`` starting ``off`` bytes into a buffer
    filled with GUARD (sentinel inside the view, guard bytes either side)."""
    numel = int(np.prod(shape))
    buf = torch.full((numel + off + 61,), GUARD, dtype=torch.uint8, device=DEV)
    return buf, buf[off:off + numel].view(shape)


def _guards_intact(buf, view, off):
    b = buf.cpu()
    return bool((b[:off] == GUARD).all()) and bool((b[off + view.numel():] == GUARD).all())


def _placed(t, off):
    """``t`` copied to the device ``off`` bytes into its allocation (an odd byte phase)."""
    _, v = _guarded(tuple(t.shape), off)
    v.copy_(t)
    return v


# ----------------------------------------------------------------------------- chain identity
@dts
@geos
def test_ids_and_colours_equal_the_chain(gi, dt):
    x, gm, want, pal, lut, frame = _case(gi, dt)
    (n, c, _, _), (ho, wo) = GEOS[gi]
    assert len(np.unique(want)) > 1  # the map is not constant
    pal_d, frame_d = pal.to(DEV), _placed(frame, 7)
    for a in ALPHAS:
        ibuf, ids = _guarded((n, ho, wo), 13)
        cbuf, rgb = _guarded((n, ho, wo, 3), 5)
        out = F.upsample_paint(x, gm, palette=pal_d, alpha=a / 256.0, frame=frame_d, ids=ids, rgb=rgb)
        assert out[0] is ids and out[1] is rgb
        torch.cuda.synchronize()
        assert np.array_equal(ids.cpu().numpy(), want), a
        assert np.array_equal(rgb.cpu().numpy(), R.paint_ref(want, pal.numpy(), a, frame.numpy())), a
        assert _guards_intact(ibuf, ids, 13) and _guards_intact(cbuf, rgb, 5), a
    assert np.array_equal(frame_d.cpu().numpy(), frame.numpy())  # the frame is only read
    # with a lut the ids are lut[chain]; the colours still follow the class
    ibuf, ids = _guarded((n, ho, wo), 3)
    _, rgb = F.upsample_paint(x, gm, palette=pal_d, lut=lut.to(DEV), ids=ids)
    torch.cuda.synchronize()
    assert np.array_equal(ids.cpu().numpy(), R.ids_ref(want, lut.numpy()))
    assert np.array_equal(rgb.cpu().numpy(), pal.numpy()[want]) and _guards_intact(ibuf, ids, 3)


# ----------------------------------------------------------------------------- ties and NaNs
@dts
def test_ties_and_nans_follow_the_chain(dt):
    x0, gm, _, pal, _, _ = _case(1, dt)  # (1, 19, 13, 17) -> (97, 129)
    pal_d = pal.to(DEV)

    def both(x):
        ids, rgb = F.upsample_paint(x, gm, palette=pal_d)
        want = _chain(x, gm)
        torch.cuda.synchronize()
        assert torch.equal(ids, want) and np.array_equal(rgb.cpu().numpy(), pal.numpy()[want.cpu().numpy()])
        return ids
    flat = torch.full_like(x0, 1.25)
    assert (both(flat) == 0).all()  # all classes equal: the first
    tie = x0.clone()
    tie[:, 3] = 40.0
    tie[:, 7] = 40.0  # two classes share the maximum everywhere: the first of them
    assert (both(tie) == 3).all()
    nan = x0.clone()
    nan[0, 5, 2, 3] = float("nan")  # one class of one head pixel
    nan[0, 9, 7, 11] = float("nan")  # two classes of another: the first NaN wins
    nan[0, 4, 7, 11] = float("nan")
    ids = both(nan)
    # output (18, 26) taps head rows 1, 2 and columns 2, 3; output (55, 87) rows 6, 7 and columns 11, 12
    assert int(ids[0, 18, 26]) == 5 and int(ids[0, 55, 87]) == 4
    assert 0 < int((ids != both(x0)).sum()) < ids.numel() // 8  # only the pixels that tap them changed


# ----------------------------------------------------------------------------- optional outputs
def test_optional_outputs_and_refusals():
    x, gm, want, pal, lut, frame = _case(0, torch.bfloat16)
    (n, c, _, _), (ho, wo) = GEOS[0]
    pal_d, frame_d, lut_d = pal.to(DEV), frame.to(DEV), lut.to(DEV)
    ids, rgb = F.upsample_paint(x, gm)  # ids alone
    assert rgb is None and ids.dtype == torch.uint8 and np.array_equal(ids.cpu().numpy(), want)
    ids, rgb = F.upsample_paint(x, gm, palette=pal_d, want_ids=False)  # rgb alone, alpha 1.0 without a frame
    assert ids is None and np.array_equal(rgb.cpu().numpy(), pal.numpy()[want])
    ids, rgb = F.upsample_paint(x, gm, palette=pal_d, alpha=0.5, frame=frame_d, want_ids=False)
    assert ids is None and np.array_equal(rgb.cpu().numpy(), R.paint_ref(want, pal.numpy(), 128, frame.numpy()))
    good_i = torch.zeros((n, ho, wo), dtype=torch.uint8, device=DEV)
    good_c = torch.zeros((n, ho, wo, 3), dtype=torch.uint8, device=DEV)
    bad = [{"ids": good_i.to(torch.int8)}, {"ids": good_i[:, :, :-1]}, {"ids": good_i.cpu()},
           {"ids": torch.zeros((n, wo, ho), dtype=torch.uint8, device=DEV).transpose(1, 2)},  # not contiguous
           {"rgb": good_c.to(torch.int32)}, {"rgb": good_c[:1]}, {"rgb": good_c.cpu()},
           {"rgb": torch.zeros((n, ho, wo, 4), dtype=torch.uint8, device=DEV)[..., :3]},       # not contiguous
           {"frame": frame_d.float(), "alpha": 0.5}, {"frame": frame_d[:, :-1], "alpha": 0.5},
           {"frame": frame, "alpha": 0.5}, {"alpha": 0.5},  # the last: a blend without the frame
           {"palette": pal_d[:5]}, {"palette": pal_d.long()}, {"palette": pal}, {"palette": pal_d.t().contiguous().t()},
           {"lut": lut_d.long()}, {"lut": lut_d[:7]}, {"lut": lut}, {"alpha": 1.5}, {"alpha": -0.1},
           {"palette": None}]  # the last: rgb without a palette
    for kw in bad:
        with pytest.raises(RuntimeError, match="^rtsds_amd: upsample_paint"):
            F.upsample_paint(x, gm, **dict({"palette": pal_d, "ids": good_i, "rgb": good_c}, **kw))
    with pytest.raises(RuntimeError, match="^rtsds_amd: upsample_paint"):
        F.upsample_paint(x, gm, want_ids=False)  # nothing to produce
    with pytest.raises(RuntimeError, match="^rtsds_amd: upsample_paint"):
        F.upsample_paint(x.double(), gm)
    with pytest.raises(RuntimeError, match="^rtsds_amd: upsample_paint"):
        F.upsample_paint(x[:, :1], gm)  # c = 1
    torch.cuda.synchronize()
    assert int(good_i.max()) == 0 and int(good_c.max()) == 0  # nothing was launched on the valid buffers


# ----------------------------------------------------------------------------- batch independence
@dts
def test_batch_items_are_independent_and_layout_free(dt):
    x, gm, want, pal, _, frame = _case(0, dt)  # n = 2
    pal_d, frame_d = pal.to(DEV), frame.to(DEV)
    ids, rgb = F.upsample_paint(x, gm, palette=pal_d, alpha=0.25, frame=frame_d)
    for i in range(2):
        ids1, rgb1 = F.upsample_paint(x[i:i + 1], gm, palette=pal_d, alpha=0.25, frame=frame_d[i:i + 1])
        assert torch.equal(ids1[0], ids[i]) and torch.equal(rgb1[0], rgb[i])
    nchw = x.contiguous()  # NCHW memory: converted on the way in
    assert not nchw.is_contiguous(memory_format=CL)
    ids2, rgb2 = F.upsample_paint(nchw, gm, palette=pal_d, alpha=0.25, frame=frame_d)
    assert torch.equal(ids2, ids) and torch.equal(rgb2, rgb)
    assert np.array_equal(ids.cpu().numpy(), want)


# ----------------------------------------------------------------------------- round trip
@dts
def test_default_palette_round_trips_through_gta5_decode(dt):
    x, gm, want, pal, _, _ = _case(0, dt)
    ids, rgb = F.upsample_paint(x, gm, palette=predict.default_palette().to(DEV), alpha=1.0)
    for i in range(x.shape[0]):
        assert torch.equal(T.decode_gta5_labels(rgb[i]), ids[i].long())


# ----------------------------------------------------------------------------- Predictor
SIZE = (64, 128)  # the smallest BiSeNet-R18 input of the model tests
FRAME_SIZES = ((64, 128), (96, 160), (96, 160))


def _net(seed=1):
    net = BiSeNet(19, "resnet18")
    sd = net.state_dict()
    net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, seed))
    return net


def _frames(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8) for h, w in sizes]


@dts
def test_predictor_equals_the_op_chain(dt):
    net = _net().to(DEV).train()
    frames = _frames(FRAME_SIZES, 5)  # CPU tensors: moved by the Predictor
    p = predict.Predictor(net, SIZE, label_ids=predict.CITYSCAPES_LABEL_IDS, alpha=0.5, dtype=dt)
    ids, rgb = p(frames)
    assert net.training  # restored
    assert len(ids) == len(rgb) == 3
    # the same batch through the same ops, one by one
    net.eval()
    with torch.no_grad(), rtsds_amd.precision(dt):
        batch = T.ImagePipeline(SIZE)([f.to(DEV) for f in frames])
        (low, _), = net.forward_lowres(batch, main_only=True)
    assert tuple(low.shape) == (3, 19, 8, 16)
    pal = predict.default_palette().numpy()
    maps = []
    for n, f in enumerate(frames):
        one = low[n:n + 1]
        want = _chain(one, F.upsample_geometry(one, size=f.shape[:2]))[0].cpu().numpy()
        maps.append(want)
        assert ids[n].dtype == torch.uint8 and tuple(ids[n].shape) == tuple(f.shape[:2])
        assert np.array_equal(ids[n].cpu().numpy(), R.ids_ref(want, predict.CITYSCAPES_LABEL_IDS)), n
        assert np.array_equal(rgb[n].cpu().numpy(), R.paint_ref(want, pal, 128, f.numpy())), n
    assert len(np.unique(np.concatenate([m.ravel() for m in maps]))) > 1
    # frames of one size: one launch for the batch, the same results; one output alone
    net.train()
    ids2, none = p(frames[1:], rgb=False)
    assert none is None and net.training
    assert torch.equal(ids2[0], ids[1]) and torch.equal(ids2[1], ids[2])
    none, rgb2 = p(frames[1:], ids=False)
    assert none is None and torch.equal(rgb2[0], rgb[1]) and torch.equal(rgb2[1], rgb[2])


def test_predictor_refusals():
    net = _net().to(DEV)
    with pytest.raises(RuntimeError, match="at most 32 classes"):
        predict.Predictor(net, SIZE, palette=torch.zeros((33, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="label_ids"):
        predict.Predictor(net, SIZE, label_ids=(1, 2, 3))
    with pytest.raises(RuntimeError, match="Predictor: alpha"):
        predict.Predictor(net, SIZE, alpha=2.0)
    p = predict.Predictor(net, SIZE, palette=torch.zeros((7, 3), dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="19 classes, the palette 7"):
        p(_frames(FRAME_SIZES[:1], 1))
    with pytest.raises(RuntimeError, match="uint8 HWC"):
        predict.Predictor(net, SIZE)([torch.zeros((64, 128, 3))])


# ----------------------------------------------------------------------------- CLI
def test_cli_writes_masks_and_ids(tmp_path, capsys):
    from PIL import Image
    cfg = yaml.safe_load(open(predict.__file__.replace("predict.py", "config.yaml")))
    cfg["data"]["cityscapes"]["image_size"] = "64, 128"
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    torch.save(_net().state_dict(), tmp_path / "weights.pth")
    src = tmp_path / "frames"
    src.mkdir()
    sizes = {"a": (64, 128), "b": (96, 160)}
    for (stem, _), f in zip(sizes.items(), _frames(sizes.values(), 9)):
        Image.fromarray(f.numpy()).save(src / f"{stem}.png")
    (src / "notes.txt").write_text("not an image")
    base = ["--config", str(tmp_path / "cfg.yaml"), "--weights", str(tmp_path / "weights.pth"), "--input", str(src)]
    palette = {tuple(c) for c in predict.default_palette().tolist()}
    with rtsds_amd.precision(torch.float32):  # main() sets the configured compute dtype: put it back afterwards
        predict.main(base + ["--output", str(tmp_path / "out"), "--batch_size", "2"])
        predict.main(base + ["--output", str(tmp_path / "out_ids"), "--label_ids", "--overlay", "1.0"])
    assert "Predicted 2 frames" in capsys.readouterr().out
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["a_color.png", "a_ids.png", "b_color.png", "b_ids.png"]
    for stem, (h, w) in sizes.items():
        col = np.array(Image.open(tmp_path / "out" / f"{stem}_color.png"))
        ids = np.array(Image.open(tmp_path / "out" / f"{stem}_ids.png"))
        lab = np.array(Image.open(tmp_path / "out_ids" / f"{stem}_ids.png"))
        assert col.shape == (h, w, 3) and ids.shape == (h, w) and lab.shape == (h, w) and ids.dtype == np.uint8
        assert {tuple(c) for c in col.reshape(-1, 3).tolist()} <= palette  # --overlay 1.0: the mask alone
        assert int(ids.max()) < 19 and np.array_equal(col, predict.default_palette().numpy()[ids])
        assert set(np.unique(lab).tolist()) <= set(predict.CITYSCAPES_LABEL_IDS)
        assert np.array_equal(lab, np.array(predict.CITYSCAPES_LABEL_IDS, np.uint8)[ids])  # one model, both runs
