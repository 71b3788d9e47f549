"""ClassMix on the device (rtsds_class_presence, rtsds_classmix, functional.class_presence /
classmix, selftrain.ClassMixLoader, main --self_training with mix: classmix).

Every comparison in this file is EXACT, against the numpy restatement tests/classmix_ref.py:
labels, masks and bit masks with np.array_equal, images as raw bytes (the pad lane of the
4-element pixel pitch included).  Outputs are pre-filled with sentinels (image bytes 0xA5, labels
-1, mask 0xFF), so an element the kernel did not write shows.  In every randomly labelled case the
REFERENCE mask must take between 10 % and 90 % of each sample's window (labels uniform over c
classes plus ignore give 33 - 50 %), so neither arm of the mix is vacuous."""
import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("no HIP device", allow_module_level=True)

import rtsds_amd  # noqa: E402
from oracle.weights import recipe_state_dict, synthetic_images  # noqa: E402
from rtsds_amd import functional as F  # noqa: E402
from rtsds_amd import losses, optim, selftrain, train  # noqa: E402
from rtsds_amd import main as rmain  # noqa: E402
from rtsds_amd.callbacks import Callback  # noqa: E402
from rtsds_amd.models.bisenet.build_bisenet import BiSeNet  # noqa: E402
from tests import classmix_ref as R  # noqa: E402

DEV = torch.device("cuda", 0)
BINS = 1024
PIX = {6: (torch.bfloat16, 3), 8: (torch.bfloat16, 4), 12: (torch.float32, 3), 16: (torch.float32, 4)}


# ----------------------------------------------------------------------------- image forms
def image_from_bytes(raw, pix):
    """uint8 numpy [N, H, W, pix] -> the [N, 3, H, W] device tensor of that pixel record: NHWC for a
    pitch of 3 elements, the ``_rt_cpad`` = 4 view for a pitch of 4."""
    dtype, pitch = PIX[pix]
    buf = torch.from_numpy(np.ascontiguousarray(raw)).to(DEV).view(dtype)  # [N, H, W, pitch]
    assert buf.shape[-1] == pitch
    x = buf.permute(0, 3, 1, 2)
    if pitch == 4:
        x = x[:, :3]
        x._rt_cpad = 4
    return x


def image_bytes(x):
    """The raw bytes of an input-form image batch, uint8 numpy [N, H, W, pix] (pad lane included)."""
    n, _, h, w = x.shape
    pitch = 4 if getattr(x, "_rt_cpad", None) == 4 else 3
    if pitch == 3:
        assert x.is_contiguous(memory_format=torch.channels_last)
    else:
        assert F.is_padded_input(x)
    rec = torch.as_strided(x, (n, h, w, pitch), (h * w * pitch, w * pitch, pitch, 1))
    return rec.contiguous().view(torch.uint8).cpu().numpy().reshape(n, h, w, pitch * x.element_size())


def _u32(t):
    return t.cpu().view(torch.int32).numpy().view(np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ----------------------------------------------------------------------------- cases
def random_labels(rng, n, hs, ws, c, ignore, extra=()):
    """Uniform over the c classes plus ``ignore``; ``extra`` values (no classes) sprinkled over 5 %."""
    lab = rng.integers(0, c + 1, (n, hs, ws)).astype(np.int64)
    lab[lab == c] = ignore
    if extra:
        hit = rng.random((n, hs, ws)) < 0.05
        lab[hit] = rng.choice(np.array(extra, dtype=np.int64), size=int(hit.sum()))
    return lab


def blocky_labels(rng, n, hs, ws, c, ignore):
    """Coherent regions of 8 x 8 to 32 x 32 pixels: whole waves see one label."""
    lab = np.empty((n, hs, ws), np.int64)
    for i in range(n):
        y = 0
        while y < hs:
            bh = int(rng.integers(8, 33))
            x = 0
            while x < ws:
                bw = int(rng.integers(8, 33))
                v = int(rng.integers(0, c + 1))
                lab[i, y:y + bh, x:x + bw] = ignore if v == c else v
                x += bw
            y += bh
    return lab


class Case:
    def __init__(self, n, size, ssize, c, ignore, pix, origins, seed, slab=None, perm=None, extra=()):
        rng = np.random.default_rng(seed)
        (h, w), (hs, ws) = size, ssize
        self.n, self.size, self.c, self.ignore, self.pix = n, size, c, ignore, pix
        self.slab = random_labels(rng, n, hs, ws, c, ignore, extra) if slab is None else slab
        self.src = rng.integers(0, 256, (n, hs, ws, pix), dtype=np.uint8)
        self.tgt = rng.integers(0, 256, (n, h, w, pix), dtype=np.uint8)
        self.pred = rng.integers(0, c + 3, (n, h, w)).astype(np.uint8)   # values >= c: no class
        self.cbin = rng.integers(0, BINS, (n, h, w)).astype(np.uint16)
        self.tbin = rng.integers(0, BINS, c).astype(np.int32)
        self.perm = np.stack([rng.permutation(c) for _ in range(n)]).astype(np.int32) if perm is None else perm
        self.origins = np.array(origins, dtype=np.int32).reshape(n, 2)
        self.ref = R.classmix(self.src, self.slab, self.tgt, self.pred, self.cbin, self.tbin, self.perm, self.origins,
                              ignore)

    def mask_share(self):
        return self.ref["mask"].reshape(self.n, -1).mean(axis=1)

    def assert_not_vacuous(self):
        share = self.mask_share()
        assert ((share >= 0.1) & (share <= 0.9)).all(), share

    def device(self, block=True):
        """The device arguments; perm / origins as column slices of one [N, 2 + c] block (the
        loader's form) or as two contiguous tensors."""
        d = {"src": image_from_bytes(self.src, self.pix), "slab": _dev(self.slab),
             "tgt": image_from_bytes(self.tgt, self.pix), "pred": _dev(self.pred), "cbin": _dev(self.cbin),
             "tbin": _dev(self.tbin)}
        if block:
            blk = _dev(np.concatenate([self.origins, self.perm], axis=1))
            d["origins"], d["perm"] = blk[:, :2], blk[:, 2:]
        else:
            d["origins"], d["perm"] = _dev(self.origins), _dev(self.perm)
        return d

    def sentinels(self):
        h, w = self.size
        out = image_from_bytes(np.full((self.n, h, w, self.pix), 0xA5, np.uint8), self.pix)
        return {"out": out, "out_labels": torch.full((self.n, h, w), -1, dtype=torch.int64, device=DEV),
                "mask": torch.full((self.n, h, w), 0xFF, dtype=torch.uint8, device=DEV),
                "chosen": torch.full((self.n,), 0x5A5A5A5A, dtype=torch.int32, device=DEV).view(F._U32)}

    def check(self, out, out_labels, mask=None, chosen=None, present=None):
        torch.cuda.synchronize()
        assert out_labels.dtype == torch.int64
        assert np.array_equal(out_labels.cpu().numpy(), self.ref["out_lab"])
        assert np.array_equal(image_bytes(out), self.ref["out_img"])
        if mask is not None:
            assert np.array_equal(mask.cpu().numpy(), self.ref["mask"])
        if chosen is not None:
            assert np.array_equal(_u32(chosen), self.ref["chosen"])
        if present is not None:
            assert np.array_equal(_u32(present), self.ref["present"])

    def run(self, block=True):
        """class_presence + classmix into sentinel-filled outputs, everything checked."""
        d, s = self.device(block), self.sentinels()
        present = F.class_presence(d["slab"], self.size, d["origins"], self.c)
        got = F.classmix(d["src"], d["slab"], d["tgt"], d["pred"], d["cbin"], d["tbin"], d["perm"], d["origins"],
                         self.ignore, present=present, **s)
        assert got[0] is s["out"] and got[1] is s["out_labels"]
        self.check(s["out"], s["out_labels"], s["mask"], s["chosen"], present)
        return d, s, present


# ----------------------------------------------------------------------------- kernels
def test_less_than_one_workgroup():
    case = Case(1, (13, 17), (13, 17), 19, 19, 8, [(0, 0)], seed=1)
    case.assert_not_vacuous()
    case.run()
    case.run(block=False)


@pytest.mark.parametrize("pix", [6, 8, 12, 16])
def test_unaligned_window(pix):
    """Odd source width, x0 = 9 and 33: no source row starts on a vector boundary twice in a row;
    the target rows (300 pixels) alternate between the vector and the per-pixel form."""
    case = Case(2, (24, 300), (37, 333), 19, 19, pix, [(5, 9), (13, 33)], seed=10 + pix)
    case.assert_not_vacuous()
    case.run()


def test_unaligned_window_packed_input_form():
    """The images as pack_input leaves them in bf16: the 4-channel pitch with a zero pad lane."""
    case = Case(2, (24, 300), (37, 333), 19, 19, 8, [(5, 9), (13, 33)], seed=3)
    g = torch.Generator().manual_seed(4)
    src = F.pack_input(torch.randn(2, 3, 37, 333, generator=g).to(DEV), torch.bfloat16)
    tgt = F.pack_input(torch.randn(2, 3, 24, 300, generator=g).to(DEV), torch.bfloat16)
    assert src._rt_cpad == 4 and tgt._rt_cpad == 4
    case.src, case.tgt = image_bytes(src), image_bytes(tgt)
    case.ref = R.classmix(case.src, case.slab, case.tgt, case.pred, case.cbin, case.tbin, case.perm, case.origins, 19)
    case.assert_not_vacuous()
    d = case.device()
    out, lab = F.classmix(src, d["slab"], tgt, d["pred"], d["cbin"], d["tbin"], d["perm"], d["origins"], 19)
    assert out._rt_cpad == 4 and F.is_padded_input(out) and tuple(out.shape) == (2, 3, 24, 300)
    assert F.pack_input(out, torch.bfloat16) is out  # the model's pack_input passes it through
    case.check(out, lab)
    assert not image_bytes(out)[..., 6:].any()        # both pad lanes were zero: so is the mixture's


@pytest.mark.parametrize("pix", [6, 8, 12, 16])
@pytest.mark.parametrize("origins", [[(0, 0), (6, 8)], [(3, 32), (13, 33)]], ids=["x0-0-8", "x0-32-corner"])
def test_aligned_rows_and_the_sources_last_rows_and_columns(pix, origins):
    """x0 in {0, 8, 32} and the corner window (Hs - H, Ws - W) = (13, 33), whose last row and
    column are the source map's last."""
    case = Case(2, (24, 300), (37, 333), 19, 19, pix, origins, seed=20 + pix)
    case.assert_not_vacuous()
    case.run()


@pytest.mark.parametrize("pix", [6, 8, 12, 16])
def test_every_row_on_the_vector_form(pix):
    """Widths that are multiples of 8 with x0 a multiple of 8: every row takes 16-byte accesses;
    x0 = 3 with 8- / 16-byte records: the 8-byte-aligned source loads."""
    case = Case(2, (16, 64), (24, 96), 19, 19, pix, [(2, 8), (8, 3)], seed=30 + pix)
    case.assert_not_vacuous()
    case.run()


@pytest.mark.parametrize("c,ignore", [(2, 2), (32, 255)])
def test_class_floor_and_cap(c, ignore):
    case = Case(2, (24, 300), (37, 333), c, ignore, 8, [(5, 9), (13, 32)], seed=40 + c, extra=(-100, 255, c, c + 5))
    win = case.slab[0, 5:29, 9:309]
    assert all((win == v).any() for v in (-100, 255, c, c + 5))
    assert (case.pred >= c).any() and (case.ref["out_lab"] == ignore).any()
    case.assert_not_vacuous()
    # the pixels whose label is no class came out as target pixels; they set no presence bit
    no_class = (win < 0) | (win >= c)
    assert not case.ref["mask"][0][no_class].any() and int(case.ref["present"].max()) < (1 << c)
    if c == 32:
        assert (case.ref["present"] >> 31).all()  # class 31: the sign bit of the mask
    case.run()


def test_blocky_labels():
    rng = np.random.default_rng(50)
    case = Case(2, (96, 200), (128, 256), 19, 19, 8, [(11, 24), (32, 19)], seed=51,
                slab=blocky_labels(rng, 2, 128, 256, 19, 19))
    case.assert_not_vacuous()
    case.run()


def test_single_class_and_all_ignore_samples():
    slab = np.empty((2, 37, 333), np.int64)
    slab[0] = 7       # one class: m = 1, it is chosen, the whole window is pasted
    slab[1] = 19      # nothing but ignore: nothing is chosen
    case = Case(2, (24, 300), (37, 333), 19, 19, 8, [(5, 9), (13, 32)], seed=60, slab=slab)
    assert case.ref["present"].tolist() == [1 << 7, 0] and case.ref["chosen"].tolist() == [1 << 7, 0]
    assert case.mask_share().tolist() == [1.0, 0.0]
    d, s, _ = case.run()
    # the all-ignore sample is the target plus pseudo_select
    want = F.pseudo_select(d["pred"][1:], d["cbin"][1:], d["tbin"], 19)
    assert torch.equal(s["out_labels"][1:], want)
    assert np.array_equal(image_bytes(s["out"])[1], case.tgt[1]) and np.array_equal(image_bytes(s["out"])[0],
                                                                                  case.src[0, 5:29, 9:309])


def test_perm_is_per_sample_and_ties_break_to_the_lower_class():
    rng = np.random.default_rng(70)
    one = random_labels(rng, 1, 37, 333, 19, 19)
    slab = np.concatenate([one, one, one])
    perm = np.stack([np.arange(19), np.arange(19)[::-1], np.full(19, 4)]).astype(np.int32)
    case = Case(3, (24, 300), (37, 333), 19, 19, 8, [(5, 9)] * 3, seed=71, slab=slab, perm=perm)
    p, ch = case.ref["present"], case.ref["chosen"]
    assert p[0] == p[1] == p[2] == (1 << 19) - 1
    assert ch[0] == (1 << 10) - 1 and ch[1] == ((1 << 19) - 1) ^ ((1 << 9) - 1) and ch[2] == ch[0] != ch[1]
    case.assert_not_vacuous()
    case.run()


def test_one_large_case():
    case = Case(2, (512, 1024), (720, 1280), 19, 19, 8, [(101, 77), (208, 256)], seed=80)
    case.assert_not_vacuous()
    case.run()


def test_more_rows_than_one_pass_of_the_launch_grid():
    """4200 window rows per sample: more one-row items than the waves of the launch grid hold, so
    both kernels go round their grid-stride loops."""
    case = Case(2, (4200, 24), (4210, 40), 19, 19, 8, [(7, 8), (10, 13)], seed=81)
    case.assert_not_vacuous()
    case.run()


def test_optional_outputs_and_present_none():
    case = Case(2, (24, 300), (37, 333), 19, 19, 8, [(5, 9), (13, 32)], seed=90)
    d = case.device()
    args = (d["src"], d["slab"], d["tgt"], d["pred"], d["cbin"], d["tbin"], d["perm"], d["origins"], 19)
    out, lab = F.classmix(*args)  # present computed inside, fresh outputs, no mask, no chosen
    assert lab.dtype == torch.int64 and tuple(lab.shape) == (2, 24, 300) and out.dtype == torch.bfloat16
    case.check(out, lab)
    for keep in ("mask", "chosen"):
        s = case.sentinels()
        kw = {"out": s["out"], "out_labels": s["out_labels"], keep: s[keep]}
        F.classmix(*args, **kw)
        case.check(s["out"], s["out_labels"], **{keep: s[keep]})
    # present need not be cleared by the caller: the same result over a scribbled tensor's storage
    present = F.class_presence(d["slab"], (24, 300), d["origins"], 19)
    assert present.dtype == F._U32 and np.array_equal(_u32(present), case.ref["present"])
    # without a class count every value in [0, 32) is a class
    p32 = _u32(F.class_presence(d["slab"], (24, 300), d["origins"]))
    assert np.array_equal(p32, R.presence(case.slab, (24, 300), case.origins, 32))
    # [N, 1, Hs, Ws] labels
    out, lab = F.classmix(d["src"], d["slab"].unsqueeze(1), *args[2:])
    case.check(out, lab)


def test_equals_the_unfused_chain():
    """pseudo_select + two torch.where over the reference mask give the same mixture."""
    case = Case(2, (24, 300), (37, 333), 19, 19, 8, [(5, 9), (13, 32)], seed=100)
    case.assert_not_vacuous()
    d, s, _ = case.run()
    m = _dev(case.ref["mask"].astype(bool))
    win = torch.stack([d["slab"][i, y:y + 24, x:x + 300] for i, (y, x) in enumerate(case.origins.tolist())])
    want_lab = torch.where(m, win, F.pseudo_select(d["pred"], d["cbin"], d["tbin"], 19))
    assert torch.equal(s["out_labels"], want_lab)
    rec = lambda x, h, w: torch.as_strided(x, (2, h, w, 4), (h * w * 4, w * 4, 4, 1)).view(torch.int16)  # noqa: E731
    swin = torch.stack([rec(d["src"], 37, 333)[i, y:y + 24, x:x + 300] for i, (y, x) in enumerate(case.origins.tolist())])
    want_img = torch.where(m[..., None], swin, rec(d["tgt"], 24, 300))
    assert torch.equal(rec(s["out"], 24, 300), want_img)


def test_wrappers_reject_bad_arguments():
    case = Case(2, (8, 16), (10, 20), 19, 19, 8, [(1, 2), (2, 4)], seed=110)
    d = case.device(block=False)
    order = ("src", "slab", "tgt", "pred", "cbin", "tbin", "perm", "origins")

    def call(**kw):
        a = dict(d, **kw)
        extra = {k: a.pop(k) for k in list(a) if k not in order}
        return F.classmix(*[a[k] for k in order], 19, **extra)

    other = Case(2, (8, 16), (10, 20), 19, 19, 6, [(1, 2), (2, 4)], seed=111).device()
    bad = [{"src": other["src"]},                                        # another image form
           {"tgt": image_from_bytes(case.tgt.repeat(2, axis=3), 16)},    # another dtype
           {"src": d["tgt"], "slab": d["slab"][:, :8, :16].contiguous(), "tgt": d["src"],
            "pred": torch.zeros(2, 10, 20, dtype=torch.uint8, device=DEV),
            "cbin": torch.zeros(2, 10, 20, dtype=torch.int16, device=DEV).view(torch.uint16)},  # window > source
           {"slab": d["slab"].int()}, {"slab": d["slab"][:1]}, {"pred": d["pred"].long()},
           {"tbin": d["tbin"].long()}, {"tbin": d["tbin"][:1]}, {"tbin": d["tbin"].cpu()},
           {"perm": d["perm"].long()}, {"perm": d["perm"][:, :18]}, {"perm": d["perm"].t().contiguous().t()},
           {"origins": d["origins"][:1]}, {"origins": d["origins"].cpu()},
           {"present": torch.zeros(2, dtype=torch.int64, device=DEV)},
           {"out": other["tgt"]}, {"out_labels": torch.zeros(2, 8, 16, dtype=torch.int32, device=DEV)},
           {"mask": torch.zeros(2, 8, 16, dtype=torch.bool, device=DEV)},
           {"chosen": torch.zeros(3, dtype=torch.int32, device=DEV)},
           {"src": torch.zeros(2, 3, 10, 20, dtype=torch.bfloat16, device=DEV)}]  # NCHW: no input form
    for kw in bad:
        with pytest.raises(RuntimeError, match="rtsds_amd: classmix"):
            call(**kw)
    with pytest.raises(RuntimeError, match="window"):
        F.class_presence(d["slab"], (11, 20), d["origins"])
    with pytest.raises(RuntimeError, match="num_classes"):
        F.class_presence(d["slab"], (8, 16), d["origins"], 33)
    out, lab = call()  # and the arguments as they are pass
    case.check(out, lab)


# ----------------------------------------------------------------------------- graph replay
def test_graph_capture_replay_equals_eager():
    case = Case(2, (24, 300), (37, 333), 19, 19, 8, [(5, 9), (13, 32)], seed=120)
    d, eager, present_e = case.run()  # eager (and the first, warming call)
    s = case.sentinels()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # a straight line: memset, two kernels on one stream
        p = F.class_presence(d["slab"], case.size, d["origins"], 19)
        F.classmix(d["src"], d["slab"], d["tgt"], d["pred"], d["cbin"], d["tbin"], d["perm"], d["origins"], 19,
                   present=p, **s)
    for _ in range(2):
        fresh = case.sentinels()
        for k in s:
            if k == "out":
                rec = lambda x: torch.as_strided(x, (2, 24, 300, 4), (24 * 300 * 4, 300 * 4, 4, 1))  # noqa: E731
                rec(s[k]).copy_(rec(fresh[k]))
            else:
                s[k].copy_(fresh[k])
        p.view(torch.int32).fill_(-1)  # a stale presence mask must not survive into the replay
        graph.replay()
    torch.cuda.synchronize()
    case.check(s["out"], s["out_labels"], s["mask"], s["chosen"], p)
    assert torch.equal(s["out_labels"], eager["out_labels"]) and torch.equal(s["mask"], eager["mask"])
    assert np.array_equal(image_bytes(s["out"]), image_bytes(eager["out"]))
    assert np.array_equal(_u32(p), _u32(present_e))


# ----------------------------------------------------------------------------- loader level
SIZE, SSIZE, NB = (64, 128), (80, 160), 2
IGNORE = 19


@pytest.fixture(scope="module")
def bisenet():
    net = BiSeNet(19, "resnet18")
    sd = net.state_dict()
    net.load_state_dict(recipe_state_dict({k: tuple(v.shape) for k, v in sd.items()}, 1))
    net = net.to(DEV).eval()
    batches = [(synthetic_images(2, *SIZE, seed=60 + i), torch.zeros(2, 1, *SIZE, dtype=torch.int64)) for i in range(NB)]
    g = torch.Generator().manual_seed(9)
    source = [(synthetic_images(3, *SSIZE, seed=70 + i), torch.randint(0, 20, (3, 1, *SSIZE), generator=g))
              for i in range(3)]  # 3 samples per batch (the first 2 are used), 3 batches for 2 x 2 draws
    return net, batches, source


def test_classmix_loader_batches_equal_reference_and_train_one_epoch(bisenet):
    net, batches, source = bisenet
    with rtsds_amd.precision(torch.float32):
        labels = selftrain.generate(net, batches, 19, device=DEV)
        tbin = selftrain.class_thresholds(labels.hist, 0.5)
        loader = selftrain.ClassMixLoader(batches, source, labels, tbin, IGNORE)
        assert len(loader) == NB
        torch.manual_seed(123)
        got = []
        for _ in range(2):  # two passes: the 3-batch source loader is restarted on the fourth draw
            for x, y in loader:
                got.append((x, y, loader.last_chosen))
        torch.manual_seed(123)
        for i, (x, y, chosen) in enumerate(got):
            origins, perm = np.empty((2, 2), np.int32), np.empty((2, 19), np.int32)
            for s in range(2):  # the documented draw order: per sample y0, x0, perm
                origins[s, 0] = int(torch.randint(0, SSIZE[0] - SIZE[0] + 1, (1,)))
                origins[s, 1] = int(torch.randint(0, SSIZE[1] - SIZE[1] + 1, (1,)))
                perm[s] = torch.randperm(19).numpy()
            simg, slab = source[i % 3]
            src = image_bytes(F.pack_input(simg[:2].to(DEV), torch.float32))
            tgt = image_bytes(F.pack_input(batches[i % NB][0].to(DEV), torch.float32))
            pred, cbin = labels.pred[i % NB].cpu().numpy(), labels.cbin[i % NB].cpu().numpy()
            ref = R.classmix(src, slab[:2, 0].numpy(), tgt, pred, cbin, tbin.numpy(), perm, origins, IGNORE)
            share = ref["mask"].reshape(2, -1).mean(axis=1)
            assert ((share >= 0.1) & (share <= 0.9)).all(), share
            assert x.dtype == torch.float32 and tuple(x.shape) == (2, 3, *SIZE) and x.is_cuda
            assert y.dtype == torch.int64 and tuple(y.shape) == (2, 1, *SIZE) and y.is_cuda
            assert np.array_equal(image_bytes(x), ref["out_img"])
            assert np.array_equal(y[:, 0].cpu().numpy(), ref["out_lab"])
            assert np.array_equal(_u32(chosen), ref["chosen"])

        losses_seen = []

        class Log(Callback):
            def on_batch_end(self, batch, logs=None):
                losses_seen.append(logs["train_loss"])
        before = [p.detach().clone() for p in net.parameters()]
        opt = optim.Adam(net.parameters(), lr=1e-4)
        train.train(epoch=0, model=net, train_loader=loader, criterion=losses.CrossEntropyLoss(ignore_index=IGNORE),
                    optimizer=opt, init_lr=1e-4, max_iter=NB, device=DEV, callbacks=[Log()])
    torch.cuda.synchronize()
    net.eval()
    assert len(losses_seen) == NB and all(np.isfinite(v) and v > 0 for v in losses_seen)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    assert all(torch.isfinite(p).all() for p in net.parameters())


# ----------------------------------------------------------------------------- CLI
def _cfg(tmp_path, precision):
    cfg = yaml.safe_load(open(rmain.__file__.replace("main.py", "config.yaml")))
    cfg["precision"] = precision
    cfg["data"]["cityscapes"].update(image_size="64, 128", batch_size=2)
    cfg["data"]["gta5_modified"].update(image_size="80, 160", batch_size=2)
    cfg["data"]["synthetic_batches"] = 2
    cfg["training"]["domain_adaptation"].update(iterations=2, epochs=1)
    cfg["training"]["segmentation"].update(epochs=1)
    cfg["model"]["adversarial_model"]["generator"]["name"] = "bisenet"
    cfg["training"]["self_training"] = {"rounds": 1, "epochs": 1, "portion": 0.2, "portion_step": 0.05, "cap": 0.9,
                                        "bins": 1024, "lr_scale": 0.1, "scales": [1.0], "flip": False, "mix": "classmix"}
    p = tmp_path / "cfg.yaml"
    p.write_text(yaml.safe_dump(cfg))
    return str(p)


def _count_self_training(monkeypatch):
    calls = []
    real_gen, real_train = selftrain.generate, rmain.train
    monkeypatch.setattr(selftrain, "generate", lambda *a, **k: (calls.append("generate"), real_gen(*a, **k))[1])

    def counted(**kw):
        if isinstance(kw["train_loader"], selftrain.ClassMixLoader):
            calls.append("train")
            kw["train_loader"].last_chosen = None
        out = real_train(**kw)
        if isinstance(kw["train_loader"], selftrain.ClassMixLoader):
            assert kw["train_loader"].last_chosen is not None  # the loader mixed at least one batch
        return out
    monkeypatch.setattr(rmain, "train", counted)
    return calls


def test_main_classmix_domain_adaptation(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    calls = _count_self_training(monkeypatch)
    rmain.main(["--config", _cfg(tmp_path, "bf16"), "--domain_adaptation", "--self_training"])
    assert calls == ["generate", "train"]


def test_main_classmix_segmentation(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    calls = _count_self_training(monkeypatch)
    rmain.main(["--config", _cfg(tmp_path, "fp32"), "--model", "bisenet", "--self_training"])
    assert calls == ["generate", "train"]
