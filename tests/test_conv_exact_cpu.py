"""CPU self-check of the exact integer-operand convolution tests (tests/conv_exact_ref.py): the
generated operands of every case the GPU file uses meet the conditions that make a bit-for-bit
comparison valid, and the comparison rejects the damage a wrong kernel would do -- damage the
3e-2 tolerance of tests/test_ops_gpu.py lets through.  No device needed."""
import pytest
import torch
import torch.nn.functional as TF

from tests import conv_exact_ref as E
from tests.conv_cases import CONV_CASES, FOLD_CASES, _close

BF16, F32 = torch.bfloat16, torch.float32

# the rows whose weight gradient the tolerance test cannot tell from one that lost a tile tail
LOST_TAIL_ROWS = [
    (8, 128, 64, 64, 128, 3, 1, 1, 1),
    (8, 128, 67, 131, 128, 3, 1, 1, 1),   # persistent, ragged
    (24, 64, 161, 97, 128, 3, 2, 1, 1),   # persistent, stride 2
]


def test_lost_tail_rows_are_conv_cases():
    rows = [tuple(c[:9]) for c in CONV_CASES]
    assert all(r in rows for r in LOST_TAIL_ROWS)


def test_every_case_meets_the_conditions():
    """Operands and reference of every case of test_conv_exact_gpu.py: partial sums below 2^24,
    non-degenerate operands, every output representable in bf16 / fp32."""
    cases = E.all_cases(CONV_CASES, FOLD_CASES)
    assert len(cases) >= len(CONV_CASES) + 10
    for geo, bias in cases:
        ops, ref = E.case_data(geo, bias)
        E.check_conditions(ops, ref)
        assert (ref.db is not None) == bias
        assert not any(t.requires_grad for t in (ops.x, ops.w, ops.dy, ref.y, ref.dx, ref.dw))


def test_epilogue_cases_are_representable():
    """y = act(conv * scale + shift + res) with scale in {-1, -0.5, 0.5, 1}, integer shift and
    residual: representable in bf16 and fp32 for act NONE and RELU on every fused-epilogue case
    (the halves stay below 128, where bf16 still holds them), and scale / shift / res as specified."""
    for geo, residual in E.epilogue_cases(FOLD_CASES) + [(E.SLICE_CASE[0], False)]:
        ops, ref = E.case_data(geo, False)
        scale, shift, res = E.epilogue_operands(geo, geo[4], residual)
        assert set(scale.tolist()) <= {-1.0, -0.5, 0.5, 1.0} and len(set(scale.tolist())) > 1
        assert torch.equal(shift, shift.round()) and shift.abs().max().item() <= 8
        assert (res is not None) == residual
        if residual:
            assert torch.equal(res, res.round()) and res.abs().max().item() <= 4 and res.shape == ref.y.shape
        for act in (0, 1):
            y = E.epilogue_reference(ref.y, scale, shift, res, act)
            for dt in (BF16, F32):
                E.check_value(y, dt, (geo, act))
            assert (y != 0).double().mean().item() > 0.3, (geo, act)
            assert act == 0 or y.min().item() == 0.0


def test_accumulate_and_mask_cases_are_representable():
    """prior + reference with integer priors in [-4, 4] is representable wherever the accumulate
    tests use it."""
    g = E.generator("prior-check")
    for geo, bias in E.ACC_FWD_CASES:
        _, ref = E.case_data(geo, bias)
        for dt in (BF16, F32):
            E.check_value(ref.y.abs() + 4, dt, (geo, "y + prior"))
    for geo in E.ACC_DGRAD_CASES:
        _, ref = E.case_data(geo, False)
        for dt in (BF16, F32):
            E.check_value(ref.dx.abs() + 4, dt, (geo, "dx + prior"))
    for geo, bias in E.ACC_WGRAD_CASES:
        _, ref = E.case_data(geo, bias)
        E.check_value(ref.dw + E.integers(g, ref.dw.shape, -4, 4), F32, (geo, "dw + prior"))


def _assert_rejected(got, ref, dt, what):
    with pytest.raises(AssertionError, match="elements differ"):
        E.assert_exact(got, ref, dt, what)


def test_comparison_accepts_the_reference_and_rejects_one_element():
    ops, ref = E.case_data((1, 32, 13, 17, 64, 3, 2, 1, 1), False)
    for dt in (BF16, F32):
        for t in (ref.y, ref.dx):
            E.assert_exact(t.to(dt), t, dt, "same")
            E.assert_exact(t.to(dt).contiguous(memory_format=torch.channels_last), t, dt, "same, NHWC")
            bad = t.clone()
            bad[0, 3, 2, 1] += 1
            _assert_rejected(bad.to(dt), t, dt, "one element off by one")
            bad = t.to(dt).clone()
            bad[0, 0, 0, 0] = float("nan")
            _assert_rejected(bad, t, dt, "a NaN")
    E.assert_exact(ref.dw.float(), ref.dw, F32, "same dw")
    with pytest.raises(AssertionError):
        E.assert_exact(ref.dw.float()[:, :, :2], ref.dw, F32, "wrong shape")
    with pytest.raises(AssertionError):
        E.assert_exact(ref.dw.double(), ref.dw, F32, "wrong dtype")


@pytest.mark.parametrize("geo", LOST_TAIL_ROWS)
def test_lost_reduction_tail_is_rejected_where_the_tolerance_accepts_it(geo):
    """dw with the last 16 pixels of the N*Ho*Wo reduction left out -- a ragged final K-tile
    skipped or mis-masked.  The unmodified _close at the bf16 tolerance accepts it (the gap this
    file closes); the exact comparison does not."""
    n, c, h, w, k, kh, s, p, d = geo
    ops, ref = E.case_data(geo, False)
    ho, wo = E.out_hw(geo)
    assert wo >= 16
    tail = torch.zeros(1, k, ho, wo, dtype=ref.dw.dtype)
    tail[0, :, -1, -16:] = ops.dy[-1, :, -1, -16:].to(ref.dw.dtype)  # the last 16 pixels in (n, ho, wo) order
    lost = torch.nn.grad.conv2d_weight(ops.x[-1:].to(ref.dw.dtype), ops.w.shape, tail, s, p, d)
    damaged = ref.dw - lost
    assert (lost != 0).double().mean().item() > 0.3
    _close(damaged, ref.dw, BF16, "dw, 16 pixels lost")           # accepted at 3e-2
    _assert_rejected(damaged.float(), ref.dw, F32, "dw, 16 pixels lost")
    with pytest.raises(AssertionError):                            # (the fp32 tolerance does notice)
        _close(damaged, ref.dw, F32, "dw, 16 pixels lost")


def test_tap_lost_at_the_right_border_is_rejected():
    """y with one filter tap zeroed at the right-hand border column only (a halo column not staged,
    an edge tile's mask off by one)."""
    geo = (2, 64, 16, 24, 64, 3, 1, 1, 1)
    ops, ref = E.case_data(geo, False)
    only = torch.zeros_like(ops.w)
    only[:, :, 1, 0] = ops.w[:, :, 1, 0]  # the tap left of the centre: inside the image at the border
    part = TF.conv2d(ops.x, only, None, 1, 1, 1)
    damaged = ref.y.clone()
    damaged[..., -1] -= part[..., -1].to(ref.y.dtype)
    changed = (damaged != ref.y)
    assert bool(changed[..., -1].any()) and not bool(changed[..., :-1].any())
    for dt in (BF16, F32):
        _assert_rejected(damaged.to(dt), ref.y, dt, "y, a tap lost at the border")


def test_short_stride2_phase_is_rejected():
    """dx of a stride-2 conv whose four parity phases have unequal row counts, one phase a row
    short (a tile hole mis-sized)."""
    geo = (1, 32, 13, 17, 64, 3, 2, 1, 1)
    ops, ref = E.case_data(geo, False)
    h = geo[2]
    for a in (0, 1):
        for b in (0, 1):
            last = range(a, h, 2)[-1]
            damaged = ref.dx.clone()
            assert bool((damaged[:, :, last, b::2] != 0).any())
            damaged[:, :, last, b::2] = 0
            for dt in (BF16, F32):
                _assert_rejected(damaged.to(dt), ref.dx, dt, f"dx, phase ({a}, {b}) a row short")
