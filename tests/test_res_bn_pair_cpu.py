"""What functional.RES_BN_PAIR / RES_BN_BITS decide without a GPU: the host-side sizes of the mask bits and the pair
workspace, the rtsds_bn_params binding, and which BatchNorms qualify (everything else runs the chain)."""
import ctypes

import torch

from rtsds_amd import _lib
from rtsds_amd import functional as F
from rtsds_amd import nn as rnn

BF16, F32 = _lib.BF16, _lib.F32


def test_switch_defaults():
    # the pair measured faster and is on; the mask bits of the other residual BatchNorms did not
    assert F.RES_BN_PAIR is True and F.RES_BN_BITS is False


def test_bits_bytes_one_byte_per_channel_vector():
    lib = _lib.load()
    assert lib.rtsds_bn_bits_bytes(37, 24, BF16) == 37 * 3  # [rows][c / 8]
    assert lib.rtsds_bn_bits_bytes(37, 24, F32) == 37 * 6   # 16-byte vectors of fp32: 4 channels
    assert lib.rtsds_bn_bits_bytes(1 << 22, 2048, BF16) == (1 << 22) * 256  # past 2^31 elements of y
    for rows, c, dt in ((37, 20, BF16), (37, 4, F32), (0, 8, BF16), (8, 0, BF16), (8, 8, 7)):
        assert lib.rtsds_bn_bits_bytes(rows, c, dt) == 0


def test_pair_workspace_holds_two_batchnorms():
    lib = _lib.load()
    for rows, c in ((2, 8), (4100, 128), (262144, 64), (9, 2048)):
        assert lib.rtsds_bn_pair_workspace(rows, c) == 2 * lib.rtsds_bn_workspace(rows, c)
        assert lib.rtsds_bn_workspace(rows, c) % 256 == 0  # the second half stays 256-byte aligned


def test_bn_params_layout():
    # include/rtsds_hip.h rtsds_bn_params: 7 pointers, 2 floats, 1 pointer, 2 ints, 2 pointers
    assert ctypes.sizeof(_lib.BnParams) == 7 * 8 + 8 + 8 + 8 + 16
    assert _lib.BnParams.momentum.offset == 56 and _lib.BnParams.stats_part.offset == 64
    assert _lib.BnParams.accumulate.offset == 76 and _lib.BnParams.dgamma.offset == 80


def test_which_residual_batchnorms_keep_bits():
    x = torch.zeros(2, 16, 4, 8, dtype=torch.bfloat16)
    ok = F._res_bits_ok
    assert ok(x, x, True, _lib.ACT_RELU)
    assert ok(x.float(), x.float(), True, _lib.ACT_RELU)
    assert not ok(x, None, True, _lib.ACT_RELU)                  # no residual: the mask comes from x
    assert not ok(x, x, False, _lib.ACT_RELU)                    # running statistics
    assert not ok(x, x, True, _lib.ACT_LEAKY)                    # LeakyReLU keeps y
    assert not ok(x, x, True, _lib.ACT_NONE)
    assert not ok(x[:, :12], x[:, :12], True, _lib.ACT_RELU)     # c % 8
    assert not ok(x.half(), x.half(), True, _lib.ACT_RELU)       # fp16
    assert not ok(x, x.reshape(2, 16, 8, 4), True, _lib.ACT_RELU)  # differing shapes
    assert not ok(x, x.float(), True, _lib.ACT_RELU)


def test_which_downsample_branches_pair():
    conv, bn = rnn.Conv2d(16, 32, 1, 2, bias=False), rnn.BatchNorm2d(32)
    x = torch.zeros(2, 16, 4, 8, dtype=torch.bfloat16)
    assert rnn._bn_pair_ok(conv, bn, x)
    F.RES_BN_PAIR = False
    try:
        assert not rnn._bn_pair_ok(conv, bn, x)
    finally:
        F.RES_BN_PAIR = True
    assert not rnn._bn_pair_ok(conv, bn.eval(), x)
    bn.train()
    with torch.no_grad():
        assert not rnn._bn_pair_ok(conv, bn, x)
    assert not rnn._bn_pair_ok(rnn.Conv2d(16, 20, 1, bias=False), rnn.BatchNorm2d(20), x)
    assert not rnn._bn_pair_ok(conv, bn, x.half())
    assert not rnn._bn_pair_ok(rnn.Conv2d(3, 32, 1, bias=False), bn, x[:, :3])  # the image convs keep their own link
    conv.weight.requires_grad_(False)
    assert not rnn._bn_pair_ok(conv, bn, x) and rnn._bn_pair_ok(conv, bn, x.float().requires_grad_())
