"""Convolution geometries and the tolerance comparison shared by tests/test_ops_gpu.py and the
exact integer-operand tests (tests/conv_exact_ref.py, test_conv_exact_cpu.py, test_conv_exact_gpu.py).
Importable without a device."""
import torch

TOL = {torch.float32: 2e-4, torch.bfloat16: 3e-2}


def _close(got, ref, dt, what, tol=None):
    got = got.detach().double().cpu()
    ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    t = tol if tol is not None else TOL[dt]
    assert err <= t * scale + 1e-6, f"{what}: max err {err:.3e} vs scale {scale:.3e} (tol {t})"


CONV_CASES = [
    # n, c, h, w, k, kh, stride, pad, dil, bias
    (2, 3, 32, 48, 64, 7, 2, 3, 1, False),     # ResNet stem (Cin=3, scalar gather)
    (2, 3, 32, 32, 64, 3, 2, 1, 1, False),     # spatial path conv1
    (2, 64, 16, 24, 64, 3, 1, 1, 1, False),    # BasicBlock 3x3
    (2, 64, 16, 16, 128, 3, 2, 1, 1, False),   # stride-2 3x3
    (2, 64, 16, 16, 128, 1, 2, 0, 1, False),   # downsample 1x1 s2
    (2, 19, 32, 64, 64, 4, 2, 1, 1, True),     # TinyD conv1 (Cin=19)
    (2, 64, 16, 32, 1, 4, 2, 1, 1, True),      # D classifier (Cout=1)
    (1, 64, 13, 17, 64, 3, 1, 2, 2, False),    # atrous d=2, odd sizes
    (1, 128, 9, 11, 19, 3, 1, 6, 6, True),     # ASPP-like, Cout=19
    (2, 19, 16, 16, 19, 1, 1, 0, 1, True),     # final 1x1 19->19
    (8, 256, 1, 1, 256, 1, 1, 0, 1, True),     # ARM 1x1 on pooled vectors
    (8, 512, 1, 1, 512, 1, 1, 0, 1, True),     # pooled, vector kernels (16-B chunks, butterfly dgrad)
    (5, 64, 1, 1, 40, 1, 1, 0, 1, True),       # pooled vector kernels: 5 rows, k < 64 lanes
    (12, 256, 1, 1, 128, 1, 1, 0, 1, True),    # pooled: 12 rows (32-row vector fwd, scalar dgrad)
    (2, 19, 1, 1, 19, 1, 1, 0, 1, True),       # pooled, C % 8 != 0: scalar kernels (FFM attention)
    (2, 1024, 8, 16, 19, 3, 1, 1, 1, False),   # FFM conv (K=9216, N=19)
    (2, 256, 8, 8, 512, 3, 2, 1, 1, False),    # layer4 conv1
    (1, 32, 13, 17, 64, 3, 2, 1, 1, False),    # stride-2 dgrad phases, odd sizes
    (2, 8, 9, 11, 16, 4, 2, 1, 1, True),       # k4 s2 phases, odd sizes
    (2, 16, 7, 9, 32, 1, 2, 0, 1, False),      # 1x1 s2: odd phases receive nothing
    (8, 128, 64, 64, 128, 3, 1, 1, 1, False),  # 128x128 LDS-DMA tiles (fwd and dgrad)
    (2, 128, 8, 128, 19, 3, 1, 1, 1, False),   # halo direct conv (hconv.hip): Cout 19, w % 64 == 0
    (1, 64, 12, 64, 32, 3, 1, 1, 1, True),     # hconv with bias, Cout 32, edge tiles on 3 row-blocks
    (1, 256, 8, 64, 64, 3, 1, 1, 1, True),     # hconv N-tiled (Cin >= 256, Cout 2 x 32), fwd and dgrad
    (2, 256, 6, 100, 19, 3, 1, 1, 1, False),   # halo weight gradient (nwgrad): 2 channel chunks, partial column tiles
    (1, 128, 5, 64, 32, 3, 1, 1, 1, True),     # nwgrad: Cout 32 (no dY pad), odd rows, dbias
    (2, 512, 16, 32, 512, 3, 1, 1, 1, False),  # layer4-like: DGRAD split-K (128x128 tiles, fp32 slabs)
    (2, 512, 16, 32, 512, 3, 1, 2, 2, False),  # dilated (DeepLab layer3-like, small M): DGRAD split-K
    (2, 256, 16, 32, 19, 3, 1, 2, 2, True),    # ASPP-like narrow output, few M tiles: FWD split-K slabs
    (2, 512, 32, 64, 19, 1, 1, 0, 1, True),    # supervision 1x1 (pw.hip backward): 1 row group
    (2, 40, 32, 64, 32, 1, 1, 0, 1, True),     # pw.hip: Cout 32, 12 row groups
    (4, 19, 32, 32, 19, 1, 1, 0, 1, True),     # pw.hip: final 19->19, odd Cin (scalar lanes)
    (1, 1024, 64, 64, 16, 1, 1, 0, 1, False),  # pw.hip: two lane passes over 1024 channels
    # persistent implicit-GEMM launches (more tiles than resident workgroups: a workgroup walks
    # several tiles, the next tile's first K-tile DMA in flight during the epilogue):
    (8, 128, 67, 131, 128, 3, 1, 1, 1, False),  # 549 ragged 128x128 FWD / DGRAD tiles
    (24, 64, 161, 97, 128, 3, 2, 1, 1, False),  # stride 2, odd sizes: FWD 745 tiles; DGRAD's
                                                # 4 parity phases of unequal rows (tile holes)
]

FOLD_CASES = [
    # n, c, h, w, k, kh, stride, pad, bias, act, residual
    (2, 3, 32, 48, 64, 7, 2, 3, False, 1, False),    # stem conv + bn1 + relu
    (2, 64, 16, 24, 64, 3, 1, 1, False, 1, True),    # BasicBlock conv2 + bn2 + identity + relu
    (2, 64, 16, 16, 128, 1, 2, 0, False, 0, False),  # downsample 1x1 s2 + bn
    (8, 256, 1, 1, 256, 1, 1, 0, True, 3, False),    # ARM 1x1(bias) + bn + sigmoid (pooled-vector kernel)
    (5, 19, 1, 1, 19, 1, 1, 0, True, 1, False),      # pooled, C % 8 != 0: scalar kernel with the fold
    (2, 1024, 8, 16, 19, 3, 1, 1, False, 1, False),  # FFM ConvBlock (N=19: scalar epilogue)
    (8, 128, 64, 64, 128, 3, 1, 1, False, 1, True),  # 128x128 LDS-DMA tile + residual
    (2, 256, 8, 64, 256, 3, 1, 1, False, 1, True),   # halo conv (bf16), 4 x 64 tiles + residual
    (2, 512, 8, 32, 512, 3, 1, 1, False, 1, True),   # halo conv (bf16), 8 x 32 tiles (layer4) + residual
]
