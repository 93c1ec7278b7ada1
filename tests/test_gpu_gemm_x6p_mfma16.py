"""K2p (csrc/gemm_x6p.hip) on the 16x16x32 bf16 MFMA, at the shapes where a 32-deep k-step
on 16x16 accumulator blocks can go wrong: one step, even and odd step counts (the ring's
slot wrap and the in-place operand reloads), the 16-row block edges, a second wave row and
a second tile row, half-filled 32-row W3 blocks, N not a multiple of 16, a second tile
column, every epilogue on a ragged tile and on whole wave tiles, and more than one tile per
workgroup (the accumulator reset).  Checked: the default pick and every tile code (product
tiles 0, 1, 2, 3, 7 and the ring variants 4-6), each against float64 within the GEMM bound
of tests/test_gpu_gemm_x6p.py and bit for bit against the split-f32 tile of gemm_f32.hpp
(mq_debug_gemm_f32 tile 5), which restates the same arithmetic - test_gpu_gemm_x6p.py has
K in {32, 64, 768, 3072} only.  Tile codes 16 / 17 (the former 32x32x16 k-step, kept for
measurement) are fp32-class but not bit-identical: float64 bound only."""
import functools
import math

import pytest

from mediquery_hip import _lib
from test_gpu_gemm import _ref
from test_gpu_gemm_x6p import _split_w3, _x6p

pytestmark = pytest.mark.gpu

TILES = [-1, 0, 1, 2, 3, 4, 5, 6, 7]  # one arithmetic: bit-identical to mq_debug_gemm_f32 tile 5
OLD = [16, 17]                        # 32x32x16 k-step: same products, 16 k per MFMA
KS = [32, 64, 96, 160]
MS = [1, 15, 16, 17, 33, 129]
NS = [16, 48, 96, 200, 208]


@functools.lru_cache(maxsize=None)
def _case(M, N, K):
    """Operands (bias and residual non-zero), the W3 image and a dict of references."""
    import torch
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(M * 7 + N * 3 + K)
    A = torch.randn(M, K, device=dev, generator=g)
    W = torch.randn(N, K, device=dev, generator=g) * 0.05
    b = torch.randn(N, device=dev, generator=g)
    R = torch.randn(M, N, device=dev, generator=g)
    return A, W, b, R, _split_w3(W), {}


def _check(M, N, K, epi, tile):
    import torch
    A, W, b, R, w3, refs = _case(M, N, K)
    if epi not in refs:
        ref6 = torch.full((M, N), float("nan"), device=A.device)
        _lib.call("mq_debug_gemm_f32", _lib.ptr(A), _lib.ptr(W), _lib.ptr(b), _lib.ptr(R), _lib.ptr(ref6),
                  M, N, K, epi, 5, _lib.stream_handle())
        torch.cuda.synchronize()
        refs[epi] = (_ref(A, W, b, R, epi), ref6)
    ref64, ref6 = refs[epi]
    got = _x6p(A, w3, b, R, M, N, K, epi, tile)
    assert not torch.isnan(got).any(), (M, N, K, epi, tile)
    err = (got.double() - ref64).abs().max().item()
    print("M %d N %d K %d epi %d tile %d: max |err| %.3e" % (M, N, K, epi, tile, err))
    assert err < 2e-5 * math.sqrt(K) * 4, (M, N, K, epi, tile, err)
    if tile < 0 or tile % 100 < 16:
        assert torch.equal(got, ref6), (M, N, K, epi, tile, (got - ref6).abs().max().item())


@pytest.mark.parametrize("tile", TILES + OLD)
@pytest.mark.parametrize("K", KS)
def test_small_shapes(require_gpu, K, tile):
    for M in MS:
        for N in NS:
            _check(M, N, K, 0, tile)


@pytest.mark.parametrize("tile", TILES + OLD)
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_epilogues(require_gpu, epi, tile):
    _check(129, 200, 96, epi, tile)  # ragged in M and N
    _check(256, 192, 64, epi, tile)  # whole wave tiles: the buffer-store path


@pytest.mark.parametrize("tile", TILES + OLD + [300])  # 300: tile 0 walked in 2 x 4 regions
@pytest.mark.parametrize("K", [32, 96])
def test_two_tiles_per_workgroup(require_gpu, K, tile):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    # more 256-row (and so 128- and 64-row) tiles than workgroups: the accumulators restart
    # per tile, and the ring carries from one tile into the next
    _check(256 * (cus + 1), 384 if tile >= 100 else 192, K, 3, tile)
