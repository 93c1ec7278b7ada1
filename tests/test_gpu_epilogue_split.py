"""K2p's split consumer epilogue (csrc/gemm_x6p.hip): at each tile end of
the GELU kinds on the loader-wave tiles, a compute wave hands the last block rows of its wave
tile to the loader wave of its SIMD through the ring slot that is free there, and both finish
their rows with the same function.  Tile codes 20 / 21 of mq_debug_gemm_x6p and
mq_debug_gemm_x6p_ln run tiles 0 / 1 with the former, single-wave epilogue in the same library.

* epi 1 / 2 (mq_debug_gemm_x6p) and 7 / 8 (mq_debug_gemm_x6p_ln, stats_in given): bit-identical
  to the former epilogue for one to four k-stages (a three-slot ring two stages ahead: every
  phase of the slot that carries the hand-over), one wave tile, whole and ragged row counts, a
  second row tile, and a ragged N on the non-fold kinds; rows >= M untouched (the debug entries
  write out at row stride N, so a store to a column >= N would land in the next row: the rows
  past M catch it for the last row, the bit-identity for the others); out against a float64
  restatement at test_gpu_ln_fold.py's tolerance;
* more tiles than CUs - eight workgroups walking two tiles, and a walk of at least three tiles
  per workgroup - where the slot is reused at consecutive tile ends;
* the encoder's embeddings with epi_split 0 and 1, bit for bit.
"""
import math

import numpy as np
import pytest

from mediquery_hip import _lib
from mediquery_hip.config import BertConfig
from mediquery_hip.native import Encoder
from test_gpu_gemm_x6p import _split_w3
from test_gpu_ln_fold import EPS, H, _gemm_tol, _partials

pytestmark = pytest.mark.gpu

FORMER = 20  # tile code t + 20: tile t with the former epilogue
BM = {0: 128, 1: 256}

_CASES = {}


def _p(t):
    return _lib.ptr(t) if t is not None else None


def _gelu64(y, tanh):
    if tanh:
        return 0.5 * y * (1 + np.tanh(math.sqrt(2 / math.pi) * (y + 0.044715 * y ** 3)))
    import torch
    return 0.5 * y * (1 + torch.erf(torch.from_numpy(y / math.sqrt(2))).numpy())


def _case(M, N, K):
    """Operands of one shape and the float64 pre-activations, plain and folded, made once."""
    key = (M, N, K)
    if key not in _CASES:
        import torch
        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev).manual_seed(M * 7 + N + K)
        A = torch.randn(M, K, device=dev, generator=gen)
        W = torch.randn(N, K, device=dev, generator=gen) * 0.05
        bias = torch.randn(N, device=dev, generator=gen)
        s = torch.randn(N, device=dev, generator=gen) * 0.1
        # the row statistics the fold kinds read: partials of rows of std 1.5 and mean 0.3
        Y = torch.randn(M, H, device=dev, generator=gen) * 1.5 + 0.3
        y64 = Y.cpu().numpy().astype(np.float64)
        stats = torch.from_numpy(_partials(y64)).to(dev)
        mu = y64.mean(-1, keepdims=True)
        rho = 1.0 / np.sqrt(((y64 - mu) ** 2).mean(-1, keepdims=True) + EPS)
        acc = A.double().cpu().numpy() @ W.double().cpu().numpy().T
        b64, s64 = bias.double().cpu().numpy(), s.double().cpu().numpy()
        plain = acc + b64
        fold = rho * (acc - mu * s64) + b64
        _CASES[key] = (A, _split_w3(W), bias, s, stats, plain, fold)
    return _CASES[key]


def _run(case, M, N, K, epi, tile, rows):
    import torch
    A, w3, bias, s, stats, _, _ = case
    out = torch.full((rows, N), float("nan"), device=A.device)
    if epi >= 6:
        _lib.call("mq_debug_gemm_x6p_ln", _p(A), _p(w3), _p(bias), None, _p(out), M, N, K, epi, tile, _p(stats), None,
                  None, None, _p(s), EPS, _lib.stream_handle())
    else:
        _lib.call("mq_debug_gemm_x6p", _p(A), _p(w3), _p(bias), None, _p(out), M, N, K, epi, tile,
                  _lib.stream_handle())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(M, N, K, epi, tile):
    case = _case(M, N, K)
    rows = (M + BM[tile] - 1) // BM[tile] * BM[tile] + BM[tile]  # whole tiles and one more past M
    got = _run(case, M, N, K, epi, tile, rows)
    old = _run(case, M, N, K, epi, tile + FORMER, rows)
    ref = _gelu64(case[6] if epi >= 6 else case[5], tanh=epi in (2, 8))
    err = np.abs(got[:M] - ref).max()
    print("split M=%d N=%d K=%d epi=%d tile=%d: max |out - f64| %.3g (tol %.3g), differing from the former "
          "epilogue: %d" % (M, N, K, epi, tile, err, _gemm_tol(K), int((got[:M] != old[:M]).sum())))
    assert not np.isnan(old[:M]).any()
    assert np.array_equal(got[:M], old[:M])
    assert np.isnan(got[M:]).all() and np.isnan(old[M:]).all()
    assert err < _gemm_tol(K), err


@pytest.mark.parametrize("epi", [1, 2, 7, 8])
@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("K", [32, 64, 96, 128])
@pytest.mark.parametrize("M", [1, 64, 128, 130, 257])
def test_split_epilogue(require_gpu, M, K, tile, epi):
    _check(M, 768, K, epi, tile)


@pytest.mark.parametrize("epi", [1, 2])
@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("K", [32, 64, 96, 128])
@pytest.mark.parametrize("M", [1, 64, 128, 130, 257])
def test_split_epilogue_ragged_n(require_gpu, M, K, tile, epi):
    _check(M, 200, K, epi, tile)


@pytest.mark.parametrize("epi", [1, 2, 7, 8])
def test_split_more_tiles_than_cus(require_gpu, epi):
    """CUs + 8 tiles of 128 x 192: eight workgroups walk two tiles, so the hand-over slot is
    used at two consecutive tile ends."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _check(128 * (cus // 4 + 1) + 2, 768, 64, epi, 0)


@pytest.mark.parametrize("epi", [1, 2, 7, 8])
def test_split_three_tiles_per_workgroup(require_gpu, epi):
    """3 CUs + 4 tiles of 128 x 192 at one stage per tile: every workgroup walks at least three
    tiles, each tile end in the next ring slot."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _check(128 * (3 * cus // 4) + 2, 768, 32, epi, 0)


@pytest.mark.parametrize("B,L", [(8, 32), (2, 128), (256, 32)])
def test_encoder_epi_split(require_gpu, B, L):
    """The embeddings with epi_split 0 and 1 are the same bits ((256, 32): a shape whose FFN-up
    runs on K2p's loader-wave tile, folded)."""
    cfg = BertConfig(layers=2)
    rng = np.random.default_rng(B * 11 + L)
    ids = rng.integers(0, cfg.vocab_size, (B, L)).astype(np.int32)
    mask = np.ones((B, L), np.int32)
    enc = Encoder(cfg)
    enc.set_precision(_lib.MQ_DTYPE_F32X6)
    enc.set_option("epi_split", 0)
    assert enc.get_option("epi_split") == 0
    off = enc.embed(ids, mask)
    enc.set_option("epi_split", 1)
    assert enc.get_option("epi_split") == 1
    on = enc.embed(ids, mask)
    assert not np.isnan(off).any()
    assert np.array_equal(on, off), float(np.abs(on - off).max())
