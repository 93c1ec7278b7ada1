"""K2p's producer epilogue on the loader-wave tiles (csrc/gemm_x6p.hip):
the residual of the workgroup's last tile is prepared by the loader waves and handed to the
compute waves through LDS.  Tile codes 20 / 21 of mq_debug_gemm_x6p_ln run tiles 0 / 1 with
the former epilogue in the same library.

* epi 5: out and the partials bit-identical to the former epilogue for one to four k-stages
  (a three-slot ring two stages ahead), whole and ragged row counts, with and without
  stats_in; rows >= M untouched; out against float64 at test_gpu_ln_fold.py's tolerance;
* once more with more tiles than CUs, where some workgroups take the global-load epilogue
  first and the hand-off last.
"""
import numpy as np
import pytest

from mediquery_hip import _lib
from test_gpu_gemm_x6p import _split_w3
from test_gpu_ln_fold import EPS, H, NP, _gemm_tol, _ln64, _partials

pytestmark = pytest.mark.gpu

EPI_PRODUCER = 5
FORMER = 20  # tile code t + 20: tile t with the former epilogue
BM = {0: 128, 1: 256}

_CASES = {}


def _p(t):
    return _lib.ptr(t) if t is not None else None


def _producer_case(M, K, ln_resid):
    """Operands and the float64 reference of one producer shape, made once."""
    key = (M, K, ln_resid)
    if key not in _CASES:
        import torch
        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev).manual_seed(M * 7 + K + int(ln_resid))
        A = torch.randn(M, K, device=dev, generator=gen)
        W = torch.randn(H, K, device=dev, generator=gen) * 0.05
        bias = torch.randn(H, device=dev, generator=gen)
        R = torch.randn(M, H, device=dev, generator=gen) * 1.5 + 0.3
        g = torch.randn(H, device=dev, generator=gen) * 0.2 + 1.0
        b = torch.randn(H, device=dev, generator=gen) * 0.1
        r64 = R.cpu().numpy().astype(np.float64)
        stats_in = torch.from_numpy(_partials(r64)).to(dev) if ln_resid else None
        resid64 = _ln64(r64, g.cpu().numpy(), b.cpu().numpy()) if ln_resid else r64
        ref = A.double().cpu().numpy() @ W.double().cpu().numpy().T + bias.double().cpu().numpy() + resid64
        _CASES[key] = (A, _split_w3(W), bias, R, g if ln_resid else None, b if ln_resid else None, stats_in, ref)
    return _CASES[key]


def _run_producer(case, M, K, tile, rows):
    import torch
    A, w3, bias, R, g, b, stats_in, _ = case
    out = torch.full((rows, H), float("nan"), device=A.device)
    stats = torch.full((rows, NP, 2), float("nan"), device=A.device)
    _lib.call("mq_debug_gemm_x6p_ln", _p(A), _p(w3), _p(bias), _p(R), _p(out), M, H, K, EPI_PRODUCER, tile,
              _p(stats_in), _p(stats), _p(g), _p(b), None, EPS, _lib.stream_handle())
    torch.cuda.synchronize()
    return out.cpu().numpy(), stats.cpu().numpy()


def _check_producer(M, K, tile, ln_resid):
    case = _producer_case(M, K, ln_resid)
    rows = (M + BM[tile] - 1) // BM[tile] * BM[tile] + BM[tile]  # whole tiles and one more past M
    got, st = _run_producer(case, M, K, tile, rows)
    old, old_st = _run_producer(case, M, K, tile + FORMER, rows)
    err = np.abs(got[:M] - case[-1]).max()
    print("producer M=%d K=%d tile=%d ln_resid=%d: max |y - f64| %.3g (tol %.3g), differing from the former "
          "epilogue: %d of out, %d of the partials" % (M, K, tile, ln_resid, err, _gemm_tol(K),
                                                       int((got[:M] != old[:M]).sum()),
                                                       int((st[:M] != old_st[:M]).sum())))
    assert not np.isnan(old[:M]).any() and not np.isnan(old_st[:M]).any()
    assert np.array_equal(got[:M], old[:M])
    assert np.array_equal(st[:M], old_st[:M])
    assert np.isnan(got[M:]).all() and np.isnan(st[M:]).all()
    assert err < _gemm_tol(K), err


@pytest.mark.parametrize("ln_resid", [False, True])
@pytest.mark.parametrize("tile", [0, 1])
@pytest.mark.parametrize("K", [32, 64, 96, 128])
@pytest.mark.parametrize("M", [1, 64, 128, 130, 257])
def test_producer_handoff(require_gpu, M, K, tile, ln_resid):
    _check_producer(M, K, tile, ln_resid)


@pytest.mark.parametrize("ln_resid", [False, True])
def test_producer_more_tiles_than_cus(require_gpu, ln_resid):
    """CUs + 8 tiles of 128 x 192: eight workgroups walk two tiles, the first on the global-load
    epilogue (the ring carries the next tile's prefetch), the last on the hand-off."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _check_producer(128 * (cus // 4 + 1) + 2, 64, 0, ln_resid)
