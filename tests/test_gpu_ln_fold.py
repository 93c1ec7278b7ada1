"""LayerNorm folded into the split-f32 GEMMs (MQ_ENC_OPT_LN_FOLD).

* the producer epilogue alone (mq_debug_gemm_x6p_ln, epi 5): y = A W^T + b + LN(resid)
  against float64 at the tolerance of test_gpu_gemm_x6p.py, its per-row (mean, M2) partials
  against numpy per 96-column chunk, rows >= M untouched;
* the consumer epilogue alone (epi 6 / 7 / 8) on the gamma-scaled weights against float64
  epi(LN(y) W^T + b), rows of mean / std 0, 0.1 and 1 (the last guards the cancellation in
  acc - mu s);
* the encoder, 2 layers, split-f32: fold on against the oracle, against fold off within the
  1e-5 that test_layernorm_on_load_vs_oracle allows two LayerNorm arithmetics, run to run
  and x6_presplit 0 / 1 bit-identical, and bit-identical to fold off where the gate is shut.
"""
import math

import numpy as np
import pytest

from mediquery_hip import _lib
from mediquery_hip.config import BertConfig, POOL_CLS, POOL_MEAN
from mediquery_hip.native import Encoder
from mediquery_hip.weights import synthetic_state_dict
from oracle.encoder import OracleEncoder
from test_gpu_encoder import _close
from test_gpu_gemm import _ref
from test_gpu_gemm_x6p import _split_w3

pytestmark = pytest.mark.gpu

H = 768
PW, NP = 96, 8  # columns per partial, partials per row
EPS = 1e-12
EPI_PRODUCER, EPI_BIAS_FOLD = 5, 6


def _gemm_tol(K):
    return 2e-5 * math.sqrt(K) * 4  # test_gpu_gemm_x6p.py's


def _partials(y64):
    """[M, 768] float64 -> [M, 8, 2] float32 (mean, M2) per 96-column chunk."""
    c = y64.reshape(y64.shape[0], NP, PW)
    mean = c.mean(-1)
    m2 = ((c - mean[..., None]) ** 2).sum(-1)
    return np.stack([mean, m2], -1).astype(np.float32)


def _ln64(y64, g, b):
    mu = y64.mean(-1, keepdims=True)
    var = ((y64 - mu) ** 2).mean(-1, keepdims=True)
    return (y64 - mu) / np.sqrt(var + EPS) * g.astype(np.float64) + b.astype(np.float64)


def _x6p_ln(A, w3, bias, resid, out, M, N, K, epi, stats_in=None, stats_out=None, g=None, b=None, s=None):
    p = lambda t: _lib.ptr(t) if t is not None else None
    _lib.call("mq_debug_gemm_x6p_ln", p(A), p(w3), p(bias), p(resid), p(out), M, N, K, epi, -1, p(stats_in),
              p(stats_out), p(g), p(b), p(s), EPS, _lib.stream_handle())


@pytest.mark.parametrize("ln_resid", [False, True])
@pytest.mark.parametrize("K", [32, 768])
@pytest.mark.parametrize("M", [128, 130, 257])
def test_producer(require_gpu, M, K, ln_resid):
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(M * 7 + K + int(ln_resid))
    A = torch.randn(M, K, device=dev, generator=gen)
    W = torch.randn(H, K, device=dev, generator=gen) * 0.05
    bias = torch.randn(H, device=dev, generator=gen)
    R = torch.randn(M, H, device=dev, generator=gen) * 1.5 + 0.3
    g = torch.randn(H, device=dev, generator=gen) * 0.2 + 1.0
    b = torch.randn(H, device=dev, generator=gen) * 0.1
    w3 = _split_w3(W)
    r64 = R.cpu().numpy().astype(np.float64)
    stats_in = torch.from_numpy(_partials(r64)).to(dev) if ln_resid else None
    rows = (M + 127) // 128 * 128 + 128  # whole tiles and one more past M: must stay as they are
    out = torch.full((rows, H), float("nan"), device=dev)
    stats = torch.full((rows, NP, 2), float("nan"), device=dev)
    _x6p_ln(A, w3, bias, R, out, M, H, K, EPI_PRODUCER, stats_in, stats, g if ln_resid else None,
            b if ln_resid else None)
    torch.cuda.synchronize()
    got, st = out.cpu().numpy(), stats.cpu().numpy()
    assert np.isnan(got[M:]).all() and np.isnan(st[M:]).all()
    resid64 = _ln64(r64, g.cpu().numpy(), b.cpu().numpy()) if ln_resid else r64
    ref = A.double().cpu().numpy() @ W.double().cpu().numpy().T + bias.double().cpu().numpy() + resid64
    err = np.abs(got[:M] - ref).max()
    print("producer M=%d K=%d ln_resid=%d: max |y - f64| %.3g (tol %.3g)" % (M, K, ln_resid, err, _gemm_tol(K)))
    assert err < _gemm_tol(K), err
    # the partials of the y that was written: fp32 sums of 96 terms, error <= 95 u sum |v| / 96
    # for the mean (u = 2^-24; 2^-23 here) and a relative 96 * 2^-22 for the sum of squares
    y64 = got[:M].astype(np.float64)
    want = _partials(y64).astype(np.float64)
    absmean = np.abs(y64.reshape(M, NP, PW)).mean(-1)
    assert (np.abs(st[:M, :, 0] - want[:, :, 0]) <= PW * 2.0 ** -23 * absmean).all()
    np.testing.assert_allclose(st[:M, :, 1], want[:, :, 1], rtol=PW * 2.0 ** -22, atol=0)


@pytest.mark.parametrize("epi", [6, 7, 8])
@pytest.mark.parametrize("N", [192, 200])
@pytest.mark.parametrize("M", [128, 130])
def test_consumer(require_gpu, M, N, epi):
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(M * 7 + N + epi)
    # rows of std 1 and mean / std 0, 0.1, 1 in turn
    ratio = torch.tensor([0.0, 0.1, 1.0], device=dev)[torch.arange(M, device=dev) % 3]
    Y = torch.randn(M, H, device=dev, generator=gen)
    Y = (Y - Y.mean(1, keepdim=True)) / Y.std(1, keepdim=True) + ratio[:, None]
    W = torch.randn(N, H, device=dev, generator=gen) * 0.05
    bias = torch.randn(N, device=dev, generator=gen)
    g = torch.randn(H, device=dev, generator=gen) * 0.2 + 1.0
    b = torch.randn(H, device=dev, generator=gen) * 0.1
    Wg = torch.empty_like(W)
    s = torch.empty(N, device=dev)
    c = torch.empty(N, device=dev)
    _lib.call("mq_debug_ln_fold_weight", _lib.ptr(W), _lib.ptr(bias), _lib.ptr(g), _lib.ptr(b), N, H, _lib.ptr(Wg),
              _lib.ptr(s), _lib.ptr(c), _lib.stream_handle())
    w3 = _split_w3(Wg)
    y64 = Y.cpu().numpy().astype(np.float64)
    stats = torch.from_numpy(_partials(y64)).to(dev)
    out = torch.full((M, N), float("nan"), device=dev)
    _x6p_ln(Y, w3, c, None, out, M, N, H, epi, stats_in=stats, s=s)
    torch.cuda.synchronize()
    # the folded vectors themselves: float64 sums rounded once
    wg64 = Wg.double().cpu().numpy()
    np.testing.assert_allclose(s.cpu().numpy(), wg64.sum(1), rtol=2.0 ** -23, atol=1e-9)
    ln = torch.from_numpy(_ln64(y64, g.cpu().numpy(), b.cpu().numpy())).to(dev)
    ref = _ref(ln, W, bias, None, epi - EPI_BIAS_FOLD).cpu().numpy()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    err = np.abs(got - ref)
    for k, r in enumerate((0.0, 0.1, 1.0)):
        print("consumer M=%d N=%d epi=%d mean/std=%.1f: max |out - f64| %.3g (tol %.3g)"
              % (M, N, epi, r, err[k::3].max(), _gemm_tol(H)))
    assert err.max() < _gemm_tol(H), err.max()


# ---------------------------------------------------------------------------- encoder
_ORACLE_H = {}


def _batch(B, L):
    cfg = BertConfig(layers=2)
    rng = np.random.default_rng(B * 11 + L)
    ids = rng.integers(0, cfg.vocab_size, (B, L)).astype(np.int32)
    mask = np.ones((B, L), np.int32)
    if B == 300:  # every third sequence ragged
        for i in range(0, B, 3):
            mask[i, int(rng.integers(1, L + 1)):] = 0
    return ids, mask


def _oracle(B, L, pool):
    """The oracle's embedding; its hidden states are computed once per shape."""
    cfg = BertConfig(layers=2, pooling=pool)
    ids, mask = _batch(B, L)
    o = OracleEncoder(cfg, synthetic_state_dict(cfg, 0))
    if (B, L) not in _ORACLE_H:
        _ORACLE_H[(B, L)] = o.hidden_states(ids, mask)
    h = _ORACLE_H[(B, L)]
    o.hidden_states = lambda *_: h
    return o.embed(ids, mask)


@pytest.mark.parametrize("pool", [POOL_CLS, POOL_MEAN])
@pytest.mark.parametrize("B,L", [(256, 32), (257, 32), (300, 32)])
def test_encoder_fold(require_gpu, B, L, pool):
    cfg = BertConfig(layers=2, pooling=pool)
    ids, mask = _batch(B, L)
    enc = Encoder(cfg)
    enc.set_precision(_lib.MQ_DTYPE_F32X6)
    enc.set_option("ln_fold", 0)
    off = enc.embed(ids, mask)
    enc.set_option("ln_fold", 1)
    on = enc.embed(ids, mask)
    again = enc.embed(ids, mask)
    enc.set_option("x6_presplit", 0)
    resplit = enc.embed(ids, mask)
    print("encoder B=%d L=%d pool=%d: max |on - off| %.3g" % (B, L, pool, np.abs(on - off).max()))
    assert not np.array_equal(on, off)  # the fold ran (the gate is open at these shapes)
    _close(on, _oracle(B, L, pool))
    np.testing.assert_allclose(on, off, atol=1e-5, rtol=0)
    assert np.array_equal(on, again)
    assert np.array_equal(on, resplit), float(np.abs(on - resplit).max())


def test_encoder_gate_closed(require_gpu):
    """70 x 32 rows do not fill the chip with split-f32 tiles: the option changes nothing."""
    cfg = BertConfig(layers=2)
    ids, mask = _batch(70, 32)
    enc = Encoder(cfg)
    enc.set_precision(_lib.MQ_DTYPE_F32X6)
    enc.set_option("ln_fold", 0)
    off = enc.embed(ids, mask)
    enc.set_option("ln_fold", 1)
    assert enc.get_option("ln_fold") == 1
    assert np.array_equal(enc.embed(ids, mask), off)
