"""The CLS-pooled last layer without K and V (MQ_ENC_OPT_CLS_KFREE).

* the kernels alone (mq_debug_cls_attention: u = Wk_h^T q, the pass over the input rows, ctx =
  Wv_h z + bv) against a numpy float64 restatement of the STANDARD formulation (project K and V,
  attend, take row 0), within 4 x the error of a float32 numpy restatement of that formulation on
  the same inputs (the slack is for the accumulation order); rows given normalised, and raw with
  (mean, M2) partials and random gamma / beta;
* the encoder, 2 layers, CLS pooling, both precisions: on against off within the 1e-5 of
  test_encoder_fold, on against the oracle, and on bit-identical run to run, with x6_presplit 0,
  and for the same sequences inside another batch size;
* sharp logits at test_forward_sharp_weights' bound;
* mean pooling and L = 1: the option changes nothing, bit for bit.

Batch-size pairs: the layers before the last pick their GEMM kernels by M = B L (the split-f32
gate opens at 8065 rows) and the tail's few-row GEMMs their split-K depth by ceil(B / 32), as
before this option; the pairs stay inside one such class (256 / 253, 300 / 290, 9 / 8), so what
they check is that nothing the option adds depends on B or on a sequence's place in the batch.
"""
import numpy as np
import pytest

from mediquery_hip import _lib
from mediquery_hip.config import BertConfig, POOL_CLS, POOL_MEAN
from mediquery_hip.native import Encoder
from test_gpu_attention import FACTOR_FORWARD, _forward_refs, _ratio, _sharp_weights
from test_gpu_encoder import _close
from test_gpu_ln_fold import EPS, H, NP, PW, _batch, _oracle

pytestmark = pytest.mark.gpu

HEADS, DH, B_K = 12, 64, 3
SCALE = 1.0 / 8.0
PRECS = [_lib.MQ_DTYPE_F32, _lib.MQ_DTYPE_F32X6]


# ------------------------------------------------------------------ the kernels alone
def _mask(kind, L, rng):
    m = np.ones((B_K, L), np.int32)
    if kind == "ragged":
        for b, n in enumerate((L, max(1, L // 2), int(rng.integers(1, L + 1)))):
            m[b, n:] = 0
    elif kind == "cls":
        m[:, 1:] = 0
    return m


def _ln(y, g, b, dt):
    y = y.astype(dt)
    mu = y.mean(-1, keepdims=True)
    var = ((y - mu) ** 2).mean(-1, keepdims=True)
    return (y - mu) / np.sqrt(var + dt(EPS)) * g.astype(dt) + b.astype(dt)


def _standard(x, q, wk, bk, wv, bv, mask, dt):
    """Row 0 of softmax(scale Q K^T + mask) V per head, K and V projected for every token."""
    x, q = x.astype(dt), q.astype(dt)
    L = x.shape[1]
    k = (x @ wk.astype(dt).T + bk.astype(dt)).reshape(B_K, L, HEADS, DH)
    v = (x @ wv.astype(dt).T + bv.astype(dt)).reshape(B_K, L, HEADS, DH)
    s = np.einsum("bhd,blhd->bhl", q.reshape(B_K, HEADS, DH), k) * dt(SCALE)
    s = np.where(mask[:, None, :] != 0, s, dt(-np.inf))
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    return np.einsum("bhl,blhd->bhd", p, v).reshape(B_K, H)


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("kind", ["all", "ragged", "cls"])
@pytest.mark.parametrize("L", [2, 17, 32, 33, 130])
def test_kernels_vs_float64(require_gpu, L, kind, raw):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(L * 7 + len(kind) + int(raw))
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    q = f32(rng.standard_normal((B_K, H)))
    wk, wv = (f32(rng.standard_normal((H, H)) * 0.05) for _ in range(2))
    bk, bv = (f32(rng.standard_normal(H) * 0.5) for _ in range(2))
    mask = _mask(kind, L, rng)
    g = f32(rng.standard_normal(H) * 0.2 + 1.0)
    be = f32(rng.standard_normal(H) * 0.1)
    if raw:  # rows of std 1.5 and mean 0.3, their partials as the producer GEMM leaves them
        rows = f32(rng.standard_normal((B_K, L, H)) * 1.5 + 0.3)
        c = rows.astype(np.float64).reshape(B_K * L, NP, PW)
        mean = c.mean(-1)
        stats = f32(np.stack([mean, ((c - mean[..., None]) ** 2).sum(-1)], -1))
        x64, x32 = _ln(rows, g, be, np.float64), _ln(rows, g, be, np.float32)
    else:
        rows = f32(rng.standard_normal((B_K, L, H)))
        stats = None
        x64, x32 = rows.astype(np.float64), rows
    ref = _standard(x64, q, wk, bk, wv, bv, mask, np.float64)
    ref32 = _standard(x32, q, wk, bk, wv, bv, mask, np.float32)
    t = lambda a: torch.from_numpy(a).to(dev) if a is not None else None
    dq, dx, dst, dg, db, dm, dwk, dwv, dbv = (t(a) for a in (q, rows, stats, g, be, mask, wk, wv, bv))
    ctx = torch.full((B_K, H), float("nan"), device=dev)
    _lib.call("mq_debug_cls_attention", _lib.ptr(dq), _lib.ptr(dx), _lib.ptr(dst), _lib.ptr(dg) if raw else None,
              _lib.ptr(db) if raw else None, EPS, _lib.ptr(dm), B_K, L, H, HEADS, SCALE, _lib.ptr(dwk), _lib.ptr(dwv),
              _lib.ptr(dbv), _lib.ptr(ctx), _lib.stream_handle())
    got = ctx.cpu().numpy()
    assert not np.isnan(got).any()
    err = float(np.abs(got - ref).max())
    e32 = float(np.abs(ref32 - ref).max())
    print("CLS_ACC kernels L=%d mask=%s raw=%d err=%.3e f32_standard=%.3e ratio=%.2f"
          % (L, kind, raw, err, e32, _ratio(err, e32)))
    assert err <= 4 * e32, (err, e32)


def test_kernels_all_keys_masked(require_gpu):
    """No live key: ctx = 0, as the attention kernels give."""
    import torch
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(5)
    L = 9
    q = torch.randn(B_K, H, device=dev, generator=gen)
    x = torch.randn(B_K * L, H, device=dev, generator=gen)
    wk, wv = (torch.randn(H, H, device=dev, generator=gen) * 0.05 for _ in range(2))
    bv = torch.randn(H, device=dev, generator=gen)
    mask = torch.ones(B_K, L, dtype=torch.int32, device=dev)
    mask[1] = 0
    ctx = torch.full((B_K, H), float("nan"), device=dev)
    _lib.call("mq_debug_cls_attention", _lib.ptr(q), _lib.ptr(x), None, None, None, EPS, _lib.ptr(mask), B_K, L, H,
              HEADS, SCALE, _lib.ptr(wk), _lib.ptr(wv), _lib.ptr(bv), _lib.ptr(ctx), _lib.stream_handle())
    got = ctx.cpu().numpy()
    assert (got[1] == 0).all() and np.abs(got[0]).max() > 0 and np.abs(got[2]).max() > 0


def test_kernels_reject_bad_arguments(require_gpu):
    import torch
    z = torch.zeros(4 * 1024, device="cuda")
    m = torch.ones(8, dtype=torch.int32, device="cuda")
    p = _lib.ptr
    with pytest.raises(_lib.MQError, match="bad shape"):
        _lib.call("mq_debug_cls_attention", p(z), p(z), None, None, None, EPS, p(m), 1, 2, 768, 11, SCALE, p(z), p(z),
                  p(z), p(z), None)
    with pytest.raises(_lib.MQError, match="hidden must be"):
        _lib.call("mq_debug_cls_attention", p(z), p(z), None, None, None, EPS, p(m), 1, 2, 1024, 16, SCALE, p(z), p(z),
                  p(z), p(z), None)
    with pytest.raises(_lib.MQError, match="stats need"):
        _lib.call("mq_debug_cls_attention", p(z), p(z), p(z), None, None, EPS, p(m), 1, 2, 768, 12, SCALE, p(z), p(z),
                  p(z), p(z), None)


# ---------------------------------------------------------------------------- encoder
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,L,sub", [(256, 32, 253), (300, 32, 290), (9, 33, 8)])
def test_encoder_on_vs_off(require_gpu, B, L, sub, prec):
    cfg = BertConfig(layers=2, pooling=POOL_CLS)
    ids, mask = _batch(B, L)
    enc = Encoder(cfg)
    enc.set_precision(prec)
    enc.set_option("cls_kfree", 0)
    off = enc.embed(ids, mask)
    enc.set_option("cls_kfree", 1)
    assert enc.get_option("cls_kfree") == 1
    on = enc.embed(ids, mask)
    again = enc.embed(ids, mask)
    part = enc.embed(ids[:sub], mask[:sub])
    enc.set_option("x6_presplit", 0)
    resplit = enc.embed(ids, mask)
    print("CLS_ACC encoder B=%d L=%d prec=%d: max |on - off| %.3g" % (B, L, prec, np.abs(on - off).max()))
    assert not np.array_equal(on, off)  # the path ran
    np.testing.assert_allclose(on, off, atol=1e-5, rtol=0)
    _close(on, _oracle(B, L, POOL_CLS))
    assert np.array_equal(on, again)
    assert np.array_equal(on, resplit), float(np.abs(on - resplit).max())
    assert np.array_equal(on[:sub], part), float(np.abs(on[:sub] - part).max())


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,L,lens", [(256, 32, None), (6, 130, (130, 1, 64, 65, 100, 129))])
def test_encoder_sharp_logits(require_gpu, B, L, lens, prec):
    """test_forward_sharp_weights' weights, form and bound, the option set."""
    cfg, ids, mask, e32, e64 = _forward_refs(B, L, lens, POOL_CLS)
    enc = Encoder(cfg, weights=_sharp_weights())
    enc.set_precision(prec)
    enc.set_option("cls_kfree", 1)
    got = enc.embed(ids, mask)
    d32 = float(np.abs(e32 - e64).max())
    err = float(np.abs(got - e64).max())
    print("CLS_ACC sharp B=%d L=%d prec=%d err=%.3e d32=%.3e ratio=%.2f" % (B, L, prec, err, d32, _ratio(err, d32)))
    _close(got, e32)
    assert err <= FACTOR_FORWARD * d32, (err, d32)


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,L,pool", [(9, 33, POOL_MEAN), (300, 32, POOL_MEAN), (300, 1, POOL_CLS)])
def test_option_changes_nothing_outside_its_branch(require_gpu, B, L, pool, prec):
    """Mean pooling, and CLS pooling at L = 1 (no attention to prune): bit for bit."""
    cfg = BertConfig(layers=2, pooling=pool)
    ids, mask = _batch(B, L)
    enc = Encoder(cfg)
    enc.set_precision(prec)
    enc.set_option("cls_kfree", 0)
    off = enc.embed(ids, mask)
    enc.set_option("cls_kfree", 1)
    assert np.array_equal(enc.embed(ids, mask), off)
