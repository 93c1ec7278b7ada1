"""MQ_ENC_OPT_QKV_ATTN inside the forward: B = 256, L = 32, split-f32, two
layers with query / key weights x 4 (test_gpu_attention.py's sharp weights and references).

CLS pooling runs layer 0's QKV with the attention epilogue (the last layer is the CLS-only one);
mean pooling runs both layers', the second with LN2 of the first folded in when ln_fold is on.
The bound is test_forward_sharp_weights': 16 x the fp32 oracle's own error against float64.
Outside the gate (L != 32, exact f32) the option changes nothing, bit for bit.
"""
import numpy as np
import pytest

from mediquery_hip import _lib
from mediquery_hip.config import POOL_CLS, POOL_MEAN
from mediquery_hip.native import Encoder
from test_gpu_attention import FACTOR_FORWARD, _forward_refs, _sharp_weights

pytestmark = pytest.mark.gpu

B, L = 256, 32
# lengths 1 .. 32 across the batch; length 1 is a sequence with every key but CLS masked
RAGGED = tuple(b % 32 + 1 for b in range(B))


def _embed(cfg, ids, mask, prec, **opts):
    enc = Encoder(cfg, weights=_sharp_weights())
    enc.set_precision(prec)
    for name, value in opts.items():
        enc.set_option(name, value)
    return enc.embed(ids, mask)


@pytest.mark.parametrize("lens", [None, RAGGED], ids=["full", "ragged"])
@pytest.mark.parametrize("ln_fold", [0, 1])
@pytest.mark.parametrize("pooling", [POOL_CLS, POOL_MEAN])
def test_forward_with_attention_epilogue(require_gpu, pooling, ln_fold, lens):
    cfg, ids, mask, e32, e64 = _forward_refs(B, L, lens, pooling)
    on = _embed(cfg, ids, mask, _lib.MQ_DTYPE_F32X6, ln_fold=ln_fold, qkv_attn=1)
    off = _embed(cfg, ids, mask, _lib.MQ_DTYPE_F32X6, ln_fold=ln_fold, qkv_attn=0)
    assert not np.isnan(on).any()
    d32 = float(np.abs(e32 - e64).max())
    err = float(np.abs(on - e64).max())
    print("QKV_ATTN forward pooling=%d ln_fold=%d lens=%s err=%.3e d32=%.3e ratio=%.2f max|on-off|=%.3e"
          % (pooling, ln_fold, "ragged" if lens else "full", err, d32, err / d32, float(np.abs(on - off).max())))
    assert err <= FACTOR_FORWARD * d32, (err, d32)


@pytest.mark.parametrize("ln_fold", [0, 1])
def test_resplit_tiles_give_the_same_bits(require_gpu, ln_fold):
    """x6_presplit 0: the plain QKV launch, then the epilogue's attention as a launch of its own."""
    cfg, ids, mask, _, _ = _forward_refs(B, L, RAGGED, POOL_MEAN)
    pre = _embed(cfg, ids, mask, _lib.MQ_DTYPE_F32X6, ln_fold=ln_fold, qkv_attn=1)
    res = _embed(cfg, ids, mask, _lib.MQ_DTYPE_F32X6, ln_fold=ln_fold, qkv_attn=1, x6_presplit=0)
    off = _embed(cfg, ids, mask, _lib.MQ_DTYPE_F32X6, ln_fold=ln_fold, qkv_attn=0, x6_presplit=0)
    assert np.array_equal(pre, res), float(np.abs(pre - res).max())
    assert not np.array_equal(res, off)  # the path ran


@pytest.mark.parametrize("L_,prec", [(31, _lib.MQ_DTYPE_F32X6), (33, _lib.MQ_DTYPE_F32X6), (32, _lib.MQ_DTYPE_F32)])
def test_outside_the_gate_nothing_changes(require_gpu, L_, prec):
    from mediquery_hip.config import BertConfig
    cfg = BertConfig(layers=2, pooling=POOL_MEAN)
    rng = np.random.default_rng(L_)
    ids = rng.integers(106, cfg.vocab_size, (B, L_)).astype(np.int32)
    mask = np.ones((B, L_), np.int32)
    mask[1, 5:] = 0
    on = _embed(cfg, ids, mask, prec, qkv_attn=1)
    off = _embed(cfg, ids, mask, prec, qkv_attn=0)
    assert np.array_equal(on, off), float(np.abs(on - off).max())
