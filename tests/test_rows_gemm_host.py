"""mq_debug_rows_gemm and mq_debug_ln_pool check every argument before any HIP call: on a
machine without a GPU a bad argument answers with its own message (a HIP call would fail with
"no device" instead), as test_cross_encoder_host.py shows for the cross-encoder head."""
import numpy as np
import pytest

import rows_gemm_cases as rc
from mediquery_hip import _lib

_BUF = np.zeros(64, np.float32)


def _args(**kw):
    p = _lib.ptr(_BUF)
    base = dict(kind="oproj", A=p, lda=256, W=p, bias=p, resid=p, ldr=32, out=p, M=1, N=32, K=256)
    ln = dict(kind="qkv", A=p, W=p, bias=p, out=p, M=1, N=48, K=256, ln_g=p, ln_b=p)
    return rc.rows_gemm_args(**dict(ln if kw.get("kind") in ("qkv", "up") else base, **kw))


@pytest.mark.parametrize("kw,msg", [
    (dict(kind=4), "bad kind"),
    (dict(variant=2), "variant must be 0 or 1"),
    (dict(A=None), "NULL buffer"),
    (dict(W=None), "NULL buffer"),
    (dict(bias=None), "NULL buffer"),
    (dict(out=None), "NULL buffer"),
    (dict(resid=None), "residual kinds need resid"),
    (dict(M=0), r"M must be in \[1, 256\]"),
    (dict(M=257), r"M must be in \[1, 256\]"),
    (dict(N=40), "multiple of 16"),                       # N % 16
    (dict(kind="qkv", variant=1, N=32), "multiple of 48"),   # FL_OT: whole blocks per third
    (dict(K=384), "multiple of 256"),
    (dict(K=1280), "no kernel for a per-split depth of 1280"),   # NB 5: launch_rows' default: case
    (dict(K=2560), "no kernel for a per-split depth"),           # NB 10
    (dict(kind="down", K=3072, splits=3, variant=1), "acc needs exactly two K splits"),
    (dict(kind="down", K=2048, splits=1, variant=1), "acc needs exactly two K splits"),
    (dict(kind="down", K=3072, splits=5), r"splits must be in \[1, 4\]"),
    (dict(kind="down", K=2048, splits=3), r"multiple of 256 \* splits"),
    (dict(kind="down", K=3072, splits=2, o_plane=16), "o_plane must hold"),
    (dict(kind="oproj", K=512, splits=2), "oproj takes an unsplit K"),
    (dict(lda=128), "lda must be"),
    (dict(ldr=16), "ldr >= N"),
    (dict(kind="qkv", K=1536), "hidden in 256 / 512 / 768 / 1024"),   # H not in the set
    (dict(kind="up", K=2048), "hidden in 256 / 512 / 768 / 1024"),
    (dict(kind="qkv", ln_g=None), "LayerNorm weights"),
    (dict(kind="qkv", s_in=5), "s_in out of range"),
    (dict(kind="up", s_in=0), "s_in out of range"),            # the gather is the QKV launch's
    (dict(kind="qkv", s_in=0), "gather needs ids, pos, typ"),
    (dict(kind="qkv", s_in=2, a_plane=2), "a_plane must be"),
    (dict(nt_w=2), "nt_w must be 0 or 1"),
    (dict(zbuf=_lib.ptr(_BUF), zn=6), "zn % 4 == 0"),
    (dict(zn=8), "zn % 4 == 0"),                               # zn without a zbuf
])
def test_rows_gemm_arguments_rejected_before_any_hip_call(kw, msg):
    with pytest.raises(_lib.MQError, match=msg) as ei:
        _lib.call("mq_debug_rows_gemm", *_args(**kw))
    assert ei.value.code == -1


@pytest.mark.parametrize("kw,msg", [
    (dict(hs=None), "NULL buffer"),
    (dict(out=None), "NULL buffer"),
    (dict(H=384), "hidden must be"),
    (dict(B=0), "bad shape"),
    (dict(planes=5), r"planes must be in \[1, 4\]"),
    (dict(planes=2, plane=0), "plane must be"),
    (dict(pooling=2), "bad pooling"),
    (dict(rows=2), "rows per sequence"),
    (dict(rows=1, pooling=_lib.MQ_POOL_MEAN), "rows per sequence"),
    (dict(pooling=_lib.MQ_POOL_MEAN, rows=4, mask=None), "needs the mask"),
    (dict(raw=2), "raw must be"),
])
def test_ln_pool_arguments_rejected_before_any_hip_call(kw, msg):
    p = _lib.ptr(_BUF)
    a = dict(hs=p, planes=1, plane=0, mask=p, B=1, L=4, rows=4, pooling=_lib.MQ_POOL_CLS, g=p, b=p, eps=1e-12, H=256,
             out=p, raw=0, stream=None)
    a.update(kw)
    with pytest.raises(_lib.MQError, match=msg) as ei:
        _lib.call("mq_debug_ln_pool", *a.values())
    assert ei.value.code == -1
