"""The attention kernels of csrc/encoder.hip alone, through mq_debug_attention and
mq_debug_attn_oproj, against a float64 reference at logits that make the softmax work:
every attention_kernel variant, attention_rows_kernel and the fused attention + output
projection, under holes, wholly masked leading tiles and wholly masked sequences
(tests/attention_cases.py builds the operands; test_attention_cases.py checks them on the
CPU).  Then the same kernels inside the forward with query / key weights x 4.

Tolerances.  onehot / tie: exact equality (every product, sum, exp and rescale factor of
those cases is exact in fp32).  Everything else: FACTOR * d32, d32 = the max error of a
plain torch-CPU float32 restatement of the same operation on the same operands against
float64, computed per case.  FACTOR is one number per hook, the smallest power of two that
leaves 2x over the largest GPU / d32 ratio measured (profiles/attn_kernels/accuracy.txt);
the 2x covers summation order and expf differing from the CPU's.
"""
import functools

import numpy as np
import pytest

import attention_cases as ac
from mediquery_hip import _lib
from mediquery_hip.config import BertConfig, POOL_CLS, POOL_MEAN
from oracle.encoder import OracleEncoder
from test_gpu_encoder import _close

pytestmark = pytest.mark.gpu

FACTOR_ATTENTION = 8    # largest ratio measured 2.62 (504 cases): 2x over it is 5.2
FACTOR_ATTN_OPROJ = 16  # largest ratio measured 4.82 (2340 comparisons): 2x over it is 9.6
FACTOR_FORWARD = 16     # 4x over the 2.3e-7 / 5.5e-8 the project has on record

ATTENTION_CASES = [(v, *ac.variant_shape(v, L), m, c)
                   for v, Ls in ac.VARIANT_L.items() for L in Ls
                   for m in ac.mask_names(ac.variant_shape(v, L)[0], L) for c in ac.CLASSES]


def _dev():
    import torch
    return torch.device("cuda", 0)


def _run_attention(case, B, L, heads, variant):
    import torch
    dev = _dev()
    qkv = torch.tensor(np.array(case["qkv"]), device=dev)
    mask = torch.tensor(np.array(case["mask"]), device=dev)
    ctx = torch.full((B * L, case["H"]), float("nan"), device=dev)
    _lib.call("mq_debug_attention", _lib.ptr(qkv), _lib.ptr(mask), B, L, case["H"], heads, case["scale"],
              variant, _lib.ptr(ctx), _lib.stream_handle())
    torch.cuda.synchronize()
    return ctx.cpu().numpy()


@functools.lru_cache(maxsize=8)
def _attention_refs(cls, B, L, heads, mask_name):
    c = ac.build(cls, B, L, heads, mask_name)
    ref = ac.attention_f64(c["qkv"], c["mask"], B, L, heads, c["scale"])
    d32 = float(np.abs(ac.attention_f32_torch(c["qkv"], c["mask"], B, L, heads, c["scale"]) - ref).max())
    return ref, d32


def _ratio(err, d32):
    return 0.0 if err == 0 else float("inf") if d32 == 0 else err / d32


@pytest.mark.parametrize("variant,B,L,heads,mask_name,cls", ATTENTION_CASES,
                         ids=["v%d-B%d-L%d-h%d-%s-%s" % c for c in ATTENTION_CASES])
def test_attention_kernel(require_gpu, variant, B, L, heads, mask_name, cls):
    case = ac.build(cls, B, L, heads, mask_name)
    got = _run_attention(case, B, L, heads, variant)
    assert not np.isnan(got).any()
    dead = np.repeat(case["mask"].reshape(B, L).sum(1) == 0, L)
    assert not got[dead].any()  # a sequence with every key masked: exactly 0
    if cls in ac.EXACT:
        bad = np.flatnonzero((got != case["expect"]).any(1))
        assert bad.size == 0, "rows %s differ, max |diff| %g" % (bad[:8], np.abs(got - case["expect"]).max())
        return
    ref, d32 = _attention_refs(cls, B, L, heads, mask_name)
    err = float(np.abs(got - ref).max())
    print("ATTN_ACC attention v=%d B=%d L=%d heads=%d mask=%s cls=%s err=%.3e d32=%.3e ratio=%.2f"
          % (variant, B, L, heads, mask_name, cls, err, d32, _ratio(err, d32)))
    assert err <= FACTOR_ATTENTION * d32, (err, d32)


def test_attention_hook_rejects_bad_arguments(require_gpu):
    import torch
    dev = _dev()
    qkv = torch.zeros(64 * 3 * 768, device=dev)
    mask = torch.ones(64, dtype=torch.int32, device=dev)
    ctx = torch.zeros(64 * 768, device=dev)
    args = lambda B, L, H, heads, variant: (_lib.ptr(qkv), _lib.ptr(mask), B, L, H, heads, 0.125, variant,
                                            _lib.ptr(ctx), _lib.stream_handle())
    with pytest.raises(_lib.MQError, match="bad attention variant"):
        _lib.call("mq_debug_attention", *args(1, 8, 128, 2, 3))
    with pytest.raises(_lib.MQError, match="bad shape"):
        _lib.call("mq_debug_attention", *args(1, 8, 128, 3, 1))
    with pytest.raises(_lib.MQError, match="variant 12"):
        _lib.call("mq_debug_attention", *args(1, 8, 128, 2, 12))
    with pytest.raises(_lib.MQError, match="variant 12"):
        _lib.call("mq_debug_attention", *args(1, 33, 768, 12, 12))
    with pytest.raises(_lib.MQError, match="variant 16"):
        _lib.call("mq_debug_attention", *args(1, 65, 128, 2, 16))
    with pytest.raises(_lib.MQError, match="NULL"):
        _lib.call("mq_debug_attention", None, _lib.ptr(mask), 1, 8, 128, 2, 0.125, 1, _lib.ptr(ctx), None)
    oargs = lambda L, H, heads, hg, qf, acc: (_lib.ptr(qkv), _lib.ptr(mask), 1, L, H, heads, 0.125, _lib.ptr(qkv),
                                              _lib.ptr(qkv), _lib.ptr(qkv), 0, hg, qf, acc, _lib.ptr(ctx),
                                              _lib.stream_handle())
    for bad in ((16, 768, 12, 5, 0, 0), (16, 512, 8, 6, 0, 0), (65, 256, 4, 4, 0, 0), (17, 256, 4, 4, 1, 0),
                (16, 256, 4, 4, 0, 1), (16, 1024, 16, 4, 0, 1)):
        with pytest.raises(_lib.MQError):
            _lib.call("mq_debug_attn_oproj", *oargs(*bad))


# ------------------------------------------------- fused attention + output projection
OPROJ_SHAPES = [(12, 768, 6), (4, 256, 4), (8, 512, 4), (16, 1024, 4)]
OPROJ_L = (1, 15, 16, 17, 32, 33, 48, 64)
OPROJ_MASKS = ("ones", "holes", "prefix_mid", "dead_seq")
OPROJ_B = 2


@functools.lru_cache(maxsize=4)
def _oproj_weights(H):
    r = np.random.default_rng([5, H])
    Wo = (0.05 * r.standard_normal((H, H))).astype(np.float32)
    bo = r.standard_normal(H).astype(np.float32)
    resid = r.standard_normal((OPROJ_B * 64, H)).astype(np.float32)
    return Wo, bo, resid


def _run_oproj(dev_ops, B, L, H, heads, scale, cls_only, hg, qf, acc):
    import torch
    planes = 1 if acc else heads // hg
    rows = B if cls_only else B * L
    out = torch.full((planes, rows, H), float("nan"), device=_dev())
    qkv, mask, Wo, bo, resid = dev_ops
    _lib.call("mq_debug_attn_oproj", _lib.ptr(qkv), _lib.ptr(mask), B, L, H, heads, scale, _lib.ptr(Wo),
              _lib.ptr(bo), _lib.ptr(resid), cls_only, hg, qf, acc, _lib.ptr(out), _lib.stream_handle())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert not np.isnan(got).any()
    return got


@pytest.mark.parametrize("cls", ("flat", "sharp", "offset"))
@pytest.mark.parametrize("cls_only", (0, 1))
@pytest.mark.parametrize("L", OPROJ_L)
@pytest.mark.parametrize("heads,H,hg", OPROJ_SHAPES)
def test_attn_oproj_kernel(require_gpu, heads, H, hg, L, cls_only, cls):
    import torch
    B, planes, KG = OPROJ_B, heads // hg, hg * ac.DH
    Wo, bo, resid_all = _oproj_weights(H)
    resid = resid_all[:B * L]
    rows = np.arange(B) * L if cls_only else np.arange(B * L)
    Wo64, t = Wo.astype(np.float64), torch.tensor
    for mask_name in OPROJ_MASKS:
        if not ac.mask_fits(mask_name, B, L):
            continue
        case = ac.build(cls, B, L, heads, mask_name)
        scale = case["scale"]
        ctx64 = ac.attention_f64(case["qkv"], case["mask"], B, L, heads, scale)[rows]
        ctx32 = t(ac.attention_f32_torch(case["qkv"], case["mask"], B, L, heads, scale)[rows])
        # plane g: head group g's share; plane 0 also carries bias + residual
        ref, d32 = [], []
        for g in range(planes):
            sl = slice(g * KG, (g + 1) * KG)
            r64 = ctx64[:, sl] @ Wo64[:, sl].T
            r32 = ctx32[:, sl] @ t(Wo[:, sl]).T
            if g == 0:
                r64 = r64 + bo + resid[rows]
                r32 = r32 + t(bo) + t(resid[rows])
            ref.append(r64)
            d32.append(float(np.abs(r32.numpy() - r64).max()))
        full64 = ctx64 @ Wo64.T + bo + resid[rows]
        full32 = (ctx32 @ t(Wo).T + t(bo) + t(resid[rows])).numpy()
        dfull = float(np.abs(full32 - full64).max())
        dev = _dev()
        ops = tuple(t(np.array(a), device=dev) for a in (case["qkv"], case["mask"], Wo, bo, resid))
        got = _run_oproj(ops, B, L, H, heads, scale, cls_only, hg, 0, 0)
        tag = "heads=%d hg=%d L=%d cls_only=%d mask=%s cls=%s" % (heads, hg, L, cls_only, mask_name, cls)
        checks = [("sum", float(np.abs(got.astype(np.float64).sum(0) - full64).max()), dfull)]
        checks += [("plane%d" % g, float(np.abs(got[g] - ref[g]).max()), d32[g]) for g in range(planes)]
        for what, err, d in checks:
            print("ATTN_ACC attn_oproj %s %s err=%.3e d32=%.3e ratio=%.2f" % (tag, what, err, d, _ratio(err, d)))
        for what, err, d in checks:
            assert err <= FACTOR_ATTN_OPROJ * d, (tag, what, err, d)
        if L % 16 == 0:
            # the frag16 loads bring the same operands to the same MFMA chain: the same bits
            gq = _run_oproj(ops, B, L, H, heads, scale, cls_only, hg, 1, 0)
            assert np.array_equal(gq, got), (tag, float(np.abs(gq - got).max()))
        if planes == 2:
            # two addends into a zeroed plane: 0 + a + b in either order is fl(a + b)
            two = got[0] + got[1]
            ga = _run_oproj(ops, B, L, H, heads, scale, cls_only, hg, 0, 1)
            assert np.array_equal(ga[0], two), (tag, float(np.abs(ga[0] - two).max()))
            if L % 16 == 0:
                gqa = _run_oproj(ops, B, L, H, heads, scale, cls_only, hg, 1, 1)
                assert np.array_equal(gqa[0], two), (tag, float(np.abs(gqa[0] - two).max()))


# ------------------------------------------------ the kernels inside the real forward
FORWARD_CASES = [
    # B, L, lengths (None: all keys live), options, what it reaches
    (1, 32, None, {}),                          # fused attention + output projection, qf and acc
    (1, 20, None, {}),                          # ... row-major qkv
    (3, 21, None, {}),
    (2, 17, None, {"fuse_attn_oproj": 0}),      # attention_rows_kernel
    (70, 32, None, {}),                         # attention_kernel<1>
    (256, 32, None, {}),                        # attention_kernel<1, 12>
    (16, 96, None, {}),                         # <2>
    (6, 130, (130, 1, 64, 65, 100, 129), {}),   # <4>
    (1, 256, None, {}),                         # <8>
]


@functools.lru_cache(maxsize=2)
def _sharp_weights():
    return ac.sharp_state_dict(BertConfig(layers=2), 0)


@functools.lru_cache(maxsize=4)
def _forward_refs(B, L, lens, pooling):
    import torch
    cfg = BertConfig(layers=2, pooling=pooling)
    rng = np.random.default_rng(B * 31 + L)
    ids = rng.integers(106, cfg.vocab_size, (B, L)).astype(np.int32)
    mask = np.ones((B, L), np.int32)
    if lens is not None:
        for b, n in enumerate(lens):
            mask[b, n:] = 0
    e32 = OracleEncoder(cfg, _sharp_weights()).embed(ids, mask)
    e64 = OracleEncoder(cfg, _sharp_weights(), dtype=torch.float64).embed(ids, mask)
    return cfg, ids, mask, e32, e64


@pytest.mark.parametrize("prec", [_lib.MQ_DTYPE_F32, _lib.MQ_DTYPE_F32X6])
@pytest.mark.parametrize("pooling", [POOL_CLS, POOL_MEAN])
@pytest.mark.parametrize("B,L,lens,opts", FORWARD_CASES)
def test_forward_sharp_weights(require_gpu, B, L, lens, opts, pooling, prec):
    """Query / key weights x 4 (logit std ~5, mean top probability ~0.6): the forward within
    the suite's bound of the fp32 oracle, and within 16 x the fp32 oracle's own error of the
    float64 oracle."""
    from mediquery_hip.native import Encoder
    cfg, ids, mask, e32, e64 = _forward_refs(B, L, lens, pooling)
    enc = Encoder(cfg, weights=_sharp_weights())
    enc.set_precision(prec)
    for name, value in opts.items():
        enc.set_option(name, value)
    got = enc.embed(ids, mask)
    d32 = float(np.abs(e32 - e64).max())
    err = float(np.abs(got - e64).max())
    print("ATTN_ACC forward B=%d L=%d pooling=%d prec=%d opts=%s err=%.3e d32=%.3e ratio=%.2f"
          % (B, L, pooling, prec, opts, err, d32, _ratio(err, d32)))
    _close(got, e32)
    assert err <= FACTOR_FORWARD * d32, (err, d32)
