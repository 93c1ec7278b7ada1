"""CPU checks of tests/rows_gemm_cases.py: the numpy restatement of frag16, the operand
classes' exactness claims, the references against each other, and the float32 restatement of
the two GELU forms of csrc/gemm_epi.hpp against float64 (the figures its comment claims)."""
import numpy as np
import pytest

import rows_gemm_cases as rc


def test_frag16_offset_hand_computed_positions():
    # block (rb, cb) at ((rb * C / 16) + cb) * 256; element (r, c) at (r + 16 (c >> 2)) * 4 + (c & 3)
    assert rc.frag16_offset(0, 0, 32) == 0
    assert rc.frag16_offset(0, 3, 32) == 3            # lane 0's float4
    assert rc.frag16_offset(1, 0, 32) == 4            # lane 1 = row 1, columns 0..3
    assert rc.frag16_offset(0, 4, 32) == 64           # lane 16 = row 0, columns 4..7
    assert rc.frag16_offset(15, 15, 32) == 255        # lane 63, last float
    assert rc.frag16_offset(0, 16, 32) == 256         # column block 1
    assert rc.frag16_offset(16, 0, 32) == 512         # row block 1 of a two-block-wide matrix
    assert rc.frag16_offset(21, 27, 48) == (1 * 3 + 1) * 256 + (5 + 16 * 2) * 4 + 3


@pytest.mark.parametrize("M,C", [(1, 16), (16, 32), (17, 48), (33, 256)])
def test_frag16_encode_decode_identity(M, C):
    A = np.random.default_rng(M + C).standard_normal((M, C)).astype(np.float32)
    buf = rc.encode(A)
    assert buf.size == rc.padded_rows(M) * C
    assert np.array_equal(rc.decode(buf, M, C), A)
    full = rc.decode(buf, rc.padded_rows(M), C)
    assert np.isnan(full[M:]).all() and not np.isnan(full[:M]).any()   # the pad rows are NaN
    assert sorted(rc._offsets(rc.padded_rows(M), C).ravel()) == list(range(buf.size))  # a permutation


def test_frag16_transposed_blocks():
    M, N = 32, 48
    A = np.arange(M * N, dtype=np.float32).reshape(M, N)
    At = A.copy()
    for rb in range(2):  # the V third (columns >= 32) with every 16 x 16 block transposed
        At[16 * rb:16 * rb + 16, 32:] = A[16 * rb:16 * rb + 16, 32:].T
    buf = rc.encode(At)
    assert np.array_equal(rc.decode(buf, M, N, vt_from=32), A)
    assert np.array_equal(rc.decode(buf, M, N)[:, :32], A[:, :32])
    assert sorted(rc._offsets(M, N, 32).ravel()) == list(range(M * N))


@pytest.mark.parametrize("K,splits", [(256, 1), (4096, 1), (3072, 2), (3072, 4)])
def test_integer_class_is_exact_in_fp32(K, splits):
    assert rc.integer_bound(4096) < 2 ** 24 and rc.integer_bound(K) <= rc.integer_bound(4096)
    c = rc.build("down", "integer", 17, 32, K, 1, splits)
    for name in ("A", "W", "bias", "resid"):
        assert np.abs(c[name]).max() <= 3 and np.array_equal(c[name], np.round(c[name]))
    exp = rc.integer_expect(c)
    assert exp.shape == (splits, 17, 32) and np.abs(exp).max() <= rc.integer_bound(K // splits)
    r64, _ = rc.reference_f64(c)
    r32, _ = rc.reference_f32_torch(c)
    assert np.array_equal(exp, r64) and np.array_equal(exp, r32)
    # plane 0 alone carries bias + residual
    A, W, Ks = c["A"].astype(np.float64), c["W"].astype(np.float64), K // splits
    for z in range(1, splits):
        assert np.array_equal(exp[z], A[:, z * Ks:(z + 1) * Ks] @ W[:, z * Ks:(z + 1) * Ks].T)


@pytest.mark.parametrize("N,K", [(48, 256), (48, 1024), (768, 256), (3072, 1024), (32, 768), (1024, 256)])
def test_select_class_walks_the_depth(N, K):
    k, sign = rc.select_columns(N, K)
    assert k.min() >= 0 and k.max() < K and set(np.abs(sign)) == {1.0}
    assert len(set(k // 16)) == min(N, K // 16)       # distinct 16-deep blocks, all of them once N allows
    if N >= 48:
        assert len(set(k // (K // 16))) == 16         # every wave's K range
    c = rc.build("qkv", "select", 5, N, K)
    assert (c["W"] != 0).sum() == N and np.array_equal(c["W"][np.arange(N), k], sign)
    # the float64 reference is the selected LayerNorm column + bias
    r64, ln = rc.reference_f64(c)
    np.testing.assert_allclose(r64[0], ln[:, k] * sign + c["bias"], rtol=0, atol=1e-12)


def test_rows_class_statistics():
    x = rc.rows_class(30, 768).astype(np.float64)
    ratio = x.mean(1) / x.std(1)
    plain = np.arange(30) % 5 != 0
    for i, want in enumerate((0.0, 1.0, 30.0)):
        sel = plain & (np.arange(30) % 3 == i)
        assert np.abs(ratio[sel] - want).max() < 0.1 * max(want, 1.0)
    out = np.abs(x - np.median(x, 1, keepdims=True)).max(1)
    assert (out[::5] > 45).all() and (out[plain] < 6).all()   # the outlier channel, every fifth row
    p = rc.split_planes(rc.rows_class(7, 256), 4)
    assert p.shape == (4, 7, 256)
    assert np.abs(p.astype(np.float64).sum(0) - rc.rows_class(7, 256)).max() < 1e-5


@pytest.mark.parametrize("with_types", [True, False])
def test_gather_class_reaches_every_clamp(with_types):
    c = rc.build("qkv", "gather", 37, 48, 256, 0, 1, 7, with_types)
    assert 37 % 7 != 0
    assert set(rc.GATHER_IDS) <= set(c["ids"].tolist()) and min(rc.GATHER_IDS) < 0 and max(rc.GATHER_IDS) >= rc.VOCAB
    if with_types:
        assert set(rc.GATHER_TYPES) <= set(c["types"].tolist())
    else:
        assert c["types"] is None
    x = rc.ln_input(c, np.float64)
    for r in (0, 8, 36):
        i = min(max(int(c["ids"][r]), 0), rc.VOCAB - 1)
        t = 0 if c["types"] is None else min(max(int(c["types"][r]), 0), rc.TYPE_VOCAB - 1)
        want = c["word"][i].astype(np.float64) + c["pos"][r % 7] + c["typ"][t]
        assert np.array_equal(x[r], want)


@pytest.mark.parametrize("kind,cls,args", [("qkv", "rows", (33, 48, 768, 3)), ("up", "rows", (17, 32, 256, 2)),
                                           ("up", "randn", (16, 32, 512, 1)), ("qkv", "gather", (37, 48, 256, 0, 1, 7)),
                                           ("oproj", "randn", (17, 32, 768)), ("down", "randn", (17, 32, 3072, 1, 3))])
def test_references_agree(kind, cls, args):
    """The float32 restatement is the float64 reference to fp32 rounding, on every kind."""
    c = rc.build(kind, cls, *args)
    for tanh in ((False, True) if kind == "up" else (False,)):
        r64, l64 = rc.reference_f64(c, tanh)
        r32, l32 = rc.reference_f32_torch(c, tanh)
        assert r64.shape == r32.shape == (c["splits"], c["M"], c["N"])
        d32 = np.abs(r32 - r64).max()
        assert 0 < d32 <= 2e-5 * np.sqrt(c["K"]) * 4
        if l64 is not None:
            assert 0 < np.abs(l32 - l64).max() < 1e-4   # the 50-std rows reach ~30 after LayerNorm


def test_gelu_restatement_figures():
    """gemm_epi.hpp's forms restated in float32 with correctly rounded rcp / exp2, on the
    sweep: erf max |error| 3.8e-7 and relative 1.7e-6 where |gelu| > 1e-3 (the comment's
    claim); the tanh form 5.3e-7 and 1.3e-6; both inside the GPU tests' bounds, and the
    relative bound separates them from the plain 0.5 x (1 + erf) float32 formula."""
    x = rc.gelu_sweep()
    assert x.size == 4096 + 1024 + 10
    ea, er = rc.gelu_errors(rc.gelu_erf_f32_restated(x), x, False)
    ta, tr = rc.gelu_errors(rc.gelu_tanh_f32_restated(x), x, True)
    print("GELU restated erf abs=%.3e rel=%.3e tanh abs=%.3e rel=%.3e" % (ea, er, ta, tr))
    assert ea <= 3.9e-7 and er <= 1.7e-6
    assert ta <= 5.3e-7 and tr <= 1.3e-6
    ba, bt = rc.gelu_abs_bound(False), rc.gelu_abs_bound(True)
    print("GELU abs bounds (2 x torch float32): erf %.3e tanh %.3e" % (ba, bt))
    assert 7e-7 < ba < 2e-6 and 7e-7 < bt < 2e-6   # (torch's float32 erf differs between builds)
    assert ea <= ba and ta <= bt and max(er, tr) <= rc.GELU_REL_BOUND
    import torch
    t = torch.tensor(x)
    plain = (0.5 * t * (1 + torch.erf(t * np.float32(0.70710678)))).numpy()
    assert rc.gelu_errors(plain, x, False)[1] > 4 * rc.GELU_REL_BOUND
    # the tails: x >= 13 gives x, x <= -13 a value below the absolute bound
    big = np.array([13, 20, 40], np.float32)
    for f in (rc.gelu_erf_f32_restated, rc.gelu_tanh_f32_restated):
        assert np.array_equal(f(big), big)
        assert np.abs(f(-big)).max() <= ba and not np.isnan(f(-big)).any()


@pytest.mark.parametrize("mean", [False, True])
def test_ln_pool_references(mean):
    B, L, H = 3, 7, 256
    rows = L if mean else 1
    g, b = rc.ln_weights(H)
    planes = rc.split_planes(rc.rows_class(B * rows, H), 2)
    mask = rc.pool_mask("dead", B, L)
    assert mask[B - 1].sum() == 0 and (mask[:B - 1].sum(1) > 0).all()
    r64 = rc.ln_pool_f64(planes, mask, B, L, rows, mean, g, b, 0)
    r32 = rc.ln_pool_f32_torch(planes, mask, B, L, rows, mean, g, b, 0)
    assert 0 < np.abs(r32 - r64).max() < 1e-5
    live = slice(0, B - 1) if mean else slice(0, B)
    np.testing.assert_allclose(np.linalg.norm(r64[live], axis=1), 1.0, atol=1e-12)
    if mean:  # a wholly masked sequence: exactly 0 (count and norm clamped)
        assert not r64[B - 1].any() and not r32[B - 1].any()
    for name in ("ones", "prefix", "holes"):
        m = rc.pool_mask(name, 5, 33)
        assert (m.sum(1) >= 1).all() and (name == "ones") == bool(m.all())
