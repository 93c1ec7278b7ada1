"""The attention test operands keep their promises (CPU): the onehot / tie logit gap, the
exact expected rows under a plain float32 restatement, and the float64 reference against
the oracle's attention.  test_gpu_attention.py runs the kernels on these cases."""
import numpy as np
import pytest
import torch

import attention_cases as ac
from oracle.encoder import OracleEncoder

# every (B, L, heads) the GPU tests of mq_debug_attention use
SHAPES = sorted({ac.variant_shape(v, L) for v, Ls in ac.VARIANT_L.items() for L in Ls})


def test_masks_are_what_they_say():
    for B, L in ((2, 1), (2, 2), (2, 5), (2, 33), (2, 64), (1, 130), (3, 290)):
        names = ac.mask_names(B, L)
        assert "ones" in names
        for name in names:
            m = ac.make_mask(name, B, L)
            assert m.shape == (B, L) and m.dtype == np.int32 and set(np.unique(m)) <= {0, 1}
            if name == "ones":
                assert m.all()
            elif name == "prefix1":
                assert (m.sum(1) == 1).all() and m[:, 0].all()
            elif name == "prefix_lm1":
                assert (m.sum(1) == L - 1).all() and not m[:, -1].any()
            elif name == "prefix_mid":
                n = int(m[0].sum())
                assert 1 < n < L - 1 and n % 16 and m[:, :n].all() and not m[:, n:].any()
            elif name == "holes":
                assert m[:, 0].all() and (m.sum(1) == L - max(1, L // 5)).all()
                assert (np.diff(m, axis=1) == 1).any()  # a hole: a live key after a masked one
            elif name == "lead32":
                assert not m[:, :32].any() and m[:, 32:].all()
            elif name == "dead_seq":
                assert not m[0].any() and m[1:].all()
    assert "lead32" in ac.mask_names(2, 33) and "lead32" not in ac.mask_names(2, 32)
    assert "dead_seq" not in ac.mask_names(1, 130)
    assert ac.mask_names(2, 1) == ["ones", "dead_seq"]


@pytest.mark.parametrize("cls", ac.EXACT)
@pytest.mark.parametrize("B,L,heads", SHAPES)
def test_exact_classes_gap_and_rows(cls, B, L, heads):
    """For every (shape, mask) the GPU tests use: the winning logit is 512, every other live
    key is at least 112 below (so its fp32 exp is exactly 0), tie winners come in pairs that
    sit in different 32-key tiles wherever the pairing can reach one, masked keys copy a
    live key's row, and a plain numpy float32 softmax gives the expected rows bit for bit."""
    for name in ac.mask_names(B, L):
        c = ac.build(cls, B, L, heads, name)
        assert ac.min_gap(c, B, L, heads) >= ac.MIN_GAP, name
        mask = c["mask"].reshape(B, L)
        K = c["qkv"].reshape(B, L, 3, heads, ac.DH)[:, :, 1]
        for (b, h), win in c["winners"].items():
            live = np.flatnonzero(mask[b])
            sizes = {len(w) for w in win}
            if live.size == 0:
                assert sizes == {0}
                continue
            assert sizes <= ({1, 2} if cls == "tie" else {1})
            if cls == "tie" and live.size >= 2:
                assert 2 in sizes
                first, last = live[0], live[-1]
                if first // 32 != last // 32:  # the outermost pair always crosses a tile
                    assert any(len(w) == 2 and w[0] // 32 != w[1] // 32 for w in win)
            for d in np.flatnonzero(mask[b] == 0):  # a masked key equals some live key
                assert (K[b, live, h] == K[b, d, h]).all(1).any()
        got = ac.attention_f32_numpy(c["qkv"], c["mask"], B, L, heads, c["scale"])
        assert not np.isnan(got).any()
        assert np.array_equal(got, c["expect"]), name
        assert np.array_equal(ac.attention_f64(c["qkv"], c["mask"], B, L, heads, c["scale"]),
                              c["expect"].astype(np.float64)) or cls == "tie"


def test_issue_gap_at_long_lengths():
    for L in (1, 17, 33, 64, 130, 257, 512):
        for cls in ac.EXACT:
            assert ac.min_gap(ac.build(cls, 1, L, 1, "ones"), 1, L, 1) >= ac.MIN_GAP


def test_expf_of_minus_gap_is_zero():
    assert np.exp(np.float32(-104), dtype=np.float32) == 0
    assert np.exp(np.float32(-ac.MIN_GAP), dtype=np.float32) == 0


@pytest.mark.parametrize("cls", ("flat", "sharp", "offset"))
def test_logit_classes_statistics(cls):
    B, L, heads = 2, 130, 2
    c = ac.build(cls, B, L, heads, "ones")
    x = c["qkv"].astype(np.float64).reshape(B, L, 3, heads, ac.DH)
    s = np.stack([c["scale"] * x[b, :, 0, h] @ x[b, :, 1, h].T for b in range(B) for h in range(heads)])
    if cls == "flat":
        assert 0.9 < s.std() < 1.1
    elif cls == "sharp":
        assert 10 < s.std() < 14 and s.max() > 40
    else:
        assert s.max() > 200  # exp of the unshifted logit overflows fp32 (88.7)


@pytest.mark.parametrize("name", ("ones", "prefix1", "prefix_lm1", "prefix_mid"))
@pytest.mark.parametrize("cls", ("flat", "sharp", "offset"))
def test_reference_matches_oracle_attention(cls, name):
    """attention_f64 against OracleEncoder.attention in float64 on prefix masks (1e-12: two
    orders of the same float64 sums), and the torch float32 restatement d32 is measured from
    against the oracle's own float32 attention bit for bit."""
    B, L, heads = 2, 45, 2
    c = ac.build(cls, B, L, heads, name)
    keep = torch.as_tensor(c["mask"].reshape(B, L) != 0)
    for dtype in (torch.float64, torch.float32):
        x = torch.tensor(np.array(c["qkv"]), dtype=dtype).view(B, L, 3, heads, ac.DH)
        q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
        bias = torch.zeros(B, 1, 1, L, dtype=dtype)
        bias.masked_fill_(~keep[:, None, None, :], float("-inf"))
        ref = OracleEncoder.attention(q, k, v, bias, ac.DH).transpose(1, 2).reshape(B * L, heads * ac.DH).numpy()
        if dtype == torch.float64:
            got = ac.attention_f64(c["qkv"], c["mask"], B, L, heads, c["scale"])
            np.testing.assert_allclose(got, ref, atol=1e-12, rtol=0)
        else:
            got = ac.attention_f32_torch(c["qkv"], c["mask"], B, L, heads, c["scale"])
            assert np.array_equal(got, ref)


def test_dead_sequence_reference_is_zero_and_finite():
    B, L, heads = 2, 33, 2
    for cls in ac.CLASSES:
        c = ac.build(cls, B, L, heads, "dead_seq")
        for fn in (ac.attention_f64, ac.attention_f32_numpy, ac.attention_f32_torch):
            out = fn(c["qkv"], c["mask"], B, L, heads, c["scale"])
            assert not np.isnan(out).any() and not out[:L].any() and out[L:].any()
        alone = ac.attention_f64(c["qkv"][L:], c["mask"][L:], 1, L, heads, c["scale"])
        assert np.array_equal(ac.attention_f64(c["qkv"], c["mask"], B, L, heads, c["scale"])[L:], alone)


def test_sharp_state_dict_scales_only_query_and_key():
    from mediquery_hip.config import BertConfig
    from mediquery_hip.weights import synthetic_state_dict
    cfg = BertConfig(vocab_size=200, hidden=256, layers=2, heads=4, ffn=512, max_positions=64)
    base, sharp = synthetic_state_dict(cfg, 0), ac.sharp_state_dict(cfg, 0)
    assert base.keys() == sharp.keys()
    scaled = 0
    for k in base:
        if k.endswith("self.query.weight") or k.endswith("self.key.weight"):
            assert np.array_equal(sharp[k], base[k] * np.float32(4))
            scaled += 1
        else:
            assert np.array_equal(sharp[k], base[k])
    assert scaled == 2 * cfg.layers


def test_oracle_dtype_argument():
    """OracleEncoder(dtype=float64) restates the float32 oracle at higher precision: the two
    agree to float32 rounding, and the default is unchanged (float32 out)."""
    from mediquery_hip.config import BertConfig
    cfg = BertConfig(vocab_size=200, hidden=256, layers=2, heads=4, ffn=512, max_positions=64)
    sd = ac.sharp_state_dict(cfg, 0)
    r = np.random.default_rng(3)
    ids = r.integers(0, cfg.vocab_size, (2, 20)).astype(np.int32)
    mask = np.ones((2, 20), np.int32)
    mask[1, 11:] = 0
    e32 = OracleEncoder(cfg, sd).embed(ids, mask)
    e64 = OracleEncoder(cfg, sd, dtype=torch.float64).embed(ids, mask)
    assert e32.dtype == np.float32 and e64.dtype == np.float64
    d = np.abs(e32 - e64).max()
    assert 0 < d < 2e-6, d
