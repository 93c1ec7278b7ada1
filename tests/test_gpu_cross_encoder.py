"""Cross-encoder scoring on the GPU (mq_encoder_score, K13 cls_head_kernel, HipCrossEncoder /
HipReranker) against the float64 restatement of tests/cross_encoder_cases.py.

Every end-to-end logit check is |logit - float64| <= 1e-5 (cross_encoder_cases.LOGIT_TOL): the
float32 restatement is within 4.4e-7 of float64 at 12 layers and the split-f32 path is
documented within 3x of exact fp32, so the bound is ~8x the expected worst case, 5x below the
smallest ranking gap the fixtures guarantee (5e-5) and 600x below the effect of a missing
segment id (>= 6e-3).  The order must equal the float64 order for every pair.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import cross_encoder_cases as cc
from mediquery_hip import HipBertEmbeddings, HipChroma, HipCrossEncoder, HipReranker, _lib, synth
from mediquery_hip.config import BertConfig, POOL_MEAN
from mediquery_hip.native import Encoder
from mediquery_hip.tokenizer import CharTokenizer
from mediquery_hip.weights import HEAD_NAMES, synthetic_head_state_dict

pytestmark = pytest.mark.gpu

PRECS = [_lib.MQ_DTYPE_F32, _lib.MQ_DTYPE_F32X6]
TOL = cc.LOGIT_TOL


@functools.lru_cache(maxsize=None)
def _gold():
    return cc.load_golden()


@functools.lru_cache(maxsize=None)
def _oracle64(layers, n_labels=1):
    return cc.oracle(layers, torch.float64, n_labels)


@functools.lru_cache(maxsize=None)
def _encoder(layers, prec, n_labels=1):
    """One scoring encoder per (layers, precision, labels), options at their defaults."""
    cfg = BertConfig(layers=layers)
    enc = Encoder(cfg)
    enc.set_precision(prec)
    enc.load_head(synthetic_head_state_dict(cfg, 0, n_labels))
    return enc


def _score_device(enc, ids, types, mask):
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(dev)
    out = torch.full((ids.shape[0], enc.n_labels), float("nan"), device=dev)
    enc.score_device(t(ids), t(types), t(mask), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _check(got, ref, what, order=True):
    assert got.shape == ref.shape and got.dtype == np.float32, (got.shape, ref.shape, got.dtype)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print("RERANK %s: max |logit - float64| %.3e" % (what, err))
    assert err <= TOL, "%s: max |logit - float64| %.3e > %.0e" % (what, err, TOL)
    if order:
        col = 0 if ref.shape[1] == 1 else 1
        assert np.array_equal(np.argsort(-got[:, col], kind="stable"), np.argsort(-ref[:, col], kind="stable")), \
            "%s: order differs from float64 (max error %.3e)" % (what, err)


# ------------------------------------------------------------------ 1. golden (HF)
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("name,layers,labels", [("tiny", 2, 1), ("tiny3", 2, 3), ("base", 12, 1)])
def test_golden_hf_logits(require_gpu, name, layers, labels, prec):
    g = _gold()
    ids, types, mask = (g[name + s] for s in ("_ids", "_types", "_mask"))
    got = _encoder(layers, prec, labels).score(ids, types, mask)
    # (HF's own float32 rounding, <= 4.4e-7 of float64, is inside the bound)
    _check(got, g[name + "_logits"].astype(np.float64), "golden %s prec=%d" % (name, prec), order=False)


# ------------------------------------------- 2. shapes on each side of every path switch
@pytest.mark.parametrize("entry", ["host", "device"])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("layers,B,L", cc.RANK_CASES)
def test_shapes_vs_float64(require_gpu, layers, B, L, prec, entry):
    ids, types, mask, ref = cc.ranking_case(layers, B, L, _gold())
    enc = _encoder(layers, prec)
    got = enc.score(ids, types, mask) if entry == "host" else _score_device(enc, ids, types, mask)
    _check(got, ref, "layers=%d B=%d L=%d prec=%d %s" % (layers, B, L, prec, entry))
    again = enc.score(ids, types, mask)
    assert np.array_equal(got, again), "a repeated call differs"


# ---------------------------------------------------------------------------- 3. options
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("opts,B,L", [({"cls_kfree": 0, "ln_fold": 0}, 9, 130), ({"cls_kfree": 0, "ln_fold": 1}, 9, 130),
                                      ({"cls_kfree": 1, "ln_fold": 0}, 9, 130), ({"cls_kfree": 1, "ln_fold": 1}, 9, 130),
                                      ({"rows_max": 0}, 3, 21)])
def test_options(require_gpu, opts, B, L, prec):
    ids, types, mask, ref = cc.ranking_case(2, B, L, _gold())
    cfg = BertConfig(layers=2)
    enc = Encoder(cfg)
    enc.set_precision(prec)
    for k, v in opts.items():
        enc.set_option(k, v)
    enc.load_head(synthetic_head_state_dict(cfg, 0))
    _check(enc.score(ids, types, mask), ref, "opts=%s prec=%d" % (opts, prec))


@functools.lru_cache(maxsize=None)
def _fold_case():
    """64 x 128 = 8192 token rows: past the LayerNorm fold's fill-the-chip gate (8065 rows on 256
    CUs), where the batched split-f32 forward runs its folded GEMMs.  One float64 reference."""
    ids, types, mask = cc.pair_batch(11, 64, 128)
    return ids, types, mask, _oracle64(2).logits(ids, types, mask)


@pytest.mark.parametrize("fold", [0, 1])
def test_ln_fold_gate_open(require_gpu, fold):
    ids, types, mask, ref = _fold_case()
    cfg = BertConfig(layers=2)
    enc = Encoder(cfg)
    enc.set_precision(_lib.MQ_DTYPE_F32X6)
    enc.set_option("ln_fold", fold)
    enc.load_head(synthetic_head_state_dict(cfg, 0))
    # (64 random documents: no gap is guaranteed, so the logits alone are checked)
    _check(enc.score(ids, types, mask), ref, "B=64 L=128 ln_fold=%d" % fold, order=False)


# ------------------------------------------------- 4. segment ids are used on both paths
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("B,L", [(3, 21), (9, 130)])
def test_segment_ids_are_used(require_gpu, B, L, prec):
    ids, types, mask, ref = cc.ranking_case(2, B, L, _gold())
    enc = _encoder(2, prec)
    zeros = np.zeros_like(types)
    ref0 = _oracle64(2).logits(ids, zeros, mask)
    got = enc.score(ids, types, mask)
    got0 = enc.score(ids, zeros, mask)
    _check(got, ref, "types B=%d L=%d prec=%d" % (B, L, prec))
    _check(got0, ref0, "zero types B=%d L=%d prec=%d" % (B, L, prec), order=False)
    moved = float(np.abs(got - got0).min())
    assert moved > 1e-3, "segment ids moved the logits by only %.3g" % moved
    # out-of-range values are clamped to [0, type_vocab) on the device
    wild = np.where(types == 1, 7, -3).astype(np.int32)
    wild[mask == 0] = 1 << 20
    clamped = np.clip(wild, 0, 1)
    assert np.array_equal(enc.score(ids, wild, mask), enc.score(ids, clamped, mask))
    _check(enc.score(ids, wild, mask), _oracle64(2).logits(ids, clamped, mask), "clamped types", order=False)


# ------------------------------------------------------------- 5. embeddings untouched
def _embed_inputs(which):
    if which == "tokens":
        return synth.token_batch(256, 32)
    B, L = which
    ids, _, mask = cc.pair_batch(5, B, L)
    return ids, mask


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("kfree", [0, 1])
@pytest.mark.parametrize("which", [(3, 21), (9, 130), "tokens"])
def test_embeddings_untouched(require_gpu, which, kfree, prec):
    cfg = BertConfig(layers=2)
    ids, mask = _embed_inputs(which)
    B, L = ids.shape
    pids, ptypes, pmask = cc.pair_batch(6, min(B, 9), L)

    def make(head):
        enc = Encoder(cfg)
        enc.set_precision(prec)
        enc.set_option("cls_kfree", kfree)
        if head:
            enc.load_head(synthetic_head_state_dict(cfg, 0))
        return enc
    fresh = make(False)
    want = fresh.embed(ids, mask)
    fresh.set_graphs(True)
    assert np.array_equal(fresh.embed(ids, mask), want)
    enc = make(True)
    s0 = enc.score(pids, ptypes, pmask)              # score first, then embed
    assert np.array_equal(enc.embed(ids, mask), want)
    assert np.array_equal(enc.score(pids, ptypes, pmask), s0)
    enc.set_graphs(True)                             # graphs on for the embed calls
    assert np.array_equal(enc.embed(ids, mask), want)
    s1 = enc.score(ids, np.zeros_like(ids), mask)    # the embed graph's own shape, scored eagerly
    assert np.array_equal(enc.embed(ids, mask), want)
    assert np.array_equal(enc.score(ids, np.zeros_like(ids), mask), s1)
    assert np.array_equal(enc.score(pids, ptypes, pmask), s0)
    assert np.array_equal(enc.embed(ids, mask), want)
    other = make(True)                               # embed first, then score
    assert np.array_equal(other.embed(ids, mask), want)
    assert np.array_equal(other.score(pids, ptypes, pmask), s0)


# ---------------------------------------------------------------------- 6. K13 alone
@pytest.mark.parametrize("n_labels", [1, 3])
@pytest.mark.parametrize("H", [256, 768, 1024])
@pytest.mark.parametrize("B", [1, 3, 17, 70])
def test_head_kernel_vs_float64(require_gpu, B, H, n_labels):
    dev = torch.device("cuda", 0)
    cfg = BertConfig(hidden=H, heads=H // 64, layers=1)
    sd = synthetic_head_state_dict(cfg, 0, n_labels)
    rows = np.random.default_rng([B, H, n_labels]).standard_normal((B, H)).astype(np.float32)
    ref = cc.head_reference(rows, sd, torch.float64)
    cpu32 = float(np.abs(cc.head_reference(rows, sd, torch.float32) - ref).max())
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    drows = t(rows)
    dw = [t(sd[n]) for n in HEAD_NAMES]

    def run():
        out = torch.full((B, n_labels), float("nan"), device=dev)
        _lib.call("mq_debug_cls_head", _lib.ptr(drows), B, H, *[_lib.ptr(w) for w in dw], n_labels, _lib.ptr(out),
                  _lib.stream_handle())
        torch.cuda.synchronize()
        return out.cpu().numpy()
    got = run()
    assert not np.isnan(got).any()
    err = float(np.abs(got - ref).max())
    print("RERANK head B=%d H=%d labels=%d: err %.3e, torch-CPU fp32 %.3e" % (B, H, n_labels, err, cpu32))
    assert err <= 8 * cpu32, "head kernel error %.3e > 8 x the torch-CPU fp32 error %.3e" % (err, cpu32)
    assert np.array_equal(run(), got), "two calls differ"


# ------------------------------------------------------------------------ 7. drop-in
@functools.lru_cache(maxsize=None)
def _cross_encoder():
    return HipCrossEncoder(synthetic=True, config=BertConfig(layers=2), max_length=128, activation=None)


def _corpus():
    with open(os.path.join(cc.GOLDEN, "corpus_docs.json"), encoding="utf-8") as f:
        docs = json.load(f)["docs"]
    with open(os.path.join(cc.GOLDEN, "config1_queries.json"), encoding="utf-8") as f:
        return docs, json.load(f)["queries"]


def test_dropin_scores_in_the_restatement_order(require_gpu):
    g = _gold()
    docs, queries = _corpus()
    q = queries[int(g["dropin_query"])]
    texts = [docs[int(i)]["page_content"] for i in g["dropin_docs"]]
    assert len(texts) == 12 and max(len(t) for t in texts) + len(q) + 3 > 128  # some pairs are truncated
    ce = _cross_encoder()
    ref = np.asarray(g["dropin_logits64"], dtype=np.float64)
    # the fixture's logits are the restatement on the Python twin's tokens
    twin = CharTokenizer(ce.config.vocab_size, max_length=128).pairs([q] * 12, texts)
    assert float(np.abs(_oracle64(2).logits(*twin) - ref).max()) <= 1e-12
    _check(ce.logits([(q, t) for t in texts]), ref, "drop-in logits")
    scores = ce.score([(q, t) for t in texts])
    assert isinstance(scores, list) and len(scores) == 12 and all(isinstance(s, float) for s in scores)
    assert np.array_equal(np.argsort(-np.asarray(scores), kind="stable"), np.argsort(-ref[:, 0], kind="stable"))
    sig = HipCrossEncoder(synthetic=True, config=BertConfig(layers=2), max_length=128).score([(q, texts[0])])
    assert abs(sig[0] - 1 / (1 + np.exp(-ref[0, 0]))) <= 1e-5
    assert ce.score([]) == []


def test_dropin_reranker_over_a_similarity_search(require_gpu):
    docs, queries = _corpus()
    q = queries[2]
    emb = HipBertEmbeddings(synthetic=True, config=BertConfig(layers=2), max_length=128)
    store = HipChroma.from_texts([d["page_content"] for d in docs[:40]], emb)
    five = store.similarity_search(q, k=5)
    assert len(five) == 5
    ce = _cross_encoder()
    top = HipReranker(ce, top_n=3).compress_documents(five, q)
    assert len(top) == 3 and all(any(t is d for d in five) for t in top)
    scores = ce.score([(q, d.page_content) for d in five])
    want = [five[i] for i in np.argsort(-np.asarray(scores), kind="stable")[:3]]
    assert all(t is w for t, w in zip(top, want))  # best first
    # the same order as the float64 restatement's wherever its scores are a gap apart
    tok = CharTokenizer(ce.config.vocab_size, max_length=128)
    ref = _oracle64(2).logits(*tok.pairs([q] * 5, [d.page_content for d in five]))
    if cc.min_gap(ref) >= cc.MIN_GAP:
        assert [five[i] for i in np.argsort(-ref[:, 0], kind="stable")[:3]] == top


def test_long_pair_is_truncated_not_rejected(require_gpu):
    ce = _cross_encoder()
    q, long_doc = "糖尿病怎么治疗？", "二甲双胍是常用的降糖药物，需要遵医嘱服用。" * 40
    got = ce.logits([(q, long_doc), (long_doc, q)])
    tok = CharTokenizer(ce.config.vocab_size, max_length=128)
    ids, types, mask = tok.pairs([q, long_doc], [long_doc, q])
    assert ids.shape == (2, 128) and mask.all()
    _check(got, _oracle64(2).logits(ids, types, mask), "truncated pair", order=False)


# ------------------------------------------------------------------------- 8. errors
def test_score_errors(require_gpu):
    ids, types, mask = cc.pair_batch(1, 2, 16)
    cfg = BertConfig(layers=1)
    enc = Encoder(cfg)
    with pytest.raises(_lib.MQError, match="no cross-encoder head") as ei:
        enc.score(ids, types, mask)
    assert ei.value.code == -5  # MQ_ESTATE
    enc.load_head(synthetic_head_state_dict(cfg, 0))
    assert enc.score(ids, types, mask).shape == (2, 1)
    assert enc.score(ids[:0], types[:0], mask[:0]).shape == (0, 1)  # B == 0: a no-op
    L = cfg.max_positions + 1
    z = np.zeros((1, L), np.int32)
    with pytest.raises(_lib.MQError, match="exceeds max_positions") as ei:
        enc.score(z, z, z)
    assert ei.value.code == -1  # MQ_EINVAL
    with pytest.raises(ValueError, match="share one"):
        enc.score(ids, types[:, :8], mask)
    with pytest.raises(ValueError, match=r"n_labels must be in \[1, 8\]"):
        enc.load_head(synthetic_head_state_dict(cfg, 0, 9))
    mean_cfg = BertConfig(layers=1, pooling=POOL_MEAN)
    mean = Encoder(mean_cfg)
    mean.load_head(synthetic_head_state_dict(mean_cfg, 0))
    with pytest.raises(_lib.MQError, match="CLS pooling") as ei:
        mean.score(ids, types, mask)
    assert ei.value.code == -5
