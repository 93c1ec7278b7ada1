"""The cross-encoder restatement (tests/cross_encoder_cases.py) against the
transformers.BertForSequenceClassification fixtures, and the ranking inputs' float64 gaps."""
import numpy as np
import pytest
import torch

import cross_encoder_cases as cc


@pytest.fixture(scope="module")
def gold():
    return cc.load_golden()


@pytest.mark.parametrize("name,layers,labels", [("tiny", 2, 1), ("tiny3", 2, 3), ("base", 12, 1)])
def test_restatement_matches_hf(gold, name, layers, labels):
    ids, types, mask = (gold[name + s] for s in ("_ids", "_types", "_mask"))
    ref = gold[name + "_logits"]
    assert ref.shape == (ids.shape[0], labels)
    assert types.max() == 1 and (mask.sum(1) < ids.shape[1]).any()  # segments and ragged padding present
    got = cc.oracle(layers, torch.float32, labels).logits(ids, types, mask)
    err = float(np.abs(got - ref).max())
    assert err <= 1e-6, "restatement vs HF %s: max error %.3g" % (name, err)


def test_golden_cases_are_the_generators(gold):
    for name, seed, B, L in (("tiny", 1, 6, 48), ("tiny3", 1, 6, 48), ("base", 2, 2, 32)):
        for got, want in zip(cc.pair_batch(seed, B, L), (gold[name + s] for s in ("_ids", "_types", "_mask"))):
            np.testing.assert_array_equal(got, want)


def test_pair_batch_layout():
    ids, types, mask = cc.pair_batch(3, 7, 21)
    assert ids.shape == types.shape == mask.shape == (7, 21)
    qn = int(np.argmax(ids[0] == cc.SEP)) - 1
    assert 3 <= qn <= 11
    for b in range(7):
        n = int(mask[b].sum())
        assert (mask[b, :n] == 1).all() and (ids[b, n:] == 0).all() and (types[b, n:] == 0).all()
        assert ids[b, 0] == cc.CLS and ids[b, qn + 1] == cc.SEP and ids[b, n - 1] == cc.SEP
        np.testing.assert_array_equal(ids[b, 1:qn + 1], ids[0, 1:qn + 1])  # one shared query
        assert (types[b, :qn + 2] == 0).all() and (types[b, qn + 2:n] == 1).all() and n - qn - 3 >= 1
        assert (ids[b, 1:qn + 1] >= 106).all() and (ids[b, qn + 2:n - 1] >= 106).all()


@pytest.mark.parametrize("layers,B,L", cc.RANK_CASES)
def test_ranking_inputs_have_a_float64_gap(gold, layers, B, L):
    ids, types, mask, ref = cc.ranking_case(layers, B, L, gold)
    again = cc.oracle(layers, torch.float64).logits(ids, types, mask)
    assert float(np.abs(again - ref).max()) <= 1e-12  # the recorded logits are the restatement's
    gap = cc.min_gap(ref)
    assert gap >= cc.MIN_GAP, "smallest float64 gap %.3g" % gap
    # float32 restatement: far inside the end-to-end tolerance
    e32 = float(np.abs(cc.oracle(layers, torch.float32).logits(ids, types, mask) - ref).max())
    assert e32 <= cc.LOGIT_TOL / 3, "fp32 restatement error %.3g" % e32


def test_segment_ids_matter(gold):
    ids, types, mask, ref = cc.ranking_case(2, 9, 130, gold)
    zero = cc.oracle(2, torch.float64).logits(ids, np.zeros_like(types), mask)
    assert float(np.abs(zero - ref).min()) > 1e-3


def test_dropin_inputs_have_a_float64_gap(gold):
    assert cc.min_gap(gold["dropin_logits64"]) >= cc.MIN_GAP and len(gold["dropin_docs"]) == 12
