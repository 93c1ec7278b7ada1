"""Pair tokenisation ([CLS] A [SEP] B [SEP], mq_tokenizer_encode_pairs): the native tokenizer,
its Python twins and BertTokenizerFast's recorded encodings (pair_tokenizer_golden.json) agree."""
import ctypes
import json
import os

import numpy as np
import pytest

from mediquery_hip import _lib
from mediquery_hip.tokenizer import CharTokenizer, NativeTokenizer, WordPieceTokenizer, pair_budget

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VOCAB = os.path.join(GOLDEN, "wordpiece_vocab.txt")


def _same(a, b):
    assert len(a) == len(b) == 3
    for x, y in zip(a, b):
        assert x.dtype == y.dtype == np.int32
        np.testing.assert_array_equal(x, y)


def test_wordpiece_native_equals_twin_equals_hf():
    with open(os.path.join(GOLDEN, "pair_tokenizer_golden.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    assert {c["max_length"] for c in cases} == {8, 9, 16, 17, 30}
    branches = set()
    for ml in sorted({c["max_length"] for c in cases}):
        sub = [c for c in cases if c["max_length"] == ml]
        nat = NativeTokenizer.wordpiece(VOCAB, max_length=ml)
        twin = WordPieceTokenizer(VOCAB, max_length=ml)
        firsts, seconds = [c["first"] for c in sub], [c["second"] for c in sub]
        got = nat.pairs(firsts, seconds)
        _same(got, twin.pairs(firsts, seconds))
        ids, types, mask = got
        for i, c in enumerate(sub):
            n = len(c["ids"])
            assert n <= ml and int(mask[i].sum()) == n, (ml, i)
            assert ids[i, :n].tolist() == c["ids"], (ml, c["first"], c["second"])
            assert types[i, :n].tolist() == c["types"]
            assert not ids[i, n:].any() and not types[i, n:].any()
            a, b = len(twin.body(c["first"])), len(twin.body(c["second"]))
            T = ml - 3
            branches.add("none" if a + b <= T else "short_kept" if 2 * min(a, b) <= T else
                         "equal" if a == b else "both_odd" if T % 2 else "both_even")
    assert branches == {"none", "short_kept", "equal", "both_odd", "both_even"}, branches


def test_pair_budget_rule():
    assert pair_budget(2, 3, 8) == (2, 3)
    assert pair_budget(1, 40, 16) == (1, 12) and pair_budget(40, 1, 16) == (12, 1)
    assert pair_budget(9, 9, 16) == (6, 7)       # equal: the first is "the shorter"
    assert pair_budget(10, 9, 16) == (7, 6) and pair_budget(9, 10, 16) == (6, 7)
    assert pair_budget(9, 9, 17) == (7, 7)


@pytest.mark.parametrize("max_length", [5, 12, 64])
def test_char_native_equals_twin(max_length):
    nat = NativeTokenizer.char(21128, max_length=max_length)
    twin = CharTokenizer(21128, max_length=max_length)
    firsts = ["糖尿病 怎么 治疗", "", "hello world", "2型糖尿病的饮食控制方法有哪些，应该注意什么？", "a", "高血压" * 30]
    seconds = ["二甲双胍是常用药物。", "只有第二段", "", "短", "b" * 200, "低盐饮食" * 25]
    for pad_to in (None, max_length + 3, 7):
        got = nat.pairs(firsts, seconds, pad_to=pad_to)
        _same(got, twin.pairs(firsts, seconds, pad_to=pad_to))
        ids, types, mask = got
        assert ids.shape[1] <= max(max_length, pad_to or 0) and (pad_to is None or ids.shape[1] >= pad_to)
        for i in range(len(firsts)):
            n = int(mask[i].sum())
            assert 3 <= n <= max_length and ids[i, 0] == 101 and ids[i, n - 1] == 102
            seps = np.flatnonzero(ids[i, :n] == 102)
            assert len(seps) == 2  # also for an empty second text: its type-1 [SEP] stays
            assert (types[i, :seps[0] + 1] == 0).all() and (types[i, seps[0] + 1:n] == 1).all()
            assert types[i, n - 1] == 1 and not ids[i, n:].any() and not types[i, n:].any()
    # empty second text: [CLS] A [SEP] [SEP]
    ids, types, mask = nat.pairs(["ab"], [""])
    assert ids[0].tolist()[:1] == [101] and ids[0, -2:].tolist() == [102, 102] and types[0, -2:].tolist() == [0, 1]
    # empty first text
    ids, types, mask = nat.pairs([""], ["ab"])
    assert ids[0, :2].tolist() == [101, 102] and types[0].tolist()[:3] == [0, 0, 1]


def test_empty_batch():
    nat = NativeTokenizer.char(21128, max_length=16)
    ids, types, mask = nat.pairs([], [])
    assert ids.shape[0] == types.shape[0] == mask.shape[0] == 0
    _same(nat.pairs([], [], pad_to=4), CharTokenizer(21128, 16).pairs([], [], pad_to=4))


def test_bad_arguments_raise_with_message():
    nat = NativeTokenizer.char(21128, max_length=4)
    with pytest.raises(_lib.MQError, match="max_length >= 5"):
        nat.pairs(["a"], ["b"])
    with pytest.raises(ValueError, match="max_length >= 5"):
        CharTokenizer(21128, max_length=4).pairs(["a"], ["b"])
    ok = NativeTokenizer.char(21128, max_length=16)
    with pytest.raises(ValueError, match="2 first texts, 1 second"):
        ok.pairs(["a", "b"], ["c"])
    with pytest.raises(ValueError, match="2 first texts, 1 second"):
        CharTokenizer(21128, 16).pairs(["a", "b"], ["c"])
    L = ctypes.c_int()
    with pytest.raises(_lib.MQError, match="bad encode_pairs arguments"):
        _lib.call("mq_tokenizer_encode_pairs", ok._h, None, None, 1, 0, None, None, None, ctypes.byref(L))
    with pytest.raises(_lib.MQError, match="bad encode_pairs arguments"):
        _lib.call("mq_tokenizer_encode_pairs", None, None, None, 0, 0, None, None, None, ctypes.byref(L))
