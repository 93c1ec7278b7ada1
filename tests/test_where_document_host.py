"""`where_document` on the host: `_match_document`, the row-by-row definition of Chroma's
document filter ($contains / $not_contains / $and / $or), its validation, and the argument
checks of mq_mask_contains that come before any HIP call (no GPU needed)."""
import ctypes

import pytest

from mediquery_hip import _lib
from mediquery_hip.vectorstore import HipChroma, _check_where_document, _match_document

ZH = "二甲双胍是治疗2型糖尿病的一线药物。"
EN = "Metformin is the first-line drug for type 2 diabetes."


@pytest.mark.parametrize("text,clause,want", [
    (ZH, {"$contains": "糖尿病"}, True),
    (ZH, {"$contains": "高血压"}, False),
    (ZH, {"$contains": "2型"}, True),
    (ZH, {"$contains": ZH}, True),                 # the whole row
    (ZH, {"$contains": ZH + "。"}, False),          # longer than the row
    (ZH, {"$not_contains": "高血压"}, True),
    (ZH, {"$not_contains": "二甲双胍"}, False),
    (EN, {"$contains": "Metformin"}, True),
    (EN, {"$contains": "metformin"}, False),       # case-sensitive
    (EN, {"$contains": "first-line drug"}, True),
    (EN, {"$contains": "first line"}, False),      # no tokenisation
    (EN, {"$not_contains": "insulin"}, True),
    ("aaab", {"$contains": "aab"}, True),          # self-overlapping pattern
    ("", {"$contains": "a"}, False),
    ("", {"$not_contains": "a"}, True),
    (ZH, {"$and": [{"$contains": "糖尿病"}, {"$contains": "一线"}]}, True),
    (ZH, {"$and": [{"$contains": "糖尿病"}, {"$contains": "胰岛素"}]}, False),
    (ZH, {"$or": [{"$contains": "胰岛素"}, {"$contains": "一线"}]}, True),
    (ZH, {"$or": [{"$contains": "胰岛素"}, {"$contains": "高血压"}]}, False),
    (ZH, {"$and": [{"$contains": "糖尿病"}]}, True),   # a one-clause list
    (EN, {"$and": [{"$or": [{"$contains": "insulin"}, {"$contains": "Metformin"}]},
                   {"$not_contains": "type 1"}]}, True),
    (EN, {"$or": [{"$and": [{"$contains": "Metformin"}, {"$contains": "type 1"}]},
                  {"$not_contains": "drug"}]}, False),
])
def test_match_document_truth(text, clause, want):
    assert _match_document(text, clause) is want


def test_nfc_and_nfd_are_different_bytes():
    """No Unicode normalisation: a precomposed e-acute does not match e + combining accent."""
    assert _match_document("caf\u00e9", {"$contains": "\u00e9"})
    assert not _match_document("caf\u00e9", {"$contains": "e\u0301"})


@pytest.mark.parametrize("clause,part", [
    ({"$regex": "a.*"}, r"\$regex"),
    ({"$not_regex": "a"}, r"\$not_regex"),
    ({"$eq": "a"}, r"\$eq"),
    ({"contains": "a"}, "contains"),
    ({"$contains": 3}, "non-empty str"),
    ({"$contains": b"a"}, "non-empty str"),
    ({"$contains": None}, "non-empty str"),
    ({"$contains": ""}, "non-empty str"),
    ({"$not_contains": ""}, "non-empty str"),
    ({"$and": []}, "non-empty list"),
    ({"$or": []}, "non-empty list"),
    ({"$and": {"$contains": "a"}}, "non-empty list"),
    ({}, "exactly one key"),
    ({"$contains": "a", "$not_contains": "b"}, "exactly one key"),
    ("糖尿病", "exactly one key"),
    ({"$and": [{"$contains": "a"}, {}]}, r"\[1\]"),                 # names the nested part
    ({"$or": [{"$contains": "a"}, {"$and": [{"$regex": "x"}]}]}, r"\$regex"),
    ({"$contains": "a" * 257}, "MQ_CONTAINS_MAX_BYTES"),
    ({"$contains": "糖" * 86}, "258 UTF-8 bytes"),                   # counted in bytes
])
def test_invalid_clauses_raise(clause, part):
    with pytest.raises(ValueError, match=part):
        _check_where_document(clause)
    with pytest.raises(ValueError, match=part):
        _match_document("abc", clause)


def test_pattern_length_limit_is_256_bytes():
    assert _lib.MQ_CONTAINS_MAX_BYTES == 256
    assert not _match_document("abc", {"$contains": "a" * 256})
    assert _match_document("a" * 300, {"$contains": "a" * 256})
    assert not _match_document("abc", {"$contains": "糖" * 85})    # 255 bytes
    with pytest.raises(ValueError, match="257 UTF-8 bytes"):
        _match_document("abc", {"$contains": "a" * 257})


def test_store_validates_before_any_device_work():
    """Every search method and get() refuse a bad clause at once: on an empty store, with no
    index and no GPU, nothing else could raise."""
    store = HipChroma(dim=64, auto_persist=False)
    bad = {"$regex": "a"}
    vec = [0.0] * 64
    for call in (lambda: store.similarity_search_by_vector(vec, where_document=bad),
                 lambda: store.similarity_search_by_vector_with_score(vec, where_document=bad),
                 lambda: store.similarity_search("q", where_document=bad),
                 lambda: store.similarity_search_with_score("q", where_document=bad),
                 lambda: store.similarity_search_with_cosine("q", where_document=bad),
                 lambda: store.similarity_search_with_relevance_scores("q", where_document=bad),
                 lambda: store.similarity_search_batch(["q"], where_document=bad),
                 lambda: store.max_marginal_relevance_search_by_vector(vec, where_document=bad),
                 lambda: store.max_marginal_relevance_search("q", where_document=bad),
                 lambda: store.max_marginal_relevance_search_batch(["q"], where_document=bad),
                 lambda: store.get(where_document=bad),
                 lambda: store.get(where_document={})):
        with pytest.raises(ValueError, match="where_document"):
            call()
    assert store._doc_mirror is None
    assert store.get(where_document={"$contains": "a"}) == {"ids": [], "documents": [], "metadatas": []}
    assert store.similarity_search_by_vector(vec, where_document={"$contains": "a"}) == []


def _contains(text, text_bytes, offsets, n, pattern, plen, negate, bits, mode, scratch):
    return _lib.call("mq_mask_contains", text, text_bytes, offsets, n, pattern, plen, negate, bits, mode,
                     scratch, None)


def test_mask_contains_bad_arguments_raise_with_message():
    """The checks come before any HIP call: they answer without a GPU (the non-NULL pointers
    below are host arrays the call never gets to touch)."""
    buf, buf2 = (ctypes.c_uint8 * 96)(), (ctypes.c_uint8 * 96)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    other = ctypes.c_void_p((ctypes.addressof(buf2) + 15) & ~15)
    for plen in (0, -1, 257):
        with pytest.raises(_lib.MQError, match="pattern_len must be in"):
            _contains(p, 16, p, 1, b"a", plen, 0, p, _lib.MQ_MASK_SET, other)
    with pytest.raises(_lib.MQError, match="NULL pattern"):
        _contains(p, 16, p, 1, None, 1, 0, p, _lib.MQ_MASK_SET, other)
    with pytest.raises(_lib.MQError, match="bad mask mode"):
        _contains(p, 16, p, 1, b"a", 1, 0, p, _lib.MQ_MASK_CLEAR, other)
    with pytest.raises(_lib.MQError, match="bad mask mode"):
        _contains(p, 16, p, 1, b"a", 1, 0, p, -1, other)
    with pytest.raises(_lib.MQError, match="negate must be 0 or 1"):
        _contains(p, 16, p, 1, b"a", 1, 2, p, _lib.MQ_MASK_SET, other)
    with pytest.raises(_lib.MQError, match="negative size"):
        _contains(p, 16, p, -1, b"a", 1, 0, p, _lib.MQ_MASK_SET, other)
    with pytest.raises(_lib.MQError, match="negative size"):
        _contains(p, -16, p, 1, b"a", 1, 0, p, _lib.MQ_MASK_SET, other)
    for args in ((None, 16, p, 1, b"a", 1, 0, p, _lib.MQ_MASK_SET, other),     # text
                 (p, 16, None, 1, b"a", 1, 0, p, _lib.MQ_MASK_SET, other),     # offsets
                 (p, 16, p, 1, b"a", 1, 0, None, _lib.MQ_MASK_SET, other),     # bits
                 (p, 16, p, 1, b"a", 1, 0, p, _lib.MQ_MASK_SET, None)):        # scratch
        with pytest.raises(_lib.MQError, match="NULL buffer") as e:
            _contains(*args)
        assert e.value.code == -1  # MQ_EINVAL
    with pytest.raises(_lib.MQError, match="scratch must not be bits"):
        _contains(p, 16, p, 1, b"a", 1, 0, p, _lib.MQ_MASK_SET, p)
    with pytest.raises(_lib.MQError, match="16-byte aligned"):
        _contains(ctypes.c_void_p(p.value + 1), 16, p, 1, b"a", 1, 0, p, _lib.MQ_MASK_SET, other)
    # n == 0 is a no-op, whatever the pointers are
    assert _contains(None, 0, None, 0, b"a", 1, 0, None, _lib.MQ_MASK_SET, None) == _lib.MQ_OK
    # ... but its scalar arguments are still checked
    with pytest.raises(_lib.MQError, match="pattern_len must be in"):
        _contains(None, 0, None, 0, b"a", 0, 0, None, _lib.MQ_MASK_SET, None)
