"""Host logic of the cross-encoder surface (no GPU): HipReranker's ordering, the score column /
activation rules, the head tensors of a state dict, and the n_labels argument check."""
import numpy as np
import pytest

from mediquery_hip import Document, HipCrossEncoder, HipReranker, _lib
from mediquery_hip.compat import CrossEncoderBase, DocumentCompressorBase
from mediquery_hip.config import BertConfig
from mediquery_hip.cross_encoder import rerank_order, select_scores
from mediquery_hip.weights import (HEAD_NAMES, head_from_state_dict, hf_names, load_safetensors, state_dict_to_blob,
                                   blob_size, synthetic_head_state_dict, synthetic_state_dict)


class FakeScorer(CrossEncoderBase):
    def __init__(self, table):
        self.table, self.calls = table, []

    def score(self, text_pairs):
        self.calls.append(list(text_pairs))
        return [self.table[d] for _, d in text_pairs]


def _docs(names):
    return [Document(page_content=n, metadata={"i": i}) for i, n in enumerate(names)]


def test_reranker_orders_by_score_descending():
    docs = _docs("abcde")
    fake = FakeScorer({"a": 0.1, "b": 0.9, "c": 0.5, "d": 0.7, "e": 0.3})
    rr = HipReranker(fake, top_n=3)
    assert isinstance(rr, DocumentCompressorBase)
    out = rr.compress_documents(docs, "q")
    assert [d.page_content for d in out] == ["b", "d", "c"]
    assert all(any(o is d for d in docs) for o in out)  # the documents themselves, not copies
    assert fake.calls == [[("q", n) for n in "abcde"]]   # one call, (query, page_content) pairs


def test_reranker_ties_keep_input_order():
    docs = _docs("abcd")
    out = HipReranker(FakeScorer({"a": 0.5, "b": 0.7, "c": 0.5, "d": 0.7}), top_n=4).compress_documents(docs, "q")
    assert [d.page_content for d in out] == ["b", "d", "a", "c"]
    assert rerank_order([1.0, 1.0, 1.0], 2) == [0, 1]


def test_reranker_top_n_larger_than_input_and_empty_input():
    docs = _docs("ab")
    fake = FakeScorer({"a": 0.0, "b": 1.0})
    assert [d.page_content for d in HipReranker(fake, top_n=5).compress_documents(docs, "q")] == ["b", "a"]
    assert HipReranker(fake, top_n=3).compress_documents([], "q") == []
    assert len(fake.calls) == 1  # the empty input never reaches the model
    assert HipReranker(fake).top_n == 3
    with pytest.raises(ValueError, match="top_n"):
        HipReranker(fake, top_n=-1)


def test_score_column_and_activation_rules():
    one = np.array([[0.0], [2.0], [-1.0]], np.float32)
    np.testing.assert_allclose(select_scores(one, None), [0.0, 2.0, -1.0])
    np.testing.assert_allclose(select_scores(one, "sigmoid"), 1 / (1 + np.exp(-one[:, 0].astype(np.float64))))
    three = np.array([[5.0, 0.5, -3.0], [1.0, -0.5, 9.0]], np.float32)
    np.testing.assert_allclose(select_scores(three, None), [0.5, -0.5])       # column 1 past one label
    two = np.array([[5.0, 0.25]], np.float32)
    np.testing.assert_allclose(select_scores(two, None), [0.25])
    with pytest.raises(ValueError, match="activation"):
        select_scores(one, "softmax")
    with pytest.raises(ValueError, match="logits must be"):
        select_scores(np.zeros(3, np.float32))


def test_constructor_argument_errors_come_before_the_gpu():
    with pytest.raises(ValueError, match="needs the model's local files"):
        HipCrossEncoder("some/model")
    with pytest.raises(ValueError, match="no classifier"):
        HipCrossEncoder(weights_path="model.gguf", vocab_file="vocab.txt")
    with pytest.raises(ValueError, match="activation"):
        HipCrossEncoder(synthetic=True, activation="softmax")
    with pytest.raises(ValueError, match="precision"):
        HipCrossEncoder(synthetic=True, precision="fp8")
    with pytest.raises(ValueError, match="synthetic=True takes no"):
        HipCrossEncoder(synthetic=True, vocab_file="vocab.txt")


def test_synthetic_head_definition():
    cfg = BertConfig(layers=2)
    sd = synthetic_head_state_dict(cfg, seed=4, n_labels=3)
    assert tuple(sd) == HEAD_NAMES
    shapes = [(768, 768), (768,), (3, 768), (3,)]
    for i, (n, shape) in enumerate(zip(HEAD_NAMES, shapes)):
        want = 0.02 * np.random.default_rng([4, 10000 + i]).standard_normal(shape, dtype=np.float32)
        assert sd[n].dtype == np.float32 and sd[n].shape == shape
        np.testing.assert_array_equal(sd[n], want.astype(np.float32))
    assert synthetic_head_state_dict(cfg)["classifier.weight"].shape == (1, 768)
    # the encoder blob and its names are what they were: the head is a separate upload
    assert not set(HEAD_NAMES) & {n for n, _ in hf_names(cfg)}
    assert state_dict_to_blob(cfg, {**synthetic_state_dict(cfg, 0), **sd}).size == blob_size(cfg)


def test_head_from_a_safetensors_file_and_missing_key_message(tmp_path):
    from safetensors.numpy import save_file
    cfg = BertConfig(vocab_size=300, hidden=256, layers=1, heads=4, ffn=512, max_positions=64)
    head = synthetic_head_state_dict(cfg, 1, n_labels=2)
    tensors = {"bert." + k: v for k, v in synthetic_state_dict(cfg, 1).items()}
    tensors.update({"bert.pooler.dense.weight": head["pooler.dense.weight"],
                    "bert.pooler.dense.bias": head["pooler.dense.bias"],
                    "classifier.weight": head["classifier.weight"], "classifier.bias": head["classifier.bias"]})
    path = str(tmp_path / "ce.safetensors")
    save_file(tensors, path)
    sd = load_safetensors(path, cfg)
    for got, n in zip(head_from_state_dict(sd, cfg), HEAD_NAMES):
        assert got.dtype == np.float32 and got.flags["C_CONTIGUOUS"]
        np.testing.assert_array_equal(got, head[n])
    assert state_dict_to_blob(cfg, sd).size == blob_size(cfg)
    del tensors["classifier.bias"], tensors["bert.pooler.dense.weight"]
    save_file(tensors, path)
    with pytest.raises(KeyError, match="missing pooler.dense.weight, classifier.bias"):
        head_from_state_dict(load_safetensors(path, cfg), cfg)
    bad = dict(head)
    bad["classifier.weight"] = np.zeros((2, 128), np.float32)
    with pytest.raises(ValueError, match="do not fit hidden 256"):
        head_from_state_dict(bad, cfg)


@pytest.mark.parametrize("n_labels", [0, 9])
def test_n_labels_rejected_before_any_hip_call(n_labels):
    """No GPU here: the checks answer before the handle or the device is touched."""
    z = np.zeros(16, np.float32)
    p = _lib.ptr(z)
    with pytest.raises(_lib.MQError, match=r"n_labels must be in \[1, 8\]") as ei:
        _lib.call("mq_encoder_load_head", None, p, p, p, p, n_labels)
    assert ei.value.code == -1
    with pytest.raises(_lib.MQError, match=r"n_labels must be in \[1, 8\]"):
        _lib.call("mq_debug_cls_head", p, 1, 256, p, p, p, p, n_labels, p, None)
    assert _lib.MQ_HEAD_MAX_LABELS == 8
