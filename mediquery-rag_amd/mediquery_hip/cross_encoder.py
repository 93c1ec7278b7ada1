"""`HipCrossEncoder` / `HipReranker` - cross-encoder reranking on the HIP BERT encoder.

The reference's Retrieve node takes `vectorstore.similarity_search(q, k=5)`
(src/agents/nodes.py:93) and its Grade step reads only the first two documents
(src/core/utils.py:64), so the order of the results decides what the LLM sees.  A bi-encoder
ranks by one CLS vector per text; a cross-encoder reads query and document together:
`[CLS] query [SEP] document [SEP]` through BERT, then BertPooler and a classifier
(transformers' BertForSequenceClassification).  LangChain's shape for it is
    CrossEncoderReranker(model=HuggingFaceCrossEncoder(...), top_n=3)
and these two classes have that surface:
    reranker = HipReranker(HipCrossEncoder(weights_path=..., vocab_file=...), top_n=3)
    docs = reranker.compress_documents(vectorstore.similarity_search(q, k=20), q)
The forward is the embedding encoder's (libmqhip.so, mq_encoder_score) with segment ids and an
un-normalised CLS tail, followed by the head kernel (K13); nothing here scores on the CPU.

Weights are resolved as HipBertEmbeddings resolves safetensors weights: `weights_path` +
`vocab_file` (or $MQ_RERANKER_WEIGHTS_PATH + $MQ_RERANKER_VOCAB_FILE), a local
BertForSequenceClassification checkpoint and its vocab.txt; nothing is downloaded.
`synthetic=True` asks for seeded random weights, head and the char tokenizer (tests,
benchmarks).  GGUF files carry no classifier and are not accepted.
"""
import os

import numpy as np

from .compat import CrossEncoderBase, DocumentCompressorBase
from .config import BertConfig, DMETA_BASE
from .embeddings import DEFAULT_PRECISION, ENV_PRECISION, PRECISIONS
from .weights import head_from_state_dict, load_safetensors, synthetic_head_state_dict

ENV_WEIGHTS = "MQ_RERANKER_WEIGHTS_PATH"
ENV_VOCAB = "MQ_RERANKER_VOCAB_FILE"
ACTIVATIONS = ("sigmoid", None)


def select_scores(logits, activation="sigmoid"):
    """[n, n_labels] logits -> [n] scores as HuggingFaceCrossEncoder / sentence-transformers
    report them: column 0 of a one-label head, column 1 of a larger one, then `activation`
    ("sigmoid" or None) on the host."""
    if activation not in ACTIVATIONS:
        raise ValueError("activation must be 'sigmoid' or None, got %r" % (activation,))
    logits = np.asarray(logits, dtype=np.float32)
    if logits.ndim != 2 or logits.shape[1] < 1:
        raise ValueError("logits must be [n, n_labels >= 1], got shape %s" % (logits.shape,))
    x = logits[:, 0 if logits.shape[1] == 1 else 1].astype(np.float64)
    if activation == "sigmoid":
        x = 1.0 / (1.0 + np.exp(-x))
    return x


class HipCrossEncoder(CrossEncoderBase):
    """BERT cross-encoder scored by the hand-written HIP encoder (module doc).

    model:        a name for logs only (nothing is resolved from it).
    weights_path: local safetensors of a BertForSequenceClassification checkpoint.
    vocab_file:   its WordPiece vocab.txt.
    synthetic:    True = seeded random encoder + head (`seed`, `n_labels`) + char tokenizer.
    batch_size:   pairs per forward (length-sorted batches).
    precision:    "f32x6" (default; $MQ_ENCODER_PRECISION) or "f32", as HipBertEmbeddings.
    activation:   "sigmoid" (default) or None, applied by `score` on the host.
    """

    def __init__(self, model=None, *, weights_path=None, vocab_file=None, synthetic=False,
                 config: BertConfig = None, seed=0, device=0, batch_size=32, max_length=512,
                 precision=None, activation="sigmoid", n_labels=1):
        from .native import Encoder
        from .tokenizer import NativeTokenizer
        precision = precision or os.environ.get(ENV_PRECISION) or DEFAULT_PRECISION
        if precision not in PRECISIONS:
            raise ValueError("precision must be one of %s, got %r" % (sorted(PRECISIONS), precision))
        if activation not in ACTIVATIONS:
            raise ValueError("activation must be 'sigmoid' or None, got %r" % (activation,))
        self.model, self.device, self.precision, self.activation = model, device, precision, activation
        self.batch_size = int(batch_size)
        self.synthetic = bool(synthetic)
        if self.synthetic:
            if weights_path or vocab_file:
                raise ValueError("synthetic=True takes no weights_path / vocab_file")
            config = config or DMETA_BASE
            weights, head = None, synthetic_head_state_dict(config, seed, n_labels)
        else:
            weights_path = weights_path or os.environ.get(ENV_WEIGHTS)
            vocab_file = vocab_file or os.environ.get(ENV_VOCAB)
            if weights_path and str(weights_path).endswith(".gguf"):
                raise ValueError("GGUF files carry no classifier head: pass a safetensors checkpoint")
            if not weights_path or not vocab_file:
                raise ValueError(
                    "HipCrossEncoder(model=%r) needs the model's local files (nothing is downloaded): "
                    "weights_path= + vocab_file= (or $%s + $%s). Missing: %s. Pass synthetic=True for "
                    "seeded random weights (tests/benchmarks only)."
                    % (model, ENV_WEIGHTS, ENV_VOCAB,
                       ", ".join(n for n, v in (("weights", weights_path), ("vocab", vocab_file)) if not v)))
            for what, p in (("weights", weights_path), ("vocab", vocab_file)):
                if not os.path.isfile(p):
                    raise FileNotFoundError("%s file %r does not exist" % (what, p))
            config = config or DMETA_BASE
            weights = load_safetensors(weights_path, config)
            head_from_state_dict(weights, config)  # a clear KeyError before the GPU is touched
            head = weights
        self.config = config
        self.max_length = min(int(max_length), config.max_positions)
        self.weights_path, self.vocab_file = weights_path, vocab_file
        self.encoder = Encoder(config, weights=weights, seed=seed, device=device)
        self.encoder.set_precision(PRECISIONS[precision])
        self.encoder.load_head(head)
        self.n_labels = self.encoder.n_labels
        if vocab_file:
            self.tokenizer = NativeTokenizer.wordpiece(vocab_file, max_length=self.max_length)
        else:
            self.tokenizer = NativeTokenizer.char(config.vocab_size, max_length=self.max_length)

    def logits(self, pairs):
        """(query, document) string pairs -> float32 [n, n_labels]; length-sorted batches cut
        padding.  A pair longer than max_length is truncated (longest first)."""
        pairs = [tuple(p) for p in pairs]
        out = np.empty((len(pairs), self.n_labels), dtype=np.float32)
        if not pairs:
            return out
        ids, types, mask = self.tokenizer.pairs([p[0] for p in pairs], [p[1] for p in pairs])
        lens = mask.sum(1)
        order = np.argsort(lens, kind="stable")
        for s in range(0, len(order), self.batch_size):
            idx = order[s:s + self.batch_size]
            L = int(lens[idx].max())
            out[idx] = self.encoder.score(np.ascontiguousarray(ids[idx, :L]), np.ascontiguousarray(types[idx, :L]),
                                          np.ascontiguousarray(mask[idx, :L]))
        return out

    # ---- LangChain BaseCrossEncoder interface ---------------------------------------
    def score(self, text_pairs):
        return select_scores(self.logits(text_pairs), self.activation).tolist()


def rerank_order(scores, top_n):
    """Indices of the top_n scores, descending, ties in input order."""
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    return np.argsort(-scores, kind="stable")[:max(0, int(top_n))].tolist()


class HipReranker(DocumentCompressorBase):
    """LangChain's CrossEncoderReranker: `compress_documents(documents, query)` returns the
    top_n documents by `model.score([(query, doc.page_content), ...])`, best first, ties in
    input order - the documents themselves, not copies.  `model`: anything with a
    BaseCrossEncoder `score(text_pairs) -> list[float]`, e.g. HipCrossEncoder.  Use it
    directly after a search, or as `ContextualCompressionRetriever(base_compressor=...)`."""

    def __init__(self, model, top_n=3):
        super().__init__()
        if int(top_n) < 0:
            raise ValueError("top_n must be >= 0 (got %r)" % (top_n,))
        self.model = model
        self.top_n = int(top_n)

    def compress_documents(self, documents, query, callbacks=None):
        documents = list(documents)
        if not documents:
            return []
        scores = self.model.score([(query, d.page_content) for d in documents])
        if len(scores) != len(documents):
            raise ValueError("the model returned %d scores for %d documents" % (len(scores), len(documents)))
        return [documents[i] for i in rerank_order(scores, self.top_n)]
