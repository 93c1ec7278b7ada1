"""LangChain interop: subclass the real base classes when langchain_core is
importable, otherwise provide duck-typed stand-ins with the same surface (the
reference's own environment has langchain_core; this image does not)."""
import asyncio

try:  # pragma: no cover - exercised only where langchain_core is installed
    from langchain_core.documents import Document  # type: ignore
    from langchain_core.embeddings import Embeddings as EmbeddingsBase  # type: ignore
    from langchain_core.vectorstores import VectorStore as VectorStoreBase  # type: ignore
    HAVE_LANGCHAIN = True
except Exception:
    HAVE_LANGCHAIN = False

    class Document:
        """Minimal langchain_core.documents.Document: page_content + metadata (+ id)."""

        def __init__(self, page_content, metadata=None, id=None, **kwargs):
            self.page_content = page_content
            self.metadata = dict(metadata or {})
            self.id = id
            self.type = "Document"

        def __eq__(self, other):
            return (isinstance(other, Document) and self.page_content == other.page_content
                    and self.metadata == other.metadata)

        def __repr__(self):
            return "Document(page_content=%r, metadata=%r)" % (self.page_content[:40], self.metadata)

    class EmbeddingsBase:
        def embed_documents(self, texts):
            raise NotImplementedError

        def embed_query(self, text):
            raise NotImplementedError

        async def aembed_documents(self, texts):
            return await asyncio.get_running_loop().run_in_executor(None, self.embed_documents, texts)

        async def aembed_query(self, text):
            return await asyncio.get_running_loop().run_in_executor(None, self.embed_query, text)

    class VectorStoreBase:
        def add_documents(self, documents, **kwargs):
            texts = [d.page_content for d in documents]
            metadatas = [d.metadata for d in documents]
            if "ids" not in kwargs:
                ids = [getattr(d, "id", None) for d in documents]
                if all(ids):
                    kwargs["ids"] = ids
            return self.add_texts(texts, metadatas, **kwargs)

        @classmethod
        def from_documents(cls, documents, embedding, **kwargs):
            texts = [d.page_content for d in documents]
            metadatas = [d.metadata for d in documents]
            return cls.from_texts(texts, embedding, metadatas=metadatas, **kwargs)

        def as_retriever(self, **kwargs):
            search_kwargs = kwargs.get("search_kwargs", {})
            k = search_kwargs.get("k", 4)
            store = self
            # search_type="mmr" (LangChain's VectorStoreRetriever): k, fetch_k, lambda_mult,
            # filter and where_document of search_kwargs go to max_marginal_relevance_search;
            # the plain type passes filter and where_document on too, as LangChain's does
            mmr = kwargs.get("search_type") == "mmr"
            mmr_kwargs = {a: search_kwargs[a] for a in ("k", "fetch_k", "lambda_mult", "filter", "where_document")
                          if a in search_kwargs}
            sim_kwargs = {a: search_kwargs[a] for a in ("filter", "where_document") if a in search_kwargs}
            # search_type="similarity_score_threshold": score_threshold, k, filter and
            # where_document go to similarity_search_with_relevance_scores; a missing or
            # non-float threshold is refused here, as LangChain's retriever refuses it
            thresh = kwargs.get("search_type") == "similarity_score_threshold"
            thresh_kwargs = {a: search_kwargs[a] for a in ("score_threshold", "k", "filter", "where_document")
                             if a in search_kwargs}
            if thresh and not isinstance(search_kwargs.get("score_threshold"), float):
                raise ValueError("`score_threshold` is not specified with a float value(0~1) in `search_kwargs`.")

            class _Retriever:
                def invoke(self, query, **_):
                    if mmr:
                        return store.max_marginal_relevance_search(query, **mmr_kwargs)
                    if thresh:
                        return [d for d, _ in store.similarity_search_with_relevance_scores(query, **thresh_kwargs)]
                    return store.similarity_search(query, k=k, **sim_kwargs)

                get_relevant_documents = invoke

            return _Retriever()


# Cross-encoder reranking (langchain_community.cross_encoders.BaseCrossEncoder,
# langchain_core.documents.BaseDocumentCompressor): the real classes when importable, else
# stand-ins with the same surface.
try:  # pragma: no cover - exercised only where langchain is installed
    from langchain_community.cross_encoders import BaseCrossEncoder as CrossEncoderBase  # type: ignore
except Exception:
    class CrossEncoderBase:
        def score(self, text_pairs):
            raise NotImplementedError

try:  # pragma: no cover
    from langchain_core.documents import BaseDocumentCompressor as _PydanticCompressor  # type: ignore

    class DocumentCompressorBase(_PydanticCompressor):
        """LangChain's compressor base (a pydantic model) accepting plain attributes."""
        model_config = {"arbitrary_types_allowed": True, "extra": "allow"}
except Exception:
    class DocumentCompressorBase:
        def compress_documents(self, documents, query, callbacks=None):
            raise NotImplementedError

        async def acompress_documents(self, documents, query, callbacks=None):
            return await asyncio.get_running_loop().run_in_executor(
                None, self.compress_documents, documents, query, callbacks)
