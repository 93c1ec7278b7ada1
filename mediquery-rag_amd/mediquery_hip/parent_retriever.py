"""`HipParentDocumentRetriever` - LangChain's `ParentDocumentRetriever` on the store's grouped
search: small child chunks are embedded, the parent documents are returned.

LangChain's retriever searches the top-k CHILDREN and keeps their distinct parents, so several
children of one parent crowd the list and k = 5 regularly yields two or three parents.  Here
`k` counts parents: `HipChroma.similarity_search_grouped` returns the best child of each of the
top-k distinct `id_key` values over the whole store (include/mq.h, "Grouped search"), and the
docstore maps them back.
"""
import uuid

from .compat import Document


class WindowSplitter:
    """Character windows of `chunk_size` every `chunk_size - chunk_overlap` characters; each
    chunk copies its document's metadata.  The last window ends at the text's end; a text of at
    most chunk_size characters is one chunk, an empty text none."""

    def __init__(self, chunk_size=200, chunk_overlap=0):
        chunk_size, chunk_overlap = int(chunk_size), int(chunk_overlap)
        if chunk_size < 1:
            raise ValueError("chunk_size must be at least 1 (got %d)" % chunk_size)
        if not 0 <= chunk_overlap < chunk_size:
            raise ValueError("chunk_overlap must be in [0, chunk_size) (got %d with chunk_size %d)"
                             % (chunk_overlap, chunk_size))
        self.chunk_size, self.chunk_overlap = chunk_size, chunk_overlap

    def split_text(self, text):
        step = self.chunk_size - self.chunk_overlap
        out, start = [], 0
        while start < len(text):
            out.append(text[start:start + self.chunk_size])
            if start + self.chunk_size >= len(text):
                break
            start += step
        return out

    def split_documents(self, documents):
        return [Document(page_content=chunk, metadata=dict(d.metadata))
                for d in documents for chunk in self.split_text(d.page_content)]


class InMemoryDocstore:
    """The default docstore: a dict behind LangChain's `mset` / `mget` (a missing key gets None)."""

    def __init__(self):
        self.store = {}

    def mset(self, key_value_pairs):
        for key, value in key_value_pairs:
            self.store[key] = value

    def mget(self, keys):
        return [self.store.get(key) for key in keys]


class HipParentDocumentRetriever:
    """`add_documents(parents)` splits each parent with `child_splitter.split_documents` (any
    object with that method; None: the parents are their own children), tags the children with
    `id_key`, adds them to the vectorstore and stores the parents in the docstore;
    `invoke(query)` returns the parents of the top-k distinct `id_key` values, best first.
    search_kwargs go to `similarity_search_grouped` (k, filter, where_document); k counts
    parents."""

    def __init__(self, vectorstore, docstore=None, id_key="doc_id", child_splitter=None, search_kwargs=None):
        self.vectorstore = vectorstore
        self.docstore = InMemoryDocstore() if docstore is None else docstore
        self.id_key = id_key
        self.child_splitter = child_splitter
        self.search_kwargs = dict(search_kwargs or {})

    def add_documents(self, documents, ids=None, **kwargs):
        documents = list(documents)
        if ids is None:
            ids = [str(uuid.uuid4()) for _ in documents]
        ids = list(ids)
        if len(ids) != len(documents):
            raise ValueError("got %d ids for %d documents" % (len(ids), len(documents)))
        children = []
        for doc, doc_id in zip(documents, ids):
            subs = [doc] if self.child_splitter is None else self.child_splitter.split_documents([doc])
            for sub in subs:
                meta = dict(sub.metadata)
                meta[self.id_key] = doc_id
                children.append(Document(page_content=sub.page_content, metadata=meta))
        if children:
            self.vectorstore.add_documents(children, **kwargs)
        self.docstore.mset(list(zip(ids, documents)))
        return ids

    def invoke(self, query, config=None, **kwargs):
        children = self.vectorstore.similarity_search_grouped(query, group_by=self.id_key, **self.search_kwargs)
        parents = self.docstore.mget([c.metadata[self.id_key] for c in children])
        return [p for p in parents if p is not None]

    get_relevant_documents = invoke
