"""The grouped search on the host: every argument check of mq_index_search_grouped answers
MQ_EINVAL and names the offending value before any HIP call (no GPU needed), the scratch size
is monotone and bounded in nq, and WindowSplitter / HipParentDocumentRetriever keep their
books against a fake store.

Without a GPU no index handle can be made, so the checks that need the index's shape are
reached through mq_debug_group_check, which runs the same function on a stated (dim, rows);
the checks of the scalars come before the handle is looked at and are reached directly."""
import ctypes

import numpy as np
import pytest

from mediquery_hip import Document, HipParentDocumentRetriever, WindowSplitter, _lib
from mediquery_hip.native import group_scan_blocks, group_scratch_bytes
from mediquery_hip.parent_retriever import InMemoryDocstore

EINVAL = -1


def _aligned(nbytes):
    buf = (ctypes.c_uint8 * (nbytes + 64))()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)


def _check(dim=64, n=10, queries=True, nq=1, k=5, codes=True, n_groups=3, out_s=True, out_i=True, scratch=True,
           scratch_bytes=None, scratch_off=0):
    """mq_debug_group_check with sound defaults; True = a valid host buffer of its own."""
    keep = []

    def buf(flag, nbytes):
        if flag is not True:
            return flag
        b, p = _aligned(nbytes)
        keep.append(b)
        return p
    need = group_scratch_bytes(n_groups, nq, k)
    small = min(max(1, nq), 64)  # nothing is read: a refused call needs no room for 2^24 queries
    s = buf(scratch, need + 64)
    if s is not None and scratch_off:
        s = ctypes.c_void_p(s.value + scratch_off)
    return _lib.call("mq_debug_group_check", dim, n, buf(queries, small * min(max(dim, 1), 4096) * 4), nq, k,
                     buf(codes, min(max(1, n), 4096) * 4), n_groups, buf(out_s, small * 64 * 4),
                     buf(out_i, small * 64 * 8), s, need if scratch_bytes is None else scratch_bytes)


def _raises(match, **kw):
    with pytest.raises(_lib.MQError, match=match) as e:
        _check(**kw)
    assert e.value.code == EINVAL


def test_scalar_checks_come_before_the_handle():
    """No handle, no buffers: k, nq and n_groups are refused first, then the NULL index."""
    def call(nq, k, n_groups):
        return _lib.call("mq_index_search_grouped", None, None, nq, k, None, n_groups, None, None, None, 0, None, 0,
                         None)
    for k in (0, 65, -3):
        with pytest.raises(_lib.MQError, match=r"k must be in \[1, 64\] \(got %d\)" % k) as e:
            call(1, k, 3)
        assert e.value.code == EINVAL
    with pytest.raises(_lib.MQError, match=r"query count -1 out of range"):
        call(-1, 5, 3)
    with pytest.raises(_lib.MQError, match=r"n_groups must be >= 0 \(got -2\)"):
        call(1, 5, -2)
    with pytest.raises(_lib.MQError, match="NULL index") as e:
        call(1, 5, 3)
    assert e.value.code == EINVAL


def test_every_shape_and_buffer_check_names_its_value():
    assert _check() == 0
    for k in (0, 65):
        _raises(r"k must be in \[1, 64\] \(got %d\)" % k, k=k)
    for dim in (0, 32, 96, 1088, 2048, -64):
        _raises(r"dim %% 64 == 0, dim <= 1024 \(got %d\)" % dim, dim=dim)
    for dim in (64, 256, 768, 1024):
        assert _check(dim=dim) == 0
    _raises(r"fewer than 2\^31 rows \(got 2147483648\)", n=1 << 31)
    _raises(r"n_groups must be >= 0 \(got -1\)", n_groups=-1)
    _raises(r"query count %d out of range" % ((1 << 24) + 1), nq=(1 << 24) + 1)
    # NULL pointers with rows in the index
    _raises("NULL queries", queries=None)
    _raises("NULL output buffer", out_s=None)
    _raises("NULL output buffer", out_i=None)
    _raises("NULL codes", codes=None)
    _raises("NULL scratch", scratch=None)
    # the scratch: aligned, large enough, and none of the outputs
    _raises(r"scratch must be 16-byte aligned \(got 0x[0-9a-f]+8\)", scratch_off=8)
    need = group_scratch_bytes(3, 1, 5)
    _raises(r"scratch_bytes %d is below the %d bytes mq_group_scratch_bytes\(3, 1, 5\) asks" % (need - 1, need),
            scratch_bytes=need - 1)
    _raises(r"scratch_bytes 0 is below", scratch_bytes=0)
    _raises(r"scratch_bytes -5 is below", scratch_bytes=-5)
    buf, p = _aligned(need + 64)
    _raises(r"scratch overlaps out_scores \(0x[0-9a-f]+\)", scratch=p, out_s=p)
    _raises(r"scratch overlaps out_ids \(0x[0-9a-f]+\)", scratch=p, out_i=ctypes.c_void_p(p.value + need - 8))
    inside = ctypes.c_void_p(p.value + 256)
    _raises(r"scratch overlaps out_scores", scratch=p, out_s=inside)
    # what needs no buffer: no queries; an empty index or no groups return padding without
    # reading codes or scratch (the outputs are still required)
    assert _check(nq=0, queries=None, out_s=None, out_i=None, codes=None, scratch=None, scratch_bytes=0) == 0
    assert _check(n=0, codes=None, scratch=None, scratch_bytes=0) == 0
    assert _check(n_groups=0, codes=None, scratch=None, scratch_bytes=0) == 0
    _raises("NULL output buffer", n=0, out_s=None)
    _raises(r"k must be in", nq=0, k=0)


def test_group_scratch_bytes_is_monotone_and_bounded_in_nq():
    f = group_scratch_bytes
    base = f(1000, 4, 8)
    assert base > 0 and base % 256 == 0
    for more in (f(10 ** 6, 4, 8), f(1000, 16, 8), f(1000, 4, 64)):
        assert more >= base
    sizes = [f(10 ** 5, nq, 64) for nq in (0, 1, 2, 15, 16, 17, 40, 256, 4096, 10 ** 9)]
    assert sizes == sorted(sizes) and sizes[0] == 0
    assert f(10 ** 5, 16, 64) == f(10 ** 5, 17, 64) == f(10 ** 5, 1 << 40, 64)  # the passes reuse the table
    sizes = [f(g, 16, 64) for g in (0, 1, 2047, 2048, 2049, 10 ** 5, 10 ** 6, 10 ** 8)]
    assert sizes == sorted(sizes)
    sizes = [f(10 ** 5, 16, k) for k in (1, 5, 8, 9, 16, 17, 64)]
    assert sizes == sorted(sizes)
    # the table is 8 bytes per (query of a pass, group); everything else stays small
    assert 16 * 10 ** 6 * 8 <= f(10 ** 6, 256, 64) < 16 * 10 ** 6 * 8 + (2 << 20)
    # arguments out of range are clamped
    assert f(1000, 4, 0) == f(1000, 4, 1) and f(1000, 4, 1000) == f(1000, 4, 64)
    assert f(-5, -1, 8) == f(0, 0, 8) == 0


def test_scan_geometry():
    assert group_scan_blocks(0, 256) == 1 and group_scan_blocks(1, 256) == 1
    assert group_scan_blocks(128, 256) == 1 and group_scan_blocks(129, 256) == 2
    assert group_scan_blocks(10 ** 6, 256) == 512 and group_scan_blocks(10 ** 6, 0) == 2


# ---------------------------------------------------------------- the retriever ----
def test_window_splitter():
    sp = WindowSplitter(chunk_size=4, chunk_overlap=1)
    assert sp.split_text("abcdefghij") == ["abcd", "defg", "ghij"]
    assert sp.split_text("abcdefghijk") == ["abcd", "defg", "ghij", "jk"]
    assert sp.split_text("abcd") == ["abcd"] and sp.split_text("ab") == ["ab"] and sp.split_text("") == []
    assert WindowSplitter(3, 0).split_text("问题：头痛怎么办") == ["问题：", "头痛怎", "么办"]  # characters, not bytes
    docs = [Document(page_content="abcdefgh", metadata={"src": 1}), Document(page_content="", metadata={"src": 2}),
            Document(page_content="xy", metadata={"src": 3})]
    out = WindowSplitter(4, 0).split_documents(docs)
    assert [(d.page_content, d.metadata) for d in out] == [("abcd", {"src": 1}), ("efgh", {"src": 1}),
                                                            ("xy", {"src": 3})]
    out[0].metadata["src"] = 9  # a copy: the parent's metadata is its own
    assert docs[0].metadata == {"src": 1}
    for size, overlap in ((0, 0), (4, 4), (4, -1), (4, 5)):
        with pytest.raises(ValueError, match="chunk_size|chunk_overlap"):
            WindowSplitter(size, overlap)


class _FakeStore:
    def __init__(self):
        self.added, self.calls, self.answer = [], [], []

    def add_documents(self, documents, **kwargs):
        self.added += list(documents)

    def similarity_search_grouped(self, query, **kwargs):
        self.calls.append((query, kwargs))
        return self.answer


def test_retriever_bookkeeping():
    store = _FakeStore()
    r = HipParentDocumentRetriever(store, child_splitter=WindowSplitter(4, 0), search_kwargs={"k": 5, "filter": {"a": 1}})
    parents = [Document(page_content="abcdefghij", metadata={"a": 1}), Document(page_content="xyz", metadata={"a": 2})]
    assert r.add_documents(parents, ids=["p0", "p1"]) == ["p0", "p1"]
    assert [(d.page_content, d.metadata) for d in store.added] == [
        ("abcd", {"a": 1, "doc_id": "p0"}), ("efgh", {"a": 1, "doc_id": "p0"}), ("ij", {"a": 1, "doc_id": "p0"}),
        ("xyz", {"a": 2, "doc_id": "p1"})]
    assert parents[0].metadata == {"a": 1}  # the parents are stored untagged
    assert isinstance(r.docstore, InMemoryDocstore) and r.docstore.mget(["p1", "nope", "p0"]) == [parents[1], None,
                                                                                                  parents[0]]
    # invoke: the grouped search with the id key and the search kwargs; parents in its order;
    # a child whose parent the docstore lacks is dropped
    store.answer = [store.added[3], Document(page_content="?", metadata={"doc_id": "gone"}), store.added[1]]
    assert r.invoke("q") == [parents[1], parents[0]]
    assert r.get_relevant_documents("q2") == [parents[1], parents[0]]
    assert store.calls == [("q", {"group_by": "doc_id", "k": 5, "filter": {"a": 1}}),
                           ("q2", {"group_by": "doc_id", "k": 5, "filter": {"a": 1}})]
    # generated ids are distinct; a length mismatch is refused before anything is added
    ids = r.add_documents([Document(page_content="abcdefgh"), Document(page_content="abcdefgh")])
    assert len(set(ids)) == 2 and {d.metadata["doc_id"] for d in store.added[4:]} == set(ids)
    before = len(store.added)
    with pytest.raises(ValueError, match="1 ids for 2 documents"):
        r.add_documents(parents, ids=["only"])
    assert len(store.added) == before
    # another id key and docstore, no splitter: the parents are their own children
    class Dict2:
        def __init__(self):
            self.d = {}

        def mset(self, pairs):
            self.d.update(pairs)

        def mget(self, keys):
            return [self.d.get(k) for k in keys]
    store2, ds = _FakeStore(), Dict2()
    r2 = HipParentDocumentRetriever(store2, docstore=ds, id_key="parent")
    r2.add_documents(parents[:1], ids=["z"])
    assert [(d.page_content, d.metadata) for d in store2.added] == [("abcdefghij", {"a": 1, "parent": "z"})]
    assert ds.d == {"z": parents[0]}
    store2.answer = store2.added
    assert r2.invoke("q") == [parents[0]] and store2.calls == [("q", {"group_by": "parent"})]
