"""The self-join on the host: every argument check of mq_index_self_join answers MQ_EINVAL and
names the offending value before any HIP call (no GPU needed; the checks that need the index's
shape are reached through mq_debug_join_check on a stated (dim, rows)), the scratch size is
monotone, and the store's `deduplicate` rounds, driven by a numpy stand-in for the device scan,
give exactly the sequential greedy result - on constructed chains, on the near-duplicate corpus,
with `ids`, with a filter, and when max_rounds cuts the rounds short."""
import ctypes

import numpy as np
import pytest

import join_cases as jc
from mediquery_hip import DedupResult, DuplicateScan, HipChroma, _lib
from mediquery_hip.native import join_scratch_bytes
from mediquery_hip.vectorstore import greedy_dedup_rounds

EINVAL = -1
INF = float("inf")


def _aligned(nbytes):
    buf = (ctypes.c_uint8 * (nbytes + 64))()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)


def _check(dim=256, n=10, min_score=0.9, mode=_lib.MQ_JOIN_AUTO, left=None, n_left=None, out_c=True, out_f=True,
           out_n=True, out_s=True, out_info=True, scratch=True, scratch_bytes=None, scratch_off=0):
    """mq_debug_join_check with sound defaults; True = a valid host buffer of its own."""
    keep = []

    def buf(flag, nbytes):
        if flag is not True:
            return flag
        b, p = _aligned(nbytes)
        keep.append(b)
        return p
    n_left = n if n_left is None else n_left
    need = join_scratch_bytes(n, n_left)
    small = min(max(1, n_left), 64)  # nothing is read: a refused call needs no room for 2^31 rows
    s = buf(scratch, min(need, 16 << 20) + 64)
    if s is not None and scratch_off:
        s = ctypes.c_void_p(s.value + scratch_off)
    return _lib.call("mq_debug_join_check", dim, n, min_score, mode, buf(left, small * 8), n_left, buf(out_c, small * 8),
                     buf(out_f, small * 8), buf(out_n, small * 8), buf(out_s, small * 4), buf(out_info, 32), s,
                     need if scratch_bytes is None else scratch_bytes)


def _raises(match, **kw):
    with pytest.raises(_lib.MQError, match=match) as e:
        _check(**kw)
    assert e.value.code == EINVAL


def test_constants_are_the_headers():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mq.h")).read()
    for name in ("MQ_JOIN_AUTO", "MQ_JOIN_EXACT", "MQ_JOIN_SCREEN"):
        assert "#define %s %d" % (name, getattr(_lib, name)) in header


def test_scalar_checks_come_before_the_handle():
    def call(min_score, mode, n_left):
        return _lib.call("mq_index_self_join", None, min_score, None, None, n_left, mode, None, None, None, None, None,
                         0, None, 0, None)
    with pytest.raises(_lib.MQError, match="min_score must not be NaN") as e:
        call(float("nan"), 0, 1)
    assert e.value.code == EINVAL
    for mode in (-1, 3, 17):
        with pytest.raises(_lib.MQError, match=r"mode must be MQ_JOIN_AUTO \(0\), MQ_JOIN_EXACT \(1\) or "
                                               r"MQ_JOIN_SCREEN \(2\) \(got %d\)" % mode) as e:
            call(0.5, mode, 1)
        assert e.value.code == EINVAL
    with pytest.raises(_lib.MQError, match=r"left row count -1 out of range"):
        call(0.5, 0, -1)
    for tau in (-INF, INF, 0.5):
        with pytest.raises(_lib.MQError, match="NULL index") as e:
            call(tau, 1, 1)
        assert e.value.code == EINVAL


def test_every_shape_and_buffer_check_names_its_value():
    assert _check() == 0
    _raises("min_score must not be NaN", min_score=float("nan"))
    for tau in (-INF, -0.0, 0.25, INF):
        assert _check(min_score=tau) == 0
    _raises(r"mode must be .* \(got 3\)", mode=3)
    _raises(r"mode must be .* \(got -1\)", mode=-1)
    for dim in (0, 32, 96, 1088, 2048, -64):
        _raises(r"dim %% 64 == 0, dim <= 1024 \(got %d\)" % dim, dim=dim)
    for dim in (64, 256, 512, 768, 1024):
        assert _check(dim=dim) == 0 and _check(dim=dim, mode=_lib.MQ_JOIN_EXACT) == 0
    for dim in (64, 128, 320, 1024):
        _raises(r"MQ_JOIN_SCREEN serves dim 256, 512 or 768 \(got %d\)" % dim, dim=dim, mode=_lib.MQ_JOIN_SCREEN)
    for dim in (256, 512, 768):
        assert _check(dim=dim, mode=_lib.MQ_JOIN_SCREEN) == 0
    _raises(r"fewer than 2\^31 rows \(got 2147483648\)", n=1 << 31, n_left=5, left=True)
    _raises(r"left row count 2147483648 out of range", n_left=1 << 31, left=True)
    # NULL left rows mean every row
    _raises(r"n_left 7 must equal the index's 10 rows when left_rows is NULL", n_left=7)
    assert _check(n_left=7, left=True) == 0
    # NULL pointers with rows in the index
    _raises("NULL out_info", out_info=None)
    for name in ("out_c", "out_f", "out_n", "out_s"):
        _raises("NULL output buffer", **{name: None})
    _raises("NULL scratch", scratch=None)
    # the scratch: aligned, large enough, and none of the other buffers
    _raises(r"scratch must be 16-byte aligned \(got 0x[0-9a-f]+8\)", scratch_off=8)
    need = join_scratch_bytes(10, 10)
    _raises(r"scratch_bytes %d is below the %d bytes mq_join_scratch_bytes\(10, 10\) asks" % (need - 1, need),
            scratch_bytes=need - 1)
    _raises(r"scratch_bytes 0 is below", scratch_bytes=0)
    _raises(r"scratch_bytes -5 is below", scratch_bytes=-5)
    buf, p = _aligned(need + 64)
    _raises(r"scratch overlaps out_counts \(0x[0-9a-f]+\)", scratch=p, out_c=ctypes.c_void_p(p.value + need - 8))
    _raises(r"scratch overlaps out_first \(0x[0-9a-f]+\)", scratch=p, out_f=p)
    _raises(r"scratch overlaps out_nearest \(0x[0-9a-f]+\)", scratch=p, out_n=ctypes.c_void_p(p.value + 256))
    _raises(r"scratch overlaps out_nearest_scores \(0x[0-9a-f]+\)", scratch=p, out_s=ctypes.c_void_p(p.value + 512))
    _raises(r"scratch overlaps out_info \(0x[0-9a-f]+\)", scratch=p, out_info=ctypes.c_void_p(p.value + need - 32))
    _raises(r"scratch overlaps left_rows \(0x[0-9a-f]+\)", scratch=p, left=ctypes.c_void_p(p.value + 1024))
    # what needs no buffer but out_info: no left rows, an empty index
    assert _check(n_left=0, left=True, out_c=None, out_f=None, out_n=None, out_s=None, scratch=None,
                  scratch_bytes=0) == 0
    assert _check(n=0, out_c=None, out_f=None, out_n=None, out_s=None, scratch=None, scratch_bytes=0) == 0
    _raises("NULL out_info", n=0, out_info=None)


def test_join_scratch_bytes_is_monotone():
    f = join_scratch_bytes
    base = f(1000, 16)
    assert base > 0 and base % 256 == 0
    sizes = [f(n, 1000) for n in (0, 1, 127, 128, 129, 4097, 10 ** 5, 10 ** 6, 10 ** 8, (1 << 31) - 1)]
    assert sizes == sorted(sizes)
    sizes = [f(10 ** 5, m) for m in (0, 1, 15, 16, 17, 255, 256, 257, 4096, 10 ** 5, 10 ** 6)]
    assert sizes == sorted(sizes)
    # a panel's survivor lists (256 x 4096 x 8 bytes) and bf16 rows dominate; 40 bytes per left row
    # (the redo list and a host call's staging) come on top
    assert 8 << 20 <= f(10 ** 6, 0) < 10 << 20
    assert 40 * 10 ** 6 <= f(10 ** 6, 10 ** 6) - f(10 ** 6, 0) <= 40 * 10 ** 6 + 8 * 256
    # arguments out of range are clamped
    assert f(-5, -1) == f(0, 0) and f(1 << 40, 1 << 40) == f((1 << 31) - 1, (1 << 31) - 1)


# ------------------------------------------------------ the greedy rounds on the host ----
def _rounds(s, tau, left=None, mask=None, max_rounds=32):
    n = s.shape[0]
    return greedy_dedup_rounds(n, np.arange(n) if left is None else left, np.ones(n, bool) if mask is None else mask,
                               jc.numpy_scan_first(s, tau), max_rounds)


def test_chain_of_three_keeps_both_ends():
    """A ~ B ~ C with A and C apart: B goes (A is kept and its partner), C stays (its only
    earlier partner was dropped)."""
    s = np.array([[1, .95, .5], [.95, 1, .95], [.5, .95, 1]])
    dropped, keepers, und, rounds = _rounds(s, 0.9)
    assert dropped.tolist() == [1] and keepers.tolist() == [0] and len(und) == 0 and rounds == 2
    assert jc.greedy_keep(s, 0.9).tolist() == [True, False, True]


def test_chain_of_six_alternates():
    s = np.eye(6) + 0.95 * (np.eye(6, k=1) + np.eye(6, k=-1))
    dropped, keepers, und, rounds = _rounds(s, 0.9)
    assert dropped.tolist() == [1, 3, 5] and keepers.tolist() == [0, 2, 4] and len(und) == 0
    assert np.array_equal(~jc.greedy_keep(s, 0.9), np.isin(np.arange(6), dropped))
    # cut short: the decided rows are the greedy ones, the rest is reported undecided and kept
    d1, k1, u1, r1 = _rounds(s, 0.9, max_rounds=1)
    assert r1 == 1 and d1.tolist() == [1] and u1.tolist() == [2, 3, 4, 5]
    d2, _, u2, r2 = _rounds(s, 0.9, max_rounds=2)
    assert r2 == 2 and d2.tolist() == [1, 3] and u2.tolist() == [4, 5]


def test_clique_needs_one_round():
    s = np.full((5, 5), 0.97)
    dropped, keepers, und, rounds = _rounds(s, 0.9)
    assert dropped.tolist() == [1, 2, 3, 4] and keepers.tolist() == [0] * 4 and rounds == 1


@pytest.mark.parametrize("tau", jc.RANDOM_MIN_SCORES)
def test_rounds_equal_the_sequential_rule_on_the_neardup_corpus(tau):
    rows = jc.neardup_corpus(256, 1000)
    s = jc.scores64(rows)
    for left, mask in ((None, None), (np.arange(600, 1000), None), (None, jc.row_mask("third", 1000)),
                       (np.arange(1, 1000, 2), jc.row_mask("third", 1000))):
        dropped, keepers, und, rounds = _rounds(s, tau, left, mask)
        kept = jc.greedy_keep(s, tau, left, mask)
        assert np.array_equal(dropped, np.flatnonzero(~kept)) and len(und) == 0
        assert len(dropped) >= 10 and 1 <= rounds <= 8  # the case is not vacuous; the rounds stay few
        assert (keepers < dropped).all() and kept[keepers].all() and (s[dropped, keepers] >= tau).all()
        # the keeper is the smallest kept earlier partner
        for r, k in zip(dropped.tolist()[:50], keepers.tolist()):
            ok = np.ones(1000, bool) if mask is None else mask
            assert k == np.flatnonzero(kept[:r] & ok[:r] & (s[r, :r] >= tau))[0]


# ------------------------------------------------------------------- the store's side ----
class _RefIndex:
    """FlatIndex's self_join, select and get, answered by the float64 reference."""

    def __init__(self, rows):
        self.rows, self.dim, self.calls = rows, rows.shape[1], []
        self.s = jc.scores64(rows)

    def __len__(self):
        return len(self.rows)

    def self_join(self, min_score, bits=None, left_rows=None, mode=0, scratch=None):
        self.calls.append((min_score, bits is not None, None if left_rows is None else len(left_rows), mode))
        s = self.s if left_rows is None else self.s[left_rows]
        c, f, nn, sc = jc.join_reference(s, left_rows, bits, min_score)
        return c, f, nn, sc.astype(np.float32), np.array([c.sum(), 0, 0, len(c)], np.int64)

    def select(self, rows):
        return _RefIndex(self.rows[rows])

    def get(self):
        return self.rows


class _Store(HipChroma):
    """HipChroma with the device behind it replaced: the index is `_RefIndex`, a filter
    {"tag": t} is the host mask r % 3 == t, masks stay host arrays and `delete` records."""

    def __init__(self, rows):
        super().__init__(dim=rows.shape[1], auto_persist=False)
        n = len(rows)
        self._index = _RefIndex(rows)
        self._ids = ["id%d" % r for r in range(n)]
        self._texts = ["row %d" % r for r in range(n)]
        self._metas = [{"tag": r % 3} for r in range(n)]
        self._id_row.extend(self._ids)
        self.deleted = None

    def _join_room(self, n, n_left):
        return None

    def _host_bits(self, mask):
        return mask

    def _admit(self, k, filter, where_document):
        assert where_document is None
        return k, np.arange(len(self._ids)) % 3 == filter["tag"]

    def _mask_rows(self, bits):
        return bits

    def delete(self, ids=None, **kw):
        self.deleted = list(ids)


N = 600


@pytest.fixture(scope="module")
def corpus():
    rows = jc.neardup_corpus(256, N)
    return rows, jc.scores64(rows)


def test_duplicate_scan_is_the_reference(corpus):
    rows, s = corpus
    store = _Store(rows)
    scan = store.duplicate_scan(0.9)
    assert isinstance(scan, DuplicateScan) and len(scan) == N and np.array_equal(scan.rows, np.arange(N))
    c, f, nn, sc = jc.join_reference(s, None, None, 0.9)
    assert np.array_equal(scan.counts, c) and np.array_equal(scan.first, f) and np.array_equal(scan.nearest, nn)
    assert scan.nearest_cosine.dtype == np.float32 and scan.info[0] == c.sum()
    assert store._index.calls == [(0.9, False, None, _lib.MQ_JOIN_AUTO)]
    # ids pick the left rows (ascending, unknown ids ignored, repeats folded); a filter masks both sides
    scan = store.duplicate_scan(0.8, ids=["id7", "id3", "nope", "id3", "id300"], filter={"tag": 0}, mode="exact")
    assert scan.rows.tolist() == [3, 7, 300]
    mask = np.arange(N) % 3 == 0
    c, f, nn, sc = jc.join_reference(s[[3, 7, 300]], np.array([3, 7, 300]), mask, 0.8)
    assert np.array_equal(scan.counts, c) and np.array_equal(scan.first, f) and c[1] == 0  # row 7 is masked out
    assert store._index.calls[-1] == (0.8, True, 3, _lib.MQ_JOIN_EXACT)
    assert len(store.duplicate_scan(0.9, ids=["nope"])) == 0 and len(store._index.calls) == 2


def test_duplicate_arguments_are_checked(corpus):
    store = _Store(corpus[0])
    for bad in (None, float("nan"), INF, -INF, "0.9", True):
        with pytest.raises(ValueError, match="min_cosine must be"):
            store.duplicate_scan(bad)
    with pytest.raises(ValueError, match="mode must be one of"):
        store.duplicate_scan(0.9, mode="fast")
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="max_rounds must be a positive integer"):
            store.deduplicate(0.9, max_rounds=bad)
    odd = _Store(np.eye(96, dtype=np.float32))
    with pytest.raises(ValueError, match="dim is 96"):
        odd.duplicate_scan(0.9)
    wide = _Store(np.eye(1024, dtype=np.float32)[:8])
    with pytest.raises(ValueError, match="mode='screen' serves stores of dim 256, 512 or 768"):
        wide.duplicate_scan(0.9, mode="screen")
    empty = HipChroma(dim=256, auto_persist=False)
    assert len(empty.duplicate_scan(0.9)) == 0 and empty.deduplicate(0.9) == [] and empty.find_duplicates(0.9) == []


@pytest.mark.parametrize("kw", ({}, {"ids": ["id%d" % r for r in range(300, N)]}, {"filter": {"tag": 1}}))
def test_deduplicate_leaves_the_greedy_survivors(corpus, kw):
    rows, s = corpus
    left = None if "ids" not in kw else np.arange(300, N)
    mask = None if "filter" not in kw else np.arange(N) % 3 == 1
    kept = jc.greedy_keep(s, 0.9, left, mask)
    store = _Store(rows)
    found = store.find_duplicates(0.9, **kw)
    assert store.deleted is None and isinstance(found, DedupResult) and found.undecided == []
    assert [d.id for d, _, _ in found] == ["id%d" % r for r in np.flatnonzero(~kept)]
    for d, k, c in found:
        r, q = int(d.id[2:]), int(k.id[2:])
        assert q < r and kept[q] and c >= 0.9 and abs(c - s[r, q]) < 1e-6
    gone = store.deduplicate(0.9, **kw)
    assert isinstance(gone, DedupResult) and gone == [d.id for d, _, _ in found] == store.deleted
    assert gone.rounds == found.rounds >= 1 and len(gone) > 10


def test_max_rounds_reports_the_undecided():
    s = np.eye(6) + 0.95 * (np.eye(6, k=1) + np.eye(6, k=-1))

    class _Chain(_RefIndex):
        def __init__(self):
            self.rows, self.dim, self.calls, self.s = np.zeros((6, 64), np.float32), 64, [], s

    store = _Store(np.zeros((6, 64), np.float32))
    store._index = _Chain()
    gone = store.deduplicate(0.9, max_rounds=1)
    assert gone == ["id1"] and gone.undecided == ["id2", "id3", "id4", "id5"] and gone.rounds == 1
    gone = store.deduplicate(0.9)
    assert gone == ["id1", "id3", "id5"] and gone.undecided == [] and gone.rounds == 3
