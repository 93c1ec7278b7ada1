"""The self-join (K18, mq_index_self_join) on the GPU against the float64 reference of
join_cases.py: bit for bit on the exact class over the row counts, dims, modes, masks,
thresholds and left lists; through `check_random` on the near-duplicate corpora in every mode;
bit for bit against the range search (K17) on any data; the overflow of a survivor list into the
exact walk; the path each mode takes; determinism, device I/O, the empty cases; and the store's
duplicate_scan / find_duplicates / deduplicate, persisted and reloaded."""
import numpy as np
import pytest
import torch

import join_cases as jc
from mediquery_hip import DedupResult, HipChroma, _lib
from mediquery_hip.native import FlatIndex, join_scratch_bytes

pytestmark = pytest.mark.gpu

INF = float("inf")
MODES = {"exact": _lib.MQ_JOIN_EXACT, "auto": _lib.MQ_JOIN_AUTO, "screen": _lib.MQ_JOIN_SCREEN}
_cache = {}


def _modes(dim):
    return [m for m in MODES if m != "screen" or dim in jc.SCREEN_DIMS]


def _index(kind, dim, n):
    """(index, stored rows, float64 scores of every row pair); the exact class is stored bit for
    bit, the random class is read back: the reference is computed from what the index holds."""
    key = (kind, dim, n)
    if key not in _cache:
        rows = jc.exact_corpus(dim, n) if kind == "exact" else jc.neardup_corpus(dim, n)
        ix = FlatIndex(dim=dim, device=0)
        ix.add(rows)
        stored = ix.get()
        if kind == "exact":
            assert np.array_equal(stored, rows)
        _cache[key] = (ix, stored, jc.scores64(stored))
    return _cache[key]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached corpora are read-only


def _bits(mask):
    return None if mask is None else _dev(jc.mask_words(mask))


def _same(got, ref, where):
    for g, r, name in zip(got[:3], ref[:3], ("counts", "first", "nearest")):
        assert np.array_equal(g, r), (where, name)
    assert np.array_equal(got[3].view(np.int32), ref[3].astype(np.float32).view(np.int32)), (where, "scores")
    assert got[4][0] == ref[0].sum() and got[4][1] + got[4][3] == len(ref[0]), (where, got[4])


@pytest.mark.parametrize("dim", jc.DIMS)
def test_exact_class_equals_reference(require_gpu, dim):
    seen = set()
    for ni, n in enumerate(jc.NS):
        ix, rows, s_all = _index("exact", dim, n)
        for oi, mode in enumerate(_modes(dim)):
            for ti, tau in enumerate(jc.MIN_SCORES):
                # every (n, mode) meets every min_score; masks and left lists rotate against them
                mk = jc.MASKS[(ti + ni + oi) % len(jc.MASKS)]
                lk = jc.LEFTS[(ti + 2 * ni + oi) % len(jc.LEFTS)]
                mask, left = jc.row_mask(mk, n), jc.left_rows(lk, n)
                ref = jc.join_reference(s_all if left is None else s_all[left], left, mask, tau)
                got = ix.self_join(tau, _bits(mask), left, MODES[mode])
                _same(got, ref, (dim, n, mode, tau, mk, lk))
                seen.update({(mode, "mask", mk), (mode, "left", lk), (mode, "tau", ti)})
                if ref[0].max(initial=0) > 1:
                    seen.add((mode, "several"))
    for mode in _modes(dim):
        assert all((mode, "mask", mk) in seen for mk in jc.MASKS)
        assert all((mode, "left", lk) in seen for lk in jc.LEFTS)
        assert (mode, "several") in seen


@pytest.mark.parametrize("dim,n", jc.RANDOM_SHAPES)
def test_random_class_in_every_mode(require_gpu, dim, n):
    ix, rows, s_all = _index("random", dim, n)
    mask = jc.row_mask("third", n)
    for mode in _modes(dim):
        for tau in jc.RANDOM_MIN_SCORES:
            for m, left in ((None, None), (mask, jc.left_rows("third", n))):
                s = s_all if left is None else s_all[left]
                got = ix.self_join(tau, _bits(m), left, MODES[mode])
                fails, und = jc.check_random(got[:4], s, left, m, tau, dim)
                assert not fails, (mode, tau, m is not None, fails[:3])
                assert und.mean() <= jc.NEAR_TIE_CAP
                assert got[4][0] == got[0].sum()


@pytest.mark.parametrize("dim,n", ((768, 700), (256, 1000)))
def test_bit_equality_with_the_range_search(require_gpu, dim, n):
    """On any data the join's scores are the range search's: for every left row, the range
    search with the stored row as the query, the row itself dropped from its list."""
    ix, rows, _ = _index("random", dim, n)
    for tau in (0.9, 0.8):
        counts, s, ids = ix.search_range(rows, 4096, tau)
        want = []
        for i in range(n):
            keep = (ids[i] >= 0) & (ids[i] != i)
            hi, hs = ids[i][keep], s[i][keep]
            assert counts[i] <= 4096
            want.append((len(hi), hi.min() if len(hi) else -1, hi[0] if len(hi) else -1,
                         hs[0] if len(hi) else np.float32(-INF)))
        wc, wf, wn, ws = (np.array(c) for c in zip(*want))
        assert wc.sum() > n // 4
        for mode in _modes(dim):
            if mode == "auto":
                continue
            got = ix.self_join(tau, None, None, MODES[mode])
            assert np.array_equal(got[0], wc) and np.array_equal(got[1], wf) and np.array_equal(got[2], wn), mode
            assert np.array_equal(got[3].view(np.int32), ws.astype(np.float32).view(np.int32)), mode


def test_overflowing_survivor_lists_go_to_the_exact_walk(require_gpu):
    """4200 copies of one vector: each copy's survivor list (4199 > 4096) overflows and the row
    is answered by the exact walk; the 200 other rows stay with the screen."""
    dim, copies, others = 256, 4200, 200
    base = jc.exact_corpus(dim, 3 * others)
    vec = base[:1]
    rest = base[(base != vec).any(1)][:others]
    assert len(rest) == others
    rows = np.concatenate([np.repeat(vec, copies, axis=0), rest])
    rows = rows[np.random.default_rng(5).permutation(len(rows))]
    ix = FlatIndex(dim=dim, device=0)
    ix.add(rows)
    assert np.array_equal(ix.get(), rows)
    ref = jc.join_reference(jc.scores64(rows), None, None, 1.0)
    assert (ref[0] == copies - 1).sum() == copies
    screen = ix.self_join(1.0, None, None, _lib.MQ_JOIN_SCREEN)
    exact = ix.self_join(1.0, None, None, _lib.MQ_JOIN_EXACT)
    _same(screen, ref, "screen")
    _same(exact, ref, "exact")
    assert screen[4][3] == copies and screen[4][1] == others and exact[4].tolist()[1:] == [0, 0, len(rows)]
    for a, b in zip(screen[:4], exact[:4]):
        assert np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                              b.view(np.int32) if b.dtype == np.float32 else b)


def test_the_screen_answers_the_near_duplicate_corpus_alone(require_gpu):
    dim, n, tau = 256, 4500, 0.9
    ix, rows, s_all = _index("random", dim, n)
    b = jc.bound(dim)
    lo, hi = (int(jc.join_reference(s_all, None, None, t)[0].sum()) for t in (tau + b, tau - b))
    assert lo > n // 4 and lo % 2 == 0  # ordered pairs: every unordered pair counts from both sides
    info = ix.self_join(tau, None, None, _lib.MQ_JOIN_SCREEN)[4]
    assert info[1] == n and info[3] == 0 and lo <= info[0] <= hi
    # verified candidates: every partner pair from both of its sides (twice the unordered pairs),
    # and every row against itself (its bf16 self-score is about 1)
    assert info[2] >= lo + n
    info = ix.self_join(tau, None, None, _lib.MQ_JOIN_EXACT)[4]
    assert info.tolist()[1:] == [0, 0, n] and lo <= info[0] <= hi


def test_auto_screens_a_large_index_and_walks_a_small_one(require_gpu):
    dim, n = 256, 20000
    rows = jc.exact_corpus(dim, n)
    ix = FlatIndex(dim=dim, device=0)
    ix.add(rows)
    left = np.arange(7, n, 61, dtype=np.int64)
    mask = jc.row_mask("third", n)
    s = jc.scores64(rows, left)
    for m in (None, mask):
        ref = jc.join_reference(s, left, m, 0.75)
        got = ix.self_join(0.75, _bits(m), left, _lib.MQ_JOIN_AUTO)
        _same(got, ref, ("auto", m is not None))
        assert got[4][1] == len(left) and got[4][3] == 0
        _same(ix.self_join(0.75, _bits(m), left, _lib.MQ_JOIN_EXACT), ref, ("exact", m is not None))
    small = _index("exact", 256, 1000)[0]  # below the 1024 rows AUTO screens from
    assert small.self_join(0.75, None, None, _lib.MQ_JOIN_AUTO)[4].tolist()[1:] == [0, 0, 1000]
    at = FlatIndex(dim=dim, device=0)
    at.add(rows[:1024])
    info = at.self_join(0.75, None, None, _lib.MQ_JOIN_AUTO)[4]
    assert info[1] == 1024 and info[3] == 0


def test_repeated_calls_and_device_io_return_the_same_bits(require_gpu):
    dim, n, tau = 768, 700, 0.8
    ix, rows, s_all = _index("random", dim, n)
    mask = jc.row_mask("third", n)
    left = jc.left_rows("reversed", n)
    scratch = torch.empty(join_scratch_bytes(n, n), dtype=torch.uint8, device="cuda")
    for mode in (_lib.MQ_JOIN_SCREEN, _lib.MQ_JOIN_EXACT):
        for m, lf in ((None, None), (mask, left)):
            bits = _bits(m)
            first = ix.self_join(tau, bits, lf, mode, scratch)
            scratch.fill_(0xA5)  # what a call leaves in the scratch is not read by the next
            again = ix.self_join(tau, bits, lf, mode, scratch)
            outs = (torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda"),
                    torch.empty(n, dtype=torch.int64, device="cuda"),
                    torch.empty(n, dtype=torch.float32, device="cuda"),
                    torch.empty(4, dtype=torch.int64, device="cuda"))
            ix.self_join_device(tau, *outs, bits=bits, left_rows=None if lf is None else _dev(lf), mode=mode,
                                scratch=scratch)
            for a, b, c in zip(first, again, outs):
                view = (lambda x: x.view(np.int32)) if a.dtype == np.float32 else (lambda x: x)
                assert np.array_equal(view(a), view(b)) and np.array_equal(view(a), view(c.cpu().numpy()))


def test_empty_index_and_no_left_rows(require_gpu):
    empty = FlatIndex(dim=256, device=0)
    for mode in MODES.values():
        c, f, nn, s, info = empty.self_join(0.9, None, None, mode)
        assert len(c) == len(f) == len(nn) == len(s) == 0 and info.tolist() == [0, 0, 0, 0]
    ix = _index("exact", 256, 65)[0]
    for mode in MODES.values():
        c, f, nn, s, info = ix.self_join(0.9, None, np.empty(0, np.int64), mode)
        assert len(c) == 0 and info.tolist() == [0, 0, 0, 0]
    info = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    ix.self_join_device(0.9, e, e, e, torch.empty(0, device="cuda"), info, left_rows=e)
    assert info.cpu().tolist() == [0, 0, 0, 0]
    with pytest.raises(_lib.MQError, match=r"left_rows\[1\] = 65 is outside \[0, 65\)"):
        ix.self_join(0.9, None, np.array([3, 65], np.int64))
    with pytest.raises(ValueError, match="MQ_JOIN_SCREEN serves dim 256, 512 or 768"):
        _index("exact", 64, 65)[0].self_join(0.9, None, None, _lib.MQ_JOIN_SCREEN)


# ----------------------------------------------------------------------- the store ----
STORE_DIM, STORE_N = 256, 600


def _store(tmp=None):
    rows = jc.neardup_corpus(STORE_DIM, STORE_N)
    store = HipChroma(dim=STORE_DIM, persist_directory=tmp, auto_persist=tmp is not None)
    store.add_embeddings(rows, ["row %d is %s" % (r, "odd" if r % 2 else "even") for r in range(STORE_N)],
                         [{"tag": r % 3} for r in range(STORE_N)], ["id%d" % r for r in range(STORE_N)])
    stored = store._index.get()
    return store, stored, jc.scores64(stored)


def _decided(s, tau):
    """The store tests' threshold sits where no pair of the corpus is within the fp32 bound of
    it, so every count and first is decided; checked here, from the reference."""
    off = ~np.eye(len(s), dtype=bool)
    return not (np.abs(s[off] - tau) <= jc.bound(STORE_DIM)).any()


def test_store_duplicate_scan_with_ids_filter_and_where_document(require_gpu):
    store, rows, s = _store()
    tau = 0.9
    assert _decided(s, tau)
    for mode in ("auto", "exact", "screen"):
        scan = store.duplicate_scan(tau, mode=mode)
        c, f, nn, sc = jc.join_reference(s, None, None, tau)
        assert np.array_equal(scan.rows, np.arange(STORE_N)) and np.array_equal(scan.counts, c)
        assert np.array_equal(scan.first, f) and scan.info[0] == c.sum() and c.sum() > 100
        # ids pick the left rows; the filter and the text clause mask both sides
        ids = ["id%d" % r for r in range(5, STORE_N, 7)]
        left = np.arange(5, STORE_N, 7)
        for kw, mask in (({}, None), ({"filter": {"tag": 0}}, np.arange(STORE_N) % 3 == 0),
                         ({"where_document": {"$contains": "even"}}, np.arange(STORE_N) % 2 == 0),
                         ({"filter": {"tag": 1}, "where_document": {"$contains": "odd"}},
                          (np.arange(STORE_N) % 3 == 1) & (np.arange(STORE_N) % 2 == 1))):
            scan = store.duplicate_scan(tau, ids=ids, mode=mode, **kw)
            c, f, nn, sc = jc.join_reference(s[left], left, mask, tau)
            assert np.array_equal(scan.rows, left) and np.array_equal(scan.counts, c), (mode, kw)
            assert np.array_equal(scan.first, f), (mode, kw)
            und = jc.undecided_rows(s[left], left, mask, tau, STORE_DIM)
            assert np.array_equal(scan.nearest[~und], nn[~und]) and und.mean() <= jc.NEAR_TIE_CAP
            assert np.abs(scan.nearest_cosine[c > 0] - sc[c > 0]).max(initial=0) <= jc.bound(STORE_DIM)
            assert np.isneginf(scan.nearest_cosine[c == 0]).all()


def test_store_deduplicate_leaves_the_greedy_survivors_and_persists(require_gpu, tmp_path):
    store, rows, s = _store(str(tmp_path))
    tau = 0.9
    assert _decided(s, tau)
    kept = jc.greedy_keep(s, tau)
    found = store.find_duplicates(tau)
    assert isinstance(found, DedupResult) and found.undecided == [] and len(store) == STORE_N
    assert [d.id for d, _, _ in found] == ["id%d" % r for r in np.flatnonzero(~kept)]
    for d, k, c in found:
        r, q = int(d.id[2:]), int(k.id[2:])
        assert q < r and kept[q] and abs(c - s[r, q]) < 1e-6 and s[r, q] >= tau
    # only the second half may go: rows of the first half are kept and still shadow later copies
    half = ["id%d" % r for r in range(STORE_N // 2, STORE_N)]
    kept_half = jc.greedy_keep(s, tau, np.arange(STORE_N // 2, STORE_N))
    gone = store.deduplicate(tau, ids=half, mode="screen")
    assert gone == ["id%d" % r for r in np.flatnonzero(~kept_half)] and 0 < len(gone) < len(found)
    assert store.get()["ids"] == ["id%d" % r for r in np.flatnonzero(kept_half)]
    # then the whole store: what is left are the greedy survivors of what was left
    left_rows = np.flatnonzero(kept_half)
    kept_rest = jc.greedy_keep(s[np.ix_(left_rows, left_rows)], tau)
    gone = store.deduplicate(tau)
    survivors = ["id%d" % r for r in left_rows[kept_rest]]
    assert gone == ["id%d" % r for r in left_rows[~kept_rest]] and store.get()["ids"] == survivors
    assert store.deduplicate(tau) == [] and store.duplicate_scan(tau).counts.sum() == 0
    reloaded = HipChroma(dim=STORE_DIM, persist_directory=str(tmp_path))
    assert reloaded.get()["ids"] == survivors and reloaded.duplicate_scan(tau).counts.sum() == 0
    assert np.array_equal(reloaded._index.get(), rows[left_rows[kept_rest]])
