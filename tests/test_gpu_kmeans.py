"""K-means (K19, mq_index_kmeans) on the GPU against the float64 reference of kmeans_cases.py: bit
for bit on the exact class over the row counts, dims, cluster counts and masks (labels, dots,
counts, one update's centroids, out_info); through `check_assign` / `check_update` on the
near-duplicate corpora; composition of calls, convergence skipping, determinism and device I/O;
pinned trajectories and planted blobs; and the store's cluster / cluster_representatives."""
import numpy as np
import pytest
import torch

import kmeans_cases as kc
from mediquery_hip import ClusterResult, HipChroma
from mediquery_hip.native import FlatIndex, kmeans_scratch_bytes
from mediquery_hip.vectorstore import pick_representatives

pytestmark = pytest.mark.gpu

_cache = {}


def _index(kind, dim, n, *extra):
    """(index, stored rows); the exact class is stored bit for bit, the others are read back:
    the reference is computed from what the index holds."""
    key = (kind, dim, n) + extra
    if key not in _cache:
        if kind == "exact":
            rows = kc.exact_corpus(dim, n)
        elif kind == "random":
            rows = kc.neardup_corpus(dim, n)
        else:
            rows = kc.blob_corpus(dim, *extra)[0]
        ix = FlatIndex(dim=dim, device=0)
        ix.add(rows)
        stored = ix.get()
        if kind == "exact":
            assert np.array_equal(stored, rows)
        _cache[key] = (ix, stored)
    return _cache[key]


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # a copy: the cached corpora are read-only


def _bits(mask):
    return None if mask is None else _dev(kc.mask_words(mask))


def _i32(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("dim", kc.DIMS)
def test_exact_class_equals_reference(require_gpu, dim):
    seen = set()
    for ni, n in enumerate(kc.NS):
        ix, rows = _index("exact", dim, n)
        for ci, c in enumerate(kc.CLUSTERS):
            mk = kc.MASKS[(ni + ci) % len(kc.MASKS)]
            mask = kc.row_mask(mk, n)
            cents = kc.exact_centroids(dim, n, c)
            where = (dim, n, c, mk)
            lab, dots, d = kc.assign64(rows, cents, mask)
            counts = np.bincount(lab[lab >= 0], minlength=c)
            admitted = int((lab >= 0).sum())
            g_c, g_a, g_d, g_n, info = ix.kmeans(cents, 0, _bits(mask))
            assert np.array_equal(_i32(g_c), _i32(cents)), where
            assert np.array_equal(g_a, lab), where
            assert np.array_equal(_i32(g_d), _i32(dots)), where
            assert np.array_equal(g_n, counts), where
            changed0 = admitted  # against a_{-1} = -1
            assert info.tolist() == [0, changed0, admitted, int((counts == 0).sum())], (where, info)
            # one update: the sums are multiples of 1/4, exact in any order; one rounding
            u_c, u_a, u_d, u_n, uinfo = ix.kmeans(cents, 1, _bits(mask))
            want = kc.update64(rows, lab, cents)[0].astype(np.float32)
            assert np.array_equal(_i32(u_c), _i32(want)), where
            assert np.array_equal(_i32(u_c[counts == 0]), _i32(cents[counts == 0])), where
            assert np.array_equal(u_n, np.bincount(u_a[u_a >= 0], minlength=c)), where
            assert np.array_equal(u_a >= 0, lab >= 0), where
            assert uinfo.tolist() == [int(admitted > 0), int((u_a != lab).sum()), admitted,
                                      int((u_n == 0).sum())], (where, uinfo)
            seen.add(("mask", mk))
            if c > 1 and admitted:
                top = np.sort(d[lab >= 0], axis=1)
                if (top[:, -1] == top[:, -2]).any():
                    seen.add("tie")
            if admitted and (counts == 0).any():
                seen.add("empty")
            if c > 16 and admitted:
                seen.add("passes")
            if c > admitted > 0:
                seen.add("surplus")
    assert all(("mask", mk) in seen for mk in kc.MASKS)
    assert {"tie", "empty", "passes", "surplus"} <= seen


@pytest.mark.parametrize("dim,n,c", kc.RANDOM_CASES)
def test_random_class_one_step(require_gpu, dim, n, c):
    ix, rows = _index("random", dim, n)
    for mk in ("none", "third"):
        mask = kc.row_mask(mk, n)
        adm = np.arange(n) if mask is None else np.flatnonzero(mask)
        cents = rows[kc.random_centroid_rows(dim, n, c, adm)]
        g_c, g_a, g_d, g_n, info = ix.kmeans(cents, 0, _bits(mask))
        fails, und = kc.check_assign(g_a, g_d, rows, cents, mask, dim)
        assert not fails, (mk, fails[:3])
        assert und.sum() <= kc.NEAR_TIE_CAP * len(adm)
        assert np.array_equal(g_n, np.bincount(g_a[g_a >= 0], minlength=c)) and info[2] == len(adm)
        u_c = ix.kmeans(cents, 1, _bits(mask))[0]
        fails = kc.check_update(u_c, rows, g_a, cents)
        assert not fails, (mk, fails[:3])


def _same(a, b, where, info_from=2):
    for x, y, name in zip(a[:4], b[:4], ("centroids", "assign", "dots", "counts")):
        x, y = (_i32(x), _i32(y)) if x.dtype == np.float32 else (x, y)
        assert np.array_equal(x, y), (where, name)
    assert a[4].tolist()[info_from:] == b[4].tolist()[info_from:], (where, a[4], b[4])


@pytest.mark.parametrize("dim,n,c", ((256, 1000, 16), (768, 700, 33)))
def test_composition_convergence_determinism_and_device_io(require_gpu, dim, n, c):
    ix, rows = _index("random", dim, n)
    scratch = torch.empty(kmeans_scratch_bytes(n, c), dtype=torch.uint8, device="cuda")
    for mk in ("none", "third"):
        mask = kc.row_mask(mk, n)
        bits = _bits(mask)
        adm = np.arange(n) if mask is None else np.flatnonzero(mask)
        cents = rows[kc.random_centroid_rows(dim, n, c, adm)]
        for T in (2, 5):
            whole = ix.kmeans(cents, T, bits, scratch)
            step = (cents,)
            for _ in range(T):
                step = ix.kmeans(step[0], 1, bits, scratch)
            _same(whole, step, (mk, T))
            assert whole[4][0] == T or whole[4][1] == 0
        # past convergence nothing moves and the update count stops growing
        done = ix.kmeans(cents, 100, bits, scratch)
        assert done[4][1] == 0 and 1 <= done[4][0] < 100
        more = ix.kmeans(cents, 300, bits, scratch)
        _same(done, more, (mk, "past convergence"), info_from=0)
        again = ix.kmeans(done[0], 3, bits, scratch)
        _same(done, again, (mk, "from the converged centres"))
        assert again[4].tolist()[:2] == [1, 0]
        # identical calls, a dirty scratch, device I/O
        first = ix.kmeans(cents, 3, bits, scratch)
        scratch.fill_(0xA5)
        second = ix.kmeans(cents, 3, bits, scratch)
        _same(first, second, (mk, "repeat"), info_from=0)
        d_c = _dev(cents)
        outs = (torch.empty(n, dtype=torch.int32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda"),
                torch.empty(c, dtype=torch.int64, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda"))
        ix.kmeans_device(d_c, 3, *outs, bits=bits, scratch=scratch)
        torch.cuda.synchronize()
        _same(first, (d_c.cpu().numpy(),) + tuple(o.cpu().numpy() for o in outs), (mk, "device"), info_from=0)


def test_empty_index_and_all_zero_mask(require_gpu):
    empty = FlatIndex(dim=256, device=0)
    cents = kc.exact_centroids(256, 65, 5)
    c, a, d, counts, info = empty.kmeans(cents, 4)
    assert np.array_equal(_i32(c), _i32(cents)) and len(a) == len(d) == 0
    assert counts.tolist() == [0] * 5 and info.tolist() == [0, 0, 0, 5]
    outs = (torch.empty(0, dtype=torch.int32, device="cuda"), torch.empty(0, device="cuda"),
            torch.full((5,), 7, dtype=torch.int64, device="cuda"), torch.full((4,), 7, dtype=torch.int64, device="cuda"))
    empty.kmeans_device(_dev(cents), 4, *outs)
    assert outs[2].cpu().tolist() == [0] * 5 and outs[3].cpu().tolist() == [0, 0, 0, 5]
    ix, rows = _index("exact", 256, 65)
    c, a, d, counts, info = ix.kmeans(cents, 4, _bits(kc.row_mask("zeros", 65)))
    assert np.array_equal(_i32(c), _i32(cents)) and (a == -1).all() and np.isneginf(d).all()
    assert counts.tolist() == [0] * 5 and info.tolist() == [0, 0, 0, 5]
    with pytest.raises(ValueError, match="centroids must be finite"):
        ix.kmeans(np.full((2, 256), np.nan, np.float32), 1)
    # device centroids that are not finite: labels stay in range
    bad = torch.full((3, 256), float("nan"), device="cuda")
    outs = (torch.empty(65, dtype=torch.int32, device="cuda"), torch.empty(65, device="cuda"),
            torch.empty(3, dtype=torch.int64, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda"))
    ix.kmeans_device(bad, 0, *outs)
    lab = outs[0].cpu().numpy()
    assert ((lab >= 0) & (lab < 3)).all() and outs[2].cpu().sum() == 65


@pytest.mark.parametrize("case", kc.TRAJECTORY_CASES)
def test_trajectory_equals_the_reference(require_gpu, case):
    dim, blobs, per, sigma, cs, sd = case
    ix, rows = _index("blobs", dim, blobs * per, blobs, per, sigma, cs)
    init = rows[kc.trajectory_seeds(len(rows), blobs, sd)]
    r_c, r_lab, r_updates, r_conv, margins = kc.lloyd64(rows, init, None, 30)
    assert r_conv and r_updates >= 3 and min(margins) >= kc.TRAJECTORY_MARGIN * kc.bprime(dim)
    c, a, d, counts, info = ix.kmeans(init, 30)
    assert np.array_equal(a, r_lab) and info[0] == r_updates and info[1] == 0
    assert np.array_equal(counts, np.bincount(r_lab, minlength=blobs))
    assert np.abs(c.astype(np.float64) - r_c).max() <= (per * blobs + 2) * 2.0 ** -24


@pytest.mark.parametrize("dim,blobs,per", kc.PLANTED_CASES)
def test_planted_blobs_are_recovered_and_the_objective_never_rises(require_gpu, dim, blobs, per):
    ix, rows = _index("blobs", dim, blobs * per, blobs, per, kc.PLANTED_SIGMA, 0)
    planted = kc.blob_corpus(dim, blobs, per, kc.PLANTED_SIGMA)[1]
    init = rows[kc.planted_seeds(planted, blobs)]
    c, a, d, counts, info = ix.kmeans(init, 20)
    assert np.array_equal(a, planted) and info[1] == 0 and counts.tolist() == [per] * blobs
    n = len(rows)
    step = ix.kmeans(init, 0)
    prev = kc.objective64(rows, step[0], step[1])
    for _ in range(4):
        step = ix.kmeans(step[0], 1)
        j = kc.objective64(rows, step[0], step[1])
        assert j <= prev + 8 * n * kc.bprime(dim)
        prev = j


# ----------------------------------------------------------------------- the store ----
STORE_DIM, STORE_BLOBS, STORE_PER = kc.STORE_CASE
STORE_N = STORE_BLOBS * STORE_PER


def _store(tmp=None):
    rows = kc.blob_corpus(STORE_DIM, STORE_BLOBS, STORE_PER, kc.PLANTED_SIGMA)[0]
    store = HipChroma(dim=STORE_DIM, persist_directory=tmp, auto_persist=tmp is not None)
    store.add_embeddings(rows, ["row %d is %s" % (r, "odd" if r % 2 else "even") for r in range(STORE_N)],
                         [{"tag": r % 3} for r in range(STORE_N)], ["id%d" % r for r in range(STORE_N)])
    return store, store._index.get()


def _check_result(res, rows, adm, n_clusters):
    """A ClusterResult against the float64 definition on its own centroids."""
    assert isinstance(res, ClusterResult) and res.ids == ["id%d" % r for r in adm] and len(res) == len(adm)
    assert res.labels.dtype == np.int32 and res.centroids.shape == (n_clusters, STORE_DIM)
    fails, und = kc.check_assign(res.labels, None, rows[adm], res.centroids, None, STORE_DIM)
    assert not fails, fails[:3]
    assert np.array_equal(res.counts, np.bincount(res.labels, minlength=n_clusters))
    # per row: two fp32 dots' worth of error and the row's own norm, unit to fp32 rounding
    tol = len(adm) * (2 * kc.bound(STORE_DIM) + 2.0 ** -22)
    assert abs(res.inertia - kc.objective64(rows[adm], res.centroids, res.labels)) <= tol


def test_store_cluster_masks_inits_and_errors(require_gpu):
    store, rows = _store()
    planted = kc.blob_corpus(STORE_DIM, STORE_BLOBS, STORE_PER, kc.PLANTED_SIGMA)[1]
    every = np.arange(STORE_N)
    res = store.cluster(STORE_BLOBS)
    _check_result(res, rows, every, STORE_BLOBS)
    assert res.converged and res.iterations >= 1
    again = store.cluster(STORE_BLOBS)
    assert np.array_equal(res.labels, again.labels) and np.array_equal(_i32(res.centroids), _i32(again.centroids))
    ids = ["id%d" % r for r in range(5, STORE_N, 2)]
    for kw, adm in (({"filter": {"tag": 0}}, every[every % 3 == 0]),
                    ({"where_document": {"$contains": "even"}}, every[every % 2 == 0]),
                    ({"ids": ids}, every[5::2]),
                    ({"ids": ids, "filter": {"tag": 1}, "where_document": {"$contains": "odd"}},
                     every[(every % 3 == 1) & (every % 2 == 1) & (every >= 5)])):
        for init in ("k-means++", "random"):
            res = store.cluster(4, init=init, seed=3, **kw)
            _check_result(res, rows, adm, 4)
            same = store.cluster(4, init=init, seed=3, **kw)
            assert np.array_equal(res.labels, same.labels) and res.inertia == same.inertia
            # the seeds are distinct admitted rows: with max_iter = 0 the centres are those rows
            seeds = store.cluster(4, max_iter=0, init=init, seed=3, **kw)
            at = [np.flatnonzero((rows == c).all(1)) for c in seeds.centroids]
            assert all(len(a) == 1 and a[0] in adm for a in at) and len({int(a[0]) for a in at}) == 4
            assert seeds.iterations == 0
    # random: the rows default_rng(seed).choice picks
    seeds = store.cluster(4, max_iter=0, init="random", seed=11, ids=ids)
    want = np.random.default_rng(11).choice(every[5::2], 4, replace=False)
    assert np.array_equal(_i32(seeds.centroids), _i32(rows[want]))
    # max_iter = 0 with given centres labels the rows against them
    centres = rows[kc.planted_seeds(planted, STORE_BLOBS)]
    pred = store.cluster(STORE_BLOBS, max_iter=0, init=centres)
    assert np.array_equal(pred.labels, kc.assign64(rows, centres)[0]) and pred.iterations == 0
    assert np.array_equal(_i32(pred.centroids), _i32(centres))
    full = store.cluster(STORE_BLOBS, init=centres)
    assert np.array_equal(full.labels, planted) and full.converged
    with pytest.raises(ValueError, match="n_clusters=4 exceeds the 3 rows the filters admit"):
        store.cluster(4, ids=["id1", "id2", "id3", "nope"])
    with pytest.raises(ValueError, match="n_clusters=101 exceeds the 100 rows"):
        store.cluster(101, filter={"tag": 2})


def test_store_cluster_representatives_against_a_float64_ranking(require_gpu):
    """A small store whose rankings have no near-tie among the entries that matter
    (kmeans_cases.ranking_gap; test_kmeans_cases.py holds the generated rows to it too)."""
    dim, blobs, per, sigma = kc.REP_CASE
    n = blobs * per
    raw, planted = kc.blob_corpus(dim, blobs, per, sigma)
    store = HipChroma(dim=dim, auto_persist=False)
    store.add_embeddings(raw, ["row %d" % r for r in range(n)], [{"tag": r % 3} for r in range(n)],
                         ["id%d" % r for r in range(n)])
    rows = store._index.get()
    centres = rows[kc.planted_seeds(planted, blobs)]
    every = np.arange(n)
    for kw, adm in (({}, every), ({"filter": {"tag": 0}}, every[every % 3 == 0]), ({"max_iter": 0}, every)):
        res = store.cluster(blobs, init=centres, **kw)
        for num_closest, rd, srt in ((1, False, False), (3, False, True), (2, True, False), (3, True, True)):
            docs = store.cluster_representatives(blobs, num_closest, srt, rd, init=centres, **kw)
            hits = min(blobs * num_closest, len(adm))
            assert kc.ranking_gap(rows[adm], res.centroids, hits) > 2 * kc.bound(dim)
            s = kc.d64(rows[adm], res.centroids)[0].T  # [c, admitted]
            rankings = [adm[np.argsort(-s[j], kind="stable")] for j in range(blobs)]
            want = pick_representatives(rankings, num_closest, rd, srt)
            assert [d.id for d in docs] == ["id%d" % r for r in want], (kw, num_closest, rd, srt)
            assert len(docs) <= blobs * num_closest and (rd or len(docs) == hits)
    big = HipChroma(dim=64, auto_persist=False)
    big.add_embeddings(kc.neardup_corpus(64, 5000), ["t"] * 5000, [{} for _ in range(5000)],
                       ["i%d" % r for r in range(5000)])
    with pytest.raises(ValueError, match="MQ_RANGE_MAX_HITS"):
        big.cluster_representatives(100, 50, init="random", max_iter=2)


def test_store_cluster_persisted_reloaded_and_after_delete(require_gpu, tmp_path):
    store, rows = _store(str(tmp_path))
    planted = kc.blob_corpus(STORE_DIM, STORE_BLOBS, STORE_PER, kc.PLANTED_SIGMA)[1]
    centres = rows[kc.planted_seeds(planted, STORE_BLOBS)]
    every = np.arange(STORE_N)
    first = store.cluster(STORE_BLOBS, seed=2)
    reloaded = HipChroma(dim=STORE_DIM, persist_directory=str(tmp_path))
    back = reloaded.cluster(STORE_BLOBS, seed=2)
    assert back.ids == first.ids and np.array_equal(back.labels, first.labels)
    assert np.array_equal(_i32(back.centroids), _i32(first.centroids)) and back.inertia == first.inertia
    # after a delete the rows are renumbered: ids and labels follow
    gone = ["id%d" % r for r in range(0, STORE_N, 4)]
    store.delete(gone)
    keep = every[every % 4 != 0]
    res = store.cluster(STORE_BLOBS, init=centres)
    assert res.ids == ["id%d" % r for r in keep] and np.array_equal(res.labels, planted[keep])
    docs = store.cluster_representatives(STORE_BLOBS, 1, init=centres)
    # one surviving member of each blob, in cluster order
    assert len(docs) == STORE_BLOBS
    for g, d in enumerate(docs):
        assert planted[int(d.id[2:])] == g and int(d.id[2:]) % 4 != 0
