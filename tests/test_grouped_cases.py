"""The grouped search's float64 reference on hand-made cases, its agreement with LangChain's
collapse of a full ranking, the store's certificate (`collapse_candidates`), and the near-tie
share of the random-class cases the GPU test uses (tests/grouped_cases.py).  No GPU."""
import numpy as np
import pytest

import grouped_cases as gc
from mediquery_hip import _lib
from mediquery_hip.vectorstore import collapse_candidates


def _unit(*pairs, dim=8):
    v = np.zeros(dim)
    for i, x in pairs:
        v[i] = x
    return v


def test_reference_on_a_hand_made_case():
    q = _unit((0, 1.0))
    rows = np.stack([_unit((0, 0.5)),    # 0: group 2, 0.5
                     _unit((0, 0.9)),    # 1: group 0, 0.9
                     _unit((0, 0.9)),    # 2: group 0, 0.9 again: the lower row represents
                     _unit((0, 0.7)),    # 3: group 1
                     _unit((0, 0.95)),   # 4: key absent: ignored though it scores best
                     _unit((0, 0.9)),    # 5: group 3 ties with group 0: row 1 < row 5
                     _unit((0, -0.2)),   # 6: group 2 again, worse
                     _unit((0, 0.99))])  # 7: code out of range (n_groups = 4): ignored
    codes = np.array([2, 0, 0, 1, -1, 3, 2, 9], np.int32)
    s, i = gc.grouped_reference(rows, q, codes, None, 6, n_groups=4)
    assert i.tolist() == [[1, 5, 3, 0, -1, -1]]
    assert s[0, :4].tolist() == [0.9, 0.9, 0.7, 0.5] and np.isneginf(s[0, 4:]).all()
    # n_groups None: every non-negative code counts, so row 7 leads
    assert gc.grouped_reference(rows, q, codes, None, 2)[1].tolist() == [[7, 1]]
    # the mask takes row 1 out: row 2 represents group 0 and still beats row 5 on the id
    mask = np.ones(8, bool)
    mask[1] = False
    assert gc.grouped_reference(rows, q, codes, mask, 3, n_groups=4)[1].tolist() == [[2, 5, 3]]
    # a group whose only rows are masked out disappears; k = 1
    mask[:] = False
    mask[[0, 6, 4]] = True
    s, i = gc.grouped_reference(rows, q, codes, mask, 2, n_groups=4)
    assert i.tolist() == [[0, -1]] and s[0, 0] == 0.5
    # nothing admitted, and an empty corpus: padding only
    assert gc.grouped_reference(rows, q, codes, np.zeros(8, bool), 3, 4)[1].tolist() == [[-1, -1, -1]]
    assert gc.grouped_reference(np.zeros((0, 8)), q, np.zeros(0, np.int32), None, 2, 0)[1].tolist() == [[-1, -1]]
    # negative scores rank below zero ones, two queries at once
    s, i = gc.grouped_reference(rows, np.stack([q, -q]), codes, None, 4, n_groups=4)
    assert i[1].tolist() == [6, 3, 1, 5] and s[1].tolist() == [0.2, -0.7, -0.9, -0.9]


@pytest.mark.parametrize("layout", gc.LAYOUTS)
def test_reference_equals_the_loop_and_langchains_collapse(layout):
    """Three statements of one definition: the vectorised reference, the per-row loop
    (group maximum, lowest row on ties, groups by (score desc, row asc)) and the distinct codes
    of the full ranking in order - on the exact class, where ties abound, and the random one."""
    for kind, dim, n in (("exact", 64, 1000), ("exact", 256, 65), ("random", 64, 400)):
        rows = gc.exact_corpus(dim, n) if kind == "exact" else gc.random_corpus(dim, n)
        qs = gc.exact_queries(dim, 5) if kind == "exact" else gc.random_queries(dim, 5)
        codes, n_groups = gc.group_codes(layout, n)
        s_all = gc.dots64(rows, qs)
        for mk in gc.MASKS:
            mask = gc.row_mask(mk, n)
            ok = gc.candidates(codes, mask, n_groups)
            for k in (1, 5, 64):
                ref_s, ref_i = gc.grouped_reference(rows, qs, codes, mask, k, n_groups)
                for j in range(len(qs)):
                    loop = gc.reference_by_loop(s_all[j], codes, ok, k)
                    full = gc.collapse_full_ranking(s_all[j], codes, ok)
                    assert loop == full[:k], (kind, layout, mk, k, j)
                    got = [(x, int(r)) for x, r in zip(ref_s[j], ref_i[j]) if r >= 0]
                    assert got == loop, (kind, layout, mk, k, j)
                    assert (ref_i[j] >= 0).sum() == min(k, len(full))
                    if kind == "exact":  # multiples of 1/16: fp32 holds every score exactly
                        assert np.array_equal(ref_s[j] * 16, np.round(ref_s[j] * 16))


def test_exact_class_is_exact_and_ties():
    for dim in (64, 256, 768, 1024):
        rows, q = gc.exact_corpus(dim, 200), gc.exact_queries(dim, 8)
        for v in (rows, q):
            assert np.all((v != 0).sum(1) == 16) and set(np.unique(np.abs(v))) == {0.0, 0.25}
        s = gc.dots64(rows, q)
        assert np.array_equal(s * 16, np.round(s * 16)) and np.abs(s).max() <= 1
        assert np.array_equal((q @ rows.T).astype(np.float64), s)  # fp32, BLAS's order: the same values
        assert len(np.unique(rows, axis=0)) < len(rows)               # duplicate rows
        assert len(np.unique(s[0])) < 40                              # few distinct scores: ties
        assert np.flatnonzero(rows.any(0)).max() >= dim // 2           # the non-zeros reach the row's far half


def test_layouts_and_masks():
    for n in (1, 17, 1000):
        for layout in gc.LAYOUTS:
            codes, g = gc.group_codes(layout, n)
            assert codes.dtype == np.int32 and codes.shape == (n,) and g >= 1
            inside = codes[(codes >= 0) & (codes < g)]
            assert inside.size == 0 or inside.max() < g
        assert gc.group_codes("singletons", n)[1] == n and gc.group_codes("one", n)[1] == 1
    codes, g = gc.group_codes("sprinkled", 1000)
    assert (codes == -1).any() and (codes == g + 3).any() and (codes == -7).any() and (codes == 2 ** 31 - 1).any()
    sizes = np.bincount(gc.group_codes("families", 4097)[0])
    assert sizes.min() >= 1 and sizes.max() <= 100 and sizes.max() > 64
    m = gc.row_mask("third", 70)
    w = gc.mask_words(m)
    assert w.dtype == np.int32 and w.size == 3
    assert [(int(w[r >> 5]) >> (r & 31)) & 1 for r in range(70)] == m.astype(int).tolist()
    assert gc.row_mask("none", 5) is None and gc.row_mask("single", 9).sum() == 1 and not gc.row_mask("zeros", 9).any()


# ------------------------------------------------------------- the certificate ----
def _lst(ids, n=64):
    ids = list(ids) + [-1] * (n - len(ids))
    return np.array(ids, np.int64), np.linspace(1.0, 0.0, n).astype(np.float32)


def test_collapse_keeps_order_and_skips_absent_codes():
    codes = np.array([0, 0, 1, -1, 2, 1, 3, -1], np.int32)
    ids, s = _lst([3, 1, 0, 5, 7, 2, 4, 6], n=8)
    rows, sc, cert = collapse_candidates(ids, s, codes, 3)
    assert rows == [1, 5, 4] and cert           # rows 3, 7: no key; 0, 2: their group was seen
    assert sc == [float(s[1]), float(s[3]), float(s[6])]
    assert collapse_candidates(ids, s, codes, 10)[0] == [1, 5, 4, 6]
    assert collapse_candidates(ids, s, codes, 1)[0] == [1]


def test_collapse_certifies_exactly_when_k_groups_or_a_short_list():
    full = _lib.MQ_MAX_K
    codes = np.repeat(np.arange(10), 20).astype(np.int32)  # 10 groups of 20 rows
    # a full list of one group's rows and 3 more groups: 4 distinct groups
    ids, s = _lst(list(range(20)) + list(range(20, 40)) + list(range(40, 60)) + list(range(60, 64)))
    assert len(ids) == full
    for k in range(1, 8):
        rows, _, cert = collapse_candidates(ids, s, codes, k)
        assert cert == (k <= 4), k
        assert rows == [0, 20, 40, 60][:k]
    # one entry short of full: every candidate was seen, so any k is certified
    short_ids, short_s = ids.copy(), s.copy()
    short_ids[-1] = -1
    for k in (1, 4, 5, 64):
        rows, _, cert = collapse_candidates(short_ids, short_s, codes, k)
        assert cert and rows == [0, 20, 40, 60][:k]
    # absent codes fill the list but are no groups
    codes2 = codes.copy()
    codes2[20:] = -1
    assert collapse_candidates(ids, s, codes2, 1) == ([0], [1.0], True)
    assert collapse_candidates(ids, s, codes2, 2)[2] is False
    # an empty list certifies an empty answer
    e_ids, e_s = _lst([])
    assert collapse_candidates(e_ids, e_s, codes, 5) == ([], [], True)


def test_certified_answers_equal_the_reference():
    """On the exact class (ties everywhere): whenever the float64 top-64 certifies, its
    collapse is the reference's top-k; some queries certify and some do not."""
    dim, n = 64, 1000
    rows, qs = gc.exact_corpus(dim, n), gc.exact_queries(dim, 12)
    s_all = gc.dots64(rows, qs)
    seen = set()
    for layout in ("families", "interleaved", "sprinkled", "one"):
        codes, n_groups = gc.group_codes(layout, n)
        host = np.where((codes >= 0) & (codes < n_groups), codes, -1)
        for k in (1, 5, 40):
            ref_s, ref_i = gc.grouped_reference(rows, qs, codes, None, k, n_groups)
            for j in range(len(qs)):
                order = np.lexsort((np.arange(n), -s_all[j]))[:64]
                got_rows, got_s, cert = collapse_candidates(order, s_all[j][order], host, k)
                seen.add(cert)
                if cert:
                    want = [int(r) for r in ref_i[j] if r >= 0]
                    assert got_rows == want and got_s == ref_s[j][:len(want)].tolist(), (layout, k, j)
    assert seen == {True, False}


# ------------------------------------------------- the random class's near-ties ----
@pytest.mark.parametrize("case", gc.RANDOM_CASES)
def test_random_cases_stay_inside_the_near_tie_cap(case):
    dim, n, layout, mk, nq, seed = case
    rows, qs = gc.random_corpus(dim, n, seed), gc.random_queries(dim, nq, seed)
    codes, n_groups = gc.group_codes(layout, n, seed)
    mask = gc.row_mask(mk, n)
    ok = gc.candidates(codes, mask, n_groups)
    s_all = gc.dots64(rows, qs)
    near = positions = 0
    for k in gc.RANDOM_KS:
        ref_s, ref_i = gc.grouped_reference(rows, qs, codes, mask, k, n_groups)
        near += sum(int(gc.near_tie_positions(s_all[j], codes, ok, ref_s[j], ref_i[j], 2 * gc.bound(dim)).sum())
                    for j in range(nq))
        positions += nq * k
        # the reference checks itself clean
        for j in range(nq):
            fails, _ = gc.check_random(ref_s[j].astype(np.float32), ref_i[j], s_all[j], codes, ok, ref_s[j], ref_i[j],
                                       dim)
            assert fails == [], (case, k, j, fails)
    assert near <= gc.NEAR_TIE_CAP * positions, (case, near, positions)
