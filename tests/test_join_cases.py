"""The self-join's test material, checked on the CPU from the reference alone: the vectorised
float64 reference equals the plain loop, every random case keeps its undecided rows inside the
cap (the margin between a row's two best partners included), the random cases hold pairs that
pass the bf16 screen's threshold and fail the exact one, and the greedy rule's restatement in
rounds equals the loop."""
import numpy as np
import pytest

import join_cases as jc


@pytest.mark.parametrize("kind", jc.MASKS)
@pytest.mark.parametrize("left_kind", jc.LEFTS)
def test_reference_equals_loop_exact_class(kind, left_kind):
    n = 65
    rows = jc.exact_corpus(64, n)
    left, mask = jc.left_rows(left_kind, n), jc.row_mask(kind, n)
    s = jc.scores64(rows, left)
    for min_score in jc.MIN_SCORES:
        c, f, nn, sc = jc.join_reference(s, left, mask, min_score)
        for p, i in enumerate(range(n) if left is None else left.tolist()):
            assert (c[p], f[p], nn[p], sc[p]) == jc.reference_by_loop(s[p], i, mask, min_score), (p, min_score)
    # repeated rows give exact ties: some left row's nearest is a copy of it, found at the lowest row
    c, f, nn, sc = jc.join_reference(jc.scores64(rows), None, None, 1.0)
    assert c.max() >= 1 and (sc[c > 0] == 1.0).all() and (nn[c > 0] == f[c > 0]).all()


def test_reference_equals_loop_random_class():
    rows = jc.neardup_corpus(64, 300)
    s = jc.scores64(rows)
    mask = jc.row_mask("third", 300)
    for min_score in jc.RANDOM_MIN_SCORES:
        for m in (None, mask):
            c, f, nn, sc = jc.join_reference(s, None, m, min_score)
            for i in range(300):
                assert (c[i], f[i], nn[i], sc[i]) == jc.reference_by_loop(s[i], i, m, min_score)


def test_minus_zero_threshold_is_zero():
    s = np.array([[1.0, -0.0, 0.0], [-0.0, 1.0, -1.0], [0.0, -1.0, 1.0]]) + 0.0
    for tau in (-0.0, 0.0):
        c, f, nn, sc = jc.join_reference(s, None, None, tau)
        assert c.tolist() == [2, 1, 1] and f.tolist() == [1, 0, 0] and nn.tolist() == [1, 0, 0]


@pytest.mark.parametrize("dim,n", jc.RANDOM_SHAPES)
def test_random_cases_inside_the_cap_and_exercise_the_verification(dim, n):
    rows = jc.neardup_corpus(dim, n)
    assert np.abs(np.linalg.norm(rows.astype(np.float64), axis=1) - 1).max() < 1e-6
    s = jc.scores64(rows)
    for min_score in jc.RANDOM_MIN_SCORES:
        und = jc.undecided_rows(s, None, None, min_score, dim)
        assert und.mean() <= jc.NEAR_TIE_CAP, (min_score, int(und.sum()))
        counts = jc.join_reference(s, None, None, min_score)[0]
        assert counts.sum() >= n // 4 and counts.max() <= 64      # partners exist, lists stay short
        assert jc.screen_only_pairs(rows, s, min_score, dim) >= 16  # the verify step has pairs to drop
    # the cosines straddle the thresholds: some pairs of a family pass 0.95, some fail 0.8
    c80, c95 = (jc.join_reference(s, None, None, t)[0].sum() for t in (0.8, 0.95))
    assert 0 < c95 < c80


def test_bf16_rounding_restated():
    x = np.array([1.0, 1.00390625, 1.01171875, -0.25, 3.0e-5], np.float32)  # 1 + 2^-8 ties to even, 1 + 3 2^-8 up
    assert jc.to_bf16(x).tolist()[:4] == [1.0, 1.0, 1.015625, -0.25]
    rows = jc.exact_corpus(256, 50)
    assert np.array_equal(jc.to_bf16(rows), rows)  # the exact class survives bf16


@pytest.mark.parametrize("case", ("chain3", "chain6", "neardup", "neardup_left", "neardup_masked"))
def test_greedy_rounds_restated(case):
    """join_cases.numpy_scan_first and greedy_keep agree through the store's round logic; the
    cases themselves are test_join_host.py's."""
    from mediquery_hip.vectorstore import greedy_dedup_rounds
    rows = jc.neardup_corpus(64, 400)
    s, tau, left, mask = jc.scores64(rows), 0.9, None, None
    if case == "chain3":
        s, tau = np.array([[1, .95, .5], [.95, 1, .95], [.5, .95, 1]]), 0.9
    elif case == "chain6":
        s = np.eye(6) + 0.95 * (np.eye(6, k=1) + np.eye(6, k=-1))
    elif case == "neardup_left":
        left = np.arange(200, 400, dtype=np.int64)
    elif case == "neardup_masked":
        mask = jc.row_mask("third", 400)
    n = s.shape[0]
    dropped, keepers, und, rounds = greedy_dedup_rounds(
        n, np.arange(n) if left is None else left, np.ones(n, bool) if mask is None else mask,
        jc.numpy_scan_first(s, tau))
    kept = jc.greedy_keep(s, tau, left, mask)
    assert np.array_equal(dropped, np.flatnonzero(~kept)) and len(und) == 0 and rounds >= 1
    assert (keepers < dropped).all() and kept[keepers].all() and (s[dropped, keepers] >= tau).all()
