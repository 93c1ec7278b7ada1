"""The reference, the path model, the cases and the checkers of the top-k merge tests
(test_merge_cases.py on the CPU, test_gpu_merge.py on the GPU).  A plain module.

The definition (include/mq.h, mq_topk_merge_host / mq_topk_merge_device): the entries of a
query are those of its lists [n_lists, nq, k_in] with id >= 0; they rank by (score desc with
-0.0 == +0.0, id asc as unsigned); the result is the first k_out, padded with (-inf, -1).
`merge_reference` states exactly that as a plain sort.  Scores are copied, never computed, so
every comparison is exact: ids equal, scores bitwise equal up to the sign of zero
(`same_scores`).  No tolerance exists anywhere.  No case holds a NaN or repeats a valid id
within a query: both are outside the contract.

The device merge (K10, csrc/index.hip) is three paths; `path_model` restates which one a
query takes, from the shape and the data alone:
  * the thread-list kernel iff k_out <= 16 and nq > 32 (or form 1);
  * the threshold kernel otherwise, which falls back to the thread lists iff n_lists >
    256 * SEL_HEADS, or iff more than SEL_CAP entries survive its threshold T: wave w holds
    the heads of the lists with (lst % 256) // 64 == w, T_w is its k_out-th largest valid
    head key (0 if it has fewer), T = max T_w, and the survivors are each list's sorted
    prefix with key >= max(T, 1).  T == 0 admits every valid entry.

The overflow flag (`bit0_expected`, `bit1_possible`), with Tr the truncated lists given to
the kernel and kth the k_out-th entry of merge_reference(Tr), (-inf, -1) when fewer exist:
  * bit 0: some list has a valid entry at position list_kc - 1 that is better than kth;
  * bit 1 is possible only if kc < k_out and some thread t (lists t, t + 256, ...) holds at
    least kc valid entries whose kc-th best is better than kth.
"""
import functools

import numpy as np

SEL_CAP = 2048     # kSelCap of csrc/index.hip (test_merge_cases.py reads both from the source)
SEL_HEADS = 16     # kSelHeads
MAX_K = 64         # MQ_MAX_K
U64 = (1 << 64) - 1
FULL = 64          # the length of the full lists F that the overflow cases truncate

N_LISTS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096, 4097)
NQS = (1, 2, 32, 33, 70)
K_INS = (1, 5, 8, 9, 16, 17, 64)
K_OUTS = (1, 5, 8, 9, 16, 17, 50, 64)
MAX_ELEMS = 1 << 19    # per case, well inside the 2^22 that keeps a case at milliseconds


# ---------------------------------------------------------------- the definition ----
def better(sa, ia, sb, ib):
    """(score desc, id asc as unsigned): the ordering of every retrieval result."""
    return bool(sa > sb or (sa == sb and (int(ia) & U64) < (int(ib) & U64)))


def merge_reference(scores, ids, k):
    """scores float32 / ids int32 or int64 [n_lists, nq, k_in] -> (float32 [nq, k], int64 [nq, k])."""
    scores, ids = np.asarray(scores, np.float32), np.asarray(ids)
    n_lists, nq, k_in = scores.shape
    out_s = np.full((nq, k), -np.inf, np.float32)
    out_i = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        s, i = scores[:, q, :].ravel(), ids[:, q, :].ravel().astype(np.int64)
        s, i = s[i >= 0], i[i >= 0]
        order = np.lexsort((i.astype(np.uint64), -(s.astype(np.float64) + 0.0)))[:k]
        out_s[q, :len(order)] = s[order]
        out_i[q, :len(order)] = i[order]
    return out_s, out_i


def reference_by_insertion(scores, ids, k):
    """One query [n_lists, k_in], by a loop that inserts each valid entry into a ranked list
    -> [(score, id)] of at most k entries."""
    top = []
    for l in range(scores.shape[0]):
        for j in range(scores.shape[1]):
            if ids[l, j] < 0:
                continue
            x = (float(scores[l, j]), int(ids[l, j]))
            at = len(top)
            while at > 0 and better(x[0], x[1], top[at - 1][0], top[at - 1][1]):
                at -= 1
            top.insert(at, x)
            del top[k:]
    return top


def same_scores(a, b):
    """Bitwise equal up to the sign of zero, elementwise."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | ((a == 0) & (b == 0))


def mismatch(got_s, got_i, ref_s, ref_i):
    """-> '' when (got_s, got_i) is the reference, else a line naming the first difference."""
    got_s, got_i = np.asarray(got_s), np.asarray(got_i)
    bad = (got_i != ref_i) | ~same_scores(got_s, ref_s)
    if not bad.any():
        return ""
    q, r = np.argwhere(bad)[0]
    return "query %d rank %d: got (%r, %d), reference (%r, %d); %d slots differ" % (
        q, r, float(got_s[q, r]), got_i[q, r], float(ref_s[q, r]), ref_i[q, r], int(bad.sum()))


# ------------------------------------------------------------------ the path model ----
def kc_merge(k_out):
    return 8 if k_out <= 8 else (16 if k_out <= 16 else 64)


def score_key(s):
    """The threshold kernel's order-preserving key of a score, > 0; -0.0 keys as +0.0."""
    b = (np.asarray(s, np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(b & 0x80000000, ~b, b | 0x80000000).astype(np.uint32)


def path_model(scores, ids, k_out, form=0):
    """-> one dict per query: path ('threadlist' | 'select' | 'fallback_lists' |
    'fallback_survivors'), T, survivors (None where no threshold is computed)."""
    n_lists, nq, k_in = scores.shape
    if form == 1 or (form == 0 and k_out <= 16 and nq > 32):
        return [dict(path="threadlist", T=None, survivors=None) for _ in range(nq)]
    if n_lists > 256 * SEL_HEADS:
        return [dict(path="fallback_lists", T=None, survivors=None) for _ in range(nq)]
    valid = np.asarray(ids) >= 0
    key = np.where(valid, score_key(scores), 0).astype(np.int64)
    wave = (np.arange(n_lists) % 256) // 64
    out = []
    for q in range(nq):
        T = 0
        for w in range(4):
            heads = np.sort(key[wave == w, q, 0])[::-1]
            if len(heads) >= k_out:
                T = max(T, int(heads[k_out - 1]))
        admitted = np.logical_and.accumulate(valid[:, q, :] & (key[:, q, :] >= max(T, 1)), axis=1)
        n = int(admitted.sum())
        out.append(dict(path="fallback_survivors" if n > SEL_CAP else "select", T=T, survivors=n))
    return out


# ---------------------------------------------------------------- flag predicates ----
def kth_entries(scores, ids, k_out):
    rs, ri = merge_reference(scores, ids, k_out)
    return rs[:, k_out - 1], ri[:, k_out - 1]


def bit0_expected(scores, ids, list_kc, k_out):
    """scores / ids: the truncated lists Tr [n_lists, nq, k_in], list_kc <= k_in."""
    ks, ki = kth_entries(scores, ids, k_out)
    for q in range(scores.shape[1]):
        for l in np.flatnonzero(np.asarray(ids)[:, q, list_kc - 1] >= 0):
            if better(scores[l, q, list_kc - 1], ids[l, q, list_kc - 1], ks[q], ki[q]):
                return True
    return False


def bit1_possible(scores, ids, kc, k_out):
    if kc >= k_out:
        return False
    ks, ki = kth_entries(scores, ids, k_out)
    for t in range(min(256, scores.shape[0])):
        ts, ti = merge_reference(scores[t::256], ids[t::256], kc)   # thread t's list, every query
        for q in np.flatnonzero(ti[:, kc - 1] >= 0):
            if better(ts[q, kc - 1], ti[q, kc - 1], ks[q], ki[q]):
                return True
    return False


# ------------------------------------------------------------------- data classes ----
TIE_VALUES = np.array([2.0, 0.5, 0.0, -0.0, -0.75, -3.0, -np.inf], np.float32)


def sorted_lists(scores, ids):
    """Each (list, query) row by (score desc, id asc), padding (id < 0) last as (-inf, -1)."""
    scores, ids = np.array(scores, np.float32), np.array(ids, np.int64)
    pad = ids < 0
    scores[pad], ids[pad] = -np.inf, -1
    order = np.lexsort((ids.astype(np.uint64), -(scores.astype(np.float64) + 0.0), pad), axis=-1)
    return np.take_along_axis(scores, order, -1), np.take_along_axis(ids, order, -1)


def distinct_ids(r, shape, bits):
    """Distinct random ids per query (axis 1 of [n_lists, nq, L]).  32: in [0, 2^31), 2^31 - 1
    among them; 64: half below 2^31, half in [2^32, 2^62)."""
    n_lists, nq, L = shape
    n = n_lists * L
    out = np.empty((nq, n), np.int64)
    for q in range(nq):
        have = np.array([(1 << 31) - 1], np.int64)
        while len(have) < n:
            new = r.integers(0, 1 << 31, n, dtype=np.int64)
            if bits == 64:
                hi = r.integers(1 << 32, 1 << 62, n, dtype=np.int64)
                new = np.where(r.random(n) < 0.5, new, hi)
            have = np.unique(np.concatenate([have, new]))
        pick = r.permutation(have)[:n]
        if (1 << 31) - 1 not in pick:
            pick[0] = (1 << 31) - 1
        out[q] = pick
    return np.ascontiguousarray(out.reshape(nq, n_lists, L).transpose(1, 0, 2))


def distinct_scores(r, shape):
    """Normal scores, all different within a query: multiples of 1/1024 around zero, zero left out."""
    n_lists, nq, L = shape
    n = n_lists * L
    out = np.empty((nq, n), np.float32)
    for q in range(nq):
        v = r.permutation(n).astype(np.int64) - n // 2
        out[q] = np.where(v >= 0, v + 1, v).astype(np.float32) / np.float32(1024)
    return np.ascontiguousarray(out.reshape(nq, n_lists, L).transpose(1, 0, 2))


def gen_distinct(r, shape, k_out, place=None):
    return distinct_scores(r, shape), None


def gen_ties(r, shape, k_out, place=None):
    return TIE_VALUES[r.integers(0, len(TIE_VALUES), shape)], None


def gen_ragged(r, shape, k_out, place=None):
    """Lengths uniform in 0..k_in, 60 % of the lists empty, queries 1, 6, ... with nothing and
    3, 8, ... with fewer than k_out entries in all (when nq > 1); scores are quarter steps, so
    they tie, -0.0 and +0.0 among them."""
    n_lists, nq, L = shape
    s = (np.round(r.standard_normal(shape) * 4) / 4).astype(np.float32)
    length = r.integers(0, L + 1, (n_lists, nq))
    length[r.random((n_lists, nq)) < 0.6] = 0
    if nq > 1:
        for q in range(nq):
            if q % 5 == 1:
                length[:, q] = 0
            elif q % 5 == 3:
                length[:, q] = 0
                length[r.integers(0, n_lists), q] = min(L, k_out // 2)
    return s, np.arange(L)[None, None, :] < length[:, :, None]


def gen_concentrated(r, shape, k_out, place):
    """A low (negative) background with the top k_out planted high: 'one_list', 'one_thread'
    (lists t, t + 256, ... of thread t = 5) or 'one_wave' (the heads of wave 2's lists)."""
    n_lists, nq, L = shape
    s = -np.abs(distinct_scores(r, shape)) - 1
    top = (np.arange(k_out, 0, -1, dtype=np.float32) + 10)
    for q in range(nq):
        if place == "one_list":
            assert L >= k_out
            s[(3 + q) % n_lists, q, :k_out] = top
        elif place == "one_thread":
            lists = np.arange(5, n_lists, 256)
            per = -(-k_out // len(lists))
            assert len(lists) > 1 and L >= per
            for a, l in enumerate(lists):
                part = top[a * per:(a + 1) * per]
                s[l, q, :len(part)] = part
        else:
            lists = np.flatnonzero((np.arange(n_lists) % 256) // 64 == 2)[:k_out]
            assert len(lists) == k_out
            s[lists, q, 0] = r.permutation(top)
    return s, None


def gen_equal(r, shape, k_out, place=None):
    return np.full(shape, 0.5, np.float32), None


def gen_quarters(r, shape, k_out, place=None):
    return (np.round(r.standard_normal(shape) * 4) / 4).astype(np.float32), None


def gen_short(r, shape, k_out, place):
    """Every list shorter than `place` entries (nothing for a truncation to hide)."""
    s, _ = gen_quarters(r, shape, k_out)
    length = r.integers(0, place, shape[:2])
    return s, np.arange(shape[2])[None, None, :] < length[:, :, None]


GENERATORS = dict(distinct=gen_distinct, ties=gen_ties, ragged=gen_ragged, concentrated=gen_concentrated,
                  equal=gen_equal, quarters=gen_quarters, short=gen_short)


class Case:
    """name, cls, shape (n_lists, nq, k_in), k_out; `pin` names the path every query of the case
    must take at form 0 (None: whatever the data gives); `admit_all` pins T == 0."""

    def __init__(self, name, cls, n_lists, nq, k_in, k_out, place=None, pin=None, admit_all=None,
                 list_kc=0, kc=0, bit0=None):
        self.name, self.cls, self.place, self.pin, self.admit_all = name, cls, place, pin, admit_all
        self.n_lists, self.nq, self.k_in, self.k_out = n_lists, nq, k_in, k_out
        self.list_kc, self.kc, self.bit0 = list_kc, kc, bit0      # overflow cases only
        assert n_lists * nq * k_in <= 1 << 22

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def _data(case, bits):
    """The full sorted lists of a case -> (scores float32, ids int32 / int64); not to be written to."""
    shape = (case.n_lists, case.nq, case.k_in)
    r = np.random.default_rng([sum(case.name.encode()), case.n_lists, case.nq, case.k_in, case.k_out])
    s, valid = GENERATORS[case.cls](r, shape, case.k_out, case.place)
    ids = distinct_ids(r, shape, bits)
    if valid is not None:
        ids = np.where(valid, ids, -1)
    s, ids = sorted_lists(s, ids)
    ids = ids.astype(np.int32 if bits == 32 else np.int64)
    s.setflags(write=False)
    ids.setflags(write=False)
    return s, ids


def case_data(case, bits):
    return _data(case, bits)


@functools.lru_cache(maxsize=None)
def case_reference(case, bits, k_out=None):
    s, i = _data(case, bits)
    return merge_reference(s, i, k_out or case.k_out)


def truncated(case, bits):
    """Tr: the first list_kc entries of every list of an overflow case, contiguous."""
    s, i = _data(case, bits)
    return np.ascontiguousarray(s[:, :, :case.list_kc]), np.ascontiguousarray(i[:, :, :case.list_kc])


def _rotated():
    """distinct, ties and ragged over every n_lists, the other sizes rotating (as the other
    case modules do, not the full product); k_in steps down while a case is over MAX_ELEMS."""
    cases = []
    for c, cls in enumerate(("distinct", "ties", "ragged")):
        for a, n_lists in enumerate(N_LISTS):
            nq = NQS[(a + 2 * c) % len(NQS)]
            ki = (2 * a + 3 * c) % len(K_INS)
            k_out = K_OUTS[(3 * a + 5 * c + 1) % len(K_OUTS)]
            while n_lists * nq * K_INS[ki] > MAX_ELEMS:
                ki -= 1
            cases.append(Case("%s-%dx%dx%d-k%d" % (cls, n_lists, nq, K_INS[ki], k_out), cls, n_lists, nq,
                              K_INS[ki], k_out))
    return cases


# cases that pin a path (form 0)
PINNED = [
    Case("threadlist-kc8", "distinct", 257, 33, 9, 5, pin="threadlist"),
    Case("threadlist-kc16", "ties", 65, 70, 17, 16, pin="threadlist"),
    Case("threadlist-kc8-ragged", "ragged", 1000, 33, 8, 8, pin="threadlist"),
    Case("select-batch-boundary", "distinct", 257, 32, 9, 5, pin="select"),
    Case("select-k17-batch", "distinct", 300, 33, 17, 17, pin="select", admit_all=False),
    Case("select-4096-lists", "distinct", 4096, 2, 5, 50, pin="select", admit_all=False),
    Case("fallback-4097-lists-kc64", "distinct", 4097, 2, 5, 50, pin="fallback_lists"),
    Case("fallback-4097-lists-kc8", "ties", 4097, 1, 9, 8, pin="fallback_lists"),
    Case("concentrated-one-list", "concentrated", 300, 2, 64, 64, place="one_list", pin="select"),
    Case("concentrated-one-list-batch", "concentrated", 65, 33, 16, 16, place="one_list", pin="threadlist"),
    Case("concentrated-one-thread", "concentrated", 1000, 2, 17, 64, place="one_thread", pin="select"),
    Case("concentrated-one-wave", "concentrated", 256, 2, 5, 64, place="one_wave", pin="select", admit_all=False),
    Case("concentrated-one-wave-1000", "concentrated", 1000, 3, 8, 50, place="one_wave", pin="select",
         admit_all=False),
    Case("crowded-3000-equal", "equal", 3000, 2, 1, 5, pin="fallback_survivors", admit_all=False),
    Case("crowded-40x64-admit-all", "quarters", 40, 2, 64, 64, pin="fallback_survivors", admit_all=True),
    Case("crowded-20x64-admit-all", "quarters", 20, 2, 64, 64, pin="select", admit_all=True),
]
CROWDED = [c for c in PINNED if c.name.startswith("crowded")]
CASES = _rotated() + PINNED

# Overflow cases: full lists F of FULL entries, truncated to list_kc; (list_kc, kc) are the
# library's own: (8, 16) the bf16 scan's at k_out 9..64, (16, 16) the exact scan's at 17..64.
# bit0: True = a truncated list hides a member (must be set), False = must be clear.
OVERFLOW = [
    Case("ovf-distinct-8-16-k9-batch", "distinct", 65, 33, FULL, 9, list_kc=8, kc=16),
    Case("ovf-distinct-8-16-k16", "distinct", 300, 2, FULL, 16, list_kc=8, kc=16),
    Case("ovf-ties-16-16-k17-batch", "ties", 257, 33, FULL, 17, list_kc=16, kc=16),
    Case("ovf-ties-8-16-k64", "ties", 64, 2, FULL, 64, list_kc=8, kc=16),
    Case("ovf-ragged-8-16-k50", "ragged", 255, 5, FULL, 50, list_kc=8, kc=16),
    Case("ovf-hidden-one-list-k64", "concentrated", 64, 2, FULL, 64, place="one_list", list_kc=16, kc=16,
         bit0=True),
    Case("ovf-all-short-k50", "short", 1000, 3, FULL, 50, place=16, list_kc=16, kc=16, bit0=False),
    Case("ovf-all-short-8-k17", "short", 257, 2, FULL, 17, place=8, list_kc=8, kc=16, bit0=False),
    Case("ovf-one-thread-k64", "concentrated", 1000, 2, FULL, 64, place="one_thread", list_kc=16, kc=16),
    Case("ovf-one-thread-4100-k64", "concentrated", 4100, 2, FULL, 64, place="one_thread", list_kc=16, kc=16),
    Case("ovf-one-wave-k64", "concentrated", 256, 2, FULL, 64, place="one_wave", list_kc=16, kc=16),
    Case("ovf-40x64-k64", "quarters", 40, 2, FULL, 64, list_kc=16, kc=16),
    Case("ovf-equal-200-k64", "equal", 200, 2, FULL, 64, list_kc=16, kc=16),
    Case("ovf-distinct-4097-k17", "distinct", 4097, 1, FULL, 17, list_kc=16, kc=16),
]


def tie_full_lists():
    """Full lists that merely tie with the k-th result hide nothing: list 0 holds 15 entries
    of 2.0 and one padding slot, lists 1..3 are full of 1.0 with ids above the k-th's.  At
    k_out = 17 the 17th result is (1.0, id 1) and no last entry is better: bit 0 stays clear.
    -> (scores [4, 1, 16], ids int32 [4, 1, 16], list_kc, kc, k_out)."""
    s = np.full((4, 1, 16), 1.0, np.float32)
    i = np.arange(64, dtype=np.int32).reshape(4, 1, 16) - 16
    s[0, 0, :15], s[0, 0, 15] = 2.0, -np.inf
    i[0, 0, :15], i[0, 0, 15] = np.arange(100, 115), -1
    return s, i, 16, 16, 17


# (list_kc, kc, k_out) of the knife-edge inputs: the library's combinations at their ends
KNIFE_EDGES = ((8, 16, 9), (8, 16, 17), (16, 16, 17), (16, 16, 64))


def knife_edge_lists(list_kc, k_out, rank, nq=1):
    """One full list A (list 1) whose last kept entry lands at result rank `rank` (1-based),
    among k_out + 2 one-entry lists that tie with it on the score and differ by id: the flag's
    tests must be `better`, against exactly the k_out-th result.  bit 0 is due iff rank <
    k_out; at rank == k_out the entry is the k-th itself and hides nothing.  A's other
    entries score higher.  Every query is the same lists (ids repeat across queries only).
    -> (scores [k_out + 3, nq, list_kc], ids int32)."""
    assert list_kc <= rank <= k_out + 2
    n = k_out + 3
    s = np.full((n, list_kc), -np.inf, np.float32)
    i = np.full((n, list_kc), -1, np.int32)
    fillers = [l for l in range(n) if l != 1]
    s[fillers, 0] = 1.0
    i[fillers, 0] = 10 + 2 * np.arange(k_out + 2)
    s[1, :list_kc - 1], i[1, :list_kc - 1] = 2.0, 1000 + np.arange(list_kc - 1)
    s[1, list_kc - 1], i[1, list_kc - 1] = 1.0, 9 + 2 * (rank - list_kc)   # after rank - list_kc fillers
    return (np.ascontiguousarray(np.repeat(s[:, None, :], nq, axis=1)),
            np.ascontiguousarray(np.repeat(i[:, None, :], nq, axis=1)))


def zero_sign_lists():
    """[(+0.0, id 5)] and [(-0.0, id 3)]: the two tie, id 3 goes first.  -> (scores, ids int64)."""
    return (np.array([[[0.0]], [[-0.0]]], np.float32), np.array([[[5]], [[3]]], np.int64))
