"""The float64 reference, the corpora and the checkers of the k-means tests (test_kmeans_cases.py
and test_kmeans_host.py on the CPU, test_gpu_kmeans.py on the GPU).  A plain module; the exact
class, the masks and the fp32 bound are grouped_cases's, the near-duplicate corpus join_cases's.

The definition (include/mq.h, "K-means"): d_j(r) = score(c_j, r) - 0.5 score(c_j, c_j); an
admitted row's label is the argmax of d over j, ties to the lowest j, and its dot is the score
against that centre; any other row gets (-1, -inf).  update: a cluster with members gets their
mean, an empty one keeps its centroid.  `assign64` / `update64` state that in float64,
`assign_by_loop` / `update_by_loop` are the plain per-row loops.

The fp32 bound: a dot of a unit row against a centroid of norm <= 1 is within b = bound(dim) of
float64, half_j within b / 2, and the subtraction rounds once a value below 2: a device d is
within bprime(dim) = 1.5 b + 2^-23 of the float64 d.  A row is undecided when its two best d lie
within 2 bprime of each other.
"""
import functools

import numpy as np

from grouped_cases import (MASKS, NEAR_TIE_CAP, bound, exact_corpus, exact_queries, mask_words,  # noqa: F401
                           row_mask)
from join_cases import neardup_corpus  # noqa: F401

# exact class (test_gpu_kmeans.py rotates the combinations)
NS = (1, 2, 31, 32, 33, 65, 257, 1000, 4097)
DIMS = (64, 256, 768, 1024)
CLUSTERS = (1, 2, 15, 16, 17, 33, 256)
# random class: (dim, n rows, n_clusters), unmasked and under the `third` mask
RANDOM_CASES = ((64, 3000, 17), (256, 1000, 16), (768, 700, 33), (1024, 600, 5), (256, 4500, 256), (512, 900, 2))
# trajectory: (dim, blobs, rows per blob, sigma, corpus seed, seeding seed), found by a search on
# the CPU (test_kmeans_cases.py holds each to: at least 3 updates before convergence, every row's
# margin at every assign >= TRAJECTORY_MARGIN bprime)
TRAJECTORY_MARGIN = 50
TRAJECTORY_CASES = ((64, 6, 50, 1.0, 0, 14), (64, 6, 50, 1.0, 0, 25), (64, 6, 50, 1.0, 1, 13), (64, 6, 50, 1.0, 1, 5),
                    (256, 16, 20, 1.0, 1, 30))
# planted blobs: (dim, blobs, rows per blob), sigma 0.5, seeded with one member of each blob
PLANTED_CASES = ((64, 5, 40), (256, 12, 100), (768, 33, 20), (1024, 17, 30))
PLANTED_SIGMA = 0.5
STORE_CASE = (256, 6, 50)  # the store tests' planted blobs
# the store whose rankings are compared with float64: (dim, blobs, rows per blob, sigma)
REP_CASE = (64, 4, 12, 1.0)


def bprime(dim):
    """|device d - float64 d| for unit rows and centroids of norm <= 1."""
    return 1.5 * bound(dim) + 2.0 ** -23


# ---------------------------------------------------------------- the definition ----
def d64(rows, cents):
    """-> (s, d) float64 [n, c]: the dots of every row with every centroid, and d = s - half."""
    r, c = np.asarray(rows, np.float64), np.asarray(cents, np.float64)
    s = r @ c.T + 0.0
    return s, s - 0.5 * (c * c).sum(1)[None, :]


def assign64(rows, cents, mask=None):
    """-> (labels int32 [n], dots float64 [n], d float64 [n, c]): argmax of d (np.argmax: the
    lowest j of the largest d); rows outside the mask get (-1, -inf)."""
    s, d = d64(rows, cents)
    n = len(s)
    ok = np.ones(n, bool) if mask is None else np.asarray(mask, bool)
    lab = d.argmax(1).astype(np.int32) if n else np.zeros(0, np.int32)
    dots = s[np.arange(n), lab] if n else np.zeros(0)
    return np.where(ok, lab, -1).astype(np.int32), np.where(ok, dots, -np.inf), d


def update64(rows, labels, cents):
    """-> (centroids float64 [c, dim], counts int64 [c]): the members' float64 mean; an empty
    cluster keeps its centroid."""
    r = np.asarray(rows, np.float64)
    out = np.array(cents, np.float64)
    c = len(out)
    counts = np.bincount(labels[labels >= 0], minlength=c).astype(np.int64)
    sums = np.zeros_like(out)
    np.add.at(sums, labels[labels >= 0], r[labels >= 0])
    full = counts > 0
    out[full] = sums[full] / counts[full, None]
    return out, counts


def assign_by_loop(rows, cents, mask=None):
    """assign64 by a plain loop over the rows and the centroids -> (labels, dots)."""
    rows, cents = np.asarray(rows, np.float64), np.asarray(cents, np.float64)
    labels, dots = [], []
    for r in range(len(rows)):
        if mask is not None and not mask[r]:
            labels.append(-1)
            dots.append(-np.inf)
            continue
        best, bj, bs = -np.inf, -1, -np.inf
        for j in range(len(cents)):
            s = float(np.einsum("d,d->", rows[r], cents[j])) + 0.0
            d = s - 0.5 * float(np.einsum("d,d->", cents[j], cents[j]))
            if bj < 0 or d > best:  # j ascends: an equal d keeps the lower j
                best, bj, bs = d, j, s
        labels.append(bj)
        dots.append(bs)
    return np.array(labels, np.int32), np.array(dots)


def update_by_loop(rows, labels, cents):
    rows = np.asarray(rows, np.float64)
    out = np.array(cents, np.float64)
    counts = np.zeros(len(out), np.int64)
    for j in range(len(out)):
        members = [r for r in range(len(rows)) if labels[r] == j]
        counts[j] = len(members)
        if members:
            out[j] = sum(rows[r] for r in members) / len(members)
    return out, counts


def lloyd64(rows, cents, mask, n_iter):
    """The call in float64, the centroids rounded to float32 after every update as the device
    stores them -> (centroids float32, labels, updates applied before convergence, converged,
    the smallest margin (best d - second best d over the admitted rows) of every assign)."""
    cents = np.array(cents, np.float32)
    prev = np.full(len(rows), -1, np.int32)
    margins, updates = [], 0
    labels, _, d = assign64(rows, cents, mask)
    margins.append(margin64(d, mask))
    for _ in range(n_iter):
        if np.array_equal(labels, prev):
            return cents, labels, updates, True, margins
        prev = labels
        cents = update64(rows, labels, cents)[0].astype(np.float32)
        updates += 1
        labels, _, d = assign64(rows, cents, mask)
        margins.append(margin64(d, mask))
    return cents, labels, updates, bool(np.array_equal(labels, prev)), margins


def margin64(d, mask=None):
    """The smallest gap between the best and the second best d over the admitted rows (inf with
    one centroid or no admitted row)."""
    if d.shape[1] < 2:
        return np.inf
    top = -np.partition(-d, 1, axis=1)[:, :2]
    gap = top[:, 0] - top[:, 1]
    if mask is not None:
        gap = gap[np.asarray(mask, bool)]
    return float(gap.min(initial=np.inf))


def objective64(rows, cents, labels):
    """Sum over the admitted rows of |r - c_label|^2 in float64."""
    r, c = np.asarray(rows, np.float64), np.asarray(cents, np.float64)
    ok = labels >= 0
    return float(((r[ok] - c[labels[ok]]) ** 2).sum())


# -------------------------------------------------------------------- exact class ----
def exact_centroids(dim, n, c):
    """float32 [c, dim] exact-class centroids for exact_corpus(dim, n): j % 4 == 0 an exact-class
    vector over the corpus's coordinate pool, 1 a stored row, 2 a repeat of centroid j - 2 (an
    exact tie: the lower j wins), 3 an exact-class vector scaled by 2 or 1/2 (its half differs
    and stays exact)."""
    rows, q = exact_corpus(dim, n), exact_queries(dim, c)
    out = np.empty((c, dim), np.float32)
    for j in range(c):
        if j % 4 == 0:
            out[j] = q[j]
        elif j % 4 == 1:
            out[j] = rows[(7 * j) % n]
        elif j % 4 == 2:
            out[j] = out[j - 2]
        else:
            out[j] = q[j] * (2.0 if j % 8 == 3 else 0.5)
    return out


# ------------------------------------------------------------------- random class ----
def random_centroid_rows(dim, n, c, admitted):
    """The rows whose stored values seed a random-class case."""
    return np.random.default_rng([dim, n, c, 19]).choice(admitted, c, replace=False)


def undecided_rows(d, dim):
    """bool [n]: the two best d lie within 2 bprime(dim)."""
    if d.shape[1] < 2:
        return np.zeros(len(d), bool)
    top = -np.partition(-d, 1, axis=1)[:, :2]
    return top[:, 0] - top[:, 1] <= 2 * bprime(dim)


def check_assign(labels, dots, rows, cents, mask, dim):
    """The device's (labels, dots) against the float64 definition -> (failures, undecided bool
    [n]).  A decided admitted row's label equals the reference's; an undecided one's is a centroid
    within 2 bprime of its best d; dots within bound(dim) of the float64 dot with the label's
    centroid (dots None: not checked); rows outside the mask get (-1, -inf)."""
    ref, _, d = assign64(rows, cents, mask)
    s = d64(rows, cents)[0]
    und = undecided_rows(d, dim)
    ok = np.ones(len(d), bool) if mask is None else np.asarray(mask, bool)
    fails = []
    for r in range(len(d)):
        a = int(labels[r])
        if not ok[r]:
            if a != -1 or (dots is not None and dots[r] != -np.inf):
                fails.append("row %d outside the mask: label %d" % (r, a))
            continue
        if not 0 <= a < d.shape[1]:
            fails.append("row %d: label %d" % (r, a))
        elif a != ref[r] and not (und[r] and d[r, a] >= d[r].max() - 2 * bprime(dim)):
            fails.append("row %d: label %d, reference %d, d %.9g against %.9g" % (r, a, ref[r], d[r, a], d[r].max()))
        elif dots is not None and abs(float(dots[r]) - s[r, a]) > bound(dim):
            fails.append("row %d: dot %.9g, float64 %.9g" % (r, dots[r], s[r, a]))
    return fails, und & ok


def check_update(cents, rows, labels, before):
    """The device's centroids after one update under its own labels -> failures.  A cluster of m
    members: every coordinate within (m + 2) 2^-24 mean_i |x_i| of the float64 mean - the forward
    bound of an fp32 sum of m terms in any order ((m - 1) 2^-24 sum |x_i|, divided by m) plus the
    division's rounding; an empty cluster: its centroid of before, bit for bit."""
    r = np.asarray(rows, np.float64)
    fails = []
    for j in range(len(cents)):
        mem = r[labels == j]
        if not len(mem):
            if not np.array_equal(cents[j].view(np.int32), before[j].view(np.int32)):
                fails.append("empty cluster %d changed" % j)
            continue
        tol = (len(mem) + 2) * 2.0 ** -24 * np.abs(mem).mean(0)
        err = np.abs(cents[j].astype(np.float64) - mem.mean(0))
        if (err > tol).any():
            k = int((err - tol).argmax())
            fails.append("cluster %d (%d members) coordinate %d: error %.3g, bound %.3g" % (j, len(mem), k, err[k], tol[k]))
    return fails


# ------------------------------------------------------------------------- blobs ----
@functools.lru_cache(maxsize=None)
def blob_corpus(dim, blobs, per, sigma, seed=0):
    """-> (rows float32 [blobs x per, dim] read-only, the planted blob of every row): unit Gaussian
    bases, member = normalise(base + sigma z), z ~ N(0, I / dim); the rows are shuffled."""
    rng = np.random.default_rng([seed, dim, blobs, per, 19])
    base = rng.standard_normal((blobs, dim))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    planted = rng.permutation(np.repeat(np.arange(blobs), per))
    rows = base[planted] + sigma * rng.standard_normal((blobs * per, dim)) / np.sqrt(dim)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows = rows.astype(np.float32)
    rows.setflags(write=False)
    return rows, planted


def planted_seeds(planted, blobs):
    """The first member of each blob, by blob."""
    return np.array([int(np.flatnonzero(planted == g)[0]) for g in range(blobs)])


def trajectory_seeds(n, blobs, seed):
    """Random distinct rows as the initial centres."""
    return np.random.default_rng([seed, n, blobs, 20]).choice(n, blobs, replace=False)


def search_trajectories(dim, blobs, per, sigma, corpus_seeds, seeds, max_iter=30):
    """The CPU search that found TRAJECTORY_CASES: -> [(corpus seed, seeding seed, updates,
    smallest margin in bprime)] of the runs with >= 3 updates and every margin >=
    TRAJECTORY_MARGIN bprime."""
    found = []
    for cs in corpus_seeds:
        rows, _ = blob_corpus(dim, blobs, per, sigma, cs)
        for sd in seeds:
            init = rows[trajectory_seeds(len(rows), blobs, sd)]
            _, _, updates, conv, margins = lloyd64(rows, init, None, max_iter)
            worst = min(margins) / bprime(dim)
            if conv and updates >= 3 and worst >= TRAJECTORY_MARGIN:
                found.append((cs, sd, updates, worst))
    return found


def ranking_gap(rows, cents, hits):
    """The smallest gap between neighbours among the first hits + 1 entries of every centre's
    ranking of the rows by dot: above 2 bound(dim), fp32 ranks those entries as float64 does."""
    s = -np.sort(-d64(rows, cents)[0].T, axis=1)[:, :hits + 1]
    return float((s[:, :-1] - s[:, 1:]).min(initial=np.inf))


# ------------------------------------------------- LangChain's selection, restated ----
def langchain_closest_indices(distances, num_clusters, num_closest, remove_duplicates):
    """`_filter_cluster_embeddings` of langchain_community's embeddings_redundant_filter, on a
    [num_clusters, n] array of distances to the centres in place of the KMeans fit."""
    closest_indices = []
    for i in range(num_clusters):
        order = np.argsort(distances[i], kind="stable")
        if remove_duplicates:
            closest_indices_sorted = [x for x in order[:num_closest] if x not in closest_indices]
        else:
            closest_indices_sorted = [x for x in order if x not in closest_indices][:num_closest]
        closest_indices.extend(closest_indices_sorted)
    return [int(x) for x in closest_indices]


def kmeanspp_restated(dots, k, rng):
    """`kmeanspp_rows` by plain loops over a full [n, n] dot matrix."""
    n = len(dots)
    picked = [int(rng.integers(n))]
    while len(picked) < k:
        m = np.array([min(max(0.0, 2.0 - 2.0 * float(dots[p][r])) for p in picked) for r in range(n)])
        for p in picked:
            m[p] = 0.0
        if m.sum() > 0.0:
            picked.append(int(rng.choice(n, p=m / m.sum())))
        else:
            picked.append(int(rng.choice(np.array([r for r in range(n) if r not in picked]))))
    return picked
