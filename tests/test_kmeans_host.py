"""K-means on the host: every argument check of mq_index_kmeans answers MQ_EINVAL and names the
offending value before any HIP call (no GPU needed; the checks that need the index's shape are
reached through mq_debug_kmeans_check on a stated (dim, rows)), the scratch size is monotone, and
the store's `cluster` / `cluster_representatives` validate their arguments on a store without a
device."""
import ctypes
import os

import numpy as np
import pytest

from mediquery_hip import ClusterResult, HipChroma, _lib
from mediquery_hip.native import kmeans_scratch_bytes

EINVAL = -1


def _aligned(nbytes):
    buf = (ctypes.c_uint8 * (nbytes + 64))()
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 63) & ~63)


def _check(dim=256, n=10, n_clusters=3, n_iter=5, cent=True, out_a=True, out_d=True, out_c=True, out_info=True,
           io_on_device=0, scratch=True, scratch_bytes=None, scratch_off=0, poison=None):
    """mq_debug_kmeans_check with sound defaults; True = a valid host buffer of its own."""
    keep = []

    def buf(flag, nbytes):
        if flag is not True:
            return flag
        b, p = _aligned(nbytes)
        keep.append(b)
        return p
    need = kmeans_scratch_bytes(n, n_clusters)
    small = min(max(1, n), 64)  # nothing is read: a refused call needs no room for 2^31 rows
    c = max(1, min(n_clusters, 256))
    cp = buf(cent, c * max(dim, 64) * 4)  # zeroed: finite
    if poison is not None and cp is not None:
        j, k, v = poison
        ctypes.cast(cp, ctypes.POINTER(ctypes.c_float))[j * dim + k] = v
    s = buf(scratch, min(need, 16 << 20) + 64)
    if s is not None and scratch_off:
        s = ctypes.c_void_p(s.value + scratch_off)
    return _lib.call("mq_debug_kmeans_check", dim, n, n_clusters, n_iter, cp, buf(out_a, small * 4),
                     buf(out_d, small * 4), buf(out_c, c * 8), buf(out_info, 32), io_on_device, s,
                     need if scratch_bytes is None else scratch_bytes)


def _raises(match, **kw):
    with pytest.raises(_lib.MQError, match=match) as e:
        _check(**kw)
    assert e.value.code == EINVAL


def test_constant_is_the_headers():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mq.h")).read()
    assert "#define MQ_KMEANS_MAX_CLUSTERS %d" % _lib.MQ_KMEANS_MAX_CLUSTERS in header


def test_scalar_checks_come_before_the_handle():
    def call(n_clusters, n_iter):
        return _lib.call("mq_index_kmeans", None, None, n_clusters, n_iter, None, None, None, None, None, 0, None, 0,
                         None)
    for c in (0, -1, 257, 1 << 20):
        with pytest.raises(_lib.MQError, match=r"n_clusters must be in \[1, 256\] \(got %d\)" % c) as e:
            call(c, 1)
        assert e.value.code == EINVAL
    for it in (-1, 1025):
        with pytest.raises(_lib.MQError, match=r"n_iter must be in \[0, 1024\] \(got %d\)" % it) as e:
            call(3, it)
        assert e.value.code == EINVAL
    for c, it in ((1, 0), (256, 1024)):
        with pytest.raises(_lib.MQError, match="NULL index") as e:
            call(c, it)
        assert e.value.code == EINVAL


def test_every_shape_and_buffer_check_names_its_value():
    assert _check() == 0
    _raises(r"n_clusters must be in \[1, 256\] \(got 0\)", n_clusters=0)
    _raises(r"n_clusters must be in \[1, 256\] \(got 257\)", n_clusters=257)
    _raises(r"n_iter must be in \[0, 1024\] \(got -3\)", n_iter=-3)
    _raises(r"n_iter must be in \[0, 1024\] \(got 1025\)", n_iter=1025)
    assert _check(n_clusters=256, n_iter=0) == 0 and _check(n_clusters=1, n_iter=1024) == 0
    assert _check(n_clusters=50, n=10) == 0  # more clusters than rows: the surplus stays empty
    for dim in (0, 32, 96, 1088, 2048, -64):
        _raises(r"dim %% 64 == 0, dim <= 1024 \(got %d\)" % dim, dim=dim)
    for dim in (64, 256, 512, 768, 1024):
        assert _check(dim=dim) == 0
    _raises(r"fewer than 2\^31 rows \(got 2147483648\)", n=1 << 31)
    _raises("NULL centroids", cent=None)
    for name in ("out_a", "out_d", "out_c", "out_info"):
        _raises("NULL output buffer", **{name: None})
    _raises("NULL scratch", scratch=None)
    # the scratch: aligned, large enough, and none of the other buffers
    _raises(r"scratch must be 16-byte aligned \(got 0x[0-9a-f]+8\)", scratch_off=8)
    need = kmeans_scratch_bytes(10, 3)
    _raises(r"scratch_bytes %d is below the %d bytes mq_kmeans_scratch_bytes\(10, 3\) asks" % (need - 1, need),
            scratch_bytes=need - 1)
    _raises(r"scratch_bytes 0 is below", scratch_bytes=0)
    _raises(r"scratch_bytes -5 is below", scratch_bytes=-5)
    buf, p = _aligned(need + 64)
    _raises(r"scratch overlaps centroids \(0x[0-9a-f]+\)", scratch=p, cent=ctypes.c_void_p(p.value + need - 8),
            io_on_device=1)
    _raises(r"scratch overlaps out_assign \(0x[0-9a-f]+\)", scratch=p, out_a=p)
    _raises(r"scratch overlaps out_dots \(0x[0-9a-f]+\)", scratch=p, out_d=ctypes.c_void_p(p.value + 256))
    _raises(r"scratch overlaps out_counts \(0x[0-9a-f]+\)", scratch=p, out_c=ctypes.c_void_p(p.value + 512))
    _raises(r"scratch overlaps out_info \(0x[0-9a-f]+\)", scratch=p, out_info=ctypes.c_void_p(p.value + need - 32))
    # host centroids are read: all finite
    _raises(r"centroids\[2\]\[17\] = nan is not finite", poison=(2, 17, float("nan")))
    _raises(r"centroids\[0\]\[255\] = inf is not finite", poison=(0, 255, float("inf")))
    _raises(r"centroids\[1\]\[0\] = -inf is not finite", poison=(1, 0, float("-inf")))
    assert _check(poison=(2, 17, float("nan")), io_on_device=1) == 0  # device centroids are not read
    # an empty index: counts and out_info alone
    assert _check(n=0, out_a=None, out_d=None, scratch=None, scratch_bytes=0) == 0
    _raises("NULL output buffer", n=0, out_info=None)
    _raises("NULL centroids", n=0, cent=None)


def test_kmeans_scratch_bytes_is_monotone():
    f = kmeans_scratch_bytes
    assert f(1000, 16) > 0
    ns = (0, 1, 255, 256, 257, 4097, 10 ** 5, 10 ** 6, 10 ** 8, (1 << 31) - 1)
    cs = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100, 255, 256)
    table = np.array([[f(n, c) for c in cs] for n in ns])
    assert (table % 256 == 0).all()
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    # 16 bytes per row, the partial sums (32 MB at most) and 4 KB of staging per centroid
    assert 16 * 10 ** 6 <= f(10 ** 6, 256) <= 16 * 10 ** 6 + (34 << 20) + (1 << 20)
    # arguments out of range are clamped
    assert f(-5, -1) == f(0, 1) == f(0, 0) and f(1 << 40, 1 << 20) == f((1 << 31) - 1, 256)


# ------------------------------------------------------------------- the store's side ----
def test_cluster_arguments_are_checked_without_a_device():
    store = HipChroma(dim=256, auto_persist=False)
    for bad in (0, -1, 257, 2.5, True, "5", None):
        with pytest.raises(ValueError, match=r"n_clusters must be an integer in \[1, 256\]"):
            store.cluster(n_clusters=bad)
    for bad in (-1, 1025, 2.5, True, None):
        with pytest.raises(ValueError, match=r"max_iter must be an integer in \[0, 1024\]"):
            store.cluster(max_iter=bad)
    for bad in (-1, 2.5, True, None):
        with pytest.raises(ValueError, match="seed must be a non-negative integer"):
            store.cluster(seed=bad)
    for bad in ("kmeans++", "k-means", ""):
        with pytest.raises(ValueError, match="init must be one of"):
            store.cluster(init=bad)
    for bad in (np.zeros((4, 256)), np.zeros((5, 128)), np.zeros(256), np.zeros((5, 256, 1))):
        with pytest.raises(ValueError, match=r"an init array must be \[n_clusters = 5, dim = 256\]"):
            store.cluster(init=bad)
    bad = np.zeros((5, 256))
    bad[3, 7] = np.nan
    with pytest.raises(ValueError, match="an init array must be finite"):
        store.cluster(init=bad)
    with pytest.raises(ValueError, match="where_document"):
        store.cluster(where_document={"$near": "x"})
    for bad in (0, -2, 1.5, True):
        with pytest.raises(ValueError, match="num_closest must be a positive integer"):
            store.cluster_representatives(num_closest=bad)
    # an empty store admits no row: fewer than any n_clusters
    for kw in ({}, {"init": "random"}, {"init": np.zeros((5, 256))}, {"ids": ["a"]}):
        with pytest.raises(ValueError, match="n_clusters=5 exceeds the 0 rows the filters admit"):
            store.cluster(**kw)
    with pytest.raises(ValueError, match="n_clusters=2 exceeds the 0 rows"):
        store.cluster_representatives(n_clusters=2)
    assert ClusterResult([], np.zeros(0, np.int32), np.zeros((1, 4)), np.zeros(1), 0, True, 0.0).converged
