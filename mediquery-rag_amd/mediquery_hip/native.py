"""Thin handle classes over the C ABI: `FlatIndex` (mq_index_*) and `Encoder`
(mq_encoder_*).  Host calls take/return numpy arrays; `*_device` calls take torch
device tensors and run asynchronously on the given (or current) torch stream."""
import ctypes

import numpy as np

from . import _lib
from .config import BertConfig
from .weights import head_from_state_dict, state_dict_to_blob, synthetic_state_dict


class FlatIndex:
    """HBM-resident exact cosine index (K8 add, K9 fused score + top-k, K10 merge)."""

    def __init__(self, dim=768, capacity=0, device=0, dtype=_lib.MQ_DTYPE_F32):
        h = ctypes.c_void_p()
        _lib.call("mq_index_create", device, dim, capacity, dtype, ctypes.byref(h))
        self._h = h
        self.dim = dim
        self.device = device

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().mq_index_destroy(h)
            except Exception:  # interpreter shutdown
                pass

    __del__ = close

    def __len__(self):
        n = ctypes.c_int64()
        _lib.call("mq_index_size", self._h, ctypes.byref(n))
        return n.value

    def add(self, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, self.dim)
        _lib.call("mq_index_add", self._h, _lib.ptr(rows), rows.shape[0], 0, None)

    def add_device(self, rows, stream=None):
        assert rows.is_cuda and rows.dtype.is_floating_point and rows.is_contiguous()
        _lib.call("mq_index_add", self._h, _lib.ptr(rows), rows.shape[0], 1,
                  _lib.stream_handle(stream))

    def reset(self):
        _lib.call("mq_index_reset", self._h)

    def search(self, queries, k):
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        scores = np.empty((q.shape[0], k), dtype=np.float32)
        ids = np.empty((q.shape[0], k), dtype=np.int64)
        _lib.call("mq_index_search", self._h, _lib.ptr(q), q.shape[0], k, _lib.ptr(scores),
                  _lib.ptr(ids), 0, None)
        return scores, ids

    def search_device(self, queries, k, out_scores, out_ids, stream=None):
        """queries [nq, dim] f32, out_scores [nq, k] f32, out_ids [nq, k] int64 (torch, device)."""
        _lib.call("mq_index_search", self._h, _lib.ptr(queries), queries.shape[0], k,
                  _lib.ptr(out_scores), _lib.ptr(out_ids), 1, _lib.stream_handle(stream))

    def get(self, row0=0, n=None):
        """Stored (normalised) rows [row0, row0+n) as float32 numpy."""
        n = len(self) - row0 if n is None else n
        out = np.empty((n, self.dim), dtype=np.float32)
        _lib.call("mq_index_get", self._h, row0, n, _lib.ptr(out), 0, None)
        return out

    def select(self, rows, out=None):
        """Index whose row i is this index's row rows[i] (device gather, no host copy of
        the slab); out=self compacts in place.  Returns `out` (a new index if None)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        out = FlatIndex(dim=self.dim, device=self.device) if out is None else out
        _lib.call("mq_index_select", self._h, _lib.ptr(rows), rows.size, out._h)
        return out

    def data_ptr(self):
        p = ctypes.c_void_p()
        _lib.call("mq_index_data", self._h, ctypes.byref(p))
        return p.value

    STAGES = ("flat_search_kernel", "merge_kernel")

    def set_precision(self, dtype):
        """_lib.MQ_DTYPE_F32 (exact f32 MFMA), _lib.MQ_DTYPE_F32X6 (split-f32),
        _lib.MQ_DTYPE_BF16 (bf16 coarse scan + exact fp32 re-rank) or
        _lib.MQ_DTYPE_F32_SCREEN (exact fp32 top-k: certified bf16 / split-f32 screens +
        fp32 re-rank)."""
        _lib.call("mq_index_set_precision", self._h, dtype)

    def set_stream_threshold(self, max_queries):
        """Batches of <= max_queries (0..16) use the streaming fp32 kernel (K9s)."""
        _lib.call("mq_index_set_stream_threshold", self._h, int(max_queries))

    def set_threshold_scan(self, enabled=True):
        """Batched bf16 candidate scans: threshold scan (K9t, default) or tiled lists."""
        _lib.call("mq_index_set_threshold_scan", self._h, int(bool(enabled)))

    def set_int8_screen(self, enabled=True):
        """Single screened queries: int8-shadow threshold scan first (K9q, default) or
        straight to the bf16 stream tier.  Same results either way."""
        _lib.call("mq_index_set_int8_screen", self._h, int(bool(enabled)))

    def set_async_screen(self, enabled=True):
        """Batched screened searches: uncertified queries re-run exactly on the device with
        no host read-back (default), or the synchronous tiered re-run.  Same results."""
        _lib.call("mq_index_set_async_screen", self._h, int(bool(enabled)))

    @property
    def rescans(self):
        """Searches whose k > 16 list-overflow check fired (re-scanned with 64 lists)."""
        n = ctypes.c_int64()
        _lib.call("mq_index_rescans", self._h, ctypes.byref(n), None)
        return n.value

    @property
    def remerges(self):
        """Merges whose 16-entry thread lists overflowed (re-run with 64)."""
        n = ctypes.c_int64()
        _lib.call("mq_index_rescans", self._h, None, ctypes.byref(n))
        return n.value

    @property
    def screen_fallbacks(self):
        """Screened queries (MQ_DTYPE_F32_SCREEN) re-run on the direct exact scan."""
        n = ctypes.c_int64()
        _lib.call("mq_index_screen_fallbacks", self._h, ctypes.byref(n), None)
        return n.value

    @property
    def screen_passdowns(self):
        """bf16-screened queries whose certificate failed, re-run on the split-f32 screen."""
        n = ctypes.c_int64()
        _lib.call("mq_index_screen_fallbacks", self._h, None, ctypes.byref(n))
        return n.value

    @property
    def screen_skips(self):
        """Batched screened searches that bypassed the bf16 tier (failure share > 0.2)."""
        n = ctypes.c_int64()
        _lib.call("mq_index_screen_skips", self._h, ctypes.byref(n), None)
        return n.value

    @property
    def int8_skips(self):
        """Single screened queries that sat the int8 tier out (failure share > 0.3)."""
        n = ctypes.c_int64()
        _lib.call("mq_index_screen_skips", self._h, None, ctypes.byref(n))
        return n.value

    def set_timing(self, enabled=True):
        _lib.call("mq_index_set_timing", self._h, int(bool(enabled)))

    def read_timing(self):
        """{stage: device ms since the last read} (HIP events on the launch stream)."""
        ms = np.zeros(len(self.STAGES), dtype=np.float32)
        _lib.call("mq_index_read_timing", self._h, _lib.ptr(ms), len(ms))
        return dict(zip(self.STAGES, ms.tolist()))

    def save(self, path):
        _lib.call("mq_index_save", self._h, str(path).encode())

    def load(self, path):
        _lib.call("mq_index_load", self._h, str(path).encode())

    def _check_bits(self, bits):
        check_mask_words(bits, len(self), self.device)

    def search_masked(self, queries, k, bits):
        """Exact top-k of each query ([dim] or [nq, dim] host floats) over the rows allowed
        by `bits` (a device mask tensor on this index's GPU of >= ceil(n / 32) int32 words,
        bit r % 32 of word r / 32 = row r; mask_eval builds it).  One call for the whole
        batch (mq_index_search_masked_batch).  -> (scores [nq, k], ids [nq, k])."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        self._check_bits(bits)
        scores = np.empty((q.shape[0], k), dtype=np.float32)
        ids = np.empty((q.shape[0], k), dtype=np.int64)
        with _lib.device_scope(self.device):
            _lib.call("mq_index_search_masked_batch", self._h, _lib.ptr(q), q.shape[0], k, _lib.ptr(bits),
                      _lib.ptr(scores), _lib.ptr(ids), 0, _lib.stream_handle(None))
        return scores, ids

    def mmr_select(self, cand_scores, cand_ids, k, lambda_mult=0.5):
        """Maximal-marginal-relevance selection (K11, mq_index_mmr_select) over each query's
        candidate list: cand_scores [nq, fetch_k] f32 (each candidate's cosine to the query,
        taken as given), cand_ids [nq, fetch_k] int64 row ids (any order; an id outside
        [0, n) is padding).  -> (scores [nq, k], ids [nq, k]) in selection order, padded
        with (-inf, -1) when fewer than k candidates are valid."""
        s = np.ascontiguousarray(cand_scores, dtype=np.float32)
        i = np.ascontiguousarray(cand_ids, dtype=np.int64)
        s = s.reshape(1, -1) if s.ndim == 1 else s
        i = i.reshape(s.shape)
        scores = np.empty((s.shape[0], k), dtype=np.float32)
        ids = np.empty((s.shape[0], k), dtype=np.int64)
        with _lib.device_scope(self.device):
            _lib.call("mq_index_mmr_select", self._h, _lib.ptr(s), _lib.ptr(i), s.shape[0], s.shape[1], k,
                      float(lambda_mult), _lib.ptr(scores), _lib.ptr(ids), 0, _lib.stream_handle(None))
        return scores, ids

    def mmr_select_device(self, cand_scores, cand_ids, k, lambda_mult, out_scores, out_ids, stream=None):
        """mmr_select on torch device tensors (cand_* [nq, fetch_k], out_* [nq, k]),
        asynchronous on the given (or current) torch stream."""
        _lib.call("mq_index_mmr_select", self._h, _lib.ptr(cand_scores), _lib.ptr(cand_ids),
                  cand_scores.shape[0], cand_scores.shape[1], k, float(lambda_mult), _lib.ptr(out_scores),
                  _lib.ptr(out_ids), 1, _lib.stream_handle(stream))

    def search_mmr(self, queries, k, fetch_k, lambda_mult=0.5, bits=None):
        """Top-fetch_k search at the index's precision, then the MMR selection of k of them on
        the device (mq_index_search_mmr): one call, nothing row-sized leaves HBM.  `bits`: a
        row mask as for search_masked (None = every row).  -> (scores [nq, k], ids [nq, k])
        in selection order, scores = cosine to the query."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        if bits is not None:
            self._check_bits(bits)
        scores = np.empty((q.shape[0], k), dtype=np.float32)
        ids = np.empty((q.shape[0], k), dtype=np.int64)
        with _lib.device_scope(self.device):
            _lib.call("mq_index_search_mmr", self._h, _lib.ptr(q), q.shape[0], k, fetch_k, float(lambda_mult),
                      _lib.ptr(bits), _lib.ptr(scores), _lib.ptr(ids), 0, _lib.stream_handle(None))
        return scores, ids

    def _group_args(self, codes, n_groups, bits, scratch, nq, k):
        """The device checks of the grouped calls -> (n_groups, scratch)."""
        import torch
        n, n_groups, k = len(self), int(n_groups), int(k)
        if not 1 <= k <= _lib.MQ_MAX_K:
            raise ValueError("k must be in [1, %d] (got %d)" % (_lib.MQ_MAX_K, k))
        if n_groups < 0:
            raise ValueError("n_groups must be >= 0 (got %d)" % n_groups)
        if self.dim % 64 or self.dim > 1024:
            raise ValueError("the grouped scan serves dim %% 64 == 0, dim <= 1024 (got %d)" % self.dim)
        if not (getattr(codes, "is_cuda", False) and codes.dtype == torch.int32 and codes.is_contiguous()
                and codes.device.index == int(self.device) and codes.numel() >= n):
            raise ValueError("codes must be a contiguous int32 tensor of >= %d elements on cuda:%d" % (n, self.device))
        if bits is not None:
            self._check_bits(bits)
        need = group_scratch_bytes(n_groups, nq, k)
        if scratch is None:
            scratch = torch.empty(max(need, 256), dtype=torch.uint8, device=codes.device)
        if not (getattr(scratch, "is_cuda", False) and scratch.is_contiguous()
                and scratch.device.index == int(self.device)
                and scratch.numel() * scratch.element_size() >= need and scratch.data_ptr() % 16 == 0):
            raise ValueError("scratch must be a contiguous 16-byte aligned tensor of >= %d bytes on cuda:%d"
                             % (need, self.device))
        return n_groups, scratch

    def search_grouped(self, queries, k, codes, n_groups, bits=None, scratch=None):
        """Top-k distinct groups (K16, mq_index_search_grouped): codes a device int32 tensor
        [n] of each row's group code (outside [0, n_groups): the row is ignored), bits a row
        mask as for search_masked (None = every row), scratch group_scratch_bytes(n_groups,
        nq, k) device bytes (None: a torch.empty of that size).  -> (scores [nq, k], ids
        [nq, k]): each group's best score and the row reaching it (ties: the lowest row),
        groups by (score desc, row asc), padded with (-inf, -1).  Always the full scan."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        with _lib.device_scope(self.device):
            n_groups, scratch = self._group_args(codes, n_groups, bits, scratch, q.shape[0], k)
            scores = np.empty((q.shape[0], k), dtype=np.float32)
            ids = np.empty((q.shape[0], k), dtype=np.int64)
            _lib.call("mq_index_search_grouped", self._h, _lib.ptr(q), q.shape[0], int(k), _lib.ptr(codes), n_groups,
                      _lib.ptr(bits), _lib.ptr(scores), _lib.ptr(ids), 0, _lib.ptr(scratch),
                      scratch.numel() * scratch.element_size(), _lib.stream_handle(None))
        return scores, ids

    def search_grouped_device(self, queries, k, codes, n_groups, out_scores, out_ids, bits=None, scratch=None,
                              stream=None):
        """search_grouped on torch device tensors (queries [nq, dim] f32, out_scores [nq, k]
        f32, out_ids [nq, k] int64), asynchronous on the given (or current) torch stream."""
        import torch
        nq = queries.shape[0]
        for t, dt, cnt in ((queries, torch.float32, nq * self.dim), (out_scores, torch.float32, nq * int(k)),
                           (out_ids, torch.int64, nq * int(k))):
            if not (getattr(t, "is_cuda", False) and t.dtype == dt and t.is_contiguous()
                    and t.device.index == int(self.device) and t.numel() >= cnt):
                raise ValueError("queries / out_scores / out_ids must be contiguous float32 / float32 / int64 "
                                 "tensors of [nq, dim] / [nq, k] / [nq, k] on cuda:%d" % self.device)
        with _lib.device_scope(self.device):
            n_groups, scratch = self._group_args(codes, n_groups, bits, scratch, nq, k)
            if scratch.data_ptr() in (out_scores.data_ptr(), out_ids.data_ptr()):
                raise ValueError("scratch must not be one of the outputs")
            _lib.call("mq_index_search_grouped", self._h, _lib.ptr(queries), nq, int(k), _lib.ptr(codes), n_groups,
                      _lib.ptr(bits), _lib.ptr(out_scores), _lib.ptr(out_ids), 1, _lib.ptr(scratch),
                      scratch.numel() * scratch.element_size(), _lib.stream_handle(stream))

    def _range_args(self, bits, scratch, nq, max_hits, min_score):
        """The device checks of the range calls -> (max_hits, min_score, scratch)."""
        import torch
        n, max_hits, min_score = len(self), int(max_hits), float(min_score)
        if not 1 <= max_hits <= _lib.MQ_RANGE_MAX_HITS:
            raise ValueError("max_hits must be in [1, %d] (got %d)" % (_lib.MQ_RANGE_MAX_HITS, max_hits))
        if min_score != min_score:
            raise ValueError("min_score must not be NaN (-inf means no threshold)")
        if self.dim % 64 or self.dim > 1024:
            raise ValueError("the range scan serves dim %% 64 == 0, dim <= 1024 (got %d)" % self.dim)
        if bits is not None:
            self._check_bits(bits)
        need = range_scratch_bytes(n, nq, max_hits)
        if scratch is None:
            scratch = torch.empty(max(need, 256), dtype=torch.uint8, device=torch.device("cuda", int(self.device)))
        if not (getattr(scratch, "is_cuda", False) and scratch.is_contiguous()
                and scratch.device.index == int(self.device)
                and scratch.numel() * scratch.element_size() >= need and scratch.data_ptr() % 16 == 0):
            raise ValueError("scratch must be a contiguous 16-byte aligned tensor of >= %d bytes on cuda:%d"
                             % (need, self.device))
        return max_hits, min_score, scratch

    def search_range(self, queries, max_hits, min_score=-np.inf, bits=None, scratch=None):
        """Range search (K17, mq_index_search_range): the rows whose exact fp32 score is >=
        min_score (-inf: every row), among those `bits` admits (a row mask as for
        search_masked; None = every row).  scratch: range_scratch_bytes(n, nq, max_hits) device
        bytes (None: a torch.empty of that size).  -> (counts [nq] int64, scores [nq, max_hits],
        ids [nq, max_hits]): the exact number of hits, which may exceed max_hits, and the first
        min(count, max_hits) of them by (score desc, row asc), padded with (-inf, -1)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.dim)
        with _lib.device_scope(self.device):
            max_hits, min_score, scratch = self._range_args(bits, scratch, q.shape[0], max_hits, min_score)
            counts = np.empty(q.shape[0], dtype=np.int64)
            scores = np.empty((q.shape[0], max_hits), dtype=np.float32)
            ids = np.empty((q.shape[0], max_hits), dtype=np.int64)
            _lib.call("mq_index_search_range", self._h, _lib.ptr(q), q.shape[0], max_hits, min_score, _lib.ptr(bits),
                      _lib.ptr(counts), _lib.ptr(scores), _lib.ptr(ids), 0, _lib.ptr(scratch),
                      scratch.numel() * scratch.element_size(), _lib.stream_handle(None))
        return counts, scores, ids

    def search_range_device(self, queries, max_hits, out_counts, out_scores, out_ids, min_score=-np.inf, bits=None,
                            scratch=None, stream=None):
        """search_range on torch device tensors (queries [nq, dim] f32, out_counts [nq] int64,
        out_scores [nq, max_hits] f32, out_ids [nq, max_hits] int64), asynchronous on the given
        (or current) torch stream."""
        import torch
        nq = queries.shape[0]
        for t, dt, cnt in ((queries, torch.float32, nq * self.dim), (out_counts, torch.int64, nq),
                           (out_scores, torch.float32, nq * int(max_hits)), (out_ids, torch.int64, nq * int(max_hits))):
            if not (getattr(t, "is_cuda", False) and t.dtype == dt and t.is_contiguous()
                    and t.device.index == int(self.device) and t.numel() >= cnt):
                raise ValueError("queries / out_counts / out_scores / out_ids must be contiguous float32 / int64 / "
                                 "float32 / int64 tensors of [nq, dim] / [nq] / [nq, max_hits] / [nq, max_hits] on "
                                 "cuda:%d" % self.device)
        with _lib.device_scope(self.device):
            max_hits, min_score, scratch = self._range_args(bits, scratch, nq, max_hits, min_score)
            if scratch.data_ptr() in (out_counts.data_ptr(), out_scores.data_ptr(), out_ids.data_ptr()):
                raise ValueError("scratch must not be one of the outputs")
            _lib.call("mq_index_search_range", self._h, _lib.ptr(queries), nq, max_hits, min_score, _lib.ptr(bits),
                      _lib.ptr(out_counts), _lib.ptr(out_scores), _lib.ptr(out_ids), 1, _lib.ptr(scratch),
                      scratch.numel() * scratch.element_size(), _lib.stream_handle(stream))

    def _join_args(self, bits, scratch, n_left, min_score, mode):
        """The device checks of the self-join calls -> (min_score, mode, scratch)."""
        import torch
        n, min_score, mode = len(self), float(min_score), int(mode)
        if min_score != min_score:
            raise ValueError("min_score must not be NaN (-inf means no threshold)")
        if mode not in (_lib.MQ_JOIN_AUTO, _lib.MQ_JOIN_EXACT, _lib.MQ_JOIN_SCREEN):
            raise ValueError("mode must be MQ_JOIN_AUTO, MQ_JOIN_EXACT or MQ_JOIN_SCREEN (got %d)" % mode)
        if self.dim % 64 or self.dim > 1024:
            raise ValueError("the self-join serves dim %% 64 == 0, dim <= 1024 (got %d)" % self.dim)
        if mode == _lib.MQ_JOIN_SCREEN and self.dim not in (256, 512, 768):
            raise ValueError("MQ_JOIN_SCREEN serves dim 256, 512 or 768 (got %d)" % self.dim)
        if bits is not None:
            self._check_bits(bits)
        need = join_scratch_bytes(n, n_left)
        if scratch is None:
            scratch = torch.empty(max(need, 256), dtype=torch.uint8, device=torch.device("cuda", int(self.device)))
        if not (getattr(scratch, "is_cuda", False) and scratch.is_contiguous()
                and scratch.device.index == int(self.device)
                and scratch.numel() * scratch.element_size() >= need and scratch.data_ptr() % 16 == 0):
            raise ValueError("scratch must be a contiguous 16-byte aligned tensor of >= %d bytes on cuda:%d"
                             % (need, self.device))
        return min_score, mode, scratch

    def self_join(self, min_score, bits=None, left_rows=None, mode=_lib.MQ_JOIN_AUTO, scratch=None):
        """Self-join (K18, mq_index_self_join): for every left row (left_rows: distinct row ids,
        None = every row) its partners - the other rows `bits` admits (a row mask as for
        search_masked; None = every row) whose exact fp32 score against it is >= min_score.
        scratch: join_scratch_bytes(n, n_left) device bytes (None: a torch.empty of that size).
        -> (counts int64, first int64, nearest int64, nearest_scores float32, info int64 [4]),
        the first four [n_left]: the number of partners, the smallest partner row (-1: none),
        the best partner by (score desc, row asc) and its score (-1, -inf: none); info = (sum of
        the counts, left rows the screen answered, screen candidates verified, left rows the
        exact walk answered).  The modes return the same four arrays."""
        n = len(self)
        if left_rows is not None:
            left_rows = np.ascontiguousarray(left_rows, dtype=np.int64).reshape(-1)
        n_left = n if left_rows is None else len(left_rows)
        counts = np.empty(n_left, dtype=np.int64)
        first = np.empty(n_left, dtype=np.int64)
        nearest = np.empty(n_left, dtype=np.int64)
        scores = np.empty(n_left, dtype=np.float32)
        info = np.zeros(4, dtype=np.int64)
        with _lib.device_scope(self.device):
            min_score, mode, scratch = self._join_args(bits, scratch, n_left, min_score, mode)
            _lib.call("mq_index_self_join", self._h, min_score, _lib.ptr(bits), _lib.ptr(left_rows), n_left, mode,
                      _lib.ptr(counts), _lib.ptr(first), _lib.ptr(nearest), _lib.ptr(scores), _lib.ptr(info), 0,
                      _lib.ptr(scratch), scratch.numel() * scratch.element_size(), _lib.stream_handle(None))
        return counts, first, nearest, scores, info

    def self_join_device(self, min_score, out_counts, out_first, out_nearest, out_nearest_scores, out_info, bits=None,
                         left_rows=None, mode=_lib.MQ_JOIN_AUTO, scratch=None, stream=None):
        """self_join on torch device tensors (left_rows int64 [n_left] or None, out_counts /
        out_first / out_nearest int64 [n_left], out_nearest_scores float32 [n_left], out_info
        int64 [4]) on the given (or current) torch stream, which the call synchronises."""
        import torch
        n_left = len(self) if left_rows is None else left_rows.numel()
        for t, dt, cnt in ((left_rows, torch.int64, n_left), (out_counts, torch.int64, n_left),
                           (out_first, torch.int64, n_left), (out_nearest, torch.int64, n_left),
                           (out_nearest_scores, torch.float32, n_left), (out_info, torch.int64, 4)):
            if t is left_rows and t is None:
                continue
            if not (getattr(t, "is_cuda", False) and t.dtype == dt and t.is_contiguous()
                    and t.device.index == int(self.device) and t.numel() >= cnt):
                raise ValueError("left_rows / out_counts / out_first / out_nearest / out_nearest_scores / out_info must "
                                 "be contiguous int64 / int64 / int64 / int64 / float32 / int64 tensors of [n_left] "
                                 "([4] for out_info) on cuda:%d" % self.device)
        with _lib.device_scope(self.device):
            min_score, mode, scratch = self._join_args(bits, scratch, n_left, min_score, mode)
            if scratch.data_ptr() in (out_counts.data_ptr(), out_first.data_ptr(), out_nearest.data_ptr(),
                                      out_nearest_scores.data_ptr(), out_info.data_ptr()):
                raise ValueError("scratch must not be one of the outputs")
            _lib.call("mq_index_self_join", self._h, min_score, _lib.ptr(bits), _lib.ptr(left_rows), n_left, mode,
                      _lib.ptr(out_counts), _lib.ptr(out_first), _lib.ptr(out_nearest), _lib.ptr(out_nearest_scores),
                      _lib.ptr(out_info), 1, _lib.ptr(scratch), scratch.numel() * scratch.element_size(),
                      _lib.stream_handle(stream))

    def _kmeans_args(self, bits, scratch, n_clusters, n_iter):
        """The device checks of the k-means calls -> (n_iter, scratch)."""
        import torch
        n, n_iter = len(self), int(n_iter)
        if not 1 <= n_clusters <= _lib.MQ_KMEANS_MAX_CLUSTERS:
            raise ValueError("n_clusters must be in [1, %d] (got %d)" % (_lib.MQ_KMEANS_MAX_CLUSTERS, n_clusters))
        if not 0 <= n_iter <= 1024:
            raise ValueError("n_iter must be in [0, 1024] (got %d)" % n_iter)
        if self.dim % 64 or self.dim > 1024:
            raise ValueError("k-means serves dim %% 64 == 0, dim <= 1024 (got %d)" % self.dim)
        if bits is not None:
            self._check_bits(bits)
        need = kmeans_scratch_bytes(n, n_clusters)
        if scratch is None:
            scratch = torch.empty(max(need, 256), dtype=torch.uint8, device=torch.device("cuda", int(self.device)))
        if not (getattr(scratch, "is_cuda", False) and scratch.is_contiguous()
                and scratch.device.index == int(self.device)
                and scratch.numel() * scratch.element_size() >= need and scratch.data_ptr() % 16 == 0):
            raise ValueError("scratch must be a contiguous 16-byte aligned tensor of >= %d bytes on cuda:%d"
                             % (need, self.device))
        return n_iter, scratch

    def kmeans(self, centroids, n_iter, bits=None, scratch=None):
        """K-means (K19, mq_index_kmeans): n_iter Lloyd iterations from `centroids`
        [n_clusters, dim] (all finite; not modified) over the rows `bits` admits (a row mask as for
        search_masked; None = every row); n_iter = 0 only labels the rows.  scratch:
        kmeans_scratch_bytes(n, n_clusters) device bytes (None: a torch.empty of that size).
        -> (centroids float32 [n_clusters, dim], assign int32 [n], dots float32 [n], counts int64
        [n_clusters], info int64 [4]): the final centres, each row's cluster (-1: not admitted),
        its exact fp32 dot with that centre (-inf: not admitted), the cluster sizes, and info =
        (updates applied before convergence, labels changed by the last assign that ran - 0 means
        converged -, admitted rows, empty clusters)."""
        c = np.array(centroids, dtype=np.float32, order="C")  # a copy: the call overwrites it
        if c.ndim != 2 or c.shape[1] != self.dim:
            raise ValueError("centroids must be [n_clusters, %d] (got shape %r)" % (self.dim, c.shape))
        if not np.isfinite(c).all():
            raise ValueError("centroids must be finite")
        n = len(self)
        assign = np.full(n, -1, dtype=np.int32)
        dots = np.full(n, -np.inf, dtype=np.float32)
        counts = np.zeros(c.shape[0], dtype=np.int64)
        info = np.zeros(4, dtype=np.int64)
        with _lib.device_scope(self.device):
            n_iter, scratch = self._kmeans_args(bits, scratch, c.shape[0], n_iter)
            _lib.call("mq_index_kmeans", self._h, _lib.ptr(bits), c.shape[0], n_iter, _lib.ptr(c), _lib.ptr(assign),
                      _lib.ptr(dots), _lib.ptr(counts), _lib.ptr(info), 0, _lib.ptr(scratch),
                      scratch.numel() * scratch.element_size(), _lib.stream_handle(None))
        return c, assign, dots, counts, info

    def kmeans_device(self, centroids, n_iter, out_assign, out_dots, out_counts, out_info, bits=None, scratch=None,
                      stream=None):
        """kmeans on torch device tensors (centroids float32 [n_clusters, dim], updated in place;
        out_assign int32 [n], out_dots float32 [n], out_counts int64 [n_clusters], out_info int64
        [4]), asynchronous on the given (or current) torch stream."""
        import torch
        n = len(self)
        if getattr(centroids, "ndim", 0) != 2 or centroids.shape[1] != self.dim:
            raise ValueError("centroids must be [n_clusters, %d]" % self.dim)
        nc = centroids.shape[0]
        for t, dt, cnt in ((centroids, torch.float32, nc * self.dim), (out_assign, torch.int32, n),
                           (out_dots, torch.float32, n), (out_counts, torch.int64, nc), (out_info, torch.int64, 4)):
            if not (getattr(t, "is_cuda", False) and t.dtype == dt and t.is_contiguous()
                    and t.device.index == int(self.device) and t.numel() >= cnt):
                raise ValueError("centroids / out_assign / out_dots / out_counts / out_info must be contiguous float32 "
                                 "/ int32 / float32 / int64 / int64 tensors of [n_clusters, dim] / [n] / [n] / "
                                 "[n_clusters] / [4] on cuda:%d" % self.device)
        with _lib.device_scope(self.device):
            n_iter, scratch = self._kmeans_args(bits, scratch, nc, n_iter)
            if scratch.data_ptr() in (centroids.data_ptr(), out_assign.data_ptr(), out_dots.data_ptr(),
                                      out_counts.data_ptr(), out_info.data_ptr()):
                raise ValueError("scratch must not be one of the buffers")
            _lib.call("mq_index_kmeans", self._h, _lib.ptr(bits), nc, n_iter, _lib.ptr(centroids),
                      _lib.ptr(out_assign), _lib.ptr(out_dots), _lib.ptr(out_counts), _lib.ptr(out_info), 1,
                      _lib.ptr(scratch), scratch.numel() * scratch.element_size(), _lib.stream_handle(stream))

    @property
    def masked_gathers(self):
        """Masked searches the int8 screen did not certify (answered from gathered rows)."""
        n = ctypes.c_int64()
        _lib.call("mq_index_masked_gathers", self._h, ctypes.byref(n))
        return n.value

    def save_rows(self, path, row0, n):
        """Rows [row0, row0 + n) as a slab file of n rows (a store segment)."""
        _lib.call("mq_index_save_rows", self._h, str(path).encode(), int(row0), int(n))

    def load_append(self, path):
        """Append a slab file's rows, bit-identical (no re-normalisation)."""
        _lib.call("mq_index_load_append", self._h, str(path).encode())


def group_scratch_bytes(n_groups, nq, k=_lib.MQ_MAX_K):
    """Bytes of device scratch mq_index_search_grouped wants for n_groups groups, nq queries
    and a top-k of k; non-decreasing in every argument and bounded in nq."""
    return int(_lib.lib().mq_group_scratch_bytes(int(n_groups), int(nq), int(k)))


def group_scan_blocks(n_rows, compute_units):
    """Workgroups of the grouped scan over n_rows on a GPU of compute_units CUs; each holds 16
    lane groups, and lane group g walks rows g, g + 16 * blocks, ..., two per iteration."""
    return int(_lib.lib().mq_group_scan_blocks(int(n_rows), int(compute_units)))


def range_scratch_bytes(n_rows, nq, max_hits=_lib.MQ_RANGE_MAX_HITS):
    """Bytes of device scratch mq_index_search_range wants for n_rows rows, nq queries and lists
    of max_hits; non-decreasing in every argument and bounded in nq."""
    return int(_lib.lib().mq_range_scratch_bytes(int(n_rows), int(nq), int(max_hits)))


def join_scratch_bytes(n_rows, n_left):
    """Bytes of device scratch mq_index_self_join wants for n_rows rows and n_left left rows;
    non-decreasing in both."""
    return int(_lib.lib().mq_join_scratch_bytes(int(n_rows), int(n_left)))


def kmeans_scratch_bytes(n_rows, n_clusters=_lib.MQ_KMEANS_MAX_CLUSTERS):
    """Bytes of device scratch mq_index_kmeans wants for n_rows rows and n_clusters centroids;
    non-decreasing in both."""
    return int(_lib.lib().mq_kmeans_scratch_bytes(int(n_rows), int(max(-1, min(int(n_clusters), 1 << 30)))))


def range_scan_blocks(n_rows, compute_units):
    """Workgroups of the range scan over n_rows on a GPU of compute_units CUs: the grouped
    scan's geometry (16 lane groups each, lane group g walks rows g, g + 16 * blocks, ...)."""
    return int(_lib.lib().mq_range_scan_blocks(int(n_rows), int(compute_units)))


def range_select_blocks(n_rows, compute_units):
    """Workgroups per query of the range search's histogram and collect kernels; workgroup b
    walks cells b * 256 + t, + 256 * blocks, ..."""
    return int(_lib.lib().mq_range_select_blocks(int(n_rows), int(compute_units)))


def merge_topk_host(scores, ids, k_out):
    """[n_lists, nq, k_in] candidate lists -> global top-k_out (score desc, id asc)."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    n_lists, nq, k_in = scores.shape
    os_ = np.empty((nq, k_out), dtype=np.float32)
    oi = np.empty((nq, k_out), dtype=np.int64)
    _lib.call("mq_topk_merge_host", _lib.ptr(scores), _lib.ptr(ids), n_lists, nq, k_in, k_out,
              _lib.ptr(os_), _lib.ptr(oi))
    return os_, oi


def merge_topk_device(scores, ids, k_out, out_scores, out_ids, stream=None):
    n_lists, nq, k_in = scores.shape
    _lib.call("mq_topk_merge_device", _lib.ptr(scores), _lib.ptr(ids), n_lists, nq, k_in, k_out,
              _lib.ptr(out_scores), _lib.ptr(out_ids), _lib.stream_handle(stream))


class Encoder:
    """BERT encoder on one GPU (K1..K7).  `weights`: HF-named state dict, or None for
    the seeded synthetic weights of `cfg` (see weights.py).  A cross-encoder head is a
    separate upload (`load_head`); without one `score` raises."""

    def __init__(self, cfg: BertConfig, weights=None, seed=0, device=0):
        self.cfg = cfg
        self.device = device
        self._ccfg = _lib.BertConfigC.from_config(cfg)
        h = ctypes.c_void_p()
        _lib.call("mq_encoder_create", device, ctypes.byref(self._ccfg), ctypes.byref(h))
        self._h = h
        sd = weights if weights is not None else synthetic_state_dict(cfg, seed)
        blob = state_dict_to_blob(cfg, sd)
        n = _lib.lib().mq_encoder_weight_count(ctypes.byref(self._ccfg))
        if n != blob.size:
            raise ValueError("weight blob %d floats, library expects %d" % (blob.size, n))
        _lib.call("mq_encoder_load_weights", self._h, _lib.ptr(blob), blob.size)
        self.n_labels = 0

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().mq_encoder_destroy(h)
            except Exception:  # interpreter shutdown
                pass

    __del__ = close

    STAGES = ("embed_ln", "qkv_gemm", "attention", "out_proj_gemm", "layernorm", "ffn_up_gemm",
              "ffn_down_gemm", "pool")

    def set_timing(self, enabled=True):
        _lib.call("mq_encoder_set_timing", self._h, int(bool(enabled)))

    def read_timing(self):
        ms = np.zeros(len(self.STAGES), dtype=np.float32)
        _lib.call("mq_encoder_read_timing", self._h, _lib.ptr(ms), len(ms))
        return dict(zip(self.STAGES, ms.tolist()))

    def set_precision(self, dtype):
        _lib.call("mq_encoder_set_precision", self._h, dtype)

    def set_graphs(self, enabled=True):
        """Replay forwards as captured hipGraphs (default off: eager measured faster on
        MI355X for one query; bit-identical results)."""
        _lib.call("mq_encoder_set_graphs", self._h, int(bool(enabled)))

    OPTIONS = {"rows_max": _lib.MQ_ENC_OPT_ROWS_MAX, "rows_splits": _lib.MQ_ENC_OPT_ROWS_SPLITS,
               "splitk_max": _lib.MQ_ENC_OPT_SPLITK_MAX, "fuse_attn_oproj": _lib.MQ_ENC_OPT_FUSE_ATTN_OPROJ,
               "splitk_tiles": _lib.MQ_ENC_OPT_SPLITK_TILES,
               "resident_layers": _lib.MQ_ENC_OPT_RESIDENT_LAYERS, "x6_presplit": _lib.MQ_ENC_OPT_X6_PRESPLIT,
               "rows_planes": _lib.MQ_ENC_OPT_ROWS_PLANES, "ln_fold": _lib.MQ_ENC_OPT_LN_FOLD,
               "cls_kfree": _lib.MQ_ENC_OPT_CLS_KFREE, "qkv_attn": _lib.MQ_ENC_OPT_QKV_ATTN,
               "epi_split": _lib.MQ_ENC_OPT_EPI_SPLIT}

    def set_option(self, name, value):
        """Tuning option of the forward (mq_encoder_set_option): rows_max, rows_splits,
        splitk_max, fuse_attn_oproj, splitk_tiles,
        resident_layers (0..1024, default 8: the few-row forward loads layers below this
        index with the default cache policy and later layers non-temporally, so the first
        layers' weights stay in MALL between single queries; outputs are bit-identical),
        x6_presplit (split-f32 precision: 1, default, multiplies the weights' W3 plane images
        split once at load; 0 = the tiles that re-split both operands; bit-identical),
        rows_planes (few-row forward: 0, default, merges the two-addend hand-offs into one plane
        by atomic adds; 1 = two planes; bit-identical), cls_kfree (CLS pooling, batched forward:
        1, default, the last layer attends from the CLS query without projecting K and V; 0 =
        the all-token K / V projection and the attention kernel; equal to rounding), qkv_attn
        (split-f32 precision, batched forward, L == 32: 1, default, the attention runs in the
        QKV GEMM's epilogue; 0 = the QKV launch and the attention launch; equal to rounding),
        epi_split (split-f32 precision, x6_presplit 1: 1, default, shares each GELU tile
        epilogue of the loader-wave split-f32 tiles between the compute wave and the loader wave of
        its SIMD; 0 = the compute wave alone; bit-identical)."""
        _lib.call("mq_encoder_set_option", self._h, self.OPTIONS[name], int(value))

    def get_option(self, name):
        v = ctypes.c_int()
        _lib.call("mq_encoder_get_option", self._h, self.OPTIONS[name], ctypes.byref(v))
        return v.value

    def embed(self, ids, mask):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        mask = np.ascontiguousarray(mask, dtype=np.int32)
        B, L = ids.shape
        out = np.empty((B, self.cfg.hidden), dtype=np.float32)
        _lib.call("mq_encoder_embed", self._h, _lib.ptr(ids), _lib.ptr(mask), B, L, _lib.ptr(out),
                  0, None)
        return out

    def embed_device(self, ids, mask, out, stream=None):
        """ids/mask int32 [B, L], out f32 [B, hidden] - torch device tensors."""
        B, L = ids.shape
        _lib.call("mq_encoder_embed", self._h, _lib.ptr(ids), _lib.ptr(mask), B, L, _lib.ptr(out),
                  1, _lib.stream_handle(stream))

    def load_head(self, sd):
        """Upload a cross-encoder head (mq_encoder_load_head): `sd` holds pooler.dense.* and
        classifier.* (weights.HEAD_NAMES); n_labels = classifier.weight's rows, 1..8, checked
        here before any HIP call.  Loading again replaces the head."""
        pw, pb, cw, cb = head_from_state_dict(sd, self.cfg)
        n_labels = int(cw.shape[0])
        if not 1 <= n_labels <= _lib.MQ_HEAD_MAX_LABELS:
            raise ValueError("n_labels must be in [1, %d] (got %d)" % (_lib.MQ_HEAD_MAX_LABELS, n_labels))
        _lib.call("mq_encoder_load_head", self._h, _lib.ptr(pw), _lib.ptr(pb), _lib.ptr(cw), _lib.ptr(cb), n_labels)
        self.n_labels = n_labels

    def score(self, ids, types, mask):
        """Cross-encoder logits float32 [B, n_labels] of token pairs: ids / types (segment
        ids) / mask int [B, L] host arrays (mq_encoder_score)."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        types = np.ascontiguousarray(types, dtype=np.int32)
        mask = np.ascontiguousarray(mask, dtype=np.int32)
        if types.shape != ids.shape or mask.shape != ids.shape or ids.ndim != 2:
            raise ValueError("ids, types and mask must share one [B, L] shape")
        B, L = ids.shape
        out = np.empty((B, max(1, self.n_labels)), dtype=np.float32)
        _lib.call("mq_encoder_score", self._h, _lib.ptr(ids), _lib.ptr(types), _lib.ptr(mask), B, L,
                  _lib.ptr(out), 0, None)
        return out

    def score_device(self, ids, types, mask, out, stream=None):
        """ids / types / mask int32 [B, L], out f32 [B, n_labels] - contiguous torch device
        tensors; asynchronous on the given (or current) torch stream."""
        if tuple(types.shape) != tuple(ids.shape) or tuple(mask.shape) != tuple(ids.shape):
            raise ValueError("ids, types and mask must share one [B, L] shape")
        B, L = ids.shape
        if out.numel() < B * max(1, self.n_labels):
            raise ValueError("out holds %d floats, needs B * n_labels = %d" % (out.numel(), B * self.n_labels))
        _lib.call("mq_encoder_score", self._h, _lib.ptr(ids), _lib.ptr(types), _lib.ptr(mask), B, L,
                  _lib.ptr(out), 1, _lib.stream_handle(stream))


def check_mask_words(bits, n, device=None):
    """A row mask for n rows: a contiguous 4-byte-element device tensor (on `device` when
    given) of >= ceil(n / 32) words - else ValueError (the kernels would read or write past
    its end, or on another GPU's memory)."""
    if not (getattr(bits, "is_cuda", False) and bits.element_size() == 4 and bits.is_contiguous()
            and bits.numel() >= (int(n) + 31) // 32):
        raise ValueError("bits must be a contiguous 32-bit device tensor of >= ceil(n / 32) = %d words"
                         % ((int(n) + 31) // 32))
    if device is not None and bits.device.index != int(device):
        raise ValueError("bits lives on cuda:%s, the index on cuda:%d" % (bits.device.index, int(device)))


def _check_codes(codes, bits):
    import torch
    if not (getattr(codes, "is_cuda", False) and codes.dtype == torch.int32 and codes.is_contiguous()):
        raise ValueError("codes must be a contiguous int32 device tensor")
    check_mask_words(bits, codes.numel(), codes.device.index)


def mask_eval(codes, lut, bits, mode, stream=None):
    """bits (mode)= lut[codes] on the device (include/mq.h mq_mask_eval): codes int32 [n]
    (-1 = key absent -> lut[-1]), lut uint8 [n_lut], bits int32 [ceil(n / 32)] (torch,
    one device; the launch runs there, on `stream` or that device's current stream)."""
    import torch
    _check_codes(codes, bits)
    if not (getattr(lut, "is_cuda", False) and lut.dtype == torch.uint8 and lut.is_contiguous()
            and lut.device == codes.device and lut.numel() >= 1):
        raise ValueError("lut must be a non-empty contiguous uint8 tensor on the codes' device")
    with _lib.device_scope(codes.device.index):
        _lib.call("mq_mask_eval", _lib.ptr(codes), codes.numel(), _lib.ptr(lut), lut.numel(), _lib.ptr(bits),
                  mode, _lib.stream_handle(stream))


def mask_eval_bits(codes, lut, bits, mode, stream=None):
    """mask_eval with a table of <= 256 entries passed by value (numpy bool / uint8 lut)."""
    _check_codes(codes, bits)
    lut = np.asarray(lut).astype(bool)
    if not 1 <= lut.size <= 256:
        raise ValueError("a by-value table holds 1..256 entries (got %d)" % lut.size)
    words = np.zeros(4, dtype=np.uint64)
    for i in np.flatnonzero(lut).tolist():
        words[i >> 6] |= np.uint64(1 << (i & 63))
    with _lib.device_scope(codes.device.index):
        _lib.call("mq_mask_eval_bits", _lib.ptr(codes), codes.numel(), _lib.ptr(words), len(lut), _lib.ptr(bits),
                  mode, _lib.stream_handle(stream))


def mask_contains(text, offsets, pattern, bits, mode, negate=False, stream=None, scratch=None):
    """bits (mode)= (pattern occurs in row r) ^ negate on the device (include/mq.h
    mq_mask_contains): text uint8 [text_bytes] = the rows' UTF-8 bytes concatenated, offsets
    int64 [n + 1] (row r = text[offsets[r]:offsets[r + 1]]), pattern 1..MQ_CONTAINS_MAX_BYTES
    host bytes, bits int32 [ceil(n / 32)] (torch, one device; the launch runs there, on
    `stream` or that device's current stream).  scratch: ceil(n / 32) words the call
    overwrites (None: a torch.empty of that size)."""
    import torch
    if not (getattr(text, "is_cuda", False) and text.dtype == torch.uint8 and text.is_contiguous()
            and text.dim() == 1):
        raise ValueError("text must be a contiguous 1-d uint8 device tensor")
    if text.numel() and text.data_ptr() % 16:
        raise ValueError("text must start at a 16-byte aligned address")
    if not (getattr(offsets, "is_cuda", False) and offsets.dtype == torch.int64 and offsets.is_contiguous()
            and offsets.numel() >= 1 and offsets.device == text.device):
        raise ValueError("offsets must be a contiguous int64 tensor of n + 1 elements on the text's device")
    n = offsets.numel() - 1
    check_mask_words(bits, n, text.device.index)
    if not isinstance(pattern, (bytes, bytearray)) or not 1 <= len(pattern) <= _lib.MQ_CONTAINS_MAX_BYTES:
        raise ValueError("pattern must be 1..%d bytes" % _lib.MQ_CONTAINS_MAX_BYTES)
    with _lib.device_scope(text.device.index):
        if scratch is None:
            scratch = torch.empty(max(1, (n + 31) // 32), dtype=torch.int32, device=text.device)
        check_mask_words(scratch, n, text.device.index)
        if scratch.data_ptr() == bits.data_ptr():
            raise ValueError("scratch must not be bits")
        _lib.call("mq_mask_contains", _lib.ptr(text), text.numel(), _lib.ptr(offsets), n, bytes(pattern),
                  len(pattern), int(bool(negate)), _lib.ptr(bits), mode, _lib.ptr(scratch),
                  _lib.stream_handle(stream))


def lex_scratch_bytes(n, k=_lib.MQ_MAX_K):
    """Bytes of device scratch mq_lex_df / mq_lex_topk want for n rows and a top-k of k."""
    return int(_lib.lib().mq_lex_scratch_bytes(int(n), int(k)))


def _check_lex(tokens, offsets, ngram, keys, scratch, k):
    """The device and size checks shared by lex_df / lex_topk -> (n, keys uint32, scratch)."""
    import torch
    if not (getattr(tokens, "is_cuda", False) and tokens.dtype == torch.uint16 and tokens.is_contiguous()
            and tokens.dim() == 1):
        raise ValueError("tokens must be a contiguous 1-d uint16 device tensor")
    if tokens.numel() and tokens.data_ptr() % 16:
        raise ValueError("tokens must start at a 16-byte aligned address")
    if not (getattr(offsets, "is_cuda", False) and offsets.dtype == torch.int64 and offsets.is_contiguous()
            and offsets.numel() >= 1 and offsets.device == tokens.device):
        raise ValueError("offsets must be a contiguous int64 tensor of n + 1 elements on the tokens' device")
    if ngram not in (1, 2):
        raise ValueError("ngram must be 1 or 2 (got %r)" % (ngram,))
    n = offsets.numel() - 1
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
    if not 1 <= keys.size <= _lib.MQ_LEX_MAX_TERMS:
        raise ValueError("a call takes 1..%d terms (got %d)" % (_lib.MQ_LEX_MAX_TERMS, keys.size))
    if np.unique(keys).size != keys.size:
        raise ValueError("keys must be distinct")
    need = lex_scratch_bytes(n, k)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=tokens.device)
    if not (getattr(scratch, "is_cuda", False) and scratch.is_contiguous() and scratch.device == tokens.device
            and scratch.numel() * scratch.element_size() >= need and scratch.data_ptr() % 16 == 0):
        raise ValueError("scratch must be a contiguous 16-byte aligned tensor of >= %d bytes on the tokens' device"
                         % need)
    return n, keys, scratch


def lex_df(tokens, offsets, ngram, keys, scratch=None, stream=None):
    """Document frequencies int64 [n_terms] of the term keys over the token mirror (include/mq.h
    mq_lex_df): tokens uint16 [n_tokens] = the rows' token ids concatenated, offsets int64
    [n + 1] in tokens (torch, one device), keys 1..MQ_LEX_MAX_TERMS distinct uint32 (host).
    scratch: lex_scratch_bytes(n, 1) bytes (None: a torch.empty of that size).  Synchronous."""
    n, keys, scratch = _check_lex(tokens, offsets, ngram, keys, scratch, 1)
    df = np.zeros(keys.size, dtype=np.int64)
    with _lib.device_scope(tokens.device.index):
        _lib.call("mq_lex_df", _lib.ptr(tokens) if tokens.numel() else None, tokens.numel(), _lib.ptr(offsets), n,
                  int(ngram), _lib.ptr(keys), keys.size, _lib.ptr(df), _lib.ptr(scratch),
                  _lib.stream_handle(stream))
    return df


def lex_topk(tokens, offsets, ngram, keys, w, c0, c1, k, bits=None, scratch=None, stream=None, out=None):
    """BM25 top-k over the token mirror (include/mq.h mq_lex_topk): keys / w the query's distinct
    term keys and their fp32 weights (host), c0, c1 the length normalisation, bits a device row
    mask or None.  -> (scores f32 [k], ids int64 [k]) device tensors (`out`: a pair to write
    into), best first, padded with (-inf, -1); asynchronous on `stream` (or the device's
    current stream)."""
    import torch
    k = int(k)
    if not 1 <= k <= _lib.MQ_MAX_K:
        raise ValueError("k must be in [1, %d] (got %d)" % (_lib.MQ_MAX_K, k))
    n, keys, scratch = _check_lex(tokens, offsets, ngram, keys, scratch, k)
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    if w.size != keys.size:
        raise ValueError("%d keys, %d weights" % (keys.size, w.size))
    if bits is not None:
        check_mask_words(bits, n, tokens.device.index)
    with _lib.device_scope(tokens.device.index):
        if out is None:
            out = (torch.empty(k, dtype=torch.float32, device=tokens.device),
                   torch.empty(k, dtype=torch.int64, device=tokens.device))
        s, i = out
        if not (s.is_cuda and i.is_cuda and s.device == tokens.device and i.device == tokens.device
                and s.dtype == torch.float32 and i.dtype == torch.int64 and s.numel() >= k and i.numel() >= k
                and s.is_contiguous() and i.is_contiguous()):
            raise ValueError("out must be (float32 [k], int64 [k]) contiguous tensors on the tokens' device")
        _lib.call("mq_lex_topk", _lib.ptr(tokens) if tokens.numel() else None, tokens.numel(), _lib.ptr(offsets), n,
                  int(ngram), _lib.ptr(keys), _lib.ptr(w), keys.size, ctypes.c_float(float(c0)),
                  ctypes.c_float(float(c1)), _lib.ptr(bits), k, _lib.ptr(s), _lib.ptr(i), 1, _lib.ptr(scratch),
                  _lib.stream_handle(stream))
    return s, i


def lex_batch_scratch_bytes(n, nq, total_terms, k=_lib.MQ_MAX_K):
    """Bytes of device scratch mq_lex_topk_batch wants for n rows, nq queries of total_terms
    terms in all and a top-k of k (mq_lex_df_batch: nq = 0, total_terms = its keys, k = 1);
    non-decreasing in every argument and bounded in nq and total_terms."""
    return int(_lib.lib().mq_lex_batch_scratch_bytes(int(n), int(nq), int(total_terms), int(k)))


def _check_lex_mirror(tokens, offsets, ngram):
    """The device checks of the token mirror shared by the batch calls -> n."""
    import torch
    if not (getattr(tokens, "is_cuda", False) and tokens.dtype == torch.uint16 and tokens.is_contiguous()
            and tokens.dim() == 1):
        raise ValueError("tokens must be a contiguous 1-d uint16 device tensor")
    if tokens.numel() and tokens.data_ptr() % 16:
        raise ValueError("tokens must start at a 16-byte aligned address")
    if not (getattr(offsets, "is_cuda", False) and offsets.dtype == torch.int64 and offsets.is_contiguous()
            and offsets.numel() >= 1 and offsets.device == tokens.device):
        raise ValueError("offsets must be a contiguous int64 tensor of n + 1 elements on the tokens' device")
    if ngram not in (1, 2):
        raise ValueError("ngram must be 1 or 2 (got %r)" % (ngram,))
    return offsets.numel() - 1


def _batch_scratch(scratch, need, device):
    import torch
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=device)
    if not (getattr(scratch, "is_cuda", False) and scratch.is_contiguous() and scratch.device == device
            and scratch.numel() * scratch.element_size() >= need and scratch.data_ptr() % 16 == 0):
        raise ValueError("scratch must be a contiguous 16-byte aligned tensor of >= %d bytes on the tokens' device"
                         % need)
    return scratch


def lex_df_batch(tokens, offsets, ngram, keys, scratch=None, stream=None):
    """Document frequencies int64 [n_keys] of any number (>= 1) of distinct uint32 term keys
    (host) over the token mirror (include/mq.h mq_lex_df_batch): equal to lex_df's, in as many
    passes of MQ_LEX_BATCH_UNION keys as it takes and one synchronise.  scratch:
    lex_batch_scratch_bytes(n, 0, n_keys, 1) bytes (None: a torch.empty of that size)."""
    n = _check_lex_mirror(tokens, offsets, ngram)
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
    if keys.size < 1:
        raise ValueError("a call takes at least 1 key (got 0)")
    if np.unique(keys).size != keys.size:
        raise ValueError("keys must be distinct")
    df = np.zeros(keys.size, dtype=np.int64)
    with _lib.device_scope(tokens.device.index):
        scratch = _batch_scratch(scratch, lex_batch_scratch_bytes(n, 0, keys.size, 1), tokens.device)
        _lib.call("mq_lex_df_batch", _lib.ptr(tokens) if tokens.numel() else None, tokens.numel(),
                  _lib.ptr(offsets), n, int(ngram), _lib.ptr(keys), keys.size, _lib.ptr(df), _lib.ptr(scratch),
                  _lib.stream_handle(stream))
    return df


def lex_topk_batch(tokens, offsets, ngram, plans, c0, c1, k, bits=None, scratch=None, stream=None, out=None):
    """BM25 top-k of a batch of queries in one call (include/mq.h mq_lex_topk_batch): plans a
    list of (keys, w), each query's 0..MQ_LEX_MAX_TERMS distinct term keys and their fp32 weights
    (host); c0, c1, bits and k shared.  -> (scores f32 [nq, k], ids int64 [nq, k]) device tensors
    (`out`: a pair to write into); row j is bit for bit lex_topk's result for plans[j].
    Asynchronous on `stream` (or the device's current stream) once the tables are copied."""
    import torch
    k = int(k)
    if not 1 <= k <= _lib.MQ_MAX_K:
        raise ValueError("k must be in [1, %d] (got %d)" % (_lib.MQ_MAX_K, k))
    n = _check_lex_mirror(tokens, offsets, ngram)
    nq = len(plans)
    term_start = np.zeros(nq + 1, dtype=np.int64)
    all_keys, all_w = [], []
    for j, (keys, w) in enumerate(plans):
        keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(-1)
        w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
        if keys.size > _lib.MQ_LEX_MAX_TERMS:
            raise ValueError("a query takes 0..%d terms (query %d has %d)" % (_lib.MQ_LEX_MAX_TERMS, j, keys.size))
        if np.unique(keys).size != keys.size:
            raise ValueError("keys must be distinct within a query (query %d)" % j)
        if w.size != keys.size:
            raise ValueError("query %d: %d keys, %d weights" % (j, keys.size, w.size))
        term_start[j + 1] = term_start[j] + keys.size
        all_keys.append(keys)
        all_w.append(w)
    keys = np.concatenate(all_keys) if all_keys else np.zeros(0, np.uint32)
    w = np.concatenate(all_w) if all_w else np.zeros(0, np.float32)
    if bits is not None:
        check_mask_words(bits, n, tokens.device.index)
    with _lib.device_scope(tokens.device.index):
        if out is None:
            out = (torch.empty((nq, k), dtype=torch.float32, device=tokens.device),
                   torch.empty((nq, k), dtype=torch.int64, device=tokens.device))
        s, i = out
        if not (s.is_cuda and i.is_cuda and s.device == tokens.device and i.device == tokens.device
                and s.dtype == torch.float32 and i.dtype == torch.int64 and s.numel() >= nq * k
                and i.numel() >= nq * k and s.is_contiguous() and i.is_contiguous()):
            raise ValueError("out must be (float32 [nq, k], int64 [nq, k]) contiguous tensors on the tokens' device")
        if nq == 0:
            return s, i
        scratch = _batch_scratch(scratch, lex_batch_scratch_bytes(n, nq, keys.size, k), tokens.device)
        _lib.call("mq_lex_topk_batch", _lib.ptr(tokens) if tokens.numel() else None, tokens.numel(),
                  _lib.ptr(offsets), n, int(ngram), nq, _lib.ptr(term_start), _lib.ptr(keys), _lib.ptr(w),
                  ctypes.c_float(float(c0)), ctypes.c_float(float(c1)), _lib.ptr(bits), k, _lib.ptr(s), _lib.ptr(i), 1,
                  _lib.ptr(scratch), _lib.stream_handle(stream))
    return s, i


def mask_combine(dst, src, mode, stream=None):
    """dst (mode)= src (None: all ones; MQ_MASK_CLEAR: zeros) on the device."""
    check_mask_words(dst, 0)
    if src is not None:
        check_mask_words(src, 32 * dst.numel(), dst.device.index)
    with _lib.device_scope(dst.device.index):
        _lib.call("mq_mask_combine", _lib.ptr(dst), _lib.ptr(src), dst.numel(), mode, _lib.stream_handle(stream))

