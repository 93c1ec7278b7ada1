"""The device top-k merge (K10) called directly, through mq_debug_topk_merge and the public
mq_topk_merge_device, against merge_cases.merge_reference: every case on each kernel form and
both id widths, the overflow flag's two bits on truncated lists, and determinism where the
survivors' LDS order is an atomicAdd's.  Every comparison is exact (merge_cases.py).

Outputs are pre-filled with (NaN, -7) and the flag word with a bit pattern, so a slot the
kernel does not write - or a flag the hook does not zero - cannot pass."""
import numpy as np
import pytest

import merge_cases as mc
from mediquery_hip import _lib
from mediquery_hip.native import merge_topk_device, merge_topk_host

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2)


def _outputs(nq, k_out, dev):
    import torch
    return (torch.full((nq, k_out), float("nan"), dtype=torch.float32, device=dev),
            torch.full((nq, k_out), -7, dtype=torch.int64, device=dev))


def run_hook(s, i, k_out, form=0, list_kc=0, kc=0, with_flag=False):
    """-> (scores [nq, k_out], ids [nq, k_out], flag or None); ids' dtype picks the id width."""
    import torch
    dev = torch.device("cuda", 0)
    n_lists, nq, k_in = s.shape
    sd = torch.from_numpy(np.array(s, order="C")).to(dev)        # a copy: the cases are read-only
    idd = torch.from_numpy(np.array(i, order="C")).to(dev)
    os_, oi = _outputs(nq, k_out, dev)
    flag = torch.full((1,), 0x55555555, dtype=torch.int32, device=dev) if with_flag else None
    with _lib.device_scope(0):
        _lib.call("mq_debug_topk_merge", _lib.ptr(sd), _lib.ptr(idd), 8 * i.dtype.itemsize, n_lists, nq, k_in,
                  k_out, list_kc, kc, form, _lib.ptr(os_), _lib.ptr(oi), _lib.ptr(flag), _lib.stream_handle(None))
    torch.cuda.synchronize()
    return os_.cpu().numpy(), oi.cpu().numpy(), (int(flag.item()) if with_flag else None)


def run_public(s, i, k_out):
    import torch
    dev = torch.device("cuda", 0)
    os_, oi = _outputs(s.shape[1], k_out, dev)
    merge_topk_device(torch.from_numpy(np.array(s, order="C")).to(dev),
                      torch.from_numpy(np.array(i, dtype=np.int64, order="C")).to(dev), k_out, os_, oi)
    torch.cuda.synchronize()
    return os_.cpu().numpy(), oi.cpu().numpy()


def same_bits(a, b):
    return (a[0].view(np.uint32) == b[0].view(np.uint32)).all() and (a[1] == b[1]).all()


# ------------------------------------------------------------------------- result ----
@pytest.mark.parametrize("case", mc.CASES, ids=repr)
def test_every_form_and_id_width_equals_the_reference(require_gpu, case):
    for bits in (32, 64):
        s, i = mc.case_data(case, bits)
        ref = mc.case_reference(case, bits)
        got = {}
        for form in FORMS:
            gs, gi, _ = run_hook(s, i, case.k_out, form=form)
            got[form] = (gs, gi)
            assert mc.mismatch(gs, gi, *ref) == "", (case, bits, form)
        assert same_bits(got[1], got[2]), (case, bits)


def test_negative_zero_ties_positive_zero(require_gpu):
    """[(+0.0, id 5)] and [(-0.0, id 3)]: id 3 first on every form, id width, list order and
    batch size (a batch of 40 takes the public call to the thread lists, one query to the
    threshold kernel)."""
    s, i = mc.zero_sign_lists()
    for ss, ii in ((s, i), (s[::-1], i[::-1])):
        for dt in (np.int32, np.int64):
            for form in FORMS:
                for k_out, want in ((1, [3]), (2, [3, 5])):
                    gs, gi, _ = run_hook(ss, ii.astype(dt), k_out, form=form)
                    print("form %d ids %s k_out %d -> %s" % (form, dt.__name__, k_out, gi.tolist()))
                    assert gi.tolist() == [want], (form, dt, k_out)
                    assert (gs == 0).all()
        for nq in (1, 40):
            sb, ib = np.repeat(ss, nq, axis=1), np.repeat(ii, nq, axis=1)
            assert run_public(sb, ib, 1)[1].tolist() == [[3]] * nq, nq
            assert merge_topk_host(np.ascontiguousarray(sb), np.ascontiguousarray(ib), 1)[1].tolist() == [[3]] * nq


# -------------------------------------------------------------------- public call ----
@pytest.mark.parametrize("case", mc.CASES, ids=repr)
def test_public_call_equals_host_and_reference(require_gpu, case):
    s, i = mc.case_data(case, 64)
    ref = mc.case_reference(case, 64)
    got = run_public(s, i, case.k_out)
    assert mc.mismatch(*got, *ref) == "", case
    assert mc.mismatch(*got, *merge_topk_host(s, i, case.k_out)) == "", case
    # row j of the batch is query j merged alone (the lists are list-major)
    for j in sorted({0, case.nq // 2, case.nq - 1}) if case.nq > 1 else ():
        one = run_public(s[:, j:j + 1, :], i[:, j:j + 1, :], case.k_out)
        assert same_bits(one, (got[0][j:j + 1], got[1][j:j + 1])), (case, j)


def test_public_call_empty_batch_and_argument_checks(require_gpu):
    import torch
    dev = torch.device("cuda", 0)
    s = torch.zeros((3, 4, 5), dtype=torch.float32, device=dev)
    i = torch.arange(60, dtype=torch.int64, device=dev).reshape(3, 4, 5)
    os_, oi = _outputs(4, 2, dev)
    h = _lib.stream_handle(None)
    _lib.call("mq_topk_merge_device", _lib.ptr(s), _lib.ptr(i), 3, 0, 5, 2, _lib.ptr(os_), _lib.ptr(oi), h)
    _lib.call("mq_debug_topk_merge", _lib.ptr(s), _lib.ptr(i), 64, 3, 0, 5, 2, 0, 0, 0, _lib.ptr(os_), _lib.ptr(oi),
              None, h)
    torch.cuda.synchronize()
    assert torch.isnan(os_).all() and (oi == -7).all()           # nq == 0 writes nothing
    for k_out in (0, 65):
        with pytest.raises(_lib.MQError, match="k_out must be"):
            _lib.call("mq_topk_merge_device", _lib.ptr(s), _lib.ptr(i), 3, 4, 5, k_out, _lib.ptr(os_), _lib.ptr(oi), h)
    for n_lists, k_in in ((0, 5), (3, 0)):
        with pytest.raises(_lib.MQError, match="bad merge shape"):
            _lib.call("mq_topk_merge_device", _lib.ptr(s), _lib.ptr(i), n_lists, 4, k_in, 2, _lib.ptr(os_),
                      _lib.ptr(oi), h)
    for args in ((None, _lib.ptr(i), _lib.ptr(os_), _lib.ptr(oi)), (_lib.ptr(s), None, _lib.ptr(os_), _lib.ptr(oi)),
                 (_lib.ptr(s), _lib.ptr(i), None, _lib.ptr(oi)), (_lib.ptr(s), _lib.ptr(i), _lib.ptr(os_), None)):
        with pytest.raises(_lib.MQError, match="NULL buffer"):
            _lib.call("mq_topk_merge_device", args[0], args[1], 3, 4, 5, 2, args[2], args[3], h)
    torch.cuda.synchronize()
    assert torch.isnan(os_).all() and (oi == -7).all()           # a refused call writes nothing either


# -------------------------------------------------------------- overflow protocol ----
def _check_overflow(name, full, tr, list_kc, kc, k_out, bit0_must=None):
    """The module docstring's statements for one input: `tr` the truncated lists the kernel
    gets (32-bit ids), `full` the lists they were cut from."""
    ts, ti = tr
    ref_tr = mc.merge_reference(ts, ti, k_out)
    ref_full = mc.merge_reference(full[0], full[1], k_out)
    b0 = mc.bit0_expected(ts, ti, list_kc, k_out)
    b1 = mc.bit1_possible(ts, ti, kc, k_out)
    if bit0_must is not None:
        assert b0 == bit0_must, name
    for form in FORMS:
        gs, gi, flag = run_hook(ts, ti, k_out, form=form, list_kc=list_kc, kc=kc, with_flag=True)
        print("%s form %d: flag %d, bit0 expected %s, bit1 possible %s" % (name, form, flag, b0, b1))
        assert 0 <= flag <= 3, (name, form, flag)
        if flag & 2:
            assert b1, (name, form, "bit 1 set where no thread list can have dropped a member")
        else:
            assert mc.mismatch(gs, gi, *ref_tr) == "", (name, form)
            assert bool(flag & 1) == b0, (name, form, flag)
        if b0:      # a worse k-th (after a dropped member) only makes the test easier to pass
            assert flag & 1, (name, form, flag)
        if flag == 0:
            assert mc.mismatch(gs, gi, *ref_full) == "", (name, form, "zero flag, yet not the full lists' top-k")
        # the re-merge: 64-entry thread lists, no flag
        rs, ri, _ = run_hook(ts, ti, k_out, form=form, list_kc=list_kc, kc=64)
        assert mc.mismatch(rs, ri, *ref_tr) == "", (name, form, "re-merge")


@pytest.mark.parametrize("case", mc.OVERFLOW, ids=repr)
def test_overflow_flag_on_truncated_lists(require_gpu, case):
    _check_overflow(case.name, mc.case_data(case, 32), mc.truncated(case, 32), case.list_kc, case.kc, case.k_out,
                    case.bit0)


def test_overflow_flag_full_lists_that_merely_tie(require_gpu):
    s, i, list_kc, kc, k_out = mc.tie_full_lists()
    _check_overflow("tie-full", (s, i), (s, i), list_kc, kc, k_out, bit0_must=False)
    # the flag is one word for the batch: one query that hides a member sets it for all
    hidden = next(c for c in mc.OVERFLOW if c.bit0)
    ts, ti = mc.truncated(hidden, 32)
    quiet = next(c for c in mc.OVERFLOW if c.bit0 is False and c.list_kc == hidden.list_kc)
    qs, qi = mc.truncated(quiet, 32)
    n = min(ts.shape[0], qs.shape[0])
    bs = np.concatenate([qs[:n, :1], ts[:n, :1], qs[:n, 1:2]], axis=1)
    bi = np.concatenate([qi[:n, :1], ti[:n, :1], qi[:n, 1:2]], axis=1)
    assert mc.bit0_expected(bs, bi, hidden.list_kc, 64) and not mc.bit0_expected(bs[:, ::2], bi[:, ::2],
                                                                                  hidden.list_kc, 64)
    for form in FORMS:
        assert run_hook(bs, bi, 64, form=form, list_kc=hidden.list_kc, kc=64, with_flag=True)[2] == 1
        assert run_hook(np.ascontiguousarray(bs[:, ::2]), np.ascontiguousarray(bi[:, ::2]), 64, form=form,
                        list_kc=hidden.list_kc, kc=64, with_flag=True)[2] == 0


@pytest.mark.parametrize("list_kc,kc,k_out", mc.KNIFE_EDGES)
def test_overflow_flag_at_the_knife_edge(require_gpu, list_kc, kc, k_out):
    """The one full list's last kept entry at result rank k_out - 1 (bit 0 due), k_out (the
    k-th itself: clear) and k_out + 1 (clear), tying on the score with its neighbours; one
    query (threshold kernel) and a batch of 33 (thread lists when k_out <= 16)."""
    for rank in (k_out - 1, k_out, k_out + 1):
        for nq in (1, 33):
            s, i = mc.knife_edge_lists(list_kc, k_out, rank, nq)
            _check_overflow("edge-%d-%d-k%d-rank%d-nq%d" % (list_kc, kc, k_out, rank, nq), (s, i), (s, i), list_kc,
                            kc, k_out, bit0_must=rank < k_out)
            for form in FORMS:   # kc >= k_out: no bit 1, the flag is bit 0 alone
                flag = run_hook(s, i, k_out, form=form, list_kc=list_kc, kc=64, with_flag=True)[2]
                assert flag == int(rank < k_out), (rank, nq, form, flag)


# -------------------------------------------------------------------- determinism ----
@pytest.mark.parametrize("case", mc.CROWDED, ids=repr)
def test_crowded_threshold_is_deterministic(require_gpu, case):
    s, i = mc.case_data(case, 32)
    for form in (0, 2):
        first = run_hook(s, i, case.k_out, form=form)
        for _ in range(2):
            again = run_hook(s, i, case.k_out, form=form)
            assert same_bits(first, again), (case, form)
