"""GPU: the class builder (classes_launch in csrc/unique.hip: two radix sorts, the low-half gather of k_sig_heads,
the max-scan; k_dlv_best_gap / k_dlv_rep in csrc/delivery.hip) on crafted signatures, through nmz_sig_classes_dev and
nmz_delivery_classes_dev, against tests/sig_ref.py's dict and the header's representative rule.

Real 128-bit signatures never agree in one 64-bit half and differ in the other, so only crafted input reaches the
comparison of the low halves through the sorted indices, and only crafted input tells a sort that skipped a digit
(tests/sig_cases.py: all equal, all distinct in one half only, an 8 x 8 grid of halves, every single-bit value
twice). tests/test_sig_cases.py asserts that these inputs hold what they are meant to hold."""
import ctypes

import numpy as np
import pytest

import sig_cases as C
import sig_ref
from namazu_amd import _lib

pytestmark = pytest.mark.gpu


def _vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _dev(a, view):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(view)).cuda()
    torch.cuda.synchronize()
    return t


def _u32(t, n):
    return t.cpu().numpy().view(np.uint32)[:n].tolist()


@pytest.mark.parametrize("family,N", C.CLASS_CASES)
def test_sig_classes_on_crafted_signatures(ctx, family, N):
    import torch
    sigs = C.class_sigs(family, N)
    exp = sig_ref.first_equal(sigs)
    d_sig = _dev(np.array(sigs, np.uint64).reshape(-1), np.int64)
    fe = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().nmz_sig_classes_dev(ctx.handle, _vp(d_sig), N, _vp(fe), None))
    torch.cuda.synchronize()
    assert _u32(fe, N) == exp
    # the same signatures in reverse order: the smallest index of a class changes, its members do not
    rev = sigs[::-1]
    d_sig = _dev(np.array(rev, np.uint64).reshape(-1), np.int64)
    st = torch.cuda.Stream()
    _lib.check(_lib.load().nmz_sig_classes_dev(ctx.handle, _vp(d_sig), N, _vp(fe), ctypes.c_void_p(st.cuda_stream)))
    st.synchronize()
    assert _u32(fe, N) == sig_ref.first_equal(rev)


def _stats(sigs, gaps):
    st = np.zeros(len(sigs), _lib.DELIVERY_STATS_DTYPE)
    assert st.dtype.itemsize == 32
    st["sig_lo"] = np.array([lo for lo, _ in sigs], np.uint64)
    st["sig_hi"] = np.array([hi for _, hi in sigs], np.uint64)
    st["min_gap_ns"] = np.array(gaps, np.int64)
    st["gap_event"] = np.arange(len(sigs)) % 5
    st["n_counted"] = 3
    return st


@pytest.mark.parametrize("family,N", C.CLASS_CASES)
def test_delivery_classes_on_crafted_records(ctx, family, N):
    """first_equal, the representative (largest min_gap_ns, ties to the smallest index, NMZ_NONE off the heads) and
    the class count over crafted nmz_delivery_stats records; the forms without d_class_rep and without d_n_classes."""
    import torch
    L = _lib.load()
    sigs, gaps = C.class_sigs(family, N), C.class_gaps(family, N)
    exp_fe = sig_ref.first_equal(sigs)
    exp_rep = sig_ref.class_rep(exp_fe, gaps)
    exp_n = sig_ref.n_classes(exp_fe)
    assert [i for i, r in enumerate(exp_rep) if r != C.NONE] == [i for i, h in enumerate(exp_fe) if h == i]
    d_st = _dev(_stats(sigs, gaps).view(np.uint8), np.uint8)

    def run(with_rep, with_n, stream=None):
        fe = torch.full((N,), -1, dtype=torch.int32, device="cuda")
        rep = torch.full((N,), 12345, dtype=torch.int32, device="cuda") if with_rep else None
        nc = torch.full((1,), 77, dtype=torch.int32, device="cuda") if with_n else None
        torch.cuda.synchronize()
        s = ctypes.c_void_p(stream.cuda_stream) if stream is not None else None
        _lib.check(L.nmz_delivery_classes_dev(ctx.handle, _vp(d_st), N, _vp(fe), _vp(rep), _vp(nc), s))
        torch.cuda.synchronize()
        return _u32(fe, N), (_u32(rep, N) if with_rep else None), (_u32(nc, 1)[0] if with_n else None)

    assert run(True, True) == (exp_fe, exp_rep, exp_n)
    assert run(False, True, torch.cuda.Stream()) == (exp_fe, None, exp_n)
    assert run(True, False) == (exp_fe, exp_rep, None)
    assert run(False, False) == (exp_fe, None, None)
