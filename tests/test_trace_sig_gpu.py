"""GPU: the trace signatures of k_trace_sig (csrc/unique.hip), value for value against the plain-integer
restatement tests/sig_ref.py on the probe set tests/sig_cases.py, through nmz_trace_signatures, nmz_unique_traces and
nmz_unique_traces_dev. Everything is integer: every comparison is equality.

The library does not report which form of the kernel ran. The regimes follow sig_launch's thresholds:
  bound <= SIG_MASK_ENT (1,024)                      -> MODE 2, per-entity LDS masks        (B = 1, 7, 64, 65, 1024)
  the same with NMZ_SIG_MASKS=0                      -> MODE 1, kbits = ceil(log2 B) ballots (B = 1, 7, 1024: 0, 3, 10)
  SIG_MASK_ENT < bound <= SIG_MAX_ENT_LDS (4,096)    -> MODE 1, 4 waves per workgroup        (B = 1025, 4096)
  SIG_MAX_ENT_LDS < bound <= SIG_MAX_ENT (16,384)    -> MODE 1, 1 wave per workgroup         (B = 4097, 16384: 64 KB LDS)
  entity == NULL                                     -> MODE 0, rank = position
and in every form ranks >= 65,536 take the inline keys instead of the context's table (the `one` probes past 65,536
elements and the long exact probes)."""
import ctypes

import numpy as np
import pytest

import sig_cases as C
import sig_ref
from namazu_amd import _lib

pytestmark = pytest.mark.gpu


def host_signatures(ctx, probes, po=True):
    off, sym, ent = C.csr(probes, po)
    sig = np.zeros(2 * max(len(probes), 1), np.uint64)
    _lib.check(_lib.load().nmz_trace_signatures(ctx.handle, _lib.ptr(off), _lib.ptr(sym), _lib.ptr(ent), len(probes),
                                                _lib.ptr(sig)))
    return [(lo, hi) for lo, hi in sig.reshape(-1, 2)[:len(probes)].tolist()]


def assert_same(got, probes, bound=None):
    exp = [C.reference(p, bound) for p in probes]
    bad = [(p, g, e) for p, g, e in zip(probes, got, exp) if g != e]
    assert not bad, f"{len(bad)} of {len(probes)} signatures differ, first: {bad[0]}"


@pytest.mark.parametrize("B", C.BOUNDS)
def test_host_form_po(ctx, B):
    call = C.po_call(B)
    assert C.bound_of(call) == B
    assert_same(host_signatures(ctx, call), call)


def test_host_form_exact(ctx):
    call = C.exact_call()
    assert_same(host_signatures(ctx, call, po=False), call)


@pytest.mark.parametrize("B", (1, 7, 1024))
def test_ballots_at_small_bounds(ctx, ab_knobs, monkeypatch, B):
    """NMZ_SIG_MASKS=0: the ballot form below the mask threshold, with 0, 3 and 10 ballots per step."""
    monkeypatch.setenv("NMZ_SIG_MASKS", "0")
    call = C.po_call(B)
    assert_same(host_signatures(ctx, call), call)


def _ballast(B):
    e = np.array([B - 1, 0, B - 1, B - 1], np.uint32)
    return C.Probe(f"ballast@{B}", C.pool()[[5, 41, 7, 7]], e)


def test_one_trace_every_form(ctx):
    """The same traces (ids < 7) in calls whose bound a ballast trace lifts over each threshold: their signatures do
    not depend on the form that computed them."""
    sub = [p for p in C.po_call(7) if len(p) in (0, 1, 64, 65, 257, 513, 1000, 65536, 70000)]
    assert len(sub) >= 50 and C.bound_of(sub) == 7
    seen = []
    for B in (7, 1025, 4097, 16384):
        call = sub[:10] + [_ballast(B)] + sub[10:]
        assert C.bound_of(call) == B
        got = host_signatures(ctx, call)
        assert_same(got, call)
        seen.append(got[:10] + got[11:])
    assert seen[0] == seen[1] == seen[2] == seen[3]


class Dev:
    """The arrays of a call on the device, for nmz_unique_traces_dev."""

    def __init__(self, probes, po=True):
        import torch
        self.torch, self.n = torch, len(probes)
        off, sym, ent = C.csr(probes, po)
        self.off = torch.from_numpy(off.view(np.int64)).cuda()
        self.sym = torch.from_numpy(sym.view(np.int64)).cuda()
        self.ent = torch.from_numpy(ent.view(np.int32)).cuda() if po else None
        self.sig = torch.zeros(2 * self.n, dtype=torch.int64, device="cuda")
        self.fe = torch.full((self.n,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def run(self, ctx, max_entities, stream):
        P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        _lib.check(_lib.load().nmz_unique_traces_dev(ctx.handle, P(self.off), P(self.sym), P(self.ent), self.n,
                                                     max_entities, P(self.sig), P(self.fe),
                                                     ctypes.c_void_p(stream.cuda_stream)))
        stream.synchronize()
        sig = self.sig.cpu().numpy().view(np.uint64).reshape(-1, 2).tolist()
        return [(lo, hi) for lo, hi in sig], self.fe.cpu().numpy().view(np.uint32).tolist()


def test_device_form_bound_skips_ids_past_it(ctx):
    """max_entities = 7 over probes that also carry ids 7-10: those elements are skipped like NMZ_NONE (the header's
    rule), on a stream that is not torch's default; first_equal follows the signatures."""
    import torch
    call = C.po_call(11, long=False)
    assert C.bound_of(call) == 11
    assert sum(1 for p in call if len(p) and ((p.ent >= 7) & (p.ent != C.NONE)).any()) >= 30
    st = torch.cuda.Stream()
    assert st.cuda_stream != torch.cuda.default_stream().cuda_stream and st.cuda_stream != ctx.stream()
    sig, fe = Dev(call).run(ctx, 7, st)
    assert_same(sig, call, bound=7)
    assert fe == sig_ref.first_equal([C.reference(p, 7) for p in call])
    assert [C.reference(p, 7) for p in call] != [C.reference(p) for p in call]


def test_device_form_exact(ctx):
    import torch
    call = C.exact_call()
    st = torch.cuda.Stream()
    sig, fe = Dev(call, po=False).run(ctx, 0, st)
    assert_same(sig, call)
    assert fe == sig_ref.first_equal([C.reference(p) for p in call])
    # twice the same traces: every second copy points at its first
    sig2, fe2 = Dev(call + call, po=False).run(ctx, 0, st)
    assert sig2 == sig + sig and fe2 == sig_ref.first_equal(sig + sig)
    assert sig_ref.n_classes(fe2) == sig_ref.n_classes(fe)


def test_unique_traces_first_equal_with_relabelled_copies(ctx):
    """Every probe twice, the second copy with its entity ids permuted: nmz_unique_traces gives the restatement's
    first_equal (each copy joins its original; the empty and the all-skipped traces form one class)."""
    B = 64
    first = list(C.po_call(B, long=False))
    perm = np.random.default_rng(5).permutation(B).astype(np.uint32)
    assert (perm != np.arange(B)).sum() >= B - 4
    second = [C.Probe(p.name + "'", p.sym, np.where(p.ent == C.NONE, np.uint32(C.NONE),
                                                     perm[np.minimum(p.ent, B - 1)]).astype(np.uint32))
              for p in first]
    order = np.random.default_rng(6).permutation(2 * len(first)).tolist()
    call = [(first + second)[i] for i in order]
    exp = sig_ref.first_equal([C.reference(p) for p in call])
    assert sig_ref.n_classes(exp) <= len(first) < len(call)
    off, sym, ent = C.csr(call)
    fe = np.full(len(call), 0xDEADBEEF, np.uint32)
    _lib.check(_lib.load().nmz_unique_traces(ctx.handle, _lib.ptr(off), _lib.ptr(sym), _lib.ptr(ent), len(call),
                                             _lib.ptr(fe)))
    assert fe.tolist() == exp
    assert_same(host_signatures(ctx, call), call)


def test_errors(ctx):
    L = _lib.load()
    off = np.array([0, 3], np.uint64)
    sym = np.arange(3, dtype=np.uint64)
    sig = np.zeros(2, np.uint64)
    for ids, rc in (([0, 16384, 1], _lib.NMZ_EINVAL), ([0, 16383, C.NONE], _lib.NMZ_OK)):
        ent = np.array(ids, np.uint32)
        assert L.nmz_trace_signatures(ctx.handle, _lib.ptr(off), _lib.ptr(sym), _lib.ptr(ent), 1,
                                      _lib.ptr(sig)) == rc
        if rc:
            assert "16384" in _lib.last_error()
    assert (int(sig[0]), int(sig[1])) == sig_ref.signature(sym, [0, 16383, C.NONE])
    assert L.nmz_trace_signatures(ctx.handle, None, None, None, 0, None) == _lib.NMZ_OK
    assert L.nmz_trace_signatures(ctx.handle, _lib.ptr(off), _lib.ptr(sym), None, 0, _lib.ptr(sig)) == _lib.NMZ_OK
