"""GPU parity of the edit-distance kernels on alignments that leave the main diagonal (tests/ed_cases.py): indels at
the start (the path on diagonal +-d, up to the band edge d = w), shifts, rotations, an offset over one block,
random edits and periodic traces, on every plan kind and form. Every result is compared bit for bit with the CPU
oracle's distances (O.ed_pairs, through ed_cases.reference), with k = min(n - 1, 64) so that (up to 65 traces)
every pair distance is compared. The all-pairs kernels run each unordered pair once, the earlier trace as the
query (the rows): every store runs as built and reversed, so each pair is computed in both roles.
tests/test_ed_offdiag.py asserts, from the oracle alone, that each case holds the pairs it is here for."""
import ctypes

import numpy as np
import pytest

import ed_cases as C
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FORMS = {"single-kernel": _lib.NMZ_ED_OPT_SINGLE_KERNEL, "no-qgram": _lib.NMZ_ED_OPT_NO_QGRAM,
         "compact": _lib.NMZ_ED_OPT_COMPACT}


class _Plan:
    def __init__(self, ctx, trs, w, kind, opts=0):
        self.L = _lib.load()
        self.ctx, self.n = ctx, len(trs)
        self.off, self.sym = C.csr(trs)
        self.plan = ctypes.c_void_p()
        _lib.check(self.L.nmz_ed_plan_create_opts(ctx.handle, _lib.ptr(self.off), _lib.ptr(self.sym), None, self.n,
                                                  w, opts, ctypes.byref(self.plan)))
        try:
            assert self.L.nmz_ed_plan_is_fast(self.plan) == kind
        except BaseException:
            self.close()
            raise

    def close(self):
        if self.plan:
            self.L.nmz_ed_plan_destroy(self.plan)
            self.plan = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def search(self, k, shards=1):
        """(ids, dists) [n, k]: one search, or `shards` partial searches + merge + fill."""
        import torch
        L, n = self.L, self.n
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        out = torch.empty(n * k, dtype=torch.int64, device="cuda")
        if shards == 1:
            _lib.check(L.nmz_ed_allpairs_knn_dev(self.plan, k, ctypes.c_void_p(out.data_ptr()), stream))
        else:
            parts = torch.empty(shards * n * k, dtype=torch.int64, device="cuda")
            for s in range(shards):
                _lib.check(L.nmz_ed_allpairs_knn_shard_dev(self.plan, k, s, shards,
                                                           ctypes.c_void_p(parts.data_ptr() + s * n * k * 8), stream))
            _lib.check(L.nmz_knn_merge_dev(self.ctx.handle, ctypes.c_void_p(parts.data_ptr()), shards, n, k,
                                           ctypes.c_void_p(out.data_ptr()), stream))
            _lib.check(L.nmz_ed_knn_fill_dev(self.plan, k, ctypes.c_void_p(out.data_ptr()), stream))
        torch.cuda.synchronize()
        keys = out.cpu().numpy().view(np.uint64).reshape(n, k)
        return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), (keys >> np.uint64(32)).astype(np.uint32)


def _both_orders(ctx, name, opts=0, shards=1):
    trs, D, w = C.traces(name), C.reference(name), C.band(name)
    n = len(trs)
    k = min(n - 1, 64)
    for order in (np.arange(n), np.arange(n)[::-1]):
        with _Plan(ctx, [trs[i] for i in order], w, C.kind(name), opts) as p:
            ids, ds = p.search(k, shards)
        ri, rd = C.knn_from(D, order, k)
        bad = np.argwhere((ds != rd) | (ids != ri))
        assert len(bad) == 0, (name, "reversed" if order[0] else "as built", len(bad), "first (query, slot):",
                               bad[0].tolist(), "got", int(ids[tuple(bad[0])]), int(ds[tuple(bad[0])]),
                               "want", int(ri[tuple(bad[0])]), int(rd[tuple(bad[0])]))


@pytest.mark.parametrize("name", list(C.CASES))
def test_allpairs_offdiag(ctx, name):
    """Every family on its plan kind's default form (bit-parallel: two-phase with the q-gram bound), both store
    orders."""
    _both_orders(ctx, name)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["bv-w32", "bv-w64"])
def test_allpairs_offdiag_bitparallel_forms(ctx, name, form):
    """The other forms of the bit-parallel search, as plan options: the single kernel with its in-workgroup
    pre-filter, the same without the q-gram bound, and the compact tables."""
    _both_orders(ctx, name, opts=FORMS[form])


def test_allpairs_offdiag_sharded(ctx):
    """Three families over different bases in one store (pairs cross a 64-query block) through 3 shards, merged by
    nmz_knn_merge_dev and completed by nmz_ed_knn_fill_dev."""
    assert len(C.traces("bv-3fam")) >= 65
    _both_orders(ctx, "bv-3fam", shards=3)


@pytest.mark.parametrize("w", [0, 3, 32, 200])
def test_ed_pairs_offdiag(ctx, w):
    """nmz_ed_pairs (k_ed_generic) over all ordered pairs of the (32, 200, 12) family."""
    trs = C.traces("bv-w32")
    ts = hs.TraceSet(list(trs))
    pairs = C.all_ordered_pairs(len(trs))
    got = hs.ed_pairs(ts, pairs, w, ctx=ctx)
    want = O.ed_pairs(ts.off, ts.sym, pairs, w, nthreads=16)
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (len(bad), pairs[bad[0]].tolist(), int(got[bad[0]]), int(want[bad[0]]))


@pytest.mark.parametrize("name,plan", [("bv-w32", "bitparallel"), ("bv-w64", "bitparallel"),
                                       ("wide-w1024", "wide"), ("generic-w9000", "generic")])
def test_queries_offdiag(ctx, name, plan):
    """nmz_ed_plan_query_knn's three kernels: one half of a family stored (even indices), the other half as the
    queries, then swapped. Per query the stored traces by (distance asc, stored id asc), as the oracle's rows."""
    trs, D, w = C.traces(name), C.reference(name), C.band(name)
    n = len(trs)
    halves = (np.arange(0, n, 2), np.arange(1, n, 2))
    for st, qs in (halves, halves[::-1]):
        k = min(len(st), 64)
        idx = hs.SimilarityIndex(hs.TraceSet([trs[i] for i in st]), w, ctx=ctx)
        try:
            assert idx.kind == plan
            ids, ds = idx.query([trs[i] for i in qs], k)
        finally:
            idx.close()
        for r, q in enumerate(qs):
            d = D[q, st]
            order = np.lexsort((np.arange(len(st)), d))[:k]
            assert ds[r].tolist() == d[order].tolist(), (name, int(q))
            assert ids[r].tolist() == order.tolist(), (name, int(q))
