"""GPU: k_script_moves (nmz_move_profile, nmz_move_profile_dev, nmz_ed_diff_profile, Naive.DiffFailing) against the
host form nmz_move_profile_host over nmz_ed_align_host's scripts, which tests/test_moves_host.py ties to the
definition value for value.

partner, every counter of every table symbol and info are compared. The shapes: the known answers in both roles
(rotations that partner the last lane of a full band with a lane 32 away), the random family at the bands where the
alignment changes its layout, more pairs than the grid has waves, the table with a symbol missing, batches that
accumulate, the device-pointer form on a side stream, pairs beyond the band and beyond the plan, and ops that a
caller of the device form corrupted."""
import json
import os

import numpy as np
import pytest

import align_ref as AR
import ed_cases as EC
import moves_cases as MC
import moves_ref as MR
from namazu_amd import _lib
from namazu_amd import historystorage as hs

pytestmark = pytest.mark.gpu

NONE = _lib.NMZ_NONE


def same(got, want):
    assert got.counts.tobytes() == want.counts.tobytes(), \
        [(int(got.symbols[u]), got.counts[u], want.counts[u]) for u in np.nonzero(got.counts != want.counts)[0][:4]]
    assert got.info == want.info, (got.info, want.info)
    assert np.array_equal(got.dist, want.dist)
    if want.partner is not None and got.partner is not None:
        bad = np.nonzero((got.partner != want.partner).any(axis=1))[0] if want.partner.shape[1] else []
        assert len(bad) == 0, (bad[:10], got.partner[bad[0]], want.partner[bad[0]])


def check(ctx, trs, pairs, w, usym=None):
    """Scripts given (nmz_move_profile over nmz_ed_align_pairs) and scripts made (nmz_ed_diff_profile) against the
    host forms; the two device routes byte for byte. Returns the expected MoveProfile."""
    ts = hs.TraceSet(list(trs))
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    eh = MC.host_scripts(trs, pairs, w)
    want = hs.move_profile_of(ts, pairs, eh, usym=usym, want_partner=True, host=True)
    es = hs.edit_scripts(ts, pairs, w, ctx=ctx)
    assert np.array_equal(es.dist, eh.dist) and es.ops.tobytes() == eh.ops.tobytes()
    got = hs.move_profile_of(ts, pairs, es, ctx=ctx, usym=usym, want_partner=True)
    same(got, want)
    plain = hs.move_profile_of(ts, pairs, es, ctx=ctx, usym=usym)  # partner == NULL
    made = hs.move_profile(ts, pairs, w, ctx=ctx, usym=usym)
    for other in (plain, made):
        assert other.counts.tobytes() == got.counts.tobytes() and other.info.tobytes() == got.info.tobytes()
        assert np.array_equal(other.symbols, got.symbols) and np.array_equal(other.dist, got.dist)
    return want


# ---- 1. the known answers, both roles ---------------------------------------------------------------------------------
def test_known_answers(ctx, golden):
    kat = golden("move_profile_kat.json")
    trs = [MC.encode(t) for c in kat for t in (c["a"], c["b"])]
    for w in sorted({c["band"] for c in kat}):
        at = [k for k, c in enumerate(kat) if c["band"] == w]
        pairs = [(2 * k, 2 * k + 1) for k in at] + [(2 * k + 1, 2 * k) for k in at]
        want = check(ctx, trs, pairs, w)
        for p, k in enumerate(at):  # the fixture itself, role (a, b)
            c = kat[k]
            assert int(want.dist[p]) == c["dist"]
            if c["partner"] is not None:
                assert [None if q == NONE else int(q) for q in want.partner[p, :c["dist"]]] == c["partner"]
    by = {c["name"]: c for c in kat}
    assert by["rot32-w64"]["partner"][63] == 31 and by["xy16-w64"]["partner"][0] == 48


# ---- 2. the random family ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 8, 31, 32, 63, 64])
def test_random_family(ctx, w):
    fam = MC.family(w)
    want = check(ctx, [MC.encode(t) for t in fam], MC.ordered_pairs(len(fam)), w)
    assert int(want.info["n_scripts"]) >= 100 and int(want.info["n_beyond"]) >= 100
    if w >= 8:
        assert want.counts["later"].sum() >= 15 and want.counts["earlier"].sum() >= 15


def test_table_without_one_symbol(ctx):
    w = 63
    fam = MC.family(w)
    trs = [MC.encode(t) for t in fam]
    pairs = MC.ordered_pairs(len(fam))
    full = check(ctx, trs, pairs, w)
    gone = int(np.argmax(full.counts["n_pairs"]))
    want = check(ctx, trs, pairs, w, usym=np.delete(full.symbols, gone))
    assert int(want.info["n_unknown"]) > 0 and np.array_equal(want.partner, full.partner)
    assert want.counts.tobytes() == np.delete(full.counts, gone).tobytes()
    none = check(ctx, trs, pairs, w, usym=np.zeros(0, np.uint64))
    assert len(none.counts) == 0 and int(none.info["n_unknown"]) > int(want.info["n_unknown"])


# ---- 3. more pairs than the grid has waves ---------------------------------------------------------------------------
def test_more_pairs_than_waves(ctx):
    trs, w = EC.traces("bv-w8"), 8
    rng = np.random.default_rng(8)
    pairs = rng.integers(0, len(trs), size=(20000, 2)).astype(np.uint32)
    pairs[::97, 1] = pairs[::97, 0]  # (i, i)
    pairs[1::2] = pairs[0:-1:2][rng.permutation(10000)]  # duplicates
    want = check(ctx, trs, pairs, w)
    assert int(want.info["n_scripts"]) >= 2000 and int(want.info["n_ops"]) >= 4000
    assert want.counts["later"].sum() + want.counts["earlier"].sum() >= 100


# ---- 4. the device-pointer form ----------------------------------------------------------------------------------------
class Dev:
    """A store, pairs and scripts on the device (torch tensors), and nmz_move_profile_dev over slices of them."""

    def __init__(self, ctx, trs, pairs, w, usym=None, dist=None, ops=None):
        import torch
        self.torch, self.ctx, self.w = torch, ctx, w
        self.ts = hs.TraceSet(list(trs))
        self.pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        if dist is None:
            es = MC.host_scripts(trs, self.pairs, w)
            dist, ops = es.dist, es.ops
        self.dist, self.ops = dist, ops
        self.usym = np.unique(self.ts.sym[:int(self.ts.off[-1])]) if usym is None else usym
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).cuda()  # noqa: E731
        self.d_off, self.d_sym = up(self.ts.off, np.int64), up(self.ts.sym, np.int64)
        self.d_pairs, self.d_dist = up(self.pairs.reshape(-1), np.int32), up(dist, np.int32)
        self.d_ops = up(ops.reshape(-1).view(np.uint32), np.int32)
        self.d_usym = up(self.usym, np.int64)
        self.d_counts = torch.zeros(max(len(self.usym), 1) * 12, dtype=torch.int32, device="cuda")
        self.d_info = torch.zeros(8, dtype=torch.int32, device="cuda")
        self.d_partner = torch.full((max(len(self.pairs) * w, 1),), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()

    def run(self, lo, hi, accumulate, stream=None, partner=True):
        w = self.w
        _lib.check(_lib.load().nmz_move_profile_dev(
            self.ctx.handle, self.d_off.data_ptr(), self.d_sym.data_ptr(), self.d_pairs.data_ptr() + 8 * lo, hi - lo, w,
            self.d_dist.data_ptr() + 4 * lo, self.d_ops.data_ptr() + 12 * w * lo, self.d_usym.data_ptr(),
            len(self.usym), self.d_partner.data_ptr() + 4 * w * lo if partner else None, self.d_counts.data_ptr(),
            self.d_info.data_ptr(), accumulate, stream))

    def result(self, stream=None):
        """Drain `stream` (None: the context's), then the buffers as a MoveProfile."""
        if stream is None:
            self.torch.cuda.synchronize()  # a device-wide wait covers the context's own stream
        counts = self.d_counts.cpu().numpy().view(_lib.MOVE_COUNTS_DTYPE)[:len(self.usym)]
        info = self.d_info.cpu().numpy().view(_lib.MOVE_INFO_DTYPE)[0]
        P = len(self.pairs)
        partner = self.d_partner.cpu().numpy().view(np.uint32)[:P * self.w].reshape(P, self.w)
        return hs.MoveProfile(self.usym, counts, info, self.dist, partner)

    def expected(self):
        return hs.move_profile_of(self.ts, self.pairs, hs.EditScripts(self.dist, self.ops, self.w), usym=self.usym,
                                  want_partner=True, host=True)


def test_batches_accumulate(ctx):
    w = 31
    fam = MC.family(w)
    dev = Dev(ctx, [MC.encode(t) for t in fam], MC.ordered_pairs(len(fam)), w)
    want = dev.expected()
    P, half = len(dev.pairs), 433
    dev.d_counts.fill_(7)  # accumulate == 0 clears a dirty buffer
    dev.d_info.fill_(7)
    dev.torch.cuda.synchronize()
    dev.run(0, P, 0)
    whole = dev.result()
    same(whole, want)
    dev.run(0, half, 0)
    dev.run(half, P, 1)
    same(dev.result(), want)
    dev.run(0, 0, 1)  # no pairs: nothing is added ...
    same(dev.result(), want)
    dev.run(0, 0, 0)  # ... and accumulate == 0 still clears
    cleared = dev.result()
    assert not cleared.counts.view(np.uint32).any() and not np.frombuffer(cleared.info.tobytes(), np.uint32).any()


def test_dev_form_on_a_side_stream(ctx):
    w = 64
    fam = MC.family(w)
    dev = Dev(ctx, [MC.encode(t) for t in fam], MC.ordered_pairs(len(fam)), w)
    want = dev.expected()
    side = dev.torch.cuda.Stream()
    dev.run(0, len(dev.pairs), 0, stream=side.cuda_stream, partner=False)
    side.synchronize()
    got = dev.result(stream=side)
    assert (got.partner == 7).all()  # d_partner == NULL: nothing is written
    got.partner = None
    same(got, want)


def test_beyond_the_band_and_beyond_the_plan(ctx):
    """dist == band + 1 and dist == NMZ_NONE (a plan whose max_len is too short) are n_beyond, with NMZ_NONE
    partners."""
    w = 31
    fam = MC.family(w)
    trs = [MC.encode(t) for t in fam]
    dev = Dev(ctx, trs, MC.ordered_pairs(len(fam)), w)
    P = len(dev.pairs)
    d_dist = dev.torch.zeros(P, dtype=dev.torch.int32, device="cuda")
    d_ops = dev.torch.zeros(P * w * 3, dtype=dev.torch.int32, device="cuda")
    dev.torch.cuda.synchronize()
    plan = hs.AlignPlan(w, 70, ctx=ctx)  # the traces of 129 and 130 elements do not fit
    try:
        plan.pairs_dev(dev.d_off.data_ptr(), dev.d_sym.data_ptr(), dev.d_pairs.data_ptr(), P, d_dist.data_ptr(),
                       d_ops.data_ptr())
        dev.torch.cuda.synchronize()
    finally:
        plan.close()
    dist = d_dist.cpu().numpy().view(np.uint32)
    long_pair = np.array([max(len(fam[i]), len(fam[j])) > 70 for i, j in dev.pairs.tolist()])
    assert long_pair.sum() >= 100 and (dist[long_pair] == NONE).all()
    assert (dist[~long_pair] == dev.dist[~long_pair]).all()
    assert ((dist == w + 1) & ~long_pair).sum() >= 100
    dev.dist, dev.d_dist, dev.d_ops = dist, d_dist, d_ops
    dev.ops = d_ops.cpu().numpy().view(_lib.EDIT_OP_DTYPE).reshape(P, w)
    dev.run(0, P, 0)
    got = dev.result()
    same(got, dev.expected())
    assert int(got.info["n_beyond"]) == int((dist > w).sum()) and (got.partner[dist > w] == NONE).all()
    assert int(got.info["n_scripts"]) == int((dist <= w).sum()) >= 100


def test_corrupted_ops_count_for_nothing(ctx, golden):
    """kind = 7 or a position at its trace's end, through the device form (the host forms refuse them): the op names
    nothing and pairs with nothing, the other ops of the script pair up as if it were not there, and nothing is
    read out of range."""
    by = {c["name"]: c for c in golden("move_profile_kat.json")}
    picks = [("rot16-w32", 0, "kind"), ("rot16-w32", 20, "b_pos"), ("rot16-w32-rev", 31, "a_pos"),
             ("rot16-w32", 5, "a_pos")]
    w = 32
    ids, pairs, dist, ops = [], [], [], np.zeros((len(picks), w), _lib.EDIT_OP_DTYPE)
    counts, info = {}, {"n_scripts": 0, "n_beyond": 0, "n_ops": 0, "n_unknown": 0}
    partner = np.full((len(picks), w), NONE, np.uint32)
    table = set()
    for p, (name, bad, how) in enumerate(picks):
        c = by[name]
        a, b, d = c["a"], c["b"], c["dist"]
        table |= set(a) | set(b)
        ids += [a, b]
        pairs.append((2 * p, 2 * p + 1))
        dist.append(d)
        ops[p] = (NONE, NONE, NONE)
        ops[p, :d] = [tuple(o) for o in c["ops"]]
        assert {"kind": True, "a_pos": c["ops"][bad][2] == AR.DEL, "b_pos": c["ops"][bad][2] == AR.INS}[how]
        ops[p, bad][how] = {"kind": 7, "a_pos": len(a), "b_pos": len(b)}[how]
        info["n_scripts"] += 1
        info["n_ops"] += d
    for p, (name, bad, how) in enumerate(picks):
        c = by[name]
        keep = [s for s in range(c["dist"]) if s != bad]
        pr = MR.tally(c["a"], c["b"], [tuple(c["ops"][s]) for s in keep], table, counts, info)
        for k, s in enumerate(keep):
            if pr[k] is not None:
                partner[p, s] = keep[pr[k]]
    assert (partner != NONE).sum() == 2 * 15 * len(picks)  # each script lost one move
    order = sorted(table, key=MC.encode_one)
    usym = np.array([MC.encode_one(v) for v in order], np.uint64)
    dev = Dev(ctx, [MC.encode(t) for t in ids], pairs, w, usym=usym, dist=np.array(dist, np.uint32), ops=ops)
    dev.run(0, len(pairs), 0)
    got = dev.result()
    assert np.array_equal(got.partner, partner)
    assert {f: int(got.info[f]) for f in info} == info
    for u, v in enumerate(order):
        assert {f: int(got.counts[u][f]) for f in MR.FIELDS} == counts.get(v, MR.empty_counts()), v
    x = order.index(1000)
    assert int(got.counts[x]["dropped"]) + int(got.counts[x]["extra"]) == len(picks)
    with pytest.raises(_lib.NmzInvalidArgument, match="pair 0, slot 0"):
        dev.expected()


# ---- 5. Naive.DiffFailing ----------------------------------------------------------------------------------------------
def test_diff_failing_on_the_zk_store(ctx, golden, tmp_path):
    """Failing runs against their nearest passing runs on the ZooKeeper store, equal to the restatement: labels from
    IsSuccessful, a run without a readable result skipped, neighbours by (distance, id) from the host distances."""
    from test_visualize import write_store, zk_store_traces
    write_store(str(tmp_path), zk_store_traces(golden))
    labels = {0: True, 1: True, 2: False, 3: False, 5: True}  # run 4 has no result.json
    for i, ok in labels.items():
        with open(os.path.join(str(tmp_path), "%08x" % i, "result.json"), "w") as f:
            json.dump({"successful": ok, "required_time": 1}, f)
    st = hs.LoadStorage(str(tmp_path))
    runs = st.traces()
    band, k = 40, 2
    prof = st.DiffFailing(band, k=k, ctx=ctx)
    passing, failing = [i for i, ok in labels.items() if ok], [i for i, ok in labels.items() if not ok]
    want_pairs = []
    for f in failing:
        near = sorted((hs.edit_script_host(runs[j].symbols, runs[f].symbols, band)[0], j) for j in passing)[:k]
        want_pairs += [(j, f) for d, j in near if d <= band]
    assert prof.pairs.tolist() == [list(p) for p in want_pairs] and len(want_pairs) == 4
    trs = [r.symbols for r in runs]
    eh = MC.host_scripts(trs, want_pairs, band)
    usym = np.unique(np.concatenate([trs[i] for i in passing + failing]))
    want = hs.move_profile_of(hs.TraceSet(trs), np.array(want_pairs, np.uint32), eh, usym=usym, host=True)
    same(prof, want)
    assert np.array_equal(prof.symbols, usym) and int(prof.info["n_ops"]) == int(eh.dist.sum()) > 100
    top = prof.top(5)
    assert len(top) == 5 and top[0][1]["n_pairs"] == prof.counts["n_pairs"].max() > 0
    key = [(-int(c["n_pairs"]), -int(c["later"]) - int(c["earlier"]), s) for s, c in top]
    assert key == sorted(key)
    for ok in (True, False):  # one label only: the contrast's wording
        for i in labels:
            with open(os.path.join(str(tmp_path), "%08x" % i, "result.json"), "w") as f:
                json.dump({"successful": ok, "required_time": 1}, f)
        with pytest.raises(ValueError, match="no failing run" if ok else "no passing run"):
            st.DiffFailing(band, k=k, ctx=ctx)
