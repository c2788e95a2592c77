"""GPU: k_script_moves_wide (nmz_move_profile_wide, nmz_move_profile_wide_dev, nmz_ed_diff_profile_wide,
Naive.DiffFailing beyond band 64) against the host form nmz_move_profile_wide_host over nmz_ed_align_wide_host's
scripts, which tests/test_moves_wide_host.py ties to the definition value for value.

partner, every counter of every table symbol and info are compared. The shapes: the constructed rows at the first
size past one wave (k = 33) and at the full band (k = 512: every thread's four slots live, partners 512 slots apart),
the moved-block family at the bands where a thread gains a slot, narrow bands through the wide entry points, more
pairs than the grid has workgroups, a table too large for LDS, batches that accumulate, the device-pointer form on a
side stream, pairs beyond the band and beyond the plan, ops that a caller of the device form corrupted, and
Naive.DiffFailing at band 200."""
import json
import os

import numpy as np
import pytest

import moves_cases as MC
import moves_ref as MR
import moves_wide_cases as WC
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from test_moves_gpu import Dev, same
from test_moves_host import table_of
from test_moves_wide_host import check_row

pytestmark = pytest.mark.gpu

NONE = _lib.NMZ_NONE


def check(ctx, trs, pairs, w, usym=None):
    """Scripts given (nmz_move_profile_wide over nmz_ed_align_wide_pairs) and scripts made
    (nmz_ed_diff_profile_wide) against the host forms; the device routes byte for byte. Returns (the expected
    MoveProfile, the device's, the device's scripts)."""
    ts = hs.TraceSet(list(trs))
    pairs = np.asarray(pairs, np.uint32).reshape(-1, 2)
    eh = WC.host_scripts_wide(trs, pairs, w)
    want = hs.move_profile_of_wide(ts, pairs, eh, usym=usym, want_partner=True, host=True)
    es = hs.edit_scripts_wide(ts, pairs, w, ctx=ctx)
    assert np.array_equal(es.dist, eh.dist) and es.ops.tobytes() == eh.ops.tobytes()
    got = hs.move_profile_of_wide(ts, pairs, es, ctx=ctx, usym=usym, want_partner=True)
    same(got, want)
    plain = hs.move_profile_of_wide(ts, pairs, es, ctx=ctx, usym=usym)  # partner == NULL
    made = hs.move_profile_wide(ts, pairs, w, ctx=ctx, usym=usym)
    for other in (plain, made):
        assert other.counts.tobytes() == got.counts.tobytes() and other.info.tobytes() == got.info.tobytes()
        assert np.array_equal(other.symbols, got.symbols) and np.array_equal(other.dist, got.dist)
    return want, got, es


def family_pairs():
    return np.array(MC.ordered_pairs(len(WC.family())), np.uint32)


# ---- 1. the constructed rows, both roles -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [33, 512])
def test_constructed_rows(ctx, k):
    rows = WC.constructed(k)
    assert [r["name"] for r in rows] == ["rot", "rot-rev", "uneq", "xy", "rot-beyond"]
    for r in rows:
        usym, ids = table_of(set(r["a"]) | set(r["b"]))
        want, got, es = check(ctx, [MC.encode(r["a"]), MC.encode(r["b"])], [(0, 1), (1, 0)], r["band"], usym=usym)
        one = hs.move_profile_of_wide(hs.TraceSet([MC.encode(r["a"]), MC.encode(r["b"])]), [[0, 1]],
                                      hs.EditScripts(es.dist[:1], es.ops[:1], r["band"]), ctx=ctx, usym=usym,
                                      want_partner=True)
        check_row(r, es, ids, one)  # the closed forms on the device's own result
        if r["kinds"] is None:
            assert int(got.info["n_beyond"]) == 2 and (got.partner == NONE).all()
        else:
            assert int(got.info["n_scripts"]) == 2 and int(got.info["n_ops"]) == 2 * r["dist"]
    if k == 512:
        x = rows[0]["counts"][WC.X]
        assert x["later"] == 512 and x["span_later"] == 917248 and rows[0]["band"] == 1024


# ---- 2. the moved-block family ---------------------------------------------------------------------------------------
FAMILY = {}  # band -> the expected profile of the full family, default table


def family_profile(ctx, w):
    if w not in FAMILY:
        FAMILY[w] = check(ctx, WC.family_encoded(), family_pairs(), w)[0]
    return FAMILY[w]


@pytest.mark.parametrize("w", [65, 128, 256, 257, 512, 1024])
def test_family(ctx, w):
    """All 182 ordered pairs; 256 | 257 and 512 are where a thread gains a slot."""
    want = family_profile(ctx, w)
    d = want.dist
    print(w, "scripts", int(want.info["n_scripts"]), "beyond", int(want.info["n_beyond"]), "wide",
          int(((d > 64) & (d <= w)).sum()))
    assert len(d) == 182 and int(want.info["n_scripts"]) + int(want.info["n_beyond"]) == 182
    if w >= 256:
        assert int(want.info["n_scripts"]) >= 84 and ((d > 64) & (d <= w)).sum() >= 72
        assert int(want.counts["later"].sum() + want.counts["earlier"].sum()) >= 4225
    if w >= 512:
        slot = np.arange(w, dtype=np.int64)[None, :]
        far = ((want.partner != NONE) & (np.abs(want.partner.astype(np.int64) - slot) >= 256)).sum()
        assert ((d > 256) & (d <= w)).sum() >= 84 and far >= 360


# ---- 3. narrow bands through the wide entry points -------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 8, 64])
def test_narrow_bands_equal_the_narrow_entry_points(ctx, w):
    fam = MC.family(31)
    ts = hs.TraceSet([MC.encode(t) for t in fam])
    pairs = np.array(MC.ordered_pairs(len(fam)), np.uint32)
    es = hs.edit_scripts(ts, pairs, w, ctx=ctx)
    narrow = hs.move_profile_of(ts, pairs, es, ctx=ctx, want_partner=True)
    wide = hs.move_profile_of_wide(ts, pairs, es, ctx=ctx, want_partner=True)
    made_n, made_w = hs.move_profile(ts, pairs, w, ctx=ctx), hs.move_profile_wide(ts, pairs, w, ctx=ctx)
    assert wide.partner.shape == (len(pairs), w) and wide.partner.tobytes() == narrow.partner.tobytes()
    for a, b in ((wide, narrow), (made_w, made_n), (made_w, narrow)):
        assert a.counts.tobytes() == b.counts.tobytes() and a.info.tobytes() == b.info.tobytes()
        assert a.dist.tobytes() == b.dist.tobytes()
    assert int(narrow.info["n_scripts"]) >= (100 if w else 30) and int(narrow.info["n_beyond"]) >= 100


# ---- 4. more pairs than workgroups -----------------------------------------------------------------------------------
def test_more_pairs_than_workgroups(ctx):
    w = 256
    rng = np.random.default_rng(9)
    pairs = family_pairs()[rng.integers(0, 182, size=4000)]
    pairs[::97, 1] = pairs[::97, 0]  # (i, i)
    want, _, _ = check(ctx, WC.family_encoded(), pairs, w)
    d = want.dist
    assert ((d > 64) & (d <= w)).sum() >= 1000 and (d > w).sum() >= 1000 and (d == 0).sum() >= 40
    assert len({tuple(p) for p in pairs.tolist()}) < 300  # duplicates


# ---- 5. a table larger than MV_LDS_SYMS ----------------------------------------------------------------------------
def test_table_in_global_memory(ctx):
    w = 512
    trs = WC.family_encoded()
    full = family_profile(ctx, w)
    rng = np.random.default_rng(5)
    unused = np.setdiff1d(rng.integers(0, 2**63, size=3000).astype(np.uint64), full.symbols)
    usym = np.union1d(full.symbols, unused)
    assert len(usym) > 2048 + 40 and np.all(usym[1:] > usym[:-1])
    big, _, _ = check(ctx, trs, family_pairs(), w, usym=usym)
    shared = np.isin(usym, full.symbols)
    assert big.counts[shared].tobytes() == full.counts.tobytes() and not big.counts[~shared].view(np.uint32).any()
    assert big.info == full.info and np.array_equal(big.partner, full.partner)
    gone = full.symbols[int(np.argmax(full.counts["n_pairs"]))]
    less, _, _ = check(ctx, trs, family_pairs(), w, usym=usym[usym != gone])
    assert int(less.info["n_unknown"]) > 0 and np.array_equal(less.partner, full.partner)
    assert less.counts.tobytes() == big.counts[usym != gone].tobytes()
    none, _, _ = check(ctx, trs, family_pairs(), w, usym=np.zeros(0, np.uint64))
    assert len(none.counts) == 0 and int(none.info["n_unknown"]) > int(less.info["n_unknown"])
    assert np.array_equal(none.partner, full.partner)


# ---- 6. the device-pointer form --------------------------------------------------------------------------------------
class DevWide(Dev):
    """test_moves_gpu's Dev over the wide entry points: the scripts are always given."""

    def run(self, lo, hi, accumulate, stream=None, partner=True):
        w = self.w
        _lib.check(_lib.load().nmz_move_profile_wide_dev(
            self.ctx.handle, self.d_off.data_ptr(), self.d_sym.data_ptr(), self.d_pairs.data_ptr() + 8 * lo, hi - lo, w,
            self.d_dist.data_ptr() + 4 * lo, self.d_ops.data_ptr() + 12 * w * lo, self.d_usym.data_ptr(),
            len(self.usym), self.d_partner.data_ptr() + 4 * w * lo if partner else None, self.d_counts.data_ptr(),
            self.d_info.data_ptr(), accumulate, stream))

    def expected(self):
        return hs.move_profile_of_wide(self.ts, self.pairs, hs.EditScripts(self.dist, self.ops, self.w),
                                       usym=self.usym, want_partner=True, host=True)


def family_dev(ctx, w):
    trs = WC.family_encoded()
    es = WC.host_scripts_wide(trs, family_pairs(), w)
    return DevWide(ctx, trs, family_pairs(), w, dist=es.dist, ops=es.ops)


def test_batches_accumulate(ctx):
    dev = family_dev(ctx, 512)
    want = dev.expected()
    P, cut = len(dev.pairs), 77
    dev.d_counts.fill_(7)  # accumulate == 0 clears a dirty buffer
    dev.d_info.fill_(7)
    dev.torch.cuda.synchronize()
    dev.run(0, P, 0)
    same(dev.result(), want)
    dev.run(0, cut, 0)
    dev.run(cut, P, 1)
    same(dev.result(), want)
    dev.run(0, 0, 1)  # no pairs: nothing is added ...
    same(dev.result(), want)
    dev.run(0, 0, 0)  # ... and accumulate == 0 still clears
    cleared = dev.result()
    assert not cleared.counts.view(np.uint32).any() and not np.frombuffer(cleared.info.tobytes(), np.uint32).any()


def test_dev_form_on_a_side_stream(ctx):
    dev = family_dev(ctx, 257)
    want = dev.expected()
    side = dev.torch.cuda.Stream()
    dev.run(0, len(dev.pairs), 0, stream=side.cuda_stream, partner=False)
    side.synchronize()
    got = dev.result(stream=side)
    assert (got.partner == 7).all()  # d_partner == NULL: nothing is written
    got.partner = None
    same(got, want)


# ---- 7. beyond the band and beyond the plan --------------------------------------------------------------------------
def test_beyond_the_band_and_beyond_the_plan(ctx):
    """dist == NMZ_NONE (a plan whose max_len is too short for the traces of 613 and 620 elements) and dist == band
    + 1 are n_beyond, with NMZ_NONE partners. Every pair of the family has a trace beyond max_len = 600, so the
    plan's output fills the even pairs and the host aligner's scripts the odd ones."""
    w = 256
    fam = WC.family()
    dev = family_dev(ctx, w)
    P = len(dev.pairs)
    d_dist = dev.torch.zeros(P, dtype=dev.torch.int32, device="cuda")
    d_ops = dev.torch.zeros(P * w * 3, dtype=dev.torch.int32, device="cuda")
    dev.torch.cuda.synchronize()
    plan = hs.AlignWidePlan(w, 600, ctx=ctx)
    try:
        plan.pairs_dev(dev.d_off.data_ptr(), dev.d_sym.data_ptr(), dev.d_pairs.data_ptr(), P, d_dist.data_ptr(),
                       d_ops.data_ptr())
        dev.torch.cuda.synchronize()
    finally:
        plan.close()
    dist = d_dist.cpu().numpy().view(np.uint32).copy()
    ops = d_ops.cpu().numpy().view(_lib.EDIT_OP_DTYPE).reshape(P, w).copy()
    long_pair = np.array([max(len(fam[i]), len(fam[j])) > 600 for i, j in dev.pairs.tolist()])
    has_620 = np.array([max(len(fam[i]), len(fam[j])) == 620 for i, j in dev.pairs.tolist()])
    assert has_620.sum() >= 100 and (dist[has_620] == NONE).all() and (dist[long_pair] == NONE).all()
    assert (ops.view(np.uint32)[long_pair] == NONE).all()
    odd = np.arange(P) % 2 == 1
    dist[odd], ops[odd] = dev.dist[odd], dev.ops[odd]
    assert (dist == NONE).sum() >= 80 and (dist == w + 1).sum() >= 40 and ((dist > 64) & (dist <= w)).sum() >= 30
    mixed = DevWide(ctx, WC.family_encoded(), dev.pairs, w, dist=dist, ops=ops)
    mixed.run(0, P, 0)
    got = mixed.result()
    same(got, mixed.expected())
    assert int(got.info["n_beyond"]) == int((dist > w).sum()) and (got.partner[dist > w] == NONE).all()
    assert int(got.info["n_scripts"]) == int((dist <= w).sum()) >= 30


# ---- 8. corrupted ops, through the device form only ----------------------------------------------------------------
def test_corrupted_ops_count_for_nothing(ctx):
    """kind = 7 at slot 0, a_pos at its trace's end on the DEL of slot 300, b_pos at its trace's end on the INS of
    slot 900 of the k = 512 rotation: the op names nothing and pairs with nothing, the other ops of the script pair
    up as if it were not there, and nothing is read out of range."""
    r = WC.constructed(512)[0]
    a, b, w, d = r["a"], r["b"], r["band"], r["dist"]
    es = WC.host_scripts_wide([MC.encode(a), MC.encode(b)], [(0, 1)], w)
    good = [(int(o["a_pos"]), int(o["b_pos"]), int(o["kind"])) for o in es.ops[0]]
    picks = [(0, "kind", MR.DEL), (300, "a_pos", MR.DEL), (900, "b_pos", MR.INS)]
    ops = np.repeat(es.ops, len(picks), axis=0)
    table = set(a) | set(b)
    counts, info = {}, {"n_scripts": 0, "n_beyond": 0, "n_ops": 0, "n_unknown": 0}
    partner = np.full((len(picks), w), NONE, np.uint32)
    for p, (bad, how, kind) in enumerate(picks):
        assert good[bad][2] == kind
        ops[p, bad][how] = {"kind": 7, "a_pos": len(a), "b_pos": len(b)}[how]
        info["n_scripts"] += 1
        info["n_ops"] += d
        keep = [s for s in range(d) if s != bad]
        pr = MR.tally(a, b, [good[s] for s in keep], table, counts, info)
        for k, s in enumerate(keep):
            if pr[k] is not None:
                partner[p, s] = keep[pr[k]]
    assert (partner != NONE).sum() == 2 * 511 * len(picks)  # each script lost one move
    usym, order = table_of(table)
    dev = DevWide(ctx, [MC.encode(a), MC.encode(b)], [(0, 1)] * len(picks), w, usym=usym,
                  dist=np.full(len(picks), d, np.uint32), ops=ops)
    dev.run(0, len(picks), 0)
    got = dev.result()
    assert np.array_equal(got.partner, partner)
    assert {f: int(got.info[f]) for f in info} == info
    for u, v in enumerate(order):
        assert {f: int(got.counts[u][f]) for f in MR.FIELDS} == counts.get(v, MR.empty_counts()), v
    x = order.index(WC.X)
    assert int(got.counts[x]["dropped"]) + int(got.counts[x]["extra"]) == len(picks)
    assert int(got.counts[x]["later"]) == 511 * len(picks)
    with pytest.raises(_lib.NmzInvalidArgument, match="pair 0, slot 0"):
        dev.expected()


# ---- 9. Naive.DiffFailing beyond band 64 -----------------------------------------------------------------------------
def test_diff_failing_at_band_200(ctx, golden, tmp_path):
    """The store of test_diff_similar_at_band_200: the zk runs plus two runs made far from run 0 (ids 6 and 7). Runs
    0 and 2 fail; their passing neighbours include 6 and 7, more than 64 edits from run 0."""
    from test_visualize import write_store, zk_store_traces
    tr = zk_store_traces(golden)
    (a0, e0), (a1, e1), (a2, e2), (a3, e3) = tr[:4]
    tr.append((a1 + a2 + a3 + a0, e1 + e2 + e3 + e0))
    tr.append((a0 + a1 + a2, e0 + e1 + e2))
    write_store(str(tmp_path), tr)
    labels = {i: i not in (0, 2) for i in range(len(tr))}
    assert len(tr) == 8
    for i, ok in labels.items():
        with open(os.path.join(str(tmp_path), "%08x" % i, "result.json"), "w") as f:
            json.dump({"successful": ok, "required_time": 1}, f)
    st = hs.LoadStorage(str(tmp_path))
    runs = st.traces()
    trs = [r.symbols for r in runs]
    band, k = 200, 8
    prof = st.DiffFailing(band, k=k, ctx=ctx)
    passing, failing = [i for i, ok in labels.items() if ok], [i for i, ok in labels.items() if not ok]
    want_pairs = []
    for f in failing:
        near = sorted((WC.wide_slots(trs[j], trs[f], band)[0], j) for j in passing)[:k]
        want_pairs += [(j, f) for d, j in near if d <= band]
    assert prof.pairs.tolist() == [list(p) for p in want_pairs]
    assert (6, 0) in want_pairs and (7, 0) in want_pairs
    eh = WC.host_scripts_wide(trs, want_pairs, band)
    usym = np.unique(np.concatenate(trs))
    want = hs.move_profile_of_wide(hs.TraceSet(trs), np.array(want_pairs, np.uint32), eh, usym=usym, host=True)
    same(prof, want)
    assert ((eh.dist > 64) & (eh.dist <= band)).sum() >= 2 and int(prof.info["n_beyond"]) == 0
    assert np.array_equal(prof.symbols, usym) and int(prof.info["n_ops"]) == int(eh.dist.sum()) > 100
