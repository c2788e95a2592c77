"""GPU: edit scripts and move profiles per entity (k_po_project, k_po_subpairs, k_po_gather over the aligners; the
nmz_po_project*, nmz_ed_align_po_* and nmz_ed_diff_profile_po entry points; Naive.DiffSimilar / DiffFailing with
po=True) against numpy for the projection and against the host form nmz_ed_align_po_host for the scripts, which
tests/test_align_po_host.py ties to the definition.

Every slot of every pair is compared. The shapes are the smallest at which these kernels can still go wrong: trace
lengths around the 64-element chunks, one id, two ids, the two ends of the id range, no id at all, more traces than
the grid holds at once, the bands on both sides of the aligners' joint at 64 / 65, several batches of sub-pairs, one
plan on a side stream twice."""
import json
import os

import numpy as np
import pytest

import align_ref as AR
import ed_cases as EC
from namazu_amd import _lib
from namazu_amd import historystorage as hs
from test_align_po_host import expected, gpu_family, interleavings, po_slots, rot
from test_align_wide_gpu import check

pytestmark = pytest.mark.gpu

NONE = _lib.NMZ_NONE


def family_store(name):
    trs, ents, G = gpu_family(name)
    return hs.TraceSet(list(trs)), np.concatenate(ents), G


# ---- 1. the projection against numpy ---------------------------------------------------------------------------------
def numpy_projection(ts, ent, G):
    poff, psym, psrc = [0], [], []
    for t in range(len(ts)):
        lo, hi = int(ts.off[t]), int(ts.off[t + 1])
        e = ent[lo:hi]
        for g in range(G):
            idx = np.nonzero(e == g)[0]
            psym.append(ts.sym[lo:hi][idx])
            psrc.append(idx.astype(np.uint32))
            poff.append(poff[-1] + len(idx))
    return (np.array(poff, np.uint64), np.concatenate(psym) if psym else np.zeros(0, np.uint64),
            np.concatenate(psrc) if psrc else np.zeros(0, np.uint32))


def check_projection(ctx, ts, ent, G):
    want = numpy_projection(ts, ent, G)
    got = hs.po_project(ts, ent, n_entities=G, ctx=ctx)
    assert np.array_equal(got.poff, want[0])
    assert np.array_equal(got.psym, want[1]) and np.array_equal(got.psrc, want[2])
    return got


@pytest.mark.parametrize("pattern", ["one", "two", "ends", "none", "random"])
def test_projection_lengths_around_the_chunks(ctx, pattern):
    rng = np.random.default_rng(7)
    lens = [0, 1, 63, 64, 65, 127, 128, 129, 4097]
    ts = hs.TraceSet([rng.integers(0, 2**63, size=L).astype(np.uint64) for L in lens])
    N = int(ts.off[-1])
    if pattern == "one":
        ent, G = np.zeros(N, np.uint32), 1
    elif pattern == "two":
        ent, G = (np.arange(N) % 2).astype(np.uint32), 2
    elif pattern == "ends":
        ent, G = np.where(rng.integers(0, 2, size=N) == 1, 1023, 0).astype(np.uint32), 1024
    elif pattern == "none":
        ent, G = np.full(N, NONE, np.uint32), 3
    else:
        ent, G = rng.integers(0, 7, size=N).astype(np.uint32), 7
        ent[rng.random(N) < 0.2] = NONE
    got = check_projection(ctx, ts, ent, G)
    assert len(got.psym) == int((ent != NONE).sum())
    if pattern == "one":
        assert np.array_equal(got.psym, ts.sym[:N]) and got.trace(8, 0)[1].tolist() == list(range(4097))


def test_projection_more_traces_than_the_grid(ctx):
    rng = np.random.default_rng(8)
    ts = hs.TraceSet([rng.integers(0, 2**63, size=int(L)).astype(np.uint64) for L in rng.integers(0, 6, size=3000)])
    N = int(ts.off[-1])
    ent = rng.integers(0, 7, size=N).astype(np.uint32)
    ent[rng.random(N) < 0.2] = NONE
    check_projection(ctx, ts, ent, 7)


# ---- 2. the scripts, every slot of every pair ---------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 64, 65, 128, 1024])
@pytest.mark.parametrize("name", ["mod2", "sparse"])
def test_family(ctx, name, w):
    """All ordered pairs of tests/test_align_wide_gpu.py's family under both entity maps, at the narrow aligner's
    last band, the wide aligner's first, and the widest (sparse at 1,024: batches of about 560 pairs)."""
    ts, ent, G = family_store(name)
    pairs = EC.all_ordered_pairs(len(ts))
    dist, ops = expected(name, pairs, w)
    print(name, w, "within", int((dist <= w).sum()), "beyond", int((dist > w).sum()))
    assert (dist <= w).sum() >= 16 and (dist > w).sum() >= 16
    check(hs.edit_scripts_po(ts, ent, pairs, w, n_entities=G, ctx=ctx), dist, ops)


# ---- 3. one entity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [8, 65])
def test_one_entity_equals_the_wide_entry_point(ctx, w):
    ts, _, _ = family_store("mod2")
    pairs = EC.all_ordered_pairs(len(ts))
    wide = hs.edit_scripts_wide(ts, pairs, w, ctx=ctx)
    es = hs.edit_scripts_po(ts, np.zeros(int(ts.off[-1]), np.uint32), pairs, w, n_entities=1, ctx=ctx)
    assert es.dist.tobytes() == wide.dist.tobytes() and es.ops.tobytes() == wide.ops.tobytes()
    assert (es.dist <= w).sum() >= 16 and (es.dist > w).sum() >= 16


# ---- 4. PO-equal interleavings ---------------------------------------------------------------------------------------
def test_interleavings_are_equal_in_po(ctx):
    w = 128
    trs = interleavings(np.random.default_rng(40), 32, 8, lens=(40, 64, 70))
    singles = [hs.SingleTrace(s, entities=["e%d" % g for g in e]) for s, e in trs]
    fe = hs.first_equal(singles, po_reduction=True, ctx=ctx)
    ts, ent, names = hs.po_entities(singles)
    assert names == ["e0", "e1", "e2"] and np.array_equal(ent, np.concatenate([e for _, e in trs]))
    pairs = EC.all_ordered_pairs(len(trs))
    es = hs.edit_scripts_po(ts, ent, pairs, w, ctx=ctx)
    exact = hs.edit_scripts_wide(ts, pairs, w, ctx=ctx)
    same = fe[pairs[:, 0]] == fe[pairs[:, 1]]
    assert np.array_equal(es.dist == 0, same)
    off_diag = same & (pairs[:, 0] != pairs[:, 1])
    assert off_diag.sum() >= 32 * 31 and (~same).sum() >= 8 * 32
    assert (es.ops[same]["kind"] == NONE).all() and (exact.dist[off_diag] > 0).all()
    assert (es.dist[~same] <= 4).all() and (es.dist[~same] >= 1).all()  # one element changed per trace, at most


# ---- 5. the device-pointer forms on a side stream ----------------------------------------------------------------------
def test_dev_forms_on_a_side_stream(ctx):
    import torch
    w, name = 100, "mod2"
    trs, ents, G = gpu_family(name)
    n = 36
    ts = hs.TraceSet(list(trs[:n]))
    ent = np.concatenate(ents[:n])
    N = int(ts.off[-1])
    allp = EC.all_ordered_pairs(n)
    launches = [allp[::3][:400], allp[1::3][:250]]
    plan = hs.AlignPoPlan(w, G, max(len(t) for t in trs[:n]), 400, ctx=ctx)
    try:
        assert plan.slots >= 1 and plan.sub_pair_bytes >= 400 * G * (w * 12 + 12)
        side = torch.cuda.Stream()
        d_off = torch.from_numpy(ts.off.view(np.int64)).cuda()
        d_sym = torch.from_numpy(ts.sym.view(np.int64)).cuda()
        d_ent = torch.from_numpy(ent.view(np.int32)).cuda()
        d_poff = torch.full((n * G + 1,), 7, dtype=torch.int64, device="cuda")
        d_psym = torch.full((N + 1,), 7, dtype=torch.int64, device="cuda")
        d_psrc = torch.full((N + 1,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # the copies and the fills ran on torch's current stream
        plan.project_dev(d_off.data_ptr(), d_sym.data_ptr(), d_ent.data_ptr(), n, d_poff.data_ptr(), d_psym.data_ptr(),
                         d_psrc.data_ptr(), side.cuda_stream)
        for pairs in launches:  # the same plan again: the scratch holds the last launch's sub-scripts
            pairs = np.ascontiguousarray(pairs, np.uint32)
            dist, ops = expected(name, pairs, w)
            assert (dist <= w).sum() >= 16 and (dist > w).sum() >= 16
            d_pairs = torch.from_numpy(pairs.view(np.int32)).cuda()
            d_dist = torch.full((len(pairs),), 7, dtype=torch.int32, device="cuda")
            d_ops = torch.full((len(pairs) * w * 3,), 7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            plan.pairs_dev(d_off.data_ptr(), d_poff.data_ptr(), d_psym.data_ptr(), d_psrc.data_ptr(),
                           d_pairs.data_ptr(), len(pairs), d_dist.data_ptr(), d_ops.data_ptr(), side.cuda_stream)
            side.synchronize()
            assert np.array_equal(d_dist.cpu().numpy().view(np.uint32), dist)
            got_o = d_ops.cpu().numpy().view(np.uint32).reshape(len(pairs), w, 3)
            assert np.array_equal(got_o, np.stack([ops["a_pos"], ops["b_pos"], ops["kind"]], axis=2))
        want = numpy_projection(ts, ent, G)
        assert np.array_equal(d_poff.cpu().numpy().view(np.uint64), want[0])
        assert np.array_equal(d_psym.cpu().numpy().view(np.uint64)[:len(want[1])], want[1])
        assert np.array_equal(d_psrc.cpu().numpy().view(np.uint32)[:len(want[2])], want[2])
        with pytest.raises(_lib.NmzInvalidArgument, match=r"n_pairs 401 exceeds the plan's max_pairs \(400\)"):
            plan.pairs_dev(d_off.data_ptr(), d_poff.data_ptr(), d_psym.data_ptr(), d_psrc.data_ptr(),
                           d_pairs.data_ptr(), 401, d_dist.data_ptr(), d_ops.data_ptr(), side.cuda_stream)
        plan.pairs_dev(0, 0, 0, 0, 0, 0, 0, 0, side.cuda_stream)  # no pairs: nothing is enqueued
    finally:
        plan.close()


# ---- 6. the profile ----------------------------------------------------------------------------------------------------
def same_profile(got, want):
    assert np.array_equal(got.symbols, want.symbols)
    for f in _lib.MOVE_COUNTS_DTYPE.names:
        assert np.array_equal(got.counts[f], want.counts[f]), f
    for f in _lib.MOVE_INFO_DTYPE.names:
        assert int(got.info[f]) == int(want.info[f]), f
    assert np.array_equal(got.dist, want.dist)


@pytest.mark.parametrize("name", ["mod2", "sparse"])
def test_profile_of_the_family(ctx, name):
    """nmz_ed_diff_profile_po against nmz_move_profile_wide_host over the host PO scripts: the definition."""
    w = 65
    ts, ent, G = family_store(name)
    pairs = EC.all_ordered_pairs(len(ts))
    dist, ops = expected(name, pairs, w)
    want = hs.move_profile_of_wide(ts, pairs, hs.EditScripts(dist, ops, w), host=True)
    got = hs.move_profile_po(ts, ent, pairs, w, n_entities=G, ctx=ctx)
    same_profile(got, want)
    assert int(got.info["n_scripts"]) >= 16 and int(got.info["n_beyond"]) >= 16 and int(got.info["n_ops"]) > 1000
    # under `sparse` every entity holds one symbol, so a sub-script is all DELs or all INSs: nothing moves
    assert ((got.counts["later"] > 0).any() if name == "mod2" else not got.counts["later"].any())
    assert (got.counts["dropped"] > 0).any() and (got.counts["extra"] > 0).any()


def test_profile_of_the_rotation(ctx):
    k = 33
    a, b, ea, eb = rot(k)
    ts = hs.TraceSet([EC.encode(a), EC.encode(b)])
    pairs = np.array([[0, 1], [1, 0]], np.uint32)
    split = hs.move_profile_po(ts, np.array(ea + eb, np.uint32), pairs, 2 * k, n_entities=2, ctx=ctx)
    assert split.dist.tolist() == [0, 0] and not split.counts.tobytes().strip(b"\0")
    assert [int(split.info[f]) for f in _lib.MOVE_INFO_DTYPE.names] == [2, 0, 0, 0]
    one = hs.move_profile_po(ts, np.zeros(8 * k, np.uint32), pairs, 2 * k, n_entities=1, ctx=ctx)
    exact = hs.move_profile_wide(ts, pairs, 2 * k, ctx=ctx)
    assert one.dist.tolist() == [2 * k, 2 * k] and one.counts.tobytes() == exact.counts.tobytes()
    assert one.info.tobytes() == exact.info.tobytes() and one.dist.tobytes() == exact.dist.tobytes()
    x = int(np.searchsorted(one.symbols, EC.encode([1])[0]))
    assert one.counts[x]["later"] == k and one.counts[x]["earlier"] == k


# ---- 7. Naive.DiffFailing / DiffSimilar with po=True ---------------------------------------------------------------------
def _event(entity, n):
    return {"uuid": "00000000-0000-0000-0000-%012d" % (1000 * int(entity[2:]) + n), "entity": entity, "type": "event",
            "class": "PacketEvent", "deferred": True, "option": {"src_entity": entity, "dst_entity": "zk", "seq": n}}


def _action(ev):
    return {"uuid": "act-" + ev["uuid"], "entity": ev["entity"], "type": "action", "class": "AcceptEventAction",
            "event_uuid": ev["uuid"], "option": {}}


def _interleave(rng, seqs):
    order = rng.permutation(np.repeat(np.arange(len(seqs)), [len(s) for s in seqs]))
    at = [0] * len(seqs)
    out = []
    for g in order:
        out.append(seqs[g][at[g]])
        at[g] += 1
    return [_action(e) for e in out], out


def test_diff_failing_and_diff_similar_in_po(ctx, tmp_path):
    """Four passing runs are random interleavings of three entities' fixed event sequences; the two failing runs are
    two more interleavings in which one event of zk1 is delivered three places later within its entity."""
    from test_visualize import write_store
    rng = np.random.default_rng(77)
    seqs = [[_event("zk%d" % g, n) for n in range(L)] for g, L in enumerate((12, 10, 8))]
    moved = list(seqs)
    moved[1] = seqs[1][:3] + seqs[1][4:7] + [seqs[1][3]] + seqs[1][7:]
    tr = [_interleave(rng, seqs) for _ in range(4)] + [_interleave(rng, moved) for _ in range(2)]
    write_store(str(tmp_path), tr)
    for i in range(6):
        with open(os.path.join(str(tmp_path), "%08x" % i, "result.json"), "w") as f:
            json.dump({"successful": i < 4, "required_time": 1}, f)
    st = hs.LoadStorage(str(tmp_path))
    runs = st.traces()
    band, k = 64, 4
    x = int(runs[4].symbols[[e["option"]["seq"] == 3 and e["entity"] == "zk1" for e in tr[4][1]].index(True)])
    exact = st.DiffFailing(band, k=k, ctx=ctx)
    prof = st.DiffFailing(band, k=k, ctx=ctx, po=True)
    # every failing run with all four passing runs (30 elements: no two runs are more than 60 edits apart), each
    # failing run's neighbours in the exact search's order
    assert prof.pairs.tolist() == exact.pairs.tolist()
    assert sorted(prof.pairs.tolist()) == sorted([j, f] for f in (4, 5) for j in range(4))
    assert prof.dist.tolist() == [2] * 8 and (exact.dist > 2).all()
    top = prof.top(1)
    assert len(top) == 1 and top[0][0] == x and top[0][1]["later"] == 8 and top[0][1]["n_pairs"] == 8
    assert len(prof.top(10)) == 1 and len(exact.top(10)) > 1
    assert int(prof.info["n_ops"]) == 16 < int(exact.info["n_ops"])
    # the definition: the host profile over the host PO scripts
    ts, ent, names = hs.po_entities(runs)
    assert names == ["zk0", "zk1", "zk2"]
    pairs = prof.pairs.astype(np.uint32)  # stored-run ids are the traces' indices here
    slots = [po_slots(ts.trace(i), ent[int(ts.off[i]):int(ts.off[i + 1])], ts.trace(j),
                      ent[int(ts.off[j]):int(ts.off[j + 1])], 3, band) for i, j in pairs.tolist()]
    eh = hs.EditScripts(np.array([d for d, _ in slots], np.uint32), np.stack([o for _, o in slots]), band)
    same_profile(prof, hs.move_profile_of_wide(ts, pairs, eh, host=True))
    # DiffSimilar: the failing run 4 against every stored run
    got = st.DiffSimilar(runs[4], k=6, band=band, po=True)
    plain = st.DiffSimilar(runs[4], k=6, band=band)
    assert sorted(i for i, _, _ in got) == sorted(i for i, _, _ in plain) == list(range(6))
    by_id = {i: (d, sc) for i, d, sc in got}
    assert by_id[4][0] == 0 and by_id[5][0] == 0 and len(by_id[5][1]) == 0
    assert {i: d for i, d, _ in plain}[5] > 0
    for i in range(4):
        d, sc = by_id[i]
        assert d == 2 and [int(o["kind"]) for o in sc] == [AR.DEL, AR.INS]
        assert int(runs[i].symbols[sc[0]["a_pos"]]) == x and int(runs[4].symbols[sc[1]["b_pos"]]) == x
    with pytest.raises(TypeError):
        st.DiffSimilar(runs[4].symbols, k=6, band=band, po=True)
