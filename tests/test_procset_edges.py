"""CPU: the conditions under which tests/test_procset_edges_gpu.py means what it says, stated with the reference alone
(tests/procset_ref.py over the oracle's Go generator, and the plain-Python restatements of tests/procset_cases.py):
stats_from_dump is the reference's statistics, the seed ranges fill units of 64 lanes and give three units per bucket,
the sample holds whole buckets, the traces are cut into the chunk counts the docstrings quote on any device of 80
compute units or more, and every extreme cell is one the entry points accept."""
import numpy as np
import pytest

import procset_cases as C
import procset_ref as R
from oracle import oracle as O

RP = O.random_params(C.RANGED[0], C.RANGED[1], 0.0)


def test_prefix_low_byte_is_the_oracles_fnv():
    for seed in (0, 1, 255, 256, C.SEED0, 2**32 - 1, 2**63, 2**64 - 1):
        assert C.prefix_low_byte(seed) == O.fnv1a64(seed.to_bytes(8, "little")) & 0xFF
        assert C.prefix_low_byte(seed) == O.fnv1a64_py(seed.to_bytes(8, "little")) & 0xFF
    members = C.bucket_members(2**64 - 3, 7)  # a range that wraps: indices, not seeds
    assert sorted(i for m in members for i in m) == list(range(7))
    assert members[C.prefix_low_byte(1)].count(4) == 1


@pytest.mark.parametrize("name", C.POLICIES)
def test_stats_from_dump_is_the_references_statistics(name):
    """64 seeds over the E = 15 trace of the full-unit test: both entity classes, an event of 33, a zero-process
    event (mild) and targets on every second event."""
    tr = C.full_unit_trace(name, 15)
    assert set(tr.evclass.tolist()) == {0, 1} and 33 in tr.n_procs.tolist()
    assert (0 in tr.n_procs.tolist()) == (name == "mild")
    n_targets = int(np.count_nonzero(tr.target != C.NONE))
    assert 6 <= n_targets <= 8
    st, dl, at, _ = R.sweep(C.SEED0, 64, *tr.args(), RP, C.ref_params(name), n_dump=64)
    got = C.stats_from_dump(name, dl, at, tr.n_procs, tr.target)
    assert np.array_equal(got, st)
    assert len(set(st["target_score"].tolist())) > 2 and len(set(st["score_sum"].tolist())) > 4  # not degenerate
    none = C.stats_from_dump(name, dl, at, tr.n_procs, tr.without_targets().target)
    assert np.all(none["target_score"] == 0) and np.array_equal(none["score_sum"], st["score_sum"])


def test_seed_ranges_fill_the_units():
    """S = 20,000: a full unit and a partial one in every bucket (also for the range that wraps past 2^64).
    S = 33,000: three units in at least 200 buckets, the last of one or two lanes."""
    for seed0 in (C.SEED0, C.WRAP_SEED0):
        sizes = [len(m) for m in C.bucket_members(seed0, C.FULL_S)]
        assert sum(sizes) == C.FULL_S and min(sizes) >= 65 and max(sizes) <= 128
    assert (C.WRAP_SEED0 + C.FULL_S) >> 64 == 1
    sizes = [len(m) for m in C.bucket_members(C.SEED0, C.THREE_S)]
    assert sum(sizes) == C.THREE_S and max(sizes) <= 192
    assert sum(1 for s in sizes if s > 128) >= 200
    assert any(s in (129, 130) for s in sizes)
    assert min(sizes) >= 128  # every other bucket: two full units, lane < cnt at cnt == 64 twice


def test_sample_holds_two_whole_buckets():
    members = C.bucket_members(C.SEED0, C.THREE_S)
    sample = C.sample_indices()
    assert list(sample) == sorted(set(sample)) and 0 <= sample[0] and sample[-1] < C.THREE_S
    buckets = C.triple_buckets(C.SEED0, C.THREE_S)
    assert len(buckets) == 2
    for b in buckets:
        assert len(members[b]) in (129, 130) and set(members[b]) <= set(sample)
    assert set(range(64)) <= set(sample) and set(range(C.THREE_S - 64, C.THREE_S)) <= set(sample)
    assert 64 + 64 + 128 + 2 * 129 - 16 <= len(sample) <= 64 + 64 + 128 + 2 * 130


def test_chunk_counts():
    """What chunks(..., 256) gives, and that any device of 80 compute units or more cuts the same."""
    want = {(15, C.FULL_S): (15, 1), (24, C.FULL_S): (8, 3), (C.THREE_E, C.THREE_S): (C.THREE_EC, C.THREE_CHUNKS)}
    want.update({(E, C.JOINT_S): c for E, c in C.JOINT_CHUNKS.items()})
    want[(len(C.grid_trace()), C.GRID_S)] = (11, 1)
    want[(len(C.grid_trace(True)), C.GRID_S)] = (12, 1)
    want[(len(C.mild_grid_trace()), C.GRID_S)] = (4, 1)
    assert sorted(C.JOINT_CHUNKS) == [15, 16, 17, 31, 32, 33, 65]
    for (E, S), c in want.items():
        assert C.chunks(E, S, C.N_CU) == c, (E, S)
        for n_cu in list(range(80, 400)) + [512, 1024, 4096]:
            assert C.chunks(E, S, n_cu) == c, (E, S, n_cu)
    ec, n = C.chunks(C.THREE_E, C.THREE_S, C.N_CU)
    assert C.THREE_E - ec * (n - 1) == C.THREE_TAIL == 5  # the ragged last chunk
    assert [C.chunks(17, C.JOINT_S, C.N_CU), 17 - 9] == [(9, 2), 8]  # 9 + 8
    # the measured workload (tools/procset_rate.py: 2^20 seeds x 1,000 events) has units enough: 4 chunks of 250
    assert C.chunks(1000, 2**20, C.N_CU) == (250, 4)


def test_three_unit_traces():
    for name in C.POLICIES:
        tr = C.three_unit_trace(name)
        n = tr.n_procs.tolist()
        assert len(tr) == C.THREE_E and [n[e] for e in C.BIG_EVENTS] == [64, 65, 512]
        small = [x for e, x in enumerate(n) if e not in C.BIG_EVENTS and x]
        assert set(small) == set(range(1, 9))
        zeros = [e for e, x in enumerate(n) if x == 0]
        assert zeros == (list(C.MILD_ZERO_EVENTS) if name == "mild" else [])
        assert tr.target[150] == 511 and 95 <= np.count_nonzero(tr.target != C.NONE) <= 102
        assert all(t == C.NONE or t < x for t, x in zip(tr.target.tolist(), n))
    ec = C.THREE_EC
    last, first, _, tail = C.MILD_ZERO_EVENTS
    assert last % ec == ec - 1 and first % ec == 0 and tail >= ec * (C.THREE_CHUNKS - 1)


def test_every_cell_is_one_the_entry_points_accept():
    """ps_inputs' rules: n <= 512, a target is a slot of its event, extreme has a process unless prioritized <= 0,
    dirichlet always has one."""
    cells = C.extreme_cells()
    assert [pr for pr, _ in cells] == [-1, 0, 1, 64, 256]
    for pr, tr in cells:
        n = tr.n_procs.tolist()
        assert n[:11] == list(C.GRID_N_PROCS) and tr.target.tolist()[:11] == list(C.GRID_TARGETS)
        assert (0 in n) == (pr <= 0) and pr <= 256
        assert all(x > 0 or pr <= 0 for x in n) and max(n) <= 512
        assert all(t == C.NONE or t < x for t, x in zip(tr.target.tolist(), n))
    assert all(x > 0 for x in C.grid_trace().n_procs)  # dirichlet's trace
    assert [int(p * 1000.0) for p, _ in C.DIRICHLET_RESET] == [t for _, t in C.DIRICHLET_RESET] == [0, 1, 999, 1000]
    assert C.ref_params("dirichlet", reset_probability=0.999).reset_threshold == 999
    m = C.mild_grid_trace()
    assert m.n_procs.tolist() == [0, 1, 512, 512] and m.target.tolist() == [C.NONE, 0, 0, 511]
    # bit 31 of a mark word, bit 0 of a later word, and slot 511
    assert {31, 63, 95} <= set(C.GRID_TARGETS) and {32, 64} <= set(C.GRID_TARGETS) and 511 in C.GRID_TARGETS
    for name in C.POLICIES:
        for E in C.FULL_E:
            tr = C.full_unit_trace(name, E)
            assert 80 <= int(tr.n_procs.sum()) <= 150 and all(x > 0 or name == "mild" for x in tr.n_procs)
