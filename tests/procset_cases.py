"""Cases for the ProcSet sweep at full waves, many chunks and parameter edges (helper, not a test file): the bucket a
seed falls in and the chunking of the events, both restated in plain Python from namazu_amd/csrc/procset.hip and
random_dev.h; the per-seed statistics restated over full decisions; and the traces, parameter cells and seed samples of
tests/test_procset_edges.py and tests/test_procset_edges_gpu.py. Nothing here calls the library under test."""
import functools

import numpy as np

import procset_ref as R

NONE = R.NONE
M64 = R.M64
POLICIES = ["mild", "extreme", "dirichlet"]
RANGED = (30_000_000, 100_000_000)
FIXED = (5_000_000, 5_000_000)
SEED0 = 77_000
N_CU = 256  # the chunk counts quoted in the tests' docstrings are for 256 compute units

FNV_OFFSET, FNV_PRIME = 0xCBF29CE484222325, 0x100000001B3


def prefix_low_byte(seed):
    """The low byte of FNV-1a 64 over le64(seed): the bucket of the sweep kernels' units."""
    h = FNV_OFFSET
    for i in range(8):
        h = ((h ^ ((seed >> (8 * i)) & 0xFF)) * FNV_PRIME) & M64
    return h & 0xFF


def bucket_members(seed0, S):
    """256 lists: the indices i of the seeds (seed0 + i) mod 2^64, i < S, that fall in each bucket, ascending."""
    out = [[] for _ in range(256)]
    for i in range(S):
        out[prefix_low_byte((seed0 + i) & M64)].append(i)
    return out


def chunks(E, S, n_cu):
    """(ec, n_chunks) of ps_sweep_launch: the events are cut into chunks of at least 8 when the seeds alone give too
    few units for the persistent grid."""
    max_units, slots = S // 64 + 256, n_cu * 32
    n_chunks = min((8 * slots + max_units - 1) // max_units, max(1, E // 8))
    ec = (E + n_chunks - 1) // n_chunks
    return ec, (E + ec - 1) // ec


def stats_from_dump(name, delays, attrs, n_procs, target):
    """The per-seed statistics (R.STATS_DTYPE, flags 0) from full decisions: delays int64[S, E] and attrs[S, sum
    n_procs] with fields policy, nice, priority. The score of a slot is -nice (mild), 1 + priority of an RR slot
    (extreme) or 1 for a NORMAL slot (dirichlet); a slot is special when nice < 0, RR or NORMAL."""
    delays, attrs = np.asarray(delays), np.asarray(attrs)
    S = delays.shape[0]
    pol = attrs["policy"].astype(np.int64)
    if name == "mild":
        score = -attrs["nice"].astype(np.int64)
        special = attrs["nice"] < 0
    elif name == "extreme":
        special = pol == R.RR
        score = np.where(special, 1 + attrs["priority"].astype(np.int64), 0)
    else:
        special = pol == R.NORMAL
        score = special.astype(np.int64)
    out = np.zeros(S, R.STATS_DTYPE)
    out["sum_delay_ns"] = delays.astype(np.uint64).sum(axis=1, dtype=np.uint64)
    out["score_sum"] = score.reshape(S, -1).sum(axis=1)
    out["n_special"] = special.reshape(S, -1).sum(axis=1)
    off = np.concatenate([[0], np.cumsum(np.asarray(n_procs, np.int64))])
    ts = np.zeros(S, np.int64)
    for e, t in enumerate(np.asarray(target).tolist()):
        if t != NONE:
            assert t < int(n_procs[e])
            ts += score[:, off[e] + t]
    out["target_score"] = ts
    return out


def ref_params(name, use_batch=True, prioritized=3, reset_probability=0.1):
    return R.Params(POLICIES.index(name), use_batch, prioritized, reset_probability)


class Trace:
    """evhash, evclass, n_procs, target of one trace (arrays that are not modified)."""

    def __init__(self, evhash, evclass, n_procs, target):
        self.evhash = np.asarray(evhash, np.uint64)
        self.evclass = np.asarray(evclass, np.uint8)
        self.n_procs = np.asarray(n_procs, np.uint32)
        self.target = np.asarray(target, np.uint32)
        assert len(self.evhash) == len(self.evclass) == len(self.n_procs) == len(self.target)
        for a in (self.evhash, self.evclass, self.n_procs, self.target):
            a.setflags(write=False)

    def __len__(self):
        return len(self.evhash)

    def args(self):
        return self.evhash, self.evclass, self.n_procs, self.target

    def without_targets(self):
        return Trace(self.evhash, self.evclass, self.n_procs, np.full(len(self), NONE, np.uint32))


def _hashes(rng, E):
    return rng.integers(0, 2**64, size=E, dtype=np.uint64)


def _targets(rng, n_procs, every=2, phase=0):
    """a valid slot on the events e with e % every == phase that have a process"""
    t = np.full(len(n_procs), NONE, np.uint32)
    for e, n in enumerate(n_procs):
        if e % every == phase and n > 0:
            t[e] = rng.integers(0, n)
    return t


# ---- 1. full units: E = 15 (one chunk) and E = 24 (three chunks of 8), S = 20,000
FULL_S = 20_000
FULL_E = (15, 24)
WRAP_SEED0 = 2**64 - 10_000


@functools.lru_cache(maxsize=None)
def full_unit_trace(name, E):
    """n_procs in 1..8 with one event of 33 (mild: also one of 0), both entity classes, targets on every second
    event."""
    rng = np.random.default_rng(1000 + E)
    n = rng.integers(1, 9, size=E)
    n[E // 2] = 33
    if name == "mild":
        n[E - 4] = 0
    return Trace(_hashes(rng, E), rng.integers(0, 2, size=E), n, _targets(rng, n))


# ---- 2. three units per bucket, 23 chunks with a ragged tail: E = 203, S = 33,000
THREE_S = 33_000
THREE_E = 203
THREE_EC, THREE_CHUNKS, THREE_TAIL = 9, 23, 5
THREE_PRIORITIZED = 64
BIG_EVENTS = {40: 64, 101: 65, 150: 512}  # event -> n_procs
MILD_ZERO_EVENTS = (8, 27, 60, 199)  # 8: the last event of chunk 0; 27: the first of chunk 3; 199: in the ragged tail


@functools.lru_cache(maxsize=None)
def three_unit_trace(name):
    """n_procs in 1..8 except three events of 64, 65 and 512 (mild: four events of 0, one the last and one the first
    event of a chunk); targets on every second event, slot 511 on the event of 512."""
    rng = np.random.default_rng(2030)
    E = THREE_E
    n = rng.integers(1, 9, size=E)
    for e, k in BIG_EVENTS.items():
        n[e] = k
    if name == "mild":
        for e in MILD_ZERO_EVENTS:
            n[e] = 0
    t = _targets(rng, n)
    t[150] = 511
    return Trace(_hashes(rng, E), rng.integers(0, 2, size=E), n, t)


def triple_buckets(seed0, S, count=2):
    """the first `count` buckets with 129 or 130 seeds: two full units and a last unit of one or two lanes"""
    return [b for b, m in enumerate(bucket_members(seed0, S)) if len(m) in (129, 130)][:count]


@functools.lru_cache(maxsize=None)
def sample_indices(seed0=SEED0, S=THREE_S):
    """Every member of two buckets with 129 or 130 seeds, indices 0..63 and S-64..S-1, and 128 more drawn with a
    fixed rng; ascending, without repeats."""
    members = bucket_members(seed0, S)
    idx = set(range(64)) | set(range(S - 64, S))
    for b in triple_buckets(seed0, S):
        idx |= set(members[b])
    rest = np.array(sorted(set(range(S)) - idx))
    idx |= set(np.random.default_rng(33).choice(rest, size=128, replace=False).tolist())
    return tuple(sorted(idx))


# ---- 3. chunk joints at a small sweep
JOINT_S = 128
JOINT_SEED0 = 5_000
JOINT_CHUNKS = {15: (15, 1), 16: (8, 2), 17: (9, 2), 31: (11, 3), 32: (8, 4), 33: (9, 4), 65: (9, 8)}  # E: (ec, n)


@functools.lru_cache(maxsize=None)
def joint_trace(E):
    rng = np.random.default_rng(3000 + E)
    n = rng.integers(1, 7, size=E)
    return Trace(_hashes(rng, E), rng.integers(0, 2, size=E), n, _targets(rng, n))


# ---- 4. the uniform form over the parameter grid
GRID_S = 128
GRID_SEED0 = 991_000
GRID_N_PROCS = (1, 2, 3, 31, 32, 33, 64, 65, 96, 511, 512)
GRID_TARGETS = (0, 1, 2, 30, 31, 32, 63, 64, 95, 510, 511)  # bit 31 and bit 0 of mark words, and the last slot
INTERVALS = {"ranged": RANGED, "fixed": FIXED}  # the sub-policy's first output index: 1 and 0
EXTREME_PRIORITIZED = (-1, 0, 1, 64, 256)
DIRICHLET_RESET = ((0.0, 0), (0.001, 1), (0.999, 999), (1.0, 1000))  # (resetProbability, threshold)


@functools.lru_cache(maxsize=None)
def grid_trace(with_zero=False):
    """GRID_N_PROCS with GRID_TARGETS, alternating entity classes; with_zero appends an event of no process."""
    n = list(GRID_N_PROCS) + ([0] if with_zero else [])
    t = list(GRID_TARGETS) + ([NONE] if with_zero else [])
    rng = np.random.default_rng(4000)
    return Trace(_hashes(rng, len(n)), np.arange(len(n)) % 2, n, t)


def extreme_cells():
    """(prioritized, trace): with prioritized <= 0 nothing is drawn per process, so an event of 0 is legal."""
    return [(pr, grid_trace(pr <= 0)) for pr in EXTREME_PRIORITIZED]


@functools.lru_cache(maxsize=None)
def mild_grid_trace():
    """n = 0, 1, 512 with targets 0 and 511"""
    rng = np.random.default_rng(4001)
    return Trace(_hashes(rng, 4), [0, 1, 1, 0], [0, 1, 512, 512], [NONE, 0, 0, 511])


def reference(seed0, S, trace, rp, pp, hits=None):
    """R.sweep's statistics of seeds seed0 .. seed0 + S - 1."""
    return R.sweep(seed0, S, *trace.args(), rp, pp, hits=hits)[0]


def reference_of(seed0, indices, trace, rp, pp):
    """R.sweep's statistics of the seeds seed0 + i, one seed at a time."""
    out = np.zeros(len(indices), R.STATS_DTYPE)
    for j, i in enumerate(indices):
        out[j] = R.sweep((seed0 + i) & M64, 1, *trace.args(), rp, pp)[0][0]
    return out
