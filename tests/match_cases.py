"""Generator of the run-matching test storages ("Matching stored runs"): event universes with
repeated symbols, arrival ties and awkward 64-bit values, and recorded runs that miss events, repeat symbols beyond
the universe's count and carry symbols the universe does not hold. The expected rows come from
historystorage.run_positions (numpy, match_target), computed once per case and shared read-only.

Universe of E events over U distinct symbols: odd 64-bit values, except that symbol 0 is the value 0, symbol 1 is
2^64 - 1 and symbol 3 shares its low 32 bits with symbol 2 (as far as U allows). The first U events use every symbol
once, the others draw uniformly, and the events are shuffled. Arrivals are integers(0, E // 2 + 1) * 1000: many
ties, in an order unrelated to the index.

A run of length L is blocks concatenated and cut to L. A block is the events' symbols, each kept with probability
0.8, plus max(1, E // 10) unknown symbols (even, nonzero) and as many duplicates of events' symbols, shuffled."""
import functools

import numpy as np

from namazu_amd import historystorage as hs

NONE = 0xFFFFFFFF
CASES = [(1, 1), (2, 1), (64, 5), (65, 65), (300, 40), (1024, 300), (4096, 4096), (4096, 1), (4096, 300)]
# the lengths every case is run at; k_match_runs works in workgroups of 64, 256 or 1,024 threads and tiles of four
# times that, so only 256 is missing from the list: 255, 256, 257 and 513 follow it
BASE_LENGTHS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 9000]
LENGTHS = BASE_LENGTHS + [255, 256, 257, 513]
SEED = 8  # the (1, 1) and (2, 1) universes meet test_match_host's conditions only for some seeds: this is one


def universe(E, U, rng):
    vals = set()
    while len(vals) < U:
        vals.update(int(v) | 1 for v in rng.integers(0, 2**64, U - len(vals), dtype=np.uint64))
    usym = np.array(sorted(vals), np.uint64)
    rng.shuffle(usym)
    if U >= 1:
        usym[0] = 0
    if U >= 2:
        usym[1] = 2**64 - 1
    if U >= 4:
        usym[3] = int(usym[2]) ^ (0x5A5A5A5A << 32)
    assert len(set(usym.tolist())) == U
    ids = np.concatenate([np.arange(min(U, E)), rng.integers(0, U, max(E - U, 0))])[:E]
    rng.shuffle(ids)
    sym = usym[ids]
    arrival = rng.integers(0, E // 2 + 1, E).astype(np.int64) * 1000
    return sym, arrival


def run(sym, L, rng):
    E = len(sym)
    known = set(sym.tolist())
    n_extra = max(1, E // 10)
    parts, n = [], 0
    while n < L:
        kept = sym[rng.random(E) < 0.8]
        unknown = rng.integers(1, 2**63, n_extra, dtype=np.uint64) * np.uint64(2)
        assert not known & set(unknown.tolist())
        dup = sym[rng.integers(0, E, n_extra)]
        block = np.concatenate([kept, unknown, dup])
        rng.shuffle(block)
        parts.append(block)
        n += len(block)
    return np.concatenate(parts)[:L] if parts else np.zeros(0, np.uint64)


@functools.lru_cache(maxsize=None)
def case(E, U):
    """(sym, arrival, runs, expected): one run per length in LENGTHS, expected = run_positions' rows. Read-only."""
    rng = np.random.default_rng([SEED, E, U])
    sym, arrival = universe(E, U, rng)
    runs = tuple(run(sym, L, rng) for L in LENGTHS)
    exp = hs.run_positions(sym, arrival, list(runs))
    for a in (sym, arrival, exp) + runs:
        a.setflags(write=False)
    return sym, arrival, runs, exp


def over_full_pairs(sym, runs):
    """The number of (run, symbol) pairs with more occurrences in the run than the universe holds."""
    vals, cnt = np.unique(sym, return_counts=True)
    have = dict(zip(vals.tolist(), cnt.tolist()))
    n = 0
    for r in runs:
        rv, rc = np.unique(r, return_counts=True)
        n += sum(1 for v, c in zip(rv.tolist(), rc.tolist()) if v in have and c > have[v])
    return n
