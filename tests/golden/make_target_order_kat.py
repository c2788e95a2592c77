"""Writes target_order_kat.json: distances of replayable seeds' delivery orders to a recorded order, computed with
FNV-1a alone.

Imports neither the product nor the oracle. release = arrival + FNV1a64(seed || hint) % m
(replayablepolicy.go:100-126); the delivery order sorts the events by (release, index); the target is the order of
seed "100". Per seed: n_discordant (pairs of one compared sequence delivered the other way round than the target),
prefix_len (leading target events all in place), n_in_place, min_gap_ns; the top-8 in both rank modes.

    python tests/golden/make_target_order_kat.py > tests/golden/target_order_kat.json
"""
import json

MS = 1_000_000
NONE = 0xFFFFFFFF
INT64_MAX = 2**63 - 1


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for b in data:
        h = ((h ^ b) * 0x100000001b3) & (2**64 - 1)
    return h


def hint(i):
    return str(fnv1a64(b"hint%d" % i) - 2**63)


def order(seed, hints, arrival, m):
    rel = [a + (fnv1a64((seed + h).encode()) % m if m else 0) for h, a in zip(hints, arrival)]
    return sorted(range(len(hints)), key=lambda e: (rel[e], e)), rel


def distance(o, rel, tpos, entities):
    """(n_discordant, prefix_len, n_in_place, min_gap_ns) of the delivery order o against target positions tpos."""
    seqs = [o] if entities is None else [[e for e in o if entities[e] == v] for v in sorted(set(entities))]
    nd, nin, gap = 0, 0, INT64_MAX
    out_of_place = []
    for q in seqs:
        nd += sum(1 for i in range(len(q)) for j in range(i + 1, len(q)) if tpos[q[i]] > tpos[q[j]])
        by_target = sorted(q, key=lambda e: tpos[e])
        for i, e in enumerate(q):
            if by_target[i] == e:
                nin += 1
            else:
                out_of_place.append(tpos[e])
            if i:
                gap = min(gap, rel[e] - rel[q[i - 1]])
    return nd, min(out_of_place) if out_of_place else len(o), nin, gap


def fixture(n_events, m, n_seeds, target_seed, entities=None):
    hints = [hint(i) for i in range(n_events)]
    arrival = [i * MS for i in range(n_events)]
    seeds = [str(s) for s in range(n_seeds)]
    target, _ = order(target_seed, hints, arrival, m)
    tpos = [target.index(e) for e in range(n_events)]  # dense: the position is the dense target position
    rows = [distance(*order(s, hints, arrival, m), tpos, entities) for s in seeds]
    sizes = [n_events] if entities is None else [entities.count(v) for v in sorted(set(entities))]
    n_pairs = sum(n * (n - 1) // 2 for n in sizes)
    out = {"hints": hints, "arrival_ns": arrival, "max_interval_ns": m, "n_seeds": n_seeds,
           "target_seed": target_seed, "target_order": target, "target_pos": tpos, "n_counted": n_events,
           "n_pairs": n_pairs, "n_discordant": [r[0] for r in rows], "prefix_len": [r[1] for r in rows],
           "n_in_place": [r[2] for r in rows], "min_gap_ns": [r[3] for r in rows]}
    if entities is not None:
        out["entity"] = entities
    pairs = sorted(range(n_seeds), key=lambda s: (-(n_pairs - rows[s][0]), -rows[s][3], s))[:8]
    prefix = sorted(range(n_seeds), key=lambda s: (-rows[s][1], -(n_pairs - rows[s][0]), s))[:8]
    out["top8_pairs"] = [{"seed": s, "sum_delay_ns": rows[s][3], "n_fault": n_pairs - rows[s][0],
                          "first_fault": rows[s][1]} for s in pairs]
    out["top8_prefix"] = [{"seed": s, "sum_delay_ns": n_pairs - rows[s][0], "n_fault": rows[s][1],
                           "first_fault": rows[s][2]} for s in prefix]
    return out


if __name__ == "__main__":
    print(json.dumps({"G": fixture(6, 6 * MS, 512, "100"),
                      "H": fixture(8, 10 * MS, 512, "100", [0, 1, 0, 1, 2, 2, 0, 1])}, indent=1))
