"""Writes delivery_order_kat.json: delivery-order classes of replayable seeds computed with FNV-1a alone.

Imports neither the product nor the oracle. release = arrival + FNV1a64(seed || hint) % m
(replayablepolicy.go:100-126); the delivery order sorts the events by (release, index); seeds with the same order
(exact) or the same per-entity orders (PO) form a class (visualize.go:51-136).

    python tests/golden/make_delivery_order_kat.py > tests/golden/delivery_order_kat.json
"""
import json

MS = 1_000_000


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


def classes(keys):
    first, heads = {}, []
    for i, k in enumerate(keys):
        if k not in first:
            first[k] = i
            heads.append(i)
    sizes = {}
    for k in keys:
        sizes[first[k]] = sizes.get(first[k], 0) + 1
    return heads, sizes


def fixture(n_events, m, n_seeds, entities=None):
    hints = [hint(i) for i in range(n_events)]
    arrival = [i * MS for i in range(n_events)]
    seeds = [str(s) for s in range(n_seeds)]
    orders = [order(s, hints, arrival, m)[0] for s in seeds]
    out = {"hints": hints, "arrival_ns": arrival, "sym": [fnv1a64(b"hint%d" % i) for i in range(n_events)],
           "max_interval_ns": m, "n_seeds": n_seeds}
    heads, sizes = classes([tuple(o) for o in orders])
    out["exact"] = {"n_classes": len(heads), "largest_class": max(sizes.values()),
                    "n_merged": sum(1 for v in sizes.values() if v >= 2),
                    "n_singletons": sum(1 for v in sizes.values() if v == 1),
                    "heads": [{"seed": seeds[h], "order": orders[h], "size": sizes[h]} for h in heads]}
    if entities is not None:
        po = [tuple(tuple(e for e in o if entities[e] == v) for v in sorted(set(entities))) for o in orders]
        heads, sizes = classes(po)
        out["entity"] = entities
        out["po"] = {"n_classes": len(heads), "largest_class": max(sizes.values()),
                     "heads": [{"seed": seeds[h], "size": sizes[h]} for h in heads]}
    return out


if __name__ == "__main__":
    print(json.dumps({"G": fixture(6, 6 * MS, 512), "H": fixture(8, 4 * MS, 2049, [0, 1, 0, 1, 2, 2, 0, 1])},
                     indent=1))
