"""Restatement of the nearest-order sweep's definition for the tests (not a test module).

On top of delivery_ref.Ref (releases, delivery order and gaps from the C oracle's delays), the definition of
include/nmz_gpu.h in numpy:

    counted       = target_pos != NMZ_NONE and (PO mode) entity != NMZ_NONE
    n_discordant  = pairs (i < j) of one compared sequence in delivery order with target_pos[i] > target_pos[j],
                    by the O(n^2) definition
    in place      = rank inside the compared sequence in delivery order == rank there by target_pos
    prefix_len    = the smallest dense target position of an event out of place, n_counted if none
    min_gap_ns, gap_event = delivery_ref.Ref's over the counted events

Everything is integer: tests compare with equality."""
import numpy as np

import delivery_ref as R

NONE = R.NONE
STATS_DTYPE = np.dtype([("n_discordant", "<u4"), ("prefix_len", "<u4"), ("min_gap_ns", "<i8"), ("gap_event", "<u4"),
                        ("n_in_place", "<u4")])
TOPK_DTYPE = np.dtype([("seed", "<u8"), ("sum_delay_ns", "<i8"), ("n_fault", "<u4"), ("first_fault", "<u4")])
SENTINEL = (2**64 - 1, -2**63, 0, NONE)


def discordant(tp):
    """Pairs i < j with tp[i] > tp[j], by the definition."""
    tp = np.asarray(tp, np.int64)
    n, total = len(tp), 0
    for i0 in range(0, n, 512):  # blocks of rows i against every later column j
        blk = tp[i0:i0 + 512]
        total += int(np.triu(blk[:, None] > blk[None, :], 1).sum())
        total += int(np.count_nonzero(blk[:, None] > tp[None, i0 + 512:]))
    return total


class TRef:
    """stats[S] (STATS_DTYPE), n_counted, n_pairs and order[S][G] of a trace against target_pos."""

    def __init__(self, dl, arrival, target_pos, entity=None):
        tp = np.asarray(target_pos, np.uint32)
        E = len(tp)
        ent = np.zeros(E, np.uint32) if entity is None else np.asarray(entity, np.uint32).copy()
        ent[tp == NONE] = NONE  # one entity for every event is exact mode
        ref = R.Ref(dl, arrival, np.zeros(E, np.uint64), ent)
        S = dl.shape[0]
        self.order = ref.order
        counted = np.nonzero(ent != NONE)[0]
        G = len(counted)
        dense = np.zeros(E, np.int64)
        dense[counted[np.argsort(tp[counted], kind="stable")]] = np.arange(G)
        groups = [counted[ent[counted] == v] for v in np.unique(ent[counted])]
        self.n_counted = G
        self.n_pairs = sum(len(g) * (len(g) - 1) // 2 for g in groups)
        self.stats = np.zeros(S, STATS_DTYPE)
        self.stats["min_gap_ns"] = ref.stats["min_gap_ns"]
        self.stats["gap_event"] = ref.stats["gap_event"]
        for s in range(S):
            o = self.order[s]
            nd, nin, pre = 0, 0, G
            for v in (np.unique(ent[counted]) if G else []):
                seq = o[ent[o] == v]          # the entity's events in delivery order
                t = tp[seq].astype(np.int64)
                nd += discordant(t)
                trank = np.argsort(np.argsort(t, kind="stable"), kind="stable")
                ok = trank == np.arange(len(seq))
                nin += int(ok.sum())
                if not ok.all():
                    pre = min(pre, int(dense[seq[~ok]].min()))
            self.stats[s]["n_discordant"] = nd
            self.stats[s]["n_in_place"] = nin
            self.stats[s]["prefix_len"] = pre


def topk(stats, n_pairs, seed_values, k, rank_by):
    """The top-k list of the header's ranking, by a Python sort: TOPK_DTYPE[k], sentinels past the seeds."""
    rows = []
    for st, sv in zip(stats, seed_values):
        conc = n_pairs - int(st["n_discordant"])
        if rank_by == "pairs":
            rows.append((int(sv), int(st["min_gap_ns"]), conc, int(st["prefix_len"])))
        else:
            rows.append((int(sv), conc, int(st["prefix_len"]), int(st["n_in_place"])))
    rows.sort(key=lambda r: (-r[2], -r[1], r[0]))
    out = np.zeros(k, TOPK_DTYPE)
    for i in range(k):
        out[i] = rows[i] if i < len(rows) else SENTINEL
    return out


def target_of_order(order, E, stride=1, offset=0):
    """target_pos[E] whose order is `order` (event indices); events not in it get NONE; positions stride * i +
    offset."""
    tp = np.full(E, NONE, np.uint32)
    tp[np.asarray(order, np.int64)] = np.arange(len(order), dtype=np.uint32) * np.uint32(stride) + np.uint32(offset)
    return tp


def host_target(seeds, hints, arrival, entity, target_pos, m):
    """nmz_replayable_target_host per seed string: (stats[S], n_counted, n_pairs)."""
    from namazu_amd import _lib
    from oracle import oracle as O
    L = _lib.load()
    ho, hb = O.to_csr(list(hints))
    E = len(hints)
    arr = np.ascontiguousarray(arrival, np.int64)
    tp = np.ascontiguousarray(target_pos, np.uint32)
    en = None if entity is None else np.ascontiguousarray(entity, np.uint32)
    st = np.zeros(len(seeds), _lib.TARGET_STATS_DTYPE)
    info = np.zeros(2, np.uint32)
    for i, s in enumerate(seeds):
        b = s.encode()
        sb = np.frombuffer(b, np.uint8) if b else np.zeros(1, np.uint8)
        _lib.check(L.nmz_replayable_target_host(_lib.ptr(sb), len(b), _lib.ptr(ho), _lib.ptr(hb), E, m, _lib.ptr(arr),
                                                _lib.ptr(en), _lib.ptr(tp), _lib.ptr(st[i:i + 1]),
                                                _lib.ptr(info[0:1]), _lib.ptr(info[1:2])))
    return st, int(info[0]), int(info[1])
