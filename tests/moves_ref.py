"""Move profiles by the definition, in pure Python (not a test module).

Dicts and ints only, over the ops of tests/align_ref.py's `script` -- [(a_pos, b_pos, kind)] -- and nothing from the
library: DESIGN.md section 2, "Move profiles", restated. The host forms (nmz_script_moves_host,
nmz_move_profile_host) are tied to this in tests/test_moves_host.py, and the GPU tests compare with the host forms."""
import align_ref as AR

SUB, DEL, INS = AR.SUB, AR.DEL, AR.INS
FIELDS = ("later", "earlier", "dropped", "extra", "sub_from", "sub_to", "n_pairs", "reserved", "span_later",
          "span_earlier")


def names(a, b, op):
    """The symbols an op names: (from, to), None where it names none."""
    ap, bp, kind = op
    return (int(a[ap]) if kind in (SUB, DEL) else None, int(b[bp]) if kind in (SUB, INS) else None)


def partners(a, b, ops):
    """partner[s] for every op of one script: the slot of the r-th INS naming v for the r-th DEL naming v and the
    other way round, None without one (and for every SUB)."""
    dels, inss = {}, {}
    for s, op in enumerate(ops):
        frm, to = names(a, b, op)
        if op[2] == DEL:
            dels.setdefault(frm, []).append(s)
        elif op[2] == INS:
            inss.setdefault(to, []).append(s)
    out = [None] * len(ops)
    for v, ds in dels.items():
        for d, i in zip(ds, inss.get(v, [])):
            out[d], out[i] = i, d
    return out


def moves(a, b, ops):
    """[(symbol, del slot, ins slot, later?, span)] of one script."""
    pr = partners(a, b, ops)
    return [(int(a[op[0]]), s, pr[s], pr[s] > s, abs(ops[pr[s]][1] - op[1]))
            for s, op in enumerate(ops) if op[2] == DEL and pr[s] is not None]


def empty_counts():
    return dict.fromkeys(FIELDS, 0)


def tally(a, b, ops, table, counts, info):
    """Add one script to counts {symbol: {field: int}} (symbols of `table` only) and info."""
    pr = partners(a, b, ops)
    named = set()

    def rec(v):
        named.add(v)
        if v not in table:
            info["n_unknown"] += 1
            return None
        return counts.setdefault(v, empty_counts())

    for s, op in enumerate(ops):
        frm, to = names(a, b, op)
        if op[2] == SUB:
            c = rec(frm)
            if c:
                c["sub_from"] += 1
            c = rec(to)
            if c:
                c["sub_to"] += 1
        elif op[2] == DEL:
            c = rec(frm)
            if not c:
                continue
            if pr[s] is None:
                c["dropped"] += 1
            else:
                way = "later" if pr[s] > s else "earlier"
                c[way] += 1
                c["span_" + way] += abs(ops[pr[s]][1] - op[1])
        else:
            c = rec(to)
            if c and pr[s] is None:
                c["extra"] += 1
    for v in named:
        if v in table:
            counts[v]["n_pairs"] += 1
    return pr


def profile(traces, pairs, w, table=None, scripts=None):
    """(partner, counts, info, dist) over pairs of `traces` (lists of ints) at band w. partner[p] = [slot or None] *
    w; counts = {symbol: {field: int}} for the table's symbols that some op names; `table` = a set (default: every
    symbol of the traces). `scripts` = {(i, j): (dist, ops or None)} replaces align_ref."""
    if table is None:
        table = {int(x) for t in traces for x in t}
    counts, info = {}, {"n_scripts": 0, "n_beyond": 0, "n_ops": 0, "n_unknown": 0}
    partner, dist = [], []
    for i, j in pairs:
        a, b = traces[i], traces[j]
        d, ops = scripts[(i, j)] if scripts is not None else AR.script(a, b, w, band=w)
        dist.append(d)
        if ops is None:
            info["n_beyond"] += 1
            partner.append([None] * w)
            continue
        info["n_scripts"] += 1
        info["n_ops"] += d
        partner.append(tally(a, b, ops, table, counts, info) + [None] * (w - d))
    return partner, counts, info, dist


def script_kinds(a, b, ops):
    """What one script exercises, for the non-vacuity counts: (has a later move, has an earlier move, a value moves
    twice or more, a value has DELs and INSs in unequal numbers)."""
    mv = moves(a, b, ops)
    per_value = {}
    for v, *_ in mv:
        per_value[v] = per_value.get(v, 0) + 1
    nd, ni = {}, {}
    for op in ops:
        frm, to = names(a, b, op)
        if op[2] == DEL:
            nd[frm] = nd.get(frm, 0) + 1
        elif op[2] == INS:
            ni[to] = ni.get(to, 0) + 1
    unequal = any(v in ni and ni[v] != c for v, c in nd.items())
    return (any(m[3] for m in mv), any(not m[3] for m in mv), any(c >= 2 for c in per_value.values()), unequal)
