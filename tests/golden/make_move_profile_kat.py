"""Writes move_profile_kat.json: pairs of traces with their canonical script, the partner of every op, the counters
of every symbol an op names and the info record, by the definition ("Move profiles").

The scripts come from tests/align_ref.py; the pairing and the tally below are written out here with plain scans --
nothing from tests/moves_ref.py, nothing from the library -- so the known answers share nothing with the code they
check. The expectations the cases were chosen for are asserted before anything is written. Symbols are ints
(characters: code points); ops are [a_pos, b_pos, kind] with kind 0 = SUB, 1 = DEL, 2 = INS; "partner": null = none.

    python tests/golden/make_move_profile_kat.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import align_ref as AR  # noqa: E402

X, Y = 1000, 1001
B = list(range(1, 67))  # 66 distinct symbols


def chars(s):
    return [ord(c) for c in s]


CASES = [("abab-baba", chars("abab"), chars("baba"), 2), ("abcde-bcdex", chars("abcde"), chars("bcdex"), 2),
         ("ab-ba", chars("ab"), chars("ba"), 2), ("kitten-sitting", chars("kitten"), chars("sitting"), 3),
         ("kitten-sitting-beyond", chars("kitten"), chars("sitting"), 2), ("xxabc-abcx", chars("xxabc"), chars("abcx"), 4)]
for r, w in ((32, 64), (31, 63), (16, 32), (15, 31)):
    CASES += [(f"rot{r}-w{w}", [X] * r + B, B + [X] * r, w), (f"rot{r}-w{w}-rev", B + [X] * r, [X] * r + B, w)]
CASES += [("xy16-w64", [X] * 16 + [Y] * 16 + B, B + [Y] * 16 + [X] * 16, 64),
          ("x34-x30-w64", [X] * 34 + B, B + [X] * 30, 64), ("x30-x34-w64", [X] * 30 + B, B + [X] * 34, 64)]
FIELDS = ["later", "earlier", "dropped", "extra", "sub_from", "sub_to", "n_pairs", "span_later", "span_earlier"]


def kat(a, b, w):
    dist, ops = AR.script(a, b, w, band=w)
    if ops is None:
        return dist, None, None, {}, {"n_scripts": 0, "n_beyond": 1, "n_ops": 0, "n_unknown": 0}
    # the op's name as a DEL or an INS, its rank among the equal ones before it, then the partner by a scan
    name = [a[ap] if k == 1 else (b[bp] if k == 2 else None) for ap, bp, k in ops]
    rank = [sum(1 for t in range(s) if ops[t][2] == ops[s][2] and name[t] == name[s]) for s in range(len(ops))]
    partner = []
    for s, (_, _, k) in enumerate(ops):
        hit = [t for t in range(len(ops)) if k != 0 and ops[t][2] == 3 - k and name[t] == name[s] and rank[t] == rank[s]]
        assert len(hit) <= 1
        partner.append(hit[0] if hit else None)
    counts = {}

    def c(v):
        return counts.setdefault(v, dict.fromkeys(FIELDS, 0))

    for s, (ap, bp, k) in enumerate(ops):
        if k == 0:
            c(a[ap])["sub_from"] += 1
            c(b[bp])["sub_to"] += 1
        elif k == 1 and partner[s] is None:
            c(a[ap])["dropped"] += 1
        elif k == 2 and partner[s] is None:
            c(b[bp])["extra"] += 1
        elif k == 1:
            way = "later" if partner[s] > s else "earlier"
            c(a[ap])[way] += 1
            c(a[ap])["span_" + way] += abs(ops[partner[s]][1] - bp)
    for v in counts:
        counts[v]["n_pairs"] = 1
    return dist, [list(o) for o in ops], partner, counts, {"n_scripts": 1, "n_beyond": 0, "n_ops": dist, "n_unknown": 0}


def expectations(by):
    S, D, I = AR.SUB, AR.DEL, AR.INS
    a_, b_, x_, g_ = ord("a"), ord("b"), ord("x"), ord("g")
    c = by["abab-baba"]
    assert c["ops"] == [[0, 0, I], [3, 4, D]] and c["partner"] == [1, 0]
    assert c["counts"] == {str(b_): dict(zip(FIELDS, [0, 1, 0, 0, 0, 0, 1, 0, 4]))}  # a is untouched
    c = by["abcde-bcdex"]
    assert c["partner"] == [None, None] and c["counts"][str(a_)]["dropped"] == 1 and c["counts"][str(x_)]["extra"] == 1
    c = by["ab-ba"]
    assert [o[2] for o in c["ops"]] == [S, S]
    for v in (a_, b_):
        assert [c["counts"][str(v)][f] for f in ("sub_from", "sub_to", "n_pairs")] == [1, 1, 1]
    c = by["kitten-sitting"]
    assert c["counts"][str(g_)]["extra"] == 1
    assert c["counts"][str(ord("k"))]["sub_from"] == 1 and c["counts"][str(ord("s"))]["sub_to"] == 1
    assert c["counts"][str(ord("e"))]["sub_from"] == 1 and c["counts"][str(ord("i"))]["sub_to"] == 1
    assert by["kitten-sitting-beyond"]["ops"] is None
    for r, w in ((32, 64), (31, 63), (16, 32), (15, 31)):
        c = by[f"rot{r}-w{w}"]
        assert c["dist"] == 2 * r and [o[2] for o in c["ops"]] == [D] * r + [I] * r
        assert c["partner"] == [s + r for s in range(r)] + list(range(r))
        assert c["counts"][str(X)]["later"] == r and c["counts"][str(X)]["earlier"] == 0
        c = by[f"rot{r}-w{w}-rev"]
        assert [o[2] for o in c["ops"]] == [I] * r + [D] * r
        assert c["counts"][str(X)]["earlier"] == r and c["counts"][str(X)]["later"] == 0
    c = by["xy16-w64"]
    assert c["dist"] == 64 and c["partner"][0] == 48 and c["partner"][63] == 15
    c = by["x34-x30-w64"]
    assert c["dist"] == 64 and c["counts"][str(X)]["later"] == 30 and c["counts"][str(X)]["dropped"] == 4
    c = by["x30-x34-w64"]
    assert c["dist"] == 64 and c["counts"][str(X)]["later"] == 30 and c["counts"][str(X)]["extra"] == 4
    assert c["ops"][63][2] == I and c["partner"][63] is None


def main():
    out = []
    for name, a, b, w in CASES:
        dist, ops, partner, counts, info = kat(a, b, w)
        out.append({"name": name, "a": a, "b": b, "band": w, "dist": dist, "ops": ops, "partner": partner,
                    "counts": {str(v): counts[v] for v in sorted(counts)}, "info": info})
    expectations({c["name"]: c for c in out})
    with open(os.path.join(HERE, "move_profile_kat.json"), "w") as f:
        f.write("[\n" + ",\n".join("  " + json.dumps(c) for c in out) + "\n]\n")


if __name__ == "__main__":
    main()
