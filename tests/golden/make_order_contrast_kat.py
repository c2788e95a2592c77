"""Writes order_contrast_kat.json: a few small pos / failed tables with every ordered pair's F, P and score and the
ranked list of the pairs with score > 0, by the definition ("Order contrast").

Plain Python loops only -- no numpy and no library; the JSON is written by hand too (`os` only finds the directory)
-- so the known answers share nothing with the library or with tests/contrast_ref.py.

    python tests/golden/make_order_contrast_kat.py
"""
NONE = 0xFFFFFFFF


def lcg(state):
    return (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)


def table(E, R, seed, absent_of_16, equal_every):
    """R shuffled rows of positions 5 * i + 2; a cell absent when its draw's top 4 bits are below absent_of_16;
    every equal_every-th row repeats a position (two events at one position); labels alternate with a twist."""
    s = seed
    pos, failed = [], []
    for r in range(R):
        row = [5 * i + 2 for i in range(E)]
        for i in range(E - 1, 0, -1):  # Fisher-Yates
            s = lcg(s)
            j = (s >> 33) % (i + 1)
            row[i], row[j] = row[j], row[i]
        for i in range(E):
            s = lcg(s)
            if (s >> 60) < absent_of_16:
                row[i] = NONE
        if equal_every and r % equal_every == equal_every - 1 and E >= 2:
            row[1] = row[0]
        pos.append(row)
        s = lcg(s)
        failed.append(1 if (r % 3 == 0) != ((s >> 40) % 5 == 0) else 0)
    if 1 not in failed:
        failed[0] = 1
    if 0 not in failed:
        failed[-1] = 0
    return pos, failed


def solve(pos, failed):
    R, E = len(pos), len(pos[0])
    n_fail = 0
    for f in failed:
        n_fail += f
    n_pass = R - n_fail
    F = [[0] * E for _ in range(E)]
    P = [[0] * E for _ in range(E)]
    for r in range(R):
        for b in range(E):
            for a in range(E):
                if b == a or pos[r][b] == NONE or pos[r][a] == NONE:
                    continue
                if pos[r][b] < pos[r][a]:
                    if failed[r]:
                        F[b][a] += 1
                    else:
                        P[b][a] += 1
    score = [[F[b][a] * n_pass - P[b][a] * n_fail for a in range(E)] for b in range(E)]
    listed = []
    for b in range(E):
        for a in range(E):
            if b != a and score[b][a] > 0:
                listed.append((-score[b][a], -F[b][a], b * E + a))
    listed.sort()
    ranked = []
    for _, _, i in listed:
        b, a = i // E, i % E
        ranked.append([b, a, score[b][a], F[b][a], P[b][a], F[a][b], P[a][b]])
    return n_fail, n_pass, F, P, score, ranked


def fmt(v, indent):
    """JSON of nested lists of ints and dicts with string keys."""
    if isinstance(v, dict):
        inner = (",\n" + " " * (indent + 1)).join('"%s": %s' % (k, fmt(x, indent + 1)) for k, x in v.items())
        return "{\n" + " " * (indent + 1) + inner + "\n" + " " * indent + "}"
    if isinstance(v, list):
        if v and isinstance(v[0], (list, dict)):
            return "[" + (",\n" + " " * (indent + 1)).join(fmt(x, indent + 1) for x in v) + "]"
        return "[" + ", ".join(str(x) for x in v) + "]"
    return str(v)


def main():
    cases = []
    # (E, R, seed, absent of 16, a repeated position every n-th row)
    for E, R, seed, ab, eq in [(2, 2, 1, 0, 0), (3, 5, 2, 0, 2), (5, 7, 3, 3, 0), (6, 9, 4, 4, 3), (9, 12, 5, 2, 4),
                               (4, 3, 6, 8, 0)]:
        pos, failed = table(E, R, seed, ab, eq)
        n_fail, n_pass, F, P, score, ranked = solve(pos, failed)
        cases.append({"n_events": E, "n_runs": R, "pos": pos, "failed": failed, "n_fail": n_fail, "n_pass": n_pass,
                      "F": F, "P": P, "score": score, "ranked": ranked})
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "order_contrast_kat.json"), "w") as f:
        f.write(fmt({"cases": cases}, 0) + "\n")


if __name__ == "__main__":
    main()
