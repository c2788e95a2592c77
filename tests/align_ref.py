"""The canonical edit script from a plain Levenshtein matrix, in pure Python (not a test module).

Lists and ints only, no numpy arithmetic: the reference the host form (nmz_ed_align_host) is tied to, which in turn
is what the GPU tests compare with. `script` follows DESIGN.md section 2 ("Edit scripts") literally: the unit-cost
matrix D, then from (n, m) back to (0, 0) the first move that applies of diagonal, up, left. `band=w` restricts the
matrix to the cells |i - j| <= w (+inf outside), which yields the same script whenever Lev <= w (the section's
argument; tests/test_align_host.py checks it on whole families) at a fraction of the cells. `prefer` reorders the
walk's preferences, for counting the pairs on which the tie rule decides."""
SUB, DEL, INS = 0, 1, 2
INF = 1 << 60


def matrix(a, b, band=None):
    """D as a list of rows; with a band, cells outside it hold INF."""
    a, b = [int(x) for x in a], [int(x) for x in b]
    n, m = len(a), len(b)
    D = [[INF] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        lo, hi = (0, m) if band is None else (max(0, i - band), min(m, i + band))
        row, up = D[i], D[i - 1] if i else None
        for j in range(lo, hi + 1):
            if i == 0:
                row[j] = j
                continue
            if j == 0:
                row[j] = i
                continue
            v = up[j - 1] + (a[i - 1] != b[j - 1])
            if up[j] + 1 < v:
                v = up[j] + 1
            if row[j - 1] + 1 < v:
                v = row[j - 1] + 1
            row[j] = v
    return D


def walk(a, b, D, prefer=("diag", "up", "left")):
    """The ops [(a_pos, b_pos, kind)] in forward order, and the cells (i, j) the ops landed on."""
    i, j = len(a), len(b)
    ops, cells = [], []
    while i > 0 or j > 0:
        cur = D[i][j]
        ok = {
            "diag": i > 0 and j > 0 and D[i - 1][j - 1] + (int(a[i - 1]) != int(b[j - 1])) == cur,
            "up": i > 0 and D[i - 1][j] + 1 == cur,
            "left": j > 0 and D[i][j - 1] + 1 == cur,
        }
        move = next((p for p in prefer[:-1] if ok[p]), prefer[-1])
        assert ok[move], "no move explains the cell"
        if move == "diag":
            if int(a[i - 1]) != int(b[j - 1]):
                ops.append((i - 1, j - 1, SUB))
                cells.append((i, j))
            i, j = i - 1, j - 1
        elif move == "up":
            ops.append((i - 1, j, DEL))
            cells.append((i, j))
            i -= 1
        else:
            ops.append((i, j - 1, INS))
            cells.append((i, j))
            j -= 1
    return ops[::-1], cells[::-1]


def script(a, b, w, band=None, prefer=("diag", "up", "left"), want_cells=False):
    """(dist, ops): dist = min(Lev(a, b), w + 1); ops = the canonical script, or None when dist == w + 1."""
    if abs(len(a) - len(b)) > w:
        return (w + 1, None, None) if want_cells else (w + 1, None)
    D = matrix(a, b, band)
    d = min(D[len(a)][len(b)], w + 1)
    if d > w:
        return (d, None, None) if want_cells else (d, None)
    ops, cells = walk(a, b, D, prefer)
    assert len(ops) == d
    return (d, ops, cells) if want_cells else (d, ops)


def replay(a, b, ops):
    """Walk the implied matches and the ops: True iff they land on (n, m), every implied match is equal and every
    SUB is unequal."""
    i = j = 0
    n, m = len(a), len(b)
    for ap, bp, kind in ops:
        ap, bp, kind = int(ap), int(bp), int(kind)
        while i < ap and j < bp:  # the matches before the op
            if int(a[i]) != int(b[j]):
                return False
            i, j = i + 1, j + 1
        if (i, j) != (ap, bp):
            return False
        if kind == SUB:
            if i >= n or j >= m or int(a[i]) == int(b[j]):
                return False
            i, j = i + 1, j + 1
        elif kind == DEL:
            if i >= n:
                return False
            i += 1
        elif kind == INS:
            if j >= m:
                return False
            j += 1
        else:
            return False
    while i < n and j < m:
        if int(a[i]) != int(b[j]):
            return False
        i, j = i + 1, j + 1
    return (i, j) == (n, m)


def as_tuples(ops):
    """A structured ops array (a_pos, b_pos, kind) as a list of int tuples."""
    return [(int(o["a_pos"]), int(o["b_pos"]), int(o["kind"])) for o in ops]
