"""Writes edit_script_kat.json: small string pairs with their banded distance and canonical edit script, by the
definition ("Edit scripts").

A plain (n + 1) x (m + 1) matrix of Python ints and the walk -- no numpy, no library, nothing from
tests/align_ref.py -- so the known answers share nothing with the code they check. Symbols are the characters'
code points; ops are [a_pos, b_pos, kind] with kind 0 = SUB, 1 = DEL, 2 = INS; "script": null = beyond the band.

    python tests/golden/make_edit_script_kat.py
"""
import json
import os

CASES = [("kitten", "sitting", 3), ("kitten", "sitting", 2), ("abc", "", 3), ("", "ab", 2), ("ab", "ba", 2),
         ("aab", "ab", 1), ("ab", "aab", 1), ("abcde", "bcdex", 2), ("abab", "baba", 2), ("aaaa", "aa", 2),
         ("", "", 0), ("", "", 3), ("abc", "abc", 0), ("abc", "abd", 0), ("abc", "abd", 1), ("abc", "ab", 0),
         ("sunday", "saturday", 3), ("sunday", "saturday", 2), ("intention", "execution", 5),
         ("intention", "execution", 4), ("abcabcabc", "bcabcabca", 2), ("xabcdefgh", "abcdefghx", 2),
         ("aaaaaaaa", "aaaa", 4), ("aaaa", "aaaaaaaa", 4), ("aaaaaaaa", "aaaa", 3), ("abcdefgh", "hgfedcba", 8)]


def kat(a, b, w):
    n, m = len(a), len(b)
    D = [[0] * (m + 1) for _ in range(n + 1)]
    for i in range(n + 1):
        for j in range(m + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j - 1] + (a[i - 1] != b[j - 1]), D[i - 1][j] + 1, D[i][j - 1] + 1)
    dist = min(D[n][m], w + 1)
    if dist > w:
        return dist, None
    i, j, ops = n, m, []
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i - 1][j - 1] + (a[i - 1] != b[j - 1]) == D[i][j]:
            if a[i - 1] != b[j - 1]:
                ops.append([i - 1, j - 1, 0])
            i, j = i - 1, j - 1
        elif i > 0 and D[i - 1][j] + 1 == D[i][j]:
            ops.append([i - 1, j, 1])
            i -= 1
        else:
            ops.append([i, j - 1, 2])
            j -= 1
    return dist, ops[::-1]


def main():
    out = []
    for a, b, w in CASES:
        dist, ops = kat(a, b, w)
        out.append({"a": a, "b": b, "band": w, "dist": dist, "script": ops})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "edit_script_kat.json")
    with open(path, "w") as f:
        f.write("[\n" + ",\n".join("  " + json.dumps(c) for c in out) + "\n]\n")


if __name__ == "__main__":
    main()
