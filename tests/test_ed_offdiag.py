"""The off-diagonal edit-distance families (tests/ed_cases.py) on the CPU: every case that
tests/test_ed_offdiag_gpu.py compares on the GPU must exercise what it is there for -- pairs in band, pairs beyond
the band that still pass the length filter, in-band pairs whose optimal path leaves the main diagonal, and pairs on
the band edge (|n - m| = w) in both roles. All counts come from the oracle alone. The oracle itself is checked on
the same families against the pure-Python Levenshtein and the families' closed forms.

Counts are over ordered pairs (query, candidate), query != candidate: the kernels are asymmetric (the query is the
rows), and the GPU test runs every store in both orders, so each ordered pair is compared."""
import numpy as np
import pytest

import ed_cases as C
from oracle import oracle as O

SMALL = [n for n in C.CASES if max(len(t) for t in C.traces(n)) <= 400 and n != "bv-3fam"]  # base length <= 300


def _first_family(name):
    """(traces, oracle matrix) of a case, of its first family where the store holds several."""
    trs, D = C.traces(name), C.reference(name)
    n = len(trs) // C.FAMILIES.get(name, 1)
    return trs[:n], D[:n, :n]


@pytest.mark.parametrize("name", list(C.CASES))
def test_case_is_not_vacuous(name):
    s = C.stats(name)
    print(name, s)
    if name in C.FEW_FAR:  # periodic and generic cases: few pairs beyond the band by nature
        assert s["half_diagonal"] >= 4
        return
    assert s["in_band"] >= 0.25 * s["pairs"]  # in a store of several families: of the pairs inside a family
    assert s["far_in_length_band"] >= 0.20 * s["pairs"]
    assert s["half_diagonal"] >= 0.25 * s["in_band_pos"]
    assert s["edge_longer_query"] + s["edge_longer_candidate"] >= 10
    assert s["edge_longer_query"] >= 4 and s["edge_longer_candidate"] >= 4


def test_three_family_store_crosses_a_query_block():
    trs = C.traces("bv-3fam")
    D = C.reference("bv-3fam")
    assert len(trs) >= 65
    assert (D[:64, 64:] <= 32).any()  # in-band pairs with the query in block 0 and the candidate in block 1


def test_trimmed_families_keep_the_band_edge_members():
    for name, n_max in (("wide-w4096", 14), ("wide-w8192", 10)):
        w = C.band(name)
        trs = C.traces(name)
        assert len(trs) <= n_max
        L = len(trs[0])
        lens = [len(t) for t in trs]
        for want in (L + w - 1, L + w, L + w + 1, L - w):  # F_{w-1} / F_w / F_{w+1} + a and a[w:]
            assert want in lens
        assert lens.count(L) >= 5  # a, both shifts, the rotation, the offset block


@pytest.mark.parametrize("name", SMALL)
def test_oracle_matrix_symmetric_and_equal_to_full_levenshtein(name):
    """On the short families the banded oracle is min(full Levenshtein, w + 1) for every ordered pair (the C
    oracle's full DP), and symmetric -- which the mirrored references of the widest bands rely on."""
    (trs, D), w = _first_family(name), C.band(name)
    n = len(trs)
    assert np.array_equal(C.reference(name), C.reference(name).T)
    full = np.array([[min(O.levenshtein(trs[i], trs[j]), w + 1) for j in range(n)] for i in range(n)])
    assert np.array_equal(D, full)


@pytest.mark.parametrize("name", SMALL)
def test_oracle_banded_vs_python_levenshtein(name):
    """O.levenshtein_banded == min(O.levenshtein_py, w + 1): the base against every member in both roles on the
    shortest families, against every fourth member on the longer ones (the Python DP is quadratic)."""
    (trs, _), w = _first_family(name), C.band(name)
    step = 1 if len(trs[0]) <= 130 else 4
    for j in range(1, len(trs), step):
        for x, y in ((trs[0], trs[j]), (trs[j], trs[0])):
            assert O.levenshtein_banded(x, y, w) == min(O.levenshtein_py(list(x), list(y)), w + 1), (name, j)


@pytest.mark.parametrize("name,L,alphabet,seed", [("bv-w8", 70, 6, 108), ("bv-w16", 130, 20, 116),
                                                  ("bv-w32", 200, 12, 132), ("bv-w64", 300, 16, 164),
                                                  ("bv-w5", 100, 4, 105), ("bv-w33", 200, 12, 133),
                                                  ("bv-w50", 260, 12, 150), ("tile-w16", 300, 3000, 216),
                                                  ("generic-w9000", 120, 12, 400)])
def test_oracle_closed_forms(name, L, alphabet, seed):
    """d(F_d + a, a) = d and d(a[d:], a) = d for d <= w (w + 1 beyond), d(a + F_d, a) = d on the diagonal, and the
    shift's bound d(a[d:] + F_d, a) <= 2d (so in band at d = w / 2)."""
    w = C.band(name)
    kw = {"distinct": True} if name.startswith("tile") else {"shifts": (1, 5, 20)} if name.startswith("generic") else {}
    fam = dict(C.named_family(L, alphabet, w, np.random.default_rng(seed), **kw))
    assert all(np.array_equal(x, y) for x, y in zip(fam.values(), C.traces(name)))  # the case's (first) family
    a = fam["a"]
    seen = set()
    for nm, t in fam.items():
        for pre, post in (("F", "+a"), ("a[", ":]"), ("a+F", "")):
            if nm.startswith(pre) and nm.endswith(post) and nm[len(pre):len(nm) - len(post)].isdigit():
                d = int(nm[len(pre):len(nm) - len(post)])
                assert O.levenshtein_banded(t, a, w) == min(d, w + 1) == O.levenshtein_banded(a, t, w), nm
                seen.add(d)
        if nm.startswith("shift"):
            d = int(nm[5:])
            assert O.levenshtein(t, a) <= 2 * d
            assert O.levenshtein_banded(t, a, w) == min(O.levenshtein(t, a), w + 1)
            if 2 * d <= w:
                assert O.levenshtein_banded(t, a, w) <= w
    assert seen >= ({1, 5, 20} if name.startswith("generic") else {1, w // 2, w - 1, w, w + 1})


def test_shift_sets_land_on_the_layout_joints():
    """d = 0, +-1 mod 32 for the bit-parallel words and mod 32 * KL for the wide kernel's lanes, wherever such a d
    fits below w + 1."""
    for w, unit in ((8, 32), (32, 32), (33, 32), (50, 32), (64, 32), (100, 32), (1024, 32), (2048, 64),
                    (4096, 128), (8192, 256)):
        ds = C.shifts_for(w, unit)
        assert {1, w // 2, w - 1, w, w + 1} <= set(ds) and max(ds) == w + 1 and min(ds) == 1
        if unit <= w + 1:
            assert {d % unit for d in ds} >= {0, 1, unit - 1}
            assert {unit - 1, unit, unit + 1} & set(range(1, w + 2)) <= set(ds)


def test_knn_from_matches_the_oracles_knn():
    """knn_from (lists of any store order out of the ordered-pair matrix) against O.ed_allpairs_knn on the store
    as built and reversed."""
    name = "bv-w16"
    trs, D, w = C.traces(name), C.reference(name), C.band(name)
    n = len(trs)
    for order in (np.arange(n), np.arange(n)[::-1]):
        off, sym = C.csr([trs[i] for i in order])
        oi, od = O.ed_allpairs_knn(off, sym, w, n - 1)
        ki, kd = C.knn_from(D, order, n - 1)
        assert np.array_equal(oi, ki) and np.array_equal(od, kd)
