"""The PO k-NN search's filter and lists by the definition, in pure Python ints (not a test module).

DESIGN.md section 2, "PO k-NN search": the 256-byte profile of a trace's projection (lenfold[32], gram[128]), the two
lower bounds of a pair, and the k-NN lists over a distance matrix. Nothing from the library; the host form
nmz_po_knn_bound_host is tied to this in tests/test_po_knn_host.py, and the GPU tests compare with the host forms."""
import numpy as np

NONE = 0xFFFFFFFF
M64 = (1 << 64) - 1
START = 0x9E3779B97F4A7C15


def mix(x):
    """The splitmix64 finaliser, mod 2^64."""
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def bucket(g, prev, cur):
    return mix(mix((prev + g) & M64) ^ cur) >> 57


def profile(t, ent):
    """(lenfold[32], gram[128]) of trace t with entities ent; gram saturates at 255."""
    lenfold, gram, last = [0] * 32, [0] * 128, {}
    for x, g in zip(t, ent):
        x, g = int(x), int(g)
        if g == NONE:
            continue
        lenfold[g % 32] += 1
        gram[bucket(g, last.get(g, START), x)] += 1
        last[g] = x
    return lenfold, [min(c, 255) for c in gram]


def bounds_of(pa, pb):
    """(LB_len, LB_gram) of two profiles."""
    lb_len = sum(abs(x - y) for x, y in zip(pa[0], pb[0]))
    lb_gram = (sum(abs(x - y) for x, y in zip(pa[1], pb[1])) + 3) // 4
    return lb_len, lb_gram


def bounds(a, ea, b, eb):
    return bounds_of(profile(a, ea), profile(b, eb))


def length_sum(ea, eb):
    """sum over the entities of ||a|g| - |b|g||: the exact bound the search takes before any DP."""
    ca, cb = {}, {}
    for c, e in ((ca, ea), (cb, eb)):
        for g in e:
            g = int(g)
            if g != NONE:
                c[g] = c.get(g, 0) + 1
    return sum(abs(ca.get(g, 0) - cb.get(g, 0)) for g in set(ca) | set(cb))


def knn(D, k, q_self=None):
    """(ids [Q, k], dists [Q, k]) over the distance matrix D[Q][N] by (distance asc, id asc), the store index
    q_self[q] skipped (NONE or q_self None: nothing), NONE / NONE past the eligible stored traces."""
    D = np.asarray(D, np.uint32)
    Q, N = D.shape
    ids = np.full((Q, k), NONE, np.uint32)
    ds = np.full((Q, k), NONE, np.uint32)
    for q in range(Q):
        order = np.lexsort((np.arange(N), D[q]))
        if q_self is not None and int(q_self[q]) != NONE:
            order = order[order != int(q_self[q])]
        order = order[:k]
        ids[q, :len(order)] = order
        ds[q, :len(order)] = D[q, order]
    return ids, ds
