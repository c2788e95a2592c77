"""K1's rank-block planes restated on the host (tools/wt_sim.py build_planes / query_planes) against per-event
decisions: counts from two planes and a mask, predecessors by the lifting search over blocks. A design check of the
plane form of replayable_wt_plan.hip (build) and replayable_wt.hip (queries), CPU only. Sizes: no block boundary inside the segment (one block), a last block of
one rank or none, more than one 32-position word, 64 blocks (the deepest search); moduli that force ties and wholly
wrapping parts (3) and sums past 2^32."""
import os
import random
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

import wt_sim  # noqa: E402


def test_wt_sim_planes():
    rng = random.Random(12)
    for n in (9, 63, 64, 65, 127, 128, 129, 300, 1030, 4095):
        for m in (3, 1000, (1 << 31) + 5, (1 << 32) - 1):
            cm = [rng.randrange(m) for _ in range(n)]
            e = rng.sample(range(4096), n)
            img = wt_sim.build_planes(cm, e, [0] * n)
            srt = sorted(cm)
            edges = [0, n] + [r for b in range(64, n + 1, 64) for r in (b - 1, b, b + 1) if r <= n]
            # bounds whose ranks R_A / R_B sit at 0, n and the block edges, then random ones
            fixed = [(srt[r] if r < n else m) for r in edges]
            cases = [(d, x, y) for d in (0, n, rng.randrange(n + 1)) for x in fixed[:6] for y in fixed[-6:]]
            cases += [(rng.choice([0, n, rng.randrange(n + 1)]), rng.randrange(m) + 1, rng.randrange(m) + 1)
                      for _ in range(16 if n < 4000 else 6)]
            for d, XA, XB in cases:
                XA, XB = max(1, min(XA, m)), max(1, min(XB, m))  # X = m - Hm in [1, m]
                Hm, Hm2 = m - XA, m - XB
                RA = sum(1 for x in cm if x < XA)
                RB = sum(1 for x in cm if x < XB)
                bW, bk = wt_sim.brute(cm, e, d, Hm, Hm2, m)
                W, kA, kB = wt_sim.query_planes(img, d, RA, RB, Hm, Hm2, m)
                assert W == bW, (n, m, d, RA, RB)
                assert max(x for x in (kA, kB) if x is not None) == bk, (n, m, d, RA, RB)
