"""Edit scripts per entity by the definition, in pure Python (not a test module).

DESIGN.md section 2, "Edit scripts per entity", restated over tests/align_ref.py: project both traces onto every
entity, take align_ref.script per entity, lift the positions back to the whole traces, concatenate in ascending
entity id. Lists and ints only, nothing from the library. The profile of a PO script is moves_ref's over the lifted
ops. The host form (nmz_ed_align_po_host) is tied to this in tests/test_align_po_host.py, and the GPU tests compare
with the host form."""
import align_ref as AR
import moves_ref as MR

NONE = 0xFFFFFFFF


def project(t, ent):
    """{g: (t|g, src_g(t))} over the entities of t, elements with entity NONE skipped."""
    out = {}
    for i, (x, g) in enumerate(zip(t, ent)):
        g = int(g)
        if g != NONE:
            seq, src = out.setdefault(g, ([], []))
            seq.append(int(x))
            src.append(i)
    return out


def script(a, ea, b, eb, w):
    """(dist, ops): dist = min(sum_g Lev(a|g, b|g), w + 1); ops = the lifted scripts in entity order, or None when
    dist == w + 1."""
    pa, pb = project(a, ea), project(b, eb)
    total, ops = 0, []
    for g in sorted(set(pa) | set(pb)):
        ag, sa = pa.get(g, ([], []))
        bg, sb = pb.get(g, ([], []))
        d, sc = AR.script(ag, bg, w, band=w)
        if sc is None:
            return w + 1, None
        total += d
        ops += [(sa[ap] if ap < len(sa) else len(a), sb[bp] if bp < len(sb) else len(b), kind) for ap, bp, kind in sc]
    if total > w:
        return w + 1, None
    return total, ops


def equal_in_po(a, ea, b, eb):
    """tracesEqualInPO over the projections: the same entities, and per entity the same sequence."""
    pa, pb = project(a, ea), project(b, eb)
    return {g: seq for g, (seq, _) in pa.items()} == {g: seq for g, (seq, _) in pb.items()}


def profile(traces, entities, pairs, w, table=None):
    """moves_ref.profile over the PO scripts of `pairs`."""
    scripts = {(i, j): script(traces[i], entities[i], traces[j], entities[j], w) for i, j in pairs}
    return MR.profile(traces, pairs, w, table=table, scripts=scripts)
