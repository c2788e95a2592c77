"""HistoryStorage surface with GPU similarity search behind it.

Mirrors nmz/historystorage:
  * HistoryStorage interface, New(name, dir), LoadStorage(dir)
        historystorage/historystorage.go:33-83
  * Naive storage layout %08x/actions/N.{action,event}.json, result.json
        historystorage/naive/naive.go:82-233, naive/common.go:24-40
  * Search / SearchWithConverter (exact equality of the converted sequence,
    the latest trace excluded)         naive/naive.go:235-257
and adds the optional SimilaritySearcher interface: banded edit
distance k-NN over event-hash sequences, plus the `nmz tools visualize`
unique-trace count (cli/tools/visualize.go:51-172), exact and partial-order
reduced. The gob-encoded `history`/`SearchModeInfo` files are not read; the
per-action JSON files (naive.go:65-80) carry the same actions and events.

Two symbol streams per stored trace (build-defined), each the FNV-1a
64 of a canonical JSON (Go encoding/json form, namazu_amd/signal.py):
  * action symbols: the action's map without "uuid" -- Action.Equals
    (BasicSignal.EqualsSignal ignores only uuid and arrival time, signal.go:174-186),
    so "event_uuid" counts wherever the layout puts it (top level since
    action_accept_event.go:40; under "option" in the 2015 example traces).
    Search / SearchWithConverter and the exact unique count compare these
    (AreActionsSliceEqual, util/signal/misc.go:22-35). Actions of different runs
    carry different event uuids, so -- as in the reference -- they never match.
  * event symbols: the action's event without "uuid" -- Event.Equals. The
    similarity search (SearchSimilar, AllPairsKNN) and the partial-order unique
    count compare these; an action without an event file uses its action symbol
    there, and has no entity (skipped by the PO projection, visualize.go:67-76).
Every comparison runs in libnmz_gpu.so.
"""
import ctypes
import glob
import json
import os
import re

import numpy as np

from . import _lib
from .config import Config
from .signal import Event, fnv1a64, go_json

STORAGE_TOML = "config.toml"  # historystorage.go:28


class SingleTrace:
    """util/trace.SingleTrace: the stored action sequence.

    symbols         event symbols (Event.Equals; SimilaritySearcher)
    action_symbols  action symbols (Action.Equals; Equals, Search) -- default: symbols
    entities        EntityID() of each action's event, None for an action without one
    events          the events (signal.Event) or None"""

    def __init__(self, symbols, events=None, action_symbols=None, entities=None):
        self.symbols = np.asarray(symbols, np.uint64)
        self.events = events or []
        self.action_symbols = self.symbols if action_symbols is None else np.asarray(action_symbols, np.uint64)
        self.entities = entities if entities is not None else [None] * len(self.symbols)

    def __len__(self):
        return len(self.symbols)

    def Equals(self, other):
        """trace.go:29-31 -> AreActionsSliceEqual (misc.go:22-35): equal length, element-wise Action.Equals."""
        return len(self.action_symbols) == len(other.action_symbols) and \
            bool(np.array_equal(self.action_symbols, other.action_symbols))


def action_symbol(action_json):
    """Symbol of an action map: FNV-1a 64 of its canonical JSON without "uuid" (EqualsSignal keeps every
    other key, including "event_uuid" at whichever level it is stored)."""
    return fnv1a64(go_json({k: v for k, v in action_json.items() if k != "uuid"}).encode())


def action_symbols(actions):
    """[]Action (signal.Action objects or JSON maps) -> uint64 action symbols."""
    return np.array([action_symbol(a.JSONMap() if hasattr(a, "JSONMap") else a) for a in actions], np.uint64)


class TraceSet:
    """CSR of event-hash sequences, the layout the GPU kernels consume."""

    def __init__(self, traces):
        self.off = np.zeros(len(traces) + 1, np.uint64)
        if traces:
            self.off[1:] = np.cumsum([len(t) for t in traces])
        self.sym = (np.concatenate([np.asarray(t, np.uint64) for t in traces])
                    if self.off[-1] else np.zeros(1, np.uint64))

    def __len__(self):
        return len(self.off) - 1

    def trace(self, i):
        return self.sym[int(self.off[i]):int(self.off[i + 1])]


class HistoryStorage:
    def Name(self):
        raise NotImplementedError


class Naive(HistoryStorage):
    """Reader for the naive storage directory layout."""

    def __init__(self, dir_path):
        self.dir = dir_path
        self._ids = None

    def Name(self):
        return "naive"

    def Init(self):
        ids = []
        for p in glob.glob(os.path.join(self.dir, "*")):
            b = os.path.basename(p)
            if os.path.isdir(p) and re.fullmatch(r"[0-9a-f]{8}", b):
                ids.append(int(b, 16))
        self._ids = sorted(ids)

    def NrStoredHistories(self):
        if self._ids is None:
            self.Init()
        return len(self._ids)

    def _run_dir(self, i):
        return os.path.join(self.dir, "%08x" % i)

    def GetStoredHistory(self, i):
        """Returns (SingleTrace, error) like the Go getter."""
        adir = os.path.join(self._run_dir(i), "actions")
        if not os.path.isdir(adir):
            return None, FileNotFoundError(adir)
        idx = sorted(int(m.group(1)) for f in os.listdir(adir)
                     if (m := re.fullmatch(r"(\d+)\.action\.json", f)))
        syms, asyms, ents, evs = [], [], [], []
        for n in idx:
            with open(os.path.join(adir, f"{n}.action.json")) as f:
                asym = action_symbol(json.load(f))
            asyms.append(asym)
            ep = os.path.join(adir, f"{n}.event.json")
            if os.path.exists(ep):  # recordAction writes it iff act.Event() != nil (naive.go:72-79)
                with open(ep) as f:
                    ev = Event.from_json(f.read())
                syms.append(ev.evhash())
                ents.append(ev.EntityID())
                evs.append(ev)
            else:
                syms.append(asym)
                ents.append(None)
                evs.append(None)
        return SingleTrace(syms, evs, action_symbols=asyms, entities=ents), None

    def IsSuccessful(self, i):
        try:
            return bool(json.load(open(os.path.join(self._run_dir(i), "result.json")))["successful"]), None
        except Exception as e:  # getters return errors (naive.go:199-213)
            return False, e

    def GetRequiredTime(self, i):
        try:
            return int(json.load(open(os.path.join(self._run_dir(i), "result.json")))["required_time"]), None
        except Exception as e:
            return 0, e

    def traces(self):
        out = []
        for i in range(self.NrStoredHistories()):
            t, err = self.GetStoredHistory(i)
            if err is not None:
                raise RuntimeError(f"failed to get history {i}: {err}")  # naive.go:241 panics
            out.append(t)
        return out

    def load_all(self):
        """Event-symbol TraceSet of every stored trace (the SimilaritySearcher's input)."""
        return TraceSet([t.symbols for t in self.traces()])

    # ---- search surface (GPU) ------------------------------------------------
    def SearchWithConverter(self, prefix, converter):
        """naive.go:235-252: ids i < NrStoredHistories-1 (the latest trace is excluded, :238) with
        len(trace) >= len(prefix) whose converted trace equals `prefix` under AreActionsSliceEqual
        (equal length, element-wise Action.Equals: action symbols). `prefix`: a SingleTrace, a list of
        actions (signal.Action or JSON maps), or action symbols; `converter`: SingleTrace -> SingleTrace
        (the reference's func([]Action) []Action)."""
        n = self.NrStoredHistories() - 1
        if n <= 0:
            return []
        if isinstance(prefix, SingleTrace):
            p = prefix.action_symbols
        elif len(prefix) and (hasattr(prefix[0], "JSONMap") or isinstance(prefix[0], dict)):
            p = action_symbols(prefix)
        else:
            p = np.asarray(prefix, np.uint64)
        cands = []
        for i in range(n):
            t, err = self.GetStoredHistory(i)
            if err is not None:
                raise RuntimeError(f"failed to get history {i}: {err}")
            if len(t) < len(p):
                continue
            cands.append((i, converter(t)))
        if not cands:
            return []
        ts = TraceSet([p] + [c.action_symbols for _, c in cands])
        pairs = np.array([[0, j + 1] for j in range(len(cands))], np.uint32)
        d = ed_pairs(ts, pairs, band=0)  # band 0: 0 iff equal length and element-wise equal
        return [cands[j][0] for j in range(len(cands)) if d[j] == 0]

    def Search(self, prefix):
        """naive.go:254-257: SearchWithConverter with the identity converter."""
        return self.SearchWithConverter(prefix, lambda t: t)

    def UniqueTraceCurve(self, po_reduction=True):
        """`nmz tools visualize -mode gnuplot` (visualize.go:138-172): nrUniques after each stored trace;
        po_reduction defaults to true as the flag does (:42)."""
        return unique_trace_curve(self.traces(), po_reduction=po_reduction)

    # ---- SimilaritySearcher ----------------------------------------------------
    def SearchSimilar(self, trace, k, band):
        """k nearest stored traces to `trace` by (distance asc, id asc), as [(id, distance)].

        The stored traces are read once and stay on the GPU (SimilarityIndex) until the storage holds a
        different number of traces; each query is one launch against the resident store."""
        t = trace.symbols if isinstance(trace, SingleTrace) else np.asarray(trace, np.uint64)
        n = self.NrStoredHistories()
        key = (band, n)
        if getattr(self, "_index_key", None) != key:
            if getattr(self, "_index", None) is not None:
                self._index.close()
            self._index = SimilarityIndex(self.load_all(), band)
            self._index_key = key
        ids, ds = self._index.query([t], k)
        return [(int(i), int(d)) for i, d in zip(ids[0], ds[0]) if i != _lib.NMZ_NONE]

    def AllPairsKNN(self, k, band):
        return allpairs_knn(self.load_all(), k, band)

    def SearchSimilarPO(self, trace, k, band):
        """SearchSimilar under the per-entity distance: the k nearest stored traces to `trace` (a SingleTrace carrying
        entities) by (ED^PO_band asc, id asc), as [(id, distance)]; a run that merely interleaved its independent
        entities differently is at 0. The stored runs are projected once and stay on the GPU (PoSimilarityIndex)
        until the storage holds a different number of traces. band <= 64 (the library refuses wider ones;
        SearchSimilarPOWide takes them)."""
        return self._search_similar_po(trace, k, band, wide=False)

    def SearchSimilarPOWide(self, trace, k, band):
        """SearchSimilarPO for every band 0 .. 1,024, through a wide PoSimilarityIndex (K11w above band 64)."""
        return self._search_similar_po(trace, k, band, wide=True)

    def _search_similar_po(self, trace, k, band, wide):
        if not isinstance(trace, SingleTrace):
            raise TypeError("SearchSimilarPO needs a SingleTrace carrying entities")
        n = self.NrStoredHistories()
        key = (band, n, wide)
        if getattr(self, "_po_index_key", None) != key:
            if getattr(self, "_po_index", None) is not None:
                self._po_index.close()
                self._po_index = None
            ts, ent, names = po_entities(self.traces())
            self._po_index = PoSimilarityIndex(ts, ent, band, names, wide=wide)
            self._po_index_key = key
        ids, ds = self._po_index.query([trace], k)
        return [(int(i), int(d)) for i, d in zip(ids[0], ds[0]) if i != _lib.NMZ_NONE]

    def DiffSimilar(self, trace, k, band, po=False, po_search=False):
        """SearchSimilar, then what differs: [(id, distance, script)] for the neighbours within the band, script the
        ops (EDIT_OP_DTYPE rows) that turn the stored run `id` into `trace` -- one edit_scripts call for all of them
        (edit_scripts_wide for 64 < band <= 1024). script_moves(stored, trace, script) names the events delivered
        earlier or later. po=True: the neighbours still come from the exact SearchSimilar at `band`, but distance and
        script are the per-entity ones (edit_scripts_po: interleavings of independent entities vanish); a neighbour
        whose ED^PO exceeds the band is left out. `trace` must then be a SingleTrace carrying entities.
        po_search=True (needs po=True): the neighbours come from SearchSimilarPO instead (SearchSimilarPOWide for
        64 < band <= 1024), so a run whose exact distance exceeds the band is found when its ED^PO is within it."""
        if po_search and not po:
            raise ValueError("po_search=True needs po=True: the PO search goes with the per-entity scripts")
        if po and not isinstance(trace, SingleTrace):
            raise TypeError("DiffSimilar(po=True) needs a SingleTrace carrying entities")
        t = trace.symbols if isinstance(trace, SingleTrace) else np.asarray(trace, np.uint64)
        search = self.SearchSimilar
        if po_search:
            search = self.SearchSimilarPO if band <= _lib.NMZ_PO_KNN_MAX_BAND else self.SearchSimilarPOWide
        near = [(i, d) for i, d in search(trace, k, band) if d <= band]
        if po:
            if not near:
                return []
            runs = []
            for i, _ in near:
                r, err = self.GetStoredHistory(i)
                if err is not None:
                    raise RuntimeError(f"failed to get history {i}: {err}")
                runs.append(r)
            ts, ent, names = po_entities(runs + [trace])
            pairs = np.array([[r, len(near)] for r in range(len(near))], np.uint32)
            es = edit_scripts_po(ts, ent, pairs, band, n_entities=max(len(names), 1),
                                 ctx=(self._po_index if po_search else self._index).ctx)
            return [(i, int(es.dist[r]), es.script(r).copy()) for r, (i, _) in enumerate(near) if es.dist[r] <= band]
        if not near:
            return []
        ts = TraceSet([self._index.ts.trace(i) for i, _ in near] + [t])
        pairs = np.array([[r, len(near)] for r in range(len(near))], np.uint32)
        align = edit_scripts if band <= _lib.NMZ_ALIGN_MAX_BAND else edit_scripts_wide
        es = align(ts, pairs, band, ctx=self._index.ctx)
        return [(i, d, es.script(r).copy()) for r, (i, d) in enumerate(near)]

    def DiffFailing(self, band, k=1, ctx=None, po=False, po_search=False):
        """Which events are delivered later, earlier, dropped or extra in this storage's failing runs, each measured
        against its k nearest passing runs (move_profile; move_profile_wide for 64 < band <= 1024). The runs are
        loaded and labelled as OrderContrast does it (IsSuccessful, naive.go:199-213; a run whose result cannot be
        read is skipped, cli/tools/summary.go:47-51). A
        SimilarityIndex over the passing runs answers the failing runs' queries; the pairs are (a = passing
        neighbour, b = failing run) for the neighbours within the band, so "later" reads "delivered later in the
        failing run". Returns the MoveProfile of one move_profile call, its .pairs the stored-run ids behind the
        pairs; .top(k) ranks the symbols. po=True: the neighbours still come from the exact search at `band`, the
        scripts and the profile are the per-entity ones (move_profile_po), so events of independent entities that
        merely interleaved differently are not counted; pairs with ED^PO > band count as beyond. po_search=True
        (needs po=True): a PoSimilarityIndex over the passing runs (a wide one for 64 < band <= 1024) answers the
        failing runs' queries, so the neighbours are the nearest passing runs by ED^PO, whatever their exact
        distance."""
        if po_search and not po:
            raise ValueError("po_search=True needs po=True: the PO search goes with the per-entity profile")
        passing, failing = [], []
        for i in range(self.NrStoredHistories()):
            ok, err = self.IsSuccessful(i)
            if err is not None:
                continue
            t, err = self.GetStoredHistory(i)
            if err is not None:
                raise RuntimeError(f"failed to get history {i}: {err}")  # naive.go:241 panics
            (passing if ok else failing).append((i, t))
        if not failing:
            raise ValueError("no failing run: nothing to contrast")
        if not passing:
            raise ValueError("no passing run: nothing to contrast")
        if po_search:
            pts, pent, pnames = po_entities([t for _, t in passing])
            index = PoSimilarityIndex(pts, pent, band, pnames, ctx=ctx, wide=band > _lib.NMZ_PO_KNN_MAX_BAND)
        else:
            index = SimilarityIndex(TraceSet([t.symbols for _, t in passing]), band, ctx=ctx)
        try:
            ids, ds = index.query([t if po_search else t.symbols for _, t in failing], int(k))
        finally:
            index.close()
        near = [(int(j), f) for f in range(len(failing)) for j, d in zip(ids[f], ds[f])
                if j != _lib.NMZ_NONE and d <= band]
        pairs = np.array([[j, len(passing) + f] for j, f in near], np.uint32).reshape(-1, 2)
        if po:
            ts, ent, names = po_entities([t for _, t in passing] + [t for _, t in failing])
            prof = move_profile_po(ts, ent, pairs, band, ctx=index.ctx, n_entities=max(len(names), 1))
        else:
            ts = TraceSet([t.symbols for _, t in passing] + [t.symbols for _, t in failing])
            profile = move_profile if band <= _lib.NMZ_ALIGN_MAX_BAND else move_profile_wide
            prof = profile(ts, pairs, band, ctx=index.ctx)
        prof.pairs = np.array([[passing[j][0], failing[f][0]] for j, f in near], np.uint32).reshape(-1, 2)
        return prof

    # ---- order contrast ----------------------------------------------------------
    def OrderContrast(self, sym, arrival_ns, k=64, want_counts=False, ctx=None):
        """The event pairs whose order separates this storage's failing runs from its passing ones
        (order_contrast). Every stored run is loaded and labelled with IsSuccessful (naive.go:199-213); a run whose
        result cannot be read is skipped, as `nmz tools summary` does (cli/tools/summary.go:47-51). (sym,
        arrival_ns) is the event universe: the trace whose hints the sweeps take. Returns a ContrastResult whose
        run_ids are the stored runs used, in row order. From the storage to a replay:

            c = storage.OrderContrast(sym, arrival_ns, k=64)
            cons = replay.constraints_from_pairs(c.pairs, 1_000_000, per_event=2)
            r = policy.OrderSweep(hints, arrival_ns, cons, seeds=seeds, k=8, want_stats=False)
            best = replay.replayable_seeds(r.topk, seeds)
            env = replay.replay_env(best[0], os.environ)                     # NMZ_REPLAY_SEED for `nmz run`
        """
        ids, runs, failed = [], [], []
        for i in range(self.NrStoredHistories()):
            ok, err = self.IsSuccessful(i)
            if err is not None:
                continue
            t, err = self.GetStoredHistory(i)
            if err is not None:
                raise RuntimeError(f"failed to get history {i}: {err}")  # naive.go:241 panics
            ids.append(i)
            runs.append(t)
            failed.append(0 if ok else 1)
        # the matching runs on the device too: equal by definition to order_contrast(run_positions(...), ...)
        c = order_contrast_runs(sym, arrival_ns, runs, np.array(failed, np.uint8), k=k, want_counts=want_counts,
                                ctx=ctx)
        c.run_ids = ids
        return c


def New(name, dir_path):
    """historystorage.go:54-62. Returns (storage, error)."""
    if name == "naive":
        return Naive(dir_path), None
    if name == "mongodb":
        return None, NotImplementedError("mongodb storage is out of scope (SURVEY 2 #8)")
    return None, ValueError(f"unknown history storage: {name}")


def LoadStorage(dir_path):
    """historystorage.go:64-83."""
    try:
        cfg = Config.from_file(os.path.join(dir_path, STORAGE_TOML))
    except Exception as e:
        print(f"error: {e}")
        return None
    if cfg.get("storageType") == "naive":
        return Naive(dir_path)
    print(f"unknown history storage: {cfg.get('storageType')}")
    return None


# ---- GPU entry points ----------------------------------------------------------
def ed_pairs(ts, pairs, band, ctx=None):
    ctx = ctx or _lib.default_context()
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    dist = np.zeros(len(pairs), np.uint32)
    _lib.check(_lib.load().nmz_ed_pairs(ctx.handle, _lib.ptr(ts.off), _lib.ptr(ts.sym), len(ts),
                                        _lib.ptr(pairs), len(pairs), int(band), _lib.ptr(dist)))
    return dist


class SimilarityIndex:
    """A stored TraceSet resident on the GPU for single-query similarity search (SearchSimilar).

    Every band and plan kind answers through one nmz_ed_plan_query_knn call over the resident store: the
    bit-parallel query kernel (band <= 64), the wide-band query kernel (64 < band <= 8,192: each query's match
    table built once per call, one wave per (query, stored trace)), or the resident generic kernel (other plans,
    queries whose symbols overflow the compact tables, and queries longer than every stored trace)."""

    def __init__(self, ts, band, ctx=None):
        import ctypes
        self.ctx = ctx or _lib.default_context()
        self.ts = ts
        self.band = int(band)
        self.plan = ctypes.c_void_p()
        L = _lib.load()
        _lib.check(L.nmz_ed_plan_create(self.ctx.handle, _lib.ptr(ts.off), _lib.ptr(ts.sym), len(ts), self.band,
                                        ctypes.byref(self.plan)))
        self.kind = {3: "wide", 2: "bitparallel", 1: "tile", 0: "generic"}[L.nmz_ed_plan_is_fast(self.plan)]
        self.bitparallel = self.kind == "bitparallel"

    def query(self, queries, k):
        """queries: event-symbol arrays -> (ids [n, k], dists [n, k]) by (ED_band asc, id asc), NMZ_NONE padded."""
        n, N = len(queries), len(self.ts)
        ids = np.full((n, k), _lib.NMZ_NONE, np.uint32)
        ds = np.full((n, k), _lib.NMZ_NONE, np.uint32)
        if n == 0 or N == 0 or k == 0:
            return ids, ds
        if k > 64:
            return self._query_pairs(queries, k)
        qset = TraceSet([np.asarray(q, np.uint64) for q in queries])
        _lib.check(_lib.load().nmz_ed_plan_query_knn(self.plan, _lib.ptr(qset.off), _lib.ptr(qset.sym), n, k,
                                                      _lib.ptr(ids), _lib.ptr(ds)))
        return ids, ds

    def _query_pairs(self, queries, k):
        """k > 64 (the resident kernels keep at most 64 per query; the reference's search has no cap,
        naive.go:235): every (query, stored trace) distance through nmz_ed_pairs on the GPU, one call per query,
        ordered by (distance, id) on the host."""
        n, N = len(queries), len(self.ts)
        kk = min(k, N)
        ids = np.full((n, k), _lib.NMZ_NONE, np.uint32)
        ds = np.full((n, k), _lib.NMZ_NONE, np.uint32)
        stored = [self.ts.trace(i) for i in range(N)]
        pairs = np.stack([np.zeros(N, np.uint32), np.arange(1, N + 1, dtype=np.uint32)], 1)
        for r, q in enumerate(queries):
            both = TraceSet([np.asarray(q, np.uint64)] + stored)
            d = ed_pairs(both, pairs, self.band, ctx=self.ctx)
            order = np.lexsort((np.arange(N), d))[:kk]
            ids[r, :kk] = order
            ds[r, :kk] = d[order]
        return ids, ds

    def close(self):
        if self.plan:
            _lib.load().nmz_ed_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def allpairs_knn(ts, k, band, ctx=None):
    ctx = ctx or _lib.default_context()
    n = len(ts)
    ids = np.zeros((n, k), np.uint32)
    ds = np.zeros((n, k), np.uint32)
    _lib.check(_lib.load().nmz_ed_allpairs_knn(ctx.handle, _lib.ptr(ts.off), _lib.ptr(ts.sym), n, int(band),
                                               int(k), _lib.ptr(ids), _lib.ptr(ds)))
    return ids, ds


def po_inputs(traces):
    """Partial-order projection inputs of SingleTraces: CSR of event symbols and per-element entity ids,
    dense per trace in order of first appearance (the kernel needs per-trace counters only: an event
    symbol already determines its entity), NMZ_NONE for actions without an event."""
    ts = TraceSet([t.symbols for t in traces])
    ent = np.full(max(int(ts.off[-1]), 1), _lib.NMZ_NONE, np.uint32)
    pos = 0
    for t in traces:
        ids = {}
        for e in t.entities:
            if e is not None:
                ent[pos] = ids.setdefault(e, len(ids))
            pos += 1
    return ts, ent


def first_equal(traces, po_reduction=True, ctx=None):
    """first_equal[i] = the smallest j with trace j equal to trace i (exact: Equals on action symbols;
    PO: tracesEqualInPO on per-entity event sequences), computed by nmz_unique_traces."""
    ctx = ctx or _lib.default_context()
    if isinstance(traces, TraceSet):
        ts, ent = traces, None
    elif po_reduction:
        ts, ent = po_inputs(traces)
    else:
        ts, ent = TraceSet([t.action_symbols for t in traces]), None
    n = len(ts)
    out = np.zeros(max(n, 1), np.uint32)
    _lib.check(_lib.load().nmz_unique_traces(ctx.handle, _lib.ptr(ts.off), _lib.ptr(ts.sym), _lib.ptr(ent), n,
                                             _lib.ptr(out)))
    return out[:n]


def trace_signatures(traces, po_reduction=True, ctx=None):
    """sig[len(traces)][2] uint64: the 128-bit equality signatures of SingleTraces (nmz_trace_signatures; exact:
    action symbols, PO: per-entity event sequences, as first_equal). Stored runs' signatures are the known_sigs of
    DeliveryResult.representatives / replay.distinct_order_seeds: a predicted delivery order with the same
    signature has already been explored."""
    ctx = ctx or _lib.default_context()
    if isinstance(traces, TraceSet):
        ts, ent = traces, None
    elif po_reduction:
        ts, ent = po_inputs(traces)
    else:
        ts, ent = TraceSet([t.action_symbols for t in traces]), None
    n = len(ts)
    sig = np.zeros((max(n, 1), 2), np.uint64)
    _lib.check(_lib.load().nmz_trace_signatures(ctx.handle, _lib.ptr(ts.off), _lib.ptr(ts.sym), _lib.ptr(ent), n,
                                                _lib.ptr(sig)))
    return sig[:n]


def unique_trace_curve(traces, po_reduction=True, ctx=None):
    """visualize.go gnuplot mode (:138-172): after trace i, how many distinct traces have been seen.
    traces: SingleTraces (exact or PO mode), or a TraceSet (exact mode over its symbols)."""
    fe = first_equal(traces, po_reduction, ctx)
    return list(np.cumsum(fe == np.arange(len(fe))).astype(int))


def match_target(sym, arrival_ns, recorded_sym):
    """target_pos[len(sym)] (uint32) of a trace's events against a recorded run's symbol sequence, the input of
    Replayable.NearestOrders: the i-th recorded occurrence of a symbol is matched to the i-th earliest-arriving
    event of the trace with that symbol (arrival ties go to the smaller index), and the event's target position is
    the occurrence's index in recorded_sym. Events without a recorded occurrence get NMZ_NONE; recorded occurrences
    without an event leave a hole (positions need not be dense). Pure numpy."""
    sym = np.asarray(sym, np.uint64).reshape(-1)
    rec = np.asarray(recorded_sym, np.uint64).reshape(-1)
    arr = np.asarray(arrival_ns, np.int64).reshape(-1)
    if len(arr) != len(sym):
        raise ValueError(f"{len(arr)} arrival times for {len(sym)} symbols")
    out = np.full(len(sym), _lib.NMZ_NONE, np.uint32)
    if not len(sym) or not len(rec):
        return out

    def occurrence(order, s):
        """Per element (in `order`): how many earlier elements of `order` carry the same symbol."""
        by_sym = order[np.argsort(s[order], kind="stable")]  # grouped by symbol, `order` kept inside a group
        g = s[by_sym]
        start = np.r_[0, np.nonzero(g[1:] != g[:-1])[0] + 1]
        occ = np.arange(len(g)) - np.repeat(start, np.diff(np.r_[start, len(g)]))
        return by_sym, occ

    ev, ev_occ = occurrence(np.lexsort((np.arange(len(sym)), arr)), sym)  # by (arrival, index)
    rc, rc_occ = occurrence(np.arange(len(rec)), rec)
    # join on (symbol, occurrence): both sides sorted by symbol then occurrence
    ek = np.stack([sym[ev], ev_occ.astype(np.uint64)], axis=1)
    rk = np.stack([rec[rc], rc_occ.astype(np.uint64)], axis=1)
    ekv = np.ascontiguousarray(ek).view([("s", "<u8"), ("o", "<u8")]).reshape(-1)
    rkv = np.ascontiguousarray(rk).view([("s", "<u8"), ("o", "<u8")]).reshape(-1)
    at = np.searchsorted(rkv, ekv)
    hit = at < len(rkv)
    hit[hit] = rkv[at[hit]] == ekv[hit]
    out[ev[hit]] = rc[at[hit]].astype(np.uint32)
    return out


# ---- order contrast: which event pairs separate failing runs from passing ones -----------------------------
class ContrastResult:
    """order_contrast's result: pairs[k] (ORDER_PAIR_DTYPE, best first by (score desc, n_fail_with desc,
    before * E + after asc); the sentinel {NMZ_NONE, NMZ_NONE, INT64_MIN, 0, 0, 0, 0} past the pairs with
    score > 0), counts[E][E] (PAIR_COUNTS_DTYPE at [before][after], diagonal 0; None unless asked for), n_fail,
    n_pass and n_positive (the number of ordered pairs with score > 0)."""

    def __init__(self, pairs, counts, n_fail, n_pass, n_positive):
        self.pairs = pairs
        self.counts = counts
        self.n_fail = n_fail
        self.n_pass = n_pass
        self.n_positive = n_positive
        self.run_ids = None  # Naive.OrderContrast: the stored runs behind the rows


def _contrast_labels(failed, n_runs):
    failed = np.asarray(failed)
    if failed.dtype == np.bool_:
        failed = failed.astype(np.uint8)
    elif failed.size and (failed.min() < 0 or failed.max() > 255):
        raise ValueError("failed holds a label outside uint8")
    failed = np.ascontiguousarray(failed, np.uint8).reshape(-1)
    if len(failed) != n_runs:
        raise ValueError(f"{len(failed)} labels for {n_runs} runs")
    return failed


def _contrast_inputs(pos, failed):
    pos = np.ascontiguousarray(pos, np.uint32)
    if pos.ndim != 2:
        raise ValueError(f"pos must be [runs][events], got shape {pos.shape}")
    return pos, _contrast_labels(failed, pos.shape[0])


def run_positions(sym, arrival_ns, traces):
    """pos[len(traces)][len(sym)] (uint32): one match_target row per recorded run (SingleTraces or event-symbol
    arrays) against the event universe (sym, arrival_ns) -- the trace whose hints the sweeps take. pos[r][e] is the
    position of event e in run r, NMZ_NONE if the run does not hold it: order_contrast's input."""
    sym = np.asarray(sym, np.uint64).reshape(-1)
    out = np.full((len(traces), len(sym)), _lib.NMZ_NONE, np.uint32)
    for r, t in enumerate(traces):
        out[r] = match_target(sym, arrival_ns, t.symbols if isinstance(t, SingleTrace) else t)
    return out


def order_contrast(pos, failed, k=64, want_counts=False, ctx=None):
    """The ordered event pairs (before, after) released that way round in the failing runs and the other way round
    in the passing ones (nmz_order_contrast; semantics in include/nmz_gpu.h and DESIGN.md section 2). pos[R][E] as
    run_positions gives it, failed[R] 0 / 1 (or bool). For every ordered pair F = failing runs that hold both events
    and release `before` first, P = the same over passing runs, score = F * n_pass - P * n_fail. Returns a
    ContrastResult with the k best pairs; want_counts adds every pair's (F, P) -- E^2 records, off by default.
    From a storage to a replay:

        pos = historystorage.run_positions(sym, arrival_ns, runs)            # runs: the stored SingleTraces
        c = historystorage.order_contrast(pos, failed, k=64)                 # failed: not IsSuccessful, per run
        cons = replay.constraints_from_pairs(c.pairs, 1_000_000, per_event=2)
        r = policy.OrderSweep(hints, arrival_ns, cons, seeds=seeds, k=8, want_stats=False)
        env = replay.replay_env(replay.replayable_seeds(r.topk, seeds)[0], os.environ)   # NMZ_REPLAY_SEED
    """
    pos, failed = _contrast_inputs(pos, failed)
    R, E = pos.shape
    k = int(k)
    if not 0 <= k < 2**32:
        raise ValueError(f"k = {k} does not fit uint32")
    ctx = ctx or _lib.default_context()
    pairs = np.zeros(k, _lib.ORDER_PAIR_DTYPE)
    counts = np.zeros((E, E), _lib.PAIR_COUNTS_DTYPE) if want_counts else None
    info = np.zeros(1, _lib.CONTRAST_INFO_DTYPE)
    _lib.check(_lib.load().nmz_order_contrast(ctx.handle, _lib.ptr(pos), _lib.ptr(failed), R, E, k, _lib.ptr(counts),
                                              _lib.ptr(pairs) if k else None, _lib.ptr(info)))
    return ContrastResult(pairs, counts, int(info[0]["n_fail"]), int(info[0]["n_pass"]), int(info[0]["n_positive"]))


def _universe(sym, arrival_ns):
    sym = np.ascontiguousarray(sym, np.uint64).reshape(-1)
    arr = np.ascontiguousarray(arrival_ns, np.int64).reshape(-1)
    if len(arr) != len(sym):
        raise ValueError(f"{len(arr)} arrival times for {len(sym)} symbols")
    return sym, arr


def _run_set(traces):
    if isinstance(traces, TraceSet):
        return traces
    return TraceSet([t.symbols if isinstance(t, SingleTrace) else np.asarray(t, np.uint64).reshape(-1)
                     for t in traces])


def match_run_host(sym, arrival_ns, recorded_sym):
    """match_target's row on the host through nmz_match_run_host (no GPU): plain loops by the definition, sharing
    nothing with the kernel or with match_target's numpy."""
    sym, arr = _universe(sym, arrival_ns)
    rec = np.ascontiguousarray(recorded_sym, np.uint64).reshape(-1)
    out = np.zeros(len(sym), np.uint32)
    _lib.check(_lib.load().nmz_match_run_host(_lib.ptr(sym), _lib.ptr(arr), len(sym), _lib.ptr(rec), len(rec),
                                              _lib.ptr(out)))
    return out


class MatchPlan:
    """The event universe (sym, arrival_ns) resident on the GPU (nmz_match_plan): runs_dev matches a device CSR of
    recorded runs into a device pos[n_runs][E], the array nmz_order_contrast_dev and target_pos take."""

    def __init__(self, sym, arrival_ns, ctx=None):
        self.ctx = ctx or _lib.default_context()
        sym, arr = _universe(sym, arrival_ns)
        self.plan = ctypes.c_void_p()
        L = _lib.load()
        _lib.check(L.nmz_match_plan_create(self.ctx.handle, _lib.ptr(sym), _lib.ptr(arr), len(sym),
                                           ctypes.byref(self.plan)))
        e, u = ctypes.c_uint32(), ctypes.c_uint32()
        _lib.check(L.nmz_match_plan_info(self.plan, ctypes.byref(e), ctypes.byref(u)))
        self.n_events, self.n_symbols = e.value, u.value

    def runs_dev(self, d_run_off, d_run_sym, n_runs, d_pos, stream=None):
        """Device pointers (ints): uint64 offsets[n_runs + 1] and symbols in, uint32 pos[n_runs][E] out, enqueued
        on `stream` (a HIP stream handle; None = the context's)."""
        _lib.check(_lib.load().nmz_match_runs_dev(self.plan, ctypes.c_void_p(d_run_off), ctypes.c_void_p(d_run_sym),
                                                  int(n_runs), ctypes.c_void_p(d_pos),
                                                  ctypes.c_void_p(stream) if stream else None))

    def close(self):
        if self.plan:
            _lib.load().nmz_match_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def match_runs(sym, arrival_ns, traces, ctx=None):
    """run_positions on the GPU (nmz_match_runs): pos[len(traces)][len(sym)] (uint32), one match_target row per
    recorded run (SingleTraces, event-symbol arrays or a TraceSet) against the event universe (sym, arrival_ns)."""
    sym, arr = _universe(sym, arrival_ns)
    ts = _run_set(traces)
    out = np.full((len(ts), len(sym)), _lib.NMZ_NONE, np.uint32)
    ctx = ctx or _lib.default_context()
    _lib.check(_lib.load().nmz_match_runs(ctx.handle, _lib.ptr(sym), _lib.ptr(arr), len(sym), _lib.ptr(ts.off),
                                          _lib.ptr(ts.sym), len(ts), _lib.ptr(out)))
    return out


def order_contrast_runs(sym, arrival_ns, traces, failed, k=64, want_counts=False, ctx=None):
    """order_contrast(run_positions(sym, arrival_ns, traces), failed, ...) with the matching on the GPU too
    (nmz_order_contrast_runs): the runs' symbols go up, pos is made and read on the device and never comes back.
    Returns the same ContrastResult, byte for byte."""
    sym, arr = _universe(sym, arrival_ns)
    ts = _run_set(traces)
    failed = _contrast_labels(failed, len(ts))
    E = len(sym)
    k = int(k)
    if not 0 <= k < 2**32:
        raise ValueError(f"k = {k} does not fit uint32")
    ctx = ctx or _lib.default_context()
    pairs = np.zeros(k, _lib.ORDER_PAIR_DTYPE)
    counts = np.zeros((E, E), _lib.PAIR_COUNTS_DTYPE) if want_counts else None
    info = np.zeros(1, _lib.CONTRAST_INFO_DTYPE)
    _lib.check(_lib.load().nmz_order_contrast_runs(ctx.handle, _lib.ptr(sym), _lib.ptr(arr), E, _lib.ptr(ts.off),
                                                   _lib.ptr(ts.sym), _lib.ptr(failed), len(ts), k, _lib.ptr(counts),
                                                   _lib.ptr(pairs) if k else None, _lib.ptr(info)))
    return ContrastResult(pairs, counts, int(info[0]["n_fail"]), int(info[0]["n_pass"]), int(info[0]["n_positive"]))


def order_pair(pos, failed, before, after):
    """One ordered pair on the host (nmz_order_contrast_host, no GPU): (pair, n_fail, n_pass) with pair one
    ORDER_PAIR_DTYPE record holding both directions' counts. Plain loops that share nothing with the kernels: the
    check of order_contrast, and the way to vet a pair before replays are spent on it."""
    pos, failed = _contrast_inputs(pos, failed)
    R, E = pos.shape
    out = np.zeros(1, _lib.ORDER_PAIR_DTYPE)
    info = np.zeros(1, _lib.CONTRAST_INFO_DTYPE)
    if not (0 <= int(before) < 2**32 and 0 <= int(after) < 2**32):
        raise ValueError(f"event indices ({before}, {after}) do not fit uint32")
    _lib.check(_lib.load().nmz_order_contrast_host(_lib.ptr(pos), _lib.ptr(failed), R, E, int(before), int(after),
                                                   _lib.ptr(out), _lib.ptr(info)))
    return out[0], int(info[0]["n_fail"]), int(info[0]["n_pass"])


# ---- edit scripts: what differs between two traces ------------------------------------------------------------
class EditScripts:
    """edit_scripts' result: dist[P] (uint32, ED_band: band + 1 = beyond the band) and ops[P][band] (EDIT_OP_DTYPE:
    a_pos, b_pos, kind; the pair's ops in forward order, then {NMZ_NONE, NMZ_NONE, NMZ_NONE})."""

    def __init__(self, dist, ops, band):
        self.dist = dist
        self.ops = ops
        self.band = band

    def script(self, p):
        """The ops of pair p (a view of its first dist[p] rows), or None beyond the band."""
        d = int(self.dist[p])
        return self.ops[p, :d] if d <= self.band else None


class AlignPlan:
    """The history scratch of the edit-script kernel for `slots` pairs in flight of up to max_len elements each
    (nmz_ed_align_plan): pairs_dev aligns device pairs over a device CSR into device dist / ops arrays."""

    def __init__(self, band, max_len, ctx=None):
        self.ctx = ctx or _lib.default_context()
        self.band = int(band)
        self.plan = ctypes.c_void_p()
        L = _lib.load()
        _lib.check(L.nmz_ed_align_plan_create(self.ctx.handle, self.band, int(max_len), ctypes.byref(self.plan)))
        s, h = ctypes.c_uint32(), ctypes.c_uint64()
        _lib.check(L.nmz_ed_align_plan_info(self.plan, ctypes.byref(s), ctypes.byref(h)))
        self.slots, self.history_bytes = s.value, h.value

    def pairs_dev(self, d_off, d_sym, d_pairs, n_pairs, d_dist, d_ops, stream=None):
        """Device pointers (ints): uint64 offsets and symbols, uint32 pairs[n_pairs][2] in; uint32 dist[n_pairs]
        and EDIT_OP_DTYPE ops[n_pairs][band] out, enqueued on `stream` (a HIP stream handle; None = the context's).
        A pair with a trace longer than max_len gets dist = NMZ_NONE."""
        _lib.check(_lib.load().nmz_ed_align_pairs_dev(
            self.plan, ctypes.c_void_p(d_off), ctypes.c_void_p(d_sym), ctypes.c_void_p(d_pairs), int(n_pairs),
            ctypes.c_void_p(d_dist), ctypes.c_void_p(d_ops), ctypes.c_void_p(stream) if stream else None))

    def close(self):
        if self.plan:
            _lib.load().nmz_ed_align_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def edit_scripts(ts, pairs, band, ctx=None):
    """The canonical edit script of every pair (ia, ib): how trace ia becomes trace ib (nmz_ed_align_pairs; the
    semantics in include/nmz_gpu.h and DESIGN.md section 2). dist equals ed_pairs' value; band <= 64."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    band = int(band)
    if not 0 <= band < 2**32:
        raise ValueError(f"band = {band} does not fit uint32")
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), min(band, _lib.NMZ_ALIGN_MAX_BAND)), _lib.EDIT_OP_DTYPE)
    ctx = ctx or (_lib.default_context() if len(pairs) and band <= _lib.NMZ_ALIGN_MAX_BAND else None)
    _lib.check(_lib.load().nmz_ed_align_pairs(ctx.handle if ctx else None, _lib.ptr(ts.off), _lib.ptr(ts.sym), len(ts),
                                              _lib.ptr(pairs), len(pairs), band, _lib.ptr(dist),
                                              _lib.ptr(ops) if ops.size else None))
    return EditScripts(dist, ops, band)


def edit_script_host(a, b, band):
    """One pair on the host through nmz_ed_align_host (no GPU): (dist, script) with script the first dist ops, or
    None beyond the band. A plain banded matrix and the walk by the definition; shares nothing with the kernel."""
    a = np.ascontiguousarray(a, np.uint64).reshape(-1)
    b = np.ascontiguousarray(b, np.uint64).reshape(-1)
    band = int(band)
    if not 0 <= band < 2**32:
        raise ValueError(f"band = {band} does not fit uint32")
    dist = ctypes.c_uint32()
    ops = np.zeros(min(band, _lib.NMZ_ALIGN_MAX_BAND), _lib.EDIT_OP_DTYPE)
    _lib.check(_lib.load().nmz_ed_align_host(_lib.ptr(a), len(a), _lib.ptr(b), len(b), band, ctypes.byref(dist),
                                             _lib.ptr(ops) if ops.size else None))
    return dist.value, (ops[:dist.value] if dist.value <= band else None)


class AlignWidePlan:
    """AlignPlan for every band 0 .. 1024 (nmz_ed_align_wide_plan): beyond 64 the history scratch of
    k_ed_align_wide, up to 64 a narrow plan behind the same calls."""

    def __init__(self, band, max_len, ctx=None):
        self.ctx = ctx or _lib.default_context()
        self.band = int(band)
        self.plan = ctypes.c_void_p()
        L = _lib.load()
        _lib.check(L.nmz_ed_align_wide_plan_create(self.ctx.handle, self.band, int(max_len), ctypes.byref(self.plan)))
        s, h = ctypes.c_uint32(), ctypes.c_uint64()
        _lib.check(L.nmz_ed_align_wide_plan_info(self.plan, ctypes.byref(s), ctypes.byref(h)))
        self.slots, self.history_bytes = s.value, h.value

    def pairs_dev(self, d_off, d_sym, d_pairs, n_pairs, d_dist, d_ops, stream=None):
        """AlignPlan.pairs_dev's arguments and results, ops[n_pairs][band] with band up to 1024."""
        _lib.check(_lib.load().nmz_ed_align_wide_pairs_dev(
            self.plan, ctypes.c_void_p(d_off), ctypes.c_void_p(d_sym), ctypes.c_void_p(d_pairs), int(n_pairs),
            ctypes.c_void_p(d_dist), ctypes.c_void_p(d_ops), ctypes.c_void_p(stream) if stream else None))

    def close(self):
        if self.plan:
            _lib.load().nmz_ed_align_wide_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def edit_scripts_wide(ts, pairs, band, ctx=None):
    """edit_scripts for every band 0 .. 1024 (nmz_ed_align_wide_pairs): the same EditScripts, ops of shape
    [P][band]. A pair within 64 edits gets the ops edit_scripts gives at band 64; a band <= 64 gives edit_scripts'
    bytes."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    band = int(band)
    if not 0 <= band < 2**32:
        raise ValueError(f"band = {band} does not fit uint32")
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), min(band, _lib.NMZ_ALIGN_WIDE_MAX_BAND)), _lib.EDIT_OP_DTYPE)
    ctx = ctx or (_lib.default_context() if len(pairs) and band <= _lib.NMZ_ALIGN_WIDE_MAX_BAND else None)
    _lib.check(_lib.load().nmz_ed_align_wide_pairs(ctx.handle if ctx else None, _lib.ptr(ts.off), _lib.ptr(ts.sym),
                                                   len(ts), _lib.ptr(pairs), len(pairs), band, _lib.ptr(dist),
                                                   _lib.ptr(ops) if ops.size else None))
    return EditScripts(dist, ops, band)


def edit_script_wide_host(a, b, band):
    """edit_script_host for every band 0 .. 1024 (nmz_ed_align_wide_host, no GPU): (dist, script | None). The same
    plain banded matrix with 16-bit cells; the reference of edit_scripts_wide."""
    a = np.ascontiguousarray(a, np.uint64).reshape(-1)
    b = np.ascontiguousarray(b, np.uint64).reshape(-1)
    band = int(band)
    if not 0 <= band < 2**32:
        raise ValueError(f"band = {band} does not fit uint32")
    dist = ctypes.c_uint32()
    ops = np.zeros(min(band, _lib.NMZ_ALIGN_WIDE_MAX_BAND), _lib.EDIT_OP_DTYPE)
    _lib.check(_lib.load().nmz_ed_align_wide_host(_lib.ptr(a), len(a), _lib.ptr(b), len(b), band, ctypes.byref(dist),
                                                  _lib.ptr(ops) if ops.size else None))
    return dist.value, (ops[:dist.value] if dist.value <= band else None)


def script_moves(a, b, ops):
    """The events a script moved: the k-th DEL of a symbol value pairs with the k-th INS of that value, in script
    order. Returns [(symbol, a_pos, b_pos)]: a[a_pos] was delivered at b_pos of b instead. DELs and INSs without a
    partner (an event missing or extra) and SUBs are not moves. Plain Python over the ops given: a script of any
    length, edit_scripts_wide's included."""
    dels, inss = {}, {}
    for o in ops:
        k = int(o["kind"])
        if k == _lib.NMZ_EDIT_DEL:
            dels.setdefault(int(a[int(o["a_pos"])]), []).append(int(o["a_pos"]))
        elif k == _lib.NMZ_EDIT_INS:
            inss.setdefault(int(b[int(o["b_pos"])]), []).append(int(o["b_pos"]))
    out = [(s, ap, bp) for s, aps in dels.items() for ap, bp in zip(aps, inss.get(s, []))]
    return sorted(out, key=lambda t: (t[1], t[2]))



# ---- move profiles: which events move between the runs of many pairs ----------------------------------------------
def script_partners(a, b, ops):
    """script_moves' pairing as slot indices, on the host through nmz_script_moves_host (no GPU): partner[len(ops)]
    (uint32), the slot of the INS that the DEL of slot s pairs with and the other way round -- the r-th DEL naming a
    value and the r-th INS naming it, in script order -- and NMZ_NONE for a DEL or INS without a partner and for
    every SUB. Plain loops by the definition; shares nothing with the kernel."""
    a = np.ascontiguousarray(a, np.uint64).reshape(-1)
    b = np.ascontiguousarray(b, np.uint64).reshape(-1)
    ops = np.ascontiguousarray(ops, _lib.EDIT_OP_DTYPE).reshape(-1)
    partner = np.full(len(ops), _lib.NMZ_NONE, np.uint32)
    _lib.check(_lib.load().nmz_script_moves_host(_lib.ptr(a), len(a), _lib.ptr(b), len(b), _lib.ptr(ops), len(ops),
                                                 _lib.ptr(partner)))
    return partner


class MoveProfile:
    """move_profile's result: symbols[U] (uint64, increasing), counts[U] (MOVE_COUNTS_DTYPE: later, earlier, dropped,
    extra, sub_from, sub_to, n_pairs, span_later, span_earlier of that symbol over all the scripts), info (one
    MOVE_INFO_DTYPE record: n_scripts, n_beyond, n_ops, n_unknown), dist[P] (ED_band of every pair) and, from
    move_profile_of on request, partner[P][band]. "Later" = delivered later in b (the pair's second trace) than in
    a."""

    def __init__(self, symbols, counts, info, dist, partner=None):
        self.symbols = symbols
        self.counts = counts
        self.info = info
        self.dist = dist
        self.partner = partner
        self.pairs = None  # Naive.DiffFailing: the stored-run ids (passing neighbour, failing run) behind the pairs

    def top(self, k):
        """The k symbols that most scripts name, as [(symbol, counts record)]: by (n_pairs desc, later + earlier
        desc, symbol asc); symbols no script names are left out."""
        c = self.counts
        moved = c["later"].astype(np.int64) + c["earlier"].astype(np.int64)
        order = np.lexsort((self.symbols, -moved, -c["n_pairs"].astype(np.int64)))
        return [(int(self.symbols[u]), c[u]) for u in order[:int(k)] if c[u]["n_pairs"] > 0]


def _move_table(ts, usym):
    if usym is None:
        total = int(ts.off[-1])
        return np.unique(ts.sym[:total])
    return np.ascontiguousarray(usym, np.uint64).reshape(-1)


def _move_band(band):
    band = int(band)
    if not 0 <= band < 2**32:
        raise ValueError(f"band = {band} does not fit uint32")
    return band


def move_profile(ts, pairs, band, ctx=None, usym=None):
    """From traces to the tally in one call (nmz_ed_diff_profile; the semantics in include/nmz_gpu.h and DESIGN.md
    section 2, "Move profiles"): every pair (ia, ib) is aligned as edit_scripts aligns it and its script's ops are
    paired and counted per symbol on the device; the ops never come to the host. usym: the symbols to tally
    (strictly increasing; default: every symbol of ts). Returns a MoveProfile; band <= 64."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    band = _move_band(band)
    usym = _move_table(ts, usym)
    dist = np.zeros(len(pairs), np.uint32)
    counts = np.zeros(len(usym), _lib.MOVE_COUNTS_DTYPE)
    info = np.zeros(1, _lib.MOVE_INFO_DTYPE)
    ctx = ctx or (_lib.default_context() if len(pairs) and band <= _lib.NMZ_ALIGN_MAX_BAND else None)
    _lib.check(_lib.load().nmz_ed_diff_profile(ctx.handle if ctx else None, _lib.ptr(ts.off), _lib.ptr(ts.sym), len(ts),
                                               _lib.ptr(pairs), len(pairs), band, _lib.ptr(usym), len(usym),
                                               _lib.ptr(dist), _lib.ptr(counts) if len(usym) else None,
                                               _lib.ptr(info)))
    return MoveProfile(usym, counts, info[0], dist)


def move_profile_of(ts, pairs, es, ctx=None, usym=None, want_partner=False, host=False):
    """The tally of scripts the caller already holds (es: edit_scripts' result over the same ts and pairs), through
    nmz_move_profile -- or, with host=True, through nmz_move_profile_host on the calling thread (no GPU).
    want_partner adds partner[P][band] (uint32: the partner's slot, NMZ_NONE without one) to the MoveProfile."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    band = _move_band(es.band)
    usym = _move_table(ts, usym)
    dist = np.ascontiguousarray(es.dist, np.uint32).reshape(-1)
    ops = np.ascontiguousarray(es.ops, _lib.EDIT_OP_DTYPE)
    if len(dist) != len(pairs) or ops.shape != (len(pairs), min(band, _lib.NMZ_ALIGN_MAX_BAND)):
        raise ValueError(f"scripts of shape {ops.shape} for {len(pairs)} pairs at band {band}")
    counts = np.zeros(len(usym), _lib.MOVE_COUNTS_DTYPE)
    info = np.zeros(1, _lib.MOVE_INFO_DTYPE)
    partner = np.full(ops.shape, _lib.NMZ_NONE, np.uint32) if want_partner else None
    args = (_lib.ptr(ts.off), _lib.ptr(ts.sym), len(ts), _lib.ptr(pairs), len(pairs), band, _lib.ptr(dist),
            _lib.ptr(ops) if ops.size else None, _lib.ptr(usym), len(usym),
            _lib.ptr(partner) if want_partner and partner.size else None, _lib.ptr(counts) if len(usym) else None,
            _lib.ptr(info))
    if host:
        _lib.check(_lib.load().nmz_move_profile_host(*args))
    else:
        ctx = ctx or (_lib.default_context() if len(pairs) and band <= _lib.NMZ_ALIGN_MAX_BAND else None)
        _lib.check(_lib.load().nmz_move_profile(ctx.handle if ctx else None, *args))
    return MoveProfile(usym, counts, info[0], dist, partner)


def move_profile_wide(ts, pairs, band, ctx=None, usym=None):
    """move_profile for every band 0 .. 1024 (nmz_ed_diff_profile_wide): the pairs are aligned as edit_scripts_wide
    aligns them and tallied on the device; the ops never come to the host. The same MoveProfile; a band <= 64 gives
    move_profile's bytes."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    band = _move_band(band)
    usym = _move_table(ts, usym)
    dist = np.zeros(len(pairs), np.uint32)
    counts = np.zeros(len(usym), _lib.MOVE_COUNTS_DTYPE)
    info = np.zeros(1, _lib.MOVE_INFO_DTYPE)
    ctx = ctx or (_lib.default_context() if len(pairs) and band <= _lib.NMZ_ALIGN_WIDE_MAX_BAND else None)
    _lib.check(_lib.load().nmz_ed_diff_profile_wide(ctx.handle if ctx else None, _lib.ptr(ts.off), _lib.ptr(ts.sym),
                                                    len(ts), _lib.ptr(pairs), len(pairs), band, _lib.ptr(usym),
                                                    len(usym), _lib.ptr(dist),
                                                    _lib.ptr(counts) if len(usym) else None, _lib.ptr(info)))
    return MoveProfile(usym, counts, info[0], dist)


def move_profile_of_wide(ts, pairs, es, ctx=None, usym=None, want_partner=False, host=False):
    """move_profile_of for every band 0 .. 1024 (es: edit_scripts_wide's result over the same ts and pairs), through
    nmz_move_profile_wide -- or, with host=True, through nmz_move_profile_wide_host on the calling thread (no GPU).
    want_partner adds partner[P][band]."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    band = _move_band(es.band)
    usym = _move_table(ts, usym)
    dist = np.ascontiguousarray(es.dist, np.uint32).reshape(-1)
    ops = np.ascontiguousarray(es.ops, _lib.EDIT_OP_DTYPE)
    if len(dist) != len(pairs) or ops.shape != (len(pairs), min(band, _lib.NMZ_ALIGN_WIDE_MAX_BAND)):
        raise ValueError(f"scripts of shape {ops.shape} for {len(pairs)} pairs at band {band}")
    counts = np.zeros(len(usym), _lib.MOVE_COUNTS_DTYPE)
    info = np.zeros(1, _lib.MOVE_INFO_DTYPE)
    partner = np.full(ops.shape, _lib.NMZ_NONE, np.uint32) if want_partner else None
    args = (_lib.ptr(ts.off), _lib.ptr(ts.sym), len(ts), _lib.ptr(pairs), len(pairs), band, _lib.ptr(dist),
            _lib.ptr(ops) if ops.size else None, _lib.ptr(usym), len(usym),
            _lib.ptr(partner) if want_partner and partner.size else None, _lib.ptr(counts) if len(usym) else None,
            _lib.ptr(info))
    if host:
        _lib.check(_lib.load().nmz_move_profile_wide_host(*args))
    else:
        ctx = ctx or (_lib.default_context() if len(pairs) and band <= _lib.NMZ_ALIGN_WIDE_MAX_BAND else None)
        _lib.check(_lib.load().nmz_move_profile_wide(ctx.handle if ctx else None, *args))
    return MoveProfile(usym, counts, info[0], dist, partner)


# ---- edit scripts and move profiles per entity: the partial-order view of a diff ---------------------------------
def po_entities(traces):
    """SingleTraces -> (TraceSet of event symbols, entity[N] uint32 parallel to its sym, names): ids global to the
    set, assigned by sorted EntityID (names[id]), NMZ_NONE for an action without an event. Unlike po_inputs' ids
    (dense per trace), equal ids in two traces mean the same entity: what the per-entity diff needs."""
    ts = TraceSet([t.symbols for t in traces])
    names = sorted({e for t in traces for e in t.entities if e is not None})
    ids = {e: i for i, e in enumerate(names)}
    ent = np.full(max(int(ts.off[-1]), 1), _lib.NMZ_NONE, np.uint32)
    pos = 0
    for t in traces:
        for e in t.entities:
            if e is not None:
                ent[pos] = ids[e]
            pos += 1
    return ts, ent, names


def _po_entity(n, entity, n_entities):
    """entity[n] as a contiguous uint32 array, and n_entities (default: the largest id + 1, at least 1)."""
    entity = np.ascontiguousarray(entity, np.uint32).reshape(-1)
    if len(entity) < n:
        raise ValueError(f"{len(entity)} entity ids for {n} elements")
    if n_entities is None:
        live = entity[:n][entity[:n] != _lib.NMZ_NONE]
        n_entities = int(live.max()) + 1 if len(live) else 1
    n_entities = int(n_entities)
    if not 0 <= n_entities < 2**32:
        raise ValueError(f"n_entities = {n_entities} does not fit uint32")
    return entity, n_entities


class PoProjection:
    """po_project's result: poff[T * G + 1] (uint64), psym (uint64) and psrc (uint32): projected trace t * G + g is
    psym[poff[t * G + g]:poff[t * G + g + 1]], and psrc holds each element's index in its trace."""

    def __init__(self, poff, psym, psrc, n_entities):
        self.poff = poff
        self.psym = psym
        self.psrc = psrc
        self.n_entities = n_entities

    def trace(self, t, g):
        """(t|g, src_g(t)): the symbols of entity g in trace t, and their indices in t."""
        lo, hi = int(self.poff[t * self.n_entities + g]), int(self.poff[t * self.n_entities + g + 1])
        return self.psym[lo:hi], self.psrc[lo:hi]


def po_project(ts, entity, n_entities=None, ctx=None):
    """Every trace of ts split by entity on the device (nmz_po_project; DESIGN.md section 2, "Edit scripts per
    entity"): a stable partition, elements with entity NMZ_NONE dropped. Returns a PoProjection."""
    entity, G = _po_entity(int(ts.off[-1]), entity, n_entities)
    T = len(ts)
    kept = int((entity[:int(ts.off[-1])] != _lib.NMZ_NONE).sum())
    poff = np.zeros(T * min(G, _lib.NMZ_PO_MAX_ENTITIES) + 1, np.uint64)
    psym = np.zeros(max(kept, 1), np.uint64)
    psrc = np.zeros(max(kept, 1), np.uint32)
    ctx = ctx or (_lib.default_context() if T and 1 <= G <= _lib.NMZ_PO_MAX_ENTITIES else None)
    _lib.check(_lib.load().nmz_po_project(ctx.handle if ctx else None, _lib.ptr(ts.off), _lib.ptr(ts.sym),
                                          _lib.ptr(entity), T, G, _lib.ptr(poff), _lib.ptr(psym), _lib.ptr(psrc)))
    return PoProjection(poff, psym[:kept], psrc[:kept], G)


def edit_scripts_po(ts, entity, pairs, band, n_entities=None, ctx=None):
    """edit_scripts_wide per entity (nmz_ed_align_po_pairs): dist = min(sum over the entities of Lev(a|g, b|g),
    band + 1) and, within the band, the entities' canonical scripts concatenated in ascending entity id with the
    positions lifted back to the whole traces. dist == 0 <=> the traces are equal in partial order
    (first_equal(..., po_reduction=True)). entity[N] is parallel to ts.sym, ids global to ts (po_entities). The same
    EditScripts; with one entity and no NMZ_NONE, edit_scripts_wide's bytes."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    band = _move_band(band)
    entity, G = _po_entity(int(ts.off[-1]), entity, n_entities)
    dist = np.zeros(len(pairs), np.uint32)
    ops = np.zeros((len(pairs), min(band, _lib.NMZ_ALIGN_WIDE_MAX_BAND)), _lib.EDIT_OP_DTYPE)
    ctx = ctx or (_lib.default_context() if len(pairs) and band <= _lib.NMZ_ALIGN_WIDE_MAX_BAND
                  and 1 <= G <= _lib.NMZ_PO_MAX_ENTITIES else None)
    _lib.check(_lib.load().nmz_ed_align_po_pairs(ctx.handle if ctx else None, _lib.ptr(ts.off), _lib.ptr(ts.sym),
                                                 _lib.ptr(entity), len(ts), G, _lib.ptr(pairs), len(pairs), band,
                                                 _lib.ptr(dist), _lib.ptr(ops) if ops.size else None))
    return EditScripts(dist, ops, band)


def edit_script_po_host(a, ea, b, eb, band, n_entities=None):
    """One pair per entity on the host through nmz_ed_align_po_host (no GPU): (dist, script | None). Plain vectors
    per entity and edit_script_wide_host's matrix per entity; the reference of edit_scripts_po."""
    a = np.ascontiguousarray(a, np.uint64).reshape(-1)
    b = np.ascontiguousarray(b, np.uint64).reshape(-1)
    band = _move_band(band)
    ea, ga = _po_entity(len(a), ea, n_entities)
    eb, gb = _po_entity(len(b), eb, n_entities)
    dist = ctypes.c_uint32()
    ops = np.zeros(min(band, _lib.NMZ_ALIGN_WIDE_MAX_BAND), _lib.EDIT_OP_DTYPE)
    _lib.check(_lib.load().nmz_ed_align_po_host(_lib.ptr(a), _lib.ptr(ea), len(a), _lib.ptr(b), _lib.ptr(eb), len(b),
                                                max(ga, gb), band, ctypes.byref(dist),
                                                _lib.ptr(ops) if ops.size else None))
    return dist.value, (ops[:dist.value] if dist.value <= band else None)


def script_by_entity(ea, eb, ops):
    """A PO script split into its segments: {entity id: the ops of that entity, in script order}. The entity of an
    op is ea[a_pos] for a DEL or SUB and eb[b_pos] for an INS."""
    out = {}
    for o in ops:
        g = int(eb[int(o["b_pos"])]) if int(o["kind"]) == _lib.NMZ_EDIT_INS else int(ea[int(o["a_pos"])])
        out.setdefault(g, []).append(o)
    return {g: np.array(v, _lib.EDIT_OP_DTYPE) for g, v in out.items()}


class AlignPoPlan:
    """A wide align plan for projections of up to max_len elements plus the sub-pair scratch for max_pairs pairs per
    launch (nmz_ed_align_po_plan): pairs_dev makes the PO scripts of device pairs from nmz_po_project_dev's
    outputs."""

    def __init__(self, band, n_entities, max_len, max_pairs, ctx=None):
        self.ctx = ctx or _lib.default_context()
        self.band = int(band)
        self.n_entities = int(n_entities)
        self.plan = ctypes.c_void_p()
        L = _lib.load()
        _lib.check(L.nmz_ed_align_po_plan_create(self.ctx.handle, self.band, self.n_entities, int(max_len),
                                                 int(max_pairs), ctypes.byref(self.plan)))
        s, h, b = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.c_uint64()
        _lib.check(L.nmz_ed_align_po_plan_info(self.plan, ctypes.byref(s), ctypes.byref(h), ctypes.byref(b)))
        self.slots, self.history_bytes, self.sub_pair_bytes = s.value, h.value, b.value

    def project_dev(self, d_off, d_sym, d_entity, n_traces, d_poff, d_psym, d_psrc, stream=None):
        """nmz_po_project_dev with the plan's n_entities: device pointers (ints), enqueued on `stream`."""
        _lib.check(_lib.load().nmz_po_project_dev(
            self.ctx.handle, ctypes.c_void_p(d_off), ctypes.c_void_p(d_sym), ctypes.c_void_p(d_entity), int(n_traces),
            self.n_entities, ctypes.c_void_p(d_poff), ctypes.c_void_p(d_psym), ctypes.c_void_p(d_psrc),
            ctypes.c_void_p(stream) if stream else None))

    def pairs_dev(self, d_off, d_poff, d_psym, d_psrc, d_pairs, n_pairs, d_dist, d_ops, stream=None):
        """Device pointers (ints): the original offsets, the projection, uint32 pairs[n_pairs][2] in; uint32
        dist[n_pairs] and EDIT_OP_DTYPE ops[n_pairs][band] out, enqueued on `stream`. n_pairs <= max_pairs."""
        _lib.check(_lib.load().nmz_ed_align_po_pairs_dev(
            self.plan, ctypes.c_void_p(d_off), ctypes.c_void_p(d_poff), ctypes.c_void_p(d_psym),
            ctypes.c_void_p(d_psrc), ctypes.c_void_p(d_pairs), int(n_pairs), ctypes.c_void_p(d_dist),
            ctypes.c_void_p(d_ops), ctypes.c_void_p(stream) if stream else None))

    def close(self):
        if self.plan:
            _lib.load().nmz_ed_align_po_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def move_profile_po(ts, entity, pairs, band, ctx=None, usym=None, n_entities=None):
    """move_profile_wide over the per-entity scripts (nmz_ed_diff_profile_po): the traces are projected, the PO
    scripts made as edit_scripts_po makes them and tallied on the device; the ops never come to the host. By
    definition the profile that move_profile_of_wide gives for edit_scripts_po's output. The same MoveProfile."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    band = _move_band(band)
    usym = _move_table(ts, usym)
    entity, G = _po_entity(int(ts.off[-1]), entity, n_entities)
    dist = np.zeros(len(pairs), np.uint32)
    counts = np.zeros(len(usym), _lib.MOVE_COUNTS_DTYPE)
    info = np.zeros(1, _lib.MOVE_INFO_DTYPE)
    ctx = ctx or (_lib.default_context() if len(pairs) and band <= _lib.NMZ_ALIGN_WIDE_MAX_BAND
                  and 1 <= G <= _lib.NMZ_PO_MAX_ENTITIES else None)
    _lib.check(_lib.load().nmz_ed_diff_profile_po(ctx.handle if ctx else None, _lib.ptr(ts.off), _lib.ptr(ts.sym),
                                                  _lib.ptr(entity), len(ts), G, _lib.ptr(pairs), len(pairs), band,
                                                  _lib.ptr(usym), len(usym), _lib.ptr(dist),
                                                  _lib.ptr(counts) if len(usym) else None, _lib.ptr(info)))
    return MoveProfile(usym, counts, info[0], dist)


# ---- PO k-NN search: the nearest stored runs by per-entity edit distance ---------------------------------------------
def _po_knn_ctx(ctx, band, k, G, n_queries, n_traces, max_band=_lib.NMZ_PO_KNN_MAX_BAND):
    """The context of a PO search: none where the library answers (or refuses) without a device."""
    if ctx is not None:
        return ctx
    legal = band <= max_band and 1 <= k <= _lib.NMZ_PO_KNN_MAX_K and 1 <= G <= _lib.NMZ_PO_MAX_ENTITIES
    return _lib.default_context() if legal and n_queries and n_traces else None


def po_knn(ts, entity, queries_ts, q_entity, k, band, n_entities=None, q_self=None, ctx=None):
    """The k nearest traces of ts to every trace of queries_ts under ED^PO_band (nmz_po_knn; DESIGN.md section 2,
    "PO k-NN search"): (ids [Q, k], dists [Q, k]) by (distance asc, id asc), pairs beyond the band at band + 1,
    NMZ_NONE where fewer stored traces are eligible. entity / q_entity are parallel to ts.sym / queries_ts.sym, ids
    global to both (po_entities). q_self[Q]: the store index each query skips (NMZ_NONE for none); queries = the
    store with q_self = arange is the all-pairs k-NN. band <= 64, 1 <= k <= 64."""
    return _po_knn(ts, entity, queries_ts, q_entity, k, band, n_entities, q_self, ctx, wide=False)


def po_knn_wide(ts, entity, queries_ts, q_entity, k, band, n_entities=None, q_self=None, ctx=None):
    """po_knn for every band 0 .. 1,024 (nmz_po_knn_wide): a band above 64 searches with K11w, a band <= 64 gives
    po_knn's bytes."""
    return _po_knn(ts, entity, queries_ts, q_entity, k, band, n_entities, q_self, ctx, wide=True)


def _po_knn(ts, entity, queries_ts, q_entity, k, band, n_entities, q_self, ctx, wide):
    band, k = int(band), int(k)
    entity, G1 = _po_entity(int(ts.off[-1]), entity, n_entities)
    q_entity, G2 = _po_entity(int(queries_ts.off[-1]), q_entity, n_entities)
    G = max(G1, G2)
    Q = len(queries_ts)
    if q_self is not None:
        q_self = np.ascontiguousarray(q_self, np.uint32).reshape(-1)
        if len(q_self) < Q:
            raise ValueError(f"{len(q_self)} q_self entries for {Q} queries")
    shape = (Q, min(max(k, 0), _lib.NMZ_PO_KNN_MAX_K))
    ids = np.full(shape, _lib.NMZ_NONE, np.uint32)
    ds = np.full(shape, _lib.NMZ_NONE, np.uint32)
    ctx = _po_knn_ctx(ctx, band, k, G, Q, len(ts),
                      _lib.NMZ_PO_KNN_WIDE_MAX_BAND if wide else _lib.NMZ_PO_KNN_MAX_BAND)
    fn = _lib.load().nmz_po_knn_wide if wide else _lib.load().nmz_po_knn
    _lib.check(fn(ctx.handle if ctx else None, _lib.ptr(ts.off), _lib.ptr(ts.sym), _lib.ptr(entity), len(ts), G,
                  _lib.ptr(queries_ts.off), _lib.ptr(queries_ts.sym), _lib.ptr(q_entity), _lib.ptr(q_self), Q, band, k,
                  _lib.ptr(ids), _lib.ptr(ds)))
    return ids, ds


def po_knn_bounds(a, ea, b, eb, n_entities=None):
    """(LB_len, LB_gram) of one pair on the host (nmz_po_knn_bound_host): the two lower bounds of sum_g Lev(a|g, b|g)
    that the search's filter uses, by their definition."""
    a = np.ascontiguousarray(a, np.uint64).reshape(-1)
    b = np.ascontiguousarray(b, np.uint64).reshape(-1)
    ea, ga = _po_entity(len(a), ea, n_entities)
    eb, gb = _po_entity(len(b), eb, n_entities)
    lb_len, lb_gram = ctypes.c_uint32(), ctypes.c_uint32()
    _lib.check(_lib.load().nmz_po_knn_bound_host(_lib.ptr(a), _lib.ptr(ea), len(a), _lib.ptr(b), _lib.ptr(eb), len(b),
                                                 max(ga, gb), ctypes.byref(lb_len), ctypes.byref(lb_gram)))
    return lb_len.value, lb_gram.value


class PoSimilarityIndex:
    """A stored TraceSet with its entities, projected and profiled once and resident on the GPU for the PO search
    (nmz_po_knn_plan). `names` are the store's entity names (po_entities): names[id]. A query's entities unknown to
    the store all map to the one spare id len(names), and the plan is made with n_entities = len(names) + 1: exact,
    since the store holds nothing there and each such element costs its one DEL whichever unknown entity it has.
    wide=True makes the plan through nmz_po_knn_wide_plan_create: every band 0 .. 1,024 (K11w above 64),
    NMZ_PO_KNN_OPT_FULL_BAND among the opts, and counters() with the five per-C entity-step counts."""

    STEP_NAMES = ("steps_c1", "steps_c2", "steps_c3", "steps_c5", "steps_c9")

    def __init__(self, ts, entity, band, names=(), ctx=None, max_queries=256, max_query_elems=1 << 18, opts=0,
                 n_entities=None, wide=False):
        self.ts = ts
        self.wide = bool(wide)
        self.band = int(band)
        self.names = list(names)
        self._ids = {e: i for i, e in enumerate(self.names)}
        # n_entities: for stores whose ids are numbers already (query_csr); the default leaves the spare id
        self.n_entities = len(self.names) + 1 if n_entities is None else int(n_entities)
        self.entity, _ = _po_entity(int(ts.off[-1]), entity, self.n_entities)
        self.opts = int(opts)
        self.max_queries = int(max_queries)
        max_band = _lib.NMZ_PO_KNN_WIDE_MAX_BAND if self.wide else _lib.NMZ_PO_KNN_MAX_BAND
        legal = self.band <= max_band and self.n_entities <= _lib.NMZ_PO_MAX_ENTITIES
        self.ctx = ctx or (_lib.default_context() if legal else None)
        self.plan = None
        self._create(int(max_query_elems))

    def _create(self, max_query_elems):
        self.close()
        plan = ctypes.c_void_p()
        create = _lib.load().nmz_po_knn_wide_plan_create if self.wide else _lib.load().nmz_po_knn_plan_create
        _lib.check(create(
            self.ctx.handle if self.ctx else None, _lib.ptr(self.ts.off), _lib.ptr(self.ts.sym), _lib.ptr(self.entity),
            len(self.ts), self.n_entities, self.band, self.max_queries, max_query_elems, self.opts, ctypes.byref(plan)))
        self.plan = plan
        self.max_query_elems = max_query_elems

    def info(self):
        """(resident bytes, workgroups, waves) of the plan and its latest search launch."""
        b, g, w = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
        _lib.check(_lib.load().nmz_po_knn_plan_info(self.plan, ctypes.byref(b), ctypes.byref(g), ctypes.byref(w)))
        return b.value, g.value, w.value

    def query_inputs(self, traces):
        """SingleTraces -> (TraceSet, entity[N]) over the store's ids, unknown entities on the spare id."""
        qts = TraceSet([t.symbols for t in traces])
        ent = np.full(max(int(qts.off[-1]), 1), _lib.NMZ_NONE, np.uint32)
        pos = 0
        for t in traces:
            for e in t.entities:
                if e is not None:
                    ent[pos] = self._ids.get(e, len(self.names))
                pos += 1
        return qts, ent

    def query(self, traces, k, q_self=None):
        """traces: SingleTraces carrying entities -> (ids [n, k], dists [n, k]) by (ED^PO_band asc, id asc)."""
        qts, ent = self.query_inputs(traces)
        return self.query_csr(qts, ent, k, q_self)

    def query_csr(self, qts, q_entity, k, q_self=None):
        """The same for a TraceSet and its entity ids (< n_entities or NMZ_NONE)."""
        n, k = len(qts), int(k)
        q_entity, _ = _po_entity(int(qts.off[-1]), q_entity, self.n_entities)
        if q_self is not None:
            q_self = np.ascontiguousarray(q_self, np.uint32).reshape(-1)
            if len(q_self) < n:
                raise ValueError(f"{len(q_self)} q_self entries for {n} queries")
        longest = int(np.diff(qts.off).max()) if n else 0
        if longest > self.max_query_elems:  # a plan whose scratch takes the longest query
            self._create(2 * longest)
        shape = (n, min(max(k, 0), _lib.NMZ_PO_KNN_MAX_K))
        ids = np.full(shape, _lib.NMZ_NONE, np.uint32)
        ds = np.full(shape, _lib.NMZ_NONE, np.uint32)
        _lib.check(_lib.load().nmz_po_knn_query(self.plan, _lib.ptr(qts.off), _lib.ptr(qts.sym), _lib.ptr(q_entity),
                                                _lib.ptr(q_self), n, k, _lib.ptr(ids), _lib.ptr(ds)))
        return ids, ds

    def query_dev(self, d_q_off, d_q_sym, d_q_entity, d_q_self, n_queries, k, d_knn_keys, stream=None):
        """Device pointers (ints; d_q_self may be 0): uint64 keys dist << 32 | id into d_knn_keys[n_queries * k],
        enqueued on `stream`. n_queries <= max_queries, the queries' elements <= max_query_elems."""
        _lib.check(_lib.load().nmz_po_knn_query_dev(
            self.plan, ctypes.c_void_p(d_q_off), ctypes.c_void_p(d_q_sym), ctypes.c_void_p(d_q_entity),
            ctypes.c_void_p(d_q_self) if d_q_self else None, int(n_queries), int(k), ctypes.c_void_p(d_knn_keys),
            ctypes.c_void_p(stream) if stream else None))

    def counters(self, stream=None):
        """The latest search's work: {filtered, length_sum, dp, in_band} pair counts; with wide=True also
        {steps_c1, steps_c2, steps_c3, steps_c5, steps_c9}, the entity steps run at that many cells per thread."""
        names = ("filtered", "length_sum", "dp", "in_band") + (self.STEP_NAMES if self.wide else ())
        out = np.zeros(len(names), np.uint64)
        fn = _lib.load().nmz_po_knn_wide_counters if self.wide else _lib.load().nmz_po_knn_counters
        _lib.check(fn(self.plan, _lib.ptr(out), ctypes.c_void_p(stream) if stream else None))
        return dict(zip(names, (int(v) for v in out)))

    def close(self):
        if self.plan:
            _lib.load().nmz_po_knn_plan_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
