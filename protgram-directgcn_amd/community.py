"""Louvain communities on the GPU: the trainer's ``community`` task labels (``protgram_directgcn_trainer.py:200-220``,
the default task from n = 4 up, config.py:89-94) and its fallback partitioner (:159-170), DESIGN §11.

The reference hands ``(A_in_w + A_out_w).coalesce()`` through PyG ``to_networkx(to_undirected=True)`` to
python-louvain. Here the same undirected graph is an integer CSR on the device, local moving is the synchronous sweep
kernel ``pg_louvain_move_i64`` (csrc/pg_louvain.hip: every decision from the state at the start of the sweep, exact
128-bit gains), and aggregation between levels is a sort and an integer segmented sum in torch, as graph.py builds its
CSRs. Nothing is drawn at random and every sum is an integer sum: the same graph gives the same labels on every run.
"""
from __future__ import annotations

import ctypes
import time
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from ._lib import check, load_library
from .graph import _rowptr

_MAX_TWO_M = 1 << 61  # head-room: strengths, their sums and the 128-bit gain products stay exact below it


@dataclass
class CommunityGraph:
    """Undirected weighted graph as a symmetric CSR with int64 weights. Both directions of an edge are present; a
    diagonal entry holds TWICE its self-loop's weight, the loop's share of the node's strength (networkx's weighted
    degree counts a self-loop twice), so ``k`` is the plain row sum and aggregation a plain sum."""
    n: int
    rowptr: torch.Tensor  # int64 [n + 1]
    row: torch.Tensor     # int64 [nnz]: the row of every entry
    col: torch.Tensor     # int64 [nnz], ascending inside a row
    w: torch.Tensor       # int64 [nnz], positive
    k: torch.Tensor       # int64 [n]: node strengths
    two_m: int            # sum of the strengths = twice the total edge weight

    def edges(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(u, v, weight) of the undirected edges, u <= v, self-loops with their own weight."""
        m = self.row <= self.col
        u, v, w = self.row[m], self.col[m], self.w[m]
        return u, v, torch.where(u == v, w // 2, w)


def _vp(t: torch.Tensor):
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


def _coalesced(n: int, r: torch.Tensor, c: torch.Tensor, w: torch.Tensor) -> CommunityGraph:
    """CSR of the int64 entries (r, c, w), duplicates summed."""
    if r.numel():
        key, inv = torch.unique(r * n + c, return_inverse=True)  # sorted: by row, then column
        ws = torch.zeros(key.numel(), dtype=torch.int64, device=w.device).index_add_(0, inv, w)
        r, c = key // n, key % n
    else:
        ws = w
    k = torch.zeros(n, dtype=torch.int64, device=w.device).index_add_(0, r, ws)
    return CommunityGraph(n, _rowptr(r, n), r, c, ws, k, int(k.sum()))


def from_undirected(num_nodes: int, u: torch.Tensor, v: torch.Tensor, weight: torch.Tensor) -> CommunityGraph:
    """The graph of the undirected edges (u, v, weight), one entry per edge in either orientation, repeated edges
    summed; `weight`: whole numbers >= 0 (an edge of weight 0 is no edge). IndexError for endpoints outside
    [0, num_nodes), ValueError for weights that are not whole and non-negative or whose total leaves no head-room."""
    n = int(num_nodes)
    u, v, weight = u.reshape(-1), v.reshape(-1), weight.reshape(-1)
    if u.dtype != torch.int64 or v.dtype != torch.int64 or u.shape != v.shape or u.shape != weight.shape:
        raise ValueError("u and v must be int64 [E] and weight [E]")
    if u.numel():
        lo, hi = min(int(u.min()), int(v.min())), max(int(u.max()), int(v.max()))
        if lo < 0 or hi >= n:
            raise IndexError(f"edge endpoints in [{lo}, {hi}] outside [0, {n})")
        if weight.is_floating_point():
            if not bool(torch.isfinite(weight).all()) or bool((weight != weight.round()).any()):
                raise ValueError("edge weights must be whole numbers")
        if bool((weight < 0).any()):
            raise ValueError("edge weights must not be negative")
        # in float64 first: the bound holds for the true total (an int64 sum could wrap past it)
        if 2.0 * float(weight.to(torch.float64).sum()) >= float(_MAX_TWO_M):
            raise ValueError("total edge weight leaves no head-room for exact sums (2m must stay below 2^61)")
    wi = weight.to(torch.int64)
    keep = wi > 0
    u, v, wi = u[keep], v[keep], wi[keep]
    loop = u == v
    # both directions of an edge; a self-loop once, with twice its weight
    r = torch.cat([u, v[~loop]])
    c = torch.cat([v, u[~loop]])
    w2 = torch.cat([torch.where(loop, 2 * wi, wi), wi[~loop]])
    return _coalesced(n, r, c, w2)


def combined_graph(t) -> CommunityGraph:
    """The graph _generate_community_labels hands to Louvain (trainer :206-210) for the level `t`
    (ngram.NgramTransitions): A_in_w + A_out_w, of which to_networkx(to_undirected=True) keeps the entries u <= v --
    one edge of weight a_ij + a_ji for i != j, one self-loop of weight 2 a_ii for a raw self-loop a_ii."""
    from .ngram import _level_device
    n = int(t.num_nodes)
    src, dst, cnt = t.src, t.dst, t.cnt
    if src.dtype != torch.int64 or dst.dtype != torch.int64 or src.dim() != 1 or src.shape != dst.shape \
            or cnt.shape != src.shape:
        raise ValueError("src and dst must be int64 [E] and cnt [E]")
    if src.numel():
        if int(dst.min()) < 0 or int(dst.max()) >= n:
            raise IndexError(f"dst outside [0, {n})")
        if int(src.min()) < 0 or int(src.max()) >= n:
            raise IndexError(f"src outside [0, {n})")
        if cnt.is_floating_point() and (not bool(torch.isfinite(cnt).all()) or bool((cnt != cnt.round()).any())):
            raise ValueError("transition counts must be whole numbers (cnt == cnt.round())")
    _level_device(t, "community labels")
    lo, hi = torch.minimum(src, dst), torch.maximum(src, dst)
    cnt = cnt.to(torch.float64) if cnt.is_floating_point() else cnt
    return from_undirected(n, lo, hi, torch.where(lo == hi, 2 * cnt, cnt))


def _limb_square_sum(x: torch.Tensor) -> int:
    """sum of x^2 as a Python int, for non-negative int64 x below 2^62: 16-bit limbs, so that every partial sum of
    limb products (each below 2^32, fewer than 2^31 of them) fits int64."""
    total = 0
    limbs = [(x >> (16 * a)) & 0xFFFF for a in range(4)]
    for a in range(4):
        for b in range(a, 4):
            s = int((limbs[a] * limbs[b]).sum())
            total += (s if a == b else 2 * s) << (16 * (a + b))
    return total


def _q_terms(g: CommunityGraph, comm: torch.Tensor) -> Tuple[int, int]:
    """(numerator, denominator) of the modularity of `comm` (community ids in [0, n)) as Python ints."""
    if g.two_m == 0:
        return 0, 1
    inside = int(g.w[comm[g.row] == comm[g.col]].sum())  # sum over communities of 2 L_c
    tot = torch.zeros(g.n, dtype=torch.int64, device=comm.device).index_add_(0, comm, g.k)
    return inside * g.two_m - _limb_square_sum(tot), g.two_m * g.two_m


def _q(g: CommunityGraph, comm: torch.Tensor) -> float:
    num, den = _q_terms(g, comm)
    return num / den


def modularity(graph: CommunityGraph, labels: torch.Tensor) -> float:
    """networkx.community.modularity(G, communities, weight=...) of the partition `labels` (any int64 ids, one per
    node): sum over communities of L_c / m - (deg_c / 2m)^2, from exact integer sums and one float64 division. 0.0
    for a graph without edges."""
    labels = labels.reshape(-1).to(graph.k.device)
    if labels.numel() != graph.n:
        raise ValueError(f"labels must have one entry per node ({graph.n})")
    if graph.n == 0:
        return 0.0
    return _q(graph, torch.unique(labels, return_inverse=True)[1])


def sweep(graph: CommunityGraph, comm: torch.Tensor, classes: int, cls: int,
          moved: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One launch of pg_louvain_move_i64 from the communities `comm` (int64 [n], ids in [0, n)): (comm_out, moved), the
    device int64 counter `moved` (a fresh zero when not given) grown by the number of nodes that moved."""
    dev = graph.k.device
    if dev.type != "cuda":
        raise RuntimeError("the Louvain sweep runs on the MI355X only: the graph must be on the GPU (no CPU fallback)")
    n = graph.n
    comm = comm.contiguous()
    if comm.dtype != torch.int64 or comm.shape != (n,) or comm.device != dev:
        raise ValueError("comm must be int64 [n] on the graph's device")
    if n and (int(comm.min()) < 0 or int(comm.max()) >= n):
        raise IndexError(f"community ids outside [0, {n})")
    if moved is None:
        moved = torch.zeros(1, dtype=torch.int64, device=dev)
    if n == 0:
        return torch.empty_like(comm), moved
    return _move(graph, comm, int(classes), int(cls), moved), moved


def _move(graph: CommunityGraph, comm: torch.Tensor, classes: int, cls: int, moved: torch.Tensor,
          events: Optional[list] = None) -> torch.Tensor:
    """The launch behind sweep(), arguments unchecked: per-community strength sums and sizes, then the kernel
    (`events`: receives a pair of timing events around the launch)."""
    dev, n = comm.device, graph.n
    out = torch.empty_like(comm)
    tot = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, comm, graph.k)
    size = torch.bincount(comm, minlength=n)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    if events is not None:
        events.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
        events[-1][0].record()
    nul = graph.rowptr  # an empty col / w has no address: every row is empty then and any pointer stands in
    check(load_library().pg_louvain_move_i64(n, _vp(graph.rowptr), _vp(graph.col) or _vp(nul), _vp(graph.w) or _vp(nul),
                                             _vp(graph.k), _vp(comm), _vp(tot), _vp(size), graph.two_m, classes, cls,
                                             _vp(out), _vp(moved), stream), "pg_louvain_move_i64")
    if events is not None:
        events[-1][1].record()
    return out


def _aggregate(g: CommunityGraph, comm: torch.Tensor) -> Tuple[CommunityGraph, torch.Tensor]:
    """The level's communities as the nodes of the next graph (numbered in ascending order of their ids) and the map
    node -> new node. An entry of the coarse CSR is the plain sum of the fine entries between the two communities:
    the diagonal collects both directions of the inner edges and the inner diagonals, twice the coarse self-loop."""
    inv = torch.unique(comm, return_inverse=True)[1]
    c = int(inv.max()) + 1
    coarse = _coalesced(c, inv[g.row], inv[g.col], g.w)
    return coarse, inv


def _number_by_smallest_member(labels: torch.Tensor) -> torch.Tensor:
    n = labels.numel()
    ids, inv = torch.unique(labels, return_inverse=True)
    first = torch.full((ids.numel(),), n, dtype=torch.int64, device=labels.device)
    first.scatter_reduce_(0, inv, torch.arange(n, device=labels.device), reduce="amin")
    rank = torch.empty_like(first)
    rank[torch.argsort(first)] = torch.arange(ids.numel(), device=labels.device)
    return rank[inv]


def louvain(graph: CommunityGraph, *, classes: int = 4, max_sweeps: int = 64, max_levels: int = 32,
            min_gain: float = 1e-7, stats: Optional[list] = None) -> torch.Tensor:
    """Louvain communities of `graph`: int64 [n] on its device, communities numbered 0..C-1 in ascending order of their
    smallest member. Per level, cycles of `classes` sweeps (one per class of the node hash, so neighbours mostly decide
    in different sweeps) until a cycle moves nothing, gains less than `min_gain` in modularity (python-louvain's
    __MIN; a cycle that lowers it is dropped) or `max_sweeps` cycles have run; then the communities become the nodes
    of the next level, until a level gains less than `min_gain` or `max_levels` have run. `stats`: a list that
    receives one dict per level (nodes, cycles, launches, moved, q, milliseconds in the sweep kernel by device events,
    seconds in the level's cycles as a whole and in the aggregation; timing synchronises the device)."""
    if classes < 1 or max_sweeps < 1 or max_levels < 1:
        raise ValueError("classes, max_sweeps and max_levels must be at least 1")
    dev = graph.k.device
    if dev.type != "cuda":
        raise RuntimeError("louvain runs on the MI355X only: the graph must be on the GPU (no CPU fallback)")
    assign = torch.arange(graph.n, dtype=torch.int64, device=dev)
    if graph.n == 0 or graph.two_m == 0:
        return assign

    def now():
        if stats is not None:
            torch.cuda.synchronize(dev)
        return time.perf_counter()

    g = graph
    q = _q(g, assign)
    for _ in range(max_levels):
        comm = torch.arange(g.n, dtype=torch.int64, device=dev)
        q_level, cycles, moved_all = q, 0, 0
        events = [] if stats is not None else None
        t0 = now()
        for _ in range(max_sweeps):
            new, counter = comm, torch.zeros(1, dtype=torch.int64, device=dev)
            for cls in range(classes):
                new = _move(g, new, classes, cls, counter, events)
            moved = int(counter)
            cycles += 1
            if not moved:
                break
            moved_all += moved
            q_new = _q(g, new)
            if q_new > q_level:
                comm = new
            gain, q_level = q_new - q_level, max(q_new, q_level)
            if gain < min_gain:
                break
        if stats is not None:
            level = {"nodes": g.n, "entries": int(g.col.numel()), "cycles": cycles, "launches": len(events),
                     "moved": moved_all, "q": q_level, "kernel_ms": sum(a.elapsed_time(b) for a, b in events),
                     "cycles_s": now() - t0, "aggregate_s": 0.0}
            stats.append(level)
        if q_level - q < min_gain:
            break
        q = q_level
        t0 = now()
        g, inv = _aggregate(g, comm)
        assign = inv[assign]
        if stats is not None:
            level["aggregate_s"] = now() - t0
            level["communities"] = g.n
    return _number_by_smallest_member(assign)
