"""Yardstick for the community labels (numpy / plain Python, never the package): the graph the trainer hands to Louvain
(protgram_directgcn_trainer.py:200-212), networkx's modularity formula on exact integers, a plain sequential Louvain
(Blondel et al.: local moving in a seeded random node order, then aggregation), and a restatement of the contract of
one synchronous sweep (include/pg_directgcn.h, pg_louvain_move_i64) together with the level loop around it.

Graph rule: the trainer adds A_in_w (a_ji at [i, j]) and A_out_w (a_ij) and PyG's to_networkx(to_undirected=True) keeps
the entries with u <= v: one undirected edge of weight a_ij + a_ji for i != j, one self-loop of weight 2 a_ii for a raw
self-loop. An undirected graph is a dict {(u, v): weight} with u <= v and Python ints. Its CSR holds both directions of
an edge; a diagonal entry holds TWICE the self-loop's weight, its share of the node's strength (networkx's weighted
degree counts a self-loop twice), so a strength is a plain row sum and aggregation a plain sum."""
import random

import numpy as np

HASH_MUL = 0x9E3779B97F4A7C15


def node_class(i: int, classes: int) -> int:
    return (((i * HASH_MUL) & 0xFFFFFFFFFFFFFFFF) >> 32) % classes


def undirected_edges(src, dst, cnt):
    """{(u, v): w}, u <= v, from raw transition counts a[src -> dst] (whole numbers)."""
    edges = {}
    for s, d, c in zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(cnt).tolist()):
        c = int(c)
        if c == 0:
            continue
        key = (min(s, d), max(s, d))
        edges[key] = edges.get(key, 0) + (2 * c if s == d else c)
    return edges


def csr(n, edges):
    """(rowptr, col, w, k): lists of Python ints; rows sorted by column."""
    rows = [[] for _ in range(n)]
    for (u, v), w in edges.items():
        if u == v:
            rows[u].append((u, 2 * w))
        else:
            rows[u].append((v, w))
            rows[v].append((u, w))
    rowptr, col, wt, k = [0], [], [], []
    for r in rows:
        r.sort()
        col += [c for c, _ in r]
        wt += [w for _, w in r]
        k.append(sum(w for _, w in r))
        rowptr.append(len(col))
    return rowptr, col, wt, k


def strengths(n, edges):
    return csr(n, edges)[3]


def modularity(n, edges, labels) -> float:
    """networkx.community.modularity(G, communities, weight=...) of the partition `labels`, from integer sums."""
    labels = np.asarray(labels).tolist()
    k = [0] * n
    inside = 0  # sum over communities of 2 L_c
    for (u, v), w in edges.items():
        k[u] += w
        k[v] += w
        if labels[u] == labels[v]:
            inside += 2 * w
    two_m = sum(k)
    tot = {}
    for i in range(n):
        tot[labels[i]] = tot.get(labels[i], 0) + k[i]
    return (inside * two_m - sum(t * t for t in tot.values())) / (two_m * two_m)


def number_by_smallest_member(labels):
    seen = {}
    return np.array([seen.setdefault(c, len(seen)) for c in np.asarray(labels).tolist()], dtype=np.int64)


# ---- the sequential algorithm ------------------------------------------------------------------------------------

def _one_level_seq(n, rowptr, col, w, k, two_m, order, min_gain):
    comm = list(range(n))
    tot = list(k)
    improved = False
    q = _q_csr(n, rowptr, col, w, k, two_m, comm)
    while True:
        moved = 0
        for i in order:
            ci, ki = comm[i], k[i]
            acc = {}
            for e in range(rowptr[i], rowptr[i + 1]):
                j = col[e]
                if j != i:
                    acc[comm[j]] = acc.get(comm[j], 0) + w[e]
            tot[ci] -= ki
            best_c, best_g = ci, two_m * acc.get(ci, 0) - tot[ci] * ki
            for c, wc in acc.items():
                g = two_m * wc - tot[c] * ki
                if g > best_g:
                    best_c, best_g = c, g
            tot[best_c] += ki
            if best_c != ci:
                comm[i] = best_c
                moved += 1
        if not moved:
            break
        q_new = _q_csr(n, rowptr, col, w, k, two_m, comm)
        gain, q = q_new - q, q_new
        improved = True
        if gain < min_gain:
            break
    return comm, improved


def _q_csr(n, rowptr, col, w, k, two_m, comm):
    inside = 0
    tot = {}
    for i in range(n):
        ci = comm[i]
        tot[ci] = tot.get(ci, 0) + k[i]
        for e in range(rowptr[i], rowptr[i + 1]):
            if comm[col[e]] == ci:
                inside += w[e]
    return (inside * two_m - sum(t * t for t in tot.values())) / (two_m * two_m) if two_m else 0.0


def _aggregate(n, rowptr, col, w, k, comm):
    """Communities renumbered 0..C-1 in ascending order of their id; the coarse CSR is the plain sum of the entries."""
    ids = sorted(set(comm))
    new = {c: a for a, c in enumerate(ids)}
    inv = [new[c] for c in comm]
    C = len(ids)
    rows = [{} for _ in range(C)]
    kk = [0] * C
    for i in range(n):
        a = inv[i]
        kk[a] += k[i]
        for e in range(rowptr[i], rowptr[i + 1]):
            b = inv[col[e]]
            rows[a][b] = rows[a].get(b, 0) + w[e]
    rp, cc, ww = [0], [], []
    for r in rows:
        for b in sorted(r):
            cc.append(b)
            ww.append(r[b])
        rp.append(len(cc))
    return C, rp, cc, ww, kk, inv


def louvain_seq(n, edges, seed=0, min_gain=1e-7):
    """Sequential Louvain; labels numbered by smallest member."""
    rng = random.Random(seed)
    rowptr, col, w, k = csr(n, edges)
    two_m = sum(k)
    assign = list(range(n))
    m = n
    while two_m:
        order = list(range(m))
        rng.shuffle(order)
        comm, improved = _one_level_seq(m, rowptr, col, w, k, two_m, order, min_gain)
        if not improved:
            break
        m, rowptr, col, w, k, inv = _aggregate(m, rowptr, col, w, k, comm)
        assign = [inv[a] for a in assign]
    return number_by_smallest_member(assign)


# ---- the synchronous scheme: one sweep's contract, and the loop around it -------------------------------------------

def sweep(rowptr, col, w, k, comm, classes, cls):
    """(comm_out, moved) of one synchronous sweep: every decision from `comm` as given."""
    n = len(k)
    comm = np.asarray(comm).tolist()
    tot, size = [0] * n, [0] * n
    for i in range(n):
        tot[comm[i]] += k[i]
        size[comm[i]] += 1
    two_m = sum(k)
    out, moved = list(comm), 0
    for i in range(n):
        if node_class(i, classes) != cls:
            continue
        ci, ki = comm[i], k[i]
        acc = {}
        for e in range(rowptr[i], rowptr[i + 1]):
            j = col[e]
            if j != i:
                acc[comm[j]] = acc.get(comm[j], 0) + w[e]
        stay = two_m * acc.get(ci, 0) - (tot[ci] - ki) * ki
        best = None
        for c, wc in acc.items():
            if c == ci or (size[ci] == 1 and size[c] == 1 and c > ci):
                continue
            g = two_m * wc - tot[c] * ki
            if best is None or g > best[0] or (g == best[0] and c < best[1]):
                best = (g, c)
        if best is not None and best[0] > stay:
            out[i] = best[1]
            moved += 1
    return out, moved


def louvain_sync(n, edges, classes=4, max_sweeps=64, max_levels=32, min_gain=1e-7):
    """The level loop of community.louvain over `sweep`: a prototype of the synchronous scheme."""
    rowptr, col, w, k = csr(n, edges)
    two_m = sum(k)
    assign = list(range(n))
    m = n
    if not two_m:
        return number_by_smallest_member(assign)
    q = _q_csr(m, rowptr, col, w, k, two_m, list(range(m)))
    for _ in range(max_levels):
        comm, q_level = list(range(m)), q
        for _ in range(max_sweeps):
            new, moved = comm, 0
            for cls in range(classes):
                new, mv = sweep(rowptr, col, w, k, new, classes, cls)
                moved += mv
            if not moved:
                break
            q_new = _q_csr(m, rowptr, col, w, k, two_m, new)
            if q_new > q_level:
                comm = new
            gain, q_level = q_new - q_level, max(q_new, q_level)
            if gain < min_gain:
                break
        if q_level - q < min_gain:
            break
        q = q_level
        m, rowptr, col, w, k, inv = _aggregate(m, rowptr, col, w, k, comm)
        assign = [inv[a] for a in assign]
    return number_by_smallest_member(assign)
