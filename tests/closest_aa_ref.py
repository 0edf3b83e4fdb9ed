"""Plain-Python restatement of the trainer's closest_aa labels (protgram_directgcn_trainer.py:239-269), written from
its semantics and deliberately NOT as the product's bitmask recurrence: one breadth-first search per node over the
out-edges in (source, target) order, with a FIFO queue, a visited set that holds the start node, and the hop cut-off
(a node at hop k_hops is not expanded; a neighbour found at hop + 1 = k_hops is still tested but not queued)."""
import collections

import numpy as np

AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"


def successors(num_nodes, src, dst):
    """Out-neighbour lists in the order of a coalesced sparse matrix's entries: by (source, target)."""
    out = [[] for _ in range(num_nodes)]
    for s, d in sorted(zip((int(x) for x in src), (int(x) for x in dst))):
        out[s].append(d)
    return out


def bfs_label(start, letter, succ, strings, k_hops):
    if letter in strings[start]:
        return 0
    if k_hops <= 0:
        return k_hops
    q = collections.deque([(start, 0)])
    visited = {start}
    while q:
        cur, hop = q.popleft()
        if hop >= k_hops:
            continue
        for nb in succ[cur]:
            if nb in visited:
                continue
            visited.add(nb)
            if letter in strings[nb]:
                return hop + 1
            if hop + 1 < k_hops:
                q.append((nb, hop + 1))
    return k_hops


def labels(num_nodes, src, dst, strings, targets, k_hops, letters=AMINO_ACIDS):
    """(int64 [N] labels, num_classes): targets[i] is node i's target letter index."""
    if num_nodes == 0:
        return np.zeros(0, dtype=np.int64), k_hops + 1
    succ = successors(num_nodes, src, dst)
    out = [bfs_label(i, letters[int(targets[i])], succ, strings, k_hops) for i in range(num_nodes)]
    return np.asarray(out, dtype=np.int64), k_hops + 1


def distances(num_nodes, src, dst, strings, k_hops, letters=AMINO_ACIDS):
    """uint8 [N, len(letters)]: the label of every (node, letter) pair, one search each."""
    succ = successors(num_nodes, src, dst)
    out = np.zeros((num_nodes, len(letters)), dtype=np.uint8)
    for i in range(num_nodes):
        for b, ch in enumerate(letters):
            out[i, b] = bfs_label(i, ch, succ, strings, k_hops)
    return out


def masks(strings, letters=AMINO_ACIDS):
    """uint32 [N]: bit b set when the string contains letters[b]."""
    return np.asarray([sum(1 << b for b, ch in enumerate(letters) if ch in s) for s in strings], dtype=np.uint32)
