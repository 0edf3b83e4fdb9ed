"""Writes tests/golden/louvain_planted.npz: networkx.planted_partition_graph(16, 32, 0.5, 0.01, seed=1) with integer
weights 1-5 (numpy default_rng(1), in networkx's edge order) as an undirected edge list u < v, and the planted block
of every node (block b holds nodes 32 b .. 32 b + 31). Needs networkx; the tests read only the file."""
import os

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    G = nx.planted_partition_graph(16, 32, 0.5, 0.01, seed=1)
    e = np.array(sorted((min(u, v), max(u, v)) for u, v in G.edges()), dtype=np.int64)
    w = np.random.default_rng(1).integers(1, 6, size=len(e)).astype(np.int64)
    block = np.arange(G.number_of_nodes(), dtype=np.int64) // 32
    for b, members in enumerate(G.graph["partition"]):
        assert sorted(members) == list(range(32 * b, 32 * b + 32))
    out = os.path.join(HERE, "..", "..", "tests", "golden", "louvain_planted.npz")
    np.savez_compressed(out, n=np.int64(G.number_of_nodes()), u=e[:, 0], v=e[:, 1], w=w, block=block)
    print(os.path.normpath(out), len(e), "edges")


if __name__ == "__main__":
    main()
