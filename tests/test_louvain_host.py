"""Community labels, host side (no GPU): the yardstick louvain_ref.py against networkx (modularity, the graph the
trainer hands to Louvain, the band of Q that re-seeding the sequential algorithm gives), the package's graph
construction and modularity in their torch form on the CPU, its argument errors before any launch, no CPU fallback,
and the task_labels dispatch."""
import numpy as np
import pytest
import torch

import louvain_ref as ref
from golden_util import load

# raw transitions with a raw self-loop ("AA -> AA"), a one-directional edge and a mutual pair
STRINGS = ["AA", "AC", "CA", "CC", "CD"]
SRC = [0, 0, 1, 2, 2, 3]
DST = [0, 1, 2, 0, 1, 4]
CNT = [3, 2, 5, 4, 1, 7]
# node 0: loop of weight 6, edges to 1 (2) and 2 (4); 1-2 mutual: 5 + 1; 3-4 one-directional: 7
EDGES = {(0, 0): 6, (0, 1): 2, (0, 2): 4, (1, 2): 6, (3, 4): 7}


def level_edges(pkg, n, nseq, mean_len, seed):
    """(N, {(u, v): w}) of the padded builder's level n, built on the host."""
    seqs = pkg.ngram.preprocess(pkg.synth.protein_sequences(nseq, mean_len=mean_len, seed=seed))
    N, s, d, c, _ = pkg.synth.fasta_edges(n, seqs)
    return N, ref.undirected_edges(s, d, c)


def nx_graph(n, edges):
    import networkx as nx
    G = nx.Graph()
    G.add_nodes_from(range(n))
    for (u, v), w in edges.items():
        G.add_edge(u, v, weight=w)
    return G


def nx_q(G, labels):
    import networkx as nx
    comms = {}
    for i, c in enumerate(np.asarray(labels).tolist()):
        comms.setdefault(c, set()).add(i)
    return nx.community.modularity(G, list(comms.values()), weight="weight")


@pytest.fixture(scope="module")
def levels(pkg):
    out = {}
    for name, args in (("2gram", (2, 60, 120, 1)), ("3gram", (3, 150, 200, 2))):
        N, edges = level_edges(pkg, *args)
        qs = [ref.modularity(N, edges, ref.louvain_seq(N, edges, seed)) for seed in range(5)]
        out[name] = (N, edges, qs)
    return out


def test_levels_are_the_ones_the_bar_is_stated_for(levels):
    N, edges, _ = levels["2gram"]
    assert (N, len(edges), sum(u == v for u, v in edges)) == (424, 3804, 13)
    N, edges, _ = levels["3gram"]
    assert (N, len(edges)) == (6903, 25339)


def test_restated_graph_is_the_upper_triangle_of_the_sum():
    import networkx as nx
    assert ref.undirected_edges(SRC, DST, CNT) == EDGES
    A = np.zeros((5, 5), dtype=np.int64)
    A[SRC, DST] = CNT
    S = A + A.T  # A_out_w + A_in_w
    G = nx.Graph()
    G.add_nodes_from(range(5))
    for u in range(5):
        for v in range(u, 5):  # to_networkx(to_undirected=True) keeps u <= v
            if S[u, v]:
                G.add_edge(u, v, weight=int(S[u, v]))
    got = nx_graph(5, ref.undirected_edges(SRC, DST, CNT))
    assert {(min(u, v), max(u, v)): d["weight"] for u, v, d in got.edges(data=True)} == \
           {(min(u, v), max(u, v)): d["weight"] for u, v, d in G.edges(data=True)}
    assert G.number_of_edges() == 5 and G[0][0]["weight"] == 6
    rowptr, col, w, k = ref.csr(5, EDGES)
    assert k == [G.degree(i, weight="weight") for i in range(5)] == [18, 8, 10, 7, 7]
    assert rowptr == [0, 3, 5, 7, 8, 9] and col == [0, 1, 2, 0, 2, 0, 1, 4, 3]
    assert w == [12, 2, 4, 2, 6, 4, 6, 7, 7]  # the diagonal entry: twice the loop, its share of the strength


def test_restated_modularity_is_networkx_modularity(levels):
    rng = np.random.default_rng(0)
    cases = [(5, EDGES)] + [levels[k][:2] for k in ("2gram", "3gram")]
    for n, edges in cases:
        G = nx_graph(n, edges)
        for labels in (np.arange(n), np.zeros(n, dtype=np.int64), rng.integers(0, 7, size=n), np.arange(n) // 3):
            assert abs(ref.modularity(n, edges, labels) - nx_q(G, labels)) < 1e-12
    N, edges, _ = levels["2gram"]
    lab = ref.louvain_seq(N, edges, 0)
    assert abs(ref.modularity(N, edges, lab) - nx_q(nx_graph(N, edges), lab)) < 1e-12
    assert np.array_equal(lab, ref.number_by_smallest_member(lab))


@pytest.mark.parametrize("name", ["2gram", "3gram"])
def test_sequential_q_band_overlaps_networkx_louvain(levels, name):
    import networkx as nx
    N, edges, qs = levels[name]
    G = nx_graph(N, edges)
    nq = [nx.community.modularity(G, nx.community.louvain_communities(G, weight="weight", seed=s), weight="weight")
          for s in range(5)]
    print(f"{name}: louvain_ref Q {min(qs):.4f}-{max(qs):.4f}, networkx Q {min(nq):.4f}-{max(nq):.4f}")
    assert max(qs) >= min(nq) and max(nq) >= min(qs)


def test_prototypes_recover_the_planted_partition():
    fx = load("louvain_planted")
    n = int(fx["n"])
    edges = {(int(u), int(v)): int(w) for u, v, w in zip(fx["u"], fx["v"], fx["w"])}
    assert n == 512 and len(edges) == 5161 and set(fx["w"].tolist()) == {1, 2, 3, 4, 5}
    assert np.array_equal(ref.louvain_seq(n, edges, 0), fx["block"])
    assert np.array_equal(ref.louvain_sync(n, edges, classes=4), fx["block"])


def test_sweep_restatement_small():
    """Two triangles joined by an edge, from singletons, one class: every node takes its best neighbour at once (ties to
    the smallest id), except where the swap rule holds a singleton back from a larger singleton."""
    edges = {(0, 1): 1, (0, 2): 1, (1, 2): 1, (2, 3): 1, (3, 4): 1, (3, 5): 1, (4, 5): 1}
    rowptr, col, w, k = ref.csr(6, edges)
    out, moved = ref.sweep(rowptr, col, w, k, list(range(6)), 1, 0)
    # k = [2, 2, 3, 3, 2, 2], 2m = 14. 0: both candidates are larger singletons, stays. 1 -> 0 (2 is held back).
    # 2: gain(0) = gain(1) = 14 - 2 * 3, the smaller id. 3 -> 2 (4, 5 held back). 4 -> 3. 5: gain(4) = 10 > gain(3) = 8.
    assert out == [0, 0, 0, 2, 3, 4] and moved == 5
    assert ref.sweep(rowptr, col, w, k, list(range(6)), 4, 0)[0] == \
           [out[i] if ref.node_class(i, 4) == 0 else i for i in range(6)]
    assert ref.node_class(5, 1) == 0 and {ref.node_class(i, 4) for i in range(64)} == {0, 1, 2, 3}
    assert ref.node_class(1, 1 << 32) == 0x9E3779B9  # the multiplier's high word: hash(i) = (i * M mod 2^64) >> 32


def test_package_graph_and_modularity_on_the_cpu(pkg, levels):
    """from_undirected and modularity are torch ops: on the CPU they give the yardstick's CSR and Q."""
    cm = pkg.community
    for n, edges in ((5, EDGES), levels["2gram"][:2]):
        u = torch.tensor([e[0] for e in edges], dtype=torch.int64)
        v = torch.tensor([e[1] for e in edges], dtype=torch.int64)
        w = torch.tensor(list(edges.values()), dtype=torch.int64)
        g = cm.from_undirected(n, v, u, w)  # either orientation
        rowptr, col, wt, k = ref.csr(n, edges)
        assert g.rowptr.tolist() == rowptr and g.col.tolist() == col and g.w.tolist() == wt and g.k.tolist() == k
        assert g.two_m == sum(k) == 2 * sum(edges.values())
        eu, ev, ew = g.edges()
        assert dict(zip(zip(eu.tolist(), ev.tolist()), ew.tolist())) == edges
        for labels in (np.arange(n), np.arange(n) // 3, np.arange(n) % 5 * 10):
            assert abs(cm.modularity(g, torch.from_numpy(labels)) - ref.modularity(n, edges, labels)) < 1e-12
    g = cm.from_undirected(3, torch.tensor([0, 0]), torch.tensor([1, 1]), torch.tensor([2.0, 0.0]))
    assert g.col.tolist() == [1, 0] and g.w.tolist() == [2, 2]
    assert cm.modularity(g, torch.zeros(3, dtype=torch.int64)) == 0.0
    big = torch.tensor([1 << 40, (1 << 40) + 3, 5], dtype=torch.int64)
    assert cm._limb_square_sum(big) == sum(int(x) ** 2 for x in big.tolist())


def test_validation_errors(pkg):
    ng, cm = pkg.ngram, pkg.community
    t = ng.transitions_from_table(2, SRC, DST, CNT, STRINGS)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cm.combined_graph(t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ng.community_labels(t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ng.task_labels(t, "community", method="louvain")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ng.community_labels(ng.transitions_from_table(2, [], [], [], []))
    bad = ng.transitions_from_table(2, SRC, DST, [3, 2, 5.5, 4, 1, 7], STRINGS)
    with pytest.raises(ValueError, match="whole numbers"):
        cm.combined_graph(bad)
    for s, d in (([0, 5], [1, 1]), ([0, 1], [1, -1])):
        with pytest.raises(IndexError, match="outside"):
            cm.combined_graph(ng.transitions_from_table(2, s, d, [1, 1], STRINGS))
    one = torch.tensor([0], dtype=torch.int64)
    with pytest.raises(IndexError):
        cm.from_undirected(1, one, one + 1, one)
    with pytest.raises(ValueError, match="whole"):
        cm.from_undirected(2, one, one + 1, torch.tensor([0.5]))
    with pytest.raises(ValueError, match="negative"):
        cm.from_undirected(2, one, one + 1, torch.tensor([-1]))
    with pytest.raises(ValueError, match="head-room"):
        cm.from_undirected(2, one, one + 1, torch.tensor([1 << 60]))
    g = cm.from_undirected(2, one, one + 1, one + 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cm.louvain(g)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cm.sweep(g, torch.arange(2), 1, 0)
    with pytest.raises(ValueError):
        cm.modularity(g, torch.zeros(3, dtype=torch.int64))


def test_task_labels_dispatch(pkg, monkeypatch):
    ng = pkg.ngram
    t = ng.transitions_from_table(2, SRC, DST, CNT, STRINGS)
    seen = {}
    monkeypatch.setattr(ng, "community_labels", lambda tt, **kw: seen.update(kw, t=tt) or ("labels", 3))
    assert ng.task_labels(t, "community", method="louvain", classes=8) == ("labels", 3)
    assert seen == {"classes": 8, "t": t}
    with pytest.raises(ValueError, match="Louvain.*community_labels"):
        ng.task_labels(t, "community")
    with pytest.raises(ValueError, match="Louvain"):
        ng.task_labels(t, "community", method="metis")
    with pytest.raises(ValueError, match="method"):
        ng.task_labels(t, "next_node", method="louvain")
    assert ng.task_labels(t, "next_node")[1] == 5


def test_move_abi_argument_errors_without_gpu(pkg):
    lib = pkg.load_library()
    a, b = np.zeros(64, dtype=np.int64), np.zeros(64, dtype=np.int64)
    buf, other = a.ctypes.data, b.ctypes.data
    assert lib.pg_louvain_row_capacity() >= 128

    def move(n=8, rowptr=buf, col=buf, w=buf, k=buf, cin=buf, tot=buf, size=buf, two_m=10, classes=4, cls=0,
             cout=other, moved=other + 256):
        return lib.pg_louvain_move_i64(n, rowptr, col, w, k, cin, tot, size, two_m, classes, cls, cout, moved, None)

    assert move(n=-1) == -1 and move(n=1 << 31) == -1 and b"n_rows" in lib.pg_last_error()
    for kw in (dict(classes=0), dict(cls=4), dict(cls=-1)):
        assert move(**kw) == -1 and b"class" in lib.pg_last_error(), kw
    for kw in (dict(two_m=-1), dict(two_m=1 << 62)):
        assert move(**kw) == -1 and b"two_m" in lib.pg_last_error(), kw
    for name in ("rowptr", "col", "w", "k", "cin", "tot", "size", "cout", "moved"):
        assert move(**{name: None}) == -1 and b"null" in lib.pg_last_error(), name
    assert move(cout=buf) == -1 and b"overlap" in lib.pg_last_error()
    assert move(cout=buf + 56) == -1 and b"overlap" in lib.pg_last_error()
    assert move(n=0, rowptr=None, col=None, w=None, k=None, cin=None, tot=None, size=None, cout=None, moved=None) == 0
