"""Louvain communities on the GPU (community.py, csrc/pg_louvain.hip) against the yardstick tests/louvain_ref.py:
one sweep bit for bit on graphs that reach every row path and boundary, the planted partition, the modularity bar on
two builder levels, the contract of the labels, the fallback partitioner, and one training step on the labels."""
import numpy as np
import pytest
import torch

import louvain_ref as ref
from golden_util import load

pytestmark = pytest.mark.gpu

WAVE_CAP = 64  # entries of a row that one wave takes (include/pg_directgcn.h)


def to_graph(pkg, cuda, n, edges):
    u = torch.tensor([e[0] for e in edges], dtype=torch.int64, device=cuda)
    v = torch.tensor([e[1] for e in edges], dtype=torch.int64, device=cuda)
    w = torch.tensor(list(edges.values()), dtype=torch.int64, device=cuda)
    return pkg.community.from_undirected(n, u, v, w)


def host_level(pkg, n, nseq, mean_len, seed):
    seqs = pkg.synth.protein_sequences(nseq, mean_len=mean_len, seed=seed)
    N, s, d, c, _ = pkg.synth.fasta_edges(n, pkg.ngram.preprocess(seqs))
    return seqs, N, ref.undirected_edges(s, d, c)


def random_graph(n, p, seed, weight):
    rng = np.random.default_rng(seed)
    edges = {}
    for u in range(n):
        for v in np.flatnonzero(rng.random(n - u - 1) < p).tolist():
            edges[(u, u + 1 + v)] = int(weight(rng))
    return edges


def star_graph(cap):
    """Centres whose rows hold 0, 1, 63, 64, 65, cap - 1, cap, cap + 1 entries (both sides of the wave path's and of the
    workgroup table's capacity), each with leaves of its own, three of them with a self-loop among the entries (one per
    row path), and a hub with cap + 37 neighbours spread over every fourth node, so that from singletons its
    neighbours' communities are all distinct and span more ids than one range pass holds. Weights 1-5."""
    rng = np.random.default_rng(7)
    edges, n, centres = {}, 0, set()
    for entries, loop in ((0, False), (1, False), (63, False), (64, True), (64, False), (65, False), (cap - 1, False),
                          (cap, True), (cap, False), (cap + 1, False)):
        centre, n = n, n + 1
        centres.add(centre)
        if loop:
            edges[(centre, centre)] = int(rng.integers(1, 6))
        for _ in range(entries - loop):
            edges[(centre, n)] = int(rng.integers(1, 6))
            n += 1
    hub, n = n, n + 1
    edges[(hub, hub)] = 3
    leaves = [i for i in range(hub) if i not in centres][::4][:cap + 37]
    assert len(leaves) == cap + 37 and leaves[-1] - leaves[0] > 4096
    for v in leaves:
        edges[(v, hub)] = int(rng.integers(1, 6))
    return n, edges, hub


def check_sweeps(pkg, cuda, n, edges, starts=("singletons", "coarsened")):
    """comm_out and the move count of every (classes, cls) in {1, 4} x all, from each starting state."""
    g = to_graph(pkg, cuda, n, edges)
    rowptr, col, w, k = ref.csr(n, edges)
    assert g.rowptr.tolist() == rowptr and g.col.tolist() == col and g.w.tolist() == w and g.k.tolist() == k
    states = {"singletons": list(range(n))}
    coarse = states["singletons"]
    for cls in range(4):  # one cycle of the yardstick: communities of many sizes, sparse ids
        coarse, _ = ref.sweep(rowptr, col, w, k, coarse, 4, cls)
    states["coarsened"] = coarse
    assert len(set(coarse)) < n
    total = 0
    for name in starts:
        comm = torch.tensor(states[name], dtype=torch.int64, device=cuda)
        for classes in (1, 4):
            for cls in range(classes):
                want, moved = ref.sweep(rowptr, col, w, k, states[name], classes, cls)
                got, counter = pkg.community.sweep(g, comm, classes, cls)
                have = got.cpu().numpy()
                bad = np.flatnonzero(have != np.array(want))
                assert bad.size == 0, (name, classes, cls, bad[:8], [want[i] for i in bad[:8]], have[bad[:8]])
                assert int(counter) == moved, (name, classes, cls)
                total += moved
    assert total > 0
    return g


def test_sweep_2gram_level(pkg, cuda):
    _, N, edges = host_level(pkg, 2, 60, 120, 1)
    g = check_sweeps(pkg, cuda, N, edges)
    assert int((g.rowptr[1:] - g.rowptr[:-1]).max()) <= WAVE_CAP  # the wave path alone
    assert int((g.row == g.col).sum()) == 13  # diagonal entries


@pytest.mark.parametrize("p", [0.05, 0.4], ids=["wave_rows", "workgroup_rows"])
def test_sweep_unit_weights_many_ties(pkg, cuda, p):
    """All weights 1: many exactly equal gains, decided by the smallest id. p = 0.4 gives rows of about 120 entries,
    which take the workgroup's hash table with up to a row's worth of distinct communities in it."""
    g = check_sweeps(pkg, cuda, 300, random_graph(300, p, 3, lambda rng: 1))
    assert (int((g.rowptr[1:] - g.rowptr[:-1]).min()) > WAVE_CAP) == (p == 0.4)


def test_sweep_row_capacities_and_hub(pkg, cuda):
    cap = int(pkg.load_library().pg_louvain_row_capacity())
    assert cap > WAVE_CAP + 1
    n, edges, hub = star_graph(cap)
    g = check_sweeps(pkg, cuda, n, edges)
    deg = (g.rowptr[1:] - g.rowptr[:-1]).tolist()
    assert {0, 1, 63, 64, 65, cap - 1, cap, cap + 1} <= set(deg) and deg[hub] == cap + 38  # + its diagonal entry


def test_sweep_weights_near_2_40(pkg, cuda):
    edges = random_graph(200, 0.06, 5, lambda rng: (1 << 40) + int(rng.integers(0, 1000)))
    g = check_sweeps(pkg, cuda, 200, edges)
    assert g.two_m * min(edges.values()) > 1 << 64  # the gain's products need more than 64 bits


def test_planted_partition(pkg, cuda):
    fx = load("louvain_planted")
    n = int(fx["n"])
    edges = {(int(u), int(v)): int(w) for u, v, w in zip(fx["u"], fx["v"], fx["w"])}
    labels = pkg.community.louvain(to_graph(pkg, cuda, n, edges))
    assert labels.dtype == torch.int64 and np.array_equal(labels.cpu().numpy(), fx["block"])


@pytest.fixture(scope="module")
def bars(pkg):
    """Per level: sequences, n, N, edges and the bar Q_min - (Q_max - Q_min) over the yardstick's seeds 0-4."""
    out = {}
    for name, (n, nseq, mean_len, seed) in (("2gram", (2, 60, 120, 1)), ("3gram", (3, 150, 200, 2))):
        seqs, N, edges = host_level(pkg, n, nseq, mean_len, seed)
        qs = [ref.modularity(N, edges, ref.louvain_seq(N, edges, s)) for s in range(5)]
        out[name] = (seqs, n, N, edges, min(qs) - (max(qs) - min(qs)), qs)
    return out


@pytest.mark.parametrize("name", ["2gram", "3gram"])
def test_modularity_bar_and_contract(pkg, cuda, bars, name):
    """Q of community_labels against the yardstick's band. Measured with louvain_ref, seeds 0-4 (networkx's own Louvain
    gave 0.3407-0.3499 and 0.4487-0.4575):
      2-gram (N = 424):   Q 0.3407-0.3499, bar 0.3315; the synchronous scheme's host prototype, 4 classes: 0.3430
      3-gram (N = 6,903): Q 0.4437-0.4601, bar 0.4273; prototype: 0.4432
    The labels are the prototype's (louvain_ref.louvain_sync), entry for entry: every decision is exact."""
    seqs, n, N, edges, bar, qs = bars[name]
    t = pkg.ngram.ngram_transitions(seqs, n, device=cuda)
    assert t.num_nodes == N
    g = pkg.community.combined_graph(t)
    rowptr, col, w, k = ref.csr(N, edges)
    assert g.rowptr.tolist() == rowptr and g.col.tolist() == col and g.w.tolist() == w and g.k.tolist() == k
    labels, classes = pkg.ngram.community_labels(t)
    again, _ = pkg.ngram.task_labels(t, "community", method="louvain")
    assert torch.equal(labels, again), "two runs give the same labels"
    lab = labels.cpu().numpy()
    assert labels.dtype == torch.int64 and labels.device.type == "cuda" and lab.shape == (N,)
    assert np.array_equal(lab, ref.number_by_smallest_member(lab)) and classes == lab.max() + 1
    q = ref.modularity(N, edges, lab)
    print(f"{name}: Q = {q:.4f}, {classes} communities; yardstick {min(qs):.4f}-{max(qs):.4f}, bar {bar:.4f}")
    assert abs(pkg.community.modularity(g, labels) - q) < 1e-12
    assert q >= bar
    assert np.array_equal(lab, ref.louvain_sync(N, edges, classes=4))


def test_edge_cases(pkg, cuda):
    ng = pkg.ngram
    labels, classes = ng.community_labels(ng.transitions_from_table(2, [], [], [], [], device=cuda))
    assert labels.numel() == 0 and labels.dtype == torch.int64 and classes == 1
    strings = ["AA", "AC", "CA", "CC", "CD", "DA"]
    labels, classes = ng.community_labels(ng.transitions_from_table(2, [], [], [], strings, device=cuda))
    assert labels.tolist() == [0] * 6 and classes == 1
    # zero counts are no entries either
    labels, classes = ng.community_labels(ng.transitions_from_table(2, [0], [1], [0], strings, device=cuda))
    assert labels.tolist() == [0] * 6 and classes == 1
    # nodes 2 and 5 isolated: communities of their own
    labels, classes = ng.community_labels(ng.transitions_from_table(2, [0, 1, 3], [1, 0, 4], [2, 1, 5], strings,
                                                                    device=cuda))
    assert labels.tolist() == [0, 0, 1, 2, 2, 3] and classes == 4
    # self-loops only: every node keeps its own community (the reference's graph has edges, so Louvain runs)
    labels, classes = ng.community_labels(ng.transitions_from_table(2, [0, 3], [0, 3], [2, 1], strings, device=cuda))
    assert labels.tolist() == list(range(6)) and classes == 6
    g = pkg.community.from_undirected(4, *(torch.tensor(x, device=cuda) for x in ([0, 2], [1, 3], [1, 1])))
    with pytest.raises(IndexError):
        pkg.community.sweep(g, torch.tensor([0, 1, 2, 4], device=cuda), 1, 0)


def test_louvain_clusters(pkg, cuda):
    from oracle import graph_cpu as og
    from protgram_directgcn_amd import cluster
    _, N, _ = host_level(pkg, 2, 60, 120, 1)
    seqs = pkg.ngram.preprocess(pkg.synth.protein_sequences(60, mean_len=120, seed=1))
    _, s, d, c, _ = pkg.synth.fasta_edges(2, seqs)
    mats = og.build_matrices(N, s, d, c)
    ei = {k: v[0].to(cuda) for k, v in mats.items()}
    ew = {k: v[1].to(cuda) for k, v in mats.items()}
    frac = 20
    g = cluster.louvain_graph(N, ei["in"], ew["in"], ei["out"], ew["out"], frac_bits=frac)
    # the weights: (A_out + A_in)[u, v] for u <= v, within half a unit of the fixed point
    dense = torch.zeros(N, N, dtype=torch.float64)
    for key in ("out", "in"):
        dense.index_put_((mats[key][0][0], mats[key][0][1]), mats[key][1].double(), accumulate=True)
    u, v, w = (x.cpu() for x in g.edges())
    err = (w.double() / (1 << frac) - dense[u, v]).abs()
    assert float(err.max()) <= 2.0 ** -(frac + 1)
    upper = torch.triu(dense)
    assert int((torch.round(upper * (1 << frac)) > 0).sum()) == u.numel()
    parts = cluster.louvain_clusters(N, ei["in"], ew["in"], ei["out"], ew["out"], frac_bits=frac)
    assert parts.shape == (N,) and parts.dtype == torch.int64
    p = parts.cpu().numpy()
    assert np.array_equal(p, ref.number_by_smallest_member(p)) and 1 < p.max() + 1 < N
    assert torch.equal(parts, cluster.louvain_clusters(N, ei["in"], ew["in"], ei["out"], ew["out"]))
    x = torch.randn(N, 8, generator=torch.Generator().manual_seed(0)).to(cuda)
    subs = cluster.build_subgraphs(N, parts, ei["in"], ew["in"], ei["out"], ew["out"], ei["und"], ew["und"], x,
                                   parts.clone())
    assert len(subs) == p.max() + 1 and sum(sub.num_nodes for sub in subs) == N
    for cid, sub in enumerate(subs):  # the reference collects clusters by first appearance: here the id order
        assert bool((parts[sub.original_indices] == cid).all())


def test_community_labels_feed_a_training_step(pkg, cuda, bars):
    from protgram_directgcn_amd import train
    seqs, n, N, _, _, _ = bars["3gram"]
    t = pkg.ngram.ngram_transitions(seqs, n, device=cuda)
    y, classes = pkg.ngram.task_labels(t, "community", method="louvain")
    assert int(y.min()) == 0 and int(y.max()) == classes - 1
    g = pkg.build_propagation_csr(N, t.src.cpu().numpy(), t.dst.cpu().numpy(), t.cnt.cpu().numpy(), device=cuda,
                                  transitions=t)
    torch.manual_seed(0)
    m = pkg.ProtGramDirectGCN([32, 64, 32], N, classes, n, 0, 512, 0.5, True).to(cuda)
    m.train()
    x = torch.randn(N, 32, generator=torch.Generator().manual_seed(1)).to(cuda)
    opt = train.Adam(m.parameters(), lr=1e-3)
    loss = train.train_step(m, pkg.Data(x=x, graph=g), y, opt, l2_lambda=1e-5, scaler=None)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss))
