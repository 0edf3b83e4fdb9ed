"""Protein-level pooling on the GPU (pool.py, pg_ngram_window_ids, pg_pool_rows_f32) against the reference's recorded
outputs (tests/golden/pool_proteins.npz) and the NumPy restatement that tests/test_pool_host.py pins to them.

Everything is compared as bit patterns: no tolerance, no excluded element. The sum order is fully specified (one
sequential fp32 chain from +0.0 per column, list order or ascending id order) and the quotient is correctly rounded, so
there is exactly one right answer.
"""
import functools

import numpy as np
import pytest
import torch

from golden_util import load
from pool_ref import bits, pool_lists, window_lists

pytestmark = pytest.mark.gpu

# list lengths at the edges of the gather loop: id chunks of 8 / 16 / 32 / 64 per lane group, row batches of 8 / 16,
# the distinct walk's 64-id chunks, the 1024 entries above which a windows list gets a whole wave; one list far
# beyond all of them
LENS = [0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1024, 1025, 5000]


def _same(a, b, what=""):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype == np.float32:
        a, b = bits(a), bits(b)
    bad = np.flatnonzero((a != b).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at flat index {bad[:5]}"


@functools.lru_cache(maxsize=None)
def _case(N, F):
    """Lists of node ids (with -1 entries and duplicates), a table with -0.0 entries, and the restated results."""
    rng = np.random.default_rng(1000 * N + F)
    emb = rng.standard_normal((N, F)).astype(np.float32)
    emb[rng.random(emb.shape) < 0.02] = -0.0
    emb[5] = -0.0
    lists = [rng.integers(0, N, size=L).tolist() for L in LENS]
    for lst in lists[3:]:
        for k in rng.integers(0, len(lst), size=max(1, len(lst) // 10)):
            lst[k] = -1                       # windows that are no node
    lists[-1][17], lists[-1][4000] = 0, N - 1  # the first and the last node
    lists[4][2], lists[4][3] = N - 1, 0
    lists += [[5],                            # a single window on a row of -0.0: pools to +0.0
              [-1] * 40,                      # no valid window: zero row, count 0
              [7] * 37,                       # a homopolymer: one distinct id, 37 windows
              [N - 1, 0, N - 1, 0, 31 % N, 32 % N]]
    ref = {m: pool_lists(lists, emb, m) for m in ("windows", "distinct")}
    return emb, lists, ref


def _csr(lists, dev):
    lens = np.array([len(x) for x in lists], dtype=np.int64)
    rowptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum(lens, out=rowptr[1:])
    ids = np.array([i for x in lists for i in x], dtype=np.int32)
    return torch.from_numpy(rowptr).to(dev), torch.from_numpy(ids).to(dev)


@pytest.mark.parametrize("n", [2, 3])
def test_fixture_both_modes(pkg, cuda, n):
    fx = load("pool_proteins")
    pids, seqs = [str(x) for x in fx["ids"]], [str(x) for x in fx["seqs"]]
    t = pkg.ngram.transitions_from_table(n, [], [], [], [str(x) for x in fx[f"n{n}_nodes"]], device=cuda)
    emb = torch.from_numpy(fx[f"n{n}_emb"]).to(cuda)
    for path in ("bitmap", "sort"):
        pooled, counts = pkg.pool.pool_proteins(seqs, t, emb, mode="distinct", distinct_path=path)
        _same(counts, fx[f"n{n}_distinct_counts"], f"distinct counts ({path})")
        d = pkg.pool.pooled_dict(pids, pooled, counts)
        assert list(d) == [str(x) for x in fx[f"n{n}_fast_ids"]]
        _same(np.stack(list(d.values())), fx[f"n{n}_fast_vecs"], f"distinct vectors ({path})")
        assert not bits(pooled.cpu().numpy()[counts.cpu().numpy() == 0]).any()
    pooled, counts = pkg.pool.pool_proteins(seqs, t, emb, mode="windows")
    _same(counts, fx[f"n{n}_windows_counts"], "windows counts")
    have = counts.cpu().numpy() > 0
    _same(np.flatnonzero(have), fx[f"n{n}_windows_idx"], "windows id set")
    _same(pooled.cpu().numpy()[have], fx[f"n{n}_windows_vecs"], "windows vectors")
    assert not bits(pooled.cpu().numpy()[~have]).any()


@pytest.mark.parametrize("N", [33, 1003, 70001])
@pytest.mark.parametrize("F", [1, 6, 20, 64, 128, 256])
def test_list_shapes(pkg, cuda, N, F):
    emb_h, lists, ref = _case(N, F)
    emb = torch.from_numpy(emb_h).to(cuda)
    rowptr, ids = _csr(lists, cuda)
    for mode in ("windows", "distinct"):
        out, cnt = pkg.pool.pool_rows(emb, rowptr, ids, distinct=mode == "distinct")
        _same(cnt, ref[mode][1], f"{mode} counts")
        _same(out, ref[mode][0], f"{mode} N={N} F={F}")
    c = ref["distinct"][1]
    k = len(LENS)
    assert list(c[k:k + 3]) == [1, 0, 1] and list(ref["windows"][1][k:k + 3]) == [1, 0, 37]
    assert not bits(ref["windows"][0][k]).any() and not bits(ref["windows"][0][k + 1]).any()


@pytest.mark.parametrize("F,pad,shift", [(64, 12, 0), (64, 12, 1), (6, 3, 0), (20, 1, 0), (128, 4, 3)])
def test_row_stride_and_alignment(pkg, cuda, F, pad, shift):
    """A table with a row stride above F; shift != 0 or an odd stride takes the per-element kernels."""
    N = 1003
    emb_h, lists, ref = _case(N, F)
    wide = torch.zeros(N, F + pad + shift, device=cuda)
    emb = wide[:, shift:shift + F]
    emb.copy_(torch.from_numpy(emb_h))
    assert emb.stride(0) == F + pad + shift and not emb.is_contiguous()
    rowptr, ids = _csr(lists, cuda)
    for mode in ("windows", "distinct"):
        out, cnt = pkg.pool.pool_rows(emb, rowptr, ids, distinct=mode == "distinct")
        _same(cnt, ref[mode][1])
        _same(out, ref[mode][0], f"{mode} F={F} stride={emb.stride(0)} shift={shift}")


def test_list_order_and_launch_order_do_not_matter(pkg, cuda):
    N, F = 1003, 64
    emb_h, lists, ref = _case(N, F)
    emb = torch.from_numpy(emb_h).to(cuda)
    P = len(lists)
    perm = np.random.default_rng(3).permutation(P)
    rowptr, ids = _csr(lists, cuda)
    rowptr_p, ids_p = _csr([lists[i] for i in perm], cuda)
    for mode in ("windows", "distinct"):
        d = mode == "distinct"
        out_p, cnt_p = pkg.pool.pool_rows(emb, rowptr_p, ids_p, distinct=d)  # the same set, another protein order
        _same(out_p, ref[mode][0][perm], f"{mode} permuted")
        _same(cnt_p, ref[mode][1][perm])
        for order in (torch.arange(P, device=cuda), torch.arange(P - 1, -1, -1, device=cuda),
                      torch.from_numpy(perm).to(cuda)):
            out, cnt = pkg.pool.pool_rows(emb, rowptr, ids, distinct=d, order=order)
            _same(out, ref[mode][0], f"{mode} order")
            _same(cnt, ref[mode][1])
        out, _ = pkg.pool.pool_rows(emb, rowptr, ids, distinct=d, sort_lists=False)
        _same(out, ref[mode][0], f"{mode} no order")
    with pytest.raises(ValueError):
        pkg.pool.pool_rows(emb, rowptr, ids, order=torch.zeros(P, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError):
        pkg.pool.pool_rows(emb[:100], rowptr, ids)  # ids >= N
    with pytest.raises(ValueError):
        pkg.pool.pool_rows(emb.double(), rowptr, ids)


def test_deterministic_and_clean_between_launches(pkg, cuda):
    """The same launch twice gives the same bits, and a launch after one with another protein set is unaffected
    (the distinct kernel leaves its bitmap clean; nothing is carried in global memory either)."""
    N, F = 1003, 20
    emb_h, lists, ref = _case(N, F)
    emb = torch.from_numpy(emb_h).to(cuda)
    rowptr, ids = _csr(lists, cuda)
    other = [np.random.default_rng(9).integers(0, N, size=L).tolist() for L in (700, 3, 0, 129, 64, 2000)]
    rowptr_o, ids_o = _csr(other, cuda)
    ref_o = {m: pool_lists(other, emb_h, m) for m in ("windows", "distinct")}
    for mode in ("windows", "distinct"):
        d = mode == "distinct"
        a, ca = pkg.pool.pool_rows(emb, rowptr, ids, distinct=d)
        b, cb = pkg.pool.pool_rows(emb, rowptr, ids, distinct=d)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)
        o, co = pkg.pool.pool_rows(emb, rowptr_o, ids_o, distinct=d)
        _same(o, ref_o[mode][0], f"{mode} other set")
        _same(co, ref_o[mode][1])
        c, cc = pkg.pool.pool_rows(emb, rowptr, ids, distinct=d)
        _same(c, ref[mode][0], f"{mode} after another set")
        _same(cc, ref[mode][1])


def _host_ids(seqs, n, ngram_map):
    out = []
    for s in seqs:
        out += [ngram_map.get(s[k:k + n], -1) if k + n <= len(s) else -1 for k in range(len(s))]
    return np.array(out, dtype=np.int32)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_window_ids_table_and_search(pkg, cuda, n):
    seqs = pkg.synth.protein_sequences(40, mean_len=30, seed=n, rare=0.05) + ["", "A", "AC", "ACD", "acd", "KKKKKKK"]
    nodes = sorted({s[k:k + n] for s in seqs[:25] for k in range(len(s) - n + 1)})[::2] + ([" " * n] if n > 1 else [])
    nodes = sorted(set(nodes))
    t = pkg.ngram.transitions_from_table(n, [], [], [], nodes, device=cuda)
    want = _host_ids(seqs, n, {g: i for i, g in enumerate(nodes)})
    a, off_a = pkg.pool.window_ids(seqs, t, dense_table=True)
    b, off_b = pkg.pool.window_ids(seqs, t, dense_table=False)
    assert a.dtype == torch.int32 and off_a.dtype == torch.int64 and torch.equal(off_a, off_b)
    _same(off_a, np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64))
    _same(a, want, "dense table")
    _same(b, want, "binary search")
    assert (want >= 0).any() and (want < 0).any()
    ends = off_a[1:].cpu().numpy()
    for j in range(1, n):  # a window that would straddle the sequence boundary
        sel = ends[ends - j >= off_a[:-1].cpu().numpy()] - j
        assert (a.cpu().numpy()[sel] == -1).all()
    # no nodes at all, and no sequences
    t0 = pkg.ngram.transitions_from_table(n, [], [], [], [], alphabet=t.alphabet, device=cuda)
    assert (pkg.pool.window_ids(seqs, t0)[0] == -1).all()
    e, off_e = pkg.pool.window_ids([], t)
    assert e.numel() == 0 and off_e.tolist() == [0]
    emb0 = torch.zeros(0, 4, device=cuda)
    pooled, counts = pkg.pool.pool_proteins(seqs, t0, emb0)
    assert not bits(pooled.cpu().numpy()).any() and not counts.any() and pooled.shape == (len(seqs), 4)


def test_sequences_end_to_end_special_proteins(pkg, cuda):
    n, F = 2, 20
    seqs = pkg.synth.protein_sequences(30, mean_len=40, seed=4, rare=0.02)
    nodes = sorted({s[k:k + n] for s in seqs[:20] for k in range(len(s) - n + 1)} | {"KK"})
    seqs = seqs + ["u" * 9, nodes[3], "K" * 30, "", "A", nodes[0], nodes[-1]]
    pids = [f"p{i}" for i in range(len(seqs))]
    rng = np.random.default_rng(8)
    emb_h = rng.standard_normal((len(nodes), F)).astype(np.float32)
    emb_h[nodes.index(seqs[31])] = -0.0
    t = pkg.ngram.transitions_from_table(n, [], [], [], nodes, device=cuda)
    emb = torch.from_numpy(emb_h).to(cuda)
    lists = window_lists(seqs, n, {g: i for i, g in enumerate(nodes)})
    for mode in ("windows", "distinct"):
        ref, rc = pool_lists(lists, emb_h, mode)
        pooled, counts = pkg.pool.pool_proteins(seqs, t, emb, mode=mode)
        _same(counts, rc, mode)
        _same(pooled, ref, mode)
        d = pkg.pool.pooled_dict(pids, pooled, counts)
        assert "p30" not in d and "p33" not in d and "p34" not in d and "p31" in d  # no valid window: no vector
        assert not bits(d["p31"]).any()                                             # lone -0.0 row -> +0.0
        assert int(counts[32]) == (1 if mode == "distinct" else 29)                 # the homopolymer
        assert int(counts[35]) == 1 and int(counts[36]) == 1                        # ids 0 and N - 1
        _same(pooled[35], emb_h[0])
        _same(pooled[36], emb_h[-1])


def test_bitmap_path_equals_sort_path_on_protein_like_input(pkg, cuda):
    n, F = 3, 64
    seqs = pkg.synth.protein_sequences(2000, mean_len=350, seed=2)
    t = pkg.ngram.ngram_transitions(seqs[:1500], n, device=cuda)  # the level's nodes; later proteins bring strangers
    N = t.num_nodes
    emb = torch.randn(N, F, generator=torch.Generator().manual_seed(6)).to(cuda)
    a, ca = pkg.pool.pool_proteins(seqs, t, emb, mode="distinct", distinct_path="bitmap")
    b, cb = pkg.pool.pool_proteins(seqs, t, emb, mode="distinct", distinct_path="sort")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)
    auto, _ = pkg.pool.pool_proteins(seqs, t, emb)
    assert torch.equal(auto.view(torch.int32), a.view(torch.int32))
    w, cw = pkg.pool.pool_proteins(seqs, t, emb, mode="windows")
    emb_h = emb.cpu().numpy()
    lists = window_lists(seqs, n, {g: i for i, g in enumerate(t.node_strings())})
    ref, rc = pool_lists(lists, emb_h, "distinct")
    _same(ca, rc)
    _same(a, ref, "distinct vs the restatement")
    ref, rc = pool_lists(lists, emb_h, "windows")
    _same(cw, rc)
    _same(w, ref, "windows vs the restatement")
    assert int((cw.cpu() > ca.cpu()).sum()) > 100  # repeated 3-grams inside one protein are common at this length


def test_distinct_above_the_bitmap_cap_takes_the_sort_path(pkg, cuda):
    cap = pkg.pool.distinct_max_nodes()
    N, F = cap + 37, 4
    rng = np.random.default_rng(12)
    emb_h = rng.standard_normal((N, F)).astype(np.float32)
    lists = [rng.integers(0, N, size=L).tolist() for L in (5, 0, 300)] + [[N - 1, 0, N - 1, cap, cap - 1]]
    emb = torch.from_numpy(emb_h).to(cuda)
    rowptr, ids = _csr(lists, cuda)
    with pytest.raises(ValueError):
        pkg.pool.pool_rows(emb, rowptr, ids, distinct=True)
    ptr, uids = pkg.pool._sorted_distinct_lists(rowptr, ids, N)
    out, cnt = pkg.pool.pool_rows(emb, ptr, uids)
    ref, rc = pool_lists(lists, emb_h, "distinct")
    _same(cnt, rc)
    _same(out, ref, "sort path above the cap")
    # at the cap itself the bitmap path runs (the last word of the largest bitmap)
    out, cnt = pkg.pool.pool_rows(emb[:cap], rowptr[:2], ids[:5] % cap, distinct=True)
    ref, rc = pool_lists([[i % cap for i in lists[0]]], emb_h[:cap], "distinct")
    _same(out, ref, "bitmap at the cap")


def test_protein_embeddings_tail_of_run(pkg, cuda):
    N, s, d, c = pkg.synth.de_bruijn_edges(2)
    g = pkg.build_propagation_csr(N, s, d, c, device=cuda)
    A = pkg.synth.ALPHABET
    t = pkg.ngram.transitions_from_table(2, s, d, c, [a + b for a in A for b in A], device=cuda)
    torch.manual_seed(0)
    model = pkg.ProtGramDirectGCN([32, 32, 16], N, 20, 2, 0, 512, 0.5, True).to(cuda)
    x = torch.randn(N, 32, generator=torch.Generator().manual_seed(1)).to(cuda)
    data = pkg.Data(x=x, graph=g)
    prots = [(f"sp{i}", q) for i, q in enumerate(pkg.synth.protein_sequences(12, mean_len=30, seed=5, rare=0.05))]
    prots += [("short", "A"), ("odd", "UUXU"), ("sp3", "ACDA")]
    model.eval()
    with torch.no_grad():
        _, emb = model(data)
    for mode in ("distinct", "windows"):
        pooled, counts = pkg.pool.pool_proteins([q for _, q in prots], t, emb, mode=mode)
        want = pkg.pool.pooled_dict([p for p, _ in prots], pooled, counts, id_map={"sp0": "Q0"})
        for training in (True, False):
            model.train(training)
            got = pkg.pool.protein_embeddings(model, data, t, prots, mode=mode, id_map={"sp0": "Q0"})
            assert model.training is training
            assert list(got) == list(want) and "Q0" in got and "short" not in got and "odd" not in got
            for k in want:
                _same(got[k], want[k], k)
    ref, _ = pool_lists(window_lists(["ACDA"], 2, {a + b: i for i, (a, b) in enumerate((a, b) for a in A for b in A)}),
                        emb.cpu().numpy(), "distinct")
    _same(want["sp3"], ref[0], "the later duplicate id wins")
