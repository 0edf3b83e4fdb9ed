"""closest_aa task labels on the GPU (csrc/pg_labels.hip through ngram.letter_masks / letter_distances /
closest_aa_labels): equal to the reference's recorded labels (tests/golden/closest_aa.npz) and to the per-node BFS
restatement (closest_aa_ref.py). Integer work: every comparison is an equality."""
import random

import numpy as np
import pytest
import torch

import closest_aa_ref as ref
from golden_util import load

pytestmark = pytest.mark.gpu

KS = (0, 1, 2, 3)
ALPHABET = " ACDEFGHIKLMNPQRSTUVWXY"  # code-point order; ' ', U and X are no letters


@pytest.fixture(scope="module")
def fx():
    return load("closest_aa")


def golden_level(pkg, fx, name, dev):
    strings = [str(s) for s in fx[f"{name}:strings"]]
    return pkg.ngram.transitions_from_table(int(fx[f"{name}:n"]), fx[f"{name}:src"], fx[f"{name}:dst"],
                                            fx[f"{name}:w"], strings, device=dev)


def level(pkg, dev, N, src, dst, n=3, seed=0, alphabet=ALPHABET):
    """A level of N distinct random n-grams over `alphabet` (ids = ranks in sorted order) with the given edges."""
    rng = np.random.default_rng(seed)
    keys = np.sort(rng.choice(len(alphabet) ** n, size=N, replace=False)) if N else np.zeros(0, np.int64)
    strings = pkg.ngram.decode_keys(keys, alphabet, n)
    order = np.lexsort((np.asarray(dst, np.int64), np.asarray(src, np.int64)))
    src, dst = np.asarray(src, np.int64)[order], np.asarray(dst, np.int64)[order]
    t = pkg.ngram.transitions_from_table(n, src, dst, np.ones(src.size), strings, alphabet=alphabet, device=dev)
    return t, strings, src, dst


def random_edges(N, E, seed):
    rng = np.random.default_rng(seed)
    pairs = np.unique(rng.integers(0, N, size=(E, 2)), axis=0) if N else np.zeros((0, 2), np.int64)
    return pairs[:, 0], pairs[:, 1]


@pytest.mark.parametrize("name", ["p1_n1", "p1_n2", "p1_n3", "dense_n2", "dense_n3"])
def test_labels_equal_the_reference(pkg, cuda, fx, name):
    t = golden_level(pkg, fx, name, cuda)
    targets = fx[f"{name}:targets"]
    for k in KS:
        labels, classes = pkg.ngram.closest_aa_labels(t, k, targets=targets)
        assert classes == k + 1 and labels.dtype == torch.int64 and labels.device.type == "cuda"
        assert np.array_equal(labels.cpu().numpy(), fx[f"{name}:labels_k{k}"]), (name, k)
    # the other forms of `targets`: a tensor on the device, a str of letters
    as_str = "".join(ref.AMINO_ACIDS[i] for i in targets)
    for form in (torch.from_numpy(targets.astype(np.int64)).to(cuda), as_str):
        assert np.array_equal(pkg.ngram.closest_aa_labels(t, 3, targets=form)[0].cpu().numpy(), fx[f"{name}:labels_k3"])


def test_seeded_draw_gives_the_reference_labels(pkg, cuda, fx):
    name = "p1_n3"
    t = golden_level(pkg, fx, name, cuda)
    random.seed(int(fx[f"{name}:seed"]))
    labels, classes = pkg.ngram.task_labels(t, "closest_aa")  # k_hops = 3: GCN_CLOSEST_AA_K_HOPS
    assert classes == 4 and np.array_equal(labels.cpu().numpy(), fx[f"{name}:labels_k3"])
    labels, _ = pkg.ngram.closest_aa_labels(t, 2, rng=random.Random(int(fx[f"{name}:seed"])))
    assert np.array_equal(labels.cpu().numpy(), fx[f"{name}:labels_k2"])


@pytest.mark.parametrize("n,N", [(1, 23), (2, 300), (5, 4000)])
def test_letter_masks(pkg, cuda, n, N):
    """K = 23 with ' ', U and X in the alphabet; n = 5: keys up to 23^5 - 1 (digits taken from an int64)."""
    t, strings, _, _ = level(pkg, cuda, N, [], [], n=n, seed=n)
    assert len(t.alphabet) == 23 and t.node_strings() == strings
    if n == 5:  # keys with a nonzero leading digit
        assert int(t.node_keys.max()) >= 23 ** 4
    masks = pkg.ngram.letter_masks(t)
    assert masks.dtype == torch.uint32 and masks.shape == (N,) and masks.device.type == "cuda"
    want = ref.masks(strings)
    assert np.array_equal(masks.cpu().numpy(), want)
    assert any(set(s) <= set(" UX") for s in strings) == bool((want == 0).any())
    # other letters: bit b is letters[b]; a character outside them sets nothing
    sub = pkg.ngram.letter_masks(t, letters="YXA")
    assert np.array_equal(sub.cpu().numpy(), ref.masks(strings, "YXA"))


def distance_graphs():
    """name -> (N, src, dst): the shapes at which the hop kernel's lane-group, wave and block arithmetic can go wrong."""
    g = {"no_nodes": (0, [], []),
         "no_edges": (40, [], []),
         "self_loops": (40, list(range(40)), list(range(40))),
         "path": (30, list(range(29)), list(range(1, 30))),
         # node 0 has 300 successors (more than a lane group's 16 and a wave's 64 entries per pass), the others few
         "fan300": (320, [0] * 300 + list(range(1, 320)), list(range(20, 320)) + [(7 * i) % 320 for i in range(1, 320)])}
    for N in (1, 63, 64, 65, 257):
        g[f"random{N}"] = (N, *random_edges(N, 3 * N, seed=N))
    return g


GRAPHS = distance_graphs()


@pytest.mark.parametrize("name", list(GRAPHS))
def test_letter_distances_equal_the_restatement(pkg, cuda, name):
    N, src, dst = GRAPHS[name]
    src, dst = (np.unique(np.stack([src, dst], 1), axis=0).T if len(src) else (np.zeros(0, np.int64),) * 2)
    t, strings, src, dst = level(pkg, cuda, N, src, dst, seed=len(name) + N)
    if name == "fan300":
        assert int(np.bincount(src, minlength=N).max()) >= 300
    for k in (0, 1, 7):
        d = pkg.ngram.letter_distances(t, k)
        assert d.dtype == torch.uint8 and d.shape == (N, 20) and d.device.type == "cuda"
        want = ref.distances(N, src, dst, strings, k)
        assert np.array_equal(d.cpu().numpy(), want), (name, k)
        if name in ("no_edges", "self_loops"):  # nothing to reach: own letters 0, every other entry the clip
            assert set(np.unique(want)) <= {0, k}
    if name == "path":  # the clip is hit: some letter's nearest node lies more than 7 hops ahead, yet is reachable
        far = ref.distances(N, src, dst, strings, N)
        assert ((far > 7) & (far < N)).any()


def test_absent_letter_gives_a_column_of_k(pkg, cuda):
    alphabet = " ACDEFGHIKLMNPQRSTUVWX"  # no Y
    src, dst = random_edges(200, 900, seed=5)
    t, strings, src, dst = level(pkg, cuda, 200, src, dst, seed=9, alphabet=alphabet)
    d = pkg.ngram.letter_distances(t, 5).cpu().numpy()
    assert np.array_equal(d, ref.distances(200, src, dst, strings, 5))
    assert (d[:, 19] == 5).all() and (d[:, :19] < 5).any()


def test_labels_are_the_distances_at_the_targets(pkg, cuda):
    N = 1000
    src, dst = random_edges(N, 8000, seed=2)
    t, strings, src, dst = level(pkg, cuda, N, src, dst, seed=4)
    targets = torch.from_numpy(np.random.default_rng(6).integers(0, 20, size=N))
    for k in (1, 3):
        d = pkg.ngram.letter_distances(t, k)
        labels, classes = pkg.ngram.closest_aa_labels(t, k, targets=targets)
        assert classes == k + 1
        assert torch.equal(labels, d.gather(1, targets.to(cuda).unsqueeze(1)).squeeze(1).to(torch.int64))
        # a second call returns the same bits
        assert torch.equal(pkg.ngram.letter_distances(t, k), d)
        assert torch.equal(pkg.ngram.closest_aa_labels(t, k, targets=targets)[0], labels)
    # spot check against the restatement on a sample of the nodes
    succ = ref.successors(N, src, dst)
    got = labels.cpu().numpy()
    for v in range(0, N, 37):
        assert got[v] == ref.bfs_label(v, ref.AMINO_ACIDS[int(targets[v])], succ, strings, 3)


def test_empty_level(pkg, cuda):
    t, _, _, _ = level(pkg, cuda, 0, [], [])
    labels, classes = pkg.ngram.closest_aa_labels(t, 3)
    assert classes == 4 and labels.dtype == torch.int64 and labels.shape == (0,)
    assert pkg.ngram.letter_masks(t).shape == (0,) and pkg.ngram.letter_distances(t, 3).shape == (0, 20)


def test_producer_level_end_to_end(pkg, cuda, fx):
    """A level made by the GPU producer from the p1 FASTA's sequences has the fixture's node ids: same labels."""
    p1 = load("p1_fasta")
    t = pkg.ngram.ngram_transitions([str(s) for s in p1["seqs"]], 3, device=cuda)
    assert t.node_strings() == [str(s) for s in fx["p1_n3:strings"]]
    assert np.array_equal(t.src.cpu().numpy(), fx["p1_n3:src"]) and np.array_equal(t.dst.cpu().numpy(), fx["p1_n3:dst"])
    for k in KS:
        labels, _ = pkg.ngram.closest_aa_labels(t, k, targets=fx["p1_n3:targets"])
        assert np.array_equal(labels.cpu().numpy(), fx[f"p1_n3:labels_k{k}"]), k


def test_bad_indices_are_refused_before_any_launch(pkg, cuda, fx, monkeypatch):
    t = golden_level(pkg, fx, "dense_n2", cuda)
    N = t.num_nodes
    launched = []
    real = pkg.ngram.load_library

    def spy():
        launched.append(1)
        return real()

    monkeypatch.setattr(pkg.ngram, "load_library", spy)
    t.dst[3] = N
    with pytest.raises(IndexError, match="dst"):
        pkg.ngram.letter_distances(t, 3)
    with pytest.raises(IndexError, match="dst"):
        pkg.ngram.closest_aa_labels(t, 3, targets=[0] * N)
    t.dst[3] = -1
    with pytest.raises(IndexError, match="dst"):
        pkg.ngram.closest_aa_labels(t, 3, targets=[0] * N)
    t.dst[3] = 0
    t.src[-1] = N
    with pytest.raises(IndexError, match="src"):
        pkg.ngram.letter_distances(t, 3)
    t.src[-1] = N - 1
    with pytest.raises(ValueError, match=r"\[0, 20\)"):
        pkg.ngram.closest_aa_labels(t, 3, targets=[20] * N)
    with pytest.raises(ValueError, match="one entry per node"):
        pkg.ngram.closest_aa_labels(t, 3, targets=[0] * (N - 1))
    assert not launched, "the library was reached although the arguments were bad"
