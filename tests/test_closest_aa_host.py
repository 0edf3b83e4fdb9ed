"""closest_aa task labels, host side (no GPU): the per-node BFS restatement in closest_aa_ref.py reproduces the
reference's recorded labels (tests/golden/closest_aa.npz, tools/golden/make_closest_aa_golden.py) exactly; the host-side
target draw follows the reference's draw sequence; task_labels dispatch, the `letters` validation, no CPU fallback, and
the two entry points' argument errors before any HIP call."""
import random

import numpy as np
import pytest

import closest_aa_ref as ref
from golden_util import load

KS = (0, 1, 2, 3)


@pytest.fixture(scope="module")
def fx():
    return load("closest_aa")


def case_names(fx):
    return [str(c) for c in fx["cases"]]


def test_fixture_holds_what_it_is_meant_to(fx):
    assert case_names(fx) == ["p1_n1", "p1_n2", "p1_n3", "dense_n2", "dense_n3"]
    assert str(fx["letters"]) == ref.AMINO_ACIDS
    for name in case_names(fx):
        strings = [str(s) for s in fx[f"{name}:strings"]]
        n = int(fx[f"{name}:n"])
        assert strings == sorted(strings) and all(len(s) == n for s in strings)
        src, dst = fx[f"{name}:src"], fx[f"{name}:dst"]
        assert np.array_equal(np.lexsort((dst, src)), np.arange(src.size)), "edges sorted by (src, dst)"
        if n >= 2:  # every class of k = 3 occurs
            assert (np.bincount(fx[f"{name}:labels_k3"], minlength=4) > 0).all(), name
        if name.startswith("dense"):  # a row with every character as a successor, and true distances of 3
            assert np.bincount(src, minlength=len(strings)).max() == len(set("".join(strings)))
            d4 = ref.distances(len(strings), src, dst, strings, 4)
            assert (d4 == 2).any() and (d4 == 3).any()
    assert np.bincount(fx["p1_n2:labels_k3"]).tolist() == [37, 34, 59, 272]
    assert np.bincount(fx["p1_n3:labels_k3"]).tolist() == [84, 39, 36, 604]


@pytest.mark.parametrize("k", KS)
def test_restatement_reproduces_the_reference(fx, k):
    for name in case_names(fx):
        strings = [str(s) for s in fx[f"{name}:strings"]]
        got, classes = ref.labels(len(strings), fx[f"{name}:src"], fx[f"{name}:dst"], strings, fx[f"{name}:targets"], k)
        assert classes == k + 1
        assert got.dtype == np.int64 and np.array_equal(got, fx[f"{name}:labels_k{k}"]), (name, k)
    assert ref.labels(0, [], [], [], [], k)[1] == k + 1


def test_restated_distances_agree_with_the_labels(fx):
    name = "dense_n2"
    strings = [str(s) for s in fx[f"{name}:strings"]]
    t = fx[f"{name}:targets"].astype(np.int64)
    d = ref.distances(len(strings), fx[f"{name}:src"], fx[f"{name}:dst"], strings, 3)
    assert np.array_equal(d[np.arange(len(strings)), t], fx[f"{name}:labels_k3"])
    assert np.array_equal(d == 0, (ref.masks(strings)[:, None] >> np.arange(20, dtype=np.uint32)) & 1 == 1)


def test_host_draw_follows_the_reference_sequence(pkg, fx):
    assert pkg.ngram.AMINO_ACIDS == ref.AMINO_ACIDS == "ACDEFGHIKLMNPQRSTVWY"
    for name in case_names(fx):
        want = fx[f"{name}:targets"]
        random.seed(int(fx[f"{name}:seed"]))
        assert pkg.ngram.draw_targets(want.size) == want.tolist(), name
        # an own generator with the same seed draws the same sequence
        assert pkg.ngram.draw_targets(want.size, rng=random.Random(int(fx[f"{name}:seed"]))) == want.tolist()
    assert pkg.ngram.draw_targets(0) == []


def test_task_labels_dispatch(pkg, monkeypatch):
    t = pkg.ngram.transitions_from_table(2, [0, 0, 1], [1, 2, 2], [3, 3, 1], ["AA", "AC", "CA"])
    labels, classes = pkg.ngram.task_labels(t, "next_node")
    assert classes == 3 and labels.tolist() == [1, 2, 2]
    seen = {}
    monkeypatch.setattr(pkg.ngram, "closest_aa_labels", lambda tt, **kw: seen.update(kw, t=tt) or ("labels", 4))
    assert pkg.ngram.task_labels(t, "closest_aa", k_hops=3, targets="AAC") == ("labels", 4)
    assert seen == {"k_hops": 3, "targets": "AAC", "t": t}
    with pytest.raises(ValueError, match="Louvain"):
        pkg.ngram.task_labels(t, "community")
    with pytest.raises(ValueError, match=r"Unsupported GCN_TASK_TYPE 'nearest' for n=2\."):
        pkg.ngram.task_labels(t, "nearest")


def test_letters_and_hops_validation(pkg):
    t = pkg.ngram.transitions_from_table(2, [0], [1], [1], ["AA", "AC"])
    for fn in (lambda **kw: pkg.ngram.letter_masks(t, **kw), lambda **kw: pkg.ngram.letter_distances(t, 2, **kw),
               lambda **kw: pkg.ngram.closest_aa_labels(t, 2, **kw)):
        with pytest.raises(ValueError, match="32"):
            fn(letters="".join(chr(65 + i) for i in range(33)))
        with pytest.raises(ValueError, match="repeat"):
            fn(letters="ACA")
        with pytest.raises(ValueError):
            fn(letters="")
    for k in (-1, 256, 1.5):
        with pytest.raises(ValueError, match="k_hops"):
            pkg.ngram.letter_distances(t, k)
        with pytest.raises(ValueError, match="k_hops"):
            pkg.ngram.closest_aa_labels(t, k)


def test_closest_aa_has_no_cpu_fallback(pkg):
    t = pkg.ngram.transitions_from_table(2, [0, 1], [1, 2], [1, 1], ["AA", "AC", "CA"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.ngram.letter_masks(t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.ngram.letter_distances(t, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.ngram.closest_aa_labels(t, 3, targets=[0, 1, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.ngram.task_labels(t, "closest_aa")
    empty = pkg.ngram.transitions_from_table(2, [], [], [], [])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.ngram.closest_aa_labels(empty)


def test_letter_masks_abi_argument_errors_without_gpu(pkg):
    lib = pkg.load_library()
    buf = (np.zeros(64, dtype=np.int64)).ctypes.data  # any non-null host address: never dereferenced by the checks

    def masks(N=4, keys=buf, n=2, K=23, code_bit=buf, out=buf):
        return lib.pg_ngram_letter_masks(N, keys, n, K, code_bit, out, None)

    for kw in (dict(N=-1), dict(n=0), dict(K=0)):
        assert masks(**kw) == -1 and b"bad arguments" in lib.pg_last_error(), kw
    assert masks(n=20, K=20) == -1 and b"64-bit" in lib.pg_last_error()
    assert masks(N=0, keys=None, code_bit=None, out=None, n=20, K=20) == -1  # checked even when nothing would run
    for kw in (dict(keys=None), dict(code_bit=None), dict(out=None)):
        assert masks(**kw) == -1 and b"null" in lib.pg_last_error(), kw
    assert masks(N=0, keys=None, code_bit=None, out=None) == 0  # nothing to do, nothing launched


def test_reach_hop_abi_argument_errors_without_gpu(pkg):
    lib = pkg.load_library()
    a = np.zeros(64, dtype=np.int64)
    b = np.zeros(64, dtype=np.int64)
    buf, other = a.ctypes.data, b.ctypes.data

    def hop(N=8, rowptr=buf, col=buf, rin=buf, rout=other, hop=1, n_bits=20, dist=None, ldd=20, target=None,
            labels=None):
        return lib.pg_reach_hop_u32(N, rowptr, col, rin, rout, hop, n_bits, dist, ldd, target, labels, None)

    for kw in (dict(rowptr=None), dict(col=None), dict(rin=None), dict(rout=None)):
        assert hop(**kw) == -1 and b"null" in lib.pg_last_error(), kw
    assert hop(N=-1) == -1 and hop(N=1 << 31) == -1 and b"n_rows" in lib.pg_last_error()
    for h in (0, 256, -1):
        assert hop(hop=h) == -1 and b"hop" in lib.pg_last_error(), h
    for nb in (0, 33):
        assert hop(n_bits=nb) == -1 and b"n_bits" in lib.pg_last_error(), nb
    assert hop(dist=buf, ldd=19) == -1 and b"ldd" in lib.pg_last_error()
    assert hop(target=buf) == -1 and b"target" in lib.pg_last_error()
    assert hop(labels=buf) == -1 and b"target" in lib.pg_last_error()
    # aliasing reach buffers: the same address, and ranges that overlap by one word (8 rows = 32 bytes)
    assert hop(rout=buf) == -1 and b"overlap" in lib.pg_last_error()
    assert hop(rout=buf + 28) == -1 and b"overlap" in lib.pg_last_error()
    assert hop(rin=buf + 28, rout=buf) == -1 and b"overlap" in lib.pg_last_error()
    # nothing to do: no launch, whatever the pointers
    assert hop(N=0, rowptr=None, col=None, rin=None, rout=None) == 0
    assert hop(N=0, hop=0) == -1
