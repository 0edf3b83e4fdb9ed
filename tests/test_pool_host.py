"""Protein-level pooling, host side (no GPU): the restatement in pool_ref.py reproduces the reference's recorded
outputs (tests/golden/pool_proteins.npz, tools/golden/make_pool_golden.py) bit for bit in both modes; pooled_dict, the
foreign-byte lut, the new entry points' argument errors before any HIP call, and no CPU fallback."""
import numpy as np
import pytest
import torch

from golden_util import load
from pool_ref import bits, pool_lists, window_lists


@pytest.fixture(scope="module")
def fx():
    return load("pool_proteins")


@pytest.mark.parametrize("n", [2, 3])
def test_restatement_reproduces_the_reference_bit_for_bit(pkg, fx, n):
    ids, seqs = [str(x) for x in fx["ids"]], [str(x) for x in fx["seqs"]]
    nodes = [str(x) for x in fx[f"n{n}_nodes"]]
    assert nodes == sorted(nodes)
    emb = fx[f"n{n}_emb"]
    assert np.signbit(emb[emb == 0]).any(), "the table must hold -0.0 entries"
    lists = window_lists(seqs, n, {g: i for i, g in enumerate(nodes)})
    # distinct: the trainer's call; the reference returns a dict (a repeated id keeps its later vector)
    vec, cnt = pool_lists(lists, emb, "distinct")
    assert np.array_equal(cnt, fx[f"n{n}_distinct_counts"])
    got = pkg.pool.pooled_dict(ids, vec, cnt)
    assert list(got) == [str(x) for x in fx[f"n{n}_fast_ids"]]
    assert np.array_equal(bits(np.stack(list(got.values()))), bits(fx[f"n{n}_fast_vecs"]))
    # windows: one call per protein, None for a protein without a valid window
    vec, cnt = pool_lists(lists, emb, "windows")
    assert np.array_equal(cnt, fx[f"n{n}_windows_counts"])
    assert np.array_equal(np.flatnonzero(cnt > 0), fx[f"n{n}_windows_idx"])
    assert np.array_equal(bits(vec[cnt > 0]), bits(fx[f"n{n}_windows_vecs"]))
    # what the fixture is meant to hold
    assert (cnt == 0).sum() >= 3 and (fx[f"n{n}_distinct_counts"] < cnt).any()
    lone = seqs.index(next(s for s in seqs if len(s) == n))
    assert cnt[lone] == 1 and not bits(vec[lone]).any(), "a lone -0.0 row pools to +0.0"


def test_pooled_dict(pkg):
    pooled = np.arange(12, dtype=np.float32).reshape(4, 3)
    counts = np.array([2, 0, 1, 5], dtype=np.int32)
    d = pkg.pool.pooled_dict(["a", "b", "c", "a"], pooled, counts)
    assert list(d) == ["a", "c"] and np.array_equal(d["a"], pooled[3]) and np.array_equal(d["c"], pooled[2])
    # a later duplicate without a vector leaves the earlier one
    d = pkg.pool.pooled_dict(["a", "a"], pooled[:2], counts[:2])
    assert np.array_equal(d["a"], pooled[0])
    d = pkg.pool.pooled_dict(["a", "b", "c", "d"], torch.from_numpy(pooled), torch.from_numpy(counts),
                             id_map={"a": "A", "d": "D", "zz": "unused"})
    assert set(d) == {"A", "c", "D"} and d["A"].dtype == np.float32
    assert pkg.pool.pooled_dict([], np.zeros((0, 3), np.float32), np.zeros(0, np.int32)) == {}
    with pytest.raises(ValueError):
        pkg.pool.pooled_dict(["a"], pooled, counts)


def test_foreign_byte_lut(pkg):
    lut = pkg.pool.alphabet_lut(" ACX")
    assert lut.dtype == np.int32 and lut.shape == (256,)
    assert [lut[ord(c)] for c in " ACX"] == [0, 1, 2, 3]
    assert (lut >= 0).sum() == 4 and lut[ord("a")] == -1 and lut[ord("U")] == -1 and lut[0] == -1 and lut[255] == -1
    # ngram.encode maps a foreign byte to code 0: the producer's alphabet is every byte present
    assert (pkg.ngram.encode(["AC"])[2] >= 0).all()


def test_pool_abi_argument_errors_without_gpu(pkg):
    lib = pkg.load_library()
    cap = lib.pg_pool_distinct_max_nodes()
    assert cap == pkg.pool.distinct_max_nodes() == 262144
    buf = (np.zeros(64, dtype=np.int64)).ctypes.data  # any non-null host address: never dereferenced by the checks

    def rows(E=buf, lde=4, N=8, F=4, rowptr=buf, ids=buf, order=None, P=2, distinct=0, out=buf, ldo=4, counts=buf):
        return lib.pg_pool_rows_f32(E, lde, N, F, rowptr, ids, order, P, distinct, out, ldo, counts, 0, None)

    for kw in (dict(P=-1), dict(N=-1), dict(F=-1)):
        assert rows(**kw) == -1 and b"negative" in lib.pg_last_error(), kw
    assert rows(ldo=3) == -1 and b"ldo" in lib.pg_last_error()
    assert rows(lde=3) == -1
    assert rows(distinct=2) == -1
    assert rows(N=1 << 31) == -1
    for kw in (dict(E=None), dict(rowptr=None), dict(ids=None), dict(out=None), dict(counts=None)):
        assert rows(**kw) == -1 and b"null" in lib.pg_last_error(), kw
    assert rows(N=cap + 1, distinct=1) == -3 and b"distinct" in lib.pg_last_error()
    assert rows(N=cap + 1, distinct=1, E=None, rowptr=None, ids=None, out=None, counts=None) == -3
    assert rows(P=0, E=None, rowptr=None, ids=None, out=None, counts=None) == 0  # nothing to do

    def wid(nseq=1, offsets=buf, bytes_=buf, lut=buf, n=2, K=20, keys=buf, N=5, table=None, ids=buf):
        return lib.pg_ngram_window_ids(nseq, offsets, bytes_, lut, n, K, keys, N, table, ids, None)

    for kw in (dict(nseq=-1), dict(n=0), dict(K=0), dict(N=-1)):
        assert wid(**kw) == -1 and b"bad arguments" in lib.pg_last_error(), kw
    assert wid(N=1 << 31) == -1
    assert wid(n=20, K=20) == -1 and b"64-bit" in lib.pg_last_error()
    for kw in (dict(offsets=None), dict(bytes_=None), dict(lut=None), dict(ids=None), dict(keys=None)):
        assert wid(**kw) == -1 and b"null" in lib.pg_last_error(), kw
    assert wid(nseq=0, offsets=None, bytes_=None, lut=None, ids=None, keys=None) == 0


def test_pool_has_no_cpu_fallback(pkg):
    t = pkg.ngram.transitions_from_table(2, [], [], [], ["AA", "AC", "CA"])
    emb = torch.zeros(3, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.pool.pool_proteins(["ACA"], t, emb)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.pool.pool_proteins(["ACA"], t, emb, mode="windows")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.pool.window_ids(["ACA"], t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pkg.pool.pool_rows(emb, torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError):
        pkg.pool.pool_proteins(["ACA"], t, emb, mode="max")
    with pytest.raises(ValueError):
        pkg.pool.pool_proteins(["ACA"], t, emb, distinct_path="hash")
    with pytest.raises(ValueError):
        pkg.pool.pool_proteins(["ACA"], t, torch.zeros(3))
