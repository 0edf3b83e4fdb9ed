"""NumPy restatement of the reference's two protein pooling functions (src/utils/models_utils.py:197-262), written
for the tests: dict lookups and one explicit sequential fp32 chain per protein. tests/test_pool_host.py pins it to
the reference's recorded outputs (tests/golden/pool_proteins.npz) bit for bit; the GPU tests use it where the
fixture has no case."""
import numpy as np


def window_lists(seqs, n, ngram_map):
    """Per sequence the node ids of its valid windows, in window order (ngram_map.get per window)."""
    return [[ngram_map[s[k:k + n]] for k in range(len(s) - n + 1) if s[k:k + n] in ngram_map] for s in seqs]


def pool_lists(lists, emb, mode):
    """(vectors fp32 [P, F], counts int32 [P]): 'windows' adds every entry in list order, 'distinct' every id once
    in ascending order; fp32 adds from +0.0, then the fp32 quotient by the count; no entry: zeros and count 0."""
    emb = np.asarray(emb, dtype=np.float32)
    out = np.zeros((len(lists), emb.shape[1]), dtype=np.float32)
    counts = np.zeros(len(lists), dtype=np.int32)
    for p, ids in enumerate(lists):
        ids = [i for i in ids if 0 <= i < emb.shape[0]]
        if mode == "distinct":
            ids = sorted(set(ids))
        elif mode != "windows":
            raise ValueError(mode)
        if not ids:
            continue
        acc = np.zeros(emb.shape[1], dtype=np.float32)  # +0.0
        for i in ids:
            acc = (acc + emb[i]).astype(np.float32)     # one fp32 add per entry, in order
        counts[p] = len(ids)
        out[p] = acc / np.float32(len(ids))             # correctly rounded fp32 quotient (counts < 2^24)
    return out, counts


def bits(a):
    """The values as bit patterns: comparisons with no tolerance, -0.0 and +0.0 told apart."""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return a.view(np.uint32)
