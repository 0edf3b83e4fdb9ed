"""The middle-tile forward (pg_ngram_mid.hip) at the chunk-range shapes tests/test_gpu_ngram.py leaves out: its LDS
addresses are one register per lane plus compile-time offsets per accumulator row, tile and K-step, so every path the
chunk schedule takes is compared with the CSR kernels (|d| <= 1e-5 + 1e-5 |ref|, the tile kernels' bound) and, bit for
bit, with the schedule variants that must not change a result (PG_FLAG_MID_LOADER_SYNC, PG_FLAG_MID_NO_PAIRS).

What a shape exercises depends on the chunk ranges (one persistent workgroup per CU, 256 on MI355X; a range has more
than one chunk only where the launch has more chunks, or chunk pairs, than workgroups):
  B(20,2) F=16          one chunk in all, one workgroup
  B(20,2) F=64          two workgroup pairs, one chunk each: odd / even chunk halves
  B(20,3) F=32          one chunk per workgroup, a new middle each
  B(20,3) F=256         ranges of 1-2 chunks
  B(20,4) F=32, 48      ranges of 3-5 chunks with middle changes (A-fragment reloads) inside; F=48: an odd chunk count,
                        so no pairs; F=32 with and without pairs
  spmm3_middles         middle-major Z with m0 > 0: B(20,3) F=128 (3, 11) and, with ranges of 1-2 chunks, B(20,4) F=32
"""
import pytest
import torch

from test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

_GRAPHS = {}


def _graph(pkg, cuda, n):
    if n not in _GRAPHS:
        N, s, d, c = pkg.synth.de_bruijn_edges(n)
        _GRAPHS[n] = pkg.build_propagation_csr(N, s, d, c, device=cuda)
    return _GRAPHS[n]


def _flags():
    from protgram_directgcn_amd import _lib, ops
    return ops.default_flags(), _lib


@pytest.mark.parametrize("n,F", [(2, 16), (2, 64), (3, 32), (3, 256), (4, 32), (4, 48)])
def test_mid_whole_graph(pkg, cuda, n, F):
    from protgram_directgcn_amd import ops
    fl, _lib = _flags()
    g = _graph(pkg, cuda, n)
    assert g.ngram is not None and g.ngram.mplan is not None
    x = torch.randn(g.n_rows, F, generator=torch.Generator().manual_seed(7 * n + F)).to(cuda)
    Z = ops.spmm3(g, x, flags=fl)
    assert_close(Z, ops.spmm3(g, x, flags=fl | _lib.PG_FLAG_NO_NGRAM), f"n={n} F={F}")
    assert torch.equal(Z, ops.spmm3(g, x, flags=fl | _lib.PG_FLAG_MID_LOADER_SYNC)), "loader sync: other bits"
    assert torch.equal(Z, ops.spmm3(g, x, flags=fl | _lib.PG_FLAG_MID_NO_PAIRS)), "no pairs: other bits"


@pytest.mark.parametrize("n,F,m0,m1", [(3, 128, 3, 11), (4, 32, 37, 237)])
def test_mid_middle_major(pkg, cuda, n, F, m0, m1):
    from protgram_directgcn_amd import ops
    fl, _lib = _flags()
    g = _graph(pkg, cuda, n)
    x = torch.randn(g.n_rows, F, generator=torch.Generator().manual_seed(11 * n + F)).to(cuda)
    Z = ops.spmm3_middles(g, x, m0, m1)
    assert Z.shape == ((m1 - m0) * 400, 3 * F)
    assert torch.equal(Z, ops.spmm3_middles(g, x, m0, m1, flags=fl | _lib.PG_FLAG_MID_NO_PAIRS))
    # row (M - m0) K^2 + a K + b of Z is the graph's row a K^(n-1) + M K + b
    Kn1 = g.n_rows // 20
    M, a, b = torch.meshgrid(torch.arange(m0, m1), torch.arange(20), torch.arange(20), indexing="ij")
    rows = (a * Kn1 + M * 20 + b).reshape(-1).to(cuda)
    ref = ops.spmm3(g, x, flags=fl | _lib.PG_FLAG_NO_NGRAM)[rows]
    assert_close(Z, ref, f"middles [{m0}, {m1}) of B(20,{n}) F={F}")
