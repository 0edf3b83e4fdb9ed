"""The pipelined split-bf16 dense kernel's register epilogue (dense_x3p_kernel, pg_dense.hip; the default at
F_in = F_out = 128): its MFMAs take W first, so a lane's four accumulators are four consecutive columns of one output
row, and the constant, the residual and the output are one 16-byte access each per lane. PG_FLAG_DENSE_LDS_EPILOGUE
keeps the earlier epilogue (accumulators, constant and residual rows through LDS). Same six bf16 products in the same
order per output element, same epi_sum: the two must agree bit for bit, and the new path is checked on its own
against the float64 formula of tests/test_gpu_parity.py (test_dense_kernel_variants_vs_float64) with that test's
tolerance.

Row counts (16-row tiles, one workgroup per CU, 256 on MI355X): 1 a partial tile; 16 a full one; 17 a full and a
partial one; 4,099 (257 tiles) one or two tiles per workgroup, workgroups idle where the tile ranges leave none;
12,295 (769 tiles) three or four tiles per workgroup: the steady-state iteration and the drain."""
import pytest
import torch

from test_gpu_parity import _dense_case, assert_close

pytestmark = pytest.mark.gpu

MS = (1, 16, 17, 4099, 12295)
_CASES = {}


def _case(M, vec, cuda):
    """Operands of one (M, gates) case on the device, and the float64 pieces of the reference, made once."""
    key = (M, vec)
    if key not in _CASES:
        Z, xres, prm, const, _, _, _, _ = _dense_case(M, 128, 128, False, vec, False, 4000 + M)
        d = {k: v.double() for k, v in prm.items()}
        gv = (lambda k: d[k][:M]) if vec else (lambda k: d[k].expand(M, 1))
        s = [gv("C_all") * gv("C_directed") * gv("C_in"), gv("C_all") * gv("C_directed") * gv("C_out"),
             gv("C_all") * gv("C_undirected")]
        Wk = [d["W_main_in"] + d["W_shared"], d["W_main_out"] + d["W_shared"], d["W_undirected"] + d["W_shared"]]
        bk = [d["b_main_in"] + d["b_dir_shared_in"], d["b_main_out"] + d["b_dir_shared_out"],
              d["b_undirected"] + d["b_undirected_shared"]]
        Zd = Z.double()
        pre = sum(s[k] * (Zd[:, k * 128:(k + 1) * 128] @ Wk[k].t() + bk[k]) for k in range(3))
        Zg = torch.cat([Z[:, k * 128:(k + 1) * 128] * s[k].float() for k in range(3)], 1)  # fp32 gates: pre-gated Z
        # the constant goes with vector gates only (_dense_case gives none for scalar gates)
        _CASES[key] = dict(Z=Z.to(cuda), Zg=Zg.to(cuda), x=xres.to(cuda), c=const.to(cuda) if vec else None,
                           prm={k: v.to(cuda) for k, v in prm.items()}, pre64=pre, x64=xres.double(),
                           c64=const.double()[:M] if vec else None)
    return _CASES[key]


def _flags():
    from protgram_directgcn_amd import _lib, ops
    return ops.default_flags(), _lib.PG_FLAG_DENSE_LDS_EPILOGUE


def _combos(vec):
    for pre in (False, True):
        for res in (True, False):
            for const in ((True, False) if vec else (False,)):
                for act in (True, False):
                    yield pre, res, const, act


@pytest.mark.parametrize("vec", [True, False], ids=["vector", "scalar"])
@pytest.mark.parametrize("M", MS)
def test_register_epilogue_bitexact(pkg, cuda, M, vec):
    """Default against PG_FLAG_DENSE_LDS_EPILOGUE: torch.equal over pre-gated / ungated Z, identity residual / none,
    constant / none (vector gates), act on / off."""
    from protgram_directgcn_amd import ops
    base, lds = _flags()
    t = _case(M, vec, cuda)
    for pre, res, const, act in _combos(vec):
        kw = dict(constant=t["c"] if const else None, res_x=t["x"] if res else None, act=act, pregated=pre)
        a = ops.layer_dense(t["Zg"] if pre else t["Z"], t["prm"], 0 if vec else 1, flags=base, **kw)
        b = ops.layer_dense(t["Zg"] if pre else t["Z"], t["prm"], 0 if vec else 1, flags=base | lds, **kw)
        assert torch.equal(a, b), (M, vec, pre, res, const, act, float((a - b).abs().max()))


@pytest.mark.parametrize("vec", [True, False], ids=["vector", "scalar"])
@pytest.mark.parametrize("M", MS)
def test_register_epilogue_vs_float64(pkg, cuda, M, vec):
    """The default path against float64: y = act(sum_k s_k (Z_k (W_k + W_s)^T + b_k + b_sk) + constant + residual),
    |d| <= 2e-5 + 2e-5 |ref| (the bound of test_dense_kernel_variants_vs_float64)."""
    from protgram_directgcn_amd import ops
    base, _ = _flags()
    t = _case(M, vec, cuda)
    for pre, res, const, act in _combos(vec):
        y = t["pre64"] + (t["c64"] if const else 0.0) + (t["x64"] if res else 0.0)
        if act:
            y = torch.nn.functional.leaky_relu(y, 0.01)
        out = ops.layer_dense(t["Zg"] if pre else t["Z"], t["prm"], 0 if vec else 1, constant=t["c"] if const else None,
                              res_x=t["x"] if res else None, act=act, pregated=pre, flags=base)
        assert_close(out, y.float(), f"M={M} vec={vec} pre={pre} res={res} const={const} act={act}", rtol=2e-5,
                     atol=2e-5)


@pytest.mark.parametrize("M", MS)
def test_register_epilogue_dropout_bitexact(pkg, cuda, M):
    """The fused layer dropout draws by position (row, column), not by lane: the same mask and bits on both paths, some
    elements dropped and some kept."""
    from protgram_directgcn_amd import ops
    base, lds = _flags()
    t = _case(M, True, cuda)
    seed = torch.tensor([0x1234_5678_9ABC], dtype=torch.int64, device=cuda)
    for pre in (False, True):
        kw = dict(constant=t["c"], res_x=t["x"], act=True, pregated=pre, drop=(0.3, seed))
        a = ops.layer_dense(t["Zg"] if pre else t["Z"], t["prm"], 0, flags=base, **kw)
        b = ops.layer_dense(t["Zg"] if pre else t["Z"], t["prm"], 0, flags=base | lds, **kw)
        assert torch.equal(a, b), (M, pre)
        assert 0 < int((a == 0).sum()) < a.numel()


def test_register_epilogue_ngram_rows(pkg, cuda):
    """layer_dense_ngram_rows at M = 800 (middles 3 and 4 of B(20,3)'s 8,000 rows): residual rows read and output rows
    written at their global n-gram rows; both paths the same bits, every row outside the map keeps the sentinel, and
    the mapped rows equal the unmapped launch on the gathered residual."""
    from protgram_directgcn_amd import ops
    base, lds = _flags()
    M, Kn1, m0, N = 800, 400, 3, 8000
    Z, _, prm, const, _, _, _, _ = _dense_case(M, 128, 128, False, True, False, 77)
    dv = {k: (v[:M] if k.startswith("C_") else v).to(cuda) for k, v in prm.items()}
    X = torch.randn(N, 128, generator=torch.Generator().manual_seed(5)).to(cuda)
    cm = const[:M].to(cuda)
    q, a, b = torch.meshgrid(torch.arange(m0, m0 + M // 400), torch.arange(20), torch.arange(20), indexing="ij")
    rows = (a * Kn1 + q * 20 + b).reshape(-1).to(cuda)
    outs = []
    for fl in (base, base | lds):
        Y = torch.full((N, 128), 7.0, device=cuda)
        r = ops.layer_dense_ngram_rows(Z.to(cuda), dv, 0, Kn1, m0, constant=cm, res_x=X, map_res=True, out=Y,
                                       map_out=True, act=True, flags=fl)
        assert r is Y
        outs.append(Y)
    assert torch.equal(outs[0], outs[1])
    outside = torch.ones(N, dtype=torch.bool, device=cuda)
    outside[rows] = False
    assert int(outside.sum()) == N - M and bool((outs[0][outside] == 7.0).all())
    ref = ops.layer_dense(Z.to(cuda), dv, 0, constant=cm, res_x=X[rows].contiguous(), act=True, flags=base)
    assert torch.equal(outs[0][rows], ref)
