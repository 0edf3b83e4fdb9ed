"""The C ABI's memory contract (include/pg_directgcn.h: row-major matrices with an explicit leading dimension,
exact-size flat outputs), entry point by entry point, through ``_lib.load_library()`` directly.

Every matrix operand of a call lives in a guarded buffer (tests/abi_guard.py) in one of four layouts:

  tight    ld = width,     16-B aligned base   the baseline: equals today's ``ops`` result bit for bit
  padded   ld = width + 8, 16-B aligned base   every % 4, % 8 and alignment rule of the header still holds, so the
                                               same kernel runs: bit-equal to ``tight``, for every entry point
  odd      ld = width + 3, aligned base        per entry point, OUTCOME below (taken from the header)
  shifted  ld = width + 8, base one element past a 16-B boundary: OUTCOME below

OUTCOME[entry] = (odd, shifted), each one of
  BITS         PG_OK and the outputs are bit-equal to ``tight`` (the header promises bits: the fp32 CSR family,
               pg_rows_gather / _scatter)
  CLOSE        PG_OK, another kernel of the same contract: within the tolerance the kernel's existing float64 test
               uses (imported from test_gpu_parity: assert_close(rtol = atol = 2e-5) against float64 for the dense
               forward, assert_close's 1e-5 against float64 for the head, assert_grad_close for the backward against
               the ``tight`` result, which equals the ``ops`` result those tests check against float64 autograd)
  UNSUPPORTED  exactly PG_ERR_UNSUPPORTED, a message in pg_last_error(), and the whole output buffer -- view and
               guards -- still the sentinel: nothing was launched.
Anything else fails, so a silent move of a fall-back kernel to "unsupported" (or back) is caught.

In every layout and for every call: every guard of every output is bit-unchanged (front rows, back rows, pad
columns, the head of a shifted first row), every exact-size flat output (work, dW, dgate, gates, grads, loss, partial
sums) is followed by an unchanged tail, and no NaN appears in a result -- the pads of the INPUT buffers are NaN, so
a kernel that folds a pad into a sum fails here as well.
"""
import ctypes

import numpy as np
import pytest
import torch

import abi_guard as ag
from golden_util import load
from test_gpu_parity import _dense_case, assert_close, assert_grad_close

pytestmark = pytest.mark.gpu

LAYOUTS = {"tight": (0, 0), "padded": (8, 0), "odd": (3, 0), "shifted": (8, 1)}  # (ld - width, shift)
ALL = tuple(LAYOUTS)
BITS, CLOSE, UNSUPPORTED = "bits", "close", "unsupported"
PG_OK, PG_ERR_UNSUPPORTED = 0, -3
FULL, PARTIAL, SCRATCH = "full", "partial", "scratch"  # every element written / some left as they were / not compared

# (odd, shifted) per entry point, from the header's requirements
OUTCOME = {
    # fp32 CSR family: 16-B pieces where F, ldx, ldz % 4 == 0 and the bases are aligned, spmm_scalar_kernel otherwise:
    # the same sums in the same order
    "pg_spmm3_f32": (BITS, BITS),
    "pg_spmm3_fusednorm_f32": (BITS, BITS),
    "pg_spmm3_gated_f32": (BITS, BITS),
    "pg_spmm3t_f32": (BITS, BITS),
    "pg_spmm1_f32": (BITS, BITS),
    # "F, ldx, ldz multiples of 8; 16-B aligned (else PG_ERR_UNSUPPORTED)"
    "pg_spmm3_bf16": (UNSUPPORTED, UNSUPPORTED),
    "pg_spmm3t_bf16": (UNSUPPORTED, UNSUPPORTED),
    # n-gram tile kernels: 16-B aligned rows
    "pg_spmm3_ngram_f32": (UNSUPPORTED, UNSUPPORTED),
    "pg_spmm3t_ngram_f32": (UNSUPPORTED, UNSUPPORTED),
    "pg_spmm3t_ngram_bf16": (UNSUPPORTED, UNSUPPORTED),
    "pg_spmm3_ngram_mid_rows_f32": (UNSUPPORTED, UNSUPPORTED),
    "pg_spmm3_ngram_mid_rows_bf16": (UNSUPPORTED, UNSUPPORTED),
    "pg_spmm3t_ngram_scatter_f32": (UNSUPPORTED, UNSUPPORTED),
    "pg_spmm3t_ngram_scatter_bf16": (UNSUPPORTED, UNSUPPORTED),
    "pg_rows_gather_sum": (UNSUPPORTED, UNSUPPORTED),
    # byte-generic rows: 16-B pieces when rows, strides and pointers allow, 4-B words otherwise
    "pg_rows_gather": (BITS, BITS),
    "pg_rows_scatter": (BITS, BITS),
    # dense forward: the tiled kernel's element paths take any layout
    "pg_directgcn_dense_f32": (CLOSE, CLOSE),
    "pg_directgcn_dense_ngram_rows_f32": (UNSUPPORTED, UNSUPPORTED),
    "pg_directgcn_dense_bf16": (UNSUPPORTED, UNSUPPORTED),
    # dense backward: the any-shape kernels (F_out <= 8192)
    "pg_directgcn_dense_bwd_f32": (CLOSE, CLOSE),
    "pg_directgcn_dense_bwd_span_f32": (UNSUPPORTED, UNSUPPORTED),
    "pg_directgcn_dense_bwd_bf16": (UNSUPPORTED, UNSUPPORTED),
    # heads: the VALU kernel takes any layout; the bf16 input has the fast path only
    "pg_directgcn_head_f32": (CLOSE, CLOSE),
    "pg_directgcn_head_bf16": (UNSUPPORTED, UNSUPPORTED),
    "pg_head_train_f32": (UNSUPPORTED, UNSUPPORTED),
    "pg_head_train_bf16": (UNSUPPORTED, UNSUPPORTED),
    "pg_gemm_at_b_f32": (UNSUPPORTED, UNSUPPORTED),
}


def _expect(entry, layout):
    if layout in ("tight", "padded"):
        return BITS
    return OUTCOME[entry][0 if layout == "odd" else 1]


def test_outcome_table_covers_every_listed_entry_point(pkg, cuda):
    """Every entry has both outcomes, and every name is a symbol of the library."""
    from protgram_directgcn_amd import _lib
    for name, oc in OUTCOME.items():
        assert name in _lib.SIGNATURES, name
        assert len(oc) == 2 and set(oc) <= {BITS, CLOSE, UNSUPPORTED}, name


# ---------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------
def _gin(t, layout, name="input"):
    """Input operand: t in the layout, NaN pads and guard rows."""
    extra, shift = LAYOUTS[layout]
    return ag.Guarded.of(t, ld=t.size(1) + extra, shift=shift, name=name)


def _gout(rows, cols, dtype, dev, layout, name, prior=None):
    """Output operand in the layout: all sentinel, or (accumulating calls) the view filled from `prior`."""
    extra, shift = LAYOUTS[layout]
    if prior is not None:  # the output's own sentinel in the guards (an input's NaN carries another payload)
        g = ag.Guarded(prior.size(0), cols, prior.dtype, dev, ld=cols + extra, shift=shift, name=name)
        g.view.copy_(prior)
        g.prior = prior
        return g
    return ag.Guarded(rows, cols, dtype, dev, ld=cols + extra, shift=shift, name=name)


def _flat(n, dev, name, dtype=torch.float32):
    return ag.GuardedFlat(int(n), dtype, dev, name=name)


def _vp(x):
    return ctypes.c_void_p(x if isinstance(x, int) else x.data_ptr())


def _bits(t):
    t = t.contiguous()
    return t.view(ag.SENTINEL[t.dtype][0]) if t.dtype in ag.SENTINEL else t


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _snap(g):
    return g.view.clone(memory_format=torch.contiguous_format)


def _drive(entry, run, close=None, layouts=ALL, what=""):
    """run(layout) -> (rc, {name: (guarded buffer, FULL | PARTIAL | SCRATCH)}). Checks the return code against the
    outcome table, the guards, the NaNs and the results against `tight`; returns the tight results."""
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    assert layouts[0] == "tight"
    base = None
    for lay in layouts:
        rc, outs = run(lay)
        torch.cuda.synchronize()
        want = _expect(entry, lay)
        tag = f"{entry} {what} layout={lay}"
        if want == UNSUPPORTED:
            assert rc == PG_ERR_UNSUPPORTED, f"{tag}: rc {rc}, expected PG_ERR_UNSUPPORTED ({lib.pg_last_error()!r})"
            assert lib.pg_last_error(), f"{tag}: no message"
            for g, _ in outs.values():
                if getattr(g, "prior", None) is not None:  # an accumulating call's output: still its prior contents
                    g.check()
                    assert _same_bits(_snap(g), g.prior), f"{tag}: {g.name} changed by a call that must not launch"
                else:
                    g.assert_untouched()
            continue
        assert rc == PG_OK, f"{tag}: rc {rc}: {lib.pg_last_error()!r}"
        res = {}
        for k, (g, mode) in outs.items():
            if mode == FULL:
                g.assert_written()
            else:
                g.check()
            if mode != SCRATCH:
                res[k] = _snap(g)
        if lay == "tight":
            base = res
            continue
        for k, v in res.items():
            if want == BITS:
                assert _same_bits(v, base[k]), f"{tag}: {k} differs from the tight layout's bits"
            else:
                close(k, v, base[k], tag)
    return base


def _grad_close(k, got, ref, tag):
    assert_grad_close(got.float(), ref.float().cpu(), f"{tag} {k}")


# ---------------------------------------------------------------------------------------------------------------
# CSR propagation family
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def csr(pkg, cuda):
    fx = load("f5_fasta3")
    g = pkg.build_propagation_csr(int(fx["N"][0]), fx["src"], fx["dst"], fx["cnt"], device=cuda)
    assert g.ngram is None and g.symmetric and g.raw is not None
    return g


def _gate_prm(N, F, dev, seed=5):
    gen = torch.Generator().manual_seed(seed)
    prm = {k: (torch.rand(N, 1, generator=gen) + 0.5).to(dev) for k in ("C_in", "C_out", "C_directed", "C_undirected",
                                                                        "C_all")}
    prm["W_main_in"] = torch.zeros(F, F, device=dev)  # only its shape is read
    return prm


CSR_F32 = [("pg_spmm3_f32", 0), ("pg_spmm3_fusednorm_f32", 0), ("pg_spmm3_gated_f32", 0), ("pg_spmm3t_f32", 0),
           ("pg_spmm3t_f32", 1), ("pg_spmm1_f32", 0), ("pg_spmm1_f32", 1)]


@pytest.mark.parametrize("F", [128, 20])
@pytest.mark.parametrize("entry,acc", CSR_F32, ids=[f"{e}-acc{a}" for e, a in CSR_F32])
def test_csr_f32_layouts(pkg, cuda, csr, entry, acc, F):
    """The fp32 CSR family: the vector kernels on tight / padded, spmm_scalar_kernel on odd / shifted (at F = 128 a
    pair no other test runs), flags 0 / 2 / 128: the same bits in all four layouts, prior contents included."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import PG_FLAG_NO_NGRAM, load_library
    lib, g, N = load_library(), csr, csr.n_rows
    transposed, single = entry == "pg_spmm3t_f32", entry == "pg_spmm1_f32"
    xw = 3 * F if transposed else F
    zw = F if (transposed or single) else 3 * F
    gen = torch.Generator().manual_seed(F + acc)
    x = torch.randn(N, xw, generator=gen).to(cuda)
    prior = torch.randn(N, zw, generator=gen).to(cuda) if acc else None
    prm = _gate_prm(N, F, cuda)
    gates, keep = ops._layer_args(None, prm, 0, M=N)
    e1 = g.edges3[:, :2].contiguous()  # {col, w_in}: the single-adjacency records of A_in
    for fl in (0, 2, 128):
        def run(lay):
            X = _gin(x, lay, "X")
            Z = _gout(N, zw, torch.float32, cuda, lay, "Z", prior)
            a = (N, _vp(g.rowptr), _vp(g.row_order) if g.row_order is not None else None)
            s = ops._stream(x)
            if entry == "pg_spmm3_f32":
                rc = lib.pg_spmm3_f32(*a, _vp(g.edges3), _vp(X.ptr()), X.ld, F, _vp(Z.ptr()), Z.ld, fl, s)
            elif entry == "pg_spmm3_fusednorm_f32":
                rc = lib.pg_spmm3_fusednorm_f32(*a, _vp(g.raw), _vp(g.node_norm), g.eps, _vp(X.ptr()), X.ld, F,
                                                _vp(Z.ptr()), Z.ld, fl, s)
            elif entry == "pg_spmm3_gated_f32":
                rc = lib.pg_spmm3_gated_f32(*a, _vp(g.edges3), _vp(X.ptr()), X.ld, F, ctypes.byref(gates), _vp(Z.ptr()),
                                            Z.ld, fl, s)
            elif transposed:
                rc = lib.pg_spmm3t_f32(*a, _vp(g.edges3_t), _vp(X.ptr()), X.ld, F, _vp(Z.ptr()), Z.ld, acc, fl, s)
            else:
                rc = lib.pg_spmm1_f32(*a, _vp(e1), _vp(X.ptr()), X.ld, F, _vp(Z.ptr()), Z.ld, acc, fl, s)
            return rc, {"Z": (Z, FULL)}

        base = _drive(entry, run, what=f"F={F} acc={acc} flags={fl}")["Z"]
        csr_fl = fl | PG_FLAG_NO_NGRAM
        if entry == "pg_spmm3_f32":
            ref = ops.spmm3(g, x, flags=csr_fl)
        elif entry == "pg_spmm3_fusednorm_f32":
            ref = ops.spmm3(g, x, fused=True, flags=fl)
        elif entry == "pg_spmm3_gated_f32":
            ref = ops.spmm3_gated(g, x, prm, 0, flags=fl)
        elif transposed:
            ref = ops.spmm3_t(g, x, flags=csr_fl)
        else:
            ref = ops.spmm3(g, x, flags=csr_fl)[:, :F].contiguous()
        if acc:
            ref = prior + ref  # one fp32 add per element: dX = old + sum
        assert torch.equal(base, ref), (entry, F, acc, fl)
    del keep


@pytest.mark.parametrize("entry", ["pg_spmm3_bf16", "pg_spmm3t_bf16"])
def test_csr_bf16_layouts(pkg, cuda, csr, entry):
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib, g, N, F = load_library(), csr, csr.n_rows, 64
    t = entry == "pg_spmm3t_bf16"
    xw, zw = (3 * F, F) if t else (F, 3 * F)
    x = torch.randn(N, xw, generator=torch.Generator().manual_seed(64)).to(cuda).to(torch.bfloat16)

    def run(lay):
        X, Z = _gin(x, lay, "X"), _gout(N, zw, torch.bfloat16, cuda, lay, "Z")
        fn = lib.pg_spmm3t_bf16 if t else lib.pg_spmm3_bf16
        rc = fn(N, _vp(g.rowptr), _vp(g.row_order) if g.row_order is not None else None,
                _vp(g.edges3_t if t else g.edges3), _vp(X.ptr()), X.ld, F, _vp(Z.ptr()), Z.ld, 0, ops._stream(x))
        return rc, {"Z": (Z, FULL)}

    base = _drive(entry, run)["Z"]
    assert torch.equal(base, ops.spmm3_t(g, x, flags=0) if t else ops.spmm3(g, x, flags=0))


# ---------------------------------------------------------------------------------------------------------------
# n-gram kernels on B(20,3)
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def b3(pkg, cuda):
    N, s, d, c = pkg.synth.de_bruijn_edges(3)
    g = pkg.build_propagation_csr(N, s, d, c, device=cuda)
    assert N == 8000 and g.ngram is not None and g.ngram.mplan is not None
    return g


NGRAM = [("pg_spmm3_ngram_f32", 0), ("pg_spmm3t_ngram_f32", 0), ("pg_spmm3t_ngram_f32", 1), ("pg_spmm3t_ngram_bf16", 0)]


@pytest.mark.parametrize("entry,acc", NGRAM, ids=[f"{e}-acc{a}" for e, a in NGRAM])
def test_ngram_block_layouts(pkg, cuda, b3, entry, acc):
    """The 4x4-block n-gram kernels at F = 64 (16-B aligned rows or PG_ERR_UNSUPPORTED)."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import PG_FLAG_NGRAM_BLOCK4, load_library
    lib, g, N, F = load_library(), b3, b3.n_rows, 64
    ng = g.ngram
    fwd, bf = entry == "pg_spmm3_ngram_f32", entry.endswith("bf16")
    dt = torch.bfloat16 if bf else torch.float32
    xw, zw = (F, 3 * F) if fwd else (3 * F, F)
    gen = torch.Generator().manual_seed(7 + acc)
    x = torch.randn(N, xw, generator=gen).to(cuda).to(dt)
    prior = torch.randn(N, zw, generator=gen).to(cuda).to(dt) if acc else None

    def run(lay):
        X, Z = _gin(x, lay, "X"), _gout(N, zw, dt, cuda, lay, "Z", prior)
        s = ops._stream(x)
        if fwd:
            rc = lib.pg_spmm3_ngram_f32(ng.K, ng.n, N, _vp(ng.plan), _vp(X.ptr()), X.ld, F, None, _vp(Z.ptr()), Z.ld, 0, s)
        else:
            fn = lib.pg_spmm3t_ngram_bf16 if bf else lib.pg_spmm3t_ngram_f32
            rc = fn(ng.K, ng.n, N, _vp(ng.plan), _vp(X.ptr()), X.ld, F, _vp(Z.ptr()), Z.ld, acc, 0, s)
        return rc, {"Z": (Z, FULL)}

    base = _drive(entry, run, what=f"acc={acc}")["Z"]
    ref = ops.spmm3(g, x, flags=PG_FLAG_NGRAM_BLOCK4) if fwd else ops.spmm3_t(g, x, flags=0)
    if acc:  # old + sum: within the tile kernels' fp32 bound of the sum formed outside
        assert_close(base, (prior + ref).cpu(), f"{entry} accumulate")
    else:
        assert torch.equal(base, ref), entry


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_ngram_mid_rows_layouts(pkg, cuda, b3, bf):
    """pg_spmm3_ngram_mid_rows_* over the middles [3, 5) at F = 16: Z has 800 rows, and its guard rows catch a store
    for a middle outside the range."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib, g, N, F, m0, m1 = load_library(), b3, b3.n_rows, 16, 3, 5
    ng = g.ngram
    dt = torch.bfloat16 if bf else torch.float32
    x = torch.randn(N, F, generator=torch.Generator().manual_seed(16)).to(cuda).to(dt)
    entry = "pg_spmm3_ngram_mid_rows_bf16" if bf else "pg_spmm3_ngram_mid_rows_f32"

    def run(lay):
        X, Z = _gin(x, lay, "X"), _gout((m1 - m0) * 400, 3 * F, dt, cuda, lay, "Z")
        rc = getattr(lib, entry)(ng.K, ng.n, N, _vp(ng.mplan), _vp(X.ptr()), X.ld, F, m0, m1, _vp(Z.ptr()), Z.ld, 0,
                                 ops._stream(x))
        return rc, {"Z": (Z, FULL)}

    base = _drive(entry, run)["Z"]
    assert torch.equal(base, ops.spmm3_middles(g, x, m0, m1, flags=0))


@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_ngram_scatter_layouts(pkg, cuda, b3, bf):
    """pg_spmm3t_ngram_scatter_* of two middles at F = 16: T [2400, F] with a padded ldt."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib, g, F, m0, n_mid = load_library(), b3, 16, 3, 2
    splan = ops.ngram_scatter_plan(g, m0, m0 + n_mid)
    dt = torch.bfloat16 if bf else torch.float32
    G = torch.randn(400 * n_mid, 3 * F, generator=torch.Generator().manual_seed(17)).to(cuda).to(dt)
    entry = "pg_spmm3t_ngram_scatter_bf16" if bf else "pg_spmm3t_ngram_scatter_f32"

    def run(lay):
        Gg, T = _gin(G, lay, "G"), _gout(3 * 400 * n_mid, F, torch.float32, cuda, lay, "T")
        rc = getattr(lib, entry)(_vp(splan), n_mid, _vp(Gg.ptr()), Gg.ld, F, _vp(T.ptr()), T.ld, 0, ops._stream(G))
        return rc, {"T": (T, FULL)}

    base = _drive(entry, run)["T"]
    assert torch.equal(base, ops.spmm3t_scatter(splan, G, flags=0))


@pytest.mark.parametrize("b_bf,o_bf", [(False, False), (True, False), (False, True), (True, True)])
def test_rows_gather_sum_layouts(pkg, cuda, b_bf, o_bf):
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    gen = torch.Generator().manual_seed(3)
    F, nA, nB, n_out = 48, 300, 200, 257
    A = torch.randn(nA, F, generator=gen).to(cuda)
    B = torch.randn(nB, F, generator=gen).to(cuda).to(torch.bfloat16 if b_bf else torch.float32)
    cnt = torch.randint(0, 6, (n_out,), generator=gen)
    ptr = torch.zeros(n_out + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(cnt, 0)
    tot = int(ptr[-1])
    idx = torch.where(torch.rand(tot, generator=gen) < 0.4, -1 - torch.randint(0, nB, (tot,), generator=gen),
                      torch.randint(0, nA, (tot,), generator=gen)).to(torch.int32).to(cuda)
    ptr = ptr.to(cuda)
    odt = torch.bfloat16 if o_bf else torch.float32

    def run(lay):
        Ag, Bg, O = _gin(A, lay, "A"), _gin(B, lay, "B"), _gout(n_out, F, odt, cuda, lay, "out")
        rc = lib.pg_rows_gather_sum(_vp(Ag.ptr()), Ag.ld, _vp(Bg.ptr()), Bg.ld, int(b_bf), _vp(ptr), _vp(idx), n_out, F,
                                    _vp(O.ptr()), O.ld, int(o_bf), ops._stream(A))
        return rc, {"out": (O, FULL)}

    base = _drive("pg_rows_gather_sum", run, what=f"b_bf16={b_bf} out_bf16={o_bf}")["out"]
    assert torch.equal(base, ops.rows_gather_sum(A, ptr, idx, n_out, F, B=B, out_dtype=odt))


@pytest.mark.parametrize("F", [128, 6])
@pytest.mark.parametrize("entry", ["pg_rows_gather", "pg_rows_scatter"])
def test_rows_gather_scatter_layouts(pkg, cuda, entry, F):
    """fp32 rows: 16-B pieces on tight / padded at F = 128, 4-B words otherwise; torch indexing's bits everywhere, and
    a scatter leaves the rows it is not given, the pads and the guard rows as they were."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    gen = torch.Generator().manual_seed(F)
    n_src, n = 500, 301
    scatter = entry == "pg_rows_scatter"
    idx = torch.randperm(n_src, generator=gen)[:n].to(cuda)
    src = torch.randn(n if scatter else n_src, F, generator=gen).to(cuda)
    prior = torch.randn(n_src, F, generator=gen).to(cuda) if scatter else None

    def run(lay):
        S = _gin(src, lay, "src")
        D = _gout(n, F, torch.float32, cuda, lay, "dst", prior)
        rc = getattr(lib, entry)(_vp(S.ptr()), S.ld * 4, _vp(idx), n, F * 4, _vp(D.ptr()), D.ld * 4, ops._stream(src))
        return rc, {"dst": (D, FULL)}

    base = _drive(entry, run, what=f"F={F}")["dst"]
    if scatter:
        ref = prior.clone()
        ref[idx] = src
    else:
        ref = src[idx]
    assert torch.equal(base, ref)


# ---------------------------------------------------------------------------------------------------------------
# dense forward
# ---------------------------------------------------------------------------------------------------------------
def _dense_ref64(M, Fin, Fout, Z, xres, prm, const, W_res, b_res, vec):
    """protgram_directgcn.py:100-133 + residual + leaky_relu in float64 (test_dense_kernel_variants_vs_float64's)."""
    d = {k: v.double() for k, v in prm.items()}
    gv = (lambda k: d[k][:M]) if vec else (lambda k: d[k].expand(M, 1))
    s = [gv("C_all") * gv("C_directed") * gv("C_in"), gv("C_all") * gv("C_directed") * gv("C_out"),
         gv("C_all") * gv("C_undirected")]
    Wk = [d["W_main_in"] + d["W_shared"], d["W_main_out"] + d["W_shared"], d["W_undirected"] + d["W_shared"]]
    bk = [d["b_main_in"] + d["b_dir_shared_in"], d["b_main_out"] + d["b_dir_shared_out"],
          d["b_undirected"] + d["b_undirected_shared"]]
    Zd = Z.double()
    y = sum(s[k] * (Zd[:, k * Fin:(k + 1) * Fin] @ Wk[k].t() + bk[k]) for k in range(3))
    if const is not None:
        y = y + const.double()[:M]
    if xres is not None:
        y = y + (xres.double() @ W_res.double().t() + b_res.double() if W_res is not None else xres.double())
    return torch.nn.functional.leaky_relu(y, 0.01).float()


class _Dense:
    """One dense case on the device: operands, the argument block built by ops._layer_args, packed weights."""

    def __init__(self, ops, cuda, M, Fin, Fout, proj, vec, rows=False, seed=0, bf16=False):
        Z, xres, prm, const, r, W_res, b_res, dY = _dense_case(M, Fin, Fout, proj, vec, rows, seed)
        self.M, self.Fin, self.Fout, self.vec, self.gate = M, Fin, Fout, vec, 0 if vec else 1
        self.host = (Z, xres, prm, const, W_res, b_res)
        adt = torch.bfloat16 if bf16 else torch.float32
        self.adt = adt
        self.Z = Z.to(cuda).to(adt)
        self.xres = None if xres is None else xres.to(cuda).to(adt)
        self.dv = {k: v.to(cuda) for k, v in prm.items()}
        # without a row map the kernel reads the constant's rows 0 .. M - 1 only: guard exactly those
        self.const = None if const is None else (const.to(cuda) if rows else const[:M].contiguous().to(cuda))
        self.rows = None if r is None else r.to(cuda)
        self.W_res = None if W_res is None else W_res.to(cuda)
        self.b_res = None if b_res is None else b_res.to(cuda)
        self.dY = dY.to(cuda).to(adt)
        if bf16:
            self.packed, self.p16 = ops.pack_weights_bf16(self.dv, self.W_res, self.b_res)
        else:
            self.packed, self.p16 = ops.pack_weights(self.dv, self.W_res, self.b_res), None

    def args(self, ops, Y=None):
        return ops._layer_args(self.Z, self.dv, self.gate, self.rows, self.const, self.xres, self.W_res, True, 0.01, Y=Y)

    def forward_guards(self, lay, per=None):
        """Guarded Z, constant, res_x (inputs) and Y (output); per = {operand: layout} overrides `lay`."""
        per = per or {}
        Zg = _gin(self.Z, per.get("Z", lay), "Z")
        Cg = None if self.const is None else _gin(self.const, per.get("constant", lay), "constant")
        Rg = None if self.xres is None else _gin(self.xres, per.get("res_x", lay), "res_x")
        Yg = _gout(self.M, self.Fout, self.adt, self.Z.device, per.get("Y", lay), "Y")
        return Zg, Cg, Rg, Yg

    @staticmethod
    def point(a, Zg=None, Cg=None, Rg=None, Yg=None):
        if Zg is not None:
            a.Z, a.ldz = Zg.ptr(), Zg.ld
        if Cg is not None:
            a.constant, a.ld_const = Cg.ptr(), Cg.ld
        if Rg is not None:
            a.res_x, a.ld_res = Rg.ptr(), Rg.ld
        if Yg is not None:
            a.Y, a.ldy = Yg.ptr(), Yg.ld

    def ops_forward(self, ops, flags):
        return ops.layer_dense(self.Z, self.dv, self.gate, rows=self.rows, constant=self.const, res_x=self.xres,
                               W_res=self.W_res, b_res=self.b_res, act=True, flags=flags)

    def ref64(self):
        Z, xres, prm, const, W_res, b_res = self.host
        return _dense_ref64(self.M, self.Fin, self.Fout, Z, xres, prm, const, W_res, b_res, self.vec)


def _tiled():
    from protgram_directgcn_amd._lib import PG_FLAG_DENSE_TILED
    return PG_FLAG_DENSE_TILED


# (M, F_in, F_out, projected residual, vector gates, tiled): the pipelined kernel with a partial tile and with more
# than one tile per workgroup, the 32-row kernel, both tiled widths with a second row tile of one row, an odd shape
DENSE_F32 = [(17, 128, 128, False, True, False), (4099, 128, 128, False, True, False), (33, 64, 128, True, True, False),
             (129, 128, 128, False, True, True), (129, 32, 16, False, False, False), (129, 20, 12, True, True, False)]


@pytest.mark.parametrize("M,Fin,Fout,proj,vec,tiled", DENSE_F32)
def test_dense_forward_f32_layouts(pkg, cuda, M, Fin, Fout, proj, vec, tiled):
    """pg_directgcn_dense_f32 in the four layouts: every layout against float64 within the forward's tolerance
    (rtol = atol = 2e-5), tight == ops.layer_dense, padded == tight."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    c = _Dense(ops, cuda, M, Fin, Fout, proj, vec, seed=M + Fin + Fout)
    fl = _tiled() if tiled else 0
    y64 = c.ref64()

    def run(lay):
        a, keep = c.args(ops)
        Zg, Cg, Rg, Yg = c.forward_guards(lay)
        c.point(a, Zg, Cg, Rg, Yg)
        rc = lib.pg_directgcn_dense_f32(ctypes.byref(a), _vp(c.packed), fl, ops._stream(c.Z))
        torch.cuda.synchronize()
        del keep
        if rc == PG_OK:
            assert_close(Yg.view, y64, f"dense forward {lay} vs float64", rtol=2e-5, atol=2e-5)
        return rc, {"Y": (Yg, FULL)}

    def close(k, got, ref, tag):  # (against float64 above; the fall-back kernel sums in another order than tight's)
        assert got.shape == ref.shape

    base = _drive("pg_directgcn_dense_f32", run, close, what=f"{(M, Fin, Fout, proj, vec, tiled)}")["Y"]
    assert torch.equal(base, c.ops_forward(ops, fl))


@pytest.mark.parametrize("operand,lay", [("Y", "odd"), ("Z", "odd"), ("constant", "odd"), ("res_x", "shifted")])
def test_dense_forward_one_operand_off(pkg, cuda, operand, lay):
    """One operand in a layout off the vector path, the others tight, at F_in = F_out = 128: only Y odd is a vector
    contraction with an element epilogue (vec && !vec_out), only Z odd the reverse; the constant and the identity
    residual alone also take the element epilogue. PG_OK, float64 tolerance, guards intact."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    M, F = 129, 128
    c = _Dense(ops, cuda, M, F, F, False, True, seed=99)
    y64 = c.ref64()
    for fl in (0, _tiled()):
        a, keep = c.args(ops)
        Zg, Cg, Rg, Yg = c.forward_guards("tight", {operand: lay})
        c.point(a, Zg, Cg, Rg, Yg)
        rc = lib.pg_directgcn_dense_f32(ctypes.byref(a), _vp(c.packed), fl, ops._stream(c.Z))
        torch.cuda.synchronize()
        del keep
        assert rc == PG_OK, (operand, lay, fl, lib.pg_last_error())
        Yg.assert_written()
        assert_close(Yg.view, y64, f"dense forward, only {operand} {lay}, flags {fl}", rtol=2e-5, atol=2e-5)


def test_dense_ngram_rows_layouts(pkg, cuda):
    """pg_directgcn_dense_ngram_rows_f32 over two middles of B(20,3) (M = 800), res_x read and Y written at the
    global rows of [8000, 128 (+ pad)] buffers: the unmapped rows, the pads and the guard rows keep the sentinel."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    K, F, n, m0, nm = 20, 128, 3, 7, 2
    N, Kn1 = K ** n, K ** (n - 1)
    M = 400 * nm
    c = _Dense(ops, cuda, M, F, F, False, True, seed=800)
    X = torch.randn(N, F, generator=torch.Generator().manual_seed(8)).to(cuda)
    mm = torch.arange(m0, m0 + nm).view(-1, 1, 1)
    rows = (torch.arange(K).view(1, -1, 1) * Kn1 + mm * K + torch.arange(K).view(1, 1, -1)).reshape(-1).to(cuda)
    mapped = torch.zeros(N, dtype=torch.bool, device=cuda)
    mapped[rows] = True

    def run(lay):
        a, keep = c.args(ops)
        a.res_x, a.ld_res = None, 0
        Zg, Cg = _gin(c.Z, lay, "Z"), _gin(c.const, lay, "constant")
        Rg, Yg = _gin(X, lay, "res_x"), _gout(N, F, torch.float32, cuda, lay, "Y")
        c.point(a, Zg, Cg, Rg, Yg)
        rc = lib.pg_directgcn_dense_ngram_rows_f32(ctypes.byref(a), _vp(c.packed), Kn1, m0, 1, 1, 0, ops._stream(X))
        torch.cuda.synchronize()
        del keep
        if rc == PG_OK:
            assert not bool(torch.isnan(Yg.view[mapped]).any())
            left = _bits(Yg.view[~mapped])
            assert bool((left == ag.SENTINEL[torch.float32][1]).all()), "an unmapped row of Y was written"
        return rc, {"Y": (Yg, PARTIAL)}

    base = _drive("pg_directgcn_dense_ngram_rows_f32", run)["Y"]
    prm = dict(c.dv)
    for k in ("C_in", "C_out", "C_directed", "C_undirected", "C_all"):
        prm[k] = prm[k][:M].contiguous()
    Y = torch.full((N, F), float("nan"), device=cuda)
    ops.layer_dense_ngram_rows(c.Z, prm, 0, Kn1, m0, constant=c.const, res_x=X, map_res=True, out=Y, map_out=True,
                               act=True, flags=0)
    assert torch.equal(base[rows], Y[rows])


@pytest.mark.parametrize("M,Fin,Fout,proj", [(129, 128, 128, False), (129, 64, 128, True)])
def test_dense_forward_bf16_layouts(pkg, cuda, M, Fin, Fout, proj):
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    c = _Dense(ops, cuda, M, Fin, Fout, proj, True, seed=M + Fin, bf16=True)

    def run(lay):
        a, keep = c.args(ops)
        Zg, Cg, Rg, Yg = c.forward_guards(lay)
        c.point(a, Zg, Cg, Rg, Yg)
        rc = lib.pg_directgcn_dense_bf16(ctypes.byref(a), _vp(c.packed), _vp(c.p16), 0, ops._stream(c.Z))
        torch.cuda.synchronize()
        del keep
        return rc, {"Y": (Yg, FULL)}

    base = _drive("pg_directgcn_dense_bf16", run, what=f"{(M, Fin, Fout, proj)}")["Y"]
    assert torch.equal(base, c.ops_forward(ops, 0))


# ---------------------------------------------------------------------------------------------------------------
# dense backward
# ---------------------------------------------------------------------------------------------------------------
def _bwd_flags(name):
    from protgram_directgcn_amd import _lib
    return getattr(_lib, name) if name else 0


def _bwd_run(ops, lib, c, entry, flags, Y, lay, span=None, dpre_f32=False, dpre_f32_lay=None):
    """One backward call with every matrix operand in `lay` (dpre_f32 in dpre_f32_lay when given) and exact-size flat
    outputs; returns (rc, outputs)."""
    from protgram_directgcn_amd._lib import LayerGradArgs
    dev, M, Fin, Fout = c.Z.device, c.M, c.Fin, c.Fout
    proj = c.W_res is not None
    K = (4 if proj else 3) * Fin
    a, keep = ops._layer_args(c.Z, c.dv, c.gate, c.rows, None, c.xres, c.W_res, True, 0.01, Y=Y)
    Zg, Yg, dYg = _gin(c.Z, lay, "Z"), _gin(Y, lay, "Y"), _gin(c.dY, lay, "dY")
    Rg = None if c.xres is None else _gin(c.xres, lay, "res_x")
    c.point(a, Zg=Zg, Rg=Rg, Yg=Yg)
    nwork = int(lib.pg_directgcn_dense_bwd_workspace(ctypes.byref(a)))
    assert nwork > 0
    outs = {"dpre": (_gout(M, Fout, c.adt, dev, lay, "dpre"), FULL),
            "dZ": (_gout(M, 3 * Fin, c.adt, dev, lay, "dZ"), FULL),
            "dgate": (_flat(5 * M, dev, "dgate"), FULL), "gates": (_flat(4 * M, dev, "gates"), FULL),
            "dW": (_flat(Fout * K + 4 * Fout, dev, "dW"), FULL), "work": (_flat(nwork, dev, "work"), SCRATCH)}
    if proj:
        outs["dres"] = (_gout(M, Fin, c.adt, dev, lay, "dres"), FULL)
    if dpre_f32:
        outs["dpre_f32"] = (_gout(M, Fout, torch.float32, dev, dpre_f32_lay or lay, "dpre_f32"), FULL)
    g = LayerGradArgs()
    g.dY, g.lddy = dYg.ptr(), dYg.ld
    g.dpre, g.ldp = outs["dpre"][0].ptr(), outs["dpre"][0].ld
    g.dZ, g.lddz = outs["dZ"][0].ptr(), outs["dZ"][0].ld
    if proj:
        g.dres, g.lddres = outs["dres"][0].ptr(), outs["dres"][0].ld
    if dpre_f32:
        g.dpre_f32, g.ldp_f32 = outs["dpre_f32"][0].ptr(), outs["dpre_f32"][0].ld
    g.dgate, g.gates, g.dW = outs["dgate"][0].ptr(), outs["gates"][0].ptr(), outs["dW"][0].ptr()
    g.work, g.work_floats = outs["work"][0].ptr(), nwork
    s = ops._stream(c.Z)
    if span is not None:
        wdiag, e_res = span
        outs["E"] = (_gout(M, Fin, torch.float32, dev, lay, "E"), FULL)
        rc = lib.pg_directgcn_dense_bwd_span_f32(ctypes.byref(a), _vp(c.packed), ctypes.byref(g), _vp(wdiag),
                                                 _vp(outs["E"][0].ptr()), outs["E"][0].ld, int(e_res), flags, s)
    elif entry.endswith("bf16"):
        rc = lib.pg_directgcn_dense_bwd_bf16(ctypes.byref(a), _vp(c.packed), _vp(c.p16), ctypes.byref(g), flags, s)
    else:
        rc = lib.pg_directgcn_dense_bwd_f32(ctypes.byref(a), _vp(c.packed), ctypes.byref(g), flags, s)
    torch.cuda.synchronize()
    del keep
    return rc, outs


def _bwd_vs_ops(ops, c, base, Y, flags, span=None, dpre_f32=False):
    """The tight layout's outputs equal ops.layer_dense_backward's (what the float64 autograd tests check), bit for bit."""
    proj = c.W_res is not None
    K = (4 if proj else 3) * c.Fin
    packs = [c.packed, c.p16] if c.p16 is not None else None
    ref = ops.layer_dense_backward(c.dY, c.Z, Y, c.dv, c.gate, rows=c.rows, res_x=c.xres, W_res=c.W_res, b_res=c.b_res,
                                   act=True, flags=flags, packs=packs, span=span, dpre_f32=dpre_f32)
    assert ref is not None
    assert torch.equal(base["dpre"], ref["dpre"]) and torch.equal(base["dZ"], ref["dZ"])
    assert torch.equal(base["dgate"].view(5, c.M), ref["dgate"])
    assert torch.equal(base["dW"][:c.Fout * K].view(c.Fout, K), ref["dB"])
    assert torch.equal(base["dW"][c.Fout * K:].view(4, c.Fout), ref["dbsum"])
    if proj:
        assert torch.equal(base["dres"], ref["dres"])
    if span is not None:
        assert torch.equal(base["E"], ref["E"])
    if dpre_f32:
        assert torch.equal(base["dpre_f32"], ref["dpre_f32"])


# (M, F_in, F_out, projected, row map, flag): the MFMA kernels, the 32-row forward's shape with a row map, the
# any-shape kernels, and the two fp32-MFMA opt-outs once each
BWD_F32 = [(129, 128, 128, False, False, ""), (33, 64, 128, True, True, ""), (257, 20, 12, True, False, ""),
           (129, 128, 128, False, False, "PG_FLAG_DGRAD_F32MFMA"), (129, 128, 128, False, False, "PG_FLAG_WGRAD_F32MFMA")]


@pytest.mark.parametrize("M,Fin,Fout,proj,rows,flag", BWD_F32)
def test_dense_backward_f32_layouts(pkg, cuda, M, Fin, Fout, proj, rows, flag):
    """pg_directgcn_dense_bwd_f32: odd / shifted run its any-shape kernels (PG_OK), within assert_grad_close of the
    tight result; work is exactly the workspace query, dW / dgate / gates exact-size with guarded tails."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    c = _Dense(ops, cuda, M, Fin, Fout, proj, True, rows=rows, seed=7 * M + Fin)
    fl = _bwd_flags(flag)
    Y = c.ops_forward(ops, 0)
    entry = "pg_directgcn_dense_bwd_f32"
    base = _drive(entry, lambda lay: _bwd_run(ops, lib, c, entry, fl, Y, lay), _grad_close,
                  what=f"{(M, Fin, Fout, proj, rows, flag)}")
    _bwd_vs_ops(ops, c, base, Y, fl)
    # the fourth bias row is the plain column sum of dpre (b_res's gradient) with or without a projected residual
    assert_grad_close(base["dW"][-Fout:], base["dpre"].double().sum(0).cpu(), "dW bias row 3")


def test_dense_backward_span_layouts(pkg, cuda):
    """pg_directgcn_dense_bwd_span_f32 at (400, 64, 64) with E in the layout (a padded lde among them)."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    c = _Dense(ops, cuda, 400, 64, 64, False, True, seed=464)
    wdiag = torch.rand(400, 3, generator=torch.Generator().manual_seed(4)).to(cuda)
    Y = c.ops_forward(ops, 0)
    entry = "pg_directgcn_dense_bwd_span_f32"
    base = _drive(entry, lambda lay: _bwd_run(ops, lib, c, entry, 0, Y, lay, span=(wdiag, True)), _grad_close)
    _bwd_vs_ops(ops, c, base, Y, 0, span=(wdiag, True))


@pytest.mark.parametrize("M,F,flag", [(129, 128, ""), (300, 256, "PG_FLAG_DGRAD_BF16_RESIDENT"),
                                      (300, 256, "PG_FLAG_DGRAD_BF16_TILED")])
def test_dense_backward_bf16_layouts(pkg, cuda, M, F, flag):
    """pg_directgcn_dense_bwd_bf16 with dpre_f32 given: both input-gradient kernels at (300, 256, 256)."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    c = _Dense(ops, cuda, M, F, F, False, True, seed=13 * M + F, bf16=True)
    fl = _bwd_flags(flag)
    Y = c.ops_forward(ops, 0)
    assert Y.dtype == torch.bfloat16
    entry = "pg_directgcn_dense_bwd_bf16"
    base = _drive(entry, lambda lay: _bwd_run(ops, lib, c, entry, fl, Y, lay, dpre_f32=True), _grad_close,
                  what=f"{(M, F, flag)}")
    _bwd_vs_ops(ops, c, base, Y, fl, dpre_f32=True)


@pytest.mark.parametrize("lay", ["odd", "shifted"])
def test_dense_backward_bf16_only_dpre_f32_off(pkg, cuda, lay):
    """Only the optional fp32 copy of dpre off the 16-B path, every other operand tight: declined like any other
    layout the kernels do not take -- PG_ERR_UNSUPPORTED before the first launch, not an error after it."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    c = _Dense(ops, cuda, 129, 128, 128, False, True, seed=5, bf16=True)
    Y = c.ops_forward(ops, 0)
    rc, outs = _bwd_run(ops, lib, c, "pg_directgcn_dense_bwd_bf16", 0, Y, "tight", dpre_f32=True, dpre_f32_lay=lay)
    assert rc == PG_ERR_UNSUPPORTED and lib.pg_last_error(), (rc, lib.pg_last_error())
    for g, _ in outs.values():
        g.assert_untouched()


# ---------------------------------------------------------------------------------------------------------------
# heads
# ---------------------------------------------------------------------------------------------------------------
def _head_case(M, F, H, C, cuda, seed):
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(M, F, generator=gen)
    W1, b1 = torch.randn(H, F, generator=gen) * 0.2, torch.randn(H, generator=gen) * 0.1
    W2, b2 = torch.randn(C, H, generator=gen) * 0.2, torch.randn(C, generator=gen) * 0.1
    y = torch.randint(0, C, (M,), generator=gen)
    return h, [t.to(cuda) for t in (W1, b1, W2, b2)], (W1, b1, W2, b2), y


@pytest.mark.parametrize("M", [1, 65, 257])
@pytest.mark.parametrize("F,H,C,bf", [(128, 64, 20, False), (34, 17, 3, False), (128, 64, 20, True)])
def test_head_layouts(pkg, cuda, F, H, C, bf, M):
    """pg_directgcn_head_f32 / _bf16: h, logp and emb in the layout; the fp32 head's VALU kernel takes odd / shifted
    (float64 reference, assert_close's 1e-5 as test_head_kernel_vs_torch)."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    h, dev_w, host_w, _ = _head_case(M, F, H, C, cuda, F * 1000 + C + M)
    hd = h.to(cuda).to(torch.bfloat16 if bf else torch.float32)
    h64 = hd.double().cpu()
    W1, b1, W2, b2 = (t.double() for t in host_w)
    lp64 = torch.log_softmax(torch.relu(h64 @ W1.t() + b1) @ W2.t() + b2, dim=-1).float()
    emb64 = (h64 / (torch.norm(h64, p=2, dim=1, keepdim=True) + 1e-12)).float()
    entry = "pg_directgcn_head_bf16" if bf else "pg_directgcn_head_f32"

    def run(lay):
        Hg = _gin(hd, lay, "h")
        Lg, Eg = _gout(M, C, torch.float32, cuda, lay, "logp"), _gout(M, F, torch.float32, cuda, lay, "emb")
        rc = getattr(lib, entry)(M, F, H, C, _vp(Hg.ptr()), Hg.ld, *[_vp(t) for t in dev_w], 1e-12, _vp(Lg.ptr()), Lg.ld,
                                 _vp(Eg.ptr()), Eg.ld, ops._stream(hd))
        torch.cuda.synchronize()
        if rc == PG_OK:
            assert_close(Lg.view, lp64, f"{entry} {lay} log_probs")
            assert_close(Eg.view, emb64, f"{entry} {lay} emb")
        return rc, {"logp": (Lg, FULL), "emb": (Eg, FULL)}

    base = _drive(entry, run, lambda k, got, ref, tag: None, what=f"{(M, F, H, C)}")
    lp, emb = ops.head(hd, *dev_w, 1e-12)
    assert torch.equal(base["logp"], lp) and torch.equal(base["emb"], emb)


@pytest.mark.parametrize("drop", [0.0, 0.5])
@pytest.mark.parametrize("M", [1, 65, 257])
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
def test_head_train_layouts(pkg, cuda, bf, M, drop):
    """pg_head_train_f32 at (128, 64, 20) and pg_head_train_bf16 at (256, 128, 20): h and dh in the layout; grads,
    loss and work exact-size with guarded tails."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    F, H, C = (256, 128, 20) if bf else (128, 64, 20)
    h, dev_w, _, y = _head_case(M, F, H, C, cuda, M + int(drop * 10))
    dt = torch.bfloat16 if bf else torch.float32
    hd, yd = h.to(cuda).to(dt), y.to(cuda)
    seed = torch.tensor([0x1234_5678_9abc_def0 + M], dtype=torch.int64, device=cuda)
    entry = "pg_head_train_bf16" if bf else "pg_head_train_f32"
    nwork = int((lib.pg_head_train_bf16_workspace if bf else lib.pg_head_train_workspace)(M, F, H, C))
    assert nwork > 0

    def run(lay):
        Hg, Dg = _gin(hd, lay, "h"), _gout(M, F, dt, cuda, lay, "dh")
        grads, loss, work = _flat(H * F + H + C * H + C, cuda, "grads"), _flat(1, cuda, "loss"), _flat(nwork, cuda, "work")
        rc = getattr(lib, entry)(M, F, H, C, _vp(Hg.ptr()), Hg.ld, *[_vp(t) for t in dev_w], _vp(yd), 0.75 / M, drop,
                                 _vp(seed) if drop > 0 else None, None, _vp(Dg.ptr()), Dg.ld, _vp(grads.ptr()),
                                 _vp(loss.ptr()), _vp(work.ptr()), nwork, ops._stream(hd))
        return rc, {"dh": (Dg, FULL), "grads": (grads, FULL), "loss": (loss, FULL), "work": (work, SCRATCH)}

    base = _drive(entry, run, what=f"M={M} drop={drop}")
    fn = ops.head_train_bf16 if bf else ops.head_train
    loss, dh, gr = fn(hd, *dev_w, yd, 0.75, drop, seed if drop > 0 else None, None)
    assert torch.equal(base["dh"], dh) and torch.equal(base["loss"].view(()), loss)
    assert torch.equal(base["grads"], torch.cat([t.reshape(-1) for t in gr]))


@pytest.mark.parametrize("M,P,N", [(33, 20, 64), (1000, 128, 384)])
def test_gemm_at_b_layouts(pkg, cuda, M, P, N):
    """pg_gemm_at_b_f32: A, B in the layout; out exactly P*N + P floats, work exactly the workspace query."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    gen = torch.Generator().manual_seed(M + P + N)
    A, B = torch.randn(M, P, generator=gen).to(cuda), torch.randn(M, N, generator=gen).to(cuda)
    nwork = int(lib.pg_gemm_at_b_workspace(M, P, N))
    assert nwork > 0

    def run(lay):
        Ag, Bg = _gin(A, lay, "A"), _gin(B, lay, "B")
        out, work = _flat(P * N + P, cuda, "out"), _flat(nwork, cuda, "work")
        rc = lib.pg_gemm_at_b_f32(M, P, N, _vp(Ag.ptr()), Ag.ld, _vp(Bg.ptr()), Bg.ld, _vp(out.ptr()), _vp(work.ptr()),
                                  nwork, ops._stream(A))
        return rc, {"out": (out, FULL), "work": (work, SCRATCH)}

    base = _drive("pg_gemm_at_b_f32", run, what=f"{(M, P, N)}")["out"]
    Cm, cs = ops.gemm_at_b(A, B)
    assert torch.equal(base[:P * N].view(P, N), Cm) and torch.equal(base[P * N:], cs)
    assert_grad_close(base[:P * N].view(P, N), A.double().t().cpu() @ B.double().cpu(), "A^T B")
    assert_grad_close(base[P * N:], A.double().sum(0).cpu(), "colsum")


# ---------------------------------------------------------------------------------------------------------------
# Adam and the multi-tensor helpers: tensors carved out of one sentinel-filled buffer
# ---------------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 16383, 16384, 16385]


def _table(rows, dev):
    return torch.from_numpy(np.asarray(rows, dtype=np.int64)).to(dev)


def _chunks(lib, sizes, dev):
    cp = np.zeros(len(sizes) + 1, dtype=np.int64)
    for i, n in enumerate(sizes):
        cp[i + 1] = cp[i] + lib.pg_multi_chunks(n)
    return torch.from_numpy(cp).to(dev), int(cp[-1])


def _fill(views, vals):
    for v, t in zip(views, vals):
        v.copy_(t)


@pytest.mark.parametrize("entry", ["pg_adam_f32", "pg_adam_rows_f32", "pg_multi_axpy_f32", "pg_multi_sqsum_f32"])
def test_multi_tensor_carved_buffers(pkg, cuda, entry):
    """Tensors of 1, 3, 16383, 16384 and 16385 elements (a chunk is 16384) at 16-B aligned starts of one buffer with
    sentinel gaps between them, partial sums of exactly nchunks floats: p, m, v, y and every partial equal the same
    call on separately allocated tensors bit for bit, and every gap is unchanged."""
    from protgram_directgcn_amd import ops
    from protgram_directgcn_amd._lib import load_library
    lib = load_library()
    gen = torch.Generator().manual_seed(11)
    rnd = lambda n, s=1.0: (torch.randn(n, generator=gen) * s).to(cuda)  # noqa: E731
    chunk_ptr, nchunks = _chunks(lib, SIZES, cuda)
    assert nchunks == 1 + 1 + 1 + 1 + 2
    s = ops._stream(chunk_ptr)
    n_t = len(SIZES)
    if entry in ("pg_adam_f32", "pg_adam_rows_f32"):
        rows = entry == "pg_adam_rows_f32"
        init = {k: [rnd(n) for n in SIZES] for k in ("p", "g", "m")}
        init["v"] = [rnd(n).abs() for n in SIZES]
        # row-sparse form: width 1, every other parameter row has a gradient row (the compact g holds them in order)
        pos = [torch.where(torch.arange(n) % 2 == 0, torch.arange(n) // 2, torch.full((n,), -1)).to(torch.int32).to(cuda)
               for n in SIZES] if rows else None

        def call(bufs, part, step):
            desc = []
            for i, n in enumerate(SIZES):
                d = [bufs[k][i].data_ptr() for k in ("p", "g", "m", "v")] + [n, 0]
                if rows:
                    d += [pos[i].data_ptr(), 1]
                desc.append(d)
            dt = _table(desc, cuda)
            fn = lib.pg_adam_rows_f32 if rows else lib.pg_adam_f32
            rc = fn(n_t, _vp(dt), _vp(chunk_ptr), nchunks, 1e-3, 0.9, 0.999, 1e-8, 0.01, _vp(step), None, None, _vp(part),
                    None, s)
            torch.cuda.synchronize()
            assert rc == PG_OK, lib.pg_last_error()

        sep = {k: [t.clone() for t in v] for k, v in init.items()}
        part_sep, step_sep = torch.zeros(nchunks, device=cuda), torch.tensor([3.0], device=cuda)
        call(sep, part_sep, step_sep)
        carved = {k: ag.GuardedFlat(SIZES, torch.float32, cuda, gap=8, name=k) for k in ("p", "g", "m", "v")}
        for k in carved:
            _fill(carved[k].views, init[k])
        part, step = _flat(nchunks, cuda, "sq_partial"), _flat(1, cuda, "step")
        step.view.fill_(3.0)
        call({k: c.views for k, c in carved.items()}, part.view, step.view)
        for k in ("p", "m", "v"):
            carved[k].assert_written()
            for i in range(n_t):
                assert torch.equal(carved[k].views[i], sep[k][i]), (entry, k, SIZES[i])
        carved["g"].check()
        for i in range(n_t):
            assert torch.equal(carved["g"].views[i], init["g"][i])  # the gradient is read only
        part.assert_written()
        step.assert_written()
        assert torch.equal(part.view, part_sep) and float(step.view) == 4.0 == float(step_sep)
        return
    xs = [rnd(n) for n in SIZES]
    if entry == "pg_multi_axpy_f32":
        ys = [rnd(n) for n in SIZES]

        def call(xv, yv):
            dt = _table([[x.data_ptr(), y.data_ptr(), n] for x, y, n in zip(xv, yv, SIZES)], cuda)
            rc = lib.pg_multi_axpy_f32(n_t, _vp(dt), _vp(chunk_ptr), nchunks, 0.5, None, s)
            torch.cuda.synchronize()
            assert rc == PG_OK, lib.pg_last_error()

        sep = [y.clone() for y in ys]
        call(xs, sep)
        X, Y = (ag.GuardedFlat(SIZES, torch.float32, cuda, gap=8, name=k) for k in ("x", "y"))
        _fill(X.views, xs)
        _fill(Y.views, ys)
        call(X.views, Y.views)
        Y.assert_written()
        X.check()
        for i in range(n_t):
            assert torch.equal(Y.views[i], sep[i]) and torch.equal(X.views[i], xs[i]), SIZES[i]
        return

    def call(xv, part, out):
        dt = _table([[x.data_ptr(), x.data_ptr(), n] for x, n in zip(xv, SIZES)], cuda)
        rc = lib.pg_multi_sqsum_f32(n_t, _vp(dt), _vp(chunk_ptr), nchunks, _vp(part), _vp(out), s)
        torch.cuda.synchronize()
        assert rc == PG_OK, lib.pg_last_error()

    part_sep, out_sep = torch.zeros(nchunks, device=cuda), torch.zeros(1, device=cuda)
    call(xs, part_sep, out_sep)
    X = ag.GuardedFlat(SIZES, torch.float32, cuda, gap=8, name="x")
    _fill(X.views, xs)
    part, out = _flat(nchunks, cuda, "partial"), _flat(1, cuda, "out")
    call(X.views, part.view, out.view)
    X.check()
    part.assert_written()
    out.assert_written()
    assert torch.equal(part.view, part_sep) and torch.equal(out.view, out_sep)
    ref = sum(float((x.double() ** 2).sum()) for x in xs)
    assert abs(float(out.view) - ref) <= 1e-5 * ref
