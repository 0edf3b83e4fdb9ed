"""The fp32-accuracy claim of the split-bf16 dense kernels, tested: dense_x3p_kernel and dense_x3_kernel (forward),
dgrad_x3_kernel, dgrad_span_kernel and wgrad_x3_kernel (backward) against the float64 formula, in the componentwise
metric e = |got - ref64| / den of tests/split3_ref.py, under a bound derived per case from the host model of the
scheme: the geometric mean of the correct six-product scheme's error and the smallest error among the eight one-line
slips (a missing product, a1 w0 issued for a0 w1, a two-way split). tests/test_split3_host.py proves on the CPU that
this bound passes the scheme and fails every slip with 2x of room; here every kernel runs once per case, and every
output element counts. The plain-fp32 kernels behind the variant flags run as controls.

Each test prints one line per output (pytest -s): the figures of profiles/split_accuracy.txt.
"""
import math

import pytest
import torch

import split3_ref as sr

pytestmark = pytest.mark.gpu


def _aligned(*ts):
    return all(t is None or (t.is_contiguous() and t.data_ptr() % 16 == 0 and (t.dim() < 2 or t.stride(0) % 4 == 0))
               for t in ts)


def _upload(case, cuda):
    o = sr.operands(case)
    d = {k: (v.to(cuda) if torch.is_tensor(v) else v) for k, v in o.items() if k != "prm"}
    d["prm"] = {k: v.to(cuda) for k, v in o["prm"].items()}
    return d


def _forward_kernel(case, d, flags):
    """The kernel pg_directgcn_dense_f32 picks (dense_launch's conditions, pg_dense.hip), from the call's arguments."""
    from protgram_directgcn_amd import _lib
    ws_shape = case.F_out == 128 and case.F_in % 4 == 0 and _aligned(d["Z"], d["res_x"], d["constant"])
    if flags & _lib.PG_FLAG_DENSE_TILED or not ws_shape:  # (no row map in these tests)
        return "dense_kernel"
    if case.F_in == 128 and d["W_res"] is None:
        return "dense_x3p_kernel" if _aligned(*[d["prm"][k] for k in sr._W_KEYS]) else None
    if case.F_in == 64 and d["W_res"] is not None:
        return "dense_x3_kernel"
    return "dense_kernel"


def _backward_kernels(case, d, flags, span):
    """(dgrad, wgrad) kernels of dense_bwd_f32_impl (pg_dense_bwd.hip) for the call's arguments."""
    from protgram_directgcn_amd import _lib
    vec = case.F_in % 4 == 0 and case.F_out % 4 == 0 and _aligned(d["Z"], d["dY"], d["res_x"] if case.proj else None)
    x3 = vec and case.F_out % 32 == 0 and (span or not flags & _lib.PG_FLAG_DGRAD_F32MFMA)
    if span:
        ok = x3 and not case.proj and case.F_in % 64 == 0 and (not case.e_res or case.F_in == case.F_out)
        dg = "dgrad_span_kernel" if ok else None
    else:
        dg = "dgrad_x3_kernel" if x3 else "dgrad_kernel" if vec else "dgrad_generic_kernel"
    x3w = case.F_in % 128 == 0 and case.F_out % 128 == 0 and not case.proj and not flags & _lib.PG_FLAG_WGRAD_F32MFMA
    return dg, ("wgrad_x3_kernel" if x3w else "wgrad_kernel") if vec else "wgrad_generic_kernel"


def _control_bound(v):
    """The bound of a plain-fp32 control kernel in the backward: the same geometric mean, with the scheme's error
    replaced by the torch fp32 formula's where that is larger -- an fp32 kernel with longer fp32 chains than the split
    kernels' (wgrad: 32-row steps against 16-row splits) is held to what fp32 gives, still below every slip."""
    b, c = [max(v["model"][x], v["fp32"][x]) for x in (0, 1)], v["mutant_min"]
    return math.sqrt(b[0] * c[0]), math.sqrt(b[1] * c[1])


def _check(case, name, kernel, got, bound=None, mask=None, scale=1.0):
    v = sr.bounds(case)[name]
    r64, den = sr.reference(case)[name]
    got = got.detach().cpu().double() * scale
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    rms, mx = sr.metric(got, r64, den, mask)
    bd = v["bound"] if bound is None else bound
    head = sr.old_tolerance_headroom(case, name, got)
    print(f"\nSPLIT_ACC {case.id:34s} {name:5s} {kernel:21s} fp32 {v['fp32'][0]:.3e} {v['fp32'][1]:.3e}  "
          f"model {v['model'][0]:.3e} {v['model'][1]:.3e}  mutant_min {v['mutant_min'][0]:.3e} {v['mutant_min'][1]:.3e}  "
          f"bound {bd[0]:.3e} {bd[1]:.3e}  measured {rms:.3e} {mx:.3e}  "
          f"(x fp32 {rms / v['fp32'][0]:.2f} {mx / v['fp32'][1]:.2f}; x bound {rms / bd[0]:.2f} {mx / bd[1]:.2f})  "
          f"earlier tolerance used {head:.3f}")
    assert rms <= bd[0], f"{case.id} {name} ({kernel}): rms(e) {rms:.3e} > bound {bd[0]:.3e}"
    assert mx <= bd[1], f"{case.id} {name} ({kernel}): max(e) {mx:.3e} > bound {bd[1]:.3e}"


def _forward(case, cuda, flags, expect):
    from protgram_directgcn_amd import ops
    d = _upload(case, cuda)
    fl = ops.default_flags() | flags
    assert _forward_kernel(case, d, fl | (ops._lib.PG_FLAG_DENSE_PREGATED if case.pre else 0)) == expect
    label = expect + ("+LDSE" if fl & ops._lib.PG_FLAG_DENSE_LDS_EPILOGUE else "")
    drop = None
    if case.drop > 0:
        drop = (case.drop, torch.tensor([sr.DROP_SEED], dtype=torch.int64, device=cuda))
    # no activation in the way (slope 1 where the fused dropout needs one): errors are not scaled by 0.01
    Y = ops.layer_dense(d["Z"], d["prm"], 0 if case.vec else 1, constant=d["constant"], res_x=d["res_x"],
                        W_res=d["W_res"], b_res=d["b_res"], act=case.drop > 0, slope=1.0, flags=fl, pregated=case.pre,
                        drop=drop)
    keep = sr.drop_keep(case)
    if keep is not None:
        assert torch.equal(Y.cpu() == 0, ~keep), "dropped elements"
        _check(case, "Y", label, Y, mask=keep, scale=1.0 / sr.drop_scale(case.drop))
    else:
        _check(case, "Y", label, Y)


def _x3p_variants():
    from protgram_directgcn_amd._lib import PG_FLAG_DENSE_LDS_EPILOGUE
    return [pytest.param(c, fl, id=f"{c.id}-{n}") for c in sr.FWD_X3P + [sr.FWD_DROP, sr.FWD_WIDE]
            for n, fl in (("default", 0), ("lds_epilogue", PG_FLAG_DENSE_LDS_EPILOGUE))
            if fl == 0 or c in sr.FWD_X3P and c.M != 4099]


@pytest.mark.parametrize("case,flags", _x3p_variants())
def test_dense_x3p_fp32_accuracy(pkg, cuda, case, flags):
    """dense_x3p_kernel (F_in = F_out = 128, K = 384): one full tile and a row, 16 tiles and a row, 257 tiles (two on
    one workgroup); vector gates + constant + identity residual and scalar gates without; the ungated and the
    pre-gated operand; the register and the LDS epilogue; the fused dropout (kept elements, 1 / (1 - p) undone; the
    dropped ones exactly 0); and operands spread over 2^[-12, 12], which only a normalised metric can judge."""
    _forward(case, cuda, flags, "dense_x3p_kernel")


@pytest.mark.parametrize("case", sr.FWD_X3, ids=[c.id for c in sr.FWD_X3])
def test_dense_x3_fp32_accuracy(pkg, cuda, case):
    """dense_x3_kernel<64, 4> (F_in = 64 with the projected residual as the fourth K segment, K = 256): one 32-row
    tile and a row, eight and a row; ungated and pre-gated."""
    _forward(case, cuda, 0, "dense_x3_kernel")


def test_dense_tiled_control(pkg, cuda):
    """The tiled fp32 kernel (PG_FLAG_DENSE_TILED) on the first dense_x3p case meets the same bound."""
    from protgram_directgcn_amd._lib import PG_FLAG_DENSE_TILED
    _forward(sr.FWD_X3P[0], cuda, PG_FLAG_DENSE_TILED, "dense_kernel")


def _backward(case, cuda, flags, expect, span=False, control=False):
    from protgram_directgcn_amd import ops
    d = _upload(case, cuda)
    fl = ops.default_flags() | flags
    assert _backward_kernels(case, d, fl, span) == expect
    Y = torch.zeros(case.M, case.F_out, device=cuda)  # not read without the activation
    out = ops.layer_dense_backward(d["dY"], d["Z"], Y, d["prm"], 0 if case.vec else 1,
                                   res_x=d["res_x"] if case.proj else None, W_res=d["W_res"], b_res=d["b_res"],
                                   act=False, flags=fl, span=(d["wdiag"], case.e_res) if span else None)
    assert out is not None, f"{case.id}: the entry point does not take the shape"
    assert torch.equal(out["dpre"], d["dY"])  # no activation: dpre is dY itself
    return out, (lambda name: _control_bound(sr.bounds(case)[name]) if control else None)


@pytest.mark.parametrize("case", sr.DGRAD, ids=[c.id for c in sr.DGRAD])
def test_dgrad_x3_fp32_accuracy(pkg, cuda, case):
    """dgrad_x3_kernel: dZ = s_q (dY (W_q + W_s)) (and dres with a projected residual) at four 32-deep k-tiles and at
    one, with and without the fourth segment, and with dY's columns spread over 2^[-12, 12]."""
    out, _ = _backward(case, cuda, 0, ("dgrad_x3_kernel", "wgrad_x3_kernel" if case.F_in == 128 else "wgrad_kernel"))
    _check(case, "dZ", "dgrad_x3_kernel", out["dZ"])
    if case.proj:
        _check(case, "dres", "dgrad_x3_kernel", out["dres"])


def test_dgrad_f32mfma_control(pkg, cuda):
    from protgram_directgcn_amd._lib import PG_FLAG_DGRAD_F32MFMA
    case = sr.DGRAD[0]
    out, bound = _backward(case, cuda, PG_FLAG_DGRAD_F32MFMA, ("dgrad_kernel", "wgrad_x3_kernel"), control=True)
    _check(case, "dZ", "dgrad_kernel", out["dZ"], bound=bound("dZ"))


def _check_dbsum(case, kernel, got):
    r64, den = sr.reference(case)["dbsum"]
    rms, mx = sr.metric(got.detach().cpu(), r64, den)
    bd = sr.dbsum_bound(case)
    print(f"\nSPLIT_ACC {case.id:34s} dbsum {kernel:21s} bound {bd[0]:.3e} {bd[1]:.3e}  measured {rms:.3e} {mx:.3e}")
    assert rms <= bd[0] and mx <= bd[1], (case.id, kernel, rms, mx, bd)


@pytest.mark.parametrize("case", sr.WGRAD, ids=[c.id for c in sr.WGRAD])
def test_wgrad_x3_fp32_accuracy(pkg, cuda, case):
    """wgrad_x3_kernel: the raw dB [F_out, K] = dY^T (s_q Z_q) over 17 row splits of one 16-row step (the last with a
    single row) and over 129 splits of two steps (the last with three rows); the host model mirrors the splits and
    the fixed-order reduce. The bias sums (plain fp32 sums) against their own derived bound."""
    out, _ = _backward(case, cuda, 0, ("dgrad_x3_kernel", "wgrad_x3_kernel"))
    _check(case, "dB", "wgrad_x3_kernel", out["dB"])
    _check_dbsum(case, "wgrad_x3_kernel", out["dbsum"])


def test_wgrad_f32mfma_control(pkg, cuda):
    from protgram_directgcn_amd._lib import PG_FLAG_WGRAD_F32MFMA
    case = sr.WGRAD[0]
    out, bound = _backward(case, cuda, PG_FLAG_WGRAD_F32MFMA, ("dgrad_x3_kernel", "wgrad_kernel"), control=True)
    _check(case, "dB", "wgrad_kernel", out["dB"], bound=bound("dB"))
    _check_dbsum(case, "wgrad_kernel", out["dbsum"])


@pytest.mark.parametrize("case", sr.SPAN, ids=[c.id for c in sr.SPAN])
def test_dgrad_span_fp32_accuracy(pkg, cuda, case):
    """dgrad_span_kernel: dZ to dgrad_x3_kernel's bound, and E = sum_q wdiag_q dZ_q (+ dpre) against float64 with its
    own normaliser, with and without the residual term."""
    out, _ = _backward(case, cuda, 0, ("dgrad_span_kernel", "wgrad_x3_kernel"), span=True)
    _check(case, "dZ", "dgrad_span_kernel", out["dZ"])
    _check(case, "E", "dgrad_span_kernel", out["E"])
