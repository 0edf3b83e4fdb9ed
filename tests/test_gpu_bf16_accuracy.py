"""The bf16 dense kernels' contract, tested: "every sum is fp32, rounded once to bf16 when stored" (pg_bf16.hip).
dense_bf16_kernel (forward), dgrad_bf16r_kernel and dgrad_bf16_kernel, the gate-gradient pass, wgrad_bfs_kernel and
wgrad_bf16_kernel with the split reduction (backward), through ops.layer_dense and ops.layer_dense_backward on bf16
tensors, against the float64 formula on the same rounded operands (tests/bf16_ref.py):

* every element of Y, dZ and dres within the faithful-rounding limit ulp_bf16(ref) / 2 + (K_c + 8) 2^-24 den, the
  dropped elements of the fused dropout exactly 0;
* dpre bit-equal to the host model, dpre_f32 bit-equal to dpre widened;
* dB and dgate in the normalised metric under the bound derived per case from the host model, the torch-fp32 formula
  and the nearest of the output's mutants; dbsum under split3_ref.dbsum_bound.

tests/test_bf16_host.py proves on the CPU that these criteria pass the arithmetic the kernels document and fail each
of sixteen one-line slips of it. Every kernel runs once per case, and every output element counts.

Each test prints one line per output (pytest -s): the figures of profiles/bf16_accuracy.txt.
"""
import pytest
import torch

import bf16_ref as br

pytestmark = pytest.mark.gpu


def _dev(t, cuda, bf16=False):
    if t is None:
        return None
    return (t.to(torch.bfloat16) if bf16 else t).to(cuda)


def _upload(case, cuda):
    o = br.operands(case)
    d = {k: _dev(o[k], cuda, bf16=True) for k in ("Z", "res_x", "dY")}
    d.update({k: _dev(o[k], cuda) for k in ("W_res", "b_res", "constant", "rows")})
    d["Y"] = _dev(o.get("Y"), cuda, bf16=True)
    d["prm"] = {k: v.to(cuda) for k, v in o["prm"].items()}
    for k in ("Z", "res_x", "dY", "Y"):  # the uploads hold the operands' values exactly
        assert d[k] is None or torch.equal(d[k].float().cpu(), o[k]), k
    return d


def _spy(monkeypatch, name):
    """Record the return codes of the C entry point `name`: the test's proof that the bf16 kernels ran (ops falls back
    to the fp32 kernels on widened copies where the entry point answers PG_ERR_UNSUPPORTED)."""
    from protgram_directgcn_amd import load_library
    lib = load_library()
    real, rcs = getattr(lib, name), []

    def call(*a):
        rc = real(*a)
        rcs.append(rc)
        return rc

    monkeypatch.setattr(lib, name, call)
    return rcs


def _forward_kernel(case):
    """pg_directgcn_dense_bf16 (pg_bf16.hip): one kernel, dense_bf16_kernel<128, 128, 8>, where F_in % 8 == 0 and
    F_out % 4 == 0 (the tensors of these tests are contiguous and 16-byte aligned); nothing else."""
    return "dense_bf16_kernel" if case.F_in % 8 == 0 and case.F_out % 4 == 0 else None


def _backward_kernels(case, flags, cu_count):
    """(dgrad, wgrad) kernels of pg_directgcn_dense_bwd_bf16 (pg_dense_bwd.hip) for the call's arguments."""
    from protgram_directgcn_amd import _lib
    if case.F_in % 8 or case.F_out % 8:
        return None
    resident = (case.F_out <= 256 and case.F_out % 64 == 0 and not flags & _lib.PG_FLAG_DGRAD_BF16_TILED and
                (case.M >= 256 * cu_count or bool(flags & _lib.PG_FLAG_DGRAD_BF16_RESIDENT)))
    staged = case.F_in % 128 == 0 and case.F_out % 128 == 0 and not flags & _lib.PG_FLAG_WGRAD_BF16_TILED
    assert staged == br.wgrad_staged(case)  # the plan the host model's row splits follow
    wg = ("wgrad_bfs_kernel+wgrad_bf16_kernel" if case.proj else "wgrad_bfs_kernel") if staged else "wgrad_bf16_kernel"
    return "dgrad_bf16r_kernel" if resident else "dgrad_bf16_kernel", wg


EXPECT = {  # the kernels each backward case is there for
    "bwd-M257-128x128": ("dgrad_bf16r_kernel", "wgrad_bfs_kernel"),
    "bwd-M257-256x256": ("dgrad_bf16r_kernel", "wgrad_bfs_kernel"),
    "bwd-M257-64x128-proj": ("dgrad_bf16r_kernel", "wgrad_bf16_kernel"),
    "bwd-M65-128x64": ("dgrad_bf16r_kernel", "wgrad_bf16_kernel"),
    "bwd-M257-128x128-drop": ("dgrad_bf16r_kernel", "wgrad_bfs_kernel"),
    "bwd-M257-128x128-wide": ("dgrad_bf16r_kernel", "wgrad_bfs_kernel"),
    "bwd-M129-16x40-proj": ("dgrad_bf16_kernel", "wgrad_bf16_kernel"),
    "bwd-M129-64x512": ("dgrad_bf16_kernel", "wgrad_bf16_kernel"),
    "bwd-M257-128x128-dgrad_tiled": ("dgrad_bf16_kernel", "wgrad_bfs_kernel"),
    "bwd-M4099-128x128": ("dgrad_bf16r_kernel", "wgrad_bfs_kernel"),
    "bwd-M1025-256x256": ("dgrad_bf16r_kernel", "wgrad_bfs_kernel"),
    "bwd-M257-128x128-wgrad_tiled": ("dgrad_bf16r_kernel", "wgrad_bf16_kernel"),
    "bwd-M257-128x128-proj": ("dgrad_bf16r_kernel", "wgrad_bfs_kernel+wgrad_bf16_kernel"),
}


def _nearest(mutants, key):
    name = min(mutants, key=lambda m: key(mutants[m]))
    return name, mutants[name]


def _check_faithful(case, name, kernel, got):
    """A bf16 output: every element within the faithful-rounding limit."""
    assert got.dtype == torch.bfloat16
    got = got.detach().float().cpu()
    v = br.bounds(case)[name]
    viol, n, worst = br.faithful(case, name, got)
    mname, (mv, mn, _) = _nearest(v["mutants"], lambda x: x[0])
    used = br.earlier_tolerance_used(case, name, got)
    print(f"\nBF16_ACC {case.id:30s} {name:5s} {kernel:34s} faithful rounding, worst |d| / limit: model "
          f"{v['model'][2]:.3f} ({v['model'][0]} outside)  nearest mutant '{mname}' {100.0 * mv / mn:.1f} % outside  "
          f"measured {worst:.3f} ({viol} of {n} outside)  earlier tolerance used {used:.3f}")
    assert viol == 0, f"{case.id} {name} ({kernel}): {viol} of {n} elements outside the limit, worst {worst:.3f}x"


def _check_metric(case, name, kernel, got):
    """An fp32 output: rms and max of |got - ref64| / den under the case's bound."""
    assert got.dtype == torch.float32
    got = got.detach().cpu()
    v = br.bounds(case)[name]
    r64, den = br.reference(case)[name]
    assert got.shape == r64.shape, (name, got.shape, r64.shape)
    rms, mx = br.metric(got, r64, den)
    bd = v["bound"]
    used = br.earlier_tolerance_used(case, name, got)
    if name == "dbsum":
        print(f"\nBF16_ACC {case.id:30s} {name:5s} {kernel:34s} model {v['model'][0]:.3e} {v['model'][1]:.3e}  "
              f"bound {bd[0]:.3e} {bd[1]:.3e}  measured {rms:.3e} {mx:.3e}  earlier tolerance used {used:.3f}")
    else:
        mname, c = _nearest(v["mutants"], lambda x: x[0])
        print(f"\nBF16_ACC {case.id:30s} {name:5s} {kernel:34s} model {v['model'][0]:.3e} {v['model'][1]:.3e}  "
              f"fp32 {v['fp32'][0]:.3e} {v['fp32'][1]:.3e}  nearest mutant '{mname}' {c[0]:.3e} {c[1]:.3e}  "
              f"bound {bd[0]:.3e} {bd[1]:.3e}  measured {rms:.3e} {mx:.3e} (x bound {rms / bd[0]:.2f} "
              f"{mx / bd[1]:.2f})  earlier tolerance used {used:.3f}")
    assert rms <= bd[0], f"{case.id} {name} ({kernel}): rms(e) {rms:.3e} > bound {bd[0]:.3e}"
    assert mx <= bd[1], f"{case.id} {name} ({kernel}): max(e) {mx:.3e} > bound {bd[1]:.3e}"


@pytest.mark.parametrize("case", br.FWD, ids=[c.id for c in br.FWD])
def test_dense_bf16_faithful_rounding(pkg, cuda, monkeypatch, case):
    """dense_bf16_kernel<128, 128, 8>: one 128-row tile and a row with vector gates + constant + identity residual,
    with scalar gates, and through a row map into a 300-row gate / constant table; the projected residual as the
    fourth K segment; an N tail with a single k-tile (16 -> 40, K = 64); config 5's widths with two column tiles and
    33 row tiles; the fused dropout; and operands spread over 2^[-12, 12]. leaky_relu in every case."""
    from protgram_directgcn_amd import ops
    d = _upload(case, cuda)
    rcs = _spy(monkeypatch, "pg_directgcn_dense_bf16")
    assert _forward_kernel(case) == "dense_bf16_kernel"
    drop = (case.drop, torch.tensor([br.DROP_SEED], dtype=torch.int64, device=cuda)) if case.drop > 0 else None
    Y = ops.layer_dense(d["Z"], d["prm"], 0 if case.vec else 1, rows=d["rows"], constant=d["constant"],
                        res_x=d["res_x"], W_res=d["W_res"], b_res=d["b_res"], act=True, slope=br.SLOPE, drop=drop)
    assert rcs == [0], "pg_directgcn_dense_bf16 did not take the call"
    if case.drop > 0:
        assert torch.equal(Y.float().cpu() == 0, ~br.drop_keep(case)), "dropped elements"
    _check_faithful(case, "Y", "dense_bf16_kernel", Y)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _run_backward(case, d, flags, cuda):
    from protgram_directgcn_amd import ops
    out = ops.layer_dense_backward(d["dY"], d["Z"], d["Y"], d["prm"], 0 if case.vec else 1,
                                   res_x=d["res_x"] if case.proj else None, W_res=d["W_res"], b_res=d["b_res"],
                                   act=True, slope=br.SLOPE, flags=flags, drop_p=case.drop, dpre_f32=True)
    assert out is not None, f"{case.id}: the entry point does not take the shape"
    return out


@pytest.mark.parametrize("case", br.BWD, ids=[c.id for c in br.BWD])
def test_dense_backward_bf16_contract(pkg, cuda, monkeypatch, case):
    """pg_directgcn_dense_bwd_bf16, every output of every case. dgrad_bf16r_kernel (forced below its 256 rows per CU by
    PG_FLAG_DGRAD_BF16_RESIDENT): two, four and one k-tile, three to six n-tiles, with dres, one 64-row block and a
    row up to 65 blocks; dgrad_bf16_kernel at the shapes only it takes (F_out = 40: partial k- and n-tiles; F_out =
    512) and, by its flag, at the resident kernel's, where its outputs are also bit-equal to that kernel's.
    wgrad_bfs_kernel: 17 one-step splits, 129 two-step splits ending in three rows, four output tiles;
    wgrad_bf16_kernel by its flag, at F_in = 64 and 16, and beside the staged kernel for W_res's columns. act' with a
    slope in every case, with the fused dropout's zeros in one, dY's columns spread over 2^[-12, 12] in another."""
    from protgram_directgcn_amd import _lib, ops
    d = _upload(case, cuda)
    forced = _lib.PG_FLAG_DGRAD_BF16_RESIDENT
    fl = ops.default_flags() | {"": forced, "dgrad_tiled": _lib.PG_FLAG_DGRAD_BF16_TILED,
                                "wgrad_tiled": forced | _lib.PG_FLAG_WGRAD_BF16_TILED}[case.variant]
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    kernels = _backward_kernels(case, fl, cus)
    assert kernels == EXPECT[case.id]
    dg, wg = kernels
    rcs = _spy(monkeypatch, "pg_directgcn_dense_bwd_bf16")
    out = _run_backward(case, d, fl, cuda)
    assert rcs == [0], "pg_directgcn_dense_bwd_bf16 did not take the call"

    P = br.prepared(case)
    assert out["dpre"].dtype == torch.bfloat16 and out["dpre_f32"].dtype == torch.float32
    assert torch.equal(_bits(out["dpre"].cpu()), _bits(P.dpre.to(torch.bfloat16))), "dpre is not the model's, bit for bit"
    assert torch.equal(_bits(out["dpre_f32"]), _bits(out["dpre"].float())), "dpre_f32 is not dpre widened"
    print(f"\nBF16_ACC {case.id:30s} dpre  {dg:34s} bit-equal to the host model; dpre_f32 bit-equal to dpre widened")
    _check_faithful(case, "dZ", dg, out["dZ"])
    if case.proj:
        _check_faithful(case, "dres", dg, out["dres"])
    _check_metric(case, "dgate", dg + "+gate_grad_kernel", out["dgate"])
    _check_metric(case, "dB", wg, out["dB"])
    _check_metric(case, "dbsum", wg, out["dbsum"])

    if case.variant == "dgrad_tiled":  # the same operands on the resident kernel: every output bit for bit
        fr = ops.default_flags() | _lib.PG_FLAG_DGRAD_BF16_RESIDENT
        assert _backward_kernels(case, fr, cus) == ("dgrad_bf16r_kernel", "wgrad_bfs_kernel")
        res = _run_backward(case, d, fr, cuda)
        for k in ("dpre", "dpre_f32", "dZ", "dgate", "dB", "dbsum"):
            assert torch.equal(_bits(out[k]), _bits(res[k])), f"{k}: dgrad_bf16_kernel and dgrad_bf16r_kernel differ"
