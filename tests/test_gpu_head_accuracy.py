"""head_train_kernel and head_train5_kernel (csrc/pg_head_train.hip) at every class count, row tail and hard logit the
trainer can hand them, through ops.head_train and ops.head_train_bf16, against the float64 formula on the same
operands and the same dropout mask (tests/head_ref.py): C in {1, 2, 7, 8, 9, 16, 17, 20, 24, 25, 31, 32} on a tile and
a row or two, single tiles of 1, TR - 1 and TR rows, a workgroup's second tile holding one row, constant labels,
logits of +-120, hidden units that never / always fire, dropout at 0.5 and at 0.9 with a negative seed, and a loss
scale of 65536 with a loss weight of 0.75.

* fp32 outputs (loss, dW1, db1, dW2, db2, the fp32 kernel's dh): rms and max of |got - ref64| / den under the bound
  derived per case from the host model, the torch-fp32 formula and the nearest slip that moves the output;
* the bf16 kernel's dh: every element within ulp_bf16(ref64) / 2 + t;
* the outputs' shapes for the case's C, exact zeros (dead units' dW1 rows and db1 entries; dh of rows whose softmax is
  the one-hot label in the +-120 case), finiteness, and a second call giving the same bits.

tests/test_head_host.py proves on the CPU that these criteria pass the arithmetic the kernels document and fail each
one-line slip of it. Every element of every output counts.

Each test prints one line per output (pytest -s): the figures of profiles/head_accuracy.txt.
"""
import pytest
import torch

import head_ref as hr
from test_gpu_bf16_accuracy import _bits, _spy

pytestmark = pytest.mark.gpu


def _nearest(v, x):
    name = min(v["moving"], key=lambda m: v["mutants"][m][x])
    return name, v["mutants"][name]


def _check(case, kernel, got):
    b = hr.bounds(case)
    for name in hr.OUTPUTS:
        g = got[name].detach().float().cpu()
        v = b[name]
        if name not in hr.fp32_outputs(case):
            assert got[name].dtype == torch.bfloat16
            viol, n, worst = hr.faithful(case, g)
            mname = max(v["mutants"], key=lambda m: v["mutants"][m][0])
            print(f"\nHEAD_ACC {case.id:32s} {name:4s} {kernel:18s} |d| <= ulp / 2 + t, worst |d| / limit: model "
                  f"{v['model'][2]:.3f}  most outside: '{mname}' {100.0 * v['mutants'][mname][0] / n:.1f} %  "
                  f"measured {worst:.3f} ({viol} of {n} outside)")
            assert viol == 0, f"{case.id} {name} ({kernel}): {viol} of {n} elements outside the limit, worst {worst:.3f}x"
            continue
        assert got[name].dtype == torch.float32
        rms, mx = hr.measure(case, name, g)
        bd = v["bound"]
        mname, c = _nearest(v, 0)
        ratio = [0.0 if m == 0 else (m / d if d > 0 else float("inf")) for m, d in ((rms, bd[0]), (mx, bd[1]))]
        print(f"\nHEAD_ACC {case.id:32s} {name:4s} {kernel:18s} model {v['model'][0]:.3e} {v['model'][1]:.3e}  fp32 "
              f"{v['fp32'][0]:.3e} {v['fp32'][1]:.3e}  ulp {v['floor'][0]:.3e} {v['floor'][1]:.3e}  nearest slip '{mname}' {c[0]:.3e} {c[1]:.3e}  bound {bd[0]:.3e} "
              f"{bd[1]:.3e}  measured {rms:.3e} {mx:.3e} (x bound {ratio[0]:.2f} {ratio[1]:.2f})")
        assert rms <= bd[0], f"{case.id} {name} ({kernel}): rms(e) {rms:.3e} > bound {bd[0]:.3e}"
        assert mx <= bd[1], f"{case.id} {name} ({kernel}): max(e) {mx:.3e} > bound {bd[1]:.3e}"


def _run(case, cuda, monkeypatch):
    from protgram_directgcn_amd import ops
    bf = case.kind == "bf16"
    entry, fn, kernel = (("pg_head_train_bf16", ops.head_train_bf16, "head_train5_kernel") if bf else
                         ("pg_head_train_f32", ops.head_train, "head_train_kernel"))
    o = hr.operands(case)
    h = (o["h"].to(torch.bfloat16) if bf else o["h"]).to(cuda)
    assert torch.equal(h.float().cpu(), o["h"])                       # the upload holds the operand exactly
    W1, b1, W2, b2, y = (o[k].to(cuda) for k in ("W1", "b1", "W2", "b2", "y"))
    seed = torch.tensor([case.drop_seed], dtype=torch.int64, device=cuda) if case.drop > 0 else None
    scale = torch.tensor(case.scale, device=cuda) if case.scale > 0 else None
    rcs = _spy(monkeypatch, entry)
    runs = []
    for _ in range(2):
        r = fn(h, W1, b1, W2, b2, y, case.weight, case.drop, seed, scale)
        assert r is not None, f"{case.id}: {entry} does not take the shape"
        loss, dh, (dW1, db1, dW2, db2) = r
        runs.append({"loss": loss, "dh": dh, "dW1": dW1, "db1": db1, "dW2": dW2, "db2": db2})
    torch.cuda.synchronize()
    assert rcs == [0, 0], f"{entry} did not take the call"
    got, again = runs
    M, C, F, H = case.M, case.C, case.F, case.H
    assert {k: tuple(v.shape) for k, v in got.items()} == {"loss": (), "dh": (M, F), "dW1": (H, F), "db1": (H,),
                                                           "dW2": (C, H), "db2": (C,)}
    for k in hr.OUTPUTS:
        assert torch.equal(_bits(got[k]), _bits(again[k])), f"{case.id} {k}: a second call gives other bits"
        assert bool(torch.isfinite(got[k].float()).all()), f"{case.id} {k} is not finite"
    if case.units:  # b1 = -10: never active
        assert not bool(got["dW1"][list(hr.DEAD)].any()) and not bool(got["db1"][list(hr.DEAD)].any())
        assert bool(got["dW1"][list(hr.LIVE)].any(1).all())
    if case.hard:   # rows labelled with the +120 class: softmax == onehot(y) in fp32, so dl and the row's dh are 0
        rows = (o["y"] == C - 1).to(cuda)
        assert not bool(got["dh"][rows].any()) and bool(got["dh"][~rows].any(1).all())
    _check(case, kernel, got)


@pytest.mark.parametrize("case", hr.F32, ids=[c.id for c in hr.F32])
def test_head_train_f32_accuracy(pkg, cuda, monkeypatch, case):
    """head_train_kernel (F = 128, H = 64, 64-row tiles): 8 lanes per row own classes part + 8 u, u < 4."""
    _run(case, cuda, monkeypatch)


@pytest.mark.parametrize("case", hr.BF16, ids=[c.id for c in hr.BF16])
def test_head_train_bf16_accuracy(pkg, cuda, monkeypatch, case):
    """head_train5_kernel (bf16 h, F = 256, H = 128, 16-row tiles): W2 in registers in two zero-filled layouts, class
    tiles 0..15 and 16..31, two-term bf16 splits of every fp32 operand."""
    _run(case, cuda, monkeypatch)


def test_label_check_follows_the_tensor_not_its_address(pkg, cuda):
    """ops._check_labels caches a checked label tensor by (address, size, version, C). A freed label tensor's address
    comes back for the next tensor of its size (the clustered trainer's y[idx] per cluster): an out-of-range label
    there must still raise like F.nll_loss, whether or not the allocator reused the address in this run (printed)."""
    from protgram_directgcn_amd import ops
    case = next(c for c in hr.F32 if c.C == 8)
    o = hr.operands(case)
    args = [o[k].to(cuda) for k in ("h", "W1", "b1", "W2", "b2")]
    y = o["y"].to(cuda)
    ptr, ver = y.data_ptr(), y._version
    assert ops.head_train(*args, y) is not None
    assert ops.head_train(*args, y) is not None              # the cached tensor itself passes again
    del y
    bad_host = o["y"].clone()
    bad_host[case.M // 2] = case.C
    bad = bad_host.to(cuda)                                  # same size and dtype: the freed block
    reused = bad.data_ptr() == ptr and bad._version == ver
    print(f"\nHEAD_LABELS freed label tensor's address reused by the next one: {reused}")
    with pytest.raises(IndexError):
        ops.head_train(*args, bad)
    torch.cuda.synchronize()
