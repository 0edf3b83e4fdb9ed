"""The test of the bf16 accuracy tests (no GPU): for every case of tests/test_gpu_bf16_accuracy.py, the host model of
the bf16 dense kernels (tests/bf16_ref.py) meets the criteria the GPU test asserts, and each of the sixteen one-line
slips fails them with room -- at least 1 % of the elements outside the faithful-rounding limit of a bf16 output, or a
normalised metric at least 2x above the bound of an fp32 output, with the model (and the plain torch-fp32 formula) at
least 2x below it -- so no mutated kernel ever has to run on a GPU to know that the GPU test would catch it.

It also records why that test exists: every backward slip, the round-5 gate fault among them, stays inside the
2e-2 max|ref| + 2e-2 |ref| of test_gpu_parity.test_dense_backward_bf16_vs_float64.

'dpre not rounded' is a mutant of dB (and, in the bias dot, of dgate) only; for dZ see bf16_ref's docstring.
"""
import pytest
import torch

import bf16_ref as br

CASE_IDS = [c.id for c in br.CASES]


def test_mutant_table():
    assert {k: len(v) for k, v in br.MUTANTS.items()} == {"Y": 4, "dZ": 4, "dres": 2, "dB": 4, "dgate": 4}
    assert set(br.MUTANTS["dres"]) < set(br.MUTANTS["dZ"])  # s == 1: the two gate-scale slips are none of dres
    assert "round-5 slip" in br.MUTANTS["dgate"] and "dpre not rounded" in br.MUTANTS["dB"]
    assert len({c.id for c in br.CASES}) == len(br.CASES) == 21


def test_ulp_bf16_and_round_to_nearest():
    x = torch.tensor([0.0, 1.0, -1.0, 1.5, 2.0, 255.0, 0.75, 2.0 ** -20, 3.0e38], dtype=torch.float64)
    assert torch.equal(br.ulp_bf16(x), torch.tensor([0.0, 2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 1.0, 2.0 ** -8,
                                                     2.0 ** -27, 2.0 ** 120], dtype=torch.float64))
    g = torch.Generator().manual_seed(3)
    v = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-30, 30, (1 << 16,), generator=g).float())
    d = (br._bf(v).double() - v.double()).abs()
    assert bool((d <= br.ulp_bf16(v.double()) / 2).all())          # one rounding to nearest stays within ulp / 2
    assert bool((d > br.ulp_bf16(v.double()) * 0.49).any())        # ... and comes close to it


def test_gemm16_is_the_product_up_to_its_fp32_roundings():
    g = torch.Generator().manual_seed(4)
    A, B = br._bf(torch.randn(9, 80, generator=g)), br._bf(torch.randn(80, 5, generator=g))
    d = (br.gemm16(A, B).double() - A.double() @ B.double()).abs()
    assert bool((d <= 5 * br.U * (A.double().abs() @ B.double().abs())).all())   # five 16-deep steps
    assert torch.equal(br.gemm16(A, B, tile_bf16=True), br._bf(br.gemm16(A, B, tile_bf16=True)))


def test_act_grad_order():
    d, y = torch.tensor([1.0, 1.0, 1.0, 3.0]), torch.tensor([2.0, -2.0, 0.0, -1.0])
    sl = torch.tensor(0.3)
    assert torch.equal(br.act_grad(d, y, 0.3, 0.0), torch.stack([d[0], d[1] * sl, d[2] * sl, d[3] * sl]))
    ds = br.drop_scale(0.3)
    e = d * torch.tensor(ds)
    assert torch.equal(br.act_grad(d, y, 0.3, ds), torch.stack([e[0], e[1] * sl, torch.tensor(0.0), e[3] * sl]))


def test_wgrad_plans():
    by_id = {c.id: c for c in br.BWD}
    assert br.wgrad_plan(by_id["bwd-M257-128x128"]) == (17, 16)               # staged: one 16-row step per split
    assert br.wgrad_plan(by_id["bwd-M4099-128x128"]) == (129, 32)             # the last split holds three rows
    assert br.wgrad_plan(by_id["bwd-M1025-256x256"]) == (33, 32)
    assert br.wgrad_plan(by_id["bwd-M257-128x128-proj"]) == (17, 16)          # the staged plan serves W_res's columns
    assert br.wgrad_plan(by_id["bwd-M257-128x128-wgrad_tiled"]) == (9, 32)    # tiled: 32-row chunks
    assert br.wgrad_plan(by_id["bwd-M257-64x128-proj"]) == (9, 32)
    assert br.wgrad_plan(by_id["bwd-M129-16x40-proj"]) == (5, 32)


@pytest.mark.parametrize("case", br.CASES, ids=CASE_IDS)
def test_criteria_pass_the_model_and_fail_every_mutant(case):
    o = br.operands(case)
    for k in ("Z", "dY", "res_x"):
        assert o[k] is None or torch.equal(o[k], br._bf(o[k])), k     # bf16-valued storage
    b = br.bounds(case)
    assert list(b) == br.outputs_of(case)
    for name, v in b.items():
        what = f"{case.id} {name}: {v}"
        if name in ("Y", "dZ", "dres"):
            viol, n, worst = v["model"]
            assert viol == 0 and 0 < worst <= 1, "the model is not faithfully rounded: " + what
            assert set(v["mutants"]) == set(br.mutants_of(case, name)) and v["mutants"]
            for mut, (mv, mn, _) in v["mutants"].items():
                assert mv >= 0.01 * mn, f"mutant '{mut}' passes the faithful-rounding limit: " + what
        elif name == "dbsum":
            for x in (0, 1):
                assert 0 < 2 * v["model"][x] <= v["bound"][x], what
        else:
            assert len(v["mutants"]) == 4
            for x in (0, 1):  # rms, max
                assert 0 < 2 * max(v["model"][x], v["fp32"][x]) <= v["bound"][x], "no 2x below the bound: " + what
                for mut, e in v["mutants"].items():
                    assert e[x] >= 2 * v["bound"][x], f"mutant '{mut}' is not 2x above the bound: " + what


@pytest.mark.parametrize("case", br.BWD, ids=[c.id for c in br.BWD])
def test_earlier_tolerance_passes_every_backward_mutant(case):
    """Why the criteria exist: each backward slip uses less than half of the 2 % tolerance of
    test_dense_backward_bf16_vs_float64 on every element of its output."""
    for name in ("dZ", "dres", "dB", "dgate"):
        if name == "dres" and not case.proj:
            continue
        for mut in br.mutants_of(case, name):
            used = br.earlier_tolerance_used(case, name, br.model_outputs(case, name, mut))
            assert used < 0.5, (case.id, name, mut, used)
