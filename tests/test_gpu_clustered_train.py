"""GPU tests of clustered training: pg_adam_rows_f32 (Adam with row-sparse gradients) bit for bit against pg_adam_f32
on the dense gradient, train_step on subgraphs (original_indices) with the row-sparse path against today's dense path,
and train.fit_clustered against a restatement of the reference's clustered loop
(protgram_directgcn_trainer.py:125-150) on the CPU oracle."""
import random

import pytest
import torch
import torch.nn.functional as F

from oracle import directgcn_cpu as oc
from oracle import graph_cpu as og

pytestmark = pytest.mark.gpu

LR, LAM = 1e-3, 1e-3


# ---------------------------------------------------------------------------------------------
# 1. the kernel, bit for bit
# ---------------------------------------------------------------------------------------------
def _row_sets(n, gen):
    """137 unsorted distinct rows, no row at all (every row only decays), every row (shuffled)."""
    return [torch.randperm(n, generator=gen)[:137], torch.empty(0, dtype=torch.int64), torch.randperm(n, generator=gen)]


# (1000, 128): the 16-B gradient path; (4000, 20): width % 4 == 0 with rows straddling the 16,384-element chunk
# boundary (16384 = 819 * 20 + 4); (3000, 6): a width that is no multiple of 4 -- the per-element gradient path, rows
# straddling (16384 = 2730 * 6 + 4); (20000, 1): a gate vector over two chunks
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(1000, 128), (4000, 20), (3000, 6), (20000, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_adam_rows_bit_identical_to_dense(pkg, cuda, shape, bf16):
    """train.Adam on a filed (compact, rows) gradient against train.Adam on .grad = zeros.index_copy_(0, rows,
    compact), a dense (128, 128) member in the same launch, weight decay 0.01 and the L2 fold on: parameters, both
    moments, the step counter and the folded L2 sum are equal bit for bit over 3 steps with 3 different row sets."""
    from protgram_directgcn_amd import ops, train
    gen = torch.Generator().manual_seed(shape[0] + shape[1] + int(bf16))
    init = [torch.randn(shape, generator=gen).to(cuda), torch.randn(128, 128, generator=gen).to(cuda)]
    sides = []
    for sparse in (False, True):
        ps = [t.clone().requires_grad_(True) for t in init]
        sides.append((ps, train.Adam(ps, lr=3e-3, weight_decay=0.01), sparse))
    for k, rows in enumerate(_row_sets(shape[0], gen)):
        rows = rows.to(cuda)
        compact = (torch.randn(rows.numel(), shape[1], generator=gen) * 10.0 ** -k).to(cuda)
        if bf16:
            compact = compact.to(torch.bfloat16)
        gd = torch.randn(128, 128, generator=gen).to(cuda)
        sums = []
        for ps, opt, sparse in sides:
            ps[1].grad = gd.clone()
            with ops.deferring_const_grads(True):
                if sparse:
                    ps[0].grad = None
                    ops._DEFERRED_GRADS[ps[0].data_ptr()] = (compact, rows)
                else:
                    ps[0].grad = torch.zeros_like(ps[0]).index_copy_(0, rows, compact.float())
                with opt.l2_fold(2e-3, want_sqsum=True):
                    opt.step()
            sums.append(opt._last_sqsum)
            if sparse:
                assert ps[0].grad is None
                assert bool((opt._pos[(cuda, shape[0])] == -1).all())  # the row map is clean between steps
        assert torch.equal(sums[0], sums[1]), (k, float(sums[0]), float(sums[1]))
        for a, b in zip(sides[0][0], sides[1][0]):
            assert torch.equal(a, b), (k, float((a - b).abs().max()))
            for key in ("exp_avg", "exp_avg_sq", "step"):
                assert torch.equal(sides[0][1].state[a][key], sides[1][1].state[b][key]), (k, key)
    assert float(sides[1][1].state[sides[1][0][0]]["step"]) == 3.0


def test_adam_rows_found_inf_and_two_row_sets(pkg, cuda):
    """The found_inf skip through the row-sparse entry (nothing moves, the step counter stays, the L2 sum is still
    returned), and two different rows tensors filed in one step: the dense gradients are built, the same bits."""
    from protgram_directgcn_amd import ops, train
    gen = torch.Generator().manual_seed(5)
    init = [torch.randn(600, 8, generator=gen).to(cuda), torch.randn(600, 1, generator=gen).to(cuda)]
    rows = [torch.randperm(600, generator=gen)[:50].to(cuda), torch.randperm(600, generator=gen)[:70].to(cuda)]
    comp = [torch.randn(50, 8, generator=gen).to(cuda), torch.randn(70, 1, generator=gen).to(cuda)]
    runs = []
    for sparse in (False, True):
        ps = [t.clone().requires_grad_(True) for t in init]
        opt = train.Adam(ps, lr=1e-2)
        for inf in (0.0, 1.0, 0.0):
            opt.grad_scale = torch.full((), 4.0, device=cuda)
            opt.found_inf = torch.full((), inf, device=cuda)
            before = [p.detach().clone() for p in ps]
            with ops.deferring_const_grads(True):
                for p, g, r in zip(ps, comp, rows):
                    if sparse:
                        p.grad = None
                        ops._DEFERRED_GRADS[p.data_ptr()] = (g, r)
                    else:
                        p.grad = torch.zeros_like(p).index_copy_(0, r, g)
                with opt.l2_fold(0.0, want_sqsum=True):
                    opt.step()
            if inf:
                assert all(torch.equal(p, b) for p, b in zip(ps, before))
        runs.append((ps, [opt.state[p] for p in ps], opt._last_sqsum))
        assert float(opt.state[ps[0]]["step"]) == 2.0
    assert torch.equal(runs[0][2], runs[1][2])
    for i in range(2):
        assert torch.equal(runs[0][0][i], runs[1][0][i])
        for key in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(runs[0][1][i][key], runs[1][1][i][key])
    # one rows tensor for both parameters: the sparse launch itself, found_inf and grad_scale included
    ps = [t.clone().requires_grad_(True) for t in init]
    qs = [t.clone().requires_grad_(True) for t in init]
    o1, o2 = train.Adam(ps, lr=1e-2), train.Adam(qs, lr=1e-2)
    g1 = torch.randn(50, 1, generator=gen).to(cuda)
    for inf in (0.0, 1.0, 0.0):
        for opt in (o1, o2):
            opt.grad_scale = torch.full((), 4.0, device=cuda)
            opt.found_inf = torch.full((), inf, device=cuda)
        with ops.deferring_const_grads(True):
            for p, g in zip(ps, (comp[0], g1)):
                ops._DEFERRED_GRADS[p.data_ptr()] = (g, rows[0])
            with o1.l2_fold(0.0, want_sqsum=True):
                o1.step()
        for q, g in zip(qs, (comp[0], g1)):
            q.grad = torch.zeros_like(q).index_copy_(0, rows[0], g)
        with o2.l2_fold(0.0, want_sqsum=True):
            o2.step()
        assert torch.equal(o1._last_sqsum, o2._last_sqsum)
    for p, q in zip(ps, qs):
        assert torch.equal(p, q) and torch.equal(o1.state[p]["exp_avg_sq"], o2.state[q]["exp_avg_sq"])
        assert float(o1.state[p]["step"]) == float(o2.state[q]["step"]) == 2.0


# ---------------------------------------------------------------------------------------------
# 2. and 3.: the 3-gram de Bruijn graph (N = 8000) in 16 subgraphs, as test_clustered_subgraphs_on_gpu builds them
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clusters(pkg, cuda):
    from protgram_directgcn_amd import cluster
    N, s, d, c = pkg.synth.de_bruijn_edges(3)
    mats = og.build_matrices(N, s, d, c)
    ei = {k: v[0].to(cuda) for k, v in mats.items()}
    ew = {k: v[1].to(cuda) for k, v in mats.items()}
    order = pkg.graph.locality_schedule(N, torch.from_numpy(s).to(cuda), torch.from_numpy(d).to(cuda)).long()
    parts = cluster.range_clusters(N, cluster.cluster_count(N), order=order)
    x = torch.randn(N, 32, generator=torch.Generator().manual_seed(1234)).to(cuda)

    def build(classes):
        y = (torch.arange(N, device=cuda) // 400) % classes
        subs = cluster.build_subgraphs(N, parts, ei["in"], ew["in"], ei["out"], ew["out"], ei["und"], ew["und"], x, y)
        assert len(subs) == 16
        return subs

    return N, build


def _model(pkg, cuda, dims, N, classes, dtype=torch.float32):
    torch.manual_seed(0)
    m = pkg.ProtGramDirectGCN(dims, N, classes, 3, 0, 512, 0.5, True).to(cuda).eval()
    m.compute_dtype = dtype
    return m


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_train_step_on_subgraphs_sparse_equals_dense(pkg, cuda, clusters, monkeypatch, dtype):
    """train_step on three clusters: the row-sparse path (the default with train.Adam and no GradScaler) against an
    identically seeded model on today's dense path (train.DEFER_CONST_GRAD = False): every state_dict tensor and the
    loss are bit-identical after each of 3 steps, and on the sparse side the per-node parameters' .grad stay None."""
    from protgram_directgcn_amd import train
    N, build = clusters
    subs = build(20)
    runs = []
    for sparse in (True, False):
        monkeypatch.setattr(train, "DEFER_CONST_GRAD", sparse)
        m = _model(pkg, cuda, [32, 128, 128], N, 20, dtype)
        opt = train.Adam(m.parameters(), lr=LR)
        losses = []
        for sub in (subs[0], subs[5], subs[15]):
            losses.append(train.train_step(m, sub, sub.y, opt, l2_lambda=LAM, weight=sub.num_nodes / N).clone())
            per_node = [p for n, p in m.named_parameters() if n.endswith("constant") or n.endswith("_vec")]
            assert len(per_node) == 12
            assert all((p.grad is None) == sparse for p in per_node)
        runs.append((losses, {k: v.detach().clone() for k, v in m.state_dict().items()}))
    for a, b in zip(*[r[0] for r in runs]):
        assert torch.equal(a, b), (float(a), float(b))
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), (k, float((v - runs[1][1][k]).abs().max()))


def _oracle_fit(sd, dims, subs, N, epochs, dtype=torch.float32):
    """The reference's clustered loop restated on the CPU oracle: per epoch random.shuffle, per cluster zero_grad ->
    forward with original_indices -> nll * n_c / N + lambda * sum ||p||^2 -> backward -> torch.optim.Adam step ->
    epoch_loss += loss.item(); the epoch's loss is epoch_loss / clusters."""
    p = {k: v.detach().to("cpu", dtype, copy=True).requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(p.values()), lr=LR)
    cpu = [dict(x=s.x.cpu().to(dtype), y=s.y.cpu(), oi=s.original_indices.cpu(),
                e=[(getattr(s, "edge_index_" + k).cpu(), getattr(s, "edge_weight_" + k).cpu().to(dtype))
                   for k in ("in", "out", "undirected_norm")]) for s in subs]
    avgs = []
    for _ in range(epochs):
        random.shuffle(cpu)
        total = 0.0
        for s in cpu:
            opt.zero_grad()
            (ei, wi), (eo, wo), (eu, wu) = s["e"]
            lp, _ = oc.model_forward(p, dims, s["x"], ei, wi, eo, wo, eu, wu, original_indices=s["oi"], n_gram_len=3)
            loss = F.nll_loss(lp, s["y"]) * (s["x"].size(0) / N) + LAM * sum(v.norm(2).pow(2) for v in p.values())
            loss.backward()
            opt.step()
            total += loss.item()
        avgs.append(total / len(cpu))
    return avgs, {k: v.detach() for k, v in p.items()}


def beyond(got: dict, ref: dict) -> dict:
    """Per tensor: (max |d|, the number of elements further than 5e-5 from ref, the number allowed)."""
    out = {}
    for k, v in ref.items():
        err = (got[k].detach().cpu().double() - v.double()).abs()
        out[k] = (float(err.max()), int((err > 5e-5).sum()), max(1, err.numel() // 10000))
    return out


# [32, 128, 128] trains the fused head kernel, [32, 32, 16] with 7 classes the framework-ops head
@pytest.mark.parametrize("dims,classes", [([32, 128, 128], 20), ([32, 32, 16], 7)], ids=["128", "16"])
def test_fit_clustered_matches_oracle_loop(pkg, cuda, clusters, dims, classes):
    """train.fit_clustered (train.Adam, the row-sparse path, the L2 fold) for 2 epochs over the 16 subgraphs against
    the restated reference loop on the CPU oracle in fp32 with torch.optim.Adam and the L2 term in the loss, the same
    shuffle seed. Average losses to rtol 1e-5; parameters on Adam's scale, as
    test_train_step_adam_folded_l2_matches_reference_loop: every element within steps * 2 lr, at most
    max(1, numel // 10000) elements of a tensor beyond 5e-5 (32 Adam steps)."""
    from protgram_directgcn_amd import train
    N, build = clusters
    subs = build(classes)
    m = _model(pkg, cuda, dims, N, classes)
    sd0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = train.Adam(m.parameters(), lr=LR)
    random.seed(0)
    hist = train.fit_clustered(train.clustered_step(m, opt, l2_lambda=LAM), list(subs), opt, 2, total_nodes=N)
    assert [h["epoch"] for h in hist] == [1, 2] and hist[0]["lr"] == [LR]
    random.seed(0)
    avgs, ref = _oracle_fit(sd0, dims, subs, N, 2)
    got = [h["loss"] for h in hist]
    stats = beyond(m.state_dict(), ref)
    print("fit_clustered losses", got, "oracle", avgs)
    print("fit_clustered parameters: worst max |d| %.3e, most elements beyond 5e-5 in one tensor %d" %
          (max(v[0] for v in stats.values()), max(v[1] for v in stats.values())))
    assert got == pytest.approx(avgs, rel=1e-5)
    steps = 2 * len(subs)
    for k, (worst, count, allowed) in stats.items():
        assert worst <= steps * 2 * LR + 1e-6, (k, worst)
        assert count <= allowed, (k, count, allowed)
