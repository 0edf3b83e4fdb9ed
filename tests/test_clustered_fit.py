"""CPU-side tests (no GPU) of the clustered trainer's host logic: train.fit_clustered's epoch loop
(protgram_directgcn_trainer.py:125-150) on scripted losses, the argument errors of pg_adam_rows_f32, and the filing of
row-sparse gradients (ops._file_rows / ops.deferred_grad)."""
import ctypes
import random
import types

import pytest
import torch


def _subs(sizes):
    return [types.SimpleNamespace(num_nodes=n, name=i) for i, n in enumerate(sizes)]


def _sgd():
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)


def test_fit_clustered_order_weights_and_average():
    """Per epoch the subgraphs are shuffled in place with random.shuffle (the reference's order under random.seed),
    every cluster takes one step with weight num_nodes / total_nodes, and the epoch's loss is the float64 sum of the
    fp32 cluster losses in visiting order over the number of clusters."""
    from protgram_directgcn_amd import train
    sizes = [500, 500, 499, 501, 250, 7, 120]
    subs = _subs(sizes)
    total = sum(sizes)
    seen, losses = [], []

    def step(sub, weight):
        seen.append((sub.name, weight))
        losses.append(torch.tensor(0.1 + 1e-7 * len(seen) + sub.name, dtype=torch.float32))
        return losses[-1]

    random.seed(7)
    hist = train.fit_clustered(step, subs, _sgd(), 3, total_nodes=total, use_lr_scheduler=False,
                               use_early_stopping=False)
    expect = list(range(len(sizes)))
    random.seed(7)
    for e in range(3):
        random.shuffle(expect)  # the same list shuffled again every epoch, as the reference does
        got = seen[e * len(sizes):(e + 1) * len(sizes)]
        assert [n for n, _ in got] == expect
        assert all(w == sizes[n] / total for n, w in got)
        acc = 0.0
        for v in losses[e * len(sizes):(e + 1) * len(sizes)]:
            acc += v.item()  # the reference's epoch_loss += loss.item()
        assert hist[e]["loss"] == acc / len(sizes) and hist[e]["epoch"] == e + 1 and hist[e]["lr"] == [0.1]
    assert [s.name for s in subs] == expect  # shuffled in place


def test_fit_clustered_zero_total_nodes_and_custom_shuffle():
    from protgram_directgcn_amd import train
    subs = _subs([3, 4])
    weights = []
    hist = train.fit_clustered(lambda sub, w: (weights.append(w), torch.tensor(1.0))[1], subs, _sgd(), 1,
                               total_nodes=0, shuffle=lambda lst: lst.reverse(), use_lr_scheduler=False,
                               use_early_stopping=False)
    assert weights == [0.0, 0.0] and [s.name for s in subs] == [1, 0] and hist[0]["loss"] == 1.0
    with pytest.raises(ValueError):
        train.fit_clustered(lambda sub, w: torch.tensor(1.0), [], _sgd(), 1, total_nodes=1)


def test_fit_clustered_scheduler_and_early_stop_follow_the_average():
    """A scripted plateau: the average stays flat while the last cluster's loss keeps falling, so a loop that fed
    the last cluster's loss to the scheduler or the stopper would neither drop the learning rate nor stop."""
    from protgram_directgcn_amd import train
    subs = _subs([10, 10])
    calls = [0]

    def step(sub, weight):
        calls[0] += 1
        epoch, second = (calls[0] - 1) // 2, (calls[0] - 1) % 2
        # epoch averages: 3.0, 2.0, then 2.0 for ever; the second (last) cluster's loss falls every epoch
        avg = 3.0 if epoch == 0 else 2.0
        last = 1.0 - 0.01 * epoch
        return torch.tensor(last if second else 2 * avg - last, dtype=torch.float32)

    opt = _sgd()
    hist = train.fit_clustered(step, subs, opt, 50, total_nodes=20, shuffle=lambda lst: None, lr_patience=2,
                               lr_factor=0.5, es_patience=6, es_min_delta=1e-5)
    avgs = [h["loss"] for h in hist]
    assert avgs[0] == pytest.approx(3.0) and all(a == pytest.approx(2.0, abs=1e-6) for a in avgs[1:])
    # ReduceLROnPlateau('min', patience 2): best = 2.0 at epoch 2, bad epochs 3, 4, 5 -> reduced after epoch 5
    lrs = [h["lr"][0] for h in hist]
    assert lrs[:5] == [0.1] * 5 and lrs[5] == pytest.approx(0.05)
    # EarlyStopper(patience 6): best at epoch 2, no improvement in epochs 3..8 -> stops at epoch 8
    assert len(hist) == 8 and hist[-1].get("stopped") is True


def test_clustered_step_calls_train_step(monkeypatch):
    from protgram_directgcn_amd import train
    got = []
    monkeypatch.setattr(train, "train_step", lambda *a: (got.append(a), torch.tensor(2.5))[1])
    sub = types.SimpleNamespace(y="labels", num_nodes=5)
    step = train.clustered_step("model", "opt", l2_lambda=1e-3)
    assert float(step(sub, 0.25)) == 2.5
    assert got == [("model", sub, "labels", "opt", 1e-3, None, 0.25)]


def test_adam_rows_argument_errors_without_gpu(pkg):
    lib = pkg.load_library()
    step = ctypes.c_float(0.0)
    sp = ctypes.cast(ctypes.pointer(step), ctypes.c_void_p)

    def call(ntens=1, nchunks=1, step=sp, descs=None, beta1=0.9):
        return lib.pg_adam_rows_f32(ntens, descs, None, nchunks, 1e-3, beta1, 0.999, 1e-8, 0.0, step, None, None, None,
                                    None, None)

    assert call(ntens=-1) == -1 and b"pg_adam_rows_f32" in lib.pg_last_error()
    assert call(nchunks=-1) == -1 and b"bad arguments" in lib.pg_last_error()
    assert call(step=None) == -1 and b"bad arguments" in lib.pg_last_error()
    assert call(beta1=1.0) == -1 and b"hyper" in lib.pg_last_error()
    assert call() == -1 and b"null" in lib.pg_last_error()  # chunks to run but no descriptors


def test_row_sparse_filing_on_cpu_tensors():
    from protgram_directgcn_amd import ops
    N, F = 12, 4
    const = torch.nn.Parameter(torch.randn(N, F))
    gate = torch.nn.Parameter(torch.ones(N, 1))
    rows = torch.tensor([7, 2, 9], dtype=torch.int64)
    dup = torch.tensor([7, 2, 7], dtype=torch.int64)
    g = torch.randn(3, F)
    assert ops.rows_distinct(rows) and not ops.rows_distinct(dup) and ops.rows_info(rows) == (True, 2, 9)
    assert ops.rows_info(torch.empty(0, dtype=torch.int64)) == (True, 0, -1)
    assert not ops._file_rows(const, g, rows) and ops.deferred_grad(const) is None  # the deferral is off
    with ops.deferring_const_grads(True):
        assert ops._file_rows(const, g, rows)
        filed = ops.deferred_grad(const)
        assert isinstance(filed, tuple) and filed[0] is g and filed[1] is rows
        assert ops._file_rows(gate, g[:, :1].to(torch.bfloat16), rows)  # [n_c, 1], bf16: gtype 1
        assert ops.deferred_grad(gate)[0].is_contiguous() and ops.deferred_grad(gate)[0].shape == (3, 1)
        with pytest.raises(RuntimeError):
            ops._file_rows(const, g, rows)  # filed twice
        other = torch.nn.Parameter(torch.randn(N, F))
        assert not ops._file_rows(other * 1.0, g, rows)  # not a leaf: train.Adam never looks its address up
        assert not ops._file_rows(torch.nn.Parameter(torch.randn(N, F), requires_grad=False), g, rows)
        assert not ops._file_rows(other, g, dup)  # index_add_ sums duplicates, the row map cannot
        assert not ops._file_rows(other, g, None) and not ops._file_rows(other, g[:2], rows)
        assert not ops._file_rows(other, g.double(), rows) and not ops._file_rows(other, g, rows.int())
        assert not ops._file_rows(torch.nn.Parameter(torch.randn(N, F).t()), g.t(), rows)  # not contiguous
        assert ops.deferred_grad(other) is None
    assert ops.deferred_grad(const) is None and not ops._DEFERRED_GRADS  # cleared when the scope exits


def test_dense_grads_files_rows_or_builds_the_dense_gradient():
    """ops._dense_grads with rows: under the deferral the constant's and the gate vectors' gradients are filed and
    returned as None; without it (or with duplicate rows) they are today's zeros.index_add_."""
    from protgram_directgcn_amd import ops
    N, M, F_in, F_out = 10, 4, 4, 4
    gen = torch.Generator().manual_seed(0)
    prm = {k: None for k in ops._DENSE_KEYS}
    gates = ("C_in", "C_out", "C_directed", "C_undirected", "C_all")
    for k in gates:
        prm[k] = torch.nn.Parameter(torch.ones(N, 1))
    const = torch.nn.Parameter(torch.randn(N, F_out, generator=gen))
    out = dict(dpre=torch.randn(M, F_out, generator=gen), dB=torch.randn(F_out, 3 * F_in, generator=gen),
               dbsum=torch.randn(4, F_out, generator=gen), dgate=torch.randn(5, M, generator=gen))
    Z = torch.zeros(M, 3 * F_in)
    need = lambda i: True  # noqa: E731

    def run(rows):
        return ops._dense_grads(out, prm, 0, rows, Z, const, None, None, need, True)

    rows = torch.tensor([8, 1, 5, 3])
    grads, d_const, *_ = run(rows)
    dense = dict(zip(ops._DENSE_KEYS, grads))
    assert torch.equal(d_const, torch.zeros(N, F_out).index_add_(0, rows, out["dpre"]))
    with ops.deferring_const_grads(True):
        grads, d_const, *_ = run(rows)
        got = dict(zip(ops._DENSE_KEYS, grads))
        assert d_const is None and all(got[k] is None for k in gates)
        assert all(got[k] is not None for k in ops._DENSE_KEYS if k not in gates)
        g, r = ops.deferred_grad(const)
        assert r is rows and torch.equal(g, out["dpre"])
        for q, k in enumerate(gates):
            g, r = ops.deferred_grad(prm[k])
            assert r is rows and g.shape == (M, 1) and torch.equal(g[:, 0], out["dgate"][q])
            assert torch.equal(torch.zeros(N, 1).index_copy_(0, rows, g), dense[k])
    with ops.deferring_const_grads(True):
        dup = torch.tensor([8, 1, 8, 3])
        grads, d_const, *_ = run(dup)
        assert not ops._DEFERRED_GRADS
        assert torch.equal(d_const, torch.zeros(N, F_out).index_add_(0, dup, out["dpre"]))
        assert torch.equal(dict(zip(ops._DENSE_KEYS, grads))["C_in"],
                           torch.zeros(N, 1).index_add_(0, dup, out["dgate"][0].reshape(-1, 1)))
