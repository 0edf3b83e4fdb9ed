#!/usr/bin/env python3
"""Cluster-GCN training epoch on the 4-gram graph over subgraphs from cluster.build_subgraphs (320 clusters of ~500
nodes, the reference's default for N > 10k). Prints the subgraph build time, ms per subgraph step and one JSON line.

default: the reference's _train_model_clustered loop (protgram_directgcn_trainer.py:125-141: per subgraph zero_grad ->
         autocast forward -> weighted nll + L2 -> GradScaler backward/step, loss.item() per step), torch.optim.Adam
--ours:  train.fit_clustered over the same subgraphs with train.Adam and no GradScaler: the per-node parameters'
         gradients reach Adam row-sparse (pg_adam_rows_f32); with --dense-grads they are built as N x F tensors
         (train.DEFER_CONST_GRAD = False), the path before the row-sparse one
usage: python tools/cluster_probe.py [ngram] [dims=128,128,128] [--ours [--dense-grads]] [--epochs E]"""
import argparse
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
from protgram_directgcn_amd import cluster, train  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("ngram", nargs="?", type=int, default=4)
ap.add_argument("dims", nargs="?", default="128,128,128")
ap.add_argument("--ours", action="store_true", help="train.fit_clustered with train.Adam, no GradScaler")
ap.add_argument("--dense-grads", action="store_true",
                help="with --ours: dense N x F gradients for the per-node parameters")
ap.add_argument("--epochs", type=int, default=1, help="timed epochs (after one warm-up epoch)")
ap.add_argument("--l2", type=float, default=1e-7)
args = ap.parse_args()
n = args.ngram
dims = [int(v) for v in args.dims.split(",")]
dev = torch.device("cuda:0")
N, s, d, c = pkg.synth.de_bruijn_edges(n)
g = pkg.build_propagation_csr(N, s, d, c, device=dev)
# the reference matrices as COO (what the trainer slices): the shared pattern with the three weights
rows = torch.repeat_interleave(torch.arange(N, device=dev), g.rowptr[1:] - g.rowptr[:-1])
ei = torch.stack([g.edges3[:, 0].long(), rows])
w = [g.edges3[:, k].contiguous().view(torch.float32) for k in (1, 2, 3)]
x = torch.randn(N, dims[0], generator=torch.Generator().manual_seed(1234)).to(dev)
y = (torch.arange(N, device=dev) // (20 ** (n - 1)))
torch.cuda.synchronize()
t0 = time.perf_counter()
parts = cluster.range_clusters(N, cluster.cluster_count(N), order=g.row_order.long())
subs = cluster.build_subgraphs(N, parts, ei, w[0], ei, w[1], ei, w[2], x, y)
torch.cuda.synchronize()
t_build = time.perf_counter() - t0
kept = sum(dd.graph.nnz for dd in subs)
print(f"{len(subs)} subgraphs built in {t_build:.3f}s; intra-cluster entries {kept} of {g.nnz} "
      f"({100.0 * kept / g.nnz:.1f}%)")

torch.manual_seed(0)
model = pkg.ProtGramDirectGCN(dims, N, int(y.max()) + 1, n, 0, 512, 0.5, True).to(dev).train()

if args.ours:
    mode = "ours_dense" if args.dense_grads else "ours_sparse"
    train.DEFER_CONST_GRAD = not args.dense_grads
    opt = train.Adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    step = train.clustered_step(model, opt, l2_lambda=args.l2)

    def epochs(k):
        return train.fit_clustered(step, subs, opt, k, total_nodes=N, use_lr_scheduler=False,
                                   use_early_stopping=False)[-1]["loss"]
else:
    mode = "reference_loop"
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, weight_decay=0.0)
    scaler = torch.amp.GradScaler("cuda", enabled=True)

    def epoch():
        random.shuffle(subs)
        tot = 0.0
        for bd in subs:
            opt.zero_grad()
            with torch.amp.autocast("cuda", enabled=True):
                out, _ = model(data=bd)
                loss = F.nll_loss(out, bd.y) * (bd.num_nodes / N)
                loss = loss + args.l2 * sum(p.norm(2).pow(2) for p in model.parameters() if p.requires_grad)
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            tot += loss.item()  # the reference's per-step host sync (trainer :140)
        return tot / len(subs)

    def epochs(k):
        for _ in range(k):
            avg = epoch()
        return avg


random.seed(0)
epochs(1)
torch.cuda.synchronize()
peak0 = torch.cuda.max_memory_allocated()
torch.cuda.reset_peak_memory_stats()
t0 = time.perf_counter()
avg = epochs(args.epochs)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / args.epochs
print(f"[{mode}] epoch {dt:.3f}s = {1e3 * dt / len(subs):.3f} ms per subgraph step (avg loss {avg:.4f})")
print(json.dumps(dict(mode=mode, ngram=n, dims=dims, clusters=len(subs), epochs=args.epochs, epoch_ms=1e3 * dt,
                      step_ms=1e3 * dt / len(subs), avg_loss=avg, build_s=t_build,
                      peak_alloc_mb=torch.cuda.max_memory_allocated() / 2 ** 20, warm_peak_alloc_mb=peak0 / 2 ** 20)))
