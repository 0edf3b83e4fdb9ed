#!/usr/bin/env python3
"""Louvain community labels on the GPU, level by level: on the bench's FASTA-built 4-gram level (bench.py --graph
fasta: ngram_transitions over synth.protein_sequences(8000, 350, seed=1)) and on the 5-gram level of the same sequences
it prints, per Louvain level, the nodes and CSR entries, the cycles and sweep launches, the milliseconds in the sweep
kernel (device events around every launch), in the level's cycles as a whole (per-community sums, the modularity
check and its host read included) and in the aggregation, the modularity Q and the community count; then the wall time
of the whole ngram.community_labels call. --grid adds the complete 5-gram grid B(20, 5) (N = 3.2M, 64M transitions).

The host baseline at these sizes is NOT measured: python-louvain is not installed. For scale only, the plain-Python
sequential yardstick (tests/louvain_ref.py) is timed on the tests' 3-gram level (N = 6,903), where it finishes.

Usage: python tools/louvain_probe.py [--out profiles/louvain_probe.txt] [--classes 4] [--skip-5gram] [--grid]
"""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def probe(pkg, name, t, classes, emit):
    cm = pkg.community
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g = cm.combined_graph(t)
    torch.cuda.synchronize()
    t_graph = time.perf_counter() - t0
    emit(f"{name}: N = {g.n:,}, undirected edges = {int((g.row <= g.col).sum()):,}, 2m = {g.two_m:,}, "
         f"classes = {classes}; graph build {t_graph * 1e3:.1f} ms")
    cm.louvain(g, classes=classes)  # warm-up: library load, allocator
    stats = []
    labels = cm.louvain(g, classes=classes, stats=stats)
    emit("  level     nodes     entries  cycles  launches   kernel ms  cycles ms  aggregate ms         Q  communities")
    for i, s in enumerate(stats):
        emit(f"  {i:5d} {s['nodes']:9,d} {s['entries']:11,d} {s['cycles']:7d} {s['launches']:9d} {s['kernel_ms']:11.3f} "
             f"{s['cycles_s'] * 1e3:10.1f} {s['aggregate_s'] * 1e3:13.1f} {s['q']:9.6f} {s.get('communities', '-'):>12}")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    again, num = pkg.ngram.community_labels(t, classes=classes)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    emit(f"  community_labels: {wall * 1e3:.1f} ms wall, {num:,} communities, Q = {cm.modularity(g, again):.6f}, "
         f"same labels as the timed run: {bool(torch.equal(labels, again))}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "louvain_probe.txt"))
    ap.add_argument("--classes", type=int, default=4)
    ap.add_argument("--fasta-seqs", type=int, default=8000)
    ap.add_argument("--skip-5gram", action="store_true")
    ap.add_argument("--grid", action="store_true", help="add the complete 5-gram grid B(20, 5)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("louvain_probe.py: no GPU (a time taken elsewhere says nothing)")
    pkg = load_package()
    dev = torch.device("cuda:0")
    lines = []

    def emit(line):
        print(line, flush=True)
        lines.append(line)

    emit(f"louvain_probe on {torch.cuda.get_device_name(0)}")
    seqs = pkg.synth.protein_sequences(args.fasta_seqs, 350, seed=1)
    for n in (4,) if args.skip_5gram else (4, 5):
        t = pkg.ngram.ngram_transitions(seqs, n, device=dev)
        probe(pkg, f"fasta {n}-gram", t, args.classes, emit)
        del t
        torch.cuda.empty_cache()
    if args.grid:
        N, s, d, c = pkg.synth.de_bruijn_edges(5)
        t = pkg.ngram.NgramTransitions(5, N, torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev),
                                       torch.from_numpy(c).to(dev), torch.arange(N, dtype=torch.int64, device=dev),
                                       pkg.synth.ALPHABET)
        probe(pkg, "grid 5-gram", t, args.classes, emit)

    import louvain_ref as ref
    small = pkg.ngram.preprocess(pkg.synth.protein_sequences(150, mean_len=200, seed=2))
    N, s, d, c, _ = pkg.synth.fasta_edges(3, small)
    edges = ref.undirected_edges(s, d, c)
    t0 = time.perf_counter()
    lab = ref.louvain_seq(N, edges, 0)
    emit(f"host yardstick (plain Python, sequential, seed 0) on the 3-gram test level, N = {N:,}, {len(edges):,} edges: "
         f"{(time.perf_counter() - t0) * 1e3:.0f} ms, Q = {ref.modularity(N, edges, lab):.4f}")
    emit("host baseline at the 4-gram and 5-gram sizes: not measured (python-louvain is not installed)")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
