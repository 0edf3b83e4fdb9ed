#!/usr/bin/env python3
"""Timing of the closest_aa label path on the GPU: ngram.letter_masks plus the k = 3 launches of pg_reach_hop_u32, on

* the bench's FASTA-built 4-gram level (bench.py --graph fasta: ngram_transitions over
  synth.protein_sequences(8000, 350, seed=1)), and
* the complete 5-gram grid B(20, 5) (N = 3.2M, E = 64M),

with HIP events after warm-up, the median of --reps repetitions per launch. Every hop is set against its byte floor
8E + 8(N + 1) + 8N (col, rowptr, one read and one write of the reach words) at the 6.3 TB/s achievable HBM rate;
`frac` is floor / measured. The hops are timed in the two forms the package uses: `labels` (closest_aa_labels: target
and labels outputs) and `dist` (letter_distances: the [N, 20] byte table). For contrast the plain-Python per-node BFS
(tests/closest_aa_ref.py) is timed on the p1 fixture's 3-gram level (763 nodes) on the host.

Prints one JSON line and writes it to --out.
Usage: python tools/closest_aa_probe.py [--out profiles/closest_aa_probe.json] [--reps 30] [--skip-grid]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

HBM_BYTES_PER_S = 6.3e12  # achievable HBM rate (MI355X_MICROARCH.md)
K_HOPS = 3


def timed(fn, reps):
    """Median device time of fn() in microseconds (HIP events around each call, after two warm-up calls)."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3)
    return statistics.median(out)


def probe_level(pkg, t, reps):
    ng = pkg.ngram
    lib = pkg.load_library()
    dev = t.src.device
    N, E, L = int(t.num_nodes), int(t.src.numel()), len(ng.AMINO_ACIDS)
    rowptr, col = ng._out_csr(t, dev)
    masks = ng.letter_masks(t)
    keys = t.node_keys.to(dev).contiguous()
    code_bit = torch.tensor([ng.AMINO_ACIDS.find(ch) for ch in t.alphabet], dtype=torch.int32).to(dev)
    again = torch.empty_like(masks)

    def masks_kernel():
        ng.check(lib.pg_ngram_letter_masks(N, ng._vp(keys), int(t.n), len(t.alphabet), ng._vp(code_bit), ng._vp(again),
                                           ng._stream(dev)), "pg_ngram_letter_masks")

    # the kernel alone, and the public call with its argument checks (two device syncs)
    res = {"N": N, "E": E, "letter_masks_kernel_us": round(timed(masks_kernel, reps), 1),
           "letter_masks_call_us": round(timed(lambda: ng.letter_masks(t), reps), 1)}
    assert torch.equal(again.view(torch.int32), masks.view(torch.int32))
    floor_us = (8 * E + 8 * (N + 1) + 8 * N) / HBM_BYTES_PER_S * 1e6
    res["hop_floor_us"] = round(floor_us, 2)
    targets = torch.from_numpy(np.random.default_rng(0).integers(0, L, size=N).astype(np.uint8)).to(dev)
    labels = torch.empty(N, dtype=torch.int64, device=dev)
    dist = torch.empty(N, L, dtype=torch.uint8, device=dev)
    # the reach words entering each hop, so that every timed launch does that hop's own work
    reach = [masks]
    for h in range(1, K_HOPS + 1):
        nxt = torch.empty_like(masks)
        ng.check(lib.pg_reach_hop_u32(N, ng._vp(rowptr), ng._vp(col), ng._vp(reach[-1]), ng._vp(nxt), h, L, None, L,
                                      None, None, ng._stream(dev)), "pg_reach_hop_u32")
        reach.append(nxt)
    scratch = torch.empty_like(masks)
    for form in ("labels", "dist"):
        hops = []
        for h in range(1, K_HOPS + 1):
            def launch(h=h):
                ng.check(lib.pg_reach_hop_u32(N, ng._vp(rowptr), ng._vp(col), ng._vp(reach[h - 1]), ng._vp(scratch), h,
                                              L, ng._vp(dist) if form == "dist" else None, L,
                                              ng._vp(targets) if form == "labels" else None,
                                              ng._vp(labels) if form == "labels" else None, ng._stream(dev)),
                         "pg_reach_hop_u32")
            us = timed(launch, reps)
            hops.append({"hop": h, "us": round(us, 1), "frac": round(floor_us / us, 3)})
        res[f"hops_{form}"] = hops
    # the public calls end to end (argument checks with their device syncs, CSR build, masks, hop-0 fill, 3 hops)
    # host clock around a call that ends in a device synchronise; one warm-up call, then the median of five
    def wall_ms(fn):
        out = None
        times = []
        for i in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if i:
                times.append((time.perf_counter() - t0) * 1e3)
        return out, round(statistics.median(times), 3)

    (lab, _), res["closest_aa_labels_ms"] = wall_ms(lambda: ng.closest_aa_labels(t, K_HOPS, targets=targets))
    d, res["letter_distances_ms"] = wall_ms(lambda: ng.letter_distances(t, K_HOPS))
    res["label_hist"] = torch.bincount(lab, minlength=K_HOPS + 1).tolist()
    res["labels_equal_distances"] = bool(torch.equal(lab, d.gather(1, targets.long().unsqueeze(1)).squeeze(1).long()))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "closest_aa_probe.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--fasta-seqs", type=int, default=8000)
    ap.add_argument("--skip-grid", action="store_true", help="leave the 5-gram grid out")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("closest_aa_probe.py: no GPU (a time taken elsewhere says nothing)")
    pkg = load_package()
    dev = torch.device("cuda:0")
    out = {"probe": "closest_aa", "device": torch.cuda.get_device_name(0), "k_hops": K_HOPS, "reps": args.reps,
           "hbm_bytes_per_s": HBM_BYTES_PER_S}

    t = pkg.ngram.ngram_transitions(pkg.synth.protein_sequences(args.fasta_seqs, 350, seed=1), 4, device=dev)
    out["fasta4"] = probe_level(pkg, t, args.reps)
    del t
    torch.cuda.empty_cache()

    if not args.skip_grid:
        n = 5
        N, s, d, c = pkg.synth.de_bruijn_edges(n)
        t = pkg.ngram.NgramTransitions(n, N, torch.from_numpy(s).to(dev), torch.from_numpy(d).to(dev),
                                       torch.from_numpy(c).to(dev), torch.arange(N, dtype=torch.int64, device=dev),
                                       pkg.synth.ALPHABET)
        del s, d, c
        out["grid5"] = probe_level(pkg, t, args.reps)
        del t
        torch.cuda.empty_cache()

    import closest_aa_ref as ref
    from golden_util import load
    fx = load("closest_aa")
    strings = [str(x) for x in fx["p1_n3:strings"]]
    t0 = time.perf_counter()
    got, _ = ref.labels(len(strings), fx["p1_n3:src"], fx["p1_n3:dst"], strings, fx["p1_n3:targets"], K_HOPS)
    out["python_bfs_p1_n3"] = {"N": len(strings), "E": int(fx["p1_n3:src"].size),
                               "ms": round((time.perf_counter() - t0) * 1e3, 2),
                               "equal_golden": bool(np.array_equal(got, fx["p1_n3:labels_k3"]))}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
