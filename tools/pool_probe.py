#!/usr/bin/env python3
"""Protein-level pooling probe: times pool.py's paths on the MI355X at a user's size.

Level: the builder-produced 4-gram level of ``bench.py --graph fasta`` (ngram.ngram_transitions over
synth.protein_sequences(8000, 350, seed=1), N ~ 169k). Proteins: 100,000 synth.protein_sequences (mean length 350),
once as they are ("even") and once with a few sequences of 20,000-35,000 residues added ("skewed"). F = 64 and 128.

Timed per set and F, device events around each call, one warm-up each, then interleaved rounds (every variant once
per round, so drift hits all alike); min / median / max over the rounds are reported:
  window_ids_table / window_ids_search   pg_ngram_window_ids alone (inputs on the device)
  windows_kernel / bitmap_kernel         pg_pool_rows_f32 alone (launch order precomputed)
  windows / bitmap / sort                the pool.pool_rows paths as pool_proteins runs them after window_ids
                                         (argument checks, the length sort; `sort`: torch.unique of (protein, id))
  torch_windows                          the baseline: a plain torch formulation of the windows mode on the same GPU
                                         (emb[ids] + index_add_ + divide), written here, not the code under test
Gathered bytes = pooled entries * F * 4 over the time. No threshold is asserted; `expectations` records whether the
ranges of the interleaved rounds are disjoint in the expected direction.

Usage:  python tools/pool_probe.py [--proteins 100000] [--rounds 7] [--out profiles/pool_probe.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402


def skewed(seqs, lengths):
    """The same sequences plus a few very long ones (concatenations of the given ones)."""
    long, k = [], 0
    for L in lengths:
        parts, have = [], 0
        while have < L:
            parts.append(seqs[k % len(seqs)])
            have += len(parts[-1])
            k += 1
        long.append("".join(parts)[:L])
    return list(seqs) + long


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--proteins", type=int, default=100000)
    ap.add_argument("--level-seqs", type=int, default=8000)
    ap.add_argument("--n", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--features", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pool_probe.json"))
    args = ap.parse_args()
    pkg = load_package()
    pool = pkg.pool
    t0 = time.time()
    level = pkg.synth.protein_sequences(args.level_seqs, 350, seed=1)
    prots = pkg.synth.protein_sequences(args.proteins, 350, seed=2)
    sets = {"even": prots, "skewed": skewed(prots, [20000, 23000, 26000, 29000, 32000, 35000])}
    print(f"inputs: {time.time() - t0:.1f} s on the host", flush=True)
    if not torch.cuda.is_available():
        sys.exit("pool_probe.py: no GPU (this probe measures; it has no CPU path)")
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    t = pkg.ngram.ngram_transitions(level, args.n, device=dev)
    N, K = t.num_nodes, len(t.alphabet)
    vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    result = {"device": torch.cuda.get_device_name(0), "n": args.n, "N": N, "K": K, "proteins": args.proteins,
              "rounds": args.rounds, "bitmap_cap": pool.distinct_max_nodes(), "sets": {}}

    for set_name, seqs in sets.items():
        ids, off = pool.window_ids(seqs, t)
        P, T = len(seqs), int(ids.numel())
        lens = off[1:] - off[:-1]
        order = torch.argsort(lens, descending=True, stable=True)
        valid = int((ids >= 0).sum())
        ptr_d, ids_d = pool._sorted_distinct_lists(off, ids, N)
        distinct = int(ids_d.numel())
        # window_ids' device inputs
        buf, offsets = pool._encode_raw(seqs)
        b = torch.from_numpy(buf.copy()).to(dev)
        lut = torch.from_numpy(pool.alphabet_lut(t.alphabet)).to(dev)
        table = torch.full((K ** args.n,), -1, dtype=torch.int32, device=dev)
        table[t.node_keys] = torch.arange(N, dtype=torch.int32, device=dev)
        ids_out = torch.empty_like(ids)
        which = torch.repeat_interleave(torch.arange(P, device=dev), lens)
        entry = {"P": P, "windows_total": T, "windows_valid": valid, "distinct_entries": distinct,
                 "longest": int(lens.max()), "F": {}}

        def wid(tab):
            rc = lib.pg_ngram_window_ids(P, vp(off), vp(b), vp(lut), args.n, K, vp(t.node_keys), N, vp(tab),
                                         vp(ids_out), stream())
            assert rc == 0

        for F in args.features:
            emb = torch.randn(N, F, generator=torch.Generator().manual_seed(F)).to(dev)
            out = torch.empty(P, F, device=dev)
            cnt = torch.empty(P, dtype=torch.int32, device=dev)

            def kernel(distinct_flag):
                rc = lib.pg_pool_rows_f32(vp(emb), F, N, F, vp(off), vp(ids), vp(order), P, distinct_flag, vp(out), F,
                                          vp(cnt), 0, stream())
                assert rc == 0

            def torch_windows():
                ok = ids >= 0
                w = which[ok]
                s = torch.zeros(P, F, device=dev).index_add_(0, w, emb[ids[ok].long()])
                c = torch.bincount(w, minlength=P)
                return s / c.clamp(min=1).unsqueeze(1), c

            def sort_path():
                p2, i2 = pool._sorted_distinct_lists(off, ids, N)
                return pool.pool_rows(emb, p2, i2)

            variants = {
                "window_ids_table": (lambda: wid(table), T * 4),
                "window_ids_search": (lambda: wid(None), T * 4),
                "windows_kernel": (lambda: kernel(0), valid * F * 4),
                "bitmap_kernel": (lambda: kernel(1), distinct * F * 4),
                "windows": (lambda: pool.pool_rows(emb, off, ids), valid * F * 4),
                "bitmap": (lambda: pool.pool_rows(emb, off, ids, distinct=True), distinct * F * 4),
                "sort": (sort_path, distinct * F * 4),
                "torch_windows": (torch_windows, valid * F * 4),
            }
            # the paths agree (bits for ours; the torch baseline adds in another order)
            a, ca = pool.pool_rows(emb, off, ids, distinct=True)
            s, cs = sort_path()
            assert torch.equal(a.view(torch.int32), s.view(torch.int32)) and torch.equal(ca, cs)
            w, cw = pool.pool_rows(emb, off, ids)
            tw, tc = torch_windows()
            base_diff = float((w - tw).abs().max())
            assert torch.equal(cw.long(), tc) and base_diff < 1e-4, base_diff
            del a, s, w, tw
            times = {k: [] for k in variants}
            for fn, _ in variants.values():  # warm-up
                fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for name, (fn, _) in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1))
            rows = {}
            for name, (_, nbytes) in variants.items():
                ms = times[name]
                med = statistics.median(ms)
                rows[name] = {"ms_min": round(min(ms), 4), "ms_median": round(med, 4), "ms_max": round(max(ms), 4),
                              "bytes": nbytes, "GB_per_s_median": round(nbytes / med / 1e6, 1)}
                print(f"{set_name:7s} F={F:3d} {name:18s} {min(ms):9.3f} {med:9.3f} {max(ms):9.3f} ms  "
                      f"{nbytes / med / 1e6:9.1f} GB/s", flush=True)
            rows["expectations"] = {
                "windows_beats_torch_disjoint": rows["windows"]["ms_max"] < rows["torch_windows"]["ms_min"],
                "bitmap_beats_sort_disjoint": rows["bitmap"]["ms_max"] < rows["sort"]["ms_min"],
            }
            rows["torch_windows_max_abs_diff"] = base_diff
            entry["F"][str(F)] = rows
            del emb, out, cnt
        result["sets"][set_name] = entry
        del ids, off, which, table, b
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
