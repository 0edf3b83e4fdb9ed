#!/usr/bin/env python3
"""PCA reduction probe: times reduce.py's two kernels and apply_pca on the MI355X at Swiss-Prot size.

Table: P = 570,000 rows of seeded fp32 data with decaying column scales and a common offset, (F, k) = (64, 64) and
(128, 64). Timed per shape, device events around each variant, one warm-up each, then interleaved rounds (every variant
once per round, so drift hits all alike); min / median / max over the rounds are reported:
  moments_kernel     pg_pca_moments_f64 alone (both of its kernels), 10 launches per timing
  project_kernel     pg_pca_project alone, fp16 output, 10 launches per timing
  apply_pca          reduce.apply_pca end to end: moments, the copy to the host, the host eigen-solve, the upload of
                     center and W, the projection
  torch_f64_moments  the baseline for the moments: the same statistics written in torch float64 on the same GPU
                     (convert, mean, variance, standardise, mm), written here, not the code under test
  torch_f64          that plus the host eigh and the float64 mm of the projection, rounded to fp16
  sklearn_cpu        StandardScaler + PCA on the host with the threads the environment allows, if scikit-learn is there
Bytes: the moments kernel reads the table once (P F 4); the projection reads it once and writes P k 2. Rates are those
bytes over the median time, next to the 6.29 TB/s a float4 copy reaches on this chip. No threshold is asserted;
`decision` records whether the f64-MFMA moments kernel is at least as fast as the torch float64 formulation.

Usage:  python tools/pca_probe.py [--rows 570000] [--rounds 7] [--out profiles/pca_probe.json]
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

COPY_TB_S = 6.29  # MI355X_MICROARCH.md: HBM3E, measured float4 copy


def table(P, F, dev):
    g = torch.Generator(device=dev).manual_seed(F)
    x = torch.randn(P, F, generator=g, device=dev)
    q, _ = torch.linalg.qr(torch.randn(F, F, generator=g, device=dev))
    scale = 0.95 ** torch.arange(F, device=dev)
    return ((x * scale) @ q + torch.randn(F, generator=g, device=dev)).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=570000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--shapes", type=int, nargs="+", default=[64, 64, 128, 64], help="F k pairs")
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pca_probe.json"))
    args = ap.parse_args()
    pkg = load_package()
    red = pkg.reduce
    if not torch.cuda.is_available():
        sys.exit("pca_probe.py: no GPU (this probe measures; it has no CPU path)")
    dev = torch.device("cuda:0")
    lib = pkg.load_library()
    vp = lambda x: ctypes.c_void_p(x.data_ptr()) if x is not None else None  # noqa: E731
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)  # noqa: E731
    try:
        from sklearn.decomposition import PCA
        from sklearn.preprocessing import StandardScaler
        have_sklearn = not args.no_sklearn
    except ImportError:
        have_sklearn = False
    P = args.rows
    result = {"device": torch.cuda.get_device_name(0), "P": P, "rounds": args.rounds, "copy_TB_per_s": COPY_TB_S,
              "host_threads": torch.get_num_threads(), "sklearn": have_sklearn, "shapes": {}}

    for F, k in zip(args.shapes[0::2], args.shapes[1::2]):
        x = table(P, F, dev)
        model = red.fit_pca(x, target_dim=k)
        need = int(lib.pg_pca_moments_workspace(P, F))
        work = torch.empty(need, dtype=torch.float64, device=dev)
        mom = torch.empty(F * F + F + 1, dtype=torch.float64, device=dev)
        shift = x[0].contiguous()
        out16 = torch.empty(P, k, dtype=torch.float16, device=dev)

        def moments_kernel():
            rc = lib.pg_pca_moments_f64(vp(x), F, P, F, None, vp(shift), vp(mom), vp(work), need, stream())
            assert rc == 0

        def project_kernel():
            rc = lib.pg_pca_project(vp(x), F, P, F, None, vp(model.center), vp(model.W), k, vp(out16), k, 0, stream())
            assert rc == 0

        def torch_moments():
            xd = x.double()
            mean = xd.mean(0)
            scale = xd.var(0, unbiased=False).sqrt()
            z = (xd - mean) / scale
            return z, z.T @ z / (P - 1)

        def torch_f64():
            z, cov = torch_moments()
            w, v = np.linalg.eigh(cov.cpu().numpy())
            comps = v[:, ::-1].T[:k].copy()
            comps *= np.sign(comps[np.arange(k), np.argmax(np.abs(comps), axis=1)])[:, None]
            return (z @ torch.from_numpy(comps).to(dev).T).half()

        x_host = x.cpu().numpy() if have_sklearn else None

        def sklearn_cpu():
            return PCA(n_components=k, random_state=0).fit_transform(StandardScaler().fit_transform(x_host))

        variants = {
            "moments_kernel": (moments_kernel, 10, P * F * 4),
            "project_kernel": (project_kernel, 10, P * F * 4 + P * k * 2),
            "apply_pca": (lambda: red.apply_pca(x, target_dim=k), 1, 2 * P * F * 4 + P * k * 2),
            "torch_f64_moments": (torch_moments, 1, P * F * 4),
            "torch_f64": (torch_f64, 1, 2 * P * F * 4 + P * k * 2),
        }
        # the same answer all round (fp16 outputs; the baselines add in other orders)
        ours, _ = red.apply_pca(x, target_dim=k)
        base = torch_f64()
        base_diff = float((ours.float() - base.float()).abs().max())
        print(f"F={F} k={k}: max |apply_pca - torch_f64| = {base_diff:.3e} (fp16 outputs of magnitude up to "
              f"{float(base.float().abs().max()):.1f})", flush=True)
        del base
        times = {name: [] for name in variants}
        for fn, _, _ in variants.values():  # warm-up
            fn()
        torch.cuda.synchronize()
        cpu_s = []
        for _ in range(args.rounds):
            for name, (fn, reps, _) in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1) / reps)
            if have_sklearn:
                t0 = time.perf_counter()
                sklearn_cpu()
                cpu_s.append((time.perf_counter() - t0) * 1e3)
        rows = {}
        for name, (_, reps, nbytes) in variants.items():
            ms = times[name]
            med = statistics.median(ms)
            rows[name] = {"ms_min": round(min(ms), 4), "ms_median": round(med, 4), "ms_max": round(max(ms), 4),
                          "launches_per_timing": reps, "bytes": nbytes, "TB_per_s_median": round(nbytes / med / 1e9, 3),
                          "share_of_copy_rate": round(nbytes / med / 1e9 / COPY_TB_S, 3)}
            print(f"F={F:3d} k={k:3d} {name:18s} {min(ms):9.3f} {med:9.3f} {max(ms):9.3f} ms  "
                  f"{nbytes / med / 1e9:6.2f} TB/s", flush=True)
        if cpu_s:
            rows["sklearn_cpu"] = {"ms_min": round(min(cpu_s), 1), "ms_median": round(statistics.median(cpu_s), 1),
                                   "ms_max": round(max(cpu_s), 1)}
            print(f"F={F:3d} k={k:3d} {'sklearn_cpu':18s} {min(cpu_s):9.1f} {statistics.median(cpu_s):9.1f} "
                  f"{max(cpu_s):9.1f} ms", flush=True)
        rows["moments_flop_f64"] = 2 * P * F * F
        rows["workspace_bytes"] = need * 8
        rows["decision"] = {
            "moments_kernel_at_least_as_fast_as_torch_f64_median":
                rows["moments_kernel"]["ms_median"] <= rows["torch_f64_moments"]["ms_median"],
            "ranges_disjoint": rows["moments_kernel"]["ms_max"] < rows["torch_f64_moments"]["ms_min"],
        }
        rows["torch_f64_max_abs_diff_fp16"] = base_diff
        result["shapes"][f"F{F}_k{k}"] = rows
        del x, work, out16, ours
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
