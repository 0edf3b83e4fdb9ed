#!/usr/bin/env python3
"""A/B timing of the dense layer kernels in the in-tree library on the bench's layer-1 shape (B(20,n), F = 128,
vector gates, constant, identity residual): the default (dense_x3p_kernel: register epilogue, interleaved LDS-DMA issue)
against PG_FLAG_DENSE_LDS_EPILOGUE (the earlier epilogue through LDS), PG_FLAG_DENSE_NO_IL (all pieces at the top of the
iteration) and, with --ref-lib PATH, the default of another build of the library (same C ABI, e.g. the parent
commit's), interleaved rounds (min and median per launch, HIP events; every variant through the same direct
pg_directgcn_dense_f32 call), and a bit-equality check.
--fin64: the same rows at F_in = 64 with a projected residual (W_res; random parameters, packed weights) instead, the
shape of dense_x3_kernel: its default only, against --ref-lib's.
usage: python tools/dense_ab.py [n=4] [rounds=20] [reps=20] [--ref-lib=PATH] [--fin64]"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

pkg = load_package()
from protgram_directgcn_amd import ops  # noqa: E402
import ctypes  # noqa: E402

from protgram_directgcn_amd import _lib  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
fin64 = "--fin64" in sys.argv[1:]
ref_lib = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--ref-lib=")), None)
n = int(args[0]) if args else 4
rounds = int(args[1]) if len(args) > 1 else 20
reps = int(args[2]) if len(args) > 2 else 20
dev = torch.device("cuda:0")
N, s, d, c = pkg.synth.de_bruijn_edges(n)
g = pkg.build_propagation_csr(N, s, d, c, device=dev)
import bench  # noqa: E402

model = bench.bench_model(pkg, N, 128, 2, n).to(dev).eval()
layer = model.convs[0]
x = torch.randn(N, 128, generator=torch.Generator().manual_seed(1234)).to(dev)
prm = dict(zip(ops._DENSE_KEYS, (p.detach() for p in layer._dense_params())))
Z = ops.spmm3(g, x)
Y = torch.empty(N, 128, device=dev)
packed = None
if fin64:
    gen = torch.Generator().manual_seed(64)
    x = torch.randn(N, 64, generator=gen).to(dev)
    Z = torch.randn(N, 192, generator=gen).to(dev)
    prm = {k: (torch.randn(*v.shape[:-1], 64, generator=gen) * 0.1).to(dev) if k.startswith("W_") else v
           for k, v in prm.items()}
    W_res = (torch.randn(128, 64, generator=gen) * 0.1).to(dev)
    packed = ops.pack_weights(prm, W_res, torch.zeros(128, device=dev))
    a, keep = ops._layer_args(Z, prm, 0, None, layer.constant.detach(), x, W_res, True, ops.LEAKY_SLOPE)
else:
    a, keep = ops._layer_args(Z, prm, 0, None, layer.constant.detach(), x, None, True, ops.LEAKY_SLOPE)
a.Y, a.ldy = ops._p(Y), Y.stride(0)
raw = [ops._f32c(prm[k].detach()) for k in ops._PACK_KEYS]
(a.W_main_in, a.W_main_out, a.W_undirected, a.W_shared, a.b_main_in, a.b_dir_shared_in, a.b_main_out,
 a.b_dir_shared_out, a.b_undirected, a.b_undirected_shared) = [ops._p(t) for t in raw]
st = ops._stream(Z)


def entry(lib):
    fn = lib.pg_directgcn_dense_f32
    fn.restype, fn.argtypes = _lib.SIGNATURES["pg_directgcn_dense_f32"]
    return fn


own = entry(ctypes.CDLL(pkg.library_path()))
base = ops.default_flags()
variants = {"x3p_reg_epilogue": (own, base), "x3p_lds_epilogue": (own, base | _lib.PG_FLAG_DENSE_LDS_EPILOGUE),
            "x3p_reg_epilogue_no_il": (own, base | _lib.PG_FLAG_DENSE_NO_IL)}
if fin64:
    variants = {"x3_default": (own, base)}
if ref_lib:
    variants["ref_lib_default"] = (entry(ctypes.CDLL(os.path.abspath(ref_lib))), base)


def run(v):
    fn, fl = v
    rc = fn(ctypes.byref(a), ops._p(packed) if fin64 else None, fl, st)
    assert rc == 0, rc
    return Y


with torch.no_grad():
    outs = {k: run(v).clone() for k, v in variants.items()}
    same = all(torch.equal(next(iter(outs.values())), v) for v in outs.values())
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, v in variants.items():
            for _ in range(3):
                run(v)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run(v)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / reps * 1e3)
res = {k: {"min_us": round(min(v), 2), "median_us": round(sorted(v)[len(v) // 2], 2)} for k, v in times.items()}
res["bit_identical"] = same
res["shape"] = (f"B(20,{n}) M={N} F_in=64 F_out=128, vector gates, constant, projected residual" if fin64 else
                f"B(20,{n}) M={N} F=128, vector gates, constant, identity residual") + " (direct C-ABI calls)"
print(json.dumps(res))
