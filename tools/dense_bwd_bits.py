"""Bit-identity probe of the dense backward (or, with --forward, the dense forward; with --head, the prediction head)
between two builds of the library (a refactor's parent and its branch).

    python tools/dense_bwd_bits.py [--forward | --head] PARENT_LIB BRANCH_LIB [--out FILE] [--dir DIR] [--timeout SECONDS]

For each library one fresh child process (PG_DIRECTGCN_LIB set to it) runs the case list below on the seeded
tests/test_gpu_parity._dense_case inputs, every case with dropout 0 and 0.3, and writes the bytes of every tensor
ops.layer_dense_backward / ops.gemm_at_b returns under DIR/<parent|branch>/. This process then compares the two sets on
the host (it never opens the GPU) and prints one `equal` / `DIFFERS` line per tensor and a count; exit status 0 only
when every tensor is byte-equal. Each child has its own time limit; after a child that exits abnormally nothing more
is started.

--forward: ops.layer_dense and ops.layer_dense_ngram_rows instead (child_forward below): the pipelined split-bf16 kernel
at FWD_X3P_M rows and the 32-row one (F_in 64 with W_res) at FWD_X3_M, both gate modes, constant / identity residual /
pre-gated operand on and off, dropout 0 and 0.3, each under FWD_FLAGS; packed and unpacked weights; the n-gram row map.
Outputs above 64 KiB are dumped as their SHA-256 and length.

--head: ops.head, ops.head_train and ops.head_train_bf16 instead (child_head below) at the shapes and row counts of
HEAD_CASES, HEAD_TRAIN_M and HEAD_TRAIN5_M: logp and emb; loss, dh and the four decoder gradients with dropout 0 and 0.5,
without and with a loss scale. Every kernel of the head is deterministic, so every tensor must be byte-equal.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DROPS = (0.0, 0.3)

# flags by name (protgram_directgcn_amd._lib); bf16: bf16 operands (pg_directgcn_dense_bwd_bf16);
# span: e_res of pg_directgcn_dense_bwd_span_f32; the staged kernels take F_in, F_out % 128 == 0 without `proj`
CASES = [
    # staged fp32 (wgrad_x3_kernel, 16-row steps)
    dict(name="x3_20x128", M=20, Fin=128, Fout=128),                 # 2 splits, the last of 4 rows
    dict(name="x3_1000x128", M=1000, Fin=128, Fout=128),             # 63 splits on 64 workgroups: one idle (tile = -1)
    dict(name="x3_2050x256", M=2050, Fin=256, Fout=256),             # 4 tiles, 43 splits of 48 rows (3 steps), last 34
    dict(name="x3_1500x128to256", M=1500, Fin=128, Fout=256, rows=True),  # pt = 1
    dict(name="x3_span_eres0", M=1000, Fin=128, Fout=128, span=0),
    dict(name="x3_span_eres1", M=1000, Fin=128, Fout=128, span=1),
    # PG_FLAG_WGRAD_F32MFMA: wgrad_kernel at staged shapes
    dict(name="f32mfma_1000x128", M=1000, Fin=128, Fout=128, flags=("PG_FLAG_WGRAD_F32MFMA",)),
    dict(name="f32mfma_3001x128_rows", M=3001, Fin=128, Fout=128, rows=True, flags=("PG_FLAG_WGRAD_F32MFMA",)),
    # tiled fp32 (wgrad_kernel)
    dict(name="tiled_777x64to128_proj_rows", M=777, Fin=64, Fout=128, proj=True, rows=True),
    dict(name="tiled_513x20to12_proj", M=513, Fin=20, Fout=12, proj=True),
    dict(name="tiled_64x128to96_rows", M=64, Fin=128, Fout=96, rows=True),
    # any-shape kernels
    dict(name="any_257x7to5_proj", M=257, Fin=7, Fout=5, proj=True),
    # ops.gemm_at_b (null gates, one segment)
    dict(name="gemm_33x4x8", gemm=(33, 4, 8)),
    dict(name="gemm_1000x128x384", gemm=(1000, 128, 384)),
    dict(name="gemm_70001x256x132", gemm=(70001, 256, 132)),
    # staged bf16 (wgrad_bfs_kernel, 32-row steps)
    dict(name="bfs_1000x128", M=1000, Fin=128, Fout=128, bf16=True),
    dict(name="bfs_2050x256", M=2050, Fin=256, Fout=256, bf16=True),  # 48-row splits: the second step half empty
    dict(name="bfs_5000x256", M=5000, Fin=256, Fout=256, bf16=True),  # three steps
    dict(name="bfs_1000x128to256_proj_rows", M=1000, Fin=128, Fout=256, proj=True, rows=True, bf16=True),  # + col0 launch
    dict(name="bfs_1000x128_dpre32", M=1000, Fin=128, Fout=128, bf16=True, dpre_f32=True),
    dict(name="bfs_1000x128_resident", M=1000, Fin=128, Fout=128, bf16=True, flags=("PG_FLAG_DGRAD_BF16_RESIDENT",)),
    # tiled bf16 (wgrad_bf16_kernel)
    dict(name="bf16tiled_777x64to128_proj_rows", M=777, Fin=64, Fout=128, proj=True, rows=True, bf16=True),
    dict(name="bf16tiled_1000x128_flag", M=1000, Fin=128, Fout=128, bf16=True, flags=("PG_FLAG_WGRAD_BF16_TILED",)),
]


# rows: 1 | one tile | + 1 row | 8 tiles (a grid that is a multiple of 8: XCD-contiguous tile ranges) | 9 tiles (not) |
# 257 tiles on 256 workgroups, the last of 3 rows | 517 tiles; the 32-row kernel: 2 tiles | 8 | 514, the last of 1 row
FWD_X3P_M = (1, 16, 17, 128, 144, 4099, 8272)
FWD_X3_M = (33, 256, 16417)
FWD_FLAGS = (None, "PG_FLAG_DENSE_LDS_EPILOGUE", "PG_FLAG_DENSE_NO_IL", "PG_FLAG_DENSE_A_CACHED", "PG_FLAG_DENSE_TILED")


def child_forward(outdir: str) -> int:
    import ctypes
    import itertools

    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    from __graft_entry__ import load_package
    load_package()
    from protgram_directgcn_amd import _lib, ops
    from test_gpu_parity import _dense_case

    dev = torch.device("cuda:0")
    os.makedirs(outdir, exist_ok=True)
    lib = ops.load_library()

    def save(name, t):
        b = t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()
        if len(b) > 65536:
            b = f"sha256 {hashlib.sha256(b).hexdigest()} of {len(b)} bytes\n".encode()
        with open(os.path.join(outdir, name + ".bin"), "wb") as f:
            f.write(b)

    def gated(Z, prm, Fin):  # s_q * Z_q with fp32 gates: the operand PG_FLAG_DENSE_PREGATED expects
        ca, cd = prm["C_all"], prm["C_directed"]
        s = (ca * cd * prm["C_in"], ca * cd * prm["C_out"], ca * prm["C_undirected"])
        return torch.cat([Z[:, k * Fin:(k + 1) * Fin] * s[k][:Z.size(0)] for k in range(3)], 1)

    for Fin, proj, Ms in ((128, False, FWD_X3P_M), (64, True, FWD_X3_M)):
        for M, vec in itertools.product(Ms, (True, False)):
            Z, xres, prm, const, _, W_res, b_res, _ = _dense_case(M, Fin, 128, proj, vec, False, 7 * M + Fin)
            Zs = {False: Z.to(dev), True: gated(Z, prm, Fin).to(dev)}
            prm = {k: v.to(dev) for k, v in prm.items()}
            xg, cg = xres.to(dev), const.to(dev) if vec else None
            Wr, br = (W_res.to(dev), b_res.to(dev)) if proj else (None, None)
            seed = torch.tensor([0x0123_4567_89AB_CDEF + M], dtype=torch.int64, device=dev)
            for uc, ur, pre, drop in itertools.product((True, False) if vec else (False,), (True,) if proj else (True, False),
                                                       (False, True), DROPS):
                tag = f"fwd_{M}x{Fin}_{'vec' if vec else 'scalar'}_c{int(uc)}r{int(ur)}p{int(pre)}.drop{drop}"
                kw = dict(constant=cg if uc else None, res_x=xg if ur else None, W_res=Wr, b_res=br, act=True,
                          pregated=pre, drop=(drop, seed) if drop else None)
                for f in FWD_FLAGS:
                    fl = ops.default_flags() | (getattr(_lib, f) if f else 0)
                    save(f"{tag}.{f or 'default'}", ops.layer_dense(Zs[pre], prm, 0 if vec else 1, flags=fl, **kw))
                if not proj:  # packed weights (ops.layer_dense hands this kernel the unpacked ones)
                    Y = torch.empty(M, 128, device=dev)
                    a, keep = ops._layer_args(Zs[pre], prm, 0 if vec else 1, None, kw["constant"], kw["res_x"], None, True,
                                              drop=kw["drop"])
                    a.Y, a.ldy = ops._p(Y), Y.stride(0)
                    packed = ops.pack_weights(prm, None, None)
                    fl = ops.default_flags() | (_lib.PG_FLAG_DENSE_PREGATED if pre else 0)
                    ops.check(lib.pg_directgcn_dense_f32(ctypes.byref(a), ops._p(packed), fl, ops._stream(Y)), "dense")
                    torch.cuda.synchronize()
                    del keep
                    save(f"{tag}.packed", Y)
    # n-gram row map: two middles (3 and 4) of a K = 20, Kn1 = 400 grid; residual read / output written at global rows
    M, Kn1, m0 = 800, 400, 3
    Z, xres, prm, const, _, _, _, _ = _dense_case(M, 128, 128, False, True, False, 7 * M + 128)
    prm = {k: v.to(dev) for k, v in prm.items()}
    xglob = torch.randn(20 * Kn1, 128, generator=torch.Generator().manual_seed(M)).to(dev)
    for map_res, map_out in ((True, True), (True, False), (False, True)):
        out = torch.zeros(20 * Kn1, 128, device=dev) if map_out else None
        Y = ops.layer_dense_ngram_rows(Z.to(dev), prm, 0, Kn1, m0, constant=const.to(dev),
                                       res_x=xglob if map_res else xres.to(dev), map_res=map_res, out=out,
                                       map_out=map_out, act=True)
        if Y is None:
            print("fwd_ngram_rows: the entry point does not take this case", file=sys.stderr)
            return 2
        save(f"fwd_ngram_rows_res{int(map_res)}out{int(map_out)}", Y)
    torch.cuda.synchronize()
    return 0


# ops.head: ((F, H, C), bf16 h?, row counts). Model shape (head_x3_kernel, 32-row tiles): a one-row tile, one row short of
# a tile, one tile, one tile and a row; head_kernel (64-row tiles, persistent): 514 tiles on 512 slots and 258 on 256, so
# a block walks a second tile; the last three shapes run the generic kernel
HEAD_CASES = ([((128, 64, C), bf, (1, 31, 32, 33, 1000)) for C in (20, 32, 1) for bf in (False, True)] +
              [((32, 16, 5), False, (1, 63, 65, 32833)), ((64, 32, 5), True, (1, 63, 65, 32833)),
               ((256, 128, 50), False, (65, 16449))] +
              [(shape, False, (1, 5)) for shape in ((16, 8, 400), (34, 17, 3), (12, 6, 1))])
HEAD_TRAIN_M = (1, 63, 64, 65, 16449)   # (128, 64, C in 1, 20, 32): 258 tiles of 64 rows on 256 workgroups
HEAD_TRAIN5_M = (1, 15, 16, 17, 4113)   # (256, 128, 20): 258 tiles of 16 rows
HEAD_DROPS = (0.0, 0.5)


def child_head(outdir: str) -> int:
    import itertools

    sys.path.insert(0, REPO)
    import torch
    from __graft_entry__ import load_package
    load_package()
    from protgram_directgcn_amd import ops

    dev = torch.device("cuda:0")
    os.makedirs(outdir, exist_ok=True)

    def save(name, t):
        b = t.detach().reshape(-1).contiguous().cpu().view(torch.uint8).numpy().tobytes()  # the loss is 0-d
        if len(b) > 65536:
            b = f"sha256 {hashlib.sha256(b).hexdigest()} of {len(b)} bytes\n".encode()
        with open(os.path.join(outdir, name + ".bin"), "wb") as f:
            f.write(b)

    def decoder(g, F, H, C):  # as tests/test_gpu_parity.py's head tests draw it
        return [t.to(dev) for t in (torch.randn(H, F, generator=g) * 0.2, torch.randn(H, generator=g) * 0.1,
                                    torch.randn(C, H, generator=g) * 0.2, torch.randn(C, generator=g) * 0.1)]

    for (F, H, C), bf, Ms in HEAD_CASES:
        for M in Ms:
            g = torch.Generator().manual_seed(F * 1000 + C + M)
            h = torch.randn(M, F, generator=g)
            h[M // 2] = 0.0  # zero row: emb = 0 / (0 + eps)
            h = h.to(dev).to(torch.bfloat16) if bf else h.to(dev)
            lp, emb = ops.head(h, *decoder(g, F, H, C), 1e-12)
            tag = f"head_{F}x{H}x{C}_{'bf16' if bf else 'f32'}_M{M}"
            save(tag + ".logp", lp)
            save(tag + ".emb", emb)
    trains = [(ops.head_train, "head_train", 128, 64, C, HEAD_TRAIN_M, torch.float32) for C in (1, 20, 32)]
    trains.append((ops.head_train_bf16, "head_train_bf16", 256, 128, 20, HEAD_TRAIN5_M, torch.bfloat16))
    for fn, name, F, H, C, Ms, dt in trains:
        for M, drop, scaled in itertools.product(Ms, HEAD_DROPS, (False, True)):
            g = torch.Generator().manual_seed(M + C)
            h = torch.randn(M, F, generator=g).to(dt).to(dev)
            W = decoder(g, F, H, C)
            y = torch.randint(0, C, (M,), generator=g).to(dev)
            seed = torch.tensor([0x1234_5678_9abc_def0 + M], dtype=torch.int64, device=dev)
            r = fn(h, *W, y, 0.75, drop, seed if drop else None, torch.tensor(1024.0, device=dev) if scaled else None)
            if r is None:
                print(f"{name} C={C} M={M}: the entry point does not take this case", file=sys.stderr)
                return 2
            loss, dh, grads = r
            tag = f"{name}_C{C}_M{M}.drop{drop}.scale{int(scaled)}"
            for key, t in zip(("loss", "dh", "dW1", "db1", "dW2", "db2"), (loss, dh) + tuple(grads)):
                save(f"{tag}.{key}", t)
    torch.cuda.synchronize()
    return 0


def child(outdir: str) -> int:
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    from __graft_entry__ import load_package
    load_package()
    from protgram_directgcn_amd import _lib, ops
    from test_gpu_parity import _dense_case

    dev = torch.device("cuda:0")
    os.makedirs(outdir, exist_ok=True)

    def save(case, drop, key, t):
        t = t.detach().contiguous().cpu()
        t.view(torch.uint8).numpy().tofile(os.path.join(outdir, f"{case}.drop{drop}.{key}.bin"))

    for c in CASES:
        if "gemm" in c:  # no dropout in a plain product: once
            M, P, N = c["gemm"]
            g = torch.Generator().manual_seed(M + P + N)
            A, B = torch.randn(M, P, generator=g), torch.randn(M, N, generator=g)
            C, cs = ops.gemm_at_b(A.to(dev), B.to(dev))
            save(c["name"], 0.0, "C", C)
            save(c["name"], 0.0, "colsum", cs)
            continue
        M, Fin, Fout = c["M"], c["Fin"], c["Fout"]
        proj, rows, bf = c.get("proj", False), c.get("rows", False), c.get("bf16", False)
        Z, xres, prm, const, r, W_res, b_res, dY = _dense_case(M, Fin, Fout, proj, True, rows, 7 * M + Fin)
        cast = (lambda t: t.to(dev).to(torch.bfloat16)) if bf else (lambda t: t.to(dev))
        prm = {k: v.to(dev) for k, v in prm.items()}
        Zg, dYg = cast(Z), cast(dY)
        xg = cast(xres) if xres is not None else None
        rg = r.to(dev) if r is not None else None
        Wr, br = (W_res.to(dev), b_res.to(dev)) if proj else (None, None)
        fl = ops.default_flags()
        for f in c.get("flags", ()):
            fl |= getattr(_lib, f)
        for drop in DROPS:
            seed = torch.tensor([0x0123_4567_89AB_CDEF + M], dtype=torch.int64, device=dev)
            packs = [] if bf else None
            Y = ops.layer_dense(Zg, prm, 0, rows=rg, res_x=xg, W_res=Wr, b_res=br, act=True, flags=fl, packs=packs,
                                drop=(drop, seed) if drop else None)
            span = None
            if "span" in c:
                wd = torch.rand(M, 3, generator=torch.Generator().manual_seed(M)).to(dev)
                span = (wd, c["span"])
            out = ops.layer_dense_backward(dYg, Zg, Y, prm, 0, rows=rg, res_x=xg, W_res=Wr, b_res=br, act=True,
                                           flags=fl, packs=packs or None, span=span, drop_p=drop,
                                           dpre_f32=c.get("dpre_f32", False))
            if out is None:
                print(f"{c['name']}: the entry point does not take this case", file=sys.stderr)
                return 2
            for key, t in out.items():
                if t is not None:
                    save(c["name"], drop, key, t)
    torch.cuda.synchronize()
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent_lib")
    ap.add_argument("branch_lib")
    ap.add_argument("--out", help="also write the report to this file")
    ap.add_argument("--dir", default=os.path.join(tempfile.gettempdir(), "dense_bwd_bits"), help="tensor dumps")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--forward", action="store_true", help="the dense forward instead (child_forward)")
    ap.add_argument("--head", action="store_true", help="the prediction head instead (child_head)")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    a = ap.parse_args()
    mode = ["--forward"] if a.forward else ["--head"] if a.head else []
    if a.child:
        return child_forward(a.child) if a.forward else child_head(a.child) if a.head else child(a.child)
    dirs = {}
    for tag, lib in (("parent", a.parent_lib), ("branch", a.branch_lib)):
        dirs[tag] = os.path.join(a.dir, tag)
        shutil.rmtree(dirs[tag], ignore_errors=True)  # no dumps of an earlier run
        env = dict(os.environ, PG_DIRECTGCN_LIB=os.path.abspath(lib))
        env.pop("PG_SPMM_FLAGS", None)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), lib, lib, "--child", dirs[tag]] +
                                mode, env=env, timeout=a.timeout).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"dense_bwd_bits: the {tag} child ({lib}) ended with status {rc}; nothing more started",
                  file=sys.stderr)
            return 1
    names = sorted(set(os.listdir(dirs["parent"])) | set(os.listdir(dirs["branch"])))
    lines, bad = [], 0
    for n in names:
        pa, pb = os.path.join(dirs["parent"], n), os.path.join(dirs["branch"], n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            verdict = "DIFFERS (missing in one build)"
        else:
            with open(pa, "rb") as fa, open(pb, "rb") as fb:
                da, db = fa.read(), fb.read()
            verdict = "equal" if da == db else "DIFFERS"
            verdict += f"  {len(da)} bytes"
        bad += not verdict.startswith("equal")
        lines.append(f"{n[:-4]:60s} {verdict}")
    what = "the forward cases" if a.forward else "the head cases" if a.head else f"{len(CASES)} cases"
    drops = HEAD_DROPS if a.head else DROPS
    lines.append(f"{len(names)} tensors of {what} (dropout {drops[0]} and {drops[1]}): "
                 f"{len(names) - bad} equal, {bad} DIFFERS")
    report = "\n".join(lines)
    print(report)
    if a.out:
        with open(a.out, "w") as f:
            f.write(f"parent {a.parent_lib}\nbranch {a.branch_lib}\n{report}\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
