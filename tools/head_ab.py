#!/usr/bin/env python3
"""A/B timing of the prediction head's three entry points between two builds of the library (same C ABI, e.g. the
parent commit's and this tree's; two builds of one commit give the noise of the method): interleaved rounds, HIP
events, min and median per launch, every call a direct C-ABI call on the same buffers, and a bit-equality check.
  head            pg_directgcn_head_f32 at the bench's shape (B(20,4): M = 160000, 128 -> 64 -> 20; bench.py's head_ms)
  head_train      pg_head_train_f32, M = 160000, (128, 64, 20), dropout 0.5
  head_train_bf16 pg_head_train_bf16, M = 160000, (256, 128, 20), dropout 0.5
usage: python tools/head_ab.py A_LIB B_LIB [rounds=20] [reps=20]"""
import ctypes
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402

from __graft_entry__ import load_package  # noqa: E402

load_package()
from protgram_directgcn_amd import _lib, ops  # noqa: E402

libs = {"A": os.path.abspath(sys.argv[1]), "B": os.path.abspath(sys.argv[2])}
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 20
reps = int(sys.argv[4]) if len(sys.argv) > 4 else 20
dev = torch.device("cuda:0")
M, C = 160000, 20
gen = torch.Generator().manual_seed(1234)


def rnd(*shape, s=1.0):
    return (torch.randn(*shape, generator=gen) * s).to(dev)


def entry(lib, name):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return fn


def head_call(lib):
    F, H = 128, 64
    h, W1, b1, W2, b2 = rnd(M, F), rnd(H, F, s=0.2), rnd(H, s=0.1), rnd(C, H, s=0.2), rnd(C, s=0.1)
    logp, emb = torch.empty(M, C, device=dev), torch.empty(M, F, device=dev)
    fn, st = entry(lib, "pg_directgcn_head_f32"), ops._stream(h)

    def run():
        rc = fn(M, F, H, C, ops._p(h), h.stride(0), ops._p(W1), ops._p(b1), ops._p(W2), ops._p(b2), 1e-12, ops._p(logp),
                logp.stride(0), ops._p(emb), emb.stride(0), st)
        assert rc == 0, rc
        return logp, emb
    return run


def train_call(lib, bf16):
    F, H = (256, 128) if bf16 else (128, 64)
    name = "pg_head_train_bf16" if bf16 else "pg_head_train_f32"
    h = rnd(M, F).to(torch.bfloat16 if bf16 else torch.float32)
    W1, b1, W2, b2 = rnd(H, F, s=0.1), rnd(H, s=0.1), rnd(C, H, s=0.2), rnd(C, s=0.1)
    y = torch.randint(0, C, (M,), generator=gen).to(dev)
    seed = torch.tensor([0x1234_5678_9abc_def0], dtype=torch.int64, device=dev)
    dh = torch.empty_like(h)
    grads = torch.empty(H * F + H + C * H + C, device=dev)
    loss = torch.empty((), device=dev)
    nwork = int(entry(lib, name.replace("_f32", "") + "_workspace")(M, F, H, C))
    work = torch.empty(nwork, device=dev)
    fn, st = entry(lib, name), ops._stream(h)

    def run():
        rc = fn(M, F, H, C, ops._p(h), h.stride(0), ops._p(W1), ops._p(b1), ops._p(W2), ops._p(b2), ops._p(y), 0.75 / M,
                0.5, ops._p(seed), None, ops._p(dh), dh.stride(0), ops._p(grads), ops._p(loss), ops._p(work),
                work.numel(), st)
        assert rc == 0, rc
        return dh, grads, loss
    return run


CALLS = {"head": head_call, "head_train": lambda lib: train_call(lib, False),
         "head_train_bf16": lambda lib: train_call(lib, True)}
handles = {k: ctypes.CDLL(v) for k, v in libs.items()}
res = {"libs": libs, "shape": f"M={M} C={C}; head, head_train: 128 -> 64; head_train_bf16: 256 -> 128; dropout 0.5",
       "rounds": rounds, "reps": reps}
with torch.no_grad():
    for what, make in CALLS.items():
        runs = {}
        for k in libs:
            gen.manual_seed(1234)  # the same draws for both libraries
            runs[k] = make(handles[k])
        outs = {k: [t.clone() for t in run()] for k, run in runs.items()}
        torch.cuda.synchronize()
        same = all(torch.equal(a, b) for a, b in zip(outs["A"], outs["B"]))
        times = {k: [] for k in runs}
        for _ in range(rounds):
            for k, run in runs.items():
                for _ in range(3):
                    run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    run()
                e1.record()
                torch.cuda.synchronize()
                times[k].append(e0.elapsed_time(e1) / reps * 1e3)
        res[what] = {k: {"min_us": round(min(v), 2), "median_us": round(sorted(v)[len(v) // 2], 2)}
                     for k, v in times.items()}
        res[what]["bit_identical"] = same
        del runs, outs
print(json.dumps(res))
