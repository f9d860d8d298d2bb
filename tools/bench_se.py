"""Squeeze-and-Excitation kernels on ResNet-50's four bottleneck output shapes
(bs 64 default, ratio 16): the time of each of the six kernels, the two
reductions on each route (tiled / single pass), with the bytes each pass must
move (computed from the shapes) over its time, then (--step) the ResNet-50
hipGraph step with se_ratio=16 against the plain model, interleaved.
HIP-event timing.

    python tools/bench_se.py [--batch 64] [--ratio 16] [--reps 20] [--step 30] [--out file.json]
"""
from __future__ import annotations

import argparse
import json
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])

# (H = W, C, blocks) of the bottleneck outputs of stages 1-4
STAGES = [(56, 256, 3), (28, 512, 4), (14, 1024, 6), (7, 2048, 3)]


def step_ms(t, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        t.step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--ratio", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", type=int, default=0, help="also time the ResNet-50 graph step, this many steps x 3 rounds")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from tiresias_amd.ops import _lib

    _lib.load(required=True)
    T = torch.ops.tam
    dev = torch.device("cuda", 0)
    BF = torch.bfloat16
    N = a.batch

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.reps * 1e3      # us

    rows = []
    for H, C, blocks in STAGES:
        P, Cr = H * H, max(8, C // a.ratio)
        torch.manual_seed(0)
        u, idn, dy, add = (torch.randn(N, P, C, device=dev).to(BF) for _ in range(4))
        y, g, du = torch.empty_like(u), torch.empty_like(u), torch.empty_like(u)
        w1 = (torch.randn(Cr, C, device=dev) / C ** 0.5).to(BF)
        w2 = (torch.randn(C, Cr, device=dev) / Cr ** 0.5).to(BF)
        b1, b2 = torch.zeros(Cr, device=dev, dtype=BF), torch.zeros(C, device=dev, dtype=BF)
        z, s, ds, dz = (torch.empty(N, C, device=dev) for _ in range(4))
        h = torch.empty(N, Cr, device=dev)
        dw1, db1, dw2, db2 = (torch.zeros(sh, device=dev) for sh in ((Cr, C), (Cr,), (C, Cr), (C,)))
        act = 2 * N * P * C                               # bytes of one activation tensor
        fc = 2 * 2 * C * Cr + 4 * N * (2 * C + Cr)        # both weights, z / s / h
        row = dict(P=P, C=C, Cr=Cr, blocks=blocks, act_MB=round(act / 1e6, 2))

        def put(tag, us, nbytes):
            row[tag + "_us"] = round(us, 2)
            row[tag + "_tbs"] = round(nbytes / us / 1e6, 3)

        ref = {}
        for route, rn in ((1, "tiled"), (2, "single")):
            T.se_policy(route)
            put("squeeze_" + rn, timed(lambda: T.se_squeeze(u, z)), act)
            put("bwd_reduce_" + rn, timed(lambda: T.se_gate_bwd_reduce(dy, add, u, u, g, ds)), 5 * act)
            # the routes must agree (a launch that did not run would also show here)
            for k, v in (("z", z), ("ds", ds)):
                if route == 1:
                    ref[k] = v.clone()
                else:
                    row[k + "_single_vs_tiled"] = float((v - ref[k]).norm() / ref[k].norm())
        T.se_policy(0)
        put("excite_fwd", timed(lambda: T.se_excite_fwd(z, w1, b1, w2, b2, h, s)), fc)
        put("gate_fwd", timed(lambda: T.se_gate_fwd(u, s, idn, y)), 3 * act)
        put("excite_bwd", timed(lambda: T.se_excite_bwd(ds, s, h, z, w1, w2, dw1, db1, dw2, db2, dz)),
            fc + 2 * 4 * 2 * C * Cr + 4 * N * (2 * C + Cr))
        put("gate_bwd_apply", timed(lambda: T.se_gate_bwd_apply(g, s, dz, du)), 2 * act)
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"batch": N, "ratio": a.ratio, "rows": rows}
    if a.step:
        from tiresias_amd.executor.trainer import Trainer

        ts = {str(r): Trainer("resnet50", dev, batch=N, use_graph=True, se_ratio=r) for r in (None, a.ratio)}
        for t in ts.values():
            for _ in range(5):
                t.step()
        torch.cuda.synchronize()
        ms = {n: [] for n in ts}
        for _ in range(3):                      # interleaved rounds: the spread is in the list
            for n, t in ts.items():
                ms[n].append(round(step_ms(t, a.step), 3))
        out["step_ms"] = ms
        print(json.dumps({"step_ms": ms}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
