"""GroupNorm kernels on ResNet-50's layer shapes (bs 64 default, 32 groups):
per distinct shape the forward and backward time on each route (tiled /
resident where its tile fits) with the achieved bytes/s against the byte
model of profiles/r7/groupnorm.md, then (--step) the ResNet-50 hipGraph step
with norm=group against norm=batch, interleaved. HIP-event timing.

    python tools/bench_gn.py [--batch 64] [--reps 20] [--step 30] [--out file.json]
"""
from __future__ import annotations

import argparse
import json
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])

from tools.bench_bn import resnet50_bn_shapes  # noqa: E402

# bytes per element: (tiled, resident), + 2 with a residual
FWD_MODEL, BWD_MODEL = (6, 4), (14, 8)


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

    rows, seen = [], set()
    for name, M, C, kind in resnet50_bn_shapes(N):
        P, res = M // N, kind == "res"
        if (P, C, res) in seen:
            continue
        seen.add((P, C, res))
        G = C // max(2, C // 32)
        x = (torch.randn(N, P, C, device=dev) + 1).to(BF)
        r = torch.randn(N, P, C, device=dev).to(BF) if res else None
        dy = torch.randn(N, P, C, device=dev).to(BF)
        y, dx = torch.empty_like(x), torch.empty_like(x)
        dres = torch.empty_like(x) if res else None
        g, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        mean, rstd = torch.empty(N * G, device=dev), torch.empty(N * G, device=dev)
        dg, db = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
        cpart = torch.empty(N * ((P + 255) // 256) * 2 * C, device=dev)
        relu = kind != "plain"
        row = dict(name=name, P=P, C=C, G=G, kind=kind)
        ref = {}
        el = N * P * C
        for route, rn in ((1, "tiled"), (2, "resident")):
            T.gn_policy(route)
            for bwd in (False, True):
                tag = ("bwd_" if bwd else "fwd_") + rn
                if route == 2 and not T.gn_resident_fits(P, C, G, bwd):
                    row[tag + "_us"] = None
                    continue
                if bwd:
                    us = timed(lambda: T.groupnorm_backward(dy, y if relu else None, x, mean, rstd, g, dx, dres, cpart,
                                                            dg, db, G, relu, r))
                else:
                    us = timed(lambda: T.groupnorm_forward(x, r, y, g, b, mean, rstd, G, 1e-5, relu))
                per = (BWD_MODEL if bwd else FWD_MODEL)[route - 1] + (2 if res else 0)
                row[tag + "_us"] = round(us, 2)
                # the routes must agree (a launch that did not run would also show here)
                cur = (dx if bwd else y).float()
                if route == 1:
                    ref[bwd] = cur.clone()
                else:
                    row[tag + "_vs_tiled"] = float((cur - ref[bwd]).norm() / ref[bwd].norm())
                row[tag + "_tbs"] = round(el * per / us / 1e6, 2)      # byte model over time, TB/s
        T.gn_policy(0)
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"rows": rows}
    if a.step:
        from tiresias_amd.executor.trainer import Trainer

        ts = {n: Trainer("resnet50", dev, batch=N, use_graph=True, norm=n) for n in ("batch", "group")}
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
