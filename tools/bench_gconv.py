#!/usr/bin/env python
"""Grouped 3x3 conv kernels on ResNeXt-50 32x4d's bottleneck layers (batch 64):
time of each pass, the activation bandwidth it implies, and the same layer as
a dense conv over zero-expanded weights on the existing core (what the tree
could compute before the grouped kernels). ``--step`` adds the graph step of
``resnet50`` with and without ``cardinality=32``. Needs the GPU.

    python tools/bench_gconv.py [--batch 64] [--iters 30] [--step] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tiresias_amd.ops import _lib  # noqa: E402

BF = torch.bfloat16
# (H = W of the input, C, Cg, stride): the four distinct layers, both strides where they occur
LAYERS = [(56, 128, 4, 1), (56, 256, 8, 2), (28, 256, 8, 1), (28, 512, 16, 2), (14, 512, 16, 1),
          (14, 1024, 32, 2), (7, 1024, 32, 1)]


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def layer(N, H, C, Cg, s, iters, dev):
    T = torch.ops.tam
    torch.manual_seed(0)
    x = torch.randn(N, H, H, C, device=dev).to(BF)
    w = (torch.randn(C, 3, 3, Cg, device=dev) * 0.1).to(BF)
    P = (H - 1) // s + 1
    dy = torch.randn(N, P, P, C, device=dev).to(BF)
    y, dx = torch.empty_like(dy), torch.empty_like(x)
    img = torch.empty(T.gconv_image_elems(C, Cg), dtype=BF, device=dev)
    T.gconv_pack([w], [img])
    dw = torch.zeros(C, 3, 3, Cg, device=dev)
    # the dense stand-in: the same weights zero-expanded to [C,3,3,C]
    wd = torch.zeros(C, 3, 3, C, device=dev, dtype=BF)
    for g in range(C // Cg):
        wd[g * Cg:(g + 1) * Cg, :, :, g * Cg:(g + 1) * Cg] = w[g * Cg:(g + 1) * Cg]
    wt, dwd = torch.empty_like(wd), torch.zeros(C, 3, 3, C, device=dev)
    T.conv_weight_t_batch([wd], [wt])
    act = 2 * (x.numel() + dy.numel())              # bytes every pass must move: one read, one write / two reads
    out = {"layer": f"{H}x{H}x{C} Cg{Cg} s{s}", "act_MB": act / 1e6}
    for name, fn, dense in (
            ("fwd", lambda: T.gconv_fwd(x, w, img, y, s), lambda: T.conv_fwd(x, wd, y, s, 1, 1, None, False)),
            ("dgrad", lambda: T.gconv_dgrad(dy, w, img, dx, s, x),
             lambda: T.conv_dgrad_pre(dy, wd, wt, dx, s, 1, 1, x)),
            ("wgrad", lambda: T.gconv_wgrad(dy, x, dw, s),
             lambda: T.conv_wgrad(dy, x, dwd, s, 1, 1, 1, None, True))):
        us = timed(fn, iters)
        out[name] = {"us": round(us, 1), "GBps": round(act / us / 1e3, 1), "dense_us": round(timed(dense, iters), 1)}
    return out


def step_ms(dev, batch, card, iters):
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer("resnet50", dev, batch=batch, seed=0, use_graph=True, cardinality=card)
    for _ in range(4):
        t.step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        t.step()
    b.record()
    torch.cuda.synchronize()
    return round(a.elapsed_time(b) / iters, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--json")
    a = ap.parse_args()
    _lib.load(required=True)
    dev = torch.device("cuda", 0)
    res = {"batch": a.batch, "layers": [layer(a.batch, *l, a.iters, dev) for l in LAYERS]}
    for r in res["layers"]:
        print(json.dumps(r), flush=True)
    if a.step:
        res["step_ms"] = {"resnet50": step_ms(dev, a.batch, None, a.iters),
                          "resnet50_cardinality32": step_ms(dev, a.batch, 32, a.iters)}
        print(json.dumps(res["step_ms"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
