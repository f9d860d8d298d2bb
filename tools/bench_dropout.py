"""What training dropout costs (profiles/r7/dropout.md), one process per call:

  --kernel   the standalone kernel's bandwidth at 2^20 and 2^26 elements
             against a 16-B-per-lane bf16 copy of the same size (torch's
             copy_), device events around back-to-back launches;
  --steps-ab graph step time of each model with dropout off / on, alternating
             windows on ONE trainer (same box, same clocks; a change of p
             re-captures the graph outside the timed windows);
  --fused-ab Transformer only: the fused add + LayerNorm dropout against the
             same sites through the standalone kernel (dropout(r) followed by
             the plain fused add + LayerNorm), alternating windows.
"""
from __future__ import annotations

import argparse
import json
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from tiresias_amd.executor.trainer import Trainer  # noqa: E402
from tiresias_amd.ops import _lib  # noqa: E402
from tiresias_amd.ops import functional as Fx  # noqa: E402

RECIPE = {"transformer": 0.1, "vgg16": 0.5, "gnmt": 0.2, "resnet50": None}


def window(t, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def kernel_bw(reps):
    dev = torch.device("cuda", 0)
    T = _lib.ops()
    rec = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=dev)
    out = []
    for n in (1 << 20, 1 << 26):
        x = torch.randn(n, device=dev).to(torch.bfloat16)
        y = torch.empty_like(x)
        thr = 6554
        sc = Fx.dropout_scale(thr)

        def timed(fn):
            for _ in range(5):
                fn()
            best = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                best.append(e0.elapsed_time(e1) / reps * 1e3)
            return best

        d = timed(lambda: T.dropout_apply(x, y, rec, 0, thr, sc))
        c = timed(lambda: y.copy_(x))
        r = dict(n=n, bytes=4 * n, dropout_us=[round(v, 2) for v in d], copy_us=[round(v, 2) for v in c],
                 dropout_tbps=round(4 * n / min(d) / 1e6, 3), copy_tbps=round(4 * n / min(c) / 1e6, 3))
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def steps_ab(models, steps, warmup, rounds):
    out = []
    for m in models:
        p = RECIPE.get(m)
        t = Trainer(m, torch.device("cuda", 0), use_graph=True)
        window(t, warmup)
        off, on = [], []
        for _ in range(rounds):
            t.set_dropout(None)
            window(t, 3)                           # re-capture outside the timed window
            off.append(round(window(t, steps), 4))
            if p:
                t.set_dropout(p)
                window(t, 3)
                on.append(round(window(t, steps), 4))
        r = dict(model=m, dropout=p, steps=steps, off_ms=off, on_ms=on,
                 added_us=round((min(on) - min(off)) * 1e3, 1) if on else None)
        print(json.dumps(r), flush=True)
        out.append(r)
        t.release()
        del t
        torch.cuda.empty_cache()
    return out


def fused_ab(steps, warmup, rounds):
    """Transformer 0.1: the fused sites against the same sites through the
    standalone kernel. The unfused arm replaces Fx.add_layernorm_skip for
    the capture of its graph only; both graphs then replay alternately."""
    fused = Trainer("transformer", torch.device("cuda", 0), use_graph=True, dropout=0.1)
    window(fused, warmup)
    real = Fx.add_layernorm_skip

    def unfused(x, r, g, b, eps=1e-5, drop=None):
        return real(x, Fx.dropout(r, drop), g, b, eps)

    alone = Trainer("transformer", torch.device("cuda", 0), use_graph=True, dropout=0.1)
    Fx.add_layernorm_skip = unfused
    try:
        window(alone, warmup)                      # warm steps + capture with the standalone sites
    finally:
        Fx.add_layernorm_skip = real
    a, b = [], []
    for _ in range(rounds):
        a.append(round(window(fused, steps), 4))
        b.append(round(window(alone, steps), 4))
    r = dict(model="transformer", dropout=0.1, steps=steps, fused_ms=a, standalone_ms=b,
             fused_minus_standalone_us=round((min(a) - min(b)) * 1e3, 1))
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--steps-ab", action="store_true")
    ap.add_argument("--fused-ab", action="store_true")
    ap.add_argument("--models", default="resnet50,vgg16,transformer,gnmt")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.load(required=True)
    res = {}
    if a.kernel:
        res["kernel"] = kernel_bw(a.reps)
    if a.steps_ab:
        res["steps_ab"] = steps_ab(a.models.split(","), a.steps, a.warmup, a.rounds)
    if a.fused_ab:
        res["fused_ab"] = fused_ab(a.steps, a.warmup, a.rounds)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
