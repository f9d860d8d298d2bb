"""What global-norm gradient clipping adds to a graph step: one trainer per
model, the same captured graph, alternating windows of steps with clipping
off and on (``Trainer.set_grad_clip``) in one process, so both arms share
the box, the allocator state and the clocks (profiles/r7/grad_clip.md)."""
from __future__ import annotations

import argparse
import json
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from tiresias_amd.executor.trainer import Trainer  # noqa: E402


def window(t, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="gnmt,transformer")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grad-clip", type=float, default=5.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = []
    for m in a.models.split(","):
        t = Trainer(m, torch.device("cuda", 0), use_graph=True)
        for clip in (a.grad_clip, None):          # both arms warm (buffers, code objects)
            t.set_grad_clip(clip)
            window(t, a.warmup)
        off, on = [], []
        for _ in range(a.rounds):
            t.set_grad_clip(None)
            off.append(round(window(t, a.steps), 4))
            t.set_grad_clip(a.grad_clip)
            on.append(round(window(t, a.steps), 4))
        r = dict(model=m, params=t.arena.numel, steps=a.steps, grad_clip=a.grad_clip, off_ms=off, on_ms=on,
                 delta_us=round((min(on) - min(off)) * 1e3, 1), stats=t.clip_stats())
        print(json.dumps(r), flush=True)
        res.append(r)
        t.release()
        del t
        torch.cuda.empty_cache()
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
