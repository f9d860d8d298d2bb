"""What attention-probability dropout costs (profiles/r7/attn_dropout.md), one
process per call:

  --steps-ab  graph step time of the Transformer with the recipe's four arms
              (off / attn_dropout / dropout / both), alternating windows on ONE
              trainer (same box, same clocks; a change of either knob
              re-captures the graph outside the timed windows);
  --calls     the attention ops alone at the Transformer's shape ([32, 128, 8,
              64], the short backward) and at a key-blocked shape, with and
              without the record: device events around back-to-back launches;
  --run       plain steps of one arm (for a kernel trace of that arm).
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

ARMS = {"off": (None, None), "attn": (None, 0.1), "drop": (0.1, None), "both": (0.1, 0.1)}


def window(t, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def steps_ab(model, steps, warmup, rounds):
    t = Trainer(model, torch.device("cuda", 0), use_graph=True)
    window(t, warmup)
    ms = {a: [] for a in ARMS}
    for _ in range(rounds):
        for arm, (p, pa) in ARMS.items():
            t.set_dropout(p)
            t.set_attn_dropout(pa)
            window(t, 3)                               # re-capture outside the timed window
            ms[arm].append(round(window(t, steps), 4))
    r = dict(model=model, steps=steps, ms=ms,
             added_us={a: round((min(ms[a]) - min(ms["off"])) * 1e3, 1) for a in ARMS if a != "off"})
    print(json.dumps(r), flush=True)
    return r


def calls(reps):
    dev = torch.device("cuda", 0)
    T = _lib.ops()
    rec = torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=dev)
    thr = Fx.attn_dropout_threshold(0.1)
    extra = (rec, 0, thr, Fx.attn_dropout_scale(thr))
    out = []
    for B, H, S, causal in [(32, 8, 128, False), (32, 8, 128, True), (4, 8, 1024, False)]:
        qkv = torch.randn(B, S, 3, H, 64, device=dev).to(torch.bfloat16)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        o = torch.empty(B, S, H, 64, device=dev, dtype=torch.bfloat16)
        do = torch.randn_like(o)
        lse = torch.empty(B, H, S, device=dev)
        dqkv = torch.empty_like(qkv)
        acc, delta = torch.empty(B, S, H, 64, device=dev), torch.empty(B, H, S, device=dev)

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
                best.append(round(e0.elapsed_time(e1) / reps * 1e3, 2))
            return best

        def fwd(*x):
            T.attn_forward(q, k, v, o, lse, causal, 0.125, None, *x)

        def bwd(*x):
            T.attn_backward(q, k, v, o, do, lse, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2], acc, delta,
                            causal, 0.125, None, *x)

        r = dict(B=B, H=H, S=S, causal=causal, fwd_us=timed(fwd), fwd_drop_us=timed(lambda: fwd(*extra)),
                 bwd_us=timed(bwd), bwd_drop_us=timed(lambda: bwd(*extra)))
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps-ab", action="store_true")
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--run", choices=sorted(ARMS), default=None)
    ap.add_argument("--model", default="transformer")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.load(required=True)
    res = {}
    if a.steps_ab:
        res["steps_ab"] = steps_ab(a.model, a.steps, a.warmup, a.rounds)
    if a.calls:
        res["calls"] = calls(a.reps)
    if a.run:
        p, pa = ARMS[a.run]
        t = Trainer(a.model, torch.device("cuda", 0), dropout=p, attn_dropout=pa)
        res["run"] = dict(arm=a.run, steps=a.steps, ms=round(window(t, a.steps), 4))
        print(json.dumps(res["run"]), flush=True)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
