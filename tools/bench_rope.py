"""What rotary position embeddings inside the attention kernels cost
(profiles/r7/rope.md), one process per call:

  --calls     the attention ops alone at the Transformer's shape ([32, 128, 8,
              64], the short backward) and at a key-blocked shape, three arms in
              alternating windows: no table, the table (fused), and the unfused
              alternative -- a torch rotation of Q and K in front of the plain
              forward, the plain backward followed by a torch rotation of dQ
              and dK; device events around back-to-back launches;
  --steps-ab  graph step time of the Transformer with pos sinusoid / rope,
              alternating windows of two trainers in one process (the knob is
              fixed at construction).
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

BF = torch.bfloat16


def window(t, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def steps_ab(model, steps, warmup, rounds):
    dev = torch.device("cuda", 0)
    arms = {"sinusoid": Trainer(model, dev, use_graph=True), "rope": Trainer(model, dev, use_graph=True, pos="rope")}
    ms = {a: [] for a in arms}
    for t in arms.values():
        window(t, warmup)
    for _ in range(rounds):
        for a, t in arms.items():
            window(t, 3)
            ms[a].append(round(window(t, steps), 4))
    r = dict(model=model, steps=steps, ms=ms, added_us=round((min(ms["rope"]) - min(ms["sinusoid"])) * 1e3, 1))
    print(json.dumps(r), flush=True)
    return r


def torch_rotate(x, table, sign):
    """The unfused pass over the q and k slots at once: [B,S,2,H,64] bf16 ->
    rotated bf16 (sign -1: the transposed rotation)."""
    S = x.shape[1]
    c, s = table[:S, 0][None, :, None, None, :], sign * table[:S, 1][None, :, None, None, :]
    a, b = x[..., :32].float(), x[..., 32:].float()
    return torch.cat([a * c - b * s, b * c + a * s], -1).to(BF)


def calls(reps, rounds):
    dev = torch.device("cuda", 0)
    T = _lib.ops()
    out = []
    for B, H, S, causal in [(32, 8, 128, False), (32, 8, 128, True), (4, 8, 1024, False)]:
        table = Fx.rope_table(S, dev)
        qkv = torch.randn(B, S, 3, H, 64, device=dev).to(BF)
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
        o = torch.empty(B, S, H, 64, device=dev, dtype=BF)
        do = torch.randn_like(o)
        lse = torch.empty(B, H, S, device=dev)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]
        acc, delta = torch.empty(B, S, H, 64, device=dev), torch.empty(B, H, S, device=dev)

        def fwd(qq, kk, **x):
            T.attn_forward(qq, kk, v, o, lse, causal, 0.125, None, **x)

        def bwd(qq, kk, **x):
            T.attn_backward(qq, kk, v, o, do, lse, dq, dk, dv, acc, delta, causal, 0.125, None, **x)

        # the unfused arm keeps the packed layout the kernels read in place: the
        # rotated q and k go into the q / k slots of a second packed tensor
        # (its v slot filled once, outside the timing)
        qkv_r = qkv.clone()
        qr, kr = qkv_r[:, :, 0], qkv_r[:, :, 1]

        def fwd_unfused():
            qkv_r[:, :, :2].copy_(torch_rotate(qkv[:, :, :2], table, 1.0))
            fwd(qr, kr)

        def bwd_unfused():
            # (the rotated q / k are what the forward saved: the plain backward
            # and one rotation of the dq / dk slots are timed)
            bwd(qr, kr)
            dqkv[:, :, :2].copy_(torch_rotate(dqkv[:, :, :2], table, -1.0))

        fwd_unfused()
        arms = {"fwd_off": lambda: fwd(q, k), "fwd_rope": lambda: fwd(q, k, rope=table), "fwd_unfused": fwd_unfused,
                "bwd_off": lambda: bwd(q, k), "bwd_rope": lambda: bwd(q, k, rope=table), "bwd_unfused": bwd_unfused}
        us = {a: [] for a in arms}
        for fn in arms.values():
            for _ in range(5):
                fn()
        for _ in range(rounds):
            for a, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[a].append(round(e0.elapsed_time(e1) / reps * 1e3, 2))
        r = dict(B=B, H=H, S=S, causal=causal, us=us)
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps-ab", action="store_true")
    ap.add_argument("--calls", action="store_true")
    ap.add_argument("--model", default="transformer")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.load(required=True)
    res = {}
    if a.calls:
        res["calls"] = calls(a.reps, a.rounds)
    if a.steps_ab:
        res["steps_ab"] = steps_ab(a.model, a.steps, a.warmup, a.rounds)
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
