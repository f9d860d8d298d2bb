"""Per-shape timing of ResNet-50's pointwise (1x1 / stride-1) convs that the
gemm8p route accepts: the conv core (with whatever split + reduce it picks)
against every gemm8p tile, forward (+ BN statistics) and dgrad (+ ReLU mask).

The shapes are the ones an eager ResNet-50 step at the default batch tunes
(``torch.ops.tam.gemm_routes()``, layout ``PW``). HIP events outside graph
capture, warm-up then ``--iters`` back-to-back launches, best of two rounds.

  python tools/bench_pw_route.py [--out table.md] [--routes routes.txt]
"""
from __future__ import annotations

import argparse
import math
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from tiresias_amd.executor.trainer import Trainer  # noqa: E402
from tiresias_amd.ops import _lib  # noqa: E402
from tiresias_amd.ops.functional import BN_SHARDS  # noqa: E402

BF = torch.bfloat16
KINDS = {0: "plain", 1: "relu", 2: "stats", 3: "stats+relu", 4: "mask"}


def time_us(fn, iters):
    for _ in range(3):
        fn()
    best = 1e30
    for _ in range(2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / iters)
    return best


def pw_lines():
    return [ln.split() for ln in torch.ops.tam.gemm_routes().splitlines() if " PW " in ln]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="resnet50")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--routes", default=None, help="write the tuned PW route lines here")
    a = ap.parse_args()
    _lib.load(required=True)
    T = torch.ops.tam
    dev = torch.device("cuda", 0)
    t = Trainer(a.model, dev, use_graph=False)
    for _ in range(2):
        t.step()
    torch.cuda.synchronize()
    batch = t.batch
    del t
    lines = pw_lines()
    if a.routes:
        open(a.routes, "w").write("".join(" ".join(ln) + "\n" for ln in lines))
    out = ["| M | N | K | epilogue | conv core | 64 | 65 | 128 | 129 | 256 | best | routed (in-op) |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for ln in lines:
        M, N, K, kind = int(ln[0]), int(ln[1]), int(ln[2]), int(ln[4])
        hw = math.isqrt(M // batch) if M % batch == 0 else 0
        n, h, w_ = (batch, hw, hw) if hw and batch * hw * hw == M else (1, M, 1)
        torch.manual_seed(M + N + K)
        dgrad = kind == 4
        C, Kc = (N, K) if dgrad else (K, N)      # conv channels: x has C, y has Kc
        x = torch.randn(n, h, w_, C, device=dev).to(BF)
        y = torch.randn(n, h, w_, Kc, device=dev).to(BF)
        wgt = (torch.randn(Kc, 1, 1, C, device=dev) / C ** 0.5).to(BF)
        wt = wgt.reshape(Kc, C).t().contiguous().reshape(C, 1, 1, Kc)
        sums = torch.zeros(BN_SHARDS * 2 * Kc, device=dev, dtype=torch.float64) if kind in (2, 3) else None

        def run():
            if dgrad:
                T.conv_dgrad_pre(y, wgt, wt, x, 1, 0, 1, x_mask)
            else:
                T.conv_fwd(x, wgt, y, 1, 0, 1, None, kind in (1, 3), sums)

        x_mask = torch.randn(n, h, w_, C, device=dev).to(BF) if dgrad else None
        res = {}
        try:
            T.conv_pw_gemm_policy(0, 0)
            res[0] = time_us(run, a.iters)
            for tile in (64, 65, 128, 129, 256):
                if tile in (65, 129) and (K // 64) % 2:
                    continue
                if tile == 256 and (M < 256 or N < 256):
                    continue
                T.conv_pw_gemm_policy(2, tile)
                res[tile] = time_us(run, a.iters)
        finally:
            T.conv_pw_gemm_policy(1, 0)
        best = min((v, k) for k, v in res.items() if k)
        cell = lambda k: f"{res[k]:.1f}" if k in res else "-"
        out.append(f"| {M} | {N} | {K} | {KINDS[kind]} | {cell(0)} | {cell(64)} | {cell(65)} | {cell(128)} | {cell(129)} | "
                   f"{cell(256)} | {best[1]} ({best[0]:.1f}) | {ln[7]} {ln[12] if ln[7] == 'p8' else ''} "
                   f"({float(ln[10]) * 1e3:.1f} vs {float(ln[11]) * 1e3:.1f}) |")
        print(out[-1], flush=True)
    text = "\n".join(out) + "\n"
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
