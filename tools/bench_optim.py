"""Fused optimizer kernels (csrc/kernels/optim.hip) on the model arenas'
sizes: achieved HBM bandwidth of one SGD-momentum / AdamW step (bytes =
master+grad+state reads, master+state+grad-zero+bf16 shadow writes).

``--clip`` also times, per arena at the production variant / grid, the
global-norm pass alone (grad_sumsq + grad_clip_finalize, 4 B/param read) and
the optimizer step with and without the norm pass + ``clip`` record in front
of it (the difference is what clipping adds to a step).

``--bf16-state`` also times, per arena at the production variant / grid, the
step with fp32 state against the step with bf16 state and Philox stochastic
rounding (``*_step_bf16s``), interleaved, with the bytes each form moves per
element (Adam 34 -> 26, SGD 26 -> 22).

``--trust-ratio`` also times, per arena with the model's real segment layout,
the plain step against the layer-wise trust-ratio step of the same build
(``lars_step`` on the SGD arenas, ``lamb_step`` on the Adam arenas: segmented
norms, finalize, apply), interleaved in one process, with the bytes each form
moves per element (SGD 26 -> LARS 34, Adam 34 -> LAMB 46).
``OPTIM_VARIANTS=3`` skips the variant sweep in front of it."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from tiresias_amd.ops import _lib  # noqa: E402


def timeit(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3        # us


def main():
    clip_rows = "--clip" in sys.argv
    if clip_rows:
        sys.argv.remove("--clip")
    bf16_rows = "--bf16-state" in sys.argv
    if bf16_rows:
        sys.argv.remove("--bf16-state")
    trust_rows = "--trust-ratio" in sys.argv
    if trust_rows:
        sys.argv.remove("--trust-ratio")
    _lib.load(required=True)
    T = _lib.ops()
    dev = torch.device("cuda", 0)
    out = []
    variants = [int(v) for v in os.environ.get("OPTIM_VARIANTS", "0,3").split(",")]
    grids = [int(v) for v in os.environ.get("OPTIM_GRIDS", "0").split(",")]
    for name, n, opt in [("vgg16", 138360448, "sgd"), ("resnet50", 25572736, "sgd"),
                         ("gnmt", 226561280, "adam"), ("transformer", 60524544, "adam")]:
        w = torch.randn(n, device=dev); g = torch.randn(n, device=dev)
        m = torch.zeros(n, device=dev); wb = torch.empty(n, device=dev, dtype=torch.bfloat16)
        v = torch.zeros(n, device=dev) if opt == "adam" else None
        for var, grid in [(v_, g_) for v_ in variants for g_ in grids] * 2:   # two interleaved rounds
            T.optim_variant(var)
            T.optim_grid(grid)
            if opt == "sgd":
                us = timeit(lambda: T.sgd_step(w, g, m, wb, 0.1, 0.9, 1e-4, 1.0, False, True))
                nbytes = n * (12 + 12 + 2)
            else:
                us = timeit(lambda: T.adam_step(w, g, m, v, wb, 1e-3, 0.9, 0.98, 1e-9, 0.01, 3, 1.0, True))
                nbytes = n * (16 + 16 + 2)
            r = dict(model=name, opt=opt, variant=var, grid=grid, params=n, us=round(us, 1),
                     tb_per_s=round(nbytes / us / 1e6, 2))
            print(json.dumps(r), flush=True)
            out.append(r)
        T.optim_variant(-1)
        T.optim_grid(0)
        if clip_rows:
            part = torch.zeros(int(T.grad_sumsq_blocks(n)), dtype=torch.float64, device=dev)
            rec = torch.zeros(4, device=dev)

            def norm():
                T.grad_sumsq(g, part)
                T.grad_clip_finalize(part, 5.0, 1.0, rec)

            def step(c):
                if opt == "sgd":
                    T.sgd_step(w, g, m, wb, 0.1, 0.9, 1e-4, 1.0, False, True, None, 0, -1, c)
                else:
                    T.adam_step(w, g, m, v, wb, 1e-3, 0.9, 0.98, 1e-9, 0.01, 3, 1.0, True, None, 0, -1, c)

            def clipped():
                norm()
                step(rec)

            for _ in range(2):                                                # two interleaved rounds
                for kind, fn, nb in (("norm", norm, 4 * n), ("step", lambda: step(None), nbytes),
                                     ("norm+step_clip", clipped, nbytes + 4 * n)):
                    us = timeit(fn)
                    r = dict(model=name, opt=opt, kind=kind, params=n, us=round(us, 1),
                             tb_per_s=round(nb / us / 1e6, 2))
                    print(json.dumps(r), flush=True)
                    out.append(r)
            del part, rec
        if bf16_rows:
            mb = torch.zeros(n, device=dev, dtype=torch.bfloat16)
            vb = torch.zeros(n, device=dev, dtype=torch.bfloat16) if opt == "adam" else None
            step_no = [0]

            def f32():
                if opt == "sgd":
                    T.sgd_step(w, g, m, wb, 0.1, 0.9, 1e-4, 1.0, False, True)
                else:
                    T.adam_step(w, g, m, v, wb, 1e-3, 0.9, 0.98, 1e-9, 0.01, 3, 1.0, True)

            def b16():
                step_no[0] += 1
                if opt == "sgd":
                    T.sgd_step_bf16s(w, g, mb, wb, 0.1, 0.9, 1e-4, 1.0, False, True, 1, step_no[0], 0)
                else:
                    T.adam_step_bf16s(w, g, mb, vb, wb, 1e-3, 0.9, 0.98, 1e-9, 0.01, step_no[0], 1.0, True, 1, 0)

            per = {"sgd": (26, 22), "adam": (34, 26)}[opt]
            for _ in range(3):                                                # three interleaved rounds
                for kind, fn, bpe in (("fp32_state", f32, per[0]), ("bf16_state", b16, per[1])):
                    us = timeit(fn)
                    r = dict(model=name, opt=opt, kind=kind, params=n, bytes_per_elem=bpe, us=round(us, 1),
                             tb_per_s=round(bpe * n / us / 1e6, 2))
                    print(json.dumps(r), flush=True)
                    out.append(r)
            del mb, vb
        if trust_rows:
            from tiresias_amd.models import make_model
            from tiresias_amd.ops.arena import Arena, _padded, trust_tile_table

            lay = Arena("cpu")                   # the model's real segment layout; nothing is materialized
            make_model(name, lay)
            lay.layout()
            assert lay.numel == n, (name, lay.numel, n)
            nd = lay.n_decay
            segs = [(p.offset, _padded(p.numel)) for p in lay.decay_segments()]
            tiles, first = trust_tile_table(segs, int(T.trust_tile()))
            tiles, first = tiles.to(dev), first.to(dev)
            part = torch.zeros(2 * tiles.shape[0], dtype=torch.float64, device=dev)
            ratios = torch.zeros(len(segs), 3, device=dev)

            def plain():
                if opt == "sgd":
                    T.sgd_step(w, g, m, wb, 0.1, 0.9, 1e-4, 1.0, False, True, None, 0, nd)
                else:
                    T.adam_step(w, g, m, v, wb, 1e-3, 0.9, 0.98, 1e-9, 0.01, 3, 1.0, True, None, 0, nd)

            def trust():
                if opt == "sgd":
                    T.lars_step(w, g, m, wb, 0.1, 0.9, 1e-4, 1e-3, 1.0, tiles, first, part, ratios, None, 0, nd)
                else:
                    T.lamb_step(w, g, m, v, wb, 1e-3, 0.9, 0.98, 1e-9, 0.01, 3, 1.0, 1.0, tiles, first, part, ratios,
                                None, 0, nd)

            # bytes per element: the plain step, and the three passes (LARS:
            # w g | w g mom -> w mom g wb; LAMB: w g m v -> m v g | w m v -> w wb)
            per = {"sgd": (26, 34), "adam": (34, 46)}[opt]
            for _ in range(3):                                                # three interleaved rounds
                g.normal_()          # (the steps zero the gradient: refill, so no round times a zero one)
                for kind, fn, bpe in (("plain", plain, per[0]), ("lars" if opt == "sgd" else "lamb", trust, per[1])):
                    us = timeit(fn)
                    r = dict(model=name, opt=opt, kind=kind, params=n, segments=len(segs), tiles=int(tiles.shape[0]),
                             tile=int(T.trust_tile()), bytes_per_elem=bpe, us=round(us, 1),
                             tb_per_s=round(bpe * n / us / 1e6, 2))
                    print(json.dumps(r), flush=True)
                    out.append(r)
            del tiles, first, part, ratios
        del v
        del w, g, m, wb
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
