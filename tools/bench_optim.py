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

``--q8-state`` also times, per arena, the step with fp32 state, with bf16
state and with 8-bit block-scaled state (``*_step_q8``, optim_q8.hip),
interleaved, with the bytes each moves per element (Adam 34 / 26 / 22, SGD
26 / 22 / 20). Every timed launch of this mode gets a fresh random gradient
and a nonzero state, so that the q8 encoder has work.

``--trust-ratio`` also times, per arena with the model's real segment layout,
the plain step against the layer-wise trust-ratio step of the same build
(``lars_step`` on the SGD arenas, ``lamb_step`` on the Adam arenas: segmented
norms, finalize, apply), interleaved in one process, with the bytes each form
moves per element (SGD 26 -> LARS 34, Adam 34 -> LAMB 46).
``OPTIM_VARIANTS=3`` skips the variant sweep in front of it.

``--factored`` also times, on the Adam arenas with the model's real parameter
shapes, ``adam_step`` against ``adafactor_step`` (adafactor.hip: six launches
over the arena), interleaved in one process, with the bytes each moves per
element (Adam 34, Adafactor 26: three reads of g, w read and written, shadow,
gradient reset) and the optimizer-state bytes of each. ``OPTIM_MODELS=a,b``
restricts every mode to those arenas."""
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
    q8_rows = "--q8-state" in sys.argv
    if q8_rows:
        sys.argv.remove("--q8-state")
    trust_rows = "--trust-ratio" in sys.argv
    if trust_rows:
        sys.argv.remove("--trust-ratio")
    factored_rows = "--factored" in sys.argv
    if factored_rows:
        sys.argv.remove("--factored")
    only = [m for m in os.environ.get("OPTIM_MODELS", "").split(",") if m]
    _lib.load(required=True)
    T = _lib.ops()
    dev = torch.device("cuda", 0)
    out = []
    variants = [int(v) for v in os.environ.get("OPTIM_VARIANTS", "0,3").split(",")]
    grids = [int(v) for v in os.environ.get("OPTIM_GRIDS", "0").split(",")]
    for name, n, opt in [("vgg16", 138360448, "sgd"), ("resnet50", 25572736, "sgd"),
                         ("gnmt", 226561280, "adam"), ("transformer", 60524544, "adam")]:
        if only and name not in only:
            continue
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
        if q8_rows:
            nb = -(-n // 256)
            k = 1 if opt == "sgd" else 2
            mq = torch.zeros(256 * nb, device=dev, dtype=torch.int8)
            vq = torch.zeros(256 * nb, device=dev, dtype=torch.uint8) if opt == "adam" else None
            sc = torch.zeros(k, nb, device=dev)
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

            def q8():
                step_no[0] += 1
                if opt == "sgd":
                    T.sgd_step_q8(w, g, mq, sc, wb, 0.1, 0.9, 1e-4, 1.0, False, True, 1, step_no[0])
                else:
                    T.adam_step_q8(w, g, mq, vq, sc, wb, 1e-3, 0.9, 0.98, 1e-9, 0.01, step_no[0], 1.0, True, 1)

            # Every step zeroes the gradient, and on a zero gradient with zero state the q8 encoder has nothing to
            # do (a block whose max is 0 stores codes 0 without looking anything up). So every timed launch gets
            # a fresh random gradient, refilled outside its event pair, after a 512 MiB write that takes the
            # refilled lines out of the caches again; the warm launch leaves a nonzero state behind.
            flush = torch.empty(1 << 29, device=dev, dtype=torch.uint8)

            def timeit_live(fn, iters=20):
                g.normal_()
                fn()
                evs = []
                for _ in range(iters):
                    g.normal_()
                    flush.zero_()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    evs.append((a, b))
                torch.cuda.synchronize()
                return sum(a.elapsed_time(b) for a, b in evs) / iters * 1e3     # us

            # bytes per element (the block scales add 8 k / 256)
            per = {"sgd": (26, 22, 20), "adam": (34, 26, 22)}[opt]
            for _ in range(3):                                                # three interleaved rounds
                for kind, fn, bpe in (("fp32_state", f32, per[0]), ("bf16_state", b16, per[1]),
                                      ("q8_state", q8, per[2])):
                    us = timeit_live(fn)
                    r = dict(model=name, opt=opt, kind=kind, params=n, bytes_per_elem=bpe, us=round(us, 1),
                             tb_per_s=round(bpe * n / us / 1e6, 2))
                    print(json.dumps(r), flush=True)
                    out.append(r)
            assert bool(torch.count_nonzero(mq)) and bool(torch.count_nonzero(sc))   # the encoder had work
            del mq, vq, sc, mb, vb, flush
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
        if factored_rows and opt == "adam":
            from tiresias_amd.models import make_model
            from tiresias_amd.ops.arena import Arena, adafactor_tables

            lay = Arena("cpu")                   # the model's real parameter shapes; nothing is materialized
            make_model(name, lay)
            order = lay.layout()
            assert lay.numel == n, (name, lay.numel, n)
            nd = lay.n_decay
            tabs = adafactor_tables([(p.offset, p.shape) for p in order], *[int(x) for x in T.adafactor_tile()])
            params, tiles, tasks = (t.to(dev) for t in tabs[:3])
            nstate, npart = tabs[3:]
            state, fac = torch.zeros(nstate, device=dev), torch.zeros(nstate, device=dev)
            part = torch.zeros(npart, device=dev)
            slots = torch.zeros(tiles.shape[0], dtype=torch.float64, device=dev)
            urms = torch.zeros(len(order), 2, device=dev)

            def adam():
                T.adam_step(w, g, m, v, wb, 1e-3, 0.9, 0.98, 1e-9, 0.01, 3, 1.0, True, None, 0, nd)

            def adafactor():
                T.adafactor_step(w, g, state, fac, wb, 1e-3, 0.01, 3, 1.0, params, tiles, tasks, part, slots, urms,
                                 None, 0, nd)

            for grid in grids * 3:                                            # three interleaved rounds
                T.optim_grid(grid)
                g.normal_()          # (the steps zero the gradient: refill, so no round times a zero one)
                for kind, fn, bpe, sb in (("adam", adam, 34, 8 * n), ("adafactor", adafactor, 26, 4 * nstate)):
                    us = timeit(fn)
                    r = dict(model=name, opt=opt, kind=kind, grid=grid, params=n, tensors=len(order),
                             tiles=int(tiles.shape[0]), state_bytes=sb, bytes_per_elem=bpe, us=round(us, 1),
                             tb_per_s=round(bpe * n / us / 1e6, 2))
                    print(json.dumps(r), flush=True)
                    out.append(r)
            T.optim_grid(0)
            del params, tiles, tasks, state, fac, part, slots, urms
        del v
        del w, g, m, wb
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:
        json.dump(out, open(sys.argv[1], "w"), indent=1)


if __name__ == "__main__":
    main()
