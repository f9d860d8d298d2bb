"""8-bit block-scaled optimizer state (opt_dtype="q8") without a GPU: the
value from the submit CLI to the start action and the pool key, the
rejections, the pricing identities, and the torch mirror of the contract
against an fp64 step. ``make_case`` / ``run`` / ``check_step`` are shared with
tests/test_opt_q8_gpu.py, which runs the same checks on the kernels."""
import json
import os

import pytest
import torch

from tiresias_amd.executor.trainer import Trainer, _cpu_opt_q8
from tiresias_amd.ops import functional as Fx

F32 = lambda x: float(torch.tensor(x, dtype=torch.float32))        # a scalar as the kernels receive it
B1, B2, MOM, EPS, LR, WD, GSCALE = F32(0.9), F32(0.98), F32(0.9), F32(1e-9), F32(1e-2), F32(0.01), F32(0.37)
# Bound of a fresh moment against fp64: at most 6 fp32 roundings (clip fold, g * gscale, (1 - b) * g, * g for v,
# wd * w for SGD, the FMA), each <= 2^-24 of the FMA's addends |a| + |b|; 8 * 2^-24 covers them. A block scale (a
# max of such values) and y = |x| / s inherit it.
ULPS = 2.0 ** -21


def make_case(opt, n, seed=0):
    """A padded arena of n elements with a NONZERO prior q8 state; zero_from
    and wd_until are multiples of 4 inside a block, not of 256."""
    gen = torch.Generator().manual_seed(1000 * seed + n)
    nb = -(-n // 256)
    c = dict(n=n, w=torch.randn(nb * 256, generator=gen), g=torch.randn(nb * 256, generator=gen),
             mq=torch.randint(-127, 128, (nb * 256,), generator=gen).to(torch.int8),
             vq=torch.randint(64, 256, (nb * 256,), generator=gen).to(torch.uint8),
             scales=torch.stack([0.05 + 0.1 * torch.rand(nb, generator=gen), 1e-3 + 1e-2 * torch.rand(nb, generator=gen)]),
             zf=4 * (n // 12), wu=4 * max(1, n // 6))
    c["mq"][n:] = 0
    c["vq"][n:] = 0
    if opt == "sgd":
        c["scales"] = c["scales"][:1].clone()
    return c


def run(opt, c, dev, step=3, seed=5, gs=GSCALE, guard=None, clip=None, lr=LR, wd=WD):
    """One step on copies: [w, g, wb, state] on the CPU, w / g / wb at their
    padded length (the step sees the first n elements)."""
    n = c["n"]
    full = [c["w"].to(dev).clone(), c["g"].to(dev).clone(), torch.ones(c["w"].numel(), dtype=torch.bfloat16, device=dev)]
    state = [c[k].to(dev).clone() for k in (("mq", "scales") if opt == "sgd" else ("mq", "vq", "scales"))]
    w, g, wb = (t[:n] for t in full)
    if torch.device(dev).type == "cpu":
        _cpu_opt_q8(opt, w, g, state, wb, lr, wd, gs, step, seed, c["zf"], c["wu"])
    elif opt == "sgd":
        torch.ops.tam.sgd_step_q8(w, g, state[0], state[1], wb, lr, MOM, wd, gs, False, True, seed, step, guard,
                                  c["zf"], c["wu"], clip)
    else:
        torch.ops.tam.adam_step_q8(w, g, state[0], state[1], state[2], wb, lr, B1, B2, EPS, wd, step, gs, True, seed,
                                   guard, c["zf"], c["wu"], clip)
    return [t.cpu() for t in full] + [[s.cpu() for s in state]]


def check_step(opt, c, out, step=3, gs=GSCALE):
    """``out`` = run(...) against the fp64 step from the decoded prior state."""
    n, zf = c["n"], c["zf"]
    w, g, wb, state = out
    w0, g0 = c["w"][:n].double(), c["g"][:n].double() * gs
    wd = torch.zeros(n, dtype=torch.float64)
    wd[:c["wu"]] = WD
    m = Fx.q8_decode(c["mq"], c["scales"][0])[:n].double()
    if opt == "sgd":
        a, b = MOM * m, wd * w0 + g0
        moms = [(a + b, a.abs() + b.abs())]
        w2 = w0 - LR * (a + b)
    else:
        v = Fx.q8_decode(c["vq"], c["scales"][1])[:n].double()
        a, b, av, bv = B1 * m, (1 - B1) * g0, B2 * v, (1 - B2) * g0 * g0
        moms = [(a + b, a.abs() + b.abs()), (av + bv, av + bv)]
        w2 = w0 - LR * ((a + b) / (1 - B1 ** step) / (((av + bv) / (1 - B2 ** step)).sqrt() + EPS) + wd * w0)
    # weights as the fp32-state optimizer tests hold them; shadow, gradient reset, nothing past n touched
    assert torch.allclose(w[:n].double(), w2, atol=1e-6)
    assert torch.equal(wb[:n], w[:n].to(torch.bfloat16)) and bool((wb[n:] == 1).all())
    assert torch.equal(g[:zf], c["g"][:zf]) and int(torch.count_nonzero(g[zf:n])) == 0
    assert torch.equal(w[n:], c["w"][n:]) and torch.equal(g[n:], c["g"][n:])
    for i, (x, mag) in enumerate(moms):
        tab = Fx.q8_tables()[i].double()
        top = tab.numel() - 1
        xb, eb = torch.zeros(2, state[i].numel(), dtype=torch.float64)
        xb[:n], eb[:n] = x, ULPS * mag
        xb, eb = xb.view(-1, 256), eb.view(-1, 256)
        s, es = xb.abs().amax(1, keepdim=True), eb.amax(1, keepdim=True)
        got = state[-1][i].double()[:, None]
        assert bool(((got - s).abs() <= es).all())
        code = state[i].to(torch.int64).view(-1, 256)
        k = code.abs()
        y = xb.abs() / s
        ty = (eb + es * y) / s + ULPS * y
        # one of the two table neighbours of y (either side of a table point within the bound)
        assert bool(((y >= tab[(k - 1).clamp(min=0)] - ty) & (y <= tab[(k + 1).clamp(max=top)] + ty)).all())
        assert bool((k.gather(1, xb.abs().argmax(1, keepdim=True)) == top).all())      # the block max is +-127 / 255
        assert bool(((code.sign() == xb.sign()) | (k == 0) | (xb.abs() <= eb)).all())
        if i == 1:
            assert bool((k[xb.abs() > eb] >= 1).all())                                 # no nonzero v is code 0


# ------------------------------------------------------------------ the mirror
@pytest.mark.parametrize("n", [64, 256 * 2 + 64])
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_mirror_step_against_fp64(opt, n):
    c = make_case(opt, n)
    out = run(opt, c, "cpu")
    check_step(opt, c, out)
    again, other = run(opt, c, "cpu"), run(opt, c, "cpu", seed=6)
    assert all(torch.equal(a, b) for a, b in zip(out[3], again[3])) and torch.equal(out[0], again[0])
    assert not torch.equal(out[3][0], other[3][0]) and torch.equal(out[0], other[0])   # only the rounding moves


def test_encoder_fixed_points():
    x = torch.zeros(768)
    x[:4] = torch.tensor([2.0, -2.0, 1e-12, 0.0])
    x[256], x[512] = float("inf"), 1e-44                             # a poisoned block, a subnormal block max
    u = torch.full((768,), 0xFFFF, dtype=torch.int64)                # the draw that never rounds up
    (mq, sm), (vq, _) = Fx.q8_encode(x, u, False), Fx.q8_encode(x.abs(), u, True)
    assert mq[:4].tolist() == [127, -127, 0, 0] and vq[:4].tolist() == [255, 255, 1, 0]   # max exact, v floored at 1
    assert float(sm[1]) == float("inf") and bool(torch.isnan(Fx.q8_decode(mq, sm)[256:512]).all())
    assert mq[512:516].tolist() == [127, 0, 0, 0] and float(sm[2]) == float(x[512])


@pytest.mark.parametrize("model", ["transformer_tiny", "resnet_tiny"])
def test_cpu_trainer(model):
    t, f = Trainer(model, "cpu", seed=3, opt_dtype="q8", grad_clip=1e3), Trainer(model, "cpu", seed=3)
    n, k = t.arena.numel, len(f.opt_state)
    nb = -(-n // 256)
    assert [s.dtype for s in t.opt_state] == [torch.int8, torch.uint8][:k] + [torch.float32]
    assert f.state_bytes() - t.state_bytes() == k * (4 * n - 256 * nb - 4 * nb) == f.hbm_bytes() - t.hbm_bytes()
    losses = [float(t.step()) for _ in range(3)]
    assert all(x == x for x in losses) and all(bool(torch.count_nonzero(s)) for s in t.opt_state)
    before = [s.clone() for s in t.opt_state] + [t.arena.master.clone()]
    t._fwd_bwd()
    t.arena.grad[5] = float("inf")                       # a non-finite gradient norm: the step is skipped
    t._opt_step()
    assert all(torch.equal(a, b) for a, b in zip(list(t.opt_state) + [t.arena.master], before))
    assert int(torch.count_nonzero(t.arena.grad)) == 0 and t.clip_stats()["nonfinite_steps"] == 1


# ------------------------------------------------------------------ plumbing
def test_value_travels_and_is_rejected_where_it_cannot_run(tmp_path):
    from test_opt_dtype_cpu import _fake_controller_run
    from types import SimpleNamespace

    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.core.job import JobSpec
    from tiresias_amd.engine.ckpt_model import CkptCostModel
    from tiresias_amd.executor import fake
    from tiresias_amd.executor.cluster_runtime import Worker
    from tiresias_amd.profiler.skew import model_profile
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    assert submit_cli.main(["--spool", sp.root, "--model", "gnmt", "--iterations", "3", "--job-id", "a",
                            "--opt-dtype", "q8"]) == 0
    assert json.load(open(os.path.join(sp.root, "incoming", "a.json")))["opt_dtype"] == "q8"
    sp.submit("vgg16", 2, iterations=3, job_id="b", opt_dtype="q8")               # sgd, a replicated gang
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)
    assert len(ctrl.sched.finished) == 2 and {a["job"]: a["opt_dtype"] for a in starts} == {"a": "q8", "b": "q8"}
    base = {"model": "transformer", "iterations": 2, "job_id": "x", "opt_dtype": "q8"}
    with pytest.raises(ValueError, match="trust_ratio"):
        ctrl._validate(dict(base, trust_ratio=1e-3))
    ctrl.ddp_shard = True
    with pytest.raises(ValueError, match="opt_dtype.*ddp_shard"):
        ctrl._validate(dict(base, num_gpu=2))
    w = Worker(0, 1, torch.device("cpu"))
    t = w._make_trainer({"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1,
                         "ranks": (0,), "source": "fresh", "opt_dtype": "q8"})
    assert t.opt_dtype == "q8" and t.pool_key[-1:] == ("q8",)

    class _Comm:
        size, ranks = 2, (0, 1)

    with pytest.raises(ValueError, match="ddp_shard"):
        Trainer("transformer_tiny", "cpu", opt_dtype="q8", ddp_shard=True, group=_Comm())
    with pytest.raises(ValueError, match="trust_ratio"):
        Trainer("resnet_tiny", "cpu", opt_dtype="q8", trust_ratio=1e-3)
    # pricing: profiler, fake backend, checkpoint model and the admission estimate
    for model, opt, k in (("gnmt", "adam", 2), ("vgg16", "sgd", 1)):
        p = model_profile(model)
        want = 6 * p.params + 4 * k * -(-p.params // 256) + k * p.params
        assert p.state_bytes(opt, "q8") == want == fake._state_bytes(model, "q8")
        job = SimpleNamespace(spec=JobSpec("j", 0.0, 1.0, 1, model=model, opt_dtype="q8"))
        assert CkptCostModel("host").state_bytes_per_gpu(job) == want
    p = model_profile("gnmt")
    assert w._job_need("gnmt", None, "q8") == 1.5 * p.state_bytes("adam", "q8")
