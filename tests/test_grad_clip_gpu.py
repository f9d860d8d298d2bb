"""Global-norm gradient clipping on the device (csrc/kernels/optim.hip):
grad_sumsq + grad_clip_finalize, the optimizer kernels' ``clip`` record, the
non-finite-step skip, and the Trainer path under hipGraph replay."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
# < one wave's worth; the tail after the unrolled groups; several grid sweeps + a tail
SIZES = [64, 64 * 1000 + 64, 3 * 2 ** 20 + 4 * 1000]


def T():
    return torch.ops.tam


@pytest.fixture(scope="module")
def grads(gpu):
    """n -> (seeded gradient, its fp64 norm); computed once, never written."""
    out = {}
    gen = torch.Generator(device=gpu)
    gen.manual_seed(21)
    for n in SIZES:
        g = torch.randn(n, device=gpu, generator=gen)
        out[n] = (g, float(g.double().norm()))
    return out


def _record(g, max_norm, gscale=1.0, clip=None, slots=None):
    """grad_sumsq + grad_clip_finalize -> the clip record (device)."""
    blocks = int(T().grad_sumsq_blocks(g.numel()))
    part = torch.full((slots or blocks,), 1e300, dtype=torch.float64, device=g.device)
    if clip is None:
        clip = torch.zeros(4, device=g.device)
    T().grad_sumsq(g, part)
    T().grad_clip_finalize(part, max_norm, gscale, clip)
    return clip


def _words(clip):
    rec = clip.cpu()
    cnt = rec.view(torch.int32)
    return float(rec[0]), float(rec[1]), int(cnt[2]), int(cnt[3])


def _bits(x):
    return int(np.float32(x).view(np.int32))


@pytest.mark.parametrize("n", SIZES)
def test_norm_accuracy_and_determinism(gpu, grads, n):
    """fp64 accumulation: the fp32 rounding of the final value is the only
    error; two calls give the same bits; slots past the grid do not count."""
    g, ref = grads[n]
    a = _record(g, 1.0)
    b = _record(g, 1.0)
    c = _record(g, 1.0, slots=int(T().grad_sumsq_blocks(n)) + 37)
    norm = _words(a)[1]
    print(f"n={n} norm={norm!r} ref={ref!r} rel={abs(norm - ref) / ref:.3e}")
    assert abs(norm - ref) / ref <= 1e-6
    assert torch.equal(a[:2].view(torch.int32), b[:2].view(torch.int32))
    assert torch.equal(a[:2].view(torch.int32), c[:2].view(torch.int32))


@pytest.mark.parametrize("n", SIZES)
def test_clip_formula(gpu, grads, n):
    g, ref = grads[n]
    lo = float(np.float32(0.5 * ref))
    clip = _record(g, lo)
    scale, norm, nonfinite, clipped = _words(clip)
    want = np.float32(np.float64(lo) / (np.float64(np.float32(norm)) + 1e-6))
    print(f"n={n} scale={scale!r} want={float(want)!r}")
    assert abs(_bits(scale) - _bits(want)) <= 1
    assert (nonfinite, clipped) == (0, 1)
    # below the limit: exactly 1, the clipped count stays
    scale2, norm2, nonfinite, clipped = _words(_record(g, 2.0 * ref, clip=clip))
    assert scale2 == 1.0 and norm2 == norm and (nonfinite, clipped) == (0, 1)
    # the norm is that of gscale * g
    _, norm3, _, _ = _words(_record(g, 2.0 * ref, gscale=0.25))
    assert norm3 == 0.25 * norm


def _state(gpu, n, seed):
    gen = torch.Generator(device=gpu)
    gen.manual_seed(seed)
    w, g, m, v = (torch.randn(n, device=gpu, generator=gen) for _ in range(4))
    v.abs_()
    return [w, g, m, v, w.to(BF)]


def _step(opt, s, gscale, clip, zf, wu, step=3):
    if opt == "sgd":
        T().sgd_step(s[0], s[1], s[2], s[4], 0.1, 0.9, 1e-2, gscale, False, True, None, zf, wu, clip)
    else:
        T().adam_step(s[0], s[1], s[2], s[3], s[4], 1e-3, 0.9, 0.98, 1e-9, 1e-2, step, gscale, True, None, zf, wu,
                      clip)


@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_optimizer_consumes_clip_scale(gpu, opt, variant):
    """The record's scale is folded into gscale in fp32 before the element
    loop: bitwise the clip=None step at gscale * s; s = 1 changes nothing."""
    n, zf, wu = SIZES[2], 64 * 100, SIZES[2] - 4 * 1000 - 64 * 100
    T().optim_variant(variant)
    try:
        base = _state(gpu, n, 22)
        for s_clip, gs, gs_eff in ((0.37, 0.5, float(np.float32(0.5) * np.float32(0.37))), (1.0, 0.5, 0.5)):
            clip = torch.tensor([s_clip, 0.0, 0.0, 0.0], device=gpu)
            a = [t.clone() for t in base]
            b = [t.clone() for t in base]
            _step(opt, a, gs, clip, zf, wu)
            _step(opt, b, gs_eff, None, zf, wu)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (opt, variant, s_clip)
            assert not torch.equal(a[0], base[0])
    finally:
        T().optim_variant(-1)


@pytest.mark.parametrize("variant", [0, 3])
@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_step_is_skipped(gpu, bad, opt, variant):
    n, zf, wu = SIZES[1], 64 * 10, 64 * 500
    T().optim_variant(variant)
    try:
        s = _state(gpu, n, 23)
        clean = s[1].clone()
        s[1][zf + 12345] = bad
        before = [t.clone() for t in s]
        clip = _record(s[1], 1.0)
        _step(opt, s, 1.0, clip, zf, wu)
        for i in (0, 2, 3, 4):
            assert torch.equal(s[i], before[i]), i
        assert torch.equal(s[1][:zf], before[1][:zf]) and torch.count_nonzero(s[1][zf:]) == 0
        scale, norm, nonfinite, clipped = _words(clip)
        assert scale == -1.0 and not np.isfinite(norm) and (nonfinite, clipped) == (1, 0)
        # a clean step after it updates normally
        s[1].copy_(clean)
        twin = [t.clone() for t in s]
        _record(s[1], 1e30, clip=clip)
        _step(opt, s, 1.0, clip, zf, wu)
        _step(opt, twin, 1.0, None, zf, wu)
        for x, y in zip(s, twin):
            assert torch.equal(x, y)
        assert not torch.equal(s[0], before[0])
        assert _words(clip)[0] == 1.0 and _words(clip)[2:] == (1, 0)
    finally:
        T().optim_variant(-1)


def test_binding_checks(gpu, grads):
    g, _ = grads[SIZES[1]]
    clip = torch.zeros(4, device=gpu)
    with pytest.raises(RuntimeError, match="slots"):
        T().grad_sumsq(g, torch.zeros(int(T().grad_sumsq_blocks(g.numel())) - 1, dtype=torch.float64, device=gpu))
    with pytest.raises(RuntimeError, match="float64"):
        T().grad_sumsq(g, torch.zeros(4096, device=gpu))
    with pytest.raises(RuntimeError, match="numel % 4"):
        T().grad_sumsq(g[:62], torch.zeros(4096, dtype=torch.float64, device=gpu))
    with pytest.raises(RuntimeError, match="clip"):
        T().grad_clip_finalize(torch.zeros(8, dtype=torch.float64, device=gpu), 1.0, 1.0, clip[:3])
    with pytest.raises(RuntimeError, match="max_norm"):
        T().grad_clip_finalize(torch.zeros(8, dtype=torch.float64, device=gpu), 0.0, 1.0, clip)


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("model", ["transformer_tiny", "gnmt_tiny"])
def test_trainer_clips_under_graph_replay(gpu, model):
    from tiresias_amd.executor.trainer import Trainer
    from tiresias_amd.ops import functional as Fx

    t = Trainer(model, gpu, seed=0, use_graph=True, grad_clip=1e30)
    A = t.arena
    for _ in range(3):           # two eager warm steps, then capture + first replay
        t.step()
    assert t._graph is not None
    torch.cuda.synchronize()
    assert t.clip_stats()["clipped_steps"] == 0 and t.clip_stats()["last_scale"] == 1.0

    def fwd_bwd():
        """One replayed forward+backward; the gradient the optimizer will see."""
        t._graph_step()
        for p in A.params:
            if p.store_grad and p.gw_epoch != A.grad_epoch:
                p.grad.zero_()
        g = A.grad.clone()
        return g, float(g.double().norm())

    # 1. clip far above the norm: bitwise the clip=None step
    g, ref = fwd_bwd()
    twin = [A.master.clone(), g.clone(), t.opt_state[0].clone(), t.opt_state[1].clone(), A.shadow.clone()]
    t._opt_step()
    zf = A.n_store if Fx.STORE_GRAD else 0
    T().adam_step(twin[0], twin[1], twin[2], twin[3], twin[4], t.lr, 0.9, 0.98, 1e-9, t.spec.wd, t.step_count, 1.0,
                  True, None, zf, A.n_decay)
    torch.cuda.synchronize()
    st = t.clip_stats()
    print(model, "norm", st["last_norm"], "ref", ref)
    assert abs(st["last_norm"] - ref) / ref <= 1e-6
    assert st["last_scale"] == 1.0 and st["clipped_steps"] == 0 and st["nonfinite_steps"] == 0
    assert torch.equal(A.master, twin[0]) and torch.equal(A.shadow, twin[4])
    assert torch.count_nonzero(A.grad[zf:]) == 0

    # 2. clip at half the norm: the host formula with the reported scale
    g, ref = fwd_bwd()
    w0, m0, v0 = A.master.double(), t.opt_state[0].double(), t.opt_state[1].double()
    t.set_grad_clip(0.5 * ref)
    t._opt_step()
    torch.cuda.synchronize()
    st = t.clip_stats()
    assert abs(st["last_norm"] - ref) / ref <= 1e-6
    want = 0.5 * ref / (st["last_norm"] + 1e-6)
    assert abs(st["last_scale"] - want) <= 1e-6 * want and st["clipped_steps"] == 1
    gr = g.double() * st["last_scale"]
    m = 0.9 * m0 + 0.1 * gr
    v = 0.98 * v0 + 0.02 * gr * gr
    k = t.step_count
    wd = torch.zeros_like(w0)
    wd[:A.n_decay] = t.spec.wd
    w_ref = w0 - t.lr * ((m / (1 - 0.9 ** k)) / ((v / (1 - 0.98 ** k)).sqrt() + 1e-9) + wd * w0)
    err = _rel(A.master, w_ref)
    print(model, "clipped master rel err", err)
    assert err < 1e-5                     # tests/test_kernels_gpu.py::_sgd_adam_check, Adam
    assert _rel(t.opt_state[0], m) < 1e-5 and _rel(t.opt_state[1], v) < 1e-5

    # 3. the pooled trainer as a fresh job: counters zeroed
    t.reset(1)
    torch.cuda.synchronize()
    st = t.clip_stats()
    assert st["clipped_steps"] == 0 and st["nonfinite_steps"] == 0
    t.release()


def test_trainer_clip_off_allocates_nothing(gpu):
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer("transformer_tiny", gpu, seed=0)
    assert t.grad_clip is None and t._clip is None and t._clip_part is None
    t.step()
    assert t.clip_stats()["clipped_steps"] == 0
    t.release()
