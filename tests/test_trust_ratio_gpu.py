"""Layer-wise trust-ratio optimizers on the device (csrc/kernels/optim.hip
"layer-wise trust ratio"): lars_step / lamb_step against an fp64 host
reference of the contract, the ratio-1 fall-backs, grid independence, the
skipped step, the clip scale, the binding checks and the Trainer path under
hipGraph replay.

Bounds: a ratio of LARS is a quotient of fp64-accumulated norms rounded once
-> relative 1e-6 (the bound of test_grad_clip_gpu.py::
test_norm_accuracy_and_determinism); everything elementwise, and LAMB's
ratio (its ``u`` is fp32 arithmetic), rel_err < 1e-5 (tests/
test_kernels_gpu.py::_sgd_adam_check)."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
RATIO_BOUND = 1e-6
ADAM_BOUND = 1e-5
TAIL = 7 * 64


def T():
    return torch.ops.tam


def _f32(x):
    return float(np.float32(x))


def _layouts():
    tile = int(T().trust_tile())
    return {"small": [64, 64, 64, tile, tile + 64, 3 * tile + 5 * 64],
            "large": [64, 3 * 2 ** 20 + 5 * 64, 64]}


class Case:
    """A synthetic arena: decayed segments, a no-decay tail, tile tables."""

    def __init__(self, gpu, lens, seed):
        from tiresias_amd.ops.arena import trust_tile_table

        self.lens = lens
        self.offs = [sum(lens[:k]) for k in range(len(lens))]
        self.nd = sum(lens)
        self.n = self.nd + TAIL
        self.zf = 128                     # the gradient below it is left alone
        gen = torch.Generator(device=gpu)
        gen.manual_seed(seed)
        w, g, m, v = (torch.randn(self.n, device=gpu, generator=gen) for _ in range(4))
        for k, (o, n) in enumerate(self.bounds()):
            w[o:o + n] *= 2.0 ** k        # neighbouring ratios differ by large factors
            g[o:o + n] *= 2.0 ** -k
        v.abs_()
        self.w, self.g, self.m, self.v = w, g, m, v
        tiles, first = trust_tile_table(list(zip(self.offs, lens)), int(T().trust_tile()))
        self.tiles, self.first = tiles.to(gpu), first.to(gpu)
        self.nt, self.ns = tiles.shape[0], len(lens)

    def bounds(self):
        """(offset, length) of every segment, the tail last."""
        return list(zip(self.offs, self.lens)) + [(self.nd, TAIL)]

    def scratch(self):
        return (torch.full((2 * self.nt,), 1e300, dtype=torch.float64, device=self.w.device),
                torch.full((self.ns, 3), 7.0, device=self.w.device))

    def lars_state(self, zero_mom=True):
        mom = torch.zeros_like(self.w) if zero_mom else self.m.clone()
        return [self.w.clone(), self.g.clone(), mom, self.w.to(BF)]

    def lamb_state(self):
        return [self.w.clone(), self.g.clone(), self.m.clone(), self.v.clone(), self.w.to(BF)]


@pytest.fixture(scope="module")
def cases(gpu):
    """name -> Case; built once, the tests clone what they write."""
    return {k: Case(gpu, lens, 31 + i) for i, (k, lens) in enumerate(_layouts().items())}


def _lars(c, s, part, ratios, lr=0.1, eta=0.1, wd=1e-2, gscale=1.0, guard=None, clip=None, wu=None):
    T().lars_step(s[0], s[1], s[2], s[3], lr, 0.9, wd, eta, gscale, c.tiles, c.first, part, ratios, guard, c.zf,
                  c.nd if wu is None else wu, clip)


def _lamb(c, s, part, ratios, lr=0.05, eta=1.0, wd=0.01, gscale=1.0, guard=None, clip=None, step=3):
    T().lamb_step(s[0], s[1], s[2], s[3], s[4], lr, 0.9, 0.98, 1e-9, wd, step, eta, gscale, c.tiles, c.first, part,
                  ratios, guard, c.zf, c.nd, clip)


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


def _ratio(eta, wn, xn, extra=0.0):
    ok = 0.0 < wn < math.inf and 0.0 < xn < math.inf
    return eta * wn / (xn + extra * wn) if ok else 1.0


def _lars_ref(c, w, g, mom, lr, eta, wd, gscale):
    """The contract in fp64 on the host -> (ratios, mom, w)."""
    w, g, mom = w.double().cpu(), g.double().cpu() * gscale, mom.double().cpu()
    eta, wd, lr = _f32(eta), _f32(wd), _f32(lr)
    rs, mo, wo = [], mom.clone(), w.clone()
    for k, (o, n) in enumerate(c.bounds()):
        ws, gs = w[o:o + n], g[o:o + n]
        tail = k == len(c.lens)
        r = 1.0 if tail else _ratio(eta, float(ws.norm()), float(gs.norm()), wd)
        d = r * (gs + (0.0 if tail else wd) * ws)
        mo[o:o + n] = _f32(0.9) * mom[o:o + n] + d
        wo[o:o + n] = ws - lr * mo[o:o + n]
        if not tail:
            rs.append(r)
    return rs, mo, wo


def _lamb_ref(c, w, g, m, v, lr, eta, wd, gscale, step):
    w, g, m, v = w.double().cpu(), g.double().cpu() * gscale, m.double().cpu(), v.double().cpu()
    eta, wd, lr, b1, b2 = _f32(eta), _f32(wd), _f32(lr), _f32(0.9), _f32(0.98)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    dirn = (m / (1 - b1 ** step)) / ((v / (1 - b2 ** step)).sqrt() + 1e-9)
    rs, wo = [], w.clone()
    for k, (o, n) in enumerate(c.bounds()):
        tail = k == len(c.lens)
        u = dirn[o:o + n] + (0.0 if tail else wd) * w[o:o + n]
        r = 1.0 if tail else _ratio(eta, float(w[o:o + n].norm()), float(u.norm()))
        wo[o:o + n] = w[o:o + n] - lr * r * u
        if not tail:
            rs.append(r)
    return rs, m, v, wo


def _check_grad_reset(c, g_after, g_before):
    assert torch.equal(g_after[:c.zf], g_before[:c.zf])
    assert torch.count_nonzero(g_after[c.zf:]) == 0


@pytest.mark.parametrize("name", ["small", "large"])
def test_lars_against_host_reference(gpu, cases, name):
    c = cases[name]
    s = c.lars_state()
    part, ratios = c.scratch()
    _lars(c, s, part, ratios, lr=0.1, eta=0.1, wd=1e-2, gscale=0.5)
    rs, mo, wo = _lars_ref(c, c.w, c.g, torch.zeros_like(c.w), 0.1, 0.1, 1e-2, 0.5)
    got = ratios.cpu().double()
    for k, r in enumerate(rs):
        rel = abs(float(got[k, 0]) - r) / r
        print(f"{name} seg {k}: ratio {float(got[k, 0])!r} ref {r!r} rel {rel:.2e}")
        assert rel <= RATIO_BOUND
    for k, (o, n) in enumerate(c.bounds()):
        em, ew = _rel(s[2][o:o + n], mo[o:o + n]), _rel(s[0][o:o + n], wo[o:o + n])
        print(f"{name} seg {k}: mom rel {em:.2e} w rel {ew:.2e}")
        assert em < ADAM_BOUND and ew < ADAM_BOUND
    assert torch.equal(s[3], s[0].to(BF))
    _check_grad_reset(c, s[1], c.g)


@pytest.mark.parametrize("name", ["small", "large"])
def test_lamb_against_host_reference(gpu, cases, name):
    c = cases[name]
    s = c.lamb_state()
    part, ratios = c.scratch()
    _lamb(c, s, part, ratios, lr=0.05, eta=1.0, wd=0.01, step=3)
    rs, m, v, wo = _lamb_ref(c, c.w, c.g, c.m, c.v, 0.05, 1.0, 0.01, 1.0, 3)
    got = ratios.cpu().double()
    for k, r in enumerate(rs):
        rel = abs(float(got[k, 0]) - r) / r
        print(f"{name} seg {k}: ratio {float(got[k, 0])!r} ref {r!r} rel {rel:.2e}")
        assert rel < ADAM_BOUND
    for k, (o, n) in enumerate(c.bounds()):
        errs = [_rel(s[2][o:o + n], m[o:o + n]), _rel(s[3][o:o + n], v[o:o + n]), _rel(s[0][o:o + n], wo[o:o + n])]
        print(f"{name} seg {k}: m, v, w rel", ["%.2e" % e for e in errs])
        assert max(errs) < ADAM_BOUND
    assert torch.equal(s[4], s[0].to(BF))
    _check_grad_reset(c, s[1], c.g)
    # the no-decay tail: bitwise adam_step on the slice with wd = 0
    twin = [t[c.nd:].clone() for t in c.lamb_state()]
    T().adam_step(twin[0], twin[1], twin[2], twin[3], twin[4], 0.05, 0.9, 0.98, 1e-9, 0.0, 3, 1.0, True)
    for i in (0, 2, 3, 4):
        assert torch.equal(s[i][c.nd:], twin[i]), i


def test_ratio_falls_back_to_one(gpu, cases):
    c = cases["small"]
    o3, n3 = c.bounds()[3]
    o4, n4 = c.bounds()[4]
    # LARS: zero weights in segment 3, zero gradient in segment 4
    s = c.lars_state()
    s[0][o3:o3 + n3] = 0
    s[1][o4:o4 + n4] = 0
    part, ratios = c.scratch()
    _lars(c, s, part, ratios)
    r = ratios.cpu()
    assert float(r[3, 0]) == 1.0 and float(r[3, 1]) == 0.0
    assert float(r[4, 0]) == 1.0 and float(r[4, 2]) == 0.0
    assert float(r[5, 0]) != 1.0
    # LAMB: zero weights (3); zero weights, gradient and state (4)
    s = c.lamb_state()
    s[0][o3:o3 + n3] = 0
    for i in (0, 1, 2, 3):
        s[i][o4:o4 + n4] = 0
    part, ratios = c.scratch()
    _lamb(c, s, part, ratios)
    r = ratios.cpu()
    assert float(r[3, 0]) == 1.0
    assert tuple(float(x) for x in r[4]) == (1.0, 0.0, 0.0)
    for t in s[:4] + [s[4].float(), ratios]:
        assert bool(torch.isfinite(t).all())
    assert torch.count_nonzero(s[0][o4:o4 + n4]) == 0


@pytest.mark.parametrize("name", ["small", "large"])
@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_determinism_and_grid_independence(gpu, cases, name, opt):
    c = cases[name]

    def run():
        s = c.lars_state(zero_mom=False) if opt == "lars" else c.lamb_state()
        part, ratios = c.scratch()
        (_lars if opt == "lars" else _lamb)(c, s, part, ratios)
        return s + [ratios]

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    try:
        T().optim_grid(7)
        d = run()
        T().optim_grid(0)
        T().optim_variant(0)       # (the tail's plain step honours it; the tiled passes have one form)
        e = run()
    finally:
        T().optim_grid(0)
        T().optim_variant(-1)
    for x, y, z in zip(a, d, e):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("how", ["clip", "guard"])
@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_skipped_step_writes_nothing(gpu, cases, opt, how):
    c = cases["small"]
    step = _lars if opt == "lars" else _lamb
    s = c.lars_state(zero_mom=False) if opt == "lars" else c.lamb_state()
    before = [t.clone() for t in s]
    part, ratios = c.scratch()
    clip = torch.tensor([-1.0 if how == "clip" else 1.0, 0.0, 0.0, 0.0], device=gpu)
    guard = torch.tensor([1 if how == "guard" else 0, 0], dtype=torch.int32, device=gpu)
    step(c, s, part, ratios, guard=guard, clip=clip)
    for i in [0] + list(range(2, len(s))):
        assert torch.equal(s[i], before[i]), i
    assert bool((ratios == 7.0).all())
    _check_grad_reset(c, s[1], before[1])
    # a clean step afterwards: bitwise a twin that never skipped
    s[1].copy_(before[1])
    twin = [t.clone() for t in before]
    clip[0] = 1.0
    guard.zero_()
    step(c, s, part, ratios, guard=guard, clip=clip)
    part2, ratios2 = c.scratch()
    step(c, twin, part2, ratios2)
    for x, y in zip(s + [ratios], twin + [ratios2]):
        assert torch.equal(x, y)
    assert not torch.equal(s[0], before[0])


@pytest.mark.parametrize("opt", ["lars", "lamb"])
def test_clip_scale_is_folded_into_gscale(gpu, cases, opt):
    c = cases["small"]
    step = _lars if opt == "lars" else _lamb
    a = c.lars_state(zero_mom=False) if opt == "lars" else c.lamb_state()
    b = [t.clone() for t in a]
    pa, ra = c.scratch()
    pb, rb = c.scratch()
    step(c, a, pa, ra, gscale=0.5, clip=torch.tensor([0.37, 0.0, 0.0, 0.0], device=gpu))
    step(c, b, pb, rb, gscale=float(np.float32(0.5) * np.float32(0.37)))
    for x, y in zip(a + [ra], b + [rb]):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], c.w)


def test_binding_checks(gpu, cases):
    c = cases["small"]
    s = c.lars_state()
    part, ratios = c.scratch()

    def lars(tiles=c.tiles, first=c.first, part=part, ratios=ratios, eta=0.1, wu=c.nd):
        T().lars_step(s[0], s[1], s[2], s[3], 0.1, 0.9, 1e-2, eta, 1.0, tiles, first, part, ratios, None, c.zf, wu,
                      None)

    with pytest.raises(RuntimeError):
        lars(tiles=c.tiles.cpu())
    with pytest.raises(RuntimeError):
        lars(first=c.first.cpu())
    with pytest.raises(RuntimeError, match="int32"):
        lars(tiles=c.tiles.long())
    with pytest.raises(RuntimeError, match="ratios"):
        lars(ratios=torch.zeros(c.ns * 3 - 1, device=gpu))
    with pytest.raises(RuntimeError, match="partials"):
        lars(part=torch.zeros(2 * c.nt - 1, dtype=torch.float64, device=gpu))
    for eta in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="eta"):
            lars(eta=eta)
    with pytest.raises(RuntimeError, match="tile boundary"):
        lars(wu=c.nd + 32)
    m = c.lamb_state()
    with pytest.raises(RuntimeError, match="eta"):
        T().lamb_step(m[0], m[1], m[2], m[3], m[4], 0.05, 0.9, 0.98, 1e-9, 0.01, 3, 0.0, 1.0, c.tiles, c.first, part,
                      ratios, None, c.zf, c.nd, None)
    with pytest.raises(RuntimeError, match="int32"):
        T().lamb_step(m[0], m[1], m[2], m[3], m[4], 0.05, 0.9, 0.98, 1e-9, 0.01, 3, 1.0, 1.0, c.tiles.float(),
                      c.first, part, ratios, None, c.zf, c.nd, None)
    # nothing was launched
    assert torch.equal(s[0], c.w) and torch.equal(m[0], c.w)


def _host_step(t, g, w0, st0, scale):
    """The contract per parameter in fp64 -> ({name: ratio}, new master)."""
    A = t.arena
    eta, wd, lr, k = t.trust_ratio, t.spec.wd, t.lr, t.step_count
    g = g.double().cpu() * scale
    w0 = w0.double().cpu()
    st0 = [x.double().cpu() for x in st0]
    wn = w0.clone()
    if t.opt == "adam":
        m = 0.9 * st0[0] + 0.1 * g
        v = 0.98 * st0[1] + 0.02 * g * g
        dirn = (m / (1 - 0.9 ** k)) / ((v / (1 - 0.98 ** k)).sqrt() + 1e-9)
    ratios = {}
    for p in A.params:
        sl = slice(p.offset, p.offset + p.numel)
        if t.opt == "sgd":
            r = _ratio(eta, float(w0[sl].norm()), float(g[sl].norm()), wd) if p.decay else 1.0
            mom = 0.9 * st0[0][sl] + r * (g[sl] + (wd if p.decay else 0.0) * w0[sl])
            wn[sl] = w0[sl] - lr * mom
        else:
            u = dirn[sl] + (wd if p.decay else 0.0) * w0[sl]
            r = _ratio(eta, float(w0[sl].norm()), float(u.norm())) if p.decay else 1.0
            wn[sl] = w0[sl] - lr * r * u
        if p.decay:
            ratios[p.name] = r
    return ratios, wn


@pytest.mark.parametrize("model,eta", [("resnet_tiny", 0.02), ("transformer_tiny", 1.0)])
def test_trainer_under_graph_replay(gpu, model, eta):
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer(model, gpu, seed=0, use_graph=True, trust_ratio=eta)
    A = t.arena
    assert t.trust_ratios() == {}
    for _ in range(3):           # two eager warm steps, then capture + first replay
        t.step()
    assert t._graph is not None
    bound = RATIO_BOUND if t.opt == "sgd" else ADAM_BOUND

    def fwd_bwd():
        """One replayed forward+backward; the gradient the optimizer will see."""
        t._graph_step()
        for p in A.params:
            if p.store_grad and p.gw_epoch != A.grad_epoch:
                p.grad.zero_()
        g = A.grad.clone()
        return g, float(g.double().norm())

    def check(scale):
        w0, st0 = A.master.clone(), [x.clone() for x in t.opt_state]
        t._opt_step()
        torch.cuda.synchronize()
        if scale is None:
            scale = t.clip_stats()["last_scale"]
            assert 0.0 < scale < 1.0
        want, w_ref = _host_step(t, g, w0, st0, scale)
        got = t.trust_ratios()
        assert set(got) == set(want)
        worst = max(abs(got[k][0] - want[k]) / want[k] for k in want)
        print(model, "worst ratio rel err", worst, "ratios", min(want.values()), "..", max(want.values()))
        assert worst <= bound
        for p in A.params:
            sl = slice(p.offset, p.offset + p.numel)
            if float(w_ref[sl].norm()) == 0.0:        # (a parameter that has not moved from a zero init)
                assert torch.count_nonzero(A.master[sl]) == 0, p.name
            else:
                assert _rel(A.master[sl], w_ref[sl]) < ADAM_BOUND, p.name
        assert torch.equal(A.shadow, A.master.to(BF))

    g, ref = fwd_bwd()
    check(1.0)
    g, ref = fwd_bwd()
    t.set_grad_clip(0.5 * ref)
    check(None)
    t.reset(1)
    assert t.trust_ratios() == {} and t.trust_ratio == eta
    t.release()


def test_knob_off_is_the_plain_step(gpu):
    from tiresias_amd.executor.trainer import Trainer
    from tiresias_amd.ops import functional as Fx

    t = Trainer("transformer_tiny", gpu, seed=0)
    A = t.arena
    assert t.trust_ratio is None and t._tr is None
    t.step()
    t._fwd_bwd()
    for p in A.params:
        if p.store_grad and p.gw_epoch != A.grad_epoch:
            p.grad.zero_()
    twin = [A.master.clone(), A.grad.clone(), t.opt_state[0].clone(), t.opt_state[1].clone(), A.shadow.clone()]
    t._opt_step()
    zf = A.n_store if Fx.STORE_GRAD else 0
    T().adam_step(twin[0], twin[1], twin[2], twin[3], twin[4], t.lr, 0.9, 0.98, 1e-9, t.spec.wd, t.step_count, 1.0,
                  True, None, zf, A.n_decay)
    for x, y in zip([A.master, A.grad, t.opt_state[0], t.opt_state[1], A.shadow], twin):
        assert torch.equal(x, y)
    assert t.trust_ratios() == {} and t._tr is None
    t.release()
