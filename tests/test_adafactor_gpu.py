"""Adafactor on the device (csrc/kernels/adafactor.hip) against an fp64 host
reference; bound: rel_err < 1e-5 per parameter (test_trust_ratio_gpu.py's
ADAM_BOUND). Inputs: from zero state a 1 x n parameter has u = sign(g), so its
gradient is 1/16 dense (RMS 0.25, clip off); a matrix gets diagonal blocks of
amplitude 100 and 1 over 1e-3, which no rank-one Rv x Cv fits (RMS >> 2, clip
on). At step 3 every other parameter starts from a 1e6 state (RMS << 0.5)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
ADAM_BOUND, LR = 1e-5, 0.05
ZF = 64                         # inside the decay region: the gradient below it is left alone
PACKS = {"edges": ([(2, 4), (33, 260), (5, 6)], [(70,)]), "multi": ([(70, 516), (64, 64)], [(300,)])}
MODES = {"first": dict(step=1, gscale=1.0, wd=0.01), "third": dict(step=3, gscale=0.5, wd=0.01)}


T = lambda: torch.ops.tam   # noqa: E731


class Pack:
    """A synthetic arena laid out as ops/arena.py lays one out, with its tables."""

    def __init__(self, name, tile=(32, 256)):
        from tiresias_amd.ops.arena import _padded, adafactor_tables, factored_shape

        decay, tail = PACKS[name]
        self.shapes = decay + tail
        self.rc = [factored_shape(s) for s in self.shapes]
        lens = [_padded(r * c) for r, c in self.rc]
        self.offs = [sum(lens[:k]) for k in range(len(lens))]
        self.nd, self.n = sum(lens[:len(decay)]), sum(lens)
        self.params, self.tiles, self.tasks, self.nstate, self.npart = adafactor_tables(
            list(zip(self.offs, self.shapes)), *tile)
        self.soffs = self.params[:, 3].tolist()
        gen = torch.Generator().manual_seed(5)
        self.w, self.g, self.state = torch.zeros(self.n), torch.zeros(self.n), torch.zeros(self.nstate)
        for k, (o, (r, c)) in enumerate(zip(self.offs, self.rc)):
            self.w[o:o + r * c] = torch.randn(r * c, generator=gen)
            g = torch.randn(r, c, generator=gen)
            if r == 1:
                g *= (torch.arange(c) % 16 == 0)
            else:
                top, left = torch.arange(r)[:, None] < r // 2, torch.arange(c)[None, :] < c // 2
                g *= torch.where(top & left, 100.0, torch.where(~top & ~left, 1.0, 1e-3))
            self.g[o:o + r * c] = g.reshape(-1)
            so = self.soffs[k]
            self.state[so:so + r + c] = (0.5 + torch.rand(r + c, generator=gen)) * (1e6 if k % 2 else 1e-6)

    def ref(self, step, gscale, wd):
        b2 = 1.0 - float(step) ** -0.8
        f32 = lambda x: float(np.float32(x))   # noqa: E731
        st = (self.state.double() if step > 1 else torch.zeros(self.nstate, dtype=torch.float64))
        w, rec = self.w.double().clone(), []
        for k, (o, (r, c)) in enumerate(zip(self.offs, self.rc)):
            g = self.g[o:o + r * c].double().view(r, c) * f32(gscale)
            so = self.soffs[k]
            rv, cv = st[so:so + r], st[so + r:so + r + c]
            rv.mul_(f32(b2)).add_((1 - f32(b2)) * (g * g + 1e-30).mean(1))
            cv.mul_(f32(b2)).add_((1 - f32(b2)) * (g * g + 1e-30).mean(0))
            u = g * (rv / rv.mean()).rsqrt()[:, None] * cv.rsqrt()[None, :]
            rms = float(u.pow(2).mean().sqrt())
            s = 1.0 / max(1.0, rms)
            wk = w[o:o + r * c].view(r, c)
            wk.sub_(f32(LR) * (s * u + (f32(wd) if o < self.nd else 0.0) * wk))
            rec.append((rms, s))
        return st, w, rec

    def run(self, gpu, step, gscale, wd, guard=None, clip=None):
        d = dict(w=self.w.to(gpu), g=self.g.to(gpu), wb=self.w.to(gpu).to(BF),
                 state=self.state.to(gpu) if step > 1 else torch.zeros(self.nstate, device=gpu),
                 fac=torch.zeros(self.nstate, device=gpu), urms=torch.full((len(self.rc), 2), 7.0, device=gpu))
        T().adafactor_step(d["w"], d["g"], d["state"], d["fac"], d["wb"], LR, wd, step, gscale, self.params.to(gpu),
                           self.tiles.to(gpu), self.tasks.to(gpu), torch.full((self.npart,), 1e30, device=gpu),
                           torch.full((self.tiles.shape[0],), 1e300, dtype=torch.float64, device=gpu), d["urms"],
                           guard, ZF, self.nd, clip)
        torch.cuda.synchronize()
        return d


@pytest.fixture(scope="module")
def packs():
    return {k: Pack(k) for k in PACKS}


def _rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(PACKS))
def test_against_fp64_reference(gpu, packs, name, mode):
    c, kw = packs[name], MODES[mode]
    st, w, rec = c.ref(**kw)
    assert all(not 0.5 <= rms <= 2.0 for rms, _ in rec), rec     # no parameter sits near the clip's corner
    assert max(rec)[0] > 2.0 and min(rec)[0] < 0.5, rec            # the clip engages for one and not for another
    d = c.run(gpu, **kw)
    for k, (o, (r, cc)) in enumerate(zip(c.offs, c.rc)):
        so, sl = c.soffs[k], slice(o, o + r * cc)
        cv = slice(so + r, so + r + cc)
        errs = (_rel(d["state"][so:so + r], st[so:so + r]), _rel(d["state"][cv], st[cv]),
                _rel(d["w"][sl], w[sl]), _rel(d["urms"][k], torch.tensor(rec[k])))
        print(name, mode, c.shapes[k], "rms", rec[k][0], "rel err Rv Cv w rec", errs)
        assert max(errs) < ADAM_BOUND, (c.shapes[k], errs)
    assert torch.equal(d["wb"], d["w"].to(BF))
    assert torch.equal(d["g"][:ZF].cpu(), c.g[:ZF]) and torch.count_nonzero(d["g"][ZF:]) == 0


def test_bitwise_across_runs_and_grids(gpu, packs):
    c, kw = packs["multi"], MODES["third"]
    a, b = c.run(gpu, **kw), c.run(gpu, **kw)
    try:
        T().optim_grid(3)
        e = c.run(gpu, **kw)
        T().optim_grid(1)
        f = c.run(gpu, **kw)
    finally:
        T().optim_grid(0)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], e[k]) and torch.equal(a[k], f[k]), k


@pytest.mark.parametrize("how", ["guard", "clip"])
def test_skipped_step_only_resets_the_gradient(gpu, packs, how):
    c = packs["edges"]
    guard = torch.tensor([1, 0], dtype=torch.int32, device=gpu) if how == "guard" else None
    clip = torch.tensor([-1.0, 0.0, 0.0, 0.0], device=gpu) if how == "clip" else None
    d = c.run(gpu, guard=guard, clip=clip, **MODES["third"])
    assert torch.equal(d["w"].cpu(), c.w) and torch.equal(d["state"].cpu(), c.state)
    assert torch.equal(d["wb"].cpu(), c.w.to(BF)) and float(d["urms"].min()) == 7.0 and not d["fac"].any()
    assert torch.equal(d["g"][:ZF].cpu(), c.g[:ZF]) and torch.count_nonzero(d["g"][ZF:]) == 0


@pytest.mark.parametrize("model", ["transformer_tiny", "gnmt_tiny"])
def test_trainer_graph_replay_equals_eager(gpu, model):
    """transformer_tiny's embedding gradient uses float atomics (test_opt_dtype_gpu.py
    MODELS_7): two instances differ in 1-5 of 116736 master elements, eager against
    eager too. There the losses and the replayed step on ITS gradient are compared
    bitwise; every buffer is compared on gnmt_tiny, whose backward is reproducible."""
    from tiresias_amd.executor.trainer import Trainer
    from tiresias_amd.ops import functional as Fx
    from tiresias_amd.ops.arena import factored_state_numel

    out = {}
    for graph in (True, False):
        t = Trainer(model, gpu, seed=0, use_graph=graph, opt_dtype="factored")
        losses = [float(t.step()) for _ in range(4)]           # two eager warm steps, capture + replay, replay
        torch.cuda.synchronize()
        assert (t._graph is not None) == graph
        out[graph] = (t, losses, [t.arena.master.clone(), t.opt_state[0].clone(), t.arena.shadow.clone()])
        assert len(t.opt_state) == 1 and t.opt_state[0].dtype == torch.float32
        assert t.opt_state[0].numel() == factored_state_numel([p.shape for p in t.arena.params])
        assert set(t.update_rms()) == {p.name for p in t.arena.params}
    assert out[True][1] == out[False][1]
    ne = [int((x != y).sum()) for x, y in zip(out[True][2], out[False][2])]
    if model == "gnmt_tiny":
        assert ne == [0, 0, 0]
    # a fifth, replayed step against the eager kernel on a twin of its inputs
    t, A = out[True][0], out[True][0].arena
    t._graph_step()
    for p in A.params:
        if p.store_grad and p.gw_epoch != A.grad_epoch:
            p.grad.zero_()
    twin = [A.master.clone(), A.grad.clone(), t.opt_state[0].clone(), A.shadow.clone()]
    t._opt_step()
    params, tiles, tasks, fac, part, slots, urms = t._af
    T().adafactor_step(twin[0], twin[1], twin[2], torch.zeros_like(fac), twin[3], t.lr, t.spec.wd, t.step_count, 1.0,
                       params, tiles, tasks, torch.zeros_like(part), torch.zeros_like(slots), torch.zeros_like(urms),
                       t.model.err if t.uses_persist else None, A.n_store if Fx.STORE_GRAD else 0, A.n_decay, None)
    for x, y in zip([A.master, A.grad, t.opt_state[0], A.shadow], twin):
        assert torch.equal(x, y)
    t.release()


_Gang = type("_Gang", (), {"size": 2, "ranks": (0, 1)})     # a 2-member gang comm (parallel/gang.py comm_size)


@pytest.mark.parametrize("model,kw", [("resnet_tiny", {}), ("transformer_tiny", {"trust_ratio": 1.0}),
                                      ("transformer_tiny", {"ddp_shard": True, "group": _Gang()})])
def test_trainer_rejections(gpu, model, kw):
    from tiresias_amd.executor.trainer import Trainer

    with pytest.raises(ValueError, match="factored"):
        Trainer(model, gpu, seed=0, opt_dtype="factored", **kw)
