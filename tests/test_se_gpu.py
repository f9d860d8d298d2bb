"""Squeeze-and-Excitation kernels (csrc/kernels/se.hip) against a float64
torch reference, on both squeeze routes; sample independence; resnet_tiny with
se_ratio=16 against the CPU fp32 path of the same ops."""
import math

import pytest
import torch

from tiresias_amd.executor.trainer import Trainer

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TILED, SINGLE = 1, 2
ROUTES = pytest.mark.parametrize("route", [TILED, SINGLE], ids=["tiled", "single"])

# (N, H, W, C, r), addend, idn
CASES = [((1, 1, 1, 64, 8), False, True),      # one pixel, Cr = 8: under an MFMA tile in both dimensions
         ((3, 7, 7, 64, 16), True, True),      # Cr floor of 8, odd pixel count, N < 16
         ((17, 3, 5, 128, 4), False, False),   # Cr = 32, N one over a 16-sample tile; no identity branch
         ((2, 17, 19, 256, 16), True, True),   # 323 pixels: two 256-pixel tiles, the second ragged
         ((2, 5, 5, 2048, 4), False, True),    # Cr = 512, the widest of both
         ((33, 2, 2, 512, 32), True, True)]    # Cr = 16, three sample tiles


def T():
    return torch.ops.tam


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


def _forward(u, idn, w1, b1, w2, b2):
    N, C, Cr = u.shape[0], u.shape[-1], w1.shape[0]
    z, s = torch.empty(N, C, device=u.device), torch.empty(N, C, device=u.device)
    h, y = torch.empty(N, Cr, device=u.device), torch.empty_like(u)
    T().se_squeeze(u, z)
    T().se_excite_fwd(z, w1, b1, w2, b2, h, s)
    T().se_gate_fwd(u, s, idn, y)
    return z, h, s, y


def _backward(dy, add, u, w1, w2, z, h, s, y):
    g, du = torch.empty_like(u), torch.empty_like(u)
    ds, dz = torch.empty_like(s), torch.empty_like(s)
    grads = [torch.full(sh, 0.5, device=u.device)              # pre-filled: the kernels accumulate
             for sh in (tuple(w1.shape), (w1.shape[0],), tuple(w2.shape), (w2.shape[0],))]
    T().se_gate_bwd_reduce(dy, add, y, u, g, ds)
    T().se_excite_bwd(ds, s, h, z, w1, w2, *grads, dz)
    T().se_gate_bwd_apply(g, s, dz, du)
    return [du, g] + grads


def _inputs(shape, gpu, seed=7):
    N, H, W, C, r = shape
    Cr = max(8, C // r)
    torch.manual_seed(seed)
    u, idn, dy, add = (torch.randn(N, H, W, C, device=gpu).to(BF) for _ in range(4))
    w1 = (torch.randn(Cr, C, device=gpu) / math.sqrt(C)).to(BF)
    w2 = (torch.randn(C, Cr, device=gpu) / math.sqrt(Cr)).to(BF)
    b1, b2 = (0.5 * torch.randn(Cr, device=gpu)).to(BF), (0.5 * torch.randn(C, device=gpu)).to(BF)
    return u, idn, dy, add, w1, b1, w2, b2


@ROUTES
@pytest.mark.parametrize("shape,addend,has_idn", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_se_block_op(gpu, shape, addend, has_idn, route):
    """The six kernels vs the block's formulas in float64 autograd on the bf16
    inputs and bf16-rounded weights; tolerances: test_groupnorm_gpu.py's."""
    T().se_policy(route)
    u, idn, dy, add, w1, b1, w2, b2 = _inputs(shape, gpu)
    uf, f1, c1, f2, c2 = (t.double().requires_grad_(True) for t in (u, w1, b1, w2, b2))
    zf = uf.mean((1, 2))
    sf = torch.sigmoid((zf @ f1.t() + c1).clamp_min(0) @ f2.t() + c2)
    # y's pre-activation stays 1/16 away from the ReLU kink: an s within its own
    # bound (1e-2 of s <= 1, |u| < 6) moves it by less, so no element's backward
    # mask can flip; one flipped element is percents of a norm at these sizes
    pre = (sf[:, None, None, :] * uf + idn.double()).detach()
    idn = torch.where(pre.abs() < 1 / 16, idn + torch.where(pre < 0, -1, 1).to(BF), idn)
    idn, add = (idn if has_idn else None), (add if addend else None)
    z, h, s, y = _forward(u, idn, w1, b1, w2, b2)
    out = _backward(dy, add, u, w1, w2, z, h, s, y)
    again = _backward(dy, add, u, w1, w2, *_forward(u, idn, w1, b1, w2, b2))
    idf = idn.double().requires_grad_(True) if has_idn else None
    yf = sf[:, None, None, :] * uf
    yf = (yf + idf if has_idn else yf).clamp_min(0)
    up = dy.double() + (add.double() if addend else 0)
    ref = torch.autograd.grad(yf, [uf] + ([idf] if has_idn else []) + [f1, c1, f2, c2], up)
    names = ["du"] + (["didn"] if has_idn else []) + ["dW1", "db1", "dW2", "db2"]
    got = [out[0]] + ([out[1]] if has_idn else []) + [t - 0.5 for t in out[2:]]
    errs = {"z": rel_err(z, zf), "s": rel_err(s, sf), "y": rel_err(y, yf)}
    errs.update({k: rel_err(a, b) for k, a, b in zip(names, got, ref)})
    print(shape, route, errs)
    assert errs["du"] < 2e-2
    assert all(v < 1e-2 for k, v in errs.items() if k != "du"), errs
    assert all(torch.equal(a, b) for a, b in zip(out, again))       # no atomics: two runs, equal bits


@ROUTES
def test_sample_independence(gpu, route):
    """A sample's z, s and y do not depend on its batch-mates: bitwise."""
    T().se_policy(route)
    u, idn, _, _, w1, b1, w2, b2 = _inputs((3, 7, 11, 64, 16), gpu, seed=6)
    z, _, s, y = _forward(u, idn, w1, b1, w2, b2)
    for n in range(u.shape[0]):
        z1, _, s1, y1 = _forward(u[n:n + 1].contiguous(), idn[n:n + 1].contiguous(), w1, b1, w2, b2)
        assert torch.equal(z1[0], z[n]) and torch.equal(s1[0], s[n]) and torch.equal(y1[0], y[n])


@pytest.mark.parametrize("C,Cr", [(24, 12), (4096, 256), (64, 4)], ids=["Cr12", "C4096", "Cr4"])
def test_rejects_unsupported_shapes(gpu, C, Cr):
    u = torch.zeros(2, 3, 3, C, device=gpu, dtype=BF)
    z, h = torch.zeros(2, C, device=gpu), torch.zeros(2, Cr, device=gpu)
    w1, w2 = torch.zeros(Cr, C, device=gpu, dtype=BF), torch.zeros(C, Cr, device=gpu, dtype=BF)
    with pytest.raises(RuntimeError):
        T().se_excite_fwd(z, w1, w1[:, 0].contiguous(), w2, w2[:, 0].contiguous(), h, torch.empty_like(z))
    with pytest.raises(RuntimeError):
        T().se_excite_bwd(z, z, h, z, w1, w2, torch.zeros(Cr, C, device=gpu), torch.zeros(Cr, device=gpu),
                          torch.zeros(C, Cr, device=gpu), torch.zeros(C, device=gpu), torch.empty_like(z))
    if C > 2048:
        for op in (lambda: T().se_squeeze(u, z), lambda: T().se_gate_fwd(u, z, None, torch.empty_like(u)),
                   lambda: T().se_gate_bwd_apply(u, z, z, torch.empty_like(u))):
            with pytest.raises(RuntimeError):
                op()


@pytest.mark.parametrize("norm,cardinality", [("batch", None), ("group", 4)])
def test_resnet_tiny_se(gpu, norm, cardinality):
    """One training step of resnet_tiny with se_ratio=16 vs the CPU fp32 path
    (test_grouped_conv_gpu.py test_resnet_tiny_cardinality's comparison), then
    graph replay against eager."""
    kw = dict(se_ratio=16, norm=norm, cardinality=cardinality)
    tg = Trainer("resnet_tiny", gpu, seed=3, **kw)
    tc = Trainer("resnet_tiny", "cpu", seed=3, **kw)
    tc.arena.master.copy_(tg.arena.master.cpu())
    tc.arena.shadow.copy_(tg.arena.shadow.cpu())
    tc.data = {k: v.cpu() for k, v in tg.data.items()}
    lg, lc = tg._fwd_bwd(), tc._fwd_bwd()
    assert abs(float(lg) - float(lc)) < 0.02 * max(1.0, abs(float(lc)))
    gg, gc = tg.arena.grad.cpu(), tc.arena.grad
    assert rel_err(gg, gc) < 0.05
    floor = 1e-4 * float(gc.norm())
    worst = max((rel_err(gg[p.offset:p.offset + p.numel], gc[p.offset:p.offset + p.numel]), p.name)
                for p in tg.arena.params if float(gc[p.offset:p.offset + p.numel].norm()) > floor)
    assert worst[0] < 0.1, f"worst parameter {worst[1]} rel err {worst[0]}"
    a = Trainer("resnet_tiny", gpu, seed=5, use_graph=True, **kw)
    e = Trainer("resnet_tiny", gpu, seed=5, use_graph=False, **kw)
    la = [float(a.step()) for _ in range(4)]       # two eager warm-up steps, then two replays
    le = [float(e.step()) for _ in range(4)]
    assert a._graph is not None and all(math.isfinite(v) for v in la)
    assert la[3] <= la[2]
    for i in (2, 3):
        assert abs(la[i] - le[i]) < 1e-2 * max(1.0, abs(le[i]))
