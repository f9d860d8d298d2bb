"""GroupNorm kernels (csrc/kernels/group_norm.hip) against a float64 torch
reference, on both routes; sample independence; resnet_tiny with norm="group"
against the CPU fp32 path of the same ops."""
import math

import pytest
import torch
import torch.nn.functional as F

from tiresias_amd.executor.trainer import Trainer

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
TILED, RESIDENT = 1, 2

SHAPES = [(2, 3, 3, 8, 4),      # Cg = 2: four groups inside one vector; odd pixel count
          (2, 3, 3, 16, 4),     # Cg = 4
          (3, 5, 5, 32, 4),     # Cg = 8
          (2, 5, 5, 64, 2),     # Cg = 32: lane fold
          (2, 5, 5, 512, 2),    # Cg = 256: widest fold, slab wider than 64
          (3, 7, 11, 64, 32),   # pixel count that is no multiple of the tile
          (1, 1, 1, 64, 32)]    # one pixel: variance from two values


def T():
    return torch.ops.tam


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


def _route(route, P, C, G):
    for bwd in (False, True):
        if route == RESIDENT and not T().gn_resident_fits(P, C, G, bwd):
            pytest.skip("the resident tile does not fit this device's LDS")
    T().gn_policy(route)


def _run(x, r, g, b, G, relu, dy):
    N, C = x.shape[0], x.shape[-1]
    y, dx = torch.empty_like(x), torch.empty_like(x)
    mean = torch.empty(N * G, device=x.device)
    rstd = torch.empty_like(mean)
    T().groupnorm_forward(x, r, y, g, b, mean, rstd, G, 1e-5, relu)
    dres = torch.empty_like(x) if r is not None else None
    dg, db = torch.zeros(C, device=x.device), torch.zeros(C, device=x.device)
    tiles = (x.numel() // (N * C) + 255) // 256
    cpart = torch.empty(N * tiles * 2 * C, device=x.device)
    T().groupnorm_backward(dy, y if relu else None, x, mean, rstd, g, dx, dres, cpart, dg, db, G, relu)
    return y, dx, dres, dg, db


@pytest.mark.parametrize("route", [TILED, RESIDENT], ids=["tiled", "resident"])
@pytest.mark.parametrize("relu,res", [(False, False), (True, True)])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_groupnorm_op(gpu, shape, relu, res, route):
    """Forward and backward vs F.group_norm in float64 on the bf16 inputs;
    tolerances: test_kernels_gpu.py test_batchnorm's."""
    N, H, W, C, G = shape
    _route(route, H * W, C, G)
    torch.manual_seed(5)
    x = (torch.randn(N, H, W, C, device=gpu) + 3).to(BF)
    r = torch.randn(N, H, W, C, device=gpu).to(BF) if res else None
    g = torch.rand(C, device=gpu) + 0.5
    b = torch.randn(C, device=gpu)
    dy = torch.randn(N, H, W, C, device=gpu).to(BF)
    y, dx, dres, dg, db = _run(x, r, g, b, G, relu, dy)
    xf = x.double().requires_grad_(True)
    gf, bf = g.double().requires_grad_(True), b.double().requires_grad_(True)
    yf = F.group_norm(xf.permute(0, 3, 1, 2), G, gf, bf, 1e-5).permute(0, 2, 3, 1)
    rf = None
    if res:
        rf = r.double().requires_grad_(True)
        yf = yf + rf
    if relu:
        yf = yf.clamp_min(0)
    grads = torch.autograd.grad(yf, [xf, gf, bf] + ([rf] if res else []), dy.double())
    errs = {"y": rel_err(y, yf), "dx": rel_err(dx, grads[0]), "dgamma": rel_err(dg, grads[1]),
            "dbeta": rel_err(db, grads[2])}
    if res:
        errs["dres"] = rel_err(dres, grads[3])
    print(shape, relu, res, route, errs)
    assert errs["y"] < 1e-2
    assert errs["dx"] < 2e-2
    assert errs["dgamma"] < 1e-2 and errs["dbeta"] < 1e-2
    assert errs.get("dres", 0.0) < 1e-2


@pytest.mark.parametrize("route", [TILED, RESIDENT], ids=["tiled", "resident"])
def test_sample_independence(gpu, route):
    """A sample's y and dx do not depend on its batch-mates: bitwise."""
    N, H, W, C, G = 3, 7, 11, 64, 32
    _route(route, H * W, C, G)
    torch.manual_seed(6)
    x = (torch.randn(N, H, W, C, device=gpu) + 3).to(BF)
    r = torch.randn(N, H, W, C, device=gpu).to(BF)
    g, b = torch.rand(C, device=gpu) + 0.5, torch.randn(C, device=gpu)
    dy = torch.randn(N, H, W, C, device=gpu).to(BF)
    y, dx = _run(x, r, g, b, G, True, dy)[:2]
    for n in range(N):
        y1, dx1 = _run(x[n:n + 1].contiguous(), r[n:n + 1].contiguous(), g, b, G, True, dy[n:n + 1].contiguous())[:2]
        assert torch.equal(y1[0], y[n]) and torch.equal(dx1[0], dx[n])


def test_rejects_unsupported_shapes(gpu):
    x = torch.zeros(2, 3, 3, 24, device=gpu, dtype=BF)
    v = torch.zeros(24, device=gpu)
    for G in (24, 2, 5):                   # Cg = 1, Cg = 12, groups not dividing C
        with pytest.raises(RuntimeError):
            T().groupnorm_forward(x, None, torch.empty_like(x), v, v, torch.zeros(2 * G, device=gpu),
                                  torch.zeros(2 * G, device=gpu), G, 1e-5, False)


def test_resnet_tiny_group(gpu):
    """One training step of resnet_tiny with norm="group" vs the CPU fp32 path
    (test_models_gpu.py's comparison), then graph replay against eager."""
    tg = Trainer("resnet_tiny", gpu, seed=3, norm="group")
    tc = Trainer("resnet_tiny", "cpu", seed=3, norm="group")
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
    a = Trainer("resnet_tiny", gpu, seed=5, use_graph=True, norm="group")
    e = Trainer("resnet_tiny", gpu, seed=5, use_graph=False, norm="group")
    la = [float(a.step()) for _ in range(4)]       # two eager warm-up steps, then two replays
    le = [float(e.step()) for _ in range(4)]
    assert a._graph is not None and all(math.isfinite(v) for v in la)
    assert la[3] <= la[2]
    for i in (2, 3):
        assert abs(la[i] - le[i]) < 1e-2 * max(1.0, abs(le[i]))
