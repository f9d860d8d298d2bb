"""Grouped 3x3 conv kernels (csrc/kernels/conv_grouped.hip) against
F.conv2d(groups=) in float64 on the bf16 inputs; resnet_tiny with
cardinality=4 against the CPU fp32 path of the same ops."""
import math

import pytest
import torch
import torch.nn.functional as F

from tiresias_amd.executor.trainer import Trainer

pytestmark = pytest.mark.gpu
BF = torch.bfloat16

# (N, H, W, C, Cg, stride)
SHAPES = [(1, 5, 5, 16, 4, 1),       # one slab, four groups in it, image smaller than a tile
          (2, 7, 9, 64, 8, 1),       # a full chunk, two groups per slab
          (2, 9, 7, 32, 16, 2),      # half chunk, stride 2 on odd sizes: all four parity classes ragged
          (1, 8, 8, 64, 32, 2),      # Wd = 32, stride 2 on even sizes
          (3, 6, 6, 48, 16, 1),      # ragged chunk
          (2, 13, 11, 128, 4, 1),    # two chunks, two 8-row spatial tiles
          (130, 9, 3, 16, 8, 1)]     # 260 tiles on 256 persistent wgrad blocks: a block sums over tiles


def T():
    return torch.ops.tam


def rel_err(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-12)).item()


def _inputs(shape, gpu):
    N, H, W, C, Cg, s = shape
    torch.manual_seed(7)
    x = torch.randn(N, H, W, C, device=gpu).to(BF)
    w = (torch.randn(C, 3, 3, Cg, device=gpu) / math.sqrt(9 * Cg)).to(BF)
    dy = torch.randn(N, (H - 1) // s + 1, (W - 1) // s + 1, C, device=gpu).to(BF)
    img = torch.empty(T().gconv_image_elems(C, Cg), dtype=BF, device=gpu)
    T().gconv_pack([w], [img])
    return x, w, dy, img


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grouped_conv_op(gpu, shape):
    """Forward, data gradient (plain and x > 0 masked) and weight gradient;
    tolerances: test_kernels_gpu.py test_conv_fwd_dgrad_wgrad's."""
    N, H, W, C, Cg, s = shape
    x, w, dy, img = _inputs(shape, gpu)
    y, dx, dxm = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(x)
    dw = torch.full((C, 3, 3, Cg), 0.5, device=gpu)          # pre-filled: the kernel accumulates
    T().gconv_fwd(x, w, img, y, s)
    T().gconv_dgrad(dy, w, img, dx, s)
    T().gconv_dgrad(dy, w, img, dxm, s, x)
    T().gconv_wgrad(dy, x, dw, s)
    dw2 = torch.full_like(dw, 0.5)
    T().gconv_wgrad(dy, x, dw2, s)
    xf = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    wf = w.double().permute(0, 3, 1, 2).requires_grad_(True)
    yf = F.conv2d(xf, wf, stride=s, padding=1, groups=C // Cg)
    gx, gw = torch.autograd.grad(yf, [xf, wf], dy.double().permute(0, 3, 1, 2))
    gx, gw = gx.permute(0, 2, 3, 1), gw.permute(0, 2, 3, 1)
    errs = {"y": rel_err(y, yf.permute(0, 2, 3, 1)), "dx": rel_err(dx, gx),
            "dx_masked": rel_err(dxm, gx * (x > 0)), "dw": rel_err(dw - 0.5, gw)}
    print(shape, errs)
    assert errs["y"] < 1e-2 and errs["dx"] < 1e-2 and errs["dx_masked"] < 1e-2
    assert errs["dw"] < 1e-4
    assert torch.equal(dw, dw2)                              # no atomics: two runs, equal bits


@pytest.mark.parametrize("C,w_shape,stride", [(16, (16, 3, 3, 2), 1), (64, (64, 3, 3, 64), 1), (24, (24, 3, 3, 4), 1),
                                              (16, (16, 5, 5, 4), 1), (16, (16, 3, 3, 4), 3)],
                         ids=["Cg2", "Cg64", "C24", "5x5", "stride3"])
def test_rejects_unsupported_shapes(gpu, C, w_shape, stride):
    x = torch.zeros(1, 6, 6, C, device=gpu, dtype=BF)
    w = torch.zeros(w_shape, device=gpu, dtype=BF)
    img = torch.zeros(2 * 9 * C * 16, device=gpu, dtype=BF)
    with pytest.raises(RuntimeError):
        T().gconv_fwd(x, w, img, torch.empty_like(x), stride)
    with pytest.raises(RuntimeError):
        T().gconv_wgrad(x, x, torch.zeros(w_shape, device=gpu), stride)


def test_resnet_tiny_cardinality(gpu):
    """One training step of resnet_tiny with cardinality=4 vs the CPU fp32 path
    (test_groupnorm_gpu.py test_resnet_tiny_group's comparison), then graph
    replay against eager."""
    tg = Trainer("resnet_tiny", gpu, seed=3, cardinality=4)
    tc = Trainer("resnet_tiny", "cpu", seed=3, cardinality=4)
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
    a = Trainer("resnet_tiny", gpu, seed=5, use_graph=True, cardinality=4)
    e = Trainer("resnet_tiny", gpu, seed=5, use_graph=False, cardinality=4)
    la = [float(a.step()) for _ in range(4)]       # two eager warm-up steps, then two replays
    le = [float(e.step()) for _ in range(4)]
    assert a._graph is not None and all(math.isfinite(v) for v in la)
    assert la[3] <= la[2]
    for i in (2, 3):
        assert abs(la[i] - le[i]) < 1e-2 * max(1.0, abs(le[i]))
