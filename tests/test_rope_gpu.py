"""Rotary position embeddings inside the flash-attention kernels (attention.hip,
ROPE variants) against a plain fp64 torch reference that rotates the bf16 inputs
by the formula (angles in fp64, not from the table); the trainer under hipGraph replay."""
import functools

import pytest
import torch

from tiresias_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu

BF, B, H = torch.bfloat16, 2, 2
SEED, STREAM, STEP, SITE, THR = 1234, 0, 7, 2, 26


def rotate64(x):
    # x [B,S,H,64] fp64; angle = token index * 10000^(-j/32), pairs (j, j + 32)
    w =10000.0 ** (-torch.arange(32, dtype=torch.float64) / 32)
    ang = (torch.arange(x.shape[1], dtype=torch.float64)[:, None] * w)[None, :, None, :]
    a, b = x[..., :32], x[..., 32:]
    return torch.cat([a * ang.cos() - b * ang.sin(), b * ang.cos() + a * ang.sin()], -1)


@functools.lru_cache(maxsize=None)
def case(Sq, Sk, causal, kvl, drop):
    """bf16 inputs (one packed qkv where Sq == Sk, else q and a packed kv) and the
    fp64 reference (o, lse, dq, dk, dv): computed once per shape, never written."""
    g = torch.Generator().manual_seed(11)
    if Sq == Sk:
        qsrc = kvsrc = torch.randn(B, Sq, 3, H, 64, generator=g).to(BF)
    else:
        qsrc, kvsrc = torch.randn(B, Sq, 1, H, 64, generator=g).to(BF), torch.randn(B, Sk, 2, H, 64, generator=g).to(BF)
    do = torch.randn(B, Sq, H, 64, generator=g).to(BF)
    qd, kd, vd = (t.double().requires_grad_(True) for t in (qsrc[:, :, 0], kvsrc[:, :, -2], kvsrc[:, :, -1]))
    s = torch.einsum("bqhd,bkhd->bhqk", rotate64(qd), rotate64(kd)) / 8.0
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(Sq, Sk, dtype=torch.bool), 1), float("-inf"))
    if kvl is not None:
        s = s.masked_fill((torch.arange(Sk)[None, :] >= torch.tensor(kvl)[:, None])[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    if drop:
        keep = Fx.attn_dropout_mask(B, H, Sq, Sk, SITE, SEED, STREAM, STEP, THR)
        p = torch.where(keep, p, torch.zeros((), dtype=p.dtype)) * (256.0 / (256 - THR))
    o = torch.einsum("bhqk,bkhd->bqhd", p, vd)
    gq, gk, gv = torch.autograd.grad(o, [qd, kd, vd], do.double())
    return (qsrc, kvsrc, do), (o.detach(), torch.logsumexp(s, -1).detach(), gq, gk, gv)


def device_run(gpu, inputs, causal, kvl, short, table, drop=()):
    qsrc, kvsrc, do = inputs
    packed, qsrc = qsrc is kvsrc, qsrc.to(gpu)
    kvsrc = qsrc if packed else kvsrc.to(gpu)
    dqsrc = torch.empty_like(qsrc)
    dkvsrc = dqsrc if packed else torch.empty_like(kvsrc)
    q, k, v = qsrc[:, :, 0], kvsrc[:, :, -2], kvsrc[:, :, -1]
    dq, dk, dv = dqsrc[:, :, 0], dkvsrc[:, :, -2], dkvsrc[:, :, -1]
    Sq = q.shape[1]
    kl = torch.tensor(kvl, device=gpu, dtype=torch.int32) if kvl else None
    o = torch.empty(B, Sq, H, 64, device=gpu, dtype=BF)
    lse = torch.empty(B, H, Sq, device=gpu)
    torch.ops.tam.attn_short_policy(short)
    try:
        torch.ops.tam.attn_forward(q, k, v, o, lse, causal, 0.125, kl, *drop, **table)
        torch.ops.tam.attn_backward(q, k, v, o, do.to(gpu), lse, dq, dk, dv, torch.empty(B, Sq, H, 64, device=gpu),
                          torch.empty(B, H, Sq, device=gpu), causal, 0.125, kl, *drop, **table)
        torch.cuda.synchronize()
    finally:
        torch.ops.tam.attn_short_policy(1)
    return o, lse, dq, dk, dv


def check(got, want):
    errs = {n: ((a.double().cpu() - b).norm() / b.norm()).item()
            for n, a, b in zip(("o", "lse", "dq", "dk", "dv"), got, want)}
    print(errs)
    assert errs["o"] < 1e-2 and errs["lse"] < 1e-3 and max(errs["dq"], errs["dk"], errs["dv"]) < 2e-2


@pytest.mark.parametrize("short", [1, 0])
@pytest.mark.parametrize("Sq,Sk,causal,kvl", [(37, 37, False, None), (96, 96, True, None),
                                              (70, 130, False, None), (128, 128, False, (96, 50))])
def test_forward_backward_numerics(gpu, Sq, Sk, causal, kvl, short):
    inputs, want = case(Sq, Sk, causal, kvl, False)
    table = Fx.rope_table(max(Sq, Sk), gpu)                       # exactly max(Sq, Sk) rows
    check(device_run(gpu, inputs, causal, kvl, short, {"rope": table}), want)


@pytest.mark.parametrize("S,short", [(96, 1), (160, 0)])
def test_composes_with_attention_dropout(gpu, S, short):
    inputs, want = case(S, S, True, None, True)
    drop = (torch.tensor([SEED, STREAM, STEP, 0], dtype=torch.int32, device=gpu), SITE, THR, Fx.attn_dropout_scale(THR))
    check(device_run(gpu, inputs, True, None, short, {"rope": Fx.rope_table(S, gpu)}, drop), want)


@pytest.mark.parametrize("short", [1, 0])
def test_no_table_is_the_call_without_the_argument(gpu, short):
    inputs, _ = case(70, 130, False, None, False)
    a = device_run(gpu, inputs, False, None, short, {})
    b = device_run(gpu, inputs, False, None, short, {"rope": None})
    assert all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)) for x, y in zip(a, b))


def test_bad_tables_raise(gpu):
    q, k, v = (torch.randn(B, 16, H, 64, device=gpu).to(BF) for _ in range(3))
    o, lse = torch.empty_like(q), torch.empty(B, H, 16, device=gpu)
    grads = [torch.empty_like(q) for _ in range(3)] + [torch.empty(B, 16, H, 64, device=gpu), torch.empty_like(lse)]
    good = Fx.rope_table(16, gpu)
    for bad in (good.double(), good.view(16, 64), good[:15], good.cpu()):      # dtype, shape, rows, device
        with pytest.raises(RuntimeError, match="rope"):
            torch.ops.tam.attn_forward(q, k, v, o, lse, False, 0.125, None, rope=bad)
        with pytest.raises(RuntimeError, match="rope"):
            torch.ops.tam.attn_backward(q, k, v, o, o, lse, *grads, False, 0.125, None, rope=bad)


def test_trainer_graph_replay_equals_eager(gpu):
    from tiresias_amd.executor.trainer import Trainer

    def losses(**kw):
        t = Trainer("transformer_tiny", gpu, seed=4, **kw)
        return t, [float(t.step()) for _ in range(4)]

    t, lg = losses(pos="rope", use_graph=True)
    assert t._graph is not None and t.pos == "rope" and t.model.rope is not None and t.model.pos is None
    _, le = losses(pos="rope")
    _, lp = losses(pos=None)
    print("graph", lg, "eager", le, "sinusoid", lp)
    assert lg == le and all(v == v for v in lg)
    assert lg[0] != lp[0]
