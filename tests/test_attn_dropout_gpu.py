"""Attention-probability dropout on the device: the mask drawn inside the
flash-attention kernels (csrc/kernels/attention.hip, DROP variants) against a
host mask written from the contract text in csrc/include/tam/philox.h, the
numerics of forward and both backward kernel families against an fp32 torch
reference that applies that mask, off-is-off, the CPU mirror, and the trainers
under hipGraph replay."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEED, STREAM, STEP, SITE = 1234, 0, 7, 2
B, H = 2, 3


def T():
    return torch.ops.tam


def rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def bits(t):
    return t.contiguous().view(torch.int16)


def _mulhilo(m, x):
    p = np.uint64(m) * x                       # both factors < 2^32: no overflow
    return p & np.uint64(0xFFFFFFFF), p >> np.uint64(32)


def host_attn_mask(nb, nh, Sq, Sk, thr, site=SITE, seed=SEED, stream=STREAM, step=STEP):
    """Keep mask [nb, nh, Sq, Sk] of the attention mask contract in numpy,
    written from its text: one Philox4x32-10 call per block of 4 queries x 4
    keys, (Q, K) = (q >> 2, kv >> 2), counter (K | Q << 16, b*H + h,
    0x80000000 | a, step), key (seed, stream), u = (out[q & 3] >> 8 (kv & 3))
    & 0xff, kept iff u >= thr."""
    nq, nk = (Sq + 3) // 4, (Sk + 3) // 4
    bh, Q, K = np.meshgrid(np.arange(nb * nh, dtype=np.uint64), np.arange(nq, dtype=np.uint64),
                           np.arange(nk, dtype=np.uint64), indexing="ij")
    c = [K | (Q << np.uint64(16)), bh, np.full_like(bh, 0x80000000 | site), np.full_like(bh, step)]
    k = [seed & 0xFFFFFFFF, stream & 0xFFFFFFFF]
    for _ in range(10):
        lo0, hi0 = _mulhilo(0xD2511F53, c[0])
        lo1, hi1 = _mulhilo(0xCD9E8D57, c[2])
        c = [hi1 ^ c[1] ^ np.uint64(k[0]), lo1, hi0 ^ c[3] ^ np.uint64(k[1]), lo0]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    keep = np.zeros((nb * nh, 4 * nq, 4 * nk), dtype=bool)
    for qi in range(4):
        for ki in range(4):
            u = (c[qi] >> np.uint64(8 * ki)) & np.uint64(0xFF)
            keep[:, qi::4, ki::4] = u >= np.uint64(thr)
    return torch.from_numpy(keep[:, :Sq, :Sk].reshape(nb, nh, Sq, Sk).copy())


def scale_of(thr):
    return float(np.float32(256.0) / np.float32(256 - thr))


def record(gpu, seed=SEED, stream=STREAM, step=STEP):
    return torch.tensor([seed, stream, step, 0], dtype=torch.int32, device=gpu)


SHAPES = [(37, 50), (70, 130), (64, 64), (96, 96), (128, 128)]


@pytest.fixture(scope="module")
def masks():
    """(Sq, Sk, thr) -> host keep mask (CPU bool [B,H,Sq,Sk]); computed once,
    never written."""
    return {(sq, sk, thr): host_attn_mask(B, H, sq, sk, thr) for sq, sk in SHAPES for thr in (26, 128)}


def device_keep(gpu, Sq, Sk, thr, kv_one=None):
    """The kernel's keep pattern [B,H,Sq,Sk] and the kept values, read through
    the forward: q = 0 gives every key probability 1/Sk, and a one-hot V per
    64-key tile j (V[kv, d] = 1 iff kv // 64 == j and d == kv % 64) puts
    probability (q, 64j + d) into O[q, d]."""
    q = torch.zeros(B, Sq, H, 64, device=gpu, dtype=BF)
    k = torch.randn(B, Sk, H, 64, device=gpu).to(BF)
    rec = record(gpu)
    keep = torch.zeros(B, H, Sq, Sk, dtype=torch.bool)
    vals = torch.zeros(B, H, Sq, Sk, dtype=BF)
    for j in range((Sk + 63) // 64):
        n = min(64, Sk - 64 * j)
        v = torch.zeros(B, Sk, H, 64, device=gpu, dtype=BF)
        idx = torch.arange(n, device=gpu)
        v[:, 64 * j + idx, :, idx] = 1.0
        o = torch.full((B, Sq, H, 64), 7.0, device=gpu, dtype=BF)
        lse = torch.empty(B, H, Sq, device=gpu)
        T().attn_forward(q, k, v, o, lse, False, 0.125, None, rec, SITE, thr, scale_of(thr))
        oc = o.permute(0, 2, 1, 3).cpu()                      # [B,H,Sq,64]
        assert bool((oc[..., n:] == 0).all())                 # columns past the tile's keys stay 0
        keep[..., 64 * j:64 * j + n] = oc[..., :n] != 0
        vals[..., 64 * j:64 * j + n] = oc[..., :n]
    assert rec.tolist() == [SEED, STREAM, STEP, 0]            # the kernel only reads the record
    return keep, vals


# ------------------------------------------------------------------ 1. exact mask, forward
@pytest.mark.parametrize("thr", [26, 128])
@pytest.mark.parametrize("Sq,Sk", [(37, 50), (70, 130), (64, 64)])
def test_forward_mask_equals_host_mask(gpu, masks, Sq, Sk, thr):
    torch.manual_seed(5)
    keep, vals = device_keep(gpu, Sq, Sk, thr)
    want = masks[(Sq, Sk, thr)]
    print("kept", int(keep.sum()), "host", int(want.sum()), "of", want.numel())
    assert torch.equal(keep, want)
    # kept values: bf16(dscale / Sk) to within one bf16 ulp
    ref = int(bits(torch.tensor([np.float32(scale_of(thr)) / np.float32(Sk)], dtype=torch.float32).to(BF))[0])
    d = (bits(vals)[want].int() - ref).abs().max()
    print("max ulp distance of kept values", int(d))
    assert int(d) <= 1


# ------------------------------------------------------------------ 2. numerics, forward and backward
def _ref(q, k, v, causal, kv_len, keep, dscale):
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) / 8.0
    Sq, Sk = s.shape[-2:]
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(Sq, Sk, dtype=torch.bool, device=s.device), 1), float("-inf"))
    if kv_len is not None:
        km = torch.arange(Sk, device=s.device)[None, :] >= kv_len[:, None]
        s = s.masked_fill(km[:, None, None, :], float("-inf"))
    p = torch.softmax(s, -1)
    p = torch.where(keep, p, torch.zeros((), device=p.device)) * dscale
    return (p @ vf).permute(0, 2, 1, 3), torch.logsumexp(s, -1)


@pytest.mark.parametrize("short", [1, 0])
@pytest.mark.parametrize("Sq,Sk,causal,kvl", [(37, 50, False, None), (96, 96, True, None),
                                              (70, 130, False, None), (128, 128, False, [96, 50])])
def test_forward_backward_numerics(gpu, masks, Sq, Sk, causal, kvl, short):
    thr = 26
    sc = scale_of(thr)
    keep = masks[(Sq, Sk, thr)].to(gpu)
    torch.manual_seed(11)
    qkv = torch.randn(B, Sq, 3, H, 64, device=gpu).to(BF) if Sq == Sk else None
    if qkv is not None:
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    else:
        q = torch.randn(B, Sq, H, 64, device=gpu).to(BF)
        kv = torch.randn(B, Sk, 2, H, 64, device=gpu).to(BF)
        k, v = kv[:, :, 0], kv[:, :, 1]
    kl = torch.tensor(kvl, device=gpu, dtype=torch.int32) if kvl else None
    rec = record(gpu)
    o = torch.empty(B, Sq, H, 64, device=gpu, dtype=BF)
    lse = torch.empty(B, H, Sq, device=gpu)
    o0, lse0 = torch.empty_like(o), torch.empty_like(lse)
    T().attn_short_policy(short)
    try:
        T().attn_forward(q, k, v, o, lse, causal, 0.125, kl, rec, SITE, thr, sc)
        T().attn_forward(q, k, v, o0, lse0, causal, 0.125, kl)
        do = torch.randn_like(o)
        if qkv is not None:
            dqkv = torch.empty_like(qkv)
            dq, dk, dv = dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2]
        else:
            dq = torch.empty_like(q)
            dkv = torch.empty_like(kv)
            dk, dv = dkv[:, :, 0], dkv[:, :, 1]
        T().attn_backward(q, k, v, o, do, lse, dq, dk, dv,
                          torch.empty(B, Sq, H, 64, device=gpu), torch.empty(B, H, Sq, device=gpu),
                          causal, 0.125, kl, rec, SITE, thr, sc)
        torch.cuda.synchronize()
    finally:
        T().attn_short_policy(1)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    of, lref = _ref(qf, kf, vf, causal, kl.long() if kl is not None else None, keep, sc)
    gq, gk, gv = torch.autograd.grad(of, [qf, kf, vf], do.float())
    errs = dict(o=rel_err(o, of), lse=rel_err(lse, lref), dq=rel_err(dq, gq), dk=rel_err(dk, gk),
                dv=rel_err(dv, gv), o_vs_undropped=rel_err(o, o0))
    print(errs)
    assert errs["o"] < 1e-2
    assert errs["lse"] < 1e-3
    assert torch.equal(lse.view(torch.int32), lse0.view(torch.int32))     # the LSE of the undropped scores
    assert errs["dq"] < 2e-2 and errs["dk"] < 2e-2 and errs["dv"] < 2e-2
    assert errs["o_vs_undropped"] > 0.1                                   # ...and something was dropped


# ------------------------------------------------------------------ 3. off is off
@pytest.mark.parametrize("short", [1, 0])
def test_no_record_is_the_call_without_the_arguments(gpu, short):
    Sq, Sk = 70, 100
    torch.manual_seed(3)
    q = torch.randn(B, Sq, H, 64, device=gpu).to(BF)
    k, v = (torch.randn(B, Sk, H, 64, device=gpu).to(BF) for _ in range(2))
    do = torch.randn(B, Sq, H, 64, device=gpu).to(BF)

    def run(*extra):
        o = torch.full((B, Sq, H, 64), 7.0, device=gpu, dtype=BF)
        lse = torch.empty(B, H, Sq, device=gpu)
        T().attn_forward(q, k, v, o, lse, False, 0.125, None, *extra)
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        T().attn_backward(q, k, v, o, do, lse, dq, dk, dv, torch.empty(B, Sq, H, 64, device=gpu),
                          torch.empty(B, H, Sq, device=gpu), False, 0.125, None, *extra)
        return o, lse, dq, dk, dv

    T().attn_short_policy(short)
    try:
        a = run()
        b = run(None, 5, 26, scale_of(26))
    finally:
        T().attn_short_policy(1)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int16 if x.dtype == BF else torch.int32),
                           y.view(torch.int16 if y.dtype == BF else torch.int32))


def test_bad_arguments_raise(gpu):
    q, k, v = (torch.randn(B, 16, H, 64, device=gpu).to(BF) for _ in range(3))
    o = torch.empty_like(q)
    lse = torch.empty(B, H, 16, device=gpu)
    rec = record(gpu)
    bad = [(rec, 0, 0, 1.0), (rec, 0, 256, 1.0), (rec.cpu(), 0, 26, 1.0), (rec.float(), 0, 26, 1.0),
           (rec.long(), 0, 26, 1.0)]
    ws = torch.empty(B, 16, H, 64, device=gpu), torch.empty(B, H, 16, device=gpu)
    for extra in bad:
        with pytest.raises(RuntimeError, match="drop_"):
            T().attn_forward(q, k, v, o, lse, False, 0.125, None, *extra)
        with pytest.raises(RuntimeError, match="drop_"):
            T().attn_backward(q, k, v, o, o, lse, torch.empty_like(q), torch.empty_like(k), torch.empty_like(v),
                              *ws, False, 0.125, None, *extra)


# ------------------------------------------------------------------ 4. keep rate
def test_keep_rate(gpu, masks):
    thr, S = 26, 128
    want = masks[(S, S, thr)]
    n = want.numel()
    assert n == 98304
    qk = 1 - thr / 256
    sigma = (n * qk * (1 - qk)) ** 0.5
    print("host kept", int(want.sum()), "expected", n * qk, "sigma", sigma)
    assert abs(int(want.sum()) - n * qk) < 6 * sigma              # the host reference itself
    torch.manual_seed(6)
    keep, _ = device_keep(gpu, S, S, thr)
    print("device kept", int(keep.sum()))
    assert int(keep.sum()) == int(want.sum())


# ------------------------------------------------------------------ 5. device against the CPU mirror
def _elementwise_host_mask(n, site, seed, stream, step, thr):
    """The elementwise dropout contract (8 elements per Philox call, 16 bits
    each), as in the README."""
    g = np.arange((n + 7) // 8, dtype=np.uint64)
    c = [g & np.uint64(0xFFFFFFFF), g >> np.uint64(32), np.full_like(g, site), np.full_like(g, step)]
    k = [seed & 0xFFFFFFFF, stream & 0xFFFFFFFF]
    for _ in range(10):
        lo0, hi0 = _mulhilo(0xD2511F53, c[0])
        lo1, hi1 = _mulhilo(0xCD9E8D57, c[2])
        c = [hi1 ^ c[1] ^ np.uint64(k[0]), lo1, hi0 ^ c[3] ^ np.uint64(k[1]), lo0]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    i = np.arange(n)
    j = i & 7
    w = np.stack(c, 1)[i >> 3, j >> 1]
    u = (w >> (np.uint64(16) * (j & 1).astype(np.uint64))) & np.uint64(0xFFFF)
    return torch.from_numpy(u >= np.uint64(thr))


def test_device_and_cpu_mirror_drop_the_same_probabilities(gpu):
    from tiresias_amd.ops import functional as Fx

    S, nb = 48, 2
    gen = torch.Generator().manual_seed(9)
    qkv = torch.randn(nb, S, 3 * 64, generator=gen).to(BF)
    # second call: q = 0, V = identity on the first S columns -> O[q, d] = keep(q, d) * scale / S
    probe = torch.zeros(nb, S, 3, 1, 64)
    probe[:, :, 1] = torch.randn(nb, S, 1, 64, generator=gen)
    probe[:, torch.arange(S), 2, 0, torch.arange(S)] = 1.0
    probe = probe.view(nb, S, 3 * 64).to(BF)
    x = (torch.randn(5, 64, generator=gen).abs() + 0.5).to(BF)       # no zeros: a 0 is a drop
    out = {}
    for dev in (torch.device("cpu"), gpu):
        Fx.set_dropout(torch.tensor([5, 1, 9, 0], dtype=torch.int32, device=dev))
        try:
            o1 = Fx.self_attention(qkv.to(dev), 1, causal=True, drop=0.5)       # attention site 0
            y = Fx.dropout(x.to(dev), 0.5)                                       # elementwise site 0
            o2 = Fx.self_attention(probe.to(dev), 1, drop=0.5)                   # attention site 1
            Fx.set_dropout(torch.tensor([5, 1, 9, 0], dtype=torch.int32, device=dev))
            y_alone = Fx.dropout(x.to(dev), 0.5)                                 # elementwise site 0, no attention
        finally:
            Fx.set_dropout(None)
        out[dev.type] = (o1.cpu(), y.cpu(), o2.cpu(), y_alone.cpu())
    (o1c, yc, o2c, yac), (o1g, yg, o2g, yag) = out["cpu"], out["cuda"]
    e = rel_err(o1g, o1c)
    print("rel_err device vs cpu", e)
    assert e < 1e-2
    want1 = host_attn_mask(nb, 1, S, S, 128, site=1, seed=5, stream=1, step=9)[:, 0]
    assert torch.equal(o2g[:, :, :S] != 0, want1) and torch.equal(o2c[:, :, :S] != 0, want1)
    # site 0 is a different mask: the ordinal matters
    assert not torch.equal(host_attn_mask(nb, 1, S, S, 128, site=0, seed=5, stream=1, step=9)[:, 0], want1)
    # the elementwise sites keep their ordinals whether or not attention dropout ran
    em = _elementwise_host_mask(5 * 64, 0, 5, 1, 9, 32768).view(5, 64)
    for yy in (yc, yg, yac, yag):
        assert torch.equal(yy != 0, em)


# ------------------------------------------------------------------ 6. trainers
def _eager(gpu, steps, **kw):
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer("transformer_tiny", gpu, seed=4, **kw)
    losses = [t.step() for _ in range(steps)]
    torch.cuda.synchronize()
    return t, [float(v) for v in losses]


def _graph(gpu, steps, **kw):
    """Per-step losses of a graph trainer (the replayed loss tensor is one
    buffer: read it after every step)."""
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer("transformer_tiny", gpu, seed=4, use_graph=True, **kw)
    out = [float(t.step()) for _ in range(steps)]
    torch.cuda.synchronize()
    return t, out


@pytest.fixture(scope="module")
def plain_losses(gpu):
    return _eager(gpu, 5)[1]


def test_graph_replay_draws_new_attention_masks(gpu, plain_losses):
    t, lg = _graph(gpu, 5, attn_dropout=0.5)
    assert t._graph is not None and t.attn_dropout == 0.5 and t.dropout is None
    assert t._drop_rec.tolist() == [4, 0, 5, 0]                   # advanced on the device, once per step
    _, le = _eager(gpu, 5, attn_dropout=0.5)
    print("graph", lg, "eager", le, "plain", plain_losses)
    assert lg == le                                               # bit for bit
    assert all(a != b for a, b in zip(lg, lg[1:])) and all(v == v for v in lg)
    assert all(a != b for a, b in zip(lg, plain_losses))


def test_both_knobs_share_one_advance(gpu, plain_losses):
    t, lg = _graph(gpu, 5, dropout=0.1, attn_dropout=0.5)
    assert t._graph is not None and t._drop_rec.tolist() == [4, 0, 5, 0]
    _, le = _eager(gpu, 5, dropout=0.1, attn_dropout=0.5)
    print("graph", lg, "eager", le)
    assert lg == le
    _, ld = _eager(gpu, 5, dropout=0.1)
    assert lg != ld and lg != plain_losses


def test_off_is_off_and_resume(gpu, plain_losses):
    from tiresias_amd.executor.trainer import Trainer

    t, l_none = _eager(gpu, 3, attn_dropout=None)
    assert t.attn_dropout is None and t._drop_rec is None
    assert l_none == plain_losses[:3]
    # a resumed job continues the mask sequence: rebuilt at step 2
    _, la = _eager(gpu, 3, attn_dropout=0.5)
    b, _ = _eager(gpu, 2, attn_dropout=0.5)
    c = Trainer("transformer_tiny", gpu, seed=4, attn_dropout=0.5)
    for k, v in b.state_tensors().items():
        c.state_tensors()[k].copy_(v)
    c.step_count = 2
    assert float(c.step()) == la[2]
    assert c._drop_rec.tolist() == [4, 0, 3, 0]
