"""Training dropout on the device: the standalone Philox kernel
(csrc/kernels/dropout.hip) against the host mask of the contract, the
dropout fused into the LayerNorm forward / backward kernels (norm.hip), the
device-side advance of the record under hipGraph replay, and the CPU mirror."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEED, STREAM, STEP, SITE = 1234, 0, 7, 3


def T():
    return torch.ops.tam


def rel_err(a, b):
    a = a.float()
    b = b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _mulhilo(m, x):
    p = np.uint64(m) * x                       # both factors < 2^32: no overflow
    return p & np.uint64(0xFFFFFFFF), p >> np.uint64(32)


def host_mask(n, site=SITE, seed=SEED, stream=STREAM, step=STEP, thr=6554):
    """Keep mask of the mask contract in numpy, written from its text: one
    Philox4x32-10 call per 8 elements, counter (q lo, q hi, site, step), key
    (seed, stream), 16 bits per element, kept iff u >= thr."""
    q = np.arange((n + 7) // 8, dtype=np.uint64)
    c = [q & np.uint64(0xFFFFFFFF), q >> np.uint64(32), np.full_like(q, site), np.full_like(q, step)]
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


def scale_of(thr):
    return float(np.float32(65536.0) / np.float32(65536 - thr))


def record(gpu, seed=SEED, stream=STREAM, step=STEP):
    return torch.tensor([seed, stream, step, 0], dtype=torch.int32, device=gpu)


def bits(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------ standalone kernel
# one group; a scalar tail (4099 = 512 groups + 3); several grid sweeps (> 256 CUs x 256 threads groups)
SIZES = [8, 4099, 2 ** 20 + 8]


@pytest.fixture(scope="module")
def masks():
    """(n, thr) -> host keep mask (CPU bool); computed once, never written."""
    return {(n, thr): host_mask(n, thr=thr) for n in SIZES + [2 ** 20] for thr in (6554, 32768)}


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", SIZES)
def test_dropout_apply_bit_equal_to_host_reference(gpu, masks, n, p):
    thr = round(p * 65536)
    sc = scale_of(thr)
    keep = masks[(n, thr)].to(gpu)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(n)
    x = torch.randn(n, device=gpu, generator=gen).to(BF)
    dy = torch.randn(n, device=gpu, generator=gen).to(BF)
    rec = record(gpu)
    zero = torch.zeros((), dtype=BF, device=gpu)

    def ref(t):
        return torch.where(keep, (t.float() * sc).to(BF), zero)

    y = torch.full_like(x, 7.0)
    T().dropout_apply(x, y, rec, SITE, thr, sc)
    assert torch.equal(bits(y), bits(ref(x)))
    # the backward is the same kernel on dy
    dx = torch.full_like(x, 7.0)
    T().dropout_apply(dy, dx, rec, SITE, thr, sc)
    assert torch.equal(bits(dx), bits(ref(dy)))
    # in place
    z = x.clone()
    T().dropout_apply(z, z, rec, SITE, thr, sc)
    assert torch.equal(bits(z), bits(y))
    assert rec.tolist() == [SEED, STREAM, STEP, 0]               # the kernel only reads the record


def test_keep_rate(gpu, masks):
    n, thr = 2 ** 20, 6554
    q = 1 - thr / 65536
    sigma = (n * q * (1 - q)) ** 0.5                              # ~307
    assert abs(int(masks[(n, thr)].sum()) - n * q) < 6 * sigma    # the host reference itself
    x = torch.ones(n, dtype=BF, device=gpu)
    y = torch.empty_like(x)
    T().dropout_apply(x, y, record(gpu), SITE, thr, scale_of(thr))
    kept = int((y != 0).sum())
    print("kept", kept, "expected", n * q, "sigma", sigma)
    assert abs(kept - n * q) < 6 * sigma
    assert kept == int(masks[(n, thr)].sum())


def test_dropout_advance(gpu):
    rec = record(gpu, step=0x7FFFFFFF)
    T().dropout_advance(rec)
    assert rec.tolist() == [SEED, STREAM, -0x80000000, 0]          # the step word wraps as uint32
    T().dropout_advance(rec)
    assert rec.tolist() == [SEED, STREAM, -0x7FFFFFFF, 0]


# ------------------------------------------------------------------ fused into LayerNorm
LN_SHAPES = [(37, 512), (9, 1024), (5, 2048)]     # VEC = 1, 2, 4; rows % 4 != 0


def _ln_inputs(gpu, rows, D):
    gen = torch.Generator(device=gpu)
    gen.manual_seed(rows * D)
    x = (torch.randn(rows, D, device=gpu, generator=gen) * 2 + 0.5).to(BF)
    r = torch.randn(rows, D, device=gpu, generator=gen).to(BF)
    x.view(-1)[:16] = -0.0                          # dropped positions keep x's bits, a -0 included
    g = torch.rand(D, device=gpu, generator=gen) + 0.5
    b = torch.randn(D, device=gpu, generator=gen)
    return x, r, g, b


@pytest.mark.parametrize("rows,D", LN_SHAPES)
def test_fused_forward(gpu, rows, D):
    thr = 32768
    sc = scale_of(thr)
    x, r, g, b = _ln_inputs(gpu, rows, D)
    keep = host_mask(rows * D, thr=thr).view(rows, D).to(gpu)
    assert 0 < int((~keep.view(-1)[:16]).sum())                   # some of the -0 positions are dropped
    rec = record(gpu)
    sm, y = torch.empty_like(x), torch.empty_like(x)
    mean, rstd = torch.empty(rows, device=gpu), torch.empty(rows, device=gpu)
    T().ln_forward(x, g, b, y, mean, rstd, 1e-5, r, sm, rec, SITE, thr, sc)
    assert torch.equal(bits(sm)[~keep], bits(x)[~keep])           # dropped: sum_out == x bit for bit
    sref = x.float() + torch.where(keep, r.float() * sc, torch.zeros((), device=gpu))
    e_s, e_y = rel_err(sm, sref), rel_err(y, F.layer_norm(sref, (D,), g, b, 1e-5))
    print("rel_err sum_out", e_s, "y", e_y)
    assert e_s < 1e-2 and e_y < 1e-2
    # ...and exactly the kernel's own rounding: fp32 product, fp32 sum, one bf16 rounding
    assert torch.equal(bits(sm)[keep], bits(sref.to(BF))[keep])
    # record omitted: bit-equal to a call without the new arguments
    sm0, y0, sm1, y1 = (torch.empty_like(x) for _ in range(4))
    m0, r0, m1, r1 = (torch.empty(rows, device=gpu) for _ in range(4))
    T().ln_forward(x, g, b, y0, m0, r0, 1e-5, r, sm0)
    T().ln_forward(x, g, b, y1, m1, r1, 1e-5, r, sm1, None, SITE, thr, sc)
    assert torch.equal(bits(sm0), bits(sm1)) and torch.equal(bits(y0), bits(y1))
    assert torch.equal(m0, m1) and torch.equal(r0, r1)
    assert torch.equal(sm0, (x.float() + r.float()).to(BF))


@pytest.mark.parametrize("path", ["immediate", "split"])
def test_fused_backward(gpu, path):
    rows, D, thr = 37, 512, 32768                   # rows_per_block at its minimum of 8: 5 blocks
    sc = scale_of(thr)
    x, _, g, _ = _ln_inputs(gpu, rows, D)
    keep = host_mask(rows * D, thr=thr).view(rows, D).to(gpu)
    gen = torch.Generator(device=gpu)
    gen.manual_seed(1)
    dy = torch.randn(rows, D, device=gpu, generator=gen).to(BF)
    add = torch.randn(rows, D, device=gpu, generator=gen).to(BF)
    mean = x.float().mean(1)
    rstd = torch.rsqrt(x.float().var(1, unbiased=False) + 1e-5)
    rec = record(gpu)

    def run(*extra):
        dx = torch.empty_like(x)
        dg, db = torch.zeros(D, device=gpu), torch.zeros(D, device=gpu)
        if path == "immediate":
            T().ln_backward(dy, x, g, mean, rstd, dx, dg, db, add, *extra)
        else:
            ws = torch.empty(512 * 2 * D, device=gpu)
            nblk = T().ln_backward_split(dy, x, g, mean, rstd, dx, ws, add, *extra)
            assert nblk == 5
            T().col_reduce_acc_batch([ws], [nblk], [dg], [db])
        return dx, dg, db

    dx0, dg0, db0 = run()
    dr = torch.full_like(x, 7.0)
    dx1, dg1, db1 = run(dr, rec, SITE, thr, sc)
    assert torch.equal(bits(dx0), bits(dx1))                       # dx unchanged, bitwise
    assert torch.equal(dg0, dg1) and torch.equal(db0, db1)
    assert bool((bits(dr)[~keep] == 0).all())                      # exactly +0 at dropped positions
    xf = x.float().requires_grad_(True)
    yf = F.layer_norm(xf, (D,), g, None, 1e-5)
    dx_ref = torch.autograd.grad(yf, xf, dy.float())[0] + add.float()
    e_dx, e_dr = rel_err(dx1, dx_ref), rel_err(dr, dx_ref * keep * sc)
    print("rel_err dx", e_dx, "dr", e_dr)
    assert e_dx < 2e-2 and e_dr < 2e-2
    with pytest.raises(RuntimeError, match="dr and drop_rec"):
        run(dr)                                                    # dr without the record


# ------------------------------------------------------------------ device against the CPU mirror
def test_device_and_cpu_mirror_drop_the_same_elements(gpu):
    from tiresias_amd.ops import functional as Fx
    from tiresias_amd.ops.arena import Arena

    out = {}
    for dev in (torch.device("cpu"), gpu):
        A = Arena(dev, seed=0)
        g = A.add("g", (512,), init="ones", decay=False, fp32_compute=True)
        b = A.add("b", (512,), init="zeros", decay=False, fp32_compute=True)
        A.materialize()
        gen = torch.Generator().manual_seed(3)
        x = (torch.randn(6, 512, generator=gen).abs() + 0.5).to(BF).to(dev)     # no zeros: a 0 is a drop
        r = (torch.randn(6, 512, generator=gen).abs() + 0.5).to(BF).to(dev)
        Fx.set_dropout(torch.tensor([5, 1, 9, 0], dtype=torch.int32, device=dev))
        try:
            y = Fx.dropout(x, 0.5)                                              # site 0
            s, _ = Fx.add_layernorm_skip(x, r, g, b, drop=0.1)                  # site 1
        finally:
            Fx.set_dropout(None)
        out[dev.type] = (y.cpu(), s.cpu(), x.cpu())
    (yc, sc_, xc), (yg, sg, _) = out["cpu"], out["cuda"]
    assert torch.equal(bits(yc), bits(yg))                                      # standalone: bitwise
    assert torch.equal(yc != 0, host_mask(6 * 512, 0, 5, 1, 9, 32768).view(6, 512))
    dropped_c, dropped_g = bits(sc_) == bits(xc), bits(sg) == bits(xc)
    assert torch.equal(dropped_c, dropped_g)
    assert torch.equal(~dropped_c, host_mask(6 * 512, 1, 5, 1, 9, 6554).view(6, 512))
    assert torch.equal(bits(sc_), bits(sg))                                     # same rounding too


# ------------------------------------------------------------------ trainers: advance, replay, off
def _run(gpu, model, steps, **kw):
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer(model, gpu, seed=4, **kw)
    losses = [t.step() for _ in range(steps)]
    torch.cuda.synchronize()
    out = [float(v) for v in losses] if not kw.get("use_graph") else None
    return t, losses, out


def _graph_losses(gpu, model, steps, **kw):
    """Per-step losses of a graph trainer (the replayed loss tensor is one
    buffer: read it after every step)."""
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer(model, gpu, seed=4, use_graph=True, **kw)
    out = []
    for _ in range(steps):
        out.append(float(t.step()))
    torch.cuda.synchronize()
    return t, out


def test_transformer_graph_replay_draws_new_masks(gpu):
    t, lg = _graph_losses(gpu, "transformer_tiny", 5, dropout=0.1)
    assert t._graph is not None                                   # 2 eager warm steps, capture, replays
    assert t._drop_rec.tolist() == [4, 0, 5, 0]                   # advanced on the device, once per step
    _, _, le = _run(gpu, "transformer_tiny", 5, dropout=0.1)
    print("graph", lg, "eager", le)
    assert lg == le                                               # bit for bit
    assert lg[3] != lg[4]
    _, _, loff = _run(gpu, "transformer_tiny", 5)
    assert lg[0] != loff[0] and all(v == v for v in lg)


@pytest.mark.parametrize("model", ["vgg_tiny", "gnmt_tiny"])
def test_graph_equals_eager_with_dropout(gpu, model):
    t, lg = _graph_losses(gpu, model, 5, dropout=0.2)
    assert t._graph is not None and t._drop_rec.tolist() == [4, 0, 5, 0]
    _, _, le = _run(gpu, model, 5, dropout=0.2)
    print("graph", lg, "eager", le)
    assert lg == le
    _, _, loff = _run(gpu, model, 5)
    assert le != loff


def test_off_is_off(gpu):
    t, _, l_none = _run(gpu, "transformer_tiny", 3, dropout=None)
    assert t.dropout is None and t._drop_rec is None
    _, _, l_plain = _run(gpu, "transformer_tiny", 3)
    assert l_none == l_plain
    # a resumed job continues the sequence on the device too: rebuilt at step 2
    a, _, la = _run(gpu, "transformer_tiny", 3, dropout=0.1)
    b, _, _ = _run(gpu, "transformer_tiny", 2, dropout=0.1)
    from tiresias_amd.executor.trainer import Trainer

    c = Trainer("transformer_tiny", gpu, seed=4, dropout=0.1)
    for k, v in b.state_tensors().items():
        c.state_tensors()[k].copy_(v)
    c.step_count = 2
    assert float(c.step()) == la[2]
    assert c._drop_rec.tolist() == [4, 0, 3, 0]
