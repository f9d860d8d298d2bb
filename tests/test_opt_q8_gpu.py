"""8-bit block-scaled optimizer state on the device (csrc/kernels/optim_q8.hip
adam_stream_q8_kernel / sgd_stream_q8_kernel) against an fp64 step on the CPU
(tests/test_opt_q8_cpu.py make_case / run / check_step), the expectation of
the stored value, reproducibility across grids, skipped steps, the Trainer."""
import pytest
import torch
from test_opt_q8_cpu import B1, B2, F32, make_case, check_step, run

from tiresias_amd.ops import functional as Fx

pytestmark = pytest.mark.gpu
SIZES = [64, 256, 256 * 19 + 64]          # one partial block; one block; more blocks than waves and a partial one


@pytest.fixture
def grid1(gpu):
    """Grid cap 1 = 3 workgroups = 12 waves (at the cap 2 the fp32-state tests
    use there would be more waves than blocks): 20 blocks take some waves
    round the strided loop twice and end in a partial block."""
    torch.ops.tam.optim_grid(1)
    yield
    torch.ops.tam.optim_grid(0)


@pytest.mark.parametrize("clip", [None, 0.5])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_step_against_fp64(gpu, grid1, opt, n, clip):
    c = make_case(opt, n)
    rec = None if clip is None else torch.tensor([clip, 1.0, 0.0, 0.0], device=gpu)
    check_step(opt, c, run(opt, c, gpu, clip=rec), gs=F32(0.37) * (clip or 1.0))


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_stored_value_is_unbiased(gpu, opt):
    """lr = 0, zero prior state, 258 blocks: element 0 of a block holds the
    gradient A (it fixes the scale), the other N = 258 * 255 hold 0.6 A, so
    every fresh moment is the same x strictly between two codes. The mean
    decoded value is within 5 sigma of x, sigma = (T[k+1] - T[k]) s sqrt(p (1
    - p) / N): N independent two-point draws."""
    nb, A = 258, 0.5
    c = make_case(opt, 256 * nb)
    c["g"] = torch.full((256 * nb,), F32(0.6 * A))
    c["g"][::256] = A
    c["mq"].zero_(), c["vq"].zero_(), c["scales"].zero_()
    g32 = c["g"][:2].clone()                                    # [anchor, regular] through the fp32 update
    fresh = [g32] if opt == "sgd" else [(1 - torch.tensor(B1)) * g32, (1 - torch.tensor(B2)) * g32 * g32]
    outs = [run(opt, c, gpu, step=s, gs=1.0, lr=0.0, wd=0.0)[3] for s in (1, 2)]
    for i, (s, x) in enumerate(fresh):
        tab = Fx.q8_tables()[i].double()
        y = float(x) / float(s)
        k = int(torch.searchsorted(tab, torch.tensor(y, dtype=torch.float64), right=True)) - 1
        p = (y - float(tab[k])) / float(tab[k + 1] - tab[k])
        assert 0.05 < p < 0.95
        sigma = float(tab[k + 1] - tab[k]) * float(s) * (p * (1 - p) / (nb * 255)) ** 0.5
        assert bool((outs[0][-1][i] == s).all())
        codes = outs[0][i].view(nb, 256)[:, 1:]
        assert set(codes.unique().tolist()) == {k, k + 1}
        mean = float(Fx.q8_decode(outs[0][i], outs[0][-1][i]).double().view(nb, 256)[:, 1:].mean())
        print(opt, "moment", i, "x", float(x), "mean", mean, "diff / sigma", (mean - float(x)) / sigma)
        assert abs(mean - float(x)) <= 5 * sigma
        assert not torch.equal(outs[0][i], outs[1][i])          # another step: other codes


@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_reproducible(gpu, opt):
    c = make_case(opt, SIZES[2])
    outs = []
    for grid in (0, 0, 1, 2):
        torch.ops.tam.optim_grid(grid)
        outs.append(run(opt, c, gpu))
    torch.ops.tam.optim_grid(0)
    flat = [o[:3] + o[3] for o in outs]
    assert all(torch.equal(a, b) for o in flat[1:] for a, b in zip(flat[0], o))
    other = run(opt, c, gpu, seed=6)
    assert not torch.equal(other[3][0], outs[0][3][0]) and torch.equal(other[0], outs[0][0])


@pytest.mark.parametrize("how", ["guard", "clip"])
@pytest.mark.parametrize("opt", ["adam", "sgd"])
def test_skipped_step(gpu, grid1, opt, how):
    c = make_case(opt, SIZES[2])
    guard = torch.tensor([1, 0], dtype=torch.int32, device=gpu) if how == "guard" else None
    clip = torch.tensor([-1.0, float("inf"), 0.0, 0.0], device=gpu) if how == "clip" else None
    w, g, wb, state = run(opt, c, gpu, guard=guard, clip=clip)
    assert torch.equal(w, c["w"]) and bool((wb == 1).all())
    assert all(torch.equal(s, c[k]) for s, k in zip(state, ("mq", "scales") if opt == "sgd" else ("mq", "vq", "scales")))
    n, zf = c["n"], c["zf"]
    assert torch.equal(g[:zf], c["g"][:zf]) and int(torch.count_nonzero(g[zf:n])) == 0 and torch.equal(g[n:], c["g"][n:])


@pytest.mark.parametrize("model", ["transformer_tiny", "vgg_tiny", "gnmt_tiny"])
def test_trainer(gpu, model, tmp_path):
    from tiresias_amd.ckpt.snapshot import SnapshotWriter, load_snapshot
    from tiresias_amd.executor.trainer import Trainer

    e, g = Trainer(model, gpu, seed=4, opt_dtype="q8"), Trainer(model, gpu, seed=4, opt_dtype="q8", use_graph=True)
    f = Trainer(model, gpu, seed=4)
    n, k = e.arena.numel, len(f.opt_state)
    nb = -(-n // 256)
    # 6 P + k P + 4 k ceil(P / 256) against the fp32 state's 6 P + 4 k P (codes are allocated in whole blocks)
    assert f.state_bytes() - e.state_bytes() == k * (4 * n - 256 * nb - 4 * nb) == f.hbm_bytes() - e.hbm_bytes()
    # two warm steps (eager in both), then three eager steps against three graph-replayed ones: the same loss bits
    # on every model, and every state bit on gnmt_tiny, the one model whose forward + backward is bitwise
    # reproducible between two trainer instances (profiles/r7/opt_dtype.md)
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a.opt_state + [a.arena.master], b.opt_state + [b.arena.master]))
    le, lg = [float(e.step()) for _ in range(5)], [float(g.step()) for _ in range(5)]
    assert g._graph is not None and e._graph is None and le == lg
    assert same(e, g) or model != "gnmt_tiny"
    sw = SnapshotWriter(str(tmp_path), gpu)
    try:
        sw.snapshot("q", e)
        sw.flush()
    finally:
        sw.close()
    r = Trainer(model, gpu, seed=4, opt_dtype="q8")                         # the job's seed keys the rounding draws
    assert load_snapshot(sw.path_of("q"), r) == 5 and same(r, e)
    assert all(bool(torch.count_nonzero(s)) for s in r.opt_state)
    le += [float(e.step()) for _ in range(5)]
    lr = [float(r.step()) for _ in range(5)]
    assert lr == le[5:] and (same(r, e) or model != "gnmt_tiny")                                                    # the restored job continues the run
    with pytest.raises(ValueError, match="opt_dtype"):
        load_snapshot(sw.path_of("q"), f)
    le += [float(e.step()) for _ in range(28)]
    torch.cuda.synchronize()
    print(model, "loss", le[0], "->", le[-1])
    assert all(x == x and abs(x) != float("inf") for x in le) and le[-1] < le[0]
