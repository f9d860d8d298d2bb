"""Training dropout without a GPU: the host Philox and the contract's mask,
``Fx.dropout`` on CPU tensors, the CPU trainers of the three models with
dropout sites, resume at a later step, and the per-job option from
``submit --dropout`` to the start action."""
import json
import os

import numpy as np
import pytest
import torch

from tiresias_amd.executor.trainer import Trainer
from tiresias_amd.ops import functional as Fx

BF16 = torch.bfloat16


# ------------------------------------------------------------------ the contract, rebuilt here
def ref_philox(ctr, key):
    """Philox4x32-10 on Python ints, written from the contract alone."""
    c = list(ctr)
    k = list(key)
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def ref_mask(n, site, seed, stream, step, thr):
    """Keep mask of the contract, numpy uint64 arithmetic (its own code path,
    not the one under test)."""
    q = np.arange((n + 7) // 8, dtype=np.uint64)
    M = np.uint64(0xFFFFFFFF)
    c = [q & M, q >> np.uint64(32), np.full_like(q, site), np.full_like(q, step)]
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


def _mulhilo(m, x):
    # 32x32 -> 64 without overflowing uint64: both factors are < 2^32
    p = np.uint64(m) * x
    return p & np.uint64(0xFFFFFFFF), p >> np.uint64(32)


def ref_scale(thr):
    return float(np.float32(65536.0) / np.float32(65536 - thr))


KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_host_philox_known_answers():
    for ctr, key, want in KAT:
        assert tuple(ref_philox(ctr, key)) == want
        got = Fx.philox4x32_10(*[torch.tensor([c], dtype=torch.int64) for c in ctr], *key)
        assert tuple(int(g[0]) for g in got) == want
    # ...and the mask builder consumes it as the contract says
    for thr in (6554, 32768):
        m = Fx.dropout_mask(29, 3, 11, 2, 7, thr)
        assert torch.equal(m, ref_mask(29, 3, 11, 2, 7, thr))
        for i in (0, 7, 8, 28):
            o = ref_philox((i >> 3, 0, 3, 7), (11, 2))
            u = (o[(i & 7) >> 1] >> (16 * (i & 1))) & 0xFFFF
            assert bool(m[i]) == (u >= thr)


def _rec(seed, stream, step):
    return torch.tensor([seed, stream, step, 0], dtype=torch.int32)


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", [8, 24, 4099])
def test_cpu_dropout_equals_the_contract_bitwise(n, p):
    thr = round(p * 65536)
    assert Fx.dropout_threshold(p) == thr and Fx.dropout_scale(thr) == ref_scale(thr)
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(BF16)
    for step in (0, 5):
        Fx.set_dropout(_rec(9, 0, step))
        try:
            for site in (0, 1):                    # two calls = sites 0 and 1
                xg = x.clone().requires_grad_(True)
                y = Fx.dropout(xg, p)
                keep = ref_mask(n, site, 9, 0, step, thr)
                want = torch.where(keep, (x.float() * np.float32(ref_scale(thr))).to(BF16), torch.zeros((), dtype=BF16))
                assert torch.equal(y.view(torch.int16), want.view(torch.int16)), (n, p, step, site)
                dy = torch.randn(n, generator=torch.Generator().manual_seed(site + 1)).to(BF16)
                y.backward(dy)
                dwant = torch.where(keep, (dy.float() * np.float32(ref_scale(thr))).to(BF16),
                                    torch.zeros((), dtype=BF16))
                assert torch.equal(xg.grad.view(torch.int16), dwant.view(torch.int16))
        finally:
            Fx.set_dropout(None)


def test_masks_differ_between_sites_steps_seeds_streams():
    base = dict(site=0, seed=1, stream=0, step=0)
    n, thr = 4096, 32768
    m0 = Fx.dropout_mask(n, thr=thr, **base)
    assert torch.equal(m0, Fx.dropout_mask(n, thr=thr, **base))
    for k in base:
        m1 = Fx.dropout_mask(n, thr=thr, **dict(base, **{k: base[k] + 1}))
        # independent fair masks agree on about half the elements
        agree = int((m0 == m1).sum())
        assert abs(agree - n / 2) < 6 * (n ** 0.5) / 2, (k, agree)
    # the keep rate follows thr
    m = Fx.dropout_mask(1 << 16, 0, 3, 0, 0, 6554)
    q = 1 - 6554 / 65536
    assert abs(int(m.sum()) - (1 << 16) * q) < 6 * ((1 << 16) * q * (1 - q)) ** 0.5


def test_identity_paths_return_the_input_object():
    x = torch.randn(16).to(BF16)
    assert Fx.dropout(x, 0.5) is x                 # no record installed
    Fx.set_dropout(_rec(1, 0, 0))
    try:
        assert Fx.dropout(x, 0) is x and Fx.dropout(x, 0.0) is x and Fx.dropout(x, None) is x
        assert Fx._DROP_SITE == 0                  # identity calls take no site
        assert Fx.dropout(x, 0.5) is not x and Fx._DROP_SITE == 1
        for bad in (-0.1, 1.0, float("nan"), 0.999999):
            with pytest.raises(ValueError, match="dropout"):
                Fx.dropout(x, bad)
    finally:
        Fx.set_dropout(None)


def test_fused_add_layernorm_dropout_cpu_matches_unfused():
    """add_layernorm_skip(drop=p) is layernorm_skip(x + dropout(r)) with the
    contract's mask; its backward hands the masked, scaled gradient to r."""
    from tiresias_amd.ops.arena import Arena

    A = Arena(torch.device("cpu"), seed=0)
    g = A.add("g", (64,), init="ones", decay=False, fp32_compute=True)
    b = A.add("b", (64,), init="zeros", decay=False, fp32_compute=True)
    A.materialize()
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(5, 64, generator=gen).to(BF16).requires_grad_(True)
    r = torch.randn(5, 64, generator=gen).to(BF16).requires_grad_(True)
    thr = round(0.5 * 65536)
    Fx.set_dropout(_rec(4, 1, 2))
    try:
        s, y = Fx.add_layernorm_skip(x, r, g, b, drop=0.5)
    finally:
        Fx.set_dropout(None)
    keep = ref_mask(x.numel(), 0, 4, 1, 2, thr).view(5, 64)
    want = torch.where(keep, (x.float() + r.float() * 2.0).to(BF16), x)
    assert torch.equal(s.view(torch.int16), want.view(torch.int16))
    Fx.set_dropout(_rec(4, 1, 2))
    try:
        (y.float() * torch.randn(5, 64, generator=gen)).sum().backward()
    finally:
        Fx.set_dropout(None)
    assert bool((r.grad[~keep] == 0).all())
    assert torch.equal(r.grad[keep], (x.grad.float() * 2.0).to(BF16)[keep])


# ------------------------------------------------------------------ trainers
MODELS = ["transformer_tiny", "vgg_tiny", "gnmt_tiny"]


def _losses(t, n):
    return [float(t.step()) for _ in range(n)]


@pytest.mark.parametrize("model", MODELS)
def test_cpu_trainer_with_dropout(model):
    a = Trainer(model, "cpu", seed=5, dropout=0.1)
    la = _losses(a, 3)
    assert all(v == v and abs(v) != float("inf") for v in la)
    assert a.dropout == 0.1 and [int(v) for v in a._drop_rec] == [5, 0, 3, 0]
    off = Trainer(model, "cpu", seed=5, dropout=0)
    assert off.dropout is None and off._drop_rec is None
    lo = _losses(off, 3)
    assert lo == _losses(Trainer(model, "cpu", seed=5), 3)          # off is the trainer without the argument
    assert la != lo and la[0] != lo[0]
    assert la == _losses(Trainer(model, "cpu", seed=5, dropout=0.1), 3)   # same seed: bitwise the same
    other = Trainer(model, "cpu", seed=5, dropout=0.1)
    other.seed = 6                                                  # another mask seed, same weights and data
    assert _losses(other, 1)[0] != la[0]


@pytest.mark.parametrize("model", MODELS)
def test_resumed_trainer_continues_the_mask_sequence(model):
    a = Trainer(model, "cpu", seed=2, dropout=0.1)
    la = _losses(a, 3)
    b = Trainer(model, "cpu", seed=2, dropout=0.1)
    _losses(b, 2)
    # a rebuilt trainer (a restore after preemption): state copied in,
    # step_count set; the record is rewritten from (seed, rank, step_count)
    c = Trainer(model, "cpu", seed=2, dropout=0.1)
    for k, v in b.state_tensors().items():
        c.state_tensors()[k].copy_(v)
    assert "drop" not in " ".join(c.state_tensors())                # the record is not job state
    c.step_count = 2
    assert float(c.step()) == la[2]
    assert [int(v) for v in c._drop_rec] == [2, 0, 3, 0]
    # a pooled trainer reset for a new job starts the new seed's sequence
    c.reset(2)
    assert _losses(c, 3) == la


def test_set_dropout_validates_and_drops_the_graph():
    t = Trainer("transformer_tiny", "cpu", seed=0)
    assert t.dropout is None and t._drop_rec is None
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match="dropout"):
            t.set_dropout(bad)
    t._graph = object()
    t.set_dropout(0.25)
    assert t.dropout == 0.25 and t._graph is None and t.model.dropout == 0.25 and t._drop_rec is not None
    t._graph = object()
    t.set_dropout(0.25)
    assert t._graph is not None                                      # unchanged p keeps the graph
    t.set_dropout(None)
    assert t.dropout is None and t._graph is None and t.model.dropout == 0.0
    r = Trainer("resnet_tiny", "cpu", seed=0, dropout=0.5)           # no dropout sites: ignored
    assert r.dropout is None and r._drop_rec is None


def test_gang_members_draw_different_streams(monkeypatch):
    from tiresias_amd.executor import trainer as tr

    l0 = float(Trainer("transformer_tiny", "cpu", seed=3, dropout=0.1).step())      # stream 0
    t = Trainer("transformer_tiny", "cpu", seed=3, dropout=0.1)
    monkeypatch.setattr(tr, "comm_rank", lambda g: 1)
    l1 = float(t.step())
    assert [int(v) for v in t._drop_rec] == [3, 1, 1, 0]
    assert l1 != l0


# ------------------------------------------------------------------ submission
def _fake_controller_run(sp):
    import bench
    from tiresias_amd.executor.cluster_runtime import Controller
    from tiresias_amd.executor.fake import FakeCluster, VirtualClock

    cfg = bench.make_cfg("dlas-gpu", "tiresias", 2, 3, "none", [0.05, 0.25, 1.0], False)
    clock = VirtualClock()
    ctrl = Controller(cfg, [], 2, 0.05, spool=sp, clock=clock)
    fc = FakeCluster(2, vnode_size=ctrl.vnode_size, nic_gbps=ctrl.nic_gbps)
    ctrl.start_clock()
    starts = []
    for _ in range(10000):
        plan = ctrl.plan_round()
        starts += [a for a in plan["actions"] if a["op"] == "start"]
        cost = fc.apply(plan)
        if plan["stop"]:
            break
        reps, dt = fc.run(plan, clock(), cost)
        if not any(r["jobs"] for r in reps):
            dt = max(dt, plan.get("wait", 0.0), 1e-6)
        clock.advance(dt)
        ctrl.apply_reports(reps)
    else:
        raise AssertionError("controller did not stop")
    return ctrl, starts


def test_submit_dropout_reaches_the_start_action(tmp_path):
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    assert submit_cli.main(["--spool", sp.root, "--model", "transformer", "--iterations", "3", "--job-id", "a",
                            "--dropout", "0.1"]) == 0
    assert json.load(open(os.path.join(sp.root, "incoming", "a.json")))["dropout"] == 0.1
    sp.submit("vgg16", 2, iterations=3, job_id="b", dropout=0.5)     # a gang
    sp.submit("gnmt", 1, iterations=3, job_id="c")
    assert json.load(open(os.path.join(sp.root, "incoming", "c.json")))["dropout"] is None
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)
    assert len(ctrl.sched.finished) == 3
    assert {a["job"]: a["dropout"] for a in starts} == {"a": 0.1, "b": 0.5, "c": None}
    assert ctrl.rjobs["a"].dropout == 0.1 and ctrl.rjobs["c"].dropout is None


def test_controller_validates_dropout(tmp_path):
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    inc = os.path.join(sp.root, "incoming")
    base = {"model": "vgg16", "iterations": 2}
    bad = {"neg": -0.1, "one": 1.0, "nan": float("nan"), "str": "x"}
    good = {"zero": 0, "p3": 0.3}
    for name, v in {**bad, **good}.items():
        with open(os.path.join(inc, f"{name}.json"), "w") as f:
            json.dump(dict(base, job_id=name, dropout=v), f)
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)
    assert sorted(j.job_id for j in ctrl.sched.finished) == sorted(good)
    assert set(os.listdir(os.path.join(sp.root, "rejected"))) == {f"{n}.json" for n in bad}
    for name in bad:
        why = json.load(open(os.path.join(sp.root, "rejected", f"{name}.json")))["reason"]
        assert "dropout" in why, (name, why)
    assert {a["job"]: a["dropout"] for a in starts} == {"zero": 0.0, "p3": 0.3}
    # the validator itself raises ValueError with the reason
    for v in bad.values():
        with pytest.raises(ValueError, match="dropout"):
            ctrl._validate(dict(base, job_id="x", dropout=v))


def test_worker_passes_dropout_to_new_and_pooled_trainers():
    from tiresias_amd.executor.cluster_runtime import Worker

    w = Worker(0, 1, torch.device("cpu"))
    act = {"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1, "ranks": (0,),
           "source": "fresh", "dropout": 0.2}
    t = w._make_trainer(act)
    assert t.dropout == 0.2 and t.model.dropout == 0.2
    w.pool.setdefault(t.pool_key, []).append(t)
    t2 = w._make_trainer(dict(act, job="2", seed=2, dropout=None))
    assert t2 is t and t2.dropout is None and t2.model.dropout == 0.0
    w.pool.setdefault(t.pool_key, []).append(t)
    t3 = w._make_trainer(dict(act, job="3", seed=3))
    assert t3 is t and t3.dropout == 0.2
    float(t3.step())
    assert [int(v) for v in t3._drop_rec] == [3, 0, 1, 0]           # the new job's seed, from step 0
