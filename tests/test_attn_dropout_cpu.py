"""Attention-probability dropout without a GPU: the torch mask against the
contract rebuilt in numpy, the CPU ``_Attn`` path with ``drop``, the trainer
knob, and the per-job option from ``submit --attn-dropout`` to the worker."""
import json
import os

import numpy as np
import pytest
import torch

from tiresias_amd.executor.trainer import Trainer
from tiresias_amd.ops import functional as Fx

BF16 = torch.bfloat16
# two fp32 evaluations of one formula, each rounded to bf16: elements differ by
# at most one bf16 ulp (2^-8 relative); a wrong mask gives an error of order 1
TOL = 2.0 ** -8


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


# ------------------------------------------------------------------ the contract, rebuilt here
def _mulhilo(m, x):
    p = np.uint64(m) * x                       # both factors < 2^32: no overflow
    return p & np.uint64(0xFFFFFFFF), p >> np.uint64(32)


def ref_attn_mask(B, H, Sq, Sk, site, seed, stream, step, thr):
    """Keep mask [B,H,Sq,Sk] written from the contract text (tam/philox.h):
    block (Q, K) = (q >> 2, kv >> 2), counter (K | Q << 16, b*H + h,
    0x80000000 | a, step), key (seed, stream), 8 bits per probability."""
    nq, nk = (Sq + 3) // 4, (Sk + 3) // 4
    bh, Q, K = np.meshgrid(np.arange(B * H, dtype=np.uint64), np.arange(nq, dtype=np.uint64),
                           np.arange(nk, dtype=np.uint64), indexing="ij")
    c = [K | (Q << np.uint64(16)), bh, np.full_like(bh, 0x80000000 | site), np.full_like(bh, step)]
    k = [seed & 0xFFFFFFFF, stream & 0xFFFFFFFF]
    for _ in range(10):
        lo0, hi0 = _mulhilo(0xD2511F53, c[0])
        lo1, hi1 = _mulhilo(0xCD9E8D57, c[2])
        c = [hi1 ^ c[1] ^ np.uint64(k[0]), lo1, hi0 ^ c[3] ^ np.uint64(k[1]), lo0]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    keep = np.zeros((B * H, 4 * nq, 4 * nk), dtype=bool)
    for qi in range(4):
        for ki in range(4):
            keep[:, qi::4, ki::4] = ((c[qi] >> np.uint64(8 * ki)) & np.uint64(0xFF)) >= np.uint64(thr)
    return torch.from_numpy(keep[:, :Sq, :Sk].reshape(B, H, Sq, Sk).copy())


def ref_philox(ctr, key):
    """Philox4x32-10 on Python ints."""
    c = list(ctr)
    k = list(key)
    for _ in range(10):
        p0 = 0xD2511F53 * c[0]
        p1 = 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


# ------------------------------------------------------------------ mask function
def test_mask_equals_the_contract():
    B, H, Sq, Sk = 2, 3, 37, 50
    for thr in (26, 128):
        m = Fx.attn_dropout_mask(B, H, Sq, Sk, 2, 11, 1, 7, thr)
        assert m.shape == (B, H, Sq, Sk) and m.dtype == torch.bool
        assert torch.equal(m, ref_attn_mask(B, H, Sq, Sk, 2, 11, 1, 7, thr))
        # ...and single positions straight from the text, on Python ints
        for b, h, q, kv in [(0, 0, 0, 0), (1, 2, 36, 49), (0, 1, 5, 18), (1, 0, 22, 3)]:
            o = ref_philox(((kv >> 2) | ((q >> 2) << 16), b * H + h, 0x80000000 | 2, 7), (11, 1))
            u = (o[q & 3] >> (8 * (kv & 3))) & 0xFF
            assert bool(m[b, h, q, kv]) == (u >= thr)
    # another ordinal, step or stream is another mask
    base = Fx.attn_dropout_mask(B, H, Sq, Sk, 2, 11, 1, 7, 128)
    for args in [(3, 11, 1, 7), (2, 12, 1, 7), (2, 11, 0, 7), (2, 11, 1, 8)]:
        assert not torch.equal(Fx.attn_dropout_mask(B, H, Sq, Sk, *args, 128), base)


def test_threshold_and_scale():
    assert Fx.attn_dropout_threshold(0.1) == 26                  # p is quantised to 1/256
    assert Fx.attn_dropout_threshold(0.5) == 128
    assert Fx.attn_dropout_threshold(0) == 0 and Fx.attn_dropout_threshold(0.001) == 0
    assert Fx.attn_dropout_threshold(0.998) == 255
    for bad in (-0.1, 1.0, float("nan"), 0.9999, 255.5 / 256):
        with pytest.raises(ValueError, match="attn_dropout"):
            Fx.attn_dropout_threshold(bad)
    assert Fx.attn_dropout_scale(26) == float(np.float32(256.0) / np.float32(230.0))
    assert Fx.attn_dropout_scale(128) == 2.0


# ------------------------------------------------------------------ CPU _Attn with drop
def _masked_ref(q, k, v, causal, keep, dscale):
    qf, kf, vf = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) / 8.0
    if causal:
        S = s.shape[-1]
        s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    p = torch.where(keep, torch.softmax(s, -1), torch.zeros(())) * dscale
    return (p @ vf).permute(0, 2, 1, 3)


@pytest.mark.parametrize("causal", [False, True])
def test_cpu_attention_applies_the_mask(causal):
    B, H, S = 2, 3, 21
    gen = torch.Generator().manual_seed(2)
    qkv = torch.randn(B, S, 3 * H * 64, generator=gen).to(BF16).requires_grad_(True)
    rec = torch.tensor([11, 1, 7, 0], dtype=torch.int32)
    Fx.set_dropout(rec)
    try:
        o_first = Fx.self_attention(qkv, H, causal=causal, drop=0.5)          # attention site 0
        o = Fx.self_attention(qkv, H, causal=causal, drop=0.5)                # attention site 1
        o_off = Fx.self_attention(qkv, H, causal=causal)
    finally:
        Fx.set_dropout(None)
    keep = ref_attn_mask(B, H, S, S, 1, 11, 1, 7, 128)
    v5 = qkv.detach().view(B, S, 3, H, 64)
    qf, kf, vf = (v5[:, :, i].float().requires_grad_(True) for i in range(3))
    of = _masked_ref(qf, kf, vf, causal, keep, 2.0)
    assert rel_err(o.detach().view(B, S, H, 64), of.detach().to(BF16)) < TOL
    assert not torch.equal(o.detach(), o_first.detach()) and not torch.equal(o.detach(), o_off.detach())
    do = torch.randn(B, S, H * 64, generator=gen).to(BF16)
    (g,) = torch.autograd.grad(o, qkv, do)
    gq, gk, gv = torch.autograd.grad(of, [qf, kf, vf], do.view(B, S, H, 64).float())
    want = torch.stack([gq, gk, gv], 2).to(BF16).view(B, S, 3 * H * 64)
    assert rel_err(g, want) < TOL
    # no record installed, or p that rounds to 0: the call as it was
    assert torch.equal(Fx.self_attention(qkv, H, causal=causal, drop=0.5).detach(), o_off.detach())
    Fx.set_dropout(rec)
    try:
        assert torch.equal(Fx.self_attention(qkv, H, causal=causal, drop=0.001).detach(), o_off.detach())
        assert Fx._attn_drop_args(0.001) is None and Fx._attn_drop_args(0.5)[1] == 0   # no ordinal consumed
    finally:
        Fx.set_dropout(None)


def test_cross_attention_takes_drop():
    B, H, Sq, Sk = 2, 3, 9, 14
    gen = torch.Generator().manual_seed(4)
    q = torch.randn(B, Sq, H * 64, generator=gen).to(BF16)
    kv = torch.randn(B, Sk, 2 * H * 64, generator=gen).to(BF16)
    Fx.set_dropout(torch.tensor([3, 0, 2, 0], dtype=torch.int32))
    try:
        o = Fx.cross_attention(q, kv, H, drop=0.1)
    finally:
        Fx.set_dropout(None)
    keep = ref_attn_mask(B, H, Sq, Sk, 0, 3, 0, 2, 26)
    kv5 = kv.view(B, Sk, 2, H, 64)
    of = _masked_ref(q.view(B, Sq, H, 64).float(), kv5[:, :, 0].float(), kv5[:, :, 1].float(), False, keep,
                     Fx.attn_dropout_scale(26))
    assert rel_err(o.view(B, Sq, H, 64), of.to(BF16)) < TOL
    assert rel_err(o.view(B, Sq, H, 64), _masked_ref(q.view(B, Sq, H, 64).float(), kv5[:, :, 0].float(),
                                                     kv5[:, :, 1].float(), False, ~keep, 1.0)) > 0.5


# ------------------------------------------------------------------ trainer
def test_trainer_knob():
    t = Trainer("transformer_tiny", "cpu", seed=3)
    assert t.attn_dropout is None and t._drop_rec is None and t.model.attn_dropout == 0.0
    plain = [float(t.step()) for _ in range(2)]
    a = Trainer("transformer_tiny", "cpu", seed=3, attn_dropout=0.5)
    assert a.attn_dropout == 0.5 and a.model.attn_dropout == 0.5 and a.dropout is None
    la = [float(a.step()) for _ in range(2)]
    assert [int(v) for v in a._drop_rec] == [3, 0, 2, 0]             # one advance per step
    assert la != plain and la[0] != plain[0]
    b = Trainer("transformer_tiny", "cpu", seed=3, dropout=0.1, attn_dropout=0.5)
    lb = [float(b.step()) for _ in range(2)]
    assert [int(v) for v in b._drop_rec] == [3, 0, 2, 0]             # ...also with both knobs on
    assert lb != la
    # the same sequence again, and a change of p drops the graph
    a2 = Trainer("transformer_tiny", "cpu", seed=3)
    a2._graph = object()
    a2.set_attn_dropout(0.5)
    assert a2._graph is None and a2._drop_rec is not None
    assert [float(a2.step()) for _ in range(2)] == la
    a2._graph = object()
    a2.set_attn_dropout(0.5)
    assert a2._graph is not None                                     # unchanged p keeps it
    a2.set_attn_dropout(None)
    assert a2.attn_dropout is None and a2._graph is None and a2.model.attn_dropout == 0.0
    with pytest.raises(ValueError, match="attn_dropout"):
        a2.set_attn_dropout(1.0)
    # models without the attribute ignore it
    r = Trainer("vgg_tiny", "cpu", seed=0, attn_dropout=0.5)
    assert r.attn_dropout is None and r._drop_rec is None
    g = Trainer("gnmt_tiny", "cpu", seed=0, attn_dropout=0.5)
    assert g.attn_dropout is None and g._drop_rec is None


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


def test_submit_attn_dropout_reaches_the_start_action(tmp_path):
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    assert submit_cli.main(["--spool", sp.root, "--model", "transformer", "--iterations", "3", "--job-id", "a",
                            "--attn-dropout", "0.1"]) == 0
    req = json.load(open(os.path.join(sp.root, "incoming", "a.json")))
    assert req["attn_dropout"] == 0.1 and req["dropout"] is None
    sp.submit("transformer", 2, iterations=3, job_id="b", dropout=0.1, attn_dropout=0.5)     # a gang
    sp.submit("gnmt", 1, iterations=3, job_id="c")
    assert json.load(open(os.path.join(sp.root, "incoming", "c.json")))["attn_dropout"] is None
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)
    assert len(ctrl.sched.finished) == 3
    assert {a["job"]: a["attn_dropout"] for a in starts} == {"a": 0.1, "b": 0.5, "c": None}
    assert {a["job"]: a["dropout"] for a in starts} == {"a": None, "b": 0.1, "c": None}
    assert ctrl.rjobs["a"].attn_dropout == 0.1 and ctrl.rjobs["c"].attn_dropout is None


def test_controller_validates_attn_dropout(tmp_path):
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    inc = os.path.join(sp.root, "incoming")
    base = {"model": "transformer", "iterations": 2}
    bad = {"neg": -0.1, "one": 1.0, "nan": float("nan"), "str": "x", "bool": True, "r256": 0.999}
    good = {"zero": 0, "p3": 0.3}
    for name, v in {**bad, **good}.items():
        with open(os.path.join(inc, f"{name}.json"), "w") as f:
            json.dump(dict(base, job_id=name, attn_dropout=v), f)
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)
    assert sorted(j.job_id for j in ctrl.sched.finished) == sorted(good)
    assert set(os.listdir(os.path.join(sp.root, "rejected"))) == {f"{n}.json" for n in bad}
    for name in bad:
        why = json.load(open(os.path.join(sp.root, "rejected", f"{name}.json")))["reason"]
        assert "attn_dropout" in why, (name, why)
    assert {a["job"]: a["attn_dropout"] for a in starts} == {"zero": 0.0, "p3": 0.3}
    for v in bad.values():
        with pytest.raises(ValueError, match="attn_dropout"):
            ctrl._validate(dict(base, job_id="x", attn_dropout=v))


def test_worker_passes_attn_dropout_to_new_and_pooled_trainers():
    from tiresias_amd.executor.cluster_runtime import Worker

    w = Worker(0, 1, torch.device("cpu"))
    act = {"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1, "ranks": (0,),
           "source": "fresh", "attn_dropout": 0.25}
    t = w._make_trainer(act)
    assert t.attn_dropout == 0.25 and t.model.attn_dropout == 0.25 and t.dropout is None
    w.pool.setdefault(t.pool_key, []).append(t)
    t2 = w._make_trainer(dict(act, job="2", seed=2, attn_dropout=None))
    assert t2 is t and t2.attn_dropout is None and t2.model.attn_dropout == 0.0
    w.pool.setdefault(t.pool_key, []).append(t)
    no_key = {k: v for k, v in act.items() if k != "attn_dropout"}
    t3 = w._make_trainer(dict(no_key, job="3", seed=3))                # an action without the key: off
    assert t3 is t and t3.attn_dropout is None
    w.pool.setdefault(t.pool_key, []).append(t)
    t4 = w._make_trainer(dict(act, job="4", seed=4))
    assert t4 is t and t4.attn_dropout == 0.25
    float(t4.step())
    assert [int(v) for v in t4._drop_rec] == [4, 0, 1, 0]             # the new job's seed, from step 0
