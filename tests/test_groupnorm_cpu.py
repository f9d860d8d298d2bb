"""The ``norm`` knob without a GPU: the CPU GroupNorm path, the trainer and
model option, and the per-job option from ``submit --norm`` to the worker."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tiresias_amd.executor.trainer import Trainer
from tiresias_amd.ops import functional as Fx
from tiresias_amd.ops.arena import Arena


@pytest.mark.parametrize("shape", [(2, 3, 3, 8, 4), (2, 5, 5, 64, 2)])
def test_cpu_path_matches_group_norm(shape):
    """The CPU branch of Fx.groupnorm (what the GPU model test compares
    against) vs F.group_norm in float64, residual and ReLU on."""
    N, H, W, C, G = shape
    torch.manual_seed(1)
    A = Arena(torch.device("cpu"), seed=0)
    g = A.add("g", (C,), init="ones", decay=False, fp32_compute=True)
    b = A.add("b", (C,), init="zeros", decay=False, fp32_compute=True)
    A.materialize()
    g.master.copy_(torch.rand(C) + 0.5)
    b.master.copy_(torch.randn(C))
    x = (torch.randn(N, H, W, C) + 3).bfloat16().requires_grad_(True)
    r = torch.randn(N, H, W, C).bfloat16().requires_grad_(True)
    dy = torch.randn(N, H, W, C).bfloat16()
    y = Fx.groupnorm(x, g, b, G, relu=True, residual=r)
    y.backward(dy)
    xf, rf = x.detach().double().requires_grad_(True), r.detach().double().requires_grad_(True)
    gf, bf = g.master.double().requires_grad_(True), b.master.double().requires_grad_(True)
    yf = (F.group_norm(xf.permute(0, 3, 1, 2), G, gf, bf, 1e-5).permute(0, 2, 3, 1) + rf).clamp_min(0)
    ref = torch.autograd.grad(yf, [xf, rf, gf, bf], dy.double())
    for got, want in zip((y, x.grad, r.grad, g.grad, b.grad), (yf,) + ref):
        assert ((got.double() - want).norm() / want.norm()).item() < 1e-2
    with pytest.raises(ValueError, match="power of two"):
        Fx.groupnorm(x.detach(), g, b, C)                                  # one channel per group


def test_trainer_knob():
    t = Trainer("resnet_tiny", "cpu", seed=2, norm="group")
    assert t.norm == "group" and t.model.buffers() == {} and t.model.bn_buf is None
    assert not any(k.startswith("buf.") for k in t.state_tensors())
    losses = [float(t.step()) for _ in range(2)]
    assert all(l == l and abs(l) != float("inf") for l in losses)
    p = Trainer("resnet_tiny", "cpu", seed=2)
    assert p.norm == "batch" and p.model.buffers()                        # off by default
    assert [q.name for q in p.arena.params] == [q.name for q in t.arena.params]   # same names, same arena order
    assert [q.offset for q in p.arena.params] == [q.offset for q in t.arena.params]
    for m in ("transformer_tiny", "vgg_tiny"):
        with pytest.raises(ValueError, match="no BatchNorm layers"):
            Trainer(m, "cpu", norm="group")
    with pytest.raises(ValueError, match="norm must be"):
        Trainer("resnet_tiny", "cpu", norm="layer")


def test_warm_pool_keeps_the_norms_apart():
    from tiresias_amd.executor.cluster_runtime import Worker

    w = Worker(0, 1, torch.device("cpu"))
    act = {"op": "start", "job": "1", "model": "resnet_tiny", "batch": None, "seed": 1, "ranks": (0,),
           "source": "fresh"}
    bn = w._make_trainer(act)
    assert bn.pool_key == ("resnet_tiny", None, (0,))                     # without the key: today's pool key
    w.pool.setdefault(bn.pool_key, []).append(bn)
    gn = w._make_trainer(dict(act, job="2", seed=2, norm="group"))
    assert gn is not bn and gn.norm == "group" and gn.pool_key != bn.pool_key and w.pool[bn.pool_key] == [bn]
    w.pool.setdefault(gn.pool_key, []).append(gn)
    assert w._make_trainer(dict(act, job="3", seed=3, norm="batch")) is bn
    assert w._make_trainer(dict(act, job="4", seed=4, norm="group")) is gn


def test_snapshot_into_the_other_norm_raises(tmp_path):
    from tiresias_amd.ckpt.snapshot import SnapshotWriter, load_snapshot

    gn, bn = Trainer("resnet_tiny", "cpu", seed=4, norm="group"), Trainer("resnet_tiny", "cpu", seed=4)
    gn.step(), bn.step()
    sw = SnapshotWriter(str(tmp_path), torch.device("cpu"))
    try:
        sw.snapshot("g", gn)
        sw.snapshot("b", bn)
        sw.flush()
    finally:
        sw.close()
    g2 = Trainer("resnet_tiny", "cpu", seed=9, norm="group")
    assert load_snapshot(sw.path_of("g"), g2) == 1 and torch.equal(g2.arena.master, gn.arena.master)
    before = g2.arena.master.clone()
    with pytest.raises(ValueError, match="norm"):
        load_snapshot(sw.path_of("b"), g2)
    with pytest.raises(ValueError, match="norm"):
        load_snapshot(sw.path_of("g"), Trainer("resnet_tiny", "cpu", seed=9))
    assert torch.equal(g2.arena.master, before)                           # nothing written


def test_submit_norm_reaches_the_start_action(tmp_path, monkeypatch):
    import bench
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.cluster_runtime import Controller
    from tiresias_amd.executor.fake import FakeCluster, ProtocolError, VirtualClock
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    inc = os.path.join(sp.root, "incoming")
    assert submit_cli.main(["--spool", sp.root, "--model", "resnet50", "--iterations", "3", "--job-id", "a",
                            "--norm", "group"]) == 0
    assert json.load(open(os.path.join(inc, "a.json")))["norm"] == "group"
    with pytest.raises(SystemExit):
        submit_cli.main(["--spool", sp.root, "--model", "resnet50", "--iterations", "3", "--norm", "layer"])
    # a request without the key is the file it always was
    monkeypatch.setattr("time.time", lambda: 1.0)
    sp.submit("resnet50", 2, iterations=3, job_id="b")
    today = {"job_id": "b", "model": "resnet50", "num_gpu": 2, "iterations": 3, "duration": None, "batch": None,
             "grad_clip": None, "dropout": None, "attn_dropout": None, "opt_dtype": None, "trust_ratio": None,
             "submitted_wall": 1.0}
    assert open(os.path.join(inc, "b.json")).read() == json.dumps(today, indent=1, sort_keys=True)
    monkeypatch.undo()
    for jid, model, v in (("v", "vgg16", "group"), ("t", "transformer", "group"), ("n", "resnet50", 32)):
        with open(os.path.join(inc, f"{jid}.json"), "w") as f:
            json.dump({"job_id": jid, "model": model, "iterations": 2, "norm": v}, f)
    sp.shutdown()
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
        clock.advance(dt if any(r["jobs"] for r in reps) else max(dt, plan.get("wait", 0.0), 1e-6))
        ctrl.apply_reports(reps)
    assert sorted(j.job_id for j in ctrl.sched.finished) == ["a", "b"]
    assert set(os.listdir(os.path.join(sp.root, "rejected"))) == {"v.json", "t.json", "n.json"}
    assert "no BatchNorm layers" in json.load(open(os.path.join(sp.root, "rejected", "v.json")))["reason"]
    assert {a["job"]: a.get("norm") for a in starts} == {"a": "group", "b": None}
    assert all("norm" not in a for a in starts if a["job"] == "b")        # the action as it always was
    assert ctrl.rjobs["a"].norm == "group" and fc.norm == {"a": "group", "b": None}
    with pytest.raises(ProtocolError, match="norm"):
        fc.apply({"actions": [dict(starts[0], norm="layer")]})
