"""Global-norm gradient clipping without a GPU: the Trainer's plain-torch
mirror of the device path, a gloo world-2 gang, the sharded-gang rejection,
and the per-job option from ``submit --grad-clip`` to the start action."""
import json
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tiresias_amd.executor.trainer import Trainer


def _adam_ref(w, g, m, v, scale, lr, step):
    """AdamW of the tiny seq2seq recipes (wd 0) in fp64 on the scaled gradient."""
    gr = g.double() * scale
    m = 0.9 * m.double() + 0.1 * gr
    v = 0.98 * v.double() + 0.02 * gr * gr
    w = w.double() - lr * ((m / (1 - 0.9 ** step)) / ((v / (1 - 0.98 ** step)).sqrt() + 1e-9))
    return w, m, v


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def test_cpu_trainer_norm_and_clipped_update():
    t = Trainer("transformer_tiny", "cpu", seed=3, grad_clip=1e30)
    assert t.spec.wd == 0.0 and t.opt == "adam"
    t.step()
    assert t.clip_stats()["last_scale"] == 1.0 and t.clip_stats()["clipped_steps"] == 0
    t._fwd_bwd()
    g = t.arena.grad.clone()
    ref = float(g.double().norm())
    w0, m0, v0 = t.arena.master.clone(), t.opt_state[0].clone(), t.opt_state[1].clone()
    t.set_grad_clip(0.5 * ref)
    t._opt_step()
    st = t.clip_stats()
    assert abs(st["last_norm"] - ref) / ref <= 1e-6
    assert st["last_scale"] == pytest.approx(0.5 * ref / (ref + 1e-6), rel=1e-6)
    assert st["clipped_steps"] == 1 and st["nonfinite_steps"] == 0
    w, m, v = _adam_ref(w0, g, m0, v0, st["last_scale"], t.lr, t.step_count)
    assert _rel(t.arena.master, w) < 1e-5
    assert _rel(t.opt_state[0], m) < 1e-5 and _rel(t.opt_state[1], v) < 1e-5
    assert torch.count_nonzero(t.arena.grad) == 0
    # the unclipped update is a different one (the check above can tell)
    w1, _, _ = _adam_ref(w0, g, m0, v0, 1.0, t.lr, t.step_count)
    assert _rel(w1, w) > 1e-4
    t.reset(4)
    st = t.clip_stats()
    assert st["clipped_steps"] == 0 and st["nonfinite_steps"] == 0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_cpu_trainer_skips_nonfinite_step(bad):
    t = Trainer("transformer_tiny", "cpu", seed=3, grad_clip=1.0)
    t.step()
    t._fwd_bwd()
    t.arena.grad[1234] = bad
    before = [t.arena.master.clone(), t.arena.shadow.clone()] + [s.clone() for s in t.opt_state]
    k = t.step_count
    t._opt_step()
    after = [t.arena.master, t.arena.shadow] + list(t.opt_state)
    for a, b in zip(after, before):
        assert torch.equal(a, b)
    assert torch.count_nonzero(t.arena.grad) == 0
    st = t.clip_stats()
    assert st["nonfinite_steps"] == 1 and st["last_scale"] == -1.0 and not math.isfinite(st["last_norm"])
    assert t.step_count == k + 1          # a skipped step still counts, like a guarded LSTM step
    t.step()                              # a clean step updates again
    assert not torch.equal(t.arena.master, before[0])
    assert t.clip_stats()["nonfinite_steps"] == 1


def test_clip_off_by_default_and_validated():
    from tiresias_amd.models import MODELS

    assert all(s.clip is None for s in MODELS.values())
    t = Trainer("transformer_tiny", "cpu", seed=3)
    assert t.grad_clip is None and t._clip is None
    for v in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="grad_clip"):
            t.set_grad_clip(v)
    t.set_grad_clip(2.0)
    assert t.grad_clip == 2.0
    t.set_grad_clip(None)
    assert t.grad_clip is None


def test_grad_clip_with_sharded_gang_is_rejected():
    class _Comm:            # a 2-member gang comm (parallel/gang.py comm_size reads .size)
        size = 2
        ranks = (0, 1)

    with pytest.raises(ValueError, match="ddp_shard"):
        Trainer("transformer_tiny", "cpu", grad_clip=1.0, ddp_shard=True, group=_Comm())
    t = Trainer("transformer_tiny", "cpu")

    class _D:
        shard, dirty = True, False

    t.ddp = _D()
    with pytest.raises(ValueError, match="ddp_shard"):
        t.set_grad_clip(1.0)


# ------------------------------------------------------------------ gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gang_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    # the reduced gradient of the first step, by hand
    loc = Trainer("transformer_tiny", "cpu", seed=5, data_seed=70 + rank)
    loc._fwd_bwd()
    g = loc.arena.grad.clone()
    dist.all_reduce(g)
    ref = float((g.double() / world).norm())
    t = Trainer("transformer_tiny", "cpu", seed=5, data_seed=70 + rank, group=dist.group.WORLD, bucket_mb=0.1,
                grad_clip=0.25 * ref)
    t.step()
    st = t.clip_stats()
    for _ in range(2):
        t.step()
    w = t.arena.master.clone()
    ws = [torch.zeros_like(w) for _ in range(world)]
    dist.all_gather(ws, w)
    q.put((rank, ref, st, all(torch.equal(ws[0], x) for x in ws), t.clip_stats()["clipped_steps"]))
    dist.destroy_process_group()


def test_gang_members_clip_alike_without_a_collective():
    world = 2
    q = mp.get_context("spawn").SimpleQueue()
    mp.spawn(_gang_worker, args=(world, _free_port(), q), nprocs=world, join=True)
    res = sorted(q.get() for _ in range(world))
    (_, ref0, st0, same0, n0), (_, ref1, st1, same1, n1) = res
    assert st0["last_norm"] == st1["last_norm"] and st0["last_scale"] == st1["last_scale"]
    assert abs(st0["last_norm"] - ref0) / ref0 <= 1e-6 and ref0 == ref1
    assert st0["clipped_steps"] == 1 and st0["last_scale"] == pytest.approx(0.25, rel=1e-4)
    assert same0 and same1
    assert n0 == n1 >= 1


# ------------------------------------------------------------------ submission
def _fake_controller_run(sp):
    """The live controller over a spool against the fake backend (virtual
    time); returns (summary-ish, every start action it planned)."""
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


def test_submit_grad_clip_reaches_the_start_action(tmp_path):
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    assert submit_cli.main(["--spool", sp.root, "--model", "resnet50", "--iterations", "3", "--job-id", "a",
                            "--grad-clip", "5"]) == 0
    req = json.load(open(os.path.join(sp.root, "incoming", "a.json")))
    assert req["grad_clip"] == 5.0
    sp.submit("resnet50", 1, iterations=3, job_id="b")
    sp.submit("vgg16", 2, iterations=3, job_id="c", grad_clip=0.5)
    assert json.load(open(os.path.join(sp.root, "incoming", "b.json")))["grad_clip"] is None
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)
    assert len(ctrl.sched.finished) == 3
    clip = {a["job"]: a["grad_clip"] for a in starts}
    assert clip == {"a": 5.0, "b": None, "c": 0.5}
    assert ctrl.rjobs["a"].grad_clip == 5.0 and ctrl.rjobs["b"].grad_clip is None


def test_bad_grad_clip_is_rejected_not_fatal(tmp_path):
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    inc = os.path.join(sp.root, "incoming")
    base = {"model": "resnet50", "iterations": 2}
    bad = {"neg": -1, "zero": 0, "str": "x", "bool": True, "nan": float("nan"), "inf": float("inf")}
    for name, v in bad.items():
        with open(os.path.join(inc, f"{name}.json"), "w") as f:
            json.dump(dict(base, job_id=name, grad_clip=v), f)
    sp.submit("resnet50", 1, iterations=2, job_id="ok", grad_clip=1.5)
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)
    assert [j.job_id for j in ctrl.sched.finished] == ["ok"]
    assert set(os.listdir(os.path.join(sp.root, "rejected"))) == {f"{n}.json" for n in bad}
    assert os.listdir(inc) == []
    for name in bad:
        why = json.load(open(os.path.join(sp.root, "rejected", f"{name}.json")))["reason"]
        assert "grad_clip" in why, (name, why)
    assert [a["grad_clip"] for a in starts] == [1.5]


def test_worker_passes_grad_clip_to_new_and_pooled_trainers():
    from tiresias_amd.executor.cluster_runtime import Worker

    w = Worker(0, 1, torch.device("cpu"))
    act = {"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1, "ranks": (0,),
           "source": "fresh", "grad_clip": 3.0}
    t = w._make_trainer(act)
    assert t.grad_clip == 3.0
    w.pool.setdefault(t.pool_key, []).append(t)
    t2 = w._make_trainer(dict(act, job="2", seed=2, grad_clip=None))
    assert t2 is t and t2.grad_clip is None          # same pool key, the new job's own setting
    w.pool.setdefault(t.pool_key, []).append(t)
    del act["grad_clip"]                             # an action without the key: off
    assert w._make_trainer(act).grad_clip is None
