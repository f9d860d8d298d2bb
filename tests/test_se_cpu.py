"""The ``se_ratio`` knob without a GPU: the model and trainer option, the CPU
path of ``Fx.se_block``, and the per-job option from ``submit --se-ratio`` to
the start action."""
import hashlib
import json
import os

import pytest
import torch

from tiresias_amd.executor.trainer import Trainer, check_se_ratio

# sha256 of "name:shape:offset;..." over resnet_tiny's parameters, and its first
# two losses at seed 2, recorded before the knob existed
PLAIN_SIG = "287f22c95c7940351161a5aa224e333ae7e5268713987fea2fe309e347b36ea3"
PLAIN_LOSSES = ["0x1.6837cc0000000p+1", "0x1.531f900000000p-1"]


def test_plain_model_is_unchanged():
    t, n = Trainer("resnet_tiny", "cpu", seed=2), Trainer("resnet_tiny", "cpu", seed=2, se_ratio=None)
    sig = ";".join(f"{p.name}:{tuple(p.shape)}:{p.offset}" for p in t.arena.params)
    assert hashlib.sha256(sig.encode()).hexdigest() == PLAIN_SIG
    assert t.se_ratio is None and t.model.se_ratio is None
    assert [float(t.step()).hex() for _ in range(2)] == PLAIN_LOSSES
    assert [float(n.step()).hex() for _ in range(2)] == PLAIN_LOSSES


def test_se_ratio_adds_four_parameters_per_block():
    plain, t = Trainer("resnet_tiny", "cpu", seed=2), Trainer("resnet_tiny", "cpu", seed=2, se_ratio=16)
    added = {p.name: (tuple(p.shape), p.decay) for p in t.arena.params} \
        .items() - {p.name: (tuple(p.shape), p.decay) for p in plain.arena.params}.items()
    want = {}
    for i, blk in enumerate(t.model.blocks):
        C, pre = 4 * 8 * 2 ** i, blk["pre"]
        cr = max(8, C // 16)
        want.update({f"{pre}.se.w1": ((cr, C), True), f"{pre}.se.b1": ((cr,), False),
                     f"{pre}.se.w2": ((C, cr), True), f"{pre}.se.b2": ((C,), False)})
        assert float(blk["bn3"][0].master.abs().max()) == 0.0          # gamma keeps its zero init
    assert dict(added) == want
    names = [p.name for p in t.arena.params]
    assert names[names.index("s0.b0.dbn.b") + 1:][:4] == ["s0.b0.se.w1", "s0.b0.se.b1", "s0.b0.se.w2", "s0.b0.se.b2"]
    losses = [float(t.step()) for _ in range(4)]
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("bad", [2, 12, 64, "16", 16.0, True])
def test_invalid_values_raise(bad):
    with pytest.raises(ValueError, match="se_ratio"):
        Trainer("resnet_tiny", "cpu", se_ratio=bad)
    with pytest.raises(ValueError, match="se_ratio"):
        check_se_ratio("resnet50", bad)


@pytest.mark.parametrize("model", ["vgg_tiny", "transformer_tiny"])
def test_models_without_a_bottleneck_reject_it(model):
    with pytest.raises(ValueError, match="no bottleneck"):
        Trainer(model, "cpu", se_ratio=16)


def test_snapshot_into_another_se_ratio_raises(tmp_path):
    from tiresias_amd.ckpt.snapshot import SnapshotWriter, load_snapshot

    s16 = Trainer("resnet_tiny", "cpu", seed=4, se_ratio=16)
    s16.step()
    sw = SnapshotWriter(str(tmp_path), torch.device("cpu"))
    try:
        sw.snapshot("s16", s16)
        sw.flush()
    finally:
        sw.close()
    again = Trainer("resnet_tiny", "cpu", seed=9, se_ratio=16)
    assert load_snapshot(sw.path_of("s16"), again) == 1 and torch.equal(again.arena.master, s16.arena.master)
    for other in (None, 8):
        t = Trainer("resnet_tiny", "cpu", seed=9, se_ratio=other)
        before = t.arena.master.clone()
        with pytest.raises(ValueError, match="se_ratio"):
            load_snapshot(sw.path_of("s16"), t)
        assert torch.equal(t.arena.master, before)                        # nothing written


def test_submit_se_ratio_reaches_the_start_action(tmp_path):
    import bench
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.cluster_runtime import Controller, Worker
    from tiresias_amd.executor.fake import FakeCluster, ProtocolError, VirtualClock
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    inc = os.path.join(sp.root, "incoming")
    assert submit_cli.main(["--spool", sp.root, "--model", "resnet50", "--iterations", "3", "--job-id", "a",
                            "--se-ratio", "16"]) == 0
    assert json.load(open(os.path.join(inc, "a.json")))["se_ratio"] == 16
    assert submit_cli.main(["--spool", sp.root, "--model", "resnet50", "--iterations", "3", "--job-id", "b"]) == 0
    assert "se_ratio" not in json.load(open(os.path.join(inc, "b.json")))   # written only when asked
    for jid, model, v in (("v", "vgg16", 16), ("t", "transformer", 16), ("n", "resnet50", 3), ("s", "resnet50", "16")):
        with open(os.path.join(inc, f"{jid}.json"), "w") as f:
            json.dump({"job_id": jid, "model": model, "iterations": 2, "se_ratio": v}, f)
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
    assert set(os.listdir(os.path.join(sp.root, "rejected"))) == {"v.json", "t.json", "n.json", "s.json"}
    assert "no bottleneck" in json.load(open(os.path.join(sp.root, "rejected", "v.json")))["reason"]
    assert {a["job"]: a.get("se_ratio") for a in starts} == {"a": 16, "b": None}
    assert all("se_ratio" not in a for a in starts if a["job"] == "b")     # the action as it always was
    assert fc.se == {"a": 16, "b": None}
    with pytest.raises(ProtocolError, match="se_ratio"):
        fc.apply({"actions": [dict(starts[0], se_ratio=3)]})
    # the worker's warm pool keeps the ratios apart
    act = {"op": "start", "job": "1", "model": "resnet_tiny", "batch": None, "seed": 1, "ranks": (0,)}
    plain, s16 = Worker._pool_key(act), Worker._pool_key(dict(act, se_ratio=16))
    assert plain == ("resnet_tiny", None, (0,)) and s16 != plain and s16 != Worker._pool_key(dict(act, se_ratio=8))
