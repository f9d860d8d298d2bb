"""The ``cardinality`` knob without a GPU: the model and trainer option, the
CPU grouped-conv path, and the per-job option from ``submit --cardinality``
to the start action."""
import hashlib
import json
import os

import pytest
import torch

from tiresias_amd.executor.trainer import Trainer, check_cardinality

# sha256 of "name:shape:offset;..." over resnet_tiny's parameters, and its first
# two losses at seed 2, recorded before the knob existed
PLAIN_SIG = "287f22c95c7940351161a5aa224e333ae7e5268713987fea2fe309e347b36ea3"
PLAIN_LOSSES = ["0x1.6837cc0000000p+1", "0x1.531f900000000p-1"]


def test_plain_model_is_unchanged():
    t, n = Trainer("resnet_tiny", "cpu", seed=2), Trainer("resnet_tiny", "cpu", seed=2, cardinality=None)
    sig = ";".join(f"{p.name}:{tuple(p.shape)}:{p.offset}" for p in t.arena.params)
    assert hashlib.sha256(sig.encode()).hexdigest() == PLAIN_SIG
    assert t.cardinality is None and t.model.cardinality is None
    assert [float(t.step()).hex() for _ in range(2)] == PLAIN_LOSSES
    assert [float(n.step()).hex() for _ in range(2)] == PLAIN_LOSSES


def test_cardinality_builds_grouped_bottlenecks():
    t = Trainer("resnet_tiny", "cpu", seed=2, cardinality=4)
    for i, blk in enumerate(t.model.blocks):
        width = 4 * 4 * 2 ** i
        assert tuple(blk["c2"].shape) == (width, 3, 3, width // 4)
        assert blk["c1"].shape[0] == width and blk["c3"].shape[3] == width and blk["bn2"][0].shape == (width,)
    assert not any(p is blk["c2"] for blk in t.model.blocks for p in t.model.conv_params())
    losses = [float(t.step()) for _ in range(4)]
    assert losses[-1] < losses[0]


@pytest.mark.parametrize("bad", [3, 2, 128, "32", True])
def test_invalid_values_raise(bad):
    with pytest.raises(ValueError, match="cardinality"):
        Trainer("resnet_tiny", "cpu", cardinality=bad)
    with pytest.raises(ValueError, match="cardinality"):
        check_cardinality("resnet50", bad)


@pytest.mark.parametrize("model", ["vgg_tiny", "transformer_tiny"])
def test_models_without_a_bottleneck_reject_it(model):
    with pytest.raises(ValueError, match="no bottleneck"):
        Trainer(model, "cpu", cardinality=4)


def test_snapshot_into_another_cardinality_raises(tmp_path):
    from tiresias_amd.ckpt.snapshot import SnapshotWriter, load_snapshot

    c4 = Trainer("resnet_tiny", "cpu", seed=4, cardinality=4)
    c4.step()
    sw = SnapshotWriter(str(tmp_path), torch.device("cpu"))
    try:
        sw.snapshot("c4", c4)
        sw.flush()
    finally:
        sw.close()
    again = Trainer("resnet_tiny", "cpu", seed=9, cardinality=4)
    assert load_snapshot(sw.path_of("c4"), again) == 1 and torch.equal(again.arena.master, c4.arena.master)
    for other in (None, 8):
        t = Trainer("resnet_tiny", "cpu", seed=9, cardinality=other)
        before = t.arena.master.clone()
        with pytest.raises(ValueError, match="cardinality"):
            load_snapshot(sw.path_of("c4"), t)
        assert torch.equal(t.arena.master, before)                        # nothing written


def test_submit_cardinality_reaches_the_start_action(tmp_path, monkeypatch):
    import bench
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.cluster_runtime import Controller, Worker
    from tiresias_amd.executor.fake import FakeCluster, ProtocolError, VirtualClock
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    inc = os.path.join(sp.root, "incoming")
    assert submit_cli.main(["--spool", sp.root, "--model", "resnet50", "--iterations", "3", "--job-id", "a",
                            "--cardinality", "32"]) == 0
    assert json.load(open(os.path.join(inc, "a.json")))["cardinality"] == 32
    assert submit_cli.main(["--spool", sp.root, "--model", "resnet50", "--iterations", "3", "--job-id", "b"]) == 0
    assert "cardinality" not in json.load(open(os.path.join(inc, "b.json")))   # written only when asked
    for jid, model, v in (("v", "vgg16", 32), ("t", "transformer", 32), ("n", "resnet50", 3), ("s", "resnet50", "32")):
        with open(os.path.join(inc, f"{jid}.json"), "w") as f:
            json.dump({"job_id": jid, "model": model, "iterations": 2, "cardinality": v}, f)
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
    assert {a["job"]: a.get("cardinality") for a in starts} == {"a": 32, "b": None}
    assert all("cardinality" not in a for a in starts if a["job"] == "b")  # the action as it always was
    assert fc.card == {"a": 32, "b": None}
    with pytest.raises(ProtocolError, match="cardinality"):
        fc.apply({"actions": [dict(starts[0], cardinality=3)]})
    # the worker's warm pool keeps the cardinalities apart
    act = {"op": "start", "job": "1", "model": "resnet_tiny", "batch": None, "seed": 1, "ranks": (0,)}
    plain, c4 = Worker._pool_key(act), Worker._pool_key(dict(act, cardinality=4))
    assert plain == ("resnet_tiny", None, (0,)) and c4 != plain and c4 != Worker._pool_key(dict(act, cardinality=8))
