"""The per-job training knobs end to end (executor/knobs.py): submit CLI ->
spool request -> controller -> start action -> fake backend / worker pool
key, for a job that sets every knob its model takes and for one that sets
none. The literals are what the code wrote before the knobs had one table:
the wire format and the pool keys must not move."""
import inspect
import json
import os
from dataclasses import fields

import pytest

OFF = {"grad_clip": None, "dropout": None, "attn_dropout": None, "opt_dtype": None, "trust_ratio": None}
# (job id, model, submit options, knob keys of its request and of its start action, its pool key's tail)
JOBS = (
    ("r", "resnet50",
     ["--grad-clip", "5", "--dropout", "0.1", "--opt-dtype", "bf16", "--norm", "group", "--cardinality", "32",
      "--se-ratio", "16"],
     dict(OFF, grad_clip=5.0, dropout=0.1, opt_dtype="bf16", norm="group", cardinality=32, se_ratio=16),
     ("bf16", "norm=group", "cardinality=32", "se_ratio=16")),
    ("t", "transformer", ["--attn-dropout", "0.1", "--trust-ratio", "0.001", "--pos", "rope"],
     dict(OFF, attn_dropout=0.1, trust_ratio=0.001, pos="rope"), ("pos=rope",)),
    ("n", "resnet50", [], dict(OFF), ()),
)


def _controller(sp, world=4):
    import bench
    from tiresias_amd.executor.cluster_runtime import Controller
    from tiresias_amd.executor.fake import VirtualClock

    cfg = bench.make_cfg("dlas-gpu", "tiresias", world, 3, "none", [0.05, 0.25, 1.0], False)
    return Controller(cfg, [], world, 0.05, spool=sp, clock=VirtualClock())


def test_all_knobs_and_none_travel_as_they_always_did(tmp_path, monkeypatch):
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.cluster_runtime import Worker
    from tiresias_amd.executor.fake import FakeCluster
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    monkeypatch.setattr("time.time", lambda: 1.0)
    for jid, model, opts, knobs, _ in JOBS:
        assert submit_cli.main(["--spool", sp.root, "--model", model, "--iterations", "3", "--job-id", jid] + opts) == 0
        req = json.load(open(os.path.join(sp.root, "incoming", f"{jid}.json")))
        assert req == {"job_id": jid, "model": model, "num_gpu": 1, "iterations": 3, "duration": None, "batch": None,
                       "submitted_wall": 1.0, **knobs}
    monkeypatch.undo()
    ctrl = _controller(sp)
    fc = FakeCluster(4, vnode_size=ctrl.vnode_size, nic_gbps=ctrl.nic_gbps)
    ctrl.start_clock()
    plan = ctrl.plan_round()                       # four GPUs, three 1-GPU jobs: all start in the first round
    assert os.listdir(os.path.join(sp.root, "rejected")) == []
    starts = {a["job"]: a for a in plan["actions"] if a["op"] == "start"}
    fc.apply(plan)
    for jid, model, _, knobs, tail in JOBS:
        act = dict(starts[jid])
        ranks = tuple(act.pop("ranks"))
        assert isinstance(act.pop("seed"), int) and len(ranks) == 1
        assert act == {"op": "start", "job": jid, "model": model, "iters": 3, "batch": None, "source": "fresh",
                       **knobs}
        assert Worker._pool_key(starts[jid]) == (model, None, ranks) + tail
        assert {k: fc.knobs[k][jid] for k in fc.knobs if fc.knobs[k][jid] is not None} == \
            {k: v for k, v in knobs.items() if v is not None}
    # a structural knob fixes the job's model or buffers: a held job is not started with another value
    from tiresias_amd.executor.fake import ProtocolError

    for change in ({"opt_dtype": "fp32"}, {"opt_dtype": None}, {"cardinality": 8}):
        with pytest.raises(ProtocolError, match=f"{list(change)[0]}.*its state was built with"):
            fc.apply({"actions": [dict(starts["r"], source="resident", **change)]})
    fc.apply({"actions": [dict(starts["r"], source="resident", grad_clip=1.0, dropout=None)]})   # per-job ones may move
    with pytest.raises(ProtocolError, match="start of r with grad_clip"):
        fc.apply({"actions": [dict(starts["r"], source="resident", grad_clip=-1.0)]})


def test_pool_hit_sets_the_per_job_knobs_and_leaves_the_graph_choice_alone(monkeypatch):
    """A warm-pool hit re-sets the four per-job knobs from the action and
    turns hipGraph capture on only where the worker wants graphs."""
    import torch

    from tiresias_amd.executor.cluster_runtime import Worker
    from tiresias_amd.executor.trainer import Trainer

    calls = []
    monkeypatch.setattr(Trainer, "enable_graph", lambda self: calls.append(self))
    act = {"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1, "ranks": (0,),
           "source": "fresh", "iters": 10 ** 6, "grad_clip": 2.0, "dropout": 0.25, "attn_dropout": 0.5,
           "trust_ratio": 0.01}
    for use_graph, enabled in ((False, 0), (True, 1)):
        w = Worker(0, 1, torch.device("cpu"), use_graph=use_graph)
        t = w._make_trainer(act)
        assert (t.grad_clip, t.dropout, t.attn_dropout, t.trust_ratio) == (2.0, 0.25, 0.5, 0.01)
        w.pool.setdefault(t.pool_key, []).append(t)
        del calls[:]
        t2 = w._make_trainer(dict(act, job="2", seed=2, grad_clip=None, dropout=None, attn_dropout=0.25,
                                  trust_ratio=None))
        assert t2 is t and (t.grad_clip, t.dropout, t.attn_dropout, t.trust_ratio) == (None, None, 0.25, None)
        assert len(calls) == enabled


def test_the_table_names_every_field_and_keyword(tmp_path):
    from tiresias_amd.executor.cluster_runtime import ReplayJob
    from tiresias_amd.executor.knobs import KNOBS
    from tiresias_amd.executor.spool import Spool
    from tiresias_amd.executor.trainer import Trainer

    assert list(KNOBS) == ["grad_clip", "dropout", "attn_dropout", "opt_dtype", "trust_ratio", "norm", "cardinality",
                           "se_ratio", "pos"]
    assert {f.name for f in fields(ReplayJob)} - {"spec", "model", "iterations", "batch"} == set(KNOBS)
    assert set(KNOBS) <= set(inspect.signature(Trainer.__init__).parameters)
    sp = Spool(str(tmp_path / "spool"))
    with pytest.raises(TypeError, match="nonsense"):
        sp.submit("resnet50", 1, iterations=3, nonsense=1)
    assert os.listdir(os.path.join(sp.root, "incoming")) == []


def test_bf16_state_on_a_sharded_gang_is_rejected_at_submission(tmp_path):
    """Trainer() refuses opt_dtype="bf16" on a multi-GPU gang under
    ddp_shard; the controller must refuse the request, not schedule it."""
    from tiresias_amd.executor.spool import Spool

    ctrl = _controller(Spool(str(tmp_path / "spool")))
    base = {"model": "transformer", "iterations": 2, "job_id": "x", "opt_dtype": "bf16"}
    assert ctrl._validate(dict(base, num_gpu=2))[-1]["opt_dtype"] == "bf16"      # a replicated gang: fine
    ctrl.ddp_shard = True
    assert ctrl._validate(dict(base, num_gpu=1))[-1]["opt_dtype"] == "bf16"      # one GPU: nothing is sharded
    with pytest.raises(ValueError, match="opt_dtype.*ddp_shard"):
        ctrl._validate(dict(base, num_gpu=2))
