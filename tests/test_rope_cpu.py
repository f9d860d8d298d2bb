"""Rotary position embeddings off the device: the table, the CPU mirror of the
kernels' rotation, the model, and the knob's path from ``submit --pos`` to the trainer."""
import json
import os

import pytest
import torch

from tiresias_amd.executor.trainer import Trainer, check_pos
from tiresias_amd.ops import functional as Fx

W = 10000.0 ** (-torch.arange(32, dtype=torch.float64) / 32)


def test_table_is_fp64_cos_sin_rounded_once():
    t = Fx.rope_table(300, "cpu")
    assert t.shape == (300, 2, 32) and t.dtype == torch.float32 and t.is_contiguous()
    ang = torch.arange(300, dtype=torch.float64)[:, None] * W
    assert torch.equal(t[:, 0], ang.cos().float()) and torch.equal(t[:, 1], ang.sin().float())


@pytest.mark.parametrize("causal", [False, True])
def test_cpu_mirror_against_complex_rotation(causal):
    """``_attn_ref`` with a table against (x_j + i x_{j+32}) e^{i theta} in complex128."""
    S = 37
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(2, S, 2, 64, generator=g).to(torch.bfloat16) for _ in range(3))
    turn = torch.polar(torch.ones(S, 32, dtype=torch.float64), torch.arange(S, dtype=torch.float64)[:, None] * W)

    def rot(x):
        z = torch.complex(x[..., :32].double(), x[..., 32:].double()) * turn[:, None]
        return torch.cat([z.real, z.imag], -1)

    s = torch.einsum("bqhd,bkhd->bhqk", rot(q), rot(k)) / 8.0
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    want = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v.double())
    o, lse = Fx._attn_ref(q, k, v, causal, 0.125, None, rope=Fx.rope_table(S, "cpu"))
    # the rotated operands are rounded to bf16 (2^-9 each): the device tests' bounds
    assert ((o.double() - want).norm() / want.norm()).item() < 1e-2
    assert ((lse.double() - torch.logsumexp(s, -1)).norm() / torch.logsumexp(s, -1).norm()).item() < 1e-3
    plain, _ = Fx._attn_ref(q, k, v, causal, 0.125, None)
    assert ((plain.double() - want).norm() / want.norm()).item() > 0.1      # ...and the rotation matters


def test_model_has_the_same_parameters():
    a, b = Trainer("transformer_tiny", "cpu", seed=4), Trainer("transformer_tiny", "cpu", seed=4, pos="rope")
    assert [(p.name, tuple(p.shape)) for p in a.arena.params] == [(p.name, tuple(p.shape)) for p in b.arena.params]
    assert torch.equal(a.arena.master, b.arena.master)
    assert a.pos == "sinusoid" and a.model.rope is None and b.model.pos is None and b.model.rope.shape == (64, 2, 32)
    la, lb = float(a.step()), float(b.step())
    assert la == la and lb == lb and la != lb


def test_other_models_and_other_values_are_rejected():
    for model in ("vgg16", "resnet50", "resnet_tiny", "gnmt", "gnmt_tiny"):
        with pytest.raises(ValueError, match="pos="):
            check_pos(model, "rope")
    for bad in ("alibi", 1, True):
        with pytest.raises(ValueError, match="pos must be"):
            Trainer("transformer_tiny", "cpu", pos=bad)


def test_snapshot_into_another_pos_raises(tmp_path):
    from tiresias_amd.ckpt.snapshot import SnapshotWriter, load_snapshot

    r, p = Trainer("transformer_tiny", "cpu", seed=4, pos="rope"), Trainer("transformer_tiny", "cpu", seed=4)
    r.step()
    sw = SnapshotWriter(str(tmp_path), torch.device("cpu"))
    sw.snapshot("r", r)
    sw.snapshot("p", p)
    sw.flush()
    sw.close()
    assert "pos" not in torch.load(sw.path_of("p"), weights_only=True)      # the file as it always was
    again = Trainer("transformer_tiny", "cpu", seed=9, pos="rope")
    assert load_snapshot(sw.path_of("r"), again) == 1 and torch.equal(again.arena.master, r.arena.master)
    for path, t in ((sw.path_of("r"), Trainer("transformer_tiny", "cpu", seed=9)), (sw.path_of("p"), again)):
        before = t.arena.master.clone()
        with pytest.raises(ValueError, match="pos="):
            load_snapshot(path, t)
        assert torch.equal(t.arena.master, before)                          # nothing written


def test_submit_pos_reaches_the_start_action(tmp_path):
    import bench
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.cluster_runtime import Controller, Worker
    from tiresias_amd.executor.fake import FakeCluster, ProtocolError, VirtualClock
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    inc = os.path.join(sp.root, "incoming")
    assert submit_cli.main(["--spool", sp.root, "--model", "transformer", "--iterations", "3", "--job-id", "a",
                            "--pos", "rope"]) == 0
    assert json.load(open(os.path.join(inc, "a.json")))["pos"] == "rope"
    assert submit_cli.main(["--spool", sp.root, "--model", "transformer", "--iterations", "3", "--job-id", "b"]) == 0
    assert "pos" not in json.load(open(os.path.join(inc, "b.json")))        # written only when asked
    for jid, model, v in (("v", "vgg16", "rope"), ("g", "gnmt", "rope"), ("n", "transformer", "alibi")):
        with open(os.path.join(inc, f"{jid}.json"), "w") as f:
            json.dump({"job_id": jid, "model": model, "iterations": 2, "pos": v}, f)
    cfg = bench.make_cfg("dlas-gpu", "tiresias", 2, 3, "none", [0.05, 0.25, 1.0], False)
    ctrl = Controller(cfg, [], 2, 0.05, spool=sp, clock=VirtualClock())
    fc = FakeCluster(2, vnode_size=ctrl.vnode_size, nic_gbps=ctrl.nic_gbps)
    ctrl.start_clock()
    plan = ctrl.plan_round()                       # two GPUs, two 1-GPU jobs: both start in the first round
    starts = [a for a in plan["actions"] if a["op"] == "start"]
    fc.apply(plan)
    assert set(os.listdir(os.path.join(sp.root, "rejected"))) == {"v.json", "g.json", "n.json"}
    assert {a["job"]: a.get("pos") for a in starts} == {"a": "rope", "b": None}
    assert all("pos" not in a for a in starts if a["job"] == "b")           # the action as it always was
    assert fc.pos == {"a": "rope", "b": None}
    with pytest.raises(ProtocolError, match="pos"):
        fc.apply({"actions": [dict(starts[0], pos="alibi")]})
    act = {"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1, "ranks": (0,)}
    plain = Worker._pool_key(act)                  # the worker's warm pool keeps the two forwards apart
    assert plain == ("transformer_tiny", None, (0,)) == Worker._pool_key(dict(act, pos="sinusoid"))
    assert Worker._pool_key(dict(act, pos="rope")) == plain + ("pos=rope",)
