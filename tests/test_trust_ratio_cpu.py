"""Layer-wise trust-ratio optimizers (LARS / LAMB) without a GPU: the
Trainer's plain-torch mirror of the device path against an independent fp64
implementation of the contract, the zero-padding invariant the segment norms
rely on, the rejections, and the per-job option from ``submit --trust-ratio``
to the start action and the warm pool."""
import json
import math
import os

import pytest
import torch

from tiresias_amd.executor.trainer import Trainer
from tiresias_amd.ops.arena import _padded

MODELS_ETA = [("resnet_tiny", 0.02), ("transformer_tiny", 1.0)]


def _ratio(eta, wn, xn, extra=0.0):
    ok = 0.0 < wn < math.inf and 0.0 < xn < math.inf
    return eta * wn / (xn + extra * wn) if ok else 1.0


def _contract(t, g, w0, st0):
    """LARS / LAMB per parameter in fp64 -> ({name: ratio}, new master)."""
    eta, wd, lr, k = t.trust_ratio, t.spec.wd, t.lr, t.step_count
    g, w0 = g.double(), w0.double()
    st0 = [x.double() for x in st0]
    wn = w0.clone()
    if t.opt == "adam":
        m = 0.9 * st0[0] + 0.1 * g
        v = 0.98 * st0[1] + 0.02 * g * g
        dirn = (m / (1 - 0.9 ** k)) / ((v / (1 - 0.98 ** k)).sqrt() + 1e-9)
    ratios = {}
    for p in t.arena.params:
        sl = slice(p.offset, p.offset + p.numel)
        if t.opt == "sgd":
            r = _ratio(eta, float(w0[sl].norm()), float(g[sl].norm()), wd) if p.decay else 1.0
            mom = 0.9 * st0[0][sl] + r * (g[sl] + (wd if p.decay else 0.0) * w0[sl])
            wn[sl] = w0[sl] - lr * mom
        else:
            u = dirn[sl] + (wd if p.decay else 0.0) * w0[sl]
            r = _ratio(eta, float(w0[sl].norm()), float(u.norm())) if p.decay else 1.0
            wn[sl] = w0[sl] - lr * r * u
        if p.decay:
            ratios[p.name] = r
    return ratios, wn


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("model,eta", MODELS_ETA)
def test_cpu_trainer_follows_the_contract(model, eta):
    t = Trainer(model, "cpu", seed=3, trust_ratio=eta)
    A = t.arena
    assert t.trust_ratios() == {}
    t.step()
    t._fwd_bwd()
    g, w0, st0 = A.grad.clone(), A.master.clone(), [s.clone() for s in t.opt_state]
    t._opt_step()
    want, w_ref = _contract(t, g, w0, st0)
    got = t.trust_ratios()
    assert set(got) == set(want) == {p.name for p in A.params if p.decay}
    assert any(abs(r - 1.0) > 1e-3 for r in want.values())
    for k, r in want.items():
        assert abs(got[k][0] - r) <= 1e-6 * r, k
    for p in A.params:
        sl = slice(p.offset, p.offset + p.numel)
        if float(w_ref[sl].norm()) == 0.0:
            assert torch.count_nonzero(A.master[sl]) == 0, p.name
        else:
            assert _rel(A.master[sl], w_ref[sl]) < 1e-5, p.name
    assert torch.equal(A.shadow, A.master.to(torch.bfloat16))
    assert torch.count_nonzero(A.grad) == 0
    # the same state through a trainer with the knob off: every no-decay
    # parameter moves exactly alike, the decayed ones do not
    off = Trainer(model, "cpu", seed=3)
    assert off.trust_ratio is None and off._tr is None
    off.arena.master.copy_(w0)
    off.arena.grad.copy_(g)
    for a, b in zip(off.opt_state, st0):
        a.copy_(b)
    off.step_count = t.step_count - 1
    off._opt_step()
    assert off.trust_ratios() == {}
    assert torch.equal(off.arena.master[A.n_decay:], A.master[A.n_decay:])
    for a, b in zip(off.opt_state, t.opt_state):
        assert torch.equal(a[A.n_decay:], b[A.n_decay:])
    assert not torch.equal(off.arena.master[:A.n_decay], A.master[:A.n_decay])
    t.reset(4)
    assert t.trust_ratios() == {} and t.trust_ratio == eta


@pytest.mark.parametrize("model,eta", MODELS_ETA)
def test_padding_stays_zero(model, eta):
    """Every parameter is padded to 64 elements; the segment norms run over
    the padded extent, so the padding of master and grad must stay zero."""
    t = Trainer(model, "cpu", seed=3, trust_ratio=eta)
    A = t.arena
    pad = torch.ones(A.numel, dtype=torch.bool)
    for p in A.params:
        pad[p.offset:p.offset + p.numel] = False
        assert p.offset % 64 == 0 and _padded(p.numel) % 64 == 0
    assert int(pad.sum()) > 0 or model == "transformer_tiny"       # (its shapes are all multiples of 64)
    for _ in range(3):
        t.step()
    t._fwd_bwd()
    assert torch.count_nonzero(A.master[pad]) == 0 and torch.count_nonzero(A.grad[pad]) == 0
    for s in t.opt_state:
        assert torch.count_nonzero(s[pad]) == 0


def test_off_by_default_and_validated():
    from tiresias_amd.models import MODELS

    assert all(s.trust_ratio is None for s in MODELS.values())
    t = Trainer("transformer_tiny", "cpu", seed=3)
    assert t.trust_ratio is None and t._tr is None and t.trust_ratios() == {}
    for v in (0.0, -1.0, float("inf"), float("nan"), "0.1"):
        with pytest.raises(ValueError, match="trust_ratio"):
            t.set_trust_ratio(v)
        with pytest.raises(ValueError, match="trust_ratio"):
            Trainer("transformer_tiny", "cpu", trust_ratio=v)
    t.set_trust_ratio(0.5)
    assert t.trust_ratio == 0.5
    t.set_trust_ratio(None)
    assert t.trust_ratio is None


def test_sharded_gang_and_bf16_state_are_rejected():
    class _Comm:            # a 2-member gang comm (parallel/gang.py comm_size reads .size)
        size = 2
        ranks = (0, 1)

    with pytest.raises(ValueError, match="ddp_shard"):
        Trainer("transformer_tiny", "cpu", trust_ratio=1.0, ddp_shard=True, group=_Comm())
    t = Trainer("transformer_tiny", "cpu", trust_ratio=1.0, ddp_shard=True)       # no gang yet: fine
    with pytest.raises(ValueError, match="ddp_shard"):
        t.rebind(_Comm())
    t = Trainer("transformer_tiny", "cpu")

    class _D:
        shard, dirty = True, False

    t.ddp = _D()
    with pytest.raises(ValueError, match="ddp_shard"):
        t.set_trust_ratio(1.0)
    with pytest.raises(ValueError, match="bf16"):
        Trainer("transformer_tiny", "cpu", trust_ratio=1.0, opt_dtype="bf16")
    b = Trainer("transformer_tiny", "cpu", opt_dtype="bf16")
    with pytest.raises(ValueError, match="bf16"):
        b.set_trust_ratio(1.0)


# ------------------------------------------------------------------ submission
def _fake_controller_run(sp):
    """The live controller over a spool against the fake backend (virtual
    time); returns (controller, every start action it planned)."""
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


def test_submit_trust_ratio_reaches_the_start_action(tmp_path):
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    assert submit_cli.main(["--spool", sp.root, "--model", "resnet50", "--iterations", "3", "--job-id", "a",
                            "--trust-ratio", "0.001"]) == 0
    req = json.load(open(os.path.join(sp.root, "incoming", "a.json")))
    assert req["trust_ratio"] == 0.001
    sp.submit("resnet50", 1, iterations=3, job_id="b")
    sp.submit("transformer", 2, iterations=3, job_id="c", trust_ratio=1)
    assert json.load(open(os.path.join(sp.root, "incoming", "b.json")))["trust_ratio"] is None
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)                    # the fake backend accepts the key
    assert len(ctrl.sched.finished) == 3
    assert {a["job"]: a["trust_ratio"] for a in starts} == {"a": 0.001, "b": None, "c": 1.0}
    assert ctrl.rjobs["a"].trust_ratio == 0.001 and ctrl.rjobs["b"].trust_ratio is None


def test_bad_trust_ratio_is_rejected_not_fatal(tmp_path):
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    inc = os.path.join(sp.root, "incoming")
    base = {"model": "resnet50", "iterations": 2}
    bad = {"neg": -1, "zero": 0, "str": "0.1", "bool": True, "nan": float("nan"), "inf": float("inf")}
    for name, v in bad.items():
        with open(os.path.join(inc, f"{name}.json"), "w") as f:
            json.dump(dict(base, job_id=name, trust_ratio=v), f)
    with open(os.path.join(inc, "bf.json"), "w") as f:
        json.dump(dict(base, job_id="bf", trust_ratio=0.1, opt_dtype="bf16"), f)
    sp.submit("resnet50", 1, iterations=2, job_id="ok", trust_ratio=0.02)
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)
    assert [j.job_id for j in ctrl.sched.finished] == ["ok"]
    assert set(os.listdir(os.path.join(sp.root, "rejected"))) == {f"{n}.json" for n in list(bad) + ["bf"]}
    for name in bad:
        why = json.load(open(os.path.join(sp.root, "rejected", f"{name}.json")))["reason"]
        assert "trust_ratio must be a finite number > 0" in why, (name, why)
    assert "bf16" in json.load(open(os.path.join(sp.root, "rejected", "bf.json")))["reason"]
    assert [a["trust_ratio"] for a in starts] == [0.02]
    for v in bad.values():
        with pytest.raises(ValueError, match="trust_ratio"):
            ctrl._validate(dict(base, job_id="x", trust_ratio=v))
    # a sharded cluster: rejected for a gang, accepted for one GPU
    ctrl.ddp_shard = True
    with pytest.raises(ValueError, match="ddp_shard"):
        ctrl._validate(dict(base, job_id="x", num_gpu=2, trust_ratio=0.1))
    assert ctrl._validate(dict(base, job_id="x", num_gpu=1, trust_ratio=0.1))[-1] == 0.1


def test_worker_sets_it_per_job_on_new_and_pooled_trainers():
    from tiresias_amd.executor.cluster_runtime import Worker

    w = Worker(0, 1, torch.device("cpu"))
    act = {"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1, "ranks": (0,),
           "source": "fresh", "trust_ratio": 0.5}
    t = w._make_trainer(act)
    assert t.trust_ratio == 0.5 and t.pool_key == ("transformer_tiny", None, (0,))     # not part of the key
    float(t.step())
    assert t.trust_ratios()
    w.pool.setdefault(t.pool_key, []).append(t)
    t2 = w._make_trainer(dict(act, job="2", seed=2, trust_ratio=None))
    assert t2 is t and t2.trust_ratio is None and t2.trust_ratios() == {}
    float(t2.step())
    assert t2.trust_ratios() == {}
    w.pool.setdefault(t.pool_key, []).append(t)
    del act["trust_ratio"]                           # an action without the key: off
    assert w._make_trainer(act).trust_ratio is None
