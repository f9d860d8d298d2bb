"""Adafactor off the device: the CPU trainer step against the fp64 formulas of
adafactor.hip, request validation, and the size a factored job is priced at."""
import pytest
import torch

from tiresias_amd.executor.trainer import Trainer
from tiresias_amd.ops.arena import factored_shape, factored_state_numel

BOUND = 1e-5          # fp32 arithmetic against fp64, relative L2 (tests/test_kernels_gpu.py::_sgd_adam_check)


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm())


def test_cpu_trainer_step_obeys_the_formulas():
    assert [factored_shape(s) for s in [(2, 4), (5, 6), (70,), (4, 2, 6)]] == [(2, 4), (1, 30), (1, 70), (4, 12)]
    t = Trainer("transformer_tiny", "cpu", seed=3, opt_dtype="factored")
    A = t.arena
    assert len(t.opt_state) == 1 and t.opt_state[0].numel() == factored_state_numel([p.shape for p in A._order()])
    for step in (1, 2):
        t._fwd_bwd()
        w0, g0, st0 = A.master.double().clone(), A.grad.double().clone(), t.opt_state[0].double().clone()
        t._opt_step()
        b2 = 1.0 - float(step) ** -0.8
        for p in A._order():
            so, R, C = t._af_slices[p.name]
            g, w = g0[p.offset:p.offset + p.numel].view(R, C), w0[p.offset:p.offset + p.numel].view(R, C)
            rv = b2 * st0[so:so + R] + (1 - b2) * (g * g + 1e-30).mean(1)
            cv = b2 * st0[so + R:so + R + C] + (1 - b2) * (g * g + 1e-30).mean(0)
            u = g * (rv / rv.mean()).rsqrt()[:, None] * cv.rsqrt()[None, :]
            rms = float(u.pow(2).mean().sqrt())
            s = 1.0 / max(1.0, rms)
            want = w - t.lr * (s * u + (t.spec.wd if p.decay else 0.0) * w)
            assert _rel(t.opt_state[0][so:so + R], rv) < BOUND and _rel(t.opt_state[0][so + R:so + R + C], cv) < BOUND
            assert _rel(p.master, want.view(p.shape)) < BOUND, p.name
            assert t.update_rms()[p.name] == pytest.approx((rms, s), rel=BOUND)
        assert int(torch.count_nonzero(A.grad)) == 0 and torch.equal(A.shadow, A.master.to(torch.bfloat16))
    assert t.reset(1).update_rms() == {} and int(torch.count_nonzero(t.opt_state[0])) == 0


def test_request_validation(tmp_path):
    import bench
    from tiresias_amd.executor.cluster_runtime import Controller
    from tiresias_amd.executor.fake import VirtualClock
    from tiresias_amd.executor.spool import Spool

    cfg = bench.make_cfg("dlas-gpu", "tiresias", 2, 3, "none", [0.05, 0.25, 1.0], False)
    ctrl = Controller(cfg, [], 2, 0.05, spool=Spool(str(tmp_path / "spool")), clock=VirtualClock())
    base = {"model": "transformer", "iterations": 2, "job_id": "x", "opt_dtype": "factored"}
    assert ctrl._validate(base)[-1]["opt_dtype"] == "factored"
    with pytest.raises(ValueError, match="adam"):
        ctrl._validate(dict(base, model="vgg16"))
    with pytest.raises(ValueError, match="trust_ratio"):
        ctrl._validate(dict(base, trust_ratio=0.1))
    ctrl.ddp_shard = True
    with pytest.raises(ValueError, match="ddp_shard"):
        ctrl._validate(dict(base, num_gpu=2))


def test_a_factored_job_is_priced_at_its_size():
    from tiresias_amd.executor import fake
    from tiresias_amd.executor.cluster_runtime import Worker
    from tiresias_amd.profiler.skew import model_profile

    for m in ("transformer", "gnmt", "transformer_tiny"):
        p = model_profile(m)
        assert 0 < p.factored < p.params // 100 or m == "transformer_tiny"
        assert p.state_bytes("adam", "factored") == 6 * p.params + 4 * p.factored
        assert fake._state_bytes(m, "factored") == p.state_bytes("adam", "factored") < fake._state_bytes(m, "bf16")
    w = Worker(0, 1, torch.device("cpu"))
    assert w._job_need("gnmt", None, "factored") == 1.5 * model_profile("gnmt").state_bytes("adam", "factored")
    t = w._make_trainer({"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1,
                         "ranks": (0,), "source": "fresh", "opt_dtype": "factored"})
    assert t.opt_dtype == "factored" and t.pool_key == ("transformer_tiny", None, (0,), "factored")
