"""bf16 optimizer state without a GPU: the torch mirror of the stochastic
rounding helper against a bit-level reference, the CPU trainer's state under
the contract, a gloo world-2 gang, the sharded-gang rejection, the per-job
option from ``submit --opt-dtype`` to the start action and the warm pool, and
snapshots across formats."""
import json
import os
import socket
import struct

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tiresias_amd.executor import trainer as trainer_mod
from tiresias_amd.executor.trainer import Trainer
from tiresias_amd.ops import functional as Fx

BF16 = torch.bfloat16


# ------------------------------------------------------------------ the helper
def _py_sr(b: int, u: int) -> int:
    """The contract on one fp32 bit pattern, in plain Python."""
    if (b >> 23) & 0xFF == 0xFF:
        return (b >> 16) | (0x40 if b & 0x7FFFFF else 0)
    return ((b + u) >> 16) & 0xFFFF


def _bits(f: float) -> int:
    return struct.unpack("<I", struct.pack("<f", f))[0]


def _from_bits(pats):
    return torch.tensor([((p ^ 0x80000000) - 0x80000000) for p in pats], dtype=torch.int32).view(torch.float32)


def _bf_bits(t):
    return [int(v) & 0xFFFF for v in t.view(torch.int16)]


def test_mirror_matches_bit_level_reference():
    pats = [
        0x3F800000, 0x3F808000, 0x3F80FFFF, 0x3F800001,      # 1.0, half way, just under the next, just over
        0x3FFFFFFF,                                          # mantissa all ones: the carry reaches the exponent
        0x7F7FFFFF, 0x7F7F0001, 0x7F7F0000,                  # the largest finite values: up to inf, or exact
        0xFF7FFFFF, 0xBF808000, 0x80000001, 0x80000000,      # negative: the magnitude goes up, -denormal, -0
        0x00000001, 0x0000FFFF, 0x007FFFFF, 0x00000000,      # denormals (the last carries into the normals), +0
        0x7F800000, 0xFF800000,                              # inf
        0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7F80FFFF,      # NaN, payload in the low half only included
        _bits(0.1), _bits(-3.14159), _bits(6.1e-5),
    ]
    draws = [0, 1, 0x7FFF, 0x8000, 0xFFFE, 0xFFFF]
    x = _from_bits([p for p in pats for _ in draws])
    u = torch.tensor(draws * len(pats), dtype=torch.int64)
    got = _bf_bits(Fx.sr_bf16(x, u))
    want = [_py_sr(p, d) for p in pats for d in draws]
    assert got == want
    k = len(draws)
    at = {p: got[i * k:(i + 1) * k] for i, p in enumerate(pats)}
    assert at[0x3FFFFFFF] == [0x3FFF] + [0x4000] * 5              # carry into the exponent: 2.0
    assert at[0x7F7FFFFF] == [0x7F7F] + [0x7F80] * 5              # the largest finite value goes to inf
    assert at[0xFF7FFFFF] == [0xFF7F] + [0xFF80] * 5
    assert at[0x3F808000] == [0x3F80] * 3 + [0x3F81] * 3          # half way: up for half of the draws
    assert at[0xBF808000] == [0xBF80] * 3 + [0xBF81] * 3          # sign-magnitude
    assert at[0x007FFFFF] == [0x007F] + [0x0080] * 5
    for p in (0x3F800000, 0x7F7F0000, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000):
        assert at[p] == [p >> 16] * k                             # exact values and inf: any draw
    for p in (0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7F80FFFF):
        out = Fx.sr_bf16(_from_bits([p] * k), torch.tensor(draws))
        assert bool(torch.isnan(out.float()).all()) and set(_bf_bits(out)) == {(p >> 16) | 0x40}


def test_rounding_is_unbiased_and_draws_follow_the_counter():
    um, uv = Fx.opt_state_draws(0, 1 << 16, 7, 3)
    assert um.dtype == torch.int64 and int(um.min()) >= 0 and int(um.max()) <= 0xFFFF and int(uv.max()) <= 0xFFFF
    assert abs(float(um.double().mean()) - 32767.5) < 5 * 65536 / (12 * 65536) ** 0.5
    x = torch.full((1 << 16,), 1.0 + 3.0 / 1024)                  # 3/8 of a bf16 ulp above 1.0
    r = Fx.sr_bf16(x, um).double()
    # mean of 65536 Bernoulli(3/8) steps of one ulp (2^-7): sigma = sqrt(p q / n) ulp, 5 sigma
    assert abs(float(r.mean()) - float(x[0])) < 5 * (0.375 * 0.625 / 65536) ** 0.5 * 2 ** -7
    # a window of the arena draws what the whole arena draws there; q's high word, the step and the seed matter
    a, b = Fx.opt_state_draws(8, 1000, 7, 3)
    assert torch.equal(a, um[8:1008]) and torch.equal(b, uv[8:1008])
    hi = Fx.opt_state_draws((1 << 34) + 8, 1000, 7, 3)[0]
    assert not torch.equal(hi, a)
    assert not torch.equal(Fx.opt_state_draws(8, 1000, 7, 4)[0], a)
    assert not torch.equal(Fx.opt_state_draws(8, 1000, 8, 3)[0], a)
    # the counter words, spelled out for one group
    q = ((1 << 34) + 8) >> 2
    o = Fx.philox4x32_10(torch.tensor([q & 0xFFFFFFFF]), torch.tensor([q >> 32]), torch.tensor([0x40000000]),
                         torch.tensor([3]), 7, 0)
    assert [int(w[0]) & 0xFFFF for w in o] == [int(v) for v in hi[:4]]


def test_mirror_does_not_stall_where_round_to_nearest_does():
    """An EMA with b2 = 0.999 over 300 steps of a constant gradient, 65536
    elements. Per element the stored v differs from the fp32 one by
    sum_t b2^(T-t) e_t with e_t zero-mean, independent and inside one bf16 ulp
    (<= 2^-7 g^2, v never exceeds g^2), so Var <= (2^-7 g^2)^2 / (4 (1 - b2^2))
    and the mean over N elements has standard error sqrt(Var / N); the bound
    is 6 standard errors. Round-to-nearest must fall outside it."""
    n, steps, g2 = 65536, 300, 1.0
    b2 = torch.tensor(0.999, dtype=torch.float32)
    c = (torch.tensor(1.0) - b2) * g2
    se = (2.0 ** -7 * g2) / 2.0 / (1.0 - 0.999 ** 2) ** 0.5 / n ** 0.5
    vf, vs, vn = torch.zeros(n), torch.zeros(n, dtype=BF16), torch.zeros(n, dtype=BF16)
    for step in range(1, steps + 1):
        vf = b2 * vf + c
        vs = Fx.sr_bf16(b2 * vs.float() + c, Fx.opt_state_draws(0, n, 12, step)[1])
        vn = (b2 * vn.float() + c).to(BF16)
    mf, ms, mn = (float(x.double().mean()) for x in (vf, vs, vn))
    print("fp32", mf, "mirror", ms, "nearest", mn, "bound", 6 * se)
    assert abs(ms - mf) <= 6 * se
    assert abs(mn - mf) > 6 * se


# ------------------------------------------------------------------ trainer
@pytest.mark.parametrize("model", ["transformer_tiny", "resnet_tiny"])
def test_cpu_trainer_state_obeys_the_contract(model, monkeypatch):
    seen = []
    real = trainer_mod._cpu_opt

    def spy(opt, w, g, state, lo, hi, wb, lr, wd, gscale, step, seed=None):
        pre = [s[lo:hi].clone() for s in state]
        gg = (g * gscale).clone()
        w0 = w.clone()
        real(opt, w, g, state, lo, hi, wb, lr, wd, gscale, step, seed=seed)
        seen.append((opt, lo, hi, pre, gg, w0, wd, step, seed, [s[lo:hi].clone() for s in state]))

    monkeypatch.setattr(trainer_mod, "_cpu_opt", spy)
    t = Trainer(model, "cpu", seed=11, opt_dtype="bf16")
    assert t.opt_dtype == "bf16" and all(s.dtype == BF16 for s in t.opt_state)
    f = Trainer(model, "cpu", seed=11)
    assert f.opt_dtype == "fp32" and all(s.dtype == torch.float32 for s in f.opt_state)
    nbuf = len(t.opt_state)
    assert f.state_bytes() - t.state_bytes() == 2 * nbuf * t.arena.numel
    assert f.hbm_bytes() - t.hbm_bytes() == 2 * nbuf * t.arena.numel
    for _ in range(3):
        loss = float(t.step())
    assert loss == loss and t.step_count == 3
    assert all(bool(s.float().abs().sum() > 0) for s in t.opt_state)
    mine = [r for r in seen if r[8] is not None]
    assert len(mine) >= 3 and sorted({r[7] for r in mine}) == [1, 2, 3]
    bits = lambda x: x.view(torch.int16)
    nearest = 0
    for opt, lo, hi, pre, gg, w0, wd, step, seed, post in mine:
        assert seed == 11 and all(p.dtype == BF16 for p in post)
        um, uv = Fx.opt_state_draws(lo, hi - lo, 11, step)
        if opt == "sgd":
            m = pre[0].float().mul_(0.9).add_(gg + wd * w0)
        else:
            m = pre[0].float().mul_(0.9).add_(0.1 * gg)
            v = pre[1].float().mul_(0.98).add_(0.02 * gg * gg)
            assert torch.equal(bits(post[1]), bits(Fx.sr_bf16(v, uv)))
        assert torch.equal(bits(post[0]), bits(Fx.sr_bf16(m, um)))
        nearest += int(torch.equal(bits(post[0]), bits(m.to(BF16))))
    assert nearest < len(mine)          # rounding to nearest is a different state (the check above can tell)
    # the fp32-state trainer is untouched by the knob's existence: same steps as an explicit "fp32"
    f2 = Trainer(model, "cpu", seed=11, opt_dtype="fp32")
    for _ in range(2):
        f.step(), f2.step()
    assert torch.equal(f.arena.master, f2.arena.master) and torch.equal(f.opt_state[0], f2.opt_state[0])
    t.reset(12)
    assert all(int(torch.count_nonzero(s)) == 0 and s.dtype == BF16 for s in t.opt_state) and t.step_count == 0


def test_opt_dtype_off_by_default_and_validated():
    from tiresias_amd.models import MODELS

    assert all(s.opt_dtype is None for s in MODELS.values())
    with pytest.raises(ValueError, match="opt_dtype"):
        Trainer("transformer_tiny", "cpu", opt_dtype="fp16")
    with pytest.raises(ValueError, match="opt_dtype"):
        Trainer("transformer_tiny", "cpu", opt_dtype=16)


def test_opt_dtype_with_sharded_gang_is_rejected():
    class _Comm:            # a 2-member gang comm (parallel/gang.py comm_size reads .size)
        size = 2
        ranks = (0, 1)

    with pytest.raises(ValueError, match="ddp_shard"):
        Trainer("transformer_tiny", "cpu", opt_dtype="bf16", ddp_shard=True, group=_Comm())
    t = Trainer("transformer_tiny", "cpu", opt_dtype="bf16", ddp_shard=True)      # no gang yet: allowed
    with pytest.raises(ValueError, match="ddp_shard"):
        t.rebind(_Comm())


def test_offload_restore_keeps_bf16_bits():
    from tiresias_amd.executor.cluster_runtime import _HostEngine

    t = Trainer("transformer_tiny", "cpu", seed=2, opt_dtype="bf16")
    f = Trainer("transformer_tiny", "cpu", seed=2)
    for _ in range(2):
        t.step(), f.step()
    want = [s.clone() for s in t.opt_state] + [t.arena.master.clone()]
    nb, nf = t.offload(_HostEngine()), f.offload(_HostEngine())
    assert nf - nb == 2 * 2 * t.arena.numel
    assert t.restore() == nb and f.restore() == nf
    got = list(t.opt_state) + [t.arena.master]
    assert all(a.dtype == b.dtype and torch.equal(a, b) for a, b in zip(got, want))
    assert all(s.untyped_storage().nbytes() == 2 * s.numel() for s in t.opt_state)
    float(t.step())


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
    t = Trainer("transformer_tiny", "cpu", seed=5, data_seed=70 + rank, group=dist.group.WORLD, bucket_mb=0.1,
                opt_dtype="bf16")
    for _ in range(3):
        t.step()
    same = True
    for buf in [t.arena.master] + [s.float() for s in t.opt_state]:       # (bf16 -> fp32 is exact and one-to-one)
        bs = [torch.zeros_like(buf) for _ in range(world)]
        dist.all_gather(bs, buf.clone())
        same = same and all(torch.equal(bs[0], x) for x in bs)
    q.put((rank, same, int(torch.count_nonzero(t.opt_state[1]))))
    dist.destroy_process_group()


def test_gang_members_hold_identical_bf16_state():
    world = 2
    q = mp.get_context("spawn").SimpleQueue()
    mp.spawn(_gang_worker, args=(world, _free_port(), q), nprocs=world, join=True)
    res = sorted(q.get() for _ in range(world))
    assert all(same for _, same, _ in res)
    assert all(nz > 0 for _, _, nz in res)


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


def test_submit_opt_dtype_reaches_the_start_action(tmp_path):
    from tiresias_amd.cli import submit as submit_cli
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    assert submit_cli.main(["--spool", sp.root, "--model", "transformer", "--iterations", "3", "--job-id", "a",
                            "--opt-dtype", "bf16"]) == 0
    req = json.load(open(os.path.join(sp.root, "incoming", "a.json")))
    assert req["opt_dtype"] == "bf16" and req["dropout"] is None
    with pytest.raises(SystemExit):
        submit_cli.main(["--spool", sp.root, "--model", "transformer", "--iterations", "3", "--opt-dtype", "fp16"])
    sp.submit("vgg16", 2, iterations=3, job_id="b", opt_dtype="fp32")            # a gang
    sp.submit("gnmt", 1, iterations=3, job_id="c")
    assert json.load(open(os.path.join(sp.root, "incoming", "c.json")))["opt_dtype"] is None
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)                                      # the fake backend accepts the key
    assert len(ctrl.sched.finished) == 3
    assert {a["job"]: a["opt_dtype"] for a in starts} == {"a": "bf16", "b": "fp32", "c": None}
    assert ctrl.rjobs["a"].opt_dtype == "bf16" and ctrl.rjobs["c"].opt_dtype is None


def test_controller_validates_opt_dtype(tmp_path):
    from tiresias_amd.executor.spool import Spool

    sp = Spool(str(tmp_path / "spool"))
    inc = os.path.join(sp.root, "incoming")
    base = {"model": "transformer", "iterations": 2}
    bad = {"fp16": "fp16", "upper": "BF16", "num": 16, "bool": True, "list": ["bf16"], "empty": ""}
    good = {"f": "fp32", "b": "bf16"}
    for name, v in {**bad, **good}.items():
        with open(os.path.join(inc, f"{name}.json"), "w") as f:
            json.dump(dict(base, job_id=name, opt_dtype=v), f)
    sp.shutdown()
    ctrl, starts = _fake_controller_run(sp)
    assert sorted(j.job_id for j in ctrl.sched.finished) == sorted(good)
    assert set(os.listdir(os.path.join(sp.root, "rejected"))) == {f"{n}.json" for n in bad}
    for name in bad:
        why = json.load(open(os.path.join(sp.root, "rejected", f"{name}.json")))["reason"]
        assert "opt_dtype must be 'fp32' or 'bf16'" in why, (name, why)
    assert {a["job"]: a["opt_dtype"] for a in starts} == {"f": "fp32", "b": "bf16"}
    for v in bad.values():
        with pytest.raises(ValueError, match="opt_dtype"):
            ctrl._validate(dict(base, job_id="x", opt_dtype=v))


def test_warm_pool_keeps_the_formats_apart():
    from tiresias_amd.executor.cluster_runtime import Worker

    w = Worker(0, 1, torch.device("cpu"))
    act = {"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1, "ranks": (0,),
           "source": "fresh"}
    f = w._make_trainer(act)
    assert f.opt_dtype == "fp32" and f.pool_key == ("transformer_tiny", None, (0,))
    w.pool.setdefault(f.pool_key, []).append(f)
    b = w._make_trainer(dict(act, job="2", seed=2, opt_dtype="bf16"))
    assert b is not f and b.opt_dtype == "bf16" and all(s.dtype == BF16 for s in b.opt_state)
    assert b.pool_key != f.pool_key and w.pool[f.pool_key] == [f]               # the fp32 one stays pooled
    w.pool.setdefault(b.pool_key, []).append(b)
    f2 = w._make_trainer(dict(act, job="3", seed=3, opt_dtype="fp32"))          # "fp32" and no key: the same pool
    assert f2 is f
    b2 = w._make_trainer(dict(act, job="4", seed=4, opt_dtype="bf16"))
    assert b2 is b and b2.seed == 4 and all(int(torch.count_nonzero(s)) == 0 for s in b2.opt_state)
    float(b2.step())
    # the admission estimate prices bf16 moments at 2 B each
    from tiresias_amd.profiler.skew import model_profile

    p = model_profile("gnmt")
    assert p.state_bytes("adam") - p.state_bytes("adam", "bf16") == 4 * p.params
    assert p.state_bytes("sgd") - p.state_bytes("sgd", "bf16") == 2 * p.params
    assert p.state_bytes("adam", "fp32") == p.state_bytes("adam")
    assert w._job_need("gnmt", None) - w._job_need("gnmt", None, "bf16") == 1.5 * 4 * p.params


# ------------------------------------------------------------------ snapshots
def test_snapshot_into_the_other_format_raises(tmp_path):
    from tiresias_amd.ckpt.snapshot import SnapshotWriter, load_snapshot

    b = Trainer("transformer_tiny", "cpu", seed=4, opt_dtype="bf16")
    f = Trainer("transformer_tiny", "cpu", seed=4)
    for _ in range(2):
        b.step(), f.step()
    sw = SnapshotWriter(str(tmp_path), torch.device("cpu"))
    try:
        sw.snapshot("b", b)
        sw.snapshot("f", f)
        sw.flush()
    finally:
        sw.close()
    saved = torch.load(sw.path_of("b"), weights_only=True)["state"]
    assert saved["opt0"].dtype == BF16 and saved["opt1"].dtype == BF16          # the snapshot carries bf16 buffers
    b2 = Trainer("transformer_tiny", "cpu", seed=9, opt_dtype="bf16")
    assert load_snapshot(sw.path_of("b"), b2) == 2
    assert all(torch.equal(x.view(torch.int16), y.view(torch.int16)) for x, y in zip(b2.opt_state, b.opt_state))
    assert torch.equal(b2.arena.master, b.arena.master)
    f2 = Trainer("transformer_tiny", "cpu", seed=9)
    before = [f2.arena.master.clone()] + [s.clone() for s in f2.opt_state]
    with pytest.raises(ValueError, match="opt_dtype"):
        load_snapshot(sw.path_of("b"), f2)
    with pytest.raises(ValueError, match="opt_dtype"):
        load_snapshot(sw.path_of("f"), b2)
    assert all(torch.equal(x, y) for x, y in zip([f2.arena.master] + list(f2.opt_state), before))   # nothing written


def test_rebound_bf16_trainer_stays_out_of_the_fp32_pool():
    """A replica that stays in a moved gang gets its pool key rewritten by the
    p2p start action: the key must keep the trainer's state format, so that the
    retired trainer is not handed to a fp32-state job."""
    import time

    from tiresias_amd.executor.cluster_runtime import Worker

    w = Worker(0, 1, torch.device("cpu"))
    act = {"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1, "ranks": (0,),
           "source": "fresh", "opt_dtype": "bf16"}
    b = w._make_trainer(act)
    w.trainers["1"] = b
    bf16_key = b.pool_key
    for extra in ({"opt_dtype": "bf16"}, {}):            # the move's action with and without the key
        move = {"op": "start", "job": "1", "model": "transformer_tiny", "batch": None, "seed": 1, "ranks": (0,),
                "source": "p2p", "old": (0,), "donors": {}, **extra}
        w._apply_one(move, "start", {}, {}, time.perf_counter(), "start_p2p")
        assert b.pool_key == bf16_key and b.pool_key[-1] == "bf16"
    w._retire(w.trainers.pop("1"))
    assert w.pool.get(("transformer_tiny", None, (0,)), []) == [] and w.pool[bf16_key] == [b]
    f = w._make_trainer(dict(act, job="2", seed=2, opt_dtype=None))
    assert f is not b and f.opt_dtype == "fp32" and all(s.dtype == torch.float32 for s in f.opt_state)
    assert w._make_trainer(dict(act, job="3", seed=3)) is b
    # and a trainer of the other format that did end up under a key is not handed out
    w.pool.setdefault(f.pool_key, []).append(b)
    with pytest.raises(RuntimeError, match="bf16-state trainer is pooled"):
        w._make_trainer(dict(act, job="4", seed=4, opt_dtype="fp32"))


def test_cost_models_price_the_format(tmp_path):
    """The simulator's checkpoint model (JobSpec.opt_dtype) and the fake
    backend's world model (the start action's key) move 8 B per parameter for
    a bf16-state Adam job, 12 B for a fp32-state one."""
    from types import SimpleNamespace

    from tiresias_amd.core.job import JobSpec
    from tiresias_amd.engine.ckpt_model import CkptCostModel
    from tiresias_amd.executor import fake
    from tiresias_amd.executor.spool import Spool
    from tiresias_amd.profiler.skew import model_profile

    n = model_profile("gnmt").params
    cm = CkptCostModel("host")
    sizes = {odt: cm.state_bytes_per_gpu(SimpleNamespace(spec=JobSpec("j", 0.0, 1.0, 1, model="gnmt", opt_dtype=odt)))
             for odt in (None, "fp32", "bf16")}
    assert sizes[None] == sizes["fp32"] == 14 * n and sizes["bf16"] == 10 * n
    assert fake._state_bytes("gnmt") == 14 * n and fake._state_bytes("gnmt", "bf16") == 10 * n
    assert fake._state_bytes("vgg16") - fake._state_bytes("vgg16", "bf16") == 2 * model_profile("vgg16").params
    # the controller puts the format on the job's spec
    sp = Spool(str(tmp_path / "spool"))
    sp.submit("gnmt", 1, iterations=2, job_id="b", opt_dtype="bf16")
    sp.submit("gnmt", 1, iterations=2, job_id="f")
    sp.shutdown()
    ctrl, _ = _fake_controller_run(sp)
    assert ctrl.rjobs["b"].spec.opt_dtype == "bf16" and ctrl.rjobs["f"].spec.opt_dtype is None
