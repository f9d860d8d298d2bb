"""Multi-process (gloo, CPU) tests of the distributed paths: bucketed DDP
all-reduce, gang state moves between ranks (the xGMI P2P path on GPUs), and
a full scheduler-driven replay with gangs and preemption (SURVEY §4 plan 5)."""
import os
import time
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)


def _ddp_worker(rank, world, port, q):
    _init(rank, world, port)
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer("resnet_tiny", "cpu", seed=11, data_seed=100 + rank, group=dist.group.WORLD, bucket_mb=0.05)
    assert t.ddp is not None and len(t.ddp.buckets) > 1
    # reference: sum of the per-rank local gradients, then averaged
    loc = Trainer("resnet_tiny", "cpu", seed=11, data_seed=100 + rank)
    loc._fwd_bwd()
    g = loc.arena.grad.clone()
    dist.all_reduce(g)
    g /= world
    t._fwd_bwd()
    t.ddp.finish()
    t_grad = t.arena.grad.clone() / world
    err = ((t_grad - g).norm() / g.norm()).item()
    for _ in range(3):                        # overlap path after the first (learning) step
        t.step()
    w = t.arena.master.clone()
    ws = [torch.zeros_like(w) for _ in range(world)]
    dist.all_gather(ws, w)
    same = all(torch.equal(ws[0], x) for x in ws)
    q.put((rank, err, same, t.ddp.uses is not None))
    dist.destroy_process_group()


def test_bucketed_ddp_matches_allreduce_average():
    world = 2
    port = _free_port()
    q = mp.get_context("spawn").SimpleQueue()
    mp.spawn(_ddp_worker, args=(world, port, q), nprocs=world, join=True)
    res = [q.get() for _ in range(world)]
    for rank, err, same, learned in res:
        assert err < 1e-5, f"rank {rank} bucketed grad differs: {err}"
        assert same, "replicas diverged"
        assert learned


def _move_worker(rank, world, port, outdir):
    _init(rank, world, port)
    from tiresias_amd.executor.cluster_runtime import Worker

    w = Worker(rank, world, torch.device("cpu"), dist.group.WORLD)
    base = {"op": "start", "job": "7", "model": "transformer_tiny", "batch": None, "seed": 7}
    # fresh on rank 0, train 2 steps
    plan = {"actions": [dict(base, ranks=(0,), source="fresh")], "assign": {0: [("7", 2)]}}
    w.apply(plan)
    w.run(plan)
    snap = None
    if rank == 0:
        snap = w.trainers["7"].arena.master.clone().numpy()
    # preempted, then resumed on rank 1: state moves 0 -> 1
    plan = {"actions": [dict(base, ranks=(1,), source="p2p", donors={1: 0}, old=(0,))],
            "assign": {}}
    w.apply(plan)
    out = {}
    if rank == 1:
        out["moved"] = w.trainers["7"].arena.master.clone().numpy()
        out["opt"] = w.trainers["7"].opt_state[0].abs().sum().item()
    else:
        out["freed"] = "7" not in w.trainers
        out["snap"] = snap
    torch.save(out, os.path.join(outdir, f"r{rank}.pt"))
    dist.destroy_process_group()


def test_state_moves_between_ranks(tmp_path):
    world = 2
    port = _free_port()
    mp.spawn(_move_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    res = {r: torch.load(tmp_path / f"r{r}.pt", weights_only=False) for r in range(world)}
    assert res[0]["freed"]
    assert (res[0]["snap"] == res[1]["moved"]).all()
    assert res[1]["opt"] > 0            # optimizer state travelled too


def _replay_worker(rank, world, port, q):
    _init(rank, world, port)
    ctrl = dist.new_group(backend="gloo")
    import bench
    from tiresias_amd.executor.cluster_runtime import Worker, run_replay

    jobs = bench.bench_trace(world, 3, seed=5, work_s=0.6, tiny=True)
    # force a gang job
    jobs[1].spec.num_gpu = world
    cfg = bench.make_cfg("dlas-gpu", "tiresias", world, 5)
    w = Worker(rank, world, torch.device("cpu"), dist.group.WORLD)
    s = run_replay(cfg, jobs, rank, world, torch.device("cpu"), ctrl_pg=ctrl,
                   world_pg=dist.group.WORLD, worker=w, quantum=0.2)
    q.put((rank, s))
    dist.destroy_process_group()


@pytest.mark.slow
def test_live_replay_with_gangs():
    world = 2
    port = _free_port()
    q = mp.get_context("spawn").SimpleQueue()
    mp.spawn(_replay_worker, args=(world, port, q), nprocs=world, join=True)
    res = dict(q.get() for _ in range(world))
    s = res[0]
    assert s["finished"] == s["jobs"] == 6 and s["failed"] == 0
    assert s["avg_jct"] > 0 and s["makespan"] > 0
    assert res[1] is None


def _fault_worker(rank, world, port, outdir):
    import datetime

    # the gloo control plane has no heartbeat to bound a gang communicator's
    # rendezvous with the dying rank (the store plane does): keep that bound
    # under the test's join limit, or a loss that lands in a rendezvous waits
    # out the 180 s default (read at import of parallel/gang.py, below)
    os.environ["TAM_COMM_CREATE_TIMEOUT_S"] = "30"
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=20))
    torch.set_num_threads(1)
    ctrl = dist.new_group(backend="gloo", timeout=datetime.timedelta(seconds=20))
    import bench
    from tiresias_amd.executor.cluster_runtime import Worker, run_replay

    jobs = bench.bench_trace(world, 3, seed=5, work_s=0.6, tiny=True)
    cfg = bench.make_cfg("dlas-gpu", "count", world, 5)
    w = Worker(rank, world, torch.device("cpu"), dist.group.WORLD)
    s = run_replay(cfg, jobs, rank, world, torch.device("cpu"), ctrl_pg=ctrl, world_pg=dist.group.WORLD,
                   worker=w, quantum=0.1, fault={"rank": 1, "round": 3}, control="gloo")
    torch.save(s, os.path.join(outdir, f"f{rank}.pt"))
    os._exit(0)


def test_rank_failure_is_detected(tmp_path):
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=_fault_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(120)
    alive = [p.pid for p in ps if p.is_alive()]
    for p in ps:
        if p.is_alive():
            p.kill()
    assert ps[1].exitcode == 17
    assert (tmp_path / "f0.pt").exists(), f"rank 0 wrote no result: exitcode {ps[0].exitcode}, still running {alive}"
    s = torch.load(tmp_path / "f0.pt", weights_only=False)
    assert s["aborted"] and "rank lost" in s["reason"]


def test_trainer_offload_restore_roundtrip_cpu():
    from tiresias_amd.executor.cluster_runtime import _HostEngine
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer("resnet_tiny", "cpu", seed=1)
    t.step()
    before = t.arena.master.clone()
    mom = t.opt_state[0].clone()
    eng = _HostEngine()
    n = t.offload(eng)
    assert n > 0 and t.arena.master.untyped_storage().nbytes() == 0
    t.restore()
    assert torch.equal(t.arena.master, before) and torch.equal(t.opt_state[0], mom)
    assert torch.equal(t.arena.shadow, before.to(torch.bfloat16))
    t.step()   # keeps training after the round trip


def _spill_replay_worker(rank, world, port, outdir):
    _init(rank, world, port)
    ctrl = dist.new_group(backend="gloo")
    import bench
    from tiresias_amd.executor.cluster_runtime import Worker, run_replay

    jobs = bench.bench_trace(world, 4, seed=9, work_s=1.2, tiny=True)
    # attained service is measured wall time, so the queue limits sit far below
    # what the long jobs run for (0.3-1 s each) on any host: with the default
    # 1.0 GPU-s limit the longest job ended within a few percent of it, and
    # whether anything was demoted (and preempted) depended on the CPU's speed
    cfg = bench.make_cfg("dlas-gpu", "count", world, 9, qlimits=[0.05, 0.3])
    cfg.ckpt_policy = "host"
    w = Worker(rank, world, torch.device("cpu"), dist.group.WORLD)
    s = run_replay(cfg, jobs, rank, world, torch.device("cpu"), ctrl_pg=ctrl,
                   world_pg=dist.group.WORLD, worker=w, quantum=0.1)
    torch.save({"s": s, "spilled": w.spilled_bytes, "restored": w.restored_bytes},
               os.path.join(outdir, f"s{rank}.pt"))
    dist.destroy_process_group()


def test_live_replay_with_host_spill(tmp_path):
    world = 2
    mp.spawn(_spill_replay_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    r0 = torch.load(tmp_path / "s0.pt", weights_only=False)
    r1 = torch.load(tmp_path / "s1.pt", weights_only=False)
    s = r0["s"]
    assert s["finished"] == s["jobs"] and s["preemptions"] > 0
    assert r0["spilled"] + r1["spilled"] > 0
    assert r0["restored"] + r1["restored"] > 0


def test_live_replay_gpu_sharing_packs_jobs():
    """GPU sharing in the live runtime (reference --pack / dlas-gpu-pack,
    SURVEY §2.3): with pack placement several jobs share one rank in a round
    (run concurrently on per-job streams on a GPU) and every job finishes."""
    import dataclasses

    import bench
    from tiresias_amd.executor import cluster_runtime as cr

    jobs = bench.bench_trace(1, 6, seed=9, work_s=0.6, tiny=True)
    for j in jobs:
        j.spec.submit_time = 0.0                 # all queued at once -> contention
        j.spec.gpu_mem_max = 1000.0
    cfg = dataclasses.replace(bench.make_cfg("dlas-gpu-pack", "pack", 1, 9), pack=True)
    seen = []
    w = cr.Worker(0, 1, torch.device("cpu"))
    orig = w.run

    def run(plan):
        seen.append(len(plan["assign"].get(0) or []))
        return orig(plan)

    w.run = run
    s = cr.run_replay(cfg, jobs, 0, 1, torch.device("cpu"), worker=w, quantum=0.05)
    assert s["finished"] == len(jobs) and s["failed"] == 0
    assert max(seen) >= 2, "no round co-located jobs"


def test_round_ends_at_next_arrival():
    """A 1-GPU job's round stops at the first step boundary after the next
    trace arrival (plan["deadline"]) and reports the steps it really ran;
    without a deadline it runs its full assignment."""
    import time

    from tiresias_amd.executor import cluster_runtime as cr

    w = cr.Worker(0, 1, torch.device("cpu"))
    start = {"op": "start", "job": "1", "model": "resnet_tiny", "batch": None, "seed": 1,
             "ranks": (0,), "source": "fresh"}
    w.apply({"actions": [start], "assign": {}})
    r = w.run({"actions": [], "assign": {0: [("1", 5)]}, "deadline": time.perf_counter() - 1.0})
    assert r["jobs"][0]["iters"] == 1
    r = w.run({"actions": [], "assign": {0: [("1", 3)]}, "deadline": None})
    assert r["jobs"][0]["iters"] == 3
    r = w.run({"actions": [], "assign": {0: [("1", 2)]}, "deadline": time.perf_counter() + 60})
    assert r["jobs"][0]["iters"] == 2


def _recover_worker(rank, world, port, outdir, fault, hb_timeout=5.0, gang_timeout=12.0, snapshot_s=0.0):
    import datetime

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["TAM_GANG_TIMEOUT_S"] = str(int(gang_timeout))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    torch.set_num_threads(1)
    ctrl = dist.new_group(backend="gloo", timeout=datetime.timedelta(seconds=60))
    import bench
    from tiresias_amd.executor.cluster_runtime import Worker, run_replay
    from tiresias_amd.parallel import gang

    gang.GANG_TIMEOUT_S = gang_timeout
    import faulthandler

    # a rank still running after 60 s leaves every thread's stack behind
    stacks = open(os.path.join(outdir, f"stacks{rank}.txt"), "w")
    faulthandler.dump_traceback_later(60.0, repeat=True, file=stacks)
    jobs = bench.bench_trace(world, 4, seed=3, work_s=0.8, min_iters=4, tiny=True)
    for i in (0, 2, 5):                    # gangs spanning the victim rank
        jobs[i].spec.num_gpu = 2 if i != 5 else world - 1
    if fault.get("kind", "crash") in ("crash", "hang"):
        # once a rank is lost, every unfinished gang as wide as the cluster
        # fails. The trace draws three such gangs, and how many are unfinished
        # at the fault's round depends on the host's speed (the first round
        # ends within milliseconds of the last arrival: one round more or less
        # before the fault). Keep the first one only (it runs, and opens the
        # whole-cluster communicator, rounds before the fault), so that at most
        # one job can fail whatever the timing
        for j in [j for j in jobs if j.spec.num_gpu == world][1:]:
            j.spec.num_gpu = world - 1
    if snapshot_s > 0:                    # every job a single replica: a loss needs the snapshot
        for j in jobs:
            j.spec.num_gpu = 1
    cfg = bench.make_cfg("dlas-gpu", "count", world, 3, qlimits=[0.05, 0.3])
    w = Worker(rank, world, torch.device("cpu"), dist.group.WORLD, snapshot_s=snapshot_s,
               snapshot_dir=os.path.join(outdir, "snap"))
    try:
        s = run_replay(cfg, jobs, rank, world, torch.device("cpu"), ctrl_pg=ctrl, world_pg=dist.group.WORLD,
                       worker=w, quantum=0.05, fault=dict(fault), hb_timeout=hb_timeout, hb_period=0.3,
                       out_dir=outdir if rank == 0 else None)
    except BaseException:
        import traceback

        with open(os.path.join(outdir, f"err{rank}.txt"), "w") as f:
            f.write(traceback.format_exc())
        os._exit(3)
    torch.save(s, os.path.join(outdir, f"r{rank}.pt"))
    os._exit(0)


def _run_recover(tmp_path, fault, world=4, hb_timeout=5.0, gang_timeout=12.0, snapshot_s=0.0):
    port = _free_port()
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=_recover_worker, args=(r, world, port, str(tmp_path), fault, hb_timeout,
                                                     gang_timeout, snapshot_s)) for r in range(world)]
    for p in ps:
        p.start()
    deadline = time.time() + 240              # one bound for the whole gang, not per process
    hung = fault.get("rank") if fault.get("kind") == "hang" else None
    for r, p in enumerate(ps):
        if r != hung:
            p.join(max(1.0, deadline - time.time()))
    for p in ps:
        if p.is_alive():
            p.kill()
            p.join(10)
    return ps, torch.load(tmp_path / "r0.pt", weights_only=False)


@pytest.mark.slow
def test_rank_loss_is_recovered_in_process(tmp_path):
    """world 4, rank 3 crashes mid-replay: the store-plane heartbeat detects it
    within seconds, its GPU leaves the cluster, gangs that spanned it resume
    from their surviving replicas, and every job that still fits finishes."""
    ps, s = _run_recover(tmp_path, {"rank": 3, "round": 6, "kind": "crash"})
    errs = {f.name: f.read_text()[-1500:] for f in tmp_path.glob("err*.txt")}
    assert ps[3].exitcode == 17 and all(p.exitcode == 0 for p in ps[:3]), ([p.exitcode for p in ps], errs)
    assert s["lost_ranks"] == [3]
    assert not s.get("aborted")
    assert s["finished"] + s["failed"] == s["jobs"]
    assert s["failed"] <= 1                       # at most the (world-1)-GPU gang... which still fits
    assert s["recovered_jobs"] or s["restarted_jobs"]


@pytest.mark.slow
def test_delayed_allreduce_is_slow_not_lost(tmp_path):
    """A straggler (rank 2 stalls 8 s, past the 5 s heartbeat timeout,
    delaying its gang's all-reduce, inside the 12 s gang timeout) is NOT
    declared lost: its heartbeat thread keeps beating; the replay completes
    with every job. (Round 2 shipped this at 5 s after an 8 s stall wedged a
    run; the wedge was a gang that kept stepping on a communicator whose
    collective had timed out -- now recovered, see the next test.)"""
    ps, s = _run_recover(tmp_path, {"rank": 2, "round": 4, "kind": "delay", "seconds": 8.0},
                         hb_timeout=5.0, gang_timeout=12.0)
    errs = {f.name: f.read_text()[-1500:] for f in tmp_path.glob("err*.txt")}
    assert all(p.exitcode == 0 for p in ps), ([p.exitcode for p in ps], errs)
    assert s["lost_ranks"] == [] and s["finished"] == s["jobs"]


@pytest.mark.slow
def test_gang_timeout_is_recovered(tmp_path):
    """A straggler stalling LONGER than the gang communicator timeout (6 s vs
    2 s) fails its gang's collective. The failure is recovered, not wedged:
    the controller preempts the job, aborts the communicator (and re-creates
    it under a new generation), and resumes the gang from ONE replica copied
    to every member; the rank is not lost and every job finishes."""
    ps, s = _run_recover(tmp_path, {"rank": 2, "round": 2, "kind": "delay", "seconds": 6.0, "where": "step"},
                         hb_timeout=5.0, gang_timeout=2.0)
    errs = {f.name: f.read_text()[-1500:] for f in tmp_path.glob("err*.txt")}
    assert all(p.exitcode == 0 for p in ps), ([p.exitcode for p in ps], errs)
    assert s["lost_ranks"] == [] and s["finished"] == s["jobs"] and s["failed"] == 0
    assert s["gang_errors"] >= 1
    assert s["comm_stats"]["aborted"] >= 1


@pytest.mark.slow
def test_hung_rank_is_declared_lost(tmp_path):
    """Rank 3 hangs (no heartbeat, never returns) while gang peers may be
    blocked in a collective with it: rank 0's monitor thread declares it lost
    on its own, the survivors' communicators containing it are aborted, and
    the replay finishes on the remaining ranks."""
    ps, s = _run_recover(tmp_path, {"rank": 3, "round": 6, "kind": "hang"}, hb_timeout=3.0, gang_timeout=8.0)
    errs = {f.name: f.read_text()[-1500:] for f in tmp_path.glob("err*.txt")}
    assert all(p.exitcode == 0 for p in ps[:3]), ([p.exitcode for p in ps], errs)
    assert s["lost_ranks"] == [3] and not s.get("aborted")
    assert s["finished"] + s["failed"] == s["jobs"] and s["failed"] <= 1


def test_hbm_pressure_spills_only_when_needed(tmp_path):
    """ckpt policy "pressure": suspended jobs stay resident until a starting
    job needs the memory; then the least recently run ones spill (and are
    restored when resumed). A budget large enough for everything spills
    nothing; job.csv carries the measured bytes."""
    import csv

    import bench
    from tiresias_amd.executor import cluster_runtime as cr
    from tiresias_amd.executor.trainer import Trainer

    one = Trainer("resnet_tiny", "cpu").hbm_bytes()
    jobs = bench.bench_trace(1, 10, seed=4, work_s=0.4, min_iters=3, tiny=True)
    for j in jobs:
        j.model = "resnet_tiny"
    cfg = bench.make_cfg("dlas-gpu", "count", 1, 4, "pressure", [0.01, 0.05])
    w = cr.Worker(0, 1, torch.device("cpu"), hbm_budget_gb=2.5 * one / 2 ** 30, pool_cap=0)
    s = cr.run_replay(cfg, jobs, 0, 1, torch.device("cpu"), worker=w, quantum=0.02, out_dir=str(tmp_path))
    assert s["finished"] == len(jobs) and s["preemptions"] > 0
    assert w.pressure_spills > 0 and w.restored_bytes > 0
    rows = list(csv.DictReader(open(tmp_path / "job.csv")))
    assert sum(float(r["ckpt_bytes"]) for r in rows) > 0
    big = cr.Worker(0, 1, torch.device("cpu"), hbm_budget_gb=1000.0, pool_cap=0)
    s2 = cr.run_replay(cfg, jobs, 0, 1, torch.device("cpu"), worker=big, quantum=0.02)
    assert s2["finished"] == len(jobs) and big.pressure_spills == 0 and big.spilled_bytes == 0


@pytest.mark.slow
def test_rank_loss_restarts_from_snapshot(tmp_path):
    """Periodic durable snapshots (ckpt/snapshot.py, every 0.02 s of a job's
    run time): rank 3 crashes mid-replay; a job whose ONLY replica lived on
    rank 3 resumes from its last snapshot's iteration (not 0) on another
    rank, the redone iterations are charged in job.csv (lost_iters), and
    every job still finishes."""
    import csv
    import json

    ps, s = _run_recover(tmp_path, {"rank": 3, "round": 3, "kind": "crash", "when": "snapshotted"},
                         snapshot_s=0.02)
    errs = {f.name: f.read_text()[-1500:] for f in tmp_path.glob("err*.txt")}
    assert ps[3].exitcode == 17 and all(p.exitcode == 0 for p in ps[:3]), ([p.exitcode for p in ps], errs)
    assert s["lost_ranks"] == [3] and s["finished"] + s["failed"] == s["jobs"]
    assert s["snapshot_restored_jobs"], s
    dec = [json.loads(x) for x in open(tmp_path / "decisions.jsonl")]
    rs = [d for d in dec if d["ev"] == "restart" and d["source"] == "snapshot"]
    assert rs and all(d["from_step"] > 0 for d in rs)
    rows = {r["job_id"]: r for r in csv.DictReader(open(tmp_path / "job.csv"))}
    for d in rs:
        assert int(rows[d["job"]]["lost_iters"]) == d["lost_iters"]


@pytest.mark.slow
def test_unreadable_snapshot_restarts_from_scratch(tmp_path):
    """Rank 3 crashes AND tears the shared snapshot store (every snapshot
    file truncated): the ranks that restart a job from its snapshot fail to
    read it, agree on that verdict (nobody runs it on garbage state), and the
    controller restarts the job from scratch, charging every iteration the
    snapshot held (lost_iters) -- the replay still finishes every job."""
    import csv
    import json

    ps, s = _run_recover(tmp_path, {"rank": 3, "round": 3, "kind": "crash", "corrupt_snapshots": True,
                                    "when": "snapshotted"}, snapshot_s=0.02)
    errs = {f.name: f.read_text()[-1500:] for f in tmp_path.glob("err*.txt")}
    assert ps[3].exitcode == 17 and all(p.exitcode == 0 for p in ps[:3]), ([p.exitcode for p in ps], errs)
    assert s["lost_ranks"] == [3] and s["finished"] + s["failed"] == s["jobs"]
    dec = [json.loads(x) for x in open(tmp_path / "decisions.jsonl")]
    bad = [d for d in dec if d["ev"] == "restart" and d.get("reason") == "snapshot unreadable"]
    tried = [d for d in dec if d["ev"] == "restart" and d["source"] == "snapshot"]
    assert tried, "no job needed its snapshot"
    assert {d["job"] for d in bad} == {d["job"] for d in tried}
    rows = {r["job_id"]: r for r in csv.DictReader(open(tmp_path / "job.csv"))}
    for d in tried:
        # the iterations redone before the crash and the ones the snapshot held
        assert int(rows[d["job"]]["lost_iters"]) == d["lost_iters"] + d["from_step"]


def test_snapshot_needs_shared_dir():
    from tiresias_amd.executor.cluster_runtime import Worker

    with pytest.raises(ValueError, match="snapshot_dir"):
        Worker(0, 1, torch.device("cpu"), snapshot_s=1.0)


def test_heartbeat_liveness_ignores_wall_clock(monkeypatch):
    """Liveness is a heartbeat COUNTER timed on rank 0's monotonic clock
    (executor/control.py): with the wall clock unusable (skewed hosts; here
    time.time raises) a beating rank stays alive, and a rank whose counter
    stops is declared lost within about hb_timeout."""
    from tiresias_amd.executor import control

    port = _free_port()
    master = dist.TCPStore("127.0.0.1", port, is_master=True, wait_for_workers=False)
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", str(port))

    def _no_wall_clock():
        raise AssertionError("liveness must not read the wall clock")

    monkeypatch.setattr(control.time, "time", _no_wall_clock)
    dead = []
    p1 = control.StorePlane(1, 2, hb_period=0.1, hb_timeout=0.8, store=master)
    p0 = control.StorePlane(0, 2, hb_period=0.1, hb_timeout=0.8, store=master, on_dead=dead.append)
    try:
        time.sleep(2.5)
        assert dead == [] and p0.heartbeat_age(1) < 0.5
        p1.close()                                    # the rank stops beating
        t0 = time.monotonic()
        while not dead and time.monotonic() - t0 < 5.0:
            time.sleep(0.05)
        assert dead == [1]
        assert time.monotonic() - t0 < 0.8 + 1.0
    finally:
        p0.close()
        p1.close()


# ------------------------------------------------------------------ DDP bucket layout
@pytest.mark.parametrize("model", ["resnet50", "vgg16", "transformer", "gnmt", "transformer_tiny", "gnmt_tiny"])
@pytest.mark.parametrize("bucket_mb", [32.0, 0.1, 0.2])
def test_ddp_bucket_ranges_are_disjoint(model, bucket_mb):
    """Every DDP bucket is ONE contiguous arena range, buckets never overlap,
    and every param is in exactly one bucket whose range holds it. (Full-size
    Transformer-base at the default 32 MB used to get a bucket spanning the
    store_grad region: its Linear gradients were all-reduced twice.)"""
    from tiresias_amd.models import make_model
    from tiresias_amd.ops.arena import Arena
    from tiresias_amd.parallel.ddp import GradBucketer

    a = Arena("cpu")
    make_model(model, a)
    a.layout()                                     # offsets only, no allocation
    a.grad = torch.empty(0, device="meta")
    b = GradBucketer(a, None, bucket_mb=bucket_mb)
    rs = sorted(b.ranges)
    for (lo0, hi0), (lo1, _) in zip(rs, rs[1:]):
        assert hi0 <= lo1
    seen = set()
    for bi, ps in enumerate(b.buckets):
        lo, hi = b.ranges[bi]
        for p in ps:
            assert lo <= p.offset and p.offset + p.numel <= hi
            assert id(p) not in seen
            seen.add(id(p))
        # contiguous: the bucket's params tile its range (64-element padding)
        assert sum((p.numel + 63) // 64 * 64 for p in ps) >= (hi - lo) - 64
    assert len(seen) == len(a.params)


def _ddp_adam_worker(rank, world, port, q, model, bucket_mb):
    _init(rank, world, port)
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer(model, "cpu", seed=3, data_seed=40 + rank, group=dist.group.WORLD, bucket_mb=bucket_mb)
    # single-process reference: local gradients, averaged by hand, same Adam
    loc = Trainer(model, "cpu", seed=3, data_seed=40 + rank)
    for _ in range(3):
        t.step()
        loc._fwd_bwd()
        dist.all_reduce(loc.arena.grad)
        loc.arena.grad /= world
        loc._opt_step()
        loc.arena.grad.zero_()
    err = float((t.arena.master - loc.arena.master).norm() / loc.arena.master.norm())
    q.put((rank, err, t.ddp.bytes_reduced, t.arena.numel))
    dist.destroy_process_group()


@pytest.mark.parametrize("model,bucket_mb", [("transformer_tiny", 0.1), ("gnmt_tiny", 0.2)])
def test_ddp_adam_matches_single_process(model, bucket_mb):
    """World-2 bucketed DDP + Adam matches one process averaging the same
    gradients by hand, at bucket sizes whose buckets used to overlap; every
    gradient element is reduced exactly once per step."""
    world = 2
    q = mp.get_context("spawn").SimpleQueue()
    mp.spawn(_ddp_adam_worker, args=(world, _free_port(), q, model, bucket_mb), nprocs=world, join=True)
    for _ in range(world):
        rank, err, nbytes, numel = q.get()
        assert err < 1e-5, (rank, err)
        assert nbytes <= 3 * numel * 4, (nbytes, numel)


def _shard_pressure_worker(rank, world, port, outdir):
    _init(rank, world, port)
    ctrl = dist.new_group(backend="gloo")
    import bench
    from tiresias_amd.executor.cluster_runtime import Worker, run_replay
    from tiresias_amd.executor.trainer import Trainer

    one = Trainer("transformer_tiny", "cpu").hbm_bytes()
    jobs = bench.bench_trace(world, 5, seed=13, work_s=0.6, min_iters=3, tiny=True)
    for j in jobs:
        j.model = "transformer_tiny"
        j.spec.num_gpu = world                     # every job a 2-rank sharded gang
    cfg = bench.make_cfg("dlas-gpu", "count", world, 13, "pressure", [0.01, 0.05])
    cfg.ddp_shard = True
    w = Worker(rank, world, torch.device("cpu"), dist.group.WORLD, ddp_shard=True,
               hbm_budget_gb=2.5 * one / 2 ** 30, pool_cap=0)
    refused = []
    orig = w._spill

    def spill(jid):
        # a pressure victim must never be a member still holding only its slices
        if w.trainers[jid].state_sharded:
            refused.append(jid)
        orig(jid)

    w._spill = spill
    s = run_replay(cfg, jobs, rank, world, torch.device("cpu"), ctrl_pg=ctrl,
                   world_pg=dist.group.WORLD, worker=w, quantum=0.05)
    torch.save({"s": s, "spills": w.pressure_spills, "refused": refused}, os.path.join(outdir, f"p{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.slow
def test_sharded_gangs_under_hbm_pressure(tmp_path):
    """Sharded data parallelism + ckpt policy "pressure" (world 2, gloo):
    preempted gangs are consolidated before any pressure spill can pick them,
    suspended gangs DO get spilled (and restored), and every job finishes."""
    world = 2
    mp.spawn(_shard_pressure_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    res = [torch.load(tmp_path / f"p{r}.pt", weights_only=False) for r in range(world)]
    s = res[0]["s"]
    assert s["finished"] == s["jobs"] and s["preemptions"] > 0, s
    assert s["ddp_shard"] and s["consolidations"] > 0, s
    assert sum(r["spills"] for r in res) > 0
    assert all(not r["refused"] for r in res)


def test_offload_refuses_sharded_state():
    from tiresias_amd.executor.cluster_runtime import _HostEngine
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer("resnet_tiny", "cpu")

    class _D:
        shard, dirty = True, True

    t.ddp = _D()
    with pytest.raises(RuntimeError, match="consolidate"):
        t.offload(_HostEngine())


def test_gang_fill_votes_match_when_one_member_cannot_step():
    """Fill-mode eligibility is partly local (this rank's trainer state and
    its own report): a gang member that cannot step still joins the first
    vote and votes stop, so a peer that could step never waits in a vote the
    member would not join; a lone job with a local error does not fill."""
    from types import SimpleNamespace
    from tiresias_amd.executor.cluster_runtime import Worker

    votes = []

    class Comm:
        def start(self, v):
            votes.append(float(v.item()))
            return v

        def finish(self, hs):
            pass

    def worker(rank, trainer, job_ranks):
        w = Worker.__new__(Worker)
        w.fill_enabled, w.rank, w.device = True, rank, torch.device("cpu")
        w.trainers = {"j": trainer}
        w._job_ranks = {"j": job_ranks}
        w.fill_s_total, w.fill_steps_total = 0.0, 0
        return w

    steps = []
    t = SimpleNamespace(ddp=SimpleNamespace(comm=Comm()), group=None, broken=False, _spilled=None,
                        step=lambda: steps.append(1))
    plan = {"assign": {0: [("j", 0)]}, "left": {"j": 5}}
    bad_rep = {"jobs": [{"job": "j", "error": "RuntimeError: oom"}]}
    w = worker(0, t, (0, 1))
    w.fill_begin(plan, bad_rep)
    assert w._fill is not None and w._fill["left"] == 0
    assert w.fill_step(False) is False and votes == [1.0] and not steps   # one vote: stop
    votes.clear()
    w.fill_begin(plan, {"jobs": []})                      # healthy member: steps until a vote stops
    assert w.fill_step(False) is True and votes == [0.0] and steps == [1]
    solo = worker(0, SimpleNamespace(ddp=None, group=None, broken=False, _spilled=None, step=None), (0,))
    solo.fill_begin(plan, bad_rep)
    assert solo._fill is None


def _fill_gang_worker(rank, world, port, q):
    _init(rank, world, port)
    import time as _t

    from tiresias_amd.executor.cluster_runtime import Worker
    from tiresias_amd.executor.trainer import Trainer

    t = Trainer("resnet_tiny", "cpu", seed=3, data_seed=40 + rank, group=dist.group.WORLD, bucket_mb=0.05)
    w = Worker.__new__(Worker)
    w.fill_enabled, w.rank, w.device = True, rank, torch.device("cpu")
    w.trainers = {"g": t}
    w._job_ranks = {"g": tuple(range(world))}
    w.fill_s_total, w.fill_steps_total = 0.0, 0
    w._fill_cap = {}
    w._carry = []
    counts = []
    for left, stop_after in ((50, (2, 5)), (3, (50, 50)), (50, (0, 4))):
        # the members see "the next plan is out" after different numbers of
        # local steps (stop_after[rank]); the votes must still give every
        # member the same fill step count, never more than ``left``
        w.fill_begin({"assign": {rank: [("g", 0)]}, "left": {"g": left}}, {"jobs": []})
        n = 0
        while w.fill_step(ready=n >= stop_after[rank]):
            n += 1
            _t.sleep(0.001 * (rank + 1))
        counts.append((w.fill_counts().get("g", 0), n))
        w.fill_end({})
        w._carry = []
    wts = [torch.zeros_like(t.arena.master) for _ in range(world)]
    dist.all_gather(wts, t.arena.master)
    q.put((rank, counts, all(torch.equal(wts[0], x) for x in wts)))
    dist.barrier()              # no member tears the store / gloo pairs down under a peer
    dist.destroy_process_group()


def test_gang_fill_steps_equal_on_every_member():
    """fill mode of a 2-rank gang over gloo with the
    round-6 vote (no per-step host drain on the GPU path; bounded waits):
    members whose "next plan is ready" moment differs still run the SAME
    number of fill steps (their gradient all-reduces match), bounded by the
    plan's iterations left, and the replicas stay identical."""
    world = 2
    port = _free_port()
    q = mp.get_context("spawn").SimpleQueue()
    mp.spawn(_fill_gang_worker, args=(world, port, q), nprocs=world, join=True)
    res = sorted(q.get() for _ in range(world))
    (_, c0, same0), (_, c1, same1) = res
    assert same0 and same1
    assert c0 == c1, (c0, c1)
    assert c0[1][0] == 3                      # bounded by left (nobody ready)
    assert c0[0][0] == 2 and c0[2][0] == 0    # the first member ready stops the gang at its next vote
