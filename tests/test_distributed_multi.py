"""World-4/8 multi-process (gloo, CPU) tests of the gang machinery the 8-GPU
node runs on RCCL: hierarchical (spread) vs flat (consolidated) gang
communicators, the measured skew profile driving placement, DDP equivalence
at world 4 on both transports, concurrent disjoint gangs, a gang resumed on a
partially overlapping rank set (P2P donors), a spilled gang restored on other
ranks, and ``torch.distributed.run --nproc-per-node 8 bench.py --cpu``."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _spawn(fn, world, *args):
    mp.spawn(fn, args=(world, _free_port()) + args, nprocs=world, join=True)


# ------------------------------------------------------------------ gang comms
def _comm_worker(rank, world, port, outdir):
    _init(rank, world, port)
    import time

    from tiresias_amd.parallel.gang import FlatComm, HierComm, create_gang_comm

    cons = create_gang_comm([0, 1], rank, vnode_size=2, backend="gloo", nic_gbps=0.05)
    spread = create_gang_comm([0, 2], rank, vnode_size=2, backend="gloo", nic_gbps=0.05)
    spread4 = create_gang_comm([0, 1, 2, 3], rank, vnode_size=2, backend="gloo", nic_gbps=0.05)
    out = {"cons_kind": type(cons).__name__ if cons else None,
           "spread_kind": type(spread).__name__ if spread else None}
    n = 1 << 20                                   # 4 MB per bucket, 2 buckets
    for name, comm in (("cons", cons), ("spread", spread), ("spread4", spread4)):
        if comm is None:
            continue
        bufs = [torch.full((n,), float(rank + 1 + b)) for b in range(2)]
        t0 = time.perf_counter()
        comm.finish([comm.start(x) for x in bufs])
        out[name + "_s"] = time.perf_counter() - t0
        out[name + "_val"] = [float(x[0]) for x in bufs] + [float(x[-1]) for x in bufs]
        if isinstance(comm, HierComm):
            comm.close()
    assert cons is None or isinstance(cons, FlatComm)
    torch.save(out, os.path.join(outdir, f"c{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_spread_gang_pays_the_internode_link(tmp_path):
    """world 4 as 2 virtual nodes of 2: {0,1} is consolidated (flat), {0,2}
    and {0,1,2,3} are spread (hierarchical). All sum correctly; the spread
    sync of 8 MB over a 0.05 GB/s emulated link takes >= bytes/rate."""
    _spawn(_comm_worker, 4, str(tmp_path))
    r = {k: torch.load(tmp_path / f"c{k}.pt", weights_only=False) for k in range(4)}
    assert r[0]["cons_kind"] == "FlatComm" and r[0]["spread_kind"] == "HierComm"
    assert r[0]["cons_val"] == [3.0, 5.0, 3.0, 5.0]                 # ranks 0+1: (1+2), (2+3)
    assert r[2]["spread_val"] == [4.0, 6.0, 4.0, 6.0]               # ranks 0+2: (1+3), (2+4)
    assert r[3]["spread4_val"] == [10.0, 14.0, 10.0, 14.0]
    link_s = 2 * (1 << 22) / 0.05e9                                 # 2 buckets, k=2 leaders
    assert r[0]["spread_s"] >= 0.95 * link_s
    assert r[0]["spread_s"] > 3 * r[0]["cons_s"]


# ------------------------------------------------------------------ measured skew -> placement
def _skew_worker(rank, world, port, outdir):
    _init(rank, world, port)
    from tiresias_amd.profiler.comm import CommProfiler, default_gang_sets, save

    # a slow emulated NIC: the throttled exchange (a timed sleep) dominates the
    # CPU-bound gloo work, so the verdict holds on a loaded host too
    prof = CommProfiler(dist.group.WORLD, device=torch.device("cpu"), iters=1, warmup=0, vnode_size=2,
                        nic_gbps=0.2)
    sets = default_gang_sets(world, 2, 2)
    times = prof.profile_models(["resnet50", "vgg16"], sets)
    if rank == 0:
        # CPU gloo syncs are far slower than GPU steps: judge slowdown against a
        # CPU-scale step time so the comparison stays meaningful
        res = CommProfiler.classify(times, threshold=1.25, iter_s={"resnet50": 2.0, "vgg16": 2.0})
        save(os.path.join(outdir, "skew.json"), res)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.slow
def test_measured_skew_profile_classifies_vgg_sensitive(tmp_path):
    """The profiler measures the real bucketed gradient sync of VGG-16 and
    ResNet-50 on a consolidated vs a spread gang; VGG-16 (553 MB of
    gradients, 392 MB in one FC tensor) comes out placement-sensitive, and
    the Tiresias placement consolidates it from that measurement."""
    _spawn(_skew_worker, 4, str(tmp_path))
    path = str(tmp_path / "skew.json")
    res = json.load(open(path))
    assert res["vgg16"]["spread_s"] > res["vgg16"]["consolidated_s"]
    assert res["vgg16"]["slowdown"] > res["resnet50"]["slowdown"]
    assert res["vgg16"]["sensitive"]

    from tiresias_amd.config import ClusterSpec, SimConfig
    from tiresias_amd.core.job import JobSpec
    from tiresias_amd.engine.sim import Simulator

    cfg = SimConfig(schedule="fifo", scheme="tiresias", skew_profile=path, virtual_nodes="2x4",
                    cluster=ClusterSpec(num_switch=1, num_node_p_switch=1, num_gpu_p_node=8))
    sim = Simulator(cfg, [JobSpec("v", 0.0, 10.0, 4, model="vgg16")])
    assert sim.placement.sensitivity.source == path
    sim.run(until=1.0)
    assert len(sim.jobs["v"].allocation) == 1                      # consolidated on one virtual node


# ------------------------------------------------------------------ DDP equivalence at world 4
def _ddp4_worker(rank, world, port, q, vnode):
    _init(rank, world, port)
    from tiresias_amd.executor.trainer import Trainer
    from tiresias_amd.parallel.gang import create_gang_comm

    comm = create_gang_comm(list(range(world)), rank, vnode_size=vnode, backend="gloo", nic_gbps=50.0)
    t = Trainer("resnet_tiny", "cpu", seed=11, data_seed=100 + rank, group=comm, bucket_mb=0.05)
    loc = Trainer("resnet_tiny", "cpu", seed=11, data_seed=100 + rank)
    loc._fwd_bwd()
    g = loc.arena.grad.clone()
    dist.all_reduce(g)
    t._fwd_bwd()
    t.ddp.finish()
    err = ((t.arena.grad - g).norm() / g.norm()).item()
    for _ in range(2):
        t.step()
    w = t.arena.master.clone()
    ws = [torch.zeros_like(w) for _ in range(world)]
    dist.all_gather(ws, w)
    q.put((rank, err, all(torch.equal(ws[0], x) for x in ws), type(comm).__name__))
    if hasattr(comm, "close"):
        comm.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("vnode", [0, 2])
def test_ddp_equivalence_world4(vnode):
    world = 4
    q = mp.get_context("spawn").SimpleQueue()
    mp.spawn(_ddp4_worker, args=(world, _free_port(), q, vnode), nprocs=world, join=True)
    res = [q.get() for _ in range(world)]
    for rank, err, same, kind in res:
        assert err < 1e-5, (rank, err)
        assert same
        assert kind == ("HierComm" if vnode else "FlatComm")


# ------------------------------------------------------------------ gang protocol at world 4
def _proto_worker(rank, world, port, outdir):
    _init(rank, world, port)
    from tiresias_amd.executor.cluster_runtime import Worker

    w = Worker(rank, world, torch.device("cpu"), dist.group.WORLD)

    def start(job, ranks, **kw):
        return dict({"op": "start", "job": job, "model": "resnet_tiny", "batch": None, "seed": int(job),
                     "ranks": tuple(ranks)}, **kw)

    def grp(ranks):
        return {"op": "group", "ranks": tuple(ranks), "vnode": 2, "nic_gbps": 50.0}

    out = {}
    # 1) two concurrent, disjoint gangs: job 1 on {0,1}, job 2 on {2,3}
    plan = {"actions": [grp((0, 1)), grp((2, 3)), start("1", (0, 1), source="fresh"),
                        start("2", (2, 3), source="fresh")],
            "assign": {0: [("1", 2)], 1: [("1", 2)], 2: [("2", 2)], 3: [("2", 2)]}}
    w.apply(plan)
    w.run(plan)
    mine = "1" if rank < 2 else "2"
    m = w.trainers[mine].arena.master.clone()
    ms = [torch.zeros_like(m) for _ in range(world)]
    dist.all_gather(ms, m)
    out["disjoint_sync"] = torch.equal(ms[0], ms[1]) and torch.equal(ms[2], ms[3])
    out["disjoint_differ"] = not torch.equal(ms[0], ms[2])
    # 2) job 1 preempted, resumed on the PARTIALLY overlapping set {1,2}
    #    (spread over both virtual nodes): rank 2 receives a replica from 0
    snap = w.trainers["1"].arena.master.clone() if rank in (0, 1) else None
    plan = {"actions": [{"op": "drop", "job": "2", "ranks": (2, 3)}, grp((1, 2)),
                        start("1", (1, 2), source="p2p", donors={2: 0}, old=(0, 1))],
            "assign": {}}
    w.apply(plan)
    if rank == 2:
        out["received"] = w.trainers["1"].arena.master.clone()
    if rank == 1:
        out["kept"] = torch.equal(w.trainers["1"].arena.master, snap)
        out["snap"] = snap
    if rank == 0:
        out["donor_freed"] = "1" not in w.trainers
    plan = {"actions": [], "assign": {1: [("1", 2)], 2: [("1", 2)]}}
    w.run(plan)
    if rank in (1, 2):
        m = w.trainers["1"].arena.master.clone()
    else:
        m = torch.zeros_like(w.pool[next(iter(w.pool))][0].arena.master) if w.pool else torch.zeros(1)
    # 3) job 1 spilled to host on {1,2}, restored and moved to {0,3}
    plan = {"actions": [{"op": "spill", "job": "1", "ranks": (1, 2)}], "assign": {}}
    w.apply(plan)
    if rank in (1, 2):
        out["spilled"] = w.spilled_bytes > 0
        state = w.trainers["1"].arena.master.untyped_storage().nbytes()
        out["hbm_freed"] = state == 0
    plan = {"actions": [grp((0, 3)), start("1", (0, 3), source="p2p", donors={0: 1, 3: 2}, old=(1, 2))],
            "assign": {0: [("1", 1)], 3: [("1", 1)]}}
    w.apply(plan)
    if rank in (0, 3):
        out["after_move"] = w.trainers["1"].arena.master.clone()
    if rank in (1, 2):
        out["before_move"] = m
        out["restored"] = w.restored_bytes > 0
    w.run(plan)
    torch.save(out, os.path.join(outdir, f"p{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_gang_protocol_world4(tmp_path):
    _spawn(_proto_worker, 4, str(tmp_path))
    r = {k: torch.load(tmp_path / f"p{k}.pt", weights_only=False) for k in range(4)}
    assert r[0]["disjoint_sync"] and r[0]["disjoint_differ"]
    assert r[0]["donor_freed"] and r[1]["kept"]
    assert torch.equal(r[2]["received"], r[1]["snap"])
    assert r[1]["spilled"] and r[2]["spilled"] and r[1]["hbm_freed"]
    assert r[1]["restored"] and r[2]["restored"]
    assert torch.equal(r[0]["after_move"], r[1]["before_move"])
    assert torch.equal(r[3]["after_move"], r[2]["before_move"])


# ------------------------------------------------------------------ communicator pre-flight
def _preflight_worker(rank, world, port, q):
    from tiresias_amd.parallel import gang as G

    _init(rank, world, port)
    ctrl = dist.new_group(backend="gloo")
    sets = G.canonical_gang_sets(world)
    groups = {s: G.create_gang_comm(s, rank, backend="gloo") for s in sets}
    out = {"clean": G.preflight(groups, rank, torch.device("cpu"), dist.group.WORLD, ctrl, timeout_s=30)}
    # a member that corrupts its contribution on gang (2, 3)
    c = groups.get((2, 3))
    if c is not None and rank == 2:
        real = c.start
        c.start = lambda t, real=real: real(t.add_(1.0))
    out["corrupt"] = G.preflight(groups, rank, torch.device("cpu"), None, ctrl, timeout_s=30)
    if c is not None and rank == 2:
        c.start = real
    # a member that never joins gang (0, 1, 2, 3): its peers time out
    g2 = {k: v for k, v in groups.items() if not (rank == 3 and k == (0, 1, 2, 3))}
    out["missing"] = G.preflight(g2, rank, torch.device("cpu"), None, ctrl, timeout_s=4)
    q.put((rank, out))
    dist.barrier(group=ctrl)
    os._exit(0)


def test_preflight_names_broken_gangs():
    """bench.py's N > 1 pre-flight (parallel/gang.py preflight) on gloo world
    4: clean communicators pass; a corrupted contribution and a member that
    never joins are both caught, named by rank set, and reported to EVERY
    rank (so all of them stop together)."""
    world = 4
    q = mp.get_context("spawn").SimpleQueue()
    ctx = mp.get_context("spawn")
    port = _free_port()
    ps = [ctx.Process(target=_preflight_worker, args=(r, world, port, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = dict(q.get() for _ in range(world))
    for p in ps:
        p.join(60)
    for r in range(world):
        assert res[r]["clean"] == [], res[r]
        assert res[r]["corrupt"] and all("(2, 3)" in e for e in res[r]["corrupt"]), res[r]
        assert any("timed out" in e and "(0, 1, 2, 3)" in e for e in res[r]["missing"]), res[r]


# ------------------------------------------------------------------ torchrun, 8 ranks
@pytest.mark.slow
def test_torchrun_bench_world8_cpu(tmp_path):
    """The driver's multi-GPU launch shape, rehearsed on gloo with 8 ranks."""
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--cpu", "--gpus", "8", "--steps", "2", "--warmup", "1",
           "--jobs-per-gpu", "6", "--work-s", "0.08", "--min-iters", "1", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["steps"] == 2 and d["finished_jobs"] == 48
    assert d["vs_baseline"] is not None


# ------------------------------------------------------------------ world 8: gang churn + rank loss
def _churn_worker(rank, world, port, outdir, crash_round, shard=False):
    import datetime

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    torch.set_num_threads(1)
    ctrl = dist.new_group(backend="gloo", timeout=datetime.timedelta(seconds=120))
    import bench
    from tiresias_amd.executor.cluster_runtime import Worker, run_replay
    from tiresias_amd.parallel import gang

    gang.GANG_TIMEOUT_S = 20.0
    jobs = bench.bench_trace(world, 7, seed=21, work_s=0.5, min_iters=3, tiny=True)
    sizes = [2, 4, 2, 8, 2, 4]
    for i, j in enumerate(jobs):
        if i % 4 != 3:
            j.spec.num_gpu = sizes[i % len(sizes)]
        j.model = "resnet_tiny" if i % 2 else "transformer_tiny"
    cfg = bench.make_cfg("dlas-gpu", "tiresias", world, 21, qlimits=[0.02, 0.1])
    cfg.ddp_shard = shard
    w = Worker(rank, world, torch.device("cpu"), dist.group.WORLD, ddp_shard=shard)
    w.precreate_groups(gang.canonical_gang_sets(world), vnode=0)
    stats = {"max_pgs": len(gang.PG_CACHE), "gang_starts": 0, "groups": 0, "aborts": 0,
             "n8": sum(1 for j in jobs if j.spec.num_gpu == 8)}
    orig = w.apply

    hist = []

    def apply(plan):
        hist.append((plan.get("round"), [(a["op"], a.get("job"), a.get("ranks"), a.get("source"), a.get("old"))
                                          for a in plan["actions"]], sorted(w.trainers),
                     sorted(plan["assign"].get(rank) or [])))
        for a in plan["actions"]:
            if a["op"] == "start" and len(a["ranks"]) > 1:
                stats["gang_starts"] += 1
            stats["groups"] += a["op"] == "group"
            stats["aborts"] += a["op"] == "abort"
        try:
            orig(plan)
        except Exception:
            with open(os.path.join(outdir, f"plan{rank}.txt"), "w") as f:
                f.write(repr(plan) + "\n" + repr(sorted(w.trainers)) + "\n" + repr(stats) + "\n")
                for h in hist:
                    f.write(repr(h) + "\n")
            raise
        stats["max_pgs"] = max(stats["max_pgs"], len(gang.PG_CACHE))

    w.apply = apply
    try:
        s = run_replay(cfg, jobs, rank, world, torch.device("cpu"), ctrl_pg=ctrl, world_pg=dist.group.WORLD,
                       worker=w, quantum=0.05, fault={"rank": 5, "round": crash_round}, out_dir=outdir,
                       hb_timeout=5.0, hb_period=0.5)
    except BaseException:
        import traceback

        with open(os.path.join(outdir, f"err{rank}.txt"), "w") as f:
            f.write(traceback.format_exc())
        os._exit(3)
    torch.save({"s": s, "stats": stats}, os.path.join(outdir, f"w{rank}.pt"))
    os._exit(0)


@pytest.mark.slow
@pytest.mark.parametrize("shard", [False, True])
def test_world8_gang_churn_and_rank_loss(tmp_path, shard):
    """World 8 (gloo, 8 processes): a trace with >= 40 gang starts of sizes
    2/4/8 under 2D-LAS with preemption, gang_align placement and the 7
    canonical communicators pre-created. Every rank holds at most 15 live
    communicators throughout (the round-2 cache grew without bound), and
    rank 5 crashing mid-replay -- with gangs containing it in flight -- is
    recovered: its communicators are aborted on the survivors, and every job
    that still fits on 7 GPUs finishes. ``shard``: the same with sharded data
    parallelism -- suspended gangs consolidate their state first, and a gang
    that loses a member restarts (its slices died with it)."""
    import time

    world = 8
    port = _free_port()
    ctx = mp.get_context("spawn")
    ps = [ctx.Process(target=_churn_worker, args=(r, world, port, str(tmp_path), 15, shard)) for r in range(world)]
    for p in ps:
        p.start()
    deadline = time.time() + 280
    for p in ps:
        p.join(max(1.0, deadline - time.time()))
    for p in ps:
        if p.is_alive():
            p.kill()
    errs = {f.name: f.read_text()[-1500:] for f in tmp_path.glob("err*.txt")}
    assert ps[5].exitcode == 17, ([p.exitcode for p in ps], errs)
    assert all(p.exitcode == 0 for r, p in enumerate(ps) if r != 5), ([p.exitcode for p in ps], errs)
    res = {r: torch.load(tmp_path / f"w{r}.pt", weights_only=False) for r in range(world) if r != 5}
    s = res[0]["s"]
    assert s["lost_ranks"] == [5] and not s.get("aborted")
    assert s["finished"] + s["failed"] == s["jobs"]
    n8 = res[0]["stats"]["n8"]
    assert s["failed"] <= n8                               # only gangs larger than 7 GPUs can fail
    assert res[0]["stats"]["gang_starts"] >= 40, res[0]["stats"]
    for r, d in res.items():
        assert d["stats"]["max_pgs"] <= 15, (r, d["stats"])
    assert res[0]["stats"]["aborts"] >= 1                  # communicators containing rank 5
    if shard:
        assert s["ddp_shard"] and s["consolidations"] >= 5, s


# ------------------------------------------------------------------ sharded data parallelism
def _shard_worker(rank, world, port, q, wire):
    from tiresias_amd.executor.trainer import Trainer
    from tiresias_amd.parallel import gang as G

    _init(rank, world, port)
    ranks = tuple(range(world))
    comm = G.create_gang_comm(ranks, rank, backend="gloo")
    out = {}
    for model in ("vgg_tiny", "transformer_tiny"):
        ref = Trainer(model, "cpu", seed=7, data_seed=100 + rank, group=comm, bucket_mb=0.02)
        sh = Trainer(model, "cpu", seed=7, data_seed=100 + rank, group=comm, bucket_mb=0.02,
                     ddp_shard=True, ddp_wire=wire)
        assert sh.ddp.shard and len(sh.ddp.buckets) > 2
        for _ in range(3):
            ref.step()
            sh.step()
        # the shadow all-gathers of the last step are deferred to the next
        # forward's first parameter reads (Param.w joins its bucket only)
        pending = len(sh.ddp._gathers)
        hooked = sh.arena.on_param_use is not None
        sh.ddp.join_gather()
        # the compute copy (bf16 shadow) is complete on every member after
        # the join; the master / optimizer state only after consolidate()
        e_shadow = float((sh.arena.shadow.float() - ref.arena.shadow.float()).norm() /
                         ref.arena.shadow.float().norm())
        assert sh.state_sharded
        try:
            sh.state_tensors()
            raised = False
        except RuntimeError:
            raised = True
        nb = sh.consolidate()
        e_master = float((sh.arena.master - ref.arena.master).norm() / ref.arena.master.norm())
        e_opt = float((sh.opt_state[0] - ref.opt_state[0]).norm() / (ref.opt_state[0].norm() + 1e-12))
        out[model] = dict(e_shadow=e_shadow, e_master=e_master, e_opt=e_opt, raised=raised, nb=nb,
                          pending=pending, hooked=hooked, joined=sh.arena.on_param_use is None,
                          bytes_sh=sh.ddp.wire_bytes, bytes_ref=ref.ddp.wire_bytes,
                          master_sum=float(sh.arena.master.double().sum()))
    q.put((rank, out))
    dist.barrier()


@pytest.mark.parametrize("world,wire", [(2, "fp32"), (4, "fp32"), (4, "bf16"), (8, "fp32"), (8, "bf16")])
def test_sharded_ddp_matches_allreduce(world, wire):
    """Sharded data parallelism (reduce-scatter -> 1/N optimizer -> bf16
    shadow all-gather) on gloo world 2/4/8: the compute copy every member
    trains on matches the all-reduce path after 3 steps, the master /
    optimizer state is refused until consolidate() and then matches too,
    identical on every member; fewer bytes cross the wire."""
    q = mp.get_context("spawn").SimpleQueue()
    _spawn(_shard_worker, world, q, wire)
    res = dict(q.get() for _ in range(world))
    tol = 2e-3 if wire == "fp32" else 1e-2
    for model in ("vgg_tiny", "transformer_tiny"):
        sums = {res[r][model]["master_sum"] for r in range(world)}
        assert len(sums) == 1, sums                         # every member holds the same full state
        for r in range(world):
            o = res[r][model]
            assert o["raised"] and o["nb"] > 0
            assert o["pending"] > 0 and o["hooked"] and o["joined"], (model, r, o)
            assert o["e_shadow"] < tol and o["e_master"] < tol and o["e_opt"] < 5 * tol, (model, r, o)
            # per-member wire bytes: bf16 reduce-scatter + bf16 all-gather is
            # half of the fp32 all-reduce, fp32 reduce-scatter ~3/4 (the
            # replicated norm-parameter buckets and tails stay all-reduced)
            assert o["bytes_sh"] < (0.6 if wire == "bf16" else 0.85) * o["bytes_ref"], o


# ------------------------------------------------- reduce-scatter output aliasing
def _rs_alias_worker(rank, world, port, outdir):
    _init(rank, world, port)
    from tiresias_amd.parallel.gang import GangPG

    pg = GangPG(list(range(world)), rank, "gloo")
    n = 1 << 16                                    # per-member slice
    g = torch.Generator().manual_seed(1234 + rank)
    base = torch.randn(world * n, generator=g)
    # the sharded-DDP call: out is this member's own slice of the bucket
    inplace = base.clone()
    pg.reduce_scatter(inplace[rank * n:(rank + 1) * n], inplace).wait()
    # the same reduction into a separate output buffer
    sep_out = torch.empty(n)
    pg.reduce_scatter(sep_out, base.clone()).wait()
    torch.save({"inplace": inplace[rank * n:(rank + 1) * n].clone(), "sep": sep_out, "base": base},
               os.path.join(outdir, f"rs{rank}.pt"))
    dist.barrier()
    pg.shutdown()
    dist.destroy_process_group()


def test_gloo_reduce_scatter_in_place_equals_separate_output(tmp_path):
    """the gloo reduce-scatter used to pass a view of its
    own (staged) input as the output. At world 4 the in-place call (output =
    the member's slice of the input) must equal a reduce-scatter into a
    separate buffer and the exact fp32 sum of every member's slice."""
    world = 4
    _spawn(_rs_alias_worker, world, str(tmp_path))
    r = [torch.load(tmp_path / f"rs{k}.pt", weights_only=True) for k in range(world)]
    n = r[0]["sep"].numel()
    for k in range(world):
        ref = sum(r[j]["base"][k * n:(k + 1) * n] for j in range(world))
        assert torch.equal(r[k]["inplace"], r[k]["sep"])
        assert torch.allclose(r[k]["sep"], ref, rtol=1e-5, atol=1e-5)
