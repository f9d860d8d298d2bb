"""Real-GPU cluster runtime: the Tiresias scheduler driving DDP training jobs
on one MI355X node, one process per GPU.

Topology (SPMD, ``torch.distributed``):
  * world NCCL (= RCCL over xGMI) group over all N ranks — DDP gangs get
    member-only communicators (``parallel/gang.py``: c10d backends over a
    store prefix, hierarchical "spread" transport across virtual nodes),
    state moves use xGMI P2P (``batch_isend_irecv``);
  * the control plane (``control.py``) carries the round plan and the worker
    reports as TCPStore keys, with per-worker heartbeat threads: a rank whose
    report and heartbeat both stop for ``hb_timeout`` seconds is declared
    lost and the controller re-plans around it (``Controller.rank_lost``);
    the gloo-collective plane is kept for comparison.

Rank 0 additionally runs the CONTROLLER: the same Policy / Placement /
Cluster objects as the simulator (``LiveScheduler`` subclasses the event
engine), fed with *measured* time: a job's attained service is the wall time
it spent running (x #GPUs for 2D-LAS), its progress the iterations its gang
actually completed. Scheduling happens at round boundaries (every
``quantum`` seconds of wall time): gangs stop at an iteration boundary, so a
preemption never interrupts an in-flight collective.

Preemption = suspension in HBM: the job's ``Trainer`` (flat param arena +
optimizer state, 288 GB per GPU leaves plenty of room) stays resident on its
ranks; resuming on the same GPUs is a pointer swap, resuming elsewhere moves
the flat buffers GPU->GPU over xGMI. ``ckpt_policy=pressure`` spills the
suspended jobs the scheduler will resume last, asynchronously, only when a
starting job needs their HBM; ``host`` spills every preempted job.
"""
from __future__ import annotations

import math
import os
import sys
import time
import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import torch
import torch.distributed as dist

from ..config import ClusterSpec, SimConfig
from ..core.job import Job, JobSpec, JobState
from ..engine.sim import Simulator
from ..metrics.logger import MetricsLogger
from ..parallel.gang import GangRegistry, abort_comm, comm_failed, create_gang_comm, vnode_parts
from .trainer import Trainer

# nominal per-iteration seconds on one MI355X (tools/bench_models.py,
# profiles/model_bench_r1_v7.json, hipGraph replay); refined online from the
# workers' measurements. They seed the Gittins prior (service distribution in
# GPU-seconds) and the first round's iteration count of each job.
NOMINAL_ITER_S = {"resnet50": 0.0113, "vgg16": 0.0080, "transformer": 0.0072, "gnmt": 0.0155,
                  "resnet_tiny": 0.004, "vgg_tiny": 0.002, "transformer_tiny": 0.006,
                  "gnmt_tiny": 0.01}


# bound on a fill-mode gang vote (Worker._vote): far above a healthy vote
# (tens of microseconds on RCCL, one gloo round trip on the CPU path)
VOTE_TIMEOUT_S = float(os.environ.get("TAM_VOTE_TIMEOUT_S", "10"))


def _store_del(plane, key: str) -> None:
    """Best-effort delete of a control-store key (bookkeeping only: a failed
    delete leaves a stale key, never a wrong result)."""
    try:
        plane._retry(lambda: plane.store.delete_key(key), "store delete")
    except Exception:
        pass


def gang_ranks(alloc: Dict[str, List[int]], gpn: int) -> Tuple[int, ...]:
    """(virtual) node id + device -> global GPU rank."""
    out = []
    for nid, devs in alloc.items():
        for d in devs:
            out.append((int(nid) - 1) * gpn + d)
    return tuple(sorted(out))


class LiveScheduler(Simulator):
    """The event engine driven by measured progress instead of a model:
    progress only moves when workers report iterations (rate 0)."""

    def __init__(self, cfg, specs, logger=None, prior=None):
        super().__init__(cfg, specs, logger=logger, prior=prior)
        self.actions: List[dict] = []
        # job -> ranks holding its (suspended) state; set by the Controller
        self.holders_of = None
        self.affinity_hits = 0

    def _try_place(self, j: Job) -> bool:
        """Resume AFFINITY: a suspended job whose state is still resident on
        ranks that are all free again goes back to exactly those ranks -- a
        pointer swap instead of a placement that would move its params +
        optimizer state to other GPUs over xGMI (measured in the fake backend
        at N=8: state moves were ~18 % of all allocated GPU time). The ranks
        came from a placement this policy made, so its constraints hold."""
        hold = self.holders_of(j.job_id) if self.holders_of is not None else None
        if hold and len(hold) == j.num_gpu and j.num_gpu <= self.max_gpus:
            gpn = self.cluster.spec.num_gpu_p_node
            plan = []
            ok = True
            for t, r in zip(j.tasks, sorted(hold)):
                nid, d = str(r // gpn + 1), r % gpn
                node = self.cluster.nodes.get(nid)
                if node is None or t.gpu != 1 or d >= len(node.devices) or node.devices[d].tasks \
                        or getattr(node.devices[d], "failed", False):
                    ok = False
                    break
                plan.append((nid, (d,)))
            if ok and len(plan) == len(j.tasks):
                try:
                    self._start(j, plan)
                    self.affinity_hits += 1
                    return True
                except Exception:
                    pass
        return super()._try_place(j)

    def _start(self, j: Job, plan) -> None:
        alloc = self.cluster.commit(j, plan)
        j.start(self.now, alloc, rate=0.0, restore_cost=0.0)
        j.extra["run_start"] = self.now
        self.actions.append({"op": "start", "job": j.job_id})
        self.log.decision(self.now, "start", j.job_id, gpus=j.num_gpu,
                          ranks=list(gang_ranks(alloc, self.cluster.spec.num_gpu_p_node)))

    def _preempt(self, j: Job, reason: str = "priority") -> None:
        j.extra["last_ranks"] = gang_ranks(j.allocation, self.cluster.spec.num_gpu_p_node)
        self.cluster.release(j)
        j.preempt(self.now, 0.0, 0.0)
        self.actions.append({"op": "suspend", "job": j.job_id})
        self.log.decision(self.now, "preempt", j.job_id, reason=reason)

    def _refresh_rates(self) -> None:
        for j in self.active:
            if j.is_running:
                j.rate = 0.0


@dataclass
class ReplayJob:
    spec: JobSpec
    model: str
    iterations: int
    batch: Optional[int] = None
    grad_clip: Optional[float] = None    # global-norm gradient clip of the job (None = off)
    dropout: Optional[float] = None      # training dropout of the job (None = off)
    attn_dropout: Optional[float] = None     # attention-probability dropout of the job (None = off)
    opt_dtype: Optional[str] = None      # optimizer-state format of the job: "fp32" / "bf16" (None = fp32)
    trust_ratio: Optional[float] = None  # layer-wise trust coefficient of the job: LARS / LAMB (None = off)


class Controller:
    def __init__(self, cfg: SimConfig, jobs: List[ReplayJob], world: int, quantum: float,
                 logger: Optional[MetricsLogger] = None, spool=None, prior: Optional[List[float]] = None,
                 clock=None, comms: Optional[GangRegistry] = None):
        self.cfg = cfg
        # seconds clock: host wall clock live, a VirtualClock under the fake backend
        self.clock = clock or time.perf_counter
        self.spool = spool            # executor.spool.Spool: online job submission
        self._status_t = -1e9
        self.log = logger
        self.rjobs = {rj.spec.job_id: rj for rj in jobs}
        specs = []
        for rj in jobs:
            s = rj.spec
            # duration in work units = iterations (progress is reported in iterations)
            specs.append(JobSpec(**{**s.__dict__, "duration": float(rj.iterations)}))
        # the Gittins / expected-remaining prior is HISTORY in GPU-seconds: an
        # explicit sample (e.g. a held-out trace), cfg.gittins_prior, or --
        # with neither -- learned online from the jobs that finish (measured
        # wall seconds x GPUs). Never the replayed jobs' own (future) sizes.
        self.sched = LiveScheduler(cfg, specs, logger=logger, prior=prior)
        # job durations here are iteration counts: the spread advisor needs
        # seconds per iteration (measured, else nominal)
        self.sched.iter_s_of = lambda j: self._iter_est(j.spec.model or "", j.num_gpu)
        self.sched.holders_of = lambda jid: self.holders.get(jid)
        self.world = world
        self.quantum = quantum
        # fill mode (the workers keep stepping their jobs until the next plan,
        # Worker.fill_step): in a round in which a job FINISHES, every other
        # single-job rank gets a share of 0 steps -- it steps by fill only --
        # so the gather, and the next plan that hands the freed GPU new work,
        # come as soon as the finishing job is done instead of after the
        # slowest rank's share (fake backend, headline trace N = 8: the
        # freed ranks' idle was 2.6 % of GPU time). Set by the runtime that
        # knows its workers fill (run_replay / run_fake).
        self.fill_rounds = False
        self.gpn = self.sched.cluster.spec.num_gpu_p_node
        self.vnode_size = self.gpn if getattr(cfg, "virtual_nodes", "") else 0
        self.nic_gbps = float(getattr(cfg, "nic_gbps", 12.5))
        self.holders: Dict[str, Tuple[int, ...]] = {}      # job -> ranks holding its state
        # gang communicator lifecycle (create / LRU-evict / abort); persists
        # across replays when the caller passes the rank-0 worker's registry
        self.comms = comms if comms is not None else GangRegistry()
        self._pending_acts: List[dict] = []     # aborts decided between plans (rank loss, gang errors)
        self.resync: set = set()                # gangs whose replicas may disagree (failed step)
        self.last_old: Dict[str, Tuple[int, ...]] = {}   # job -> holders before its last P2P move
        self.snapshots: Dict[str, Tuple[int, str]] = {}  # job -> (step, path) of its last durable snapshot
        self.from_snap: Dict[str, Tuple[int, str]] = {}  # jobs to restart from their snapshot
        self.snap_restored: set = set()
        # sharded data parallelism (cfg.ddp_shard): gangs whose master /
        # optimizer state is currently sharded across their members (from
        # their start until the consolidate action of their suspension)
        self.ddp_shard = bool(getattr(cfg, "ddp_shard", False))
        self.sharded: set = set()
        self.consolidations = 0
        self.gang_errors = 0
        self.error_log: List[str] = []          # first step errors (summary)
        self.est: Dict[Tuple[str, int], float] = {}
        self.done_iters: Dict[str, int] = {j: 0 for j in self.rjobs}
        self.plan_fill: Dict[str, int] = {}     # fill steps credited for the next plan (echoed to workers)
        self.max_overrun = 0                    # max over jobs of done_iters - iterations
        self.round = 0
        self.t0 = None
        self.spill = getattr(cfg, "ckpt_policy", "none") == "host"
        # failure recovery (rank_lost)
        self.dead: set = set()
        self.rebind: set = set()          # jobs whose surviving replicas need a new gang comm
        self.recovered: set = set()       # resumed from surviving DDP replicas
        self.restarted: set = set()       # lost their only replica: restarted from scratch

    def _iter_est(self, model: str, gpus: int) -> float:
        return getattr(self, "est", {}).get((model, gpus), NOMINAL_ITER_S.get(model, 0.03) *
                                             (1.0 if gpus == 1 else 1.08))

    def start_clock(self):
        self.t0 = self.clock()

    def now(self) -> float:
        return self.clock() - self.t0

    # ---------------------------------------------------------------- reports
    def apply_reports(self, reports: List[dict]) -> None:
        per_job: Dict[str, dict] = {}
        for r in reports:
            for jid, step, path in (r or {}).get("snap") or []:
                if jid in self.rjobs and (jid not in self.snapshots or step >= self.snapshots[jid][0]):
                    self.snapshots[jid] = (int(step), path)
            for jid, c in ((r or {}).get("ckpt") or {}).items():
                j = self.sched.jobs.get(jid)
                if j is not None:
                    j.ckpt_bytes += c["bytes"]
                    j.extra["ckpt_save_s"] = j.extra.get("ckpt_save_s", 0.0) + c["save_s"]
                    j.extra["ckpt_restore_s"] = j.extra.get("ckpt_restore_s", 0.0) + c["restore_s"]
            if r and r.get("dev") and self.log is not None:
                d = r["dev"]
                self.log.device_row(self.now(), r["rank"], d.get("util_pct"), d.get("free_mb"),
                                    d.get("total_mb"), r.get("job"))
            if not r:
                continue
            # one rank's entries per job first: a fill carry (steps finished
            # after the last plan snapshot) adds to the round's own entry
            mine: Dict[str, dict] = {}
            for jr in r.get("jobs") or []:
                m = mine.get(jr["job"])
                if m is None:
                    mine[jr["job"]] = dict(jr)
                else:
                    m["iters"] += jr["iters"]
                    m["run_s"] += jr["run_s"]
                    m["fill"] = m.get("fill") and jr.get("fill")
                    for f in ("error", "move_failed", "snap_failed", "consolidate_failed"):
                        m[f] = m.get(f) or jr.get(f)
            for jr in mine.values():
                # gang members report the same job: a step counts once every
                # member completed it (min), an error from any member marks it
                agg = per_job.get(jr["job"])
                if agg is None:
                    per_job[jr["job"]] = dict(jr)
                else:
                    agg["iters"] = min(agg["iters"], jr["iters"])
                    agg["run_s"] = max(agg["run_s"], jr["run_s"])
                    agg["error"] = agg.get("error") or jr.get("error")
                    agg["move_failed"] = agg.get("move_failed") or jr.get("move_failed")
                    agg["snap_failed"] = agg.get("snap_failed") or jr.get("snap_failed")
                    agg["consolidate_failed"] = agg.get("consolidate_failed") or jr.get("consolidate_failed")
        for jid, jr in per_job.items():
            if jid not in self.rjobs:
                continue
            self.done_iters[jid] += jr["iters"]
            rj = self.rjobs[jid]
            # iterations run beyond the job's count (fill-mode accounting:
            # must stay 0, tests/test_fake_backend.py)
            self.max_overrun = max(self.max_overrun, self.done_iters[jid] - rj.iterations)
            if jr.get("snap_failed"):
                self.snapshot_failed(jid)
                continue
            if jr.get("consolidate_failed"):
                # a member of the suspended sharded gang died before its state
                # was gathered: restart from the last snapshot / scratch
                if jid in self.holders:
                    self.holders.pop(jid)
                    self._lost_all_replicas(jid)
                continue
            if jr.get("move_failed"):
                self.move_failed(jid)
                continue
            if jr.get("error"):
                if self.log is not None:
                    self.log.decision(self.now(), "step-error", jid, error=str(jr["error"])[:200])
                if len(self.error_log) < 20:
                    self.error_log.append(f"{jid}: {str(jr['error'])[:160]}")
                if jid in self.holders and len(self.holders[jid]) > 1:
                    self.gang_failed(jid)
            # co-located rounds measure the pair, not the job: keep the
            # solo estimate (it sizes rounds and seeds the Gittins prior)
            if jr["iters"] > 0 and jr["run_s"] > 0 and not jr.get("shared") and not jr.get("error"):
                k = (rj.model, rj.spec.num_gpu)
                per = jr["run_s"] / jr["iters"]
                self.est[k] = per if k not in self.est else 0.7 * self.est[k] + 0.3 * per
            j = self.sched.jobs[jid]
            j.progress = float(min(self.done_iters[jid], rj.iterations))
            for r in reports:
                for jr in (r or {}).get("jobs") or []:
                    c = jr.get("comm") if jr.get("job") == jid else None
                    if c and (r or {}).get("rank") == min(self.holders.get(jid, (r.get("rank"),))):
                        # one member's view (the gang's lowest rank)
                        j.extra["comm_exposed_s"] = j.extra.get("comm_exposed_s", 0.0) + c["exposed_s"]
                        j.extra["comm_span_s"] = j.extra.get("comm_span_s", 0.0) + c["span_s"]
                        # bytes this member put on the wire per step (the gang's wire format)
                        j.extra["comm_bytes"] = j.extra.get("comm_bytes", 0.0) + c.get("bytes", 0.0)
                        j.extra["comm_steps"] = j.extra.get("comm_steps", 0) + c.get("bytes_steps", 0)
                        # sharded gangs: the deferred shadow all-gather's joins
                        # (compute-stream waits) and the window it overlapped
                        j.extra["gather_exposed_s"] = j.extra.get("gather_exposed_s", 0.0) + \
                            c.get("gather_exposed_s", 0.0)
                        j.extra["gather_window_s"] = j.extra.get("gather_window_s", 0.0) + \
                            c.get("gather_window_s", 0.0)

    def credit_fill(self, counts: Dict[int, Dict[str, int]]) -> Dict[str, int]:
        """Per-rank fill counts -> the steps credited per job (a gang's step
        counts once every member finished it: the min over its holders)."""
        per: Dict[str, int] = {}
        for jid, hold in self.holders.items():
            vals = [int((counts.get(r) or {}).get(jid, 0)) for r in hold]
            if vals and min(vals) > 0:
                per[jid] = min(vals)
        self.apply_fill(per)
        return per

    def apply_fill(self, counts: Dict[str, int]) -> None:
        """Fill-mode progress read at plan time (``Worker.fill``): steps a
        rank took on its job after finishing its round's share, while the
        round's slowest rank was still running. Counted as progress now (a
        job that completes in fill finishes in this plan); steps completed
        after this snapshot arrive as carry in the next reports."""
        for jid, n in counts.items():
            if jid not in self.rjobs or n <= 0:
                continue
            self.done_iters[jid] += int(n)
            self.max_overrun = max(self.max_overrun, self.done_iters[jid] - self.rjobs[jid].iterations)
            j = self.sched.jobs[jid]
            j.progress = float(min(self.done_iters[jid], self.rjobs[jid].iterations))

    # ---------------------------------------------------------------- failures
    def rank_lost(self, r: int) -> None:
        """Rank ``r`` (its GPU / process) is gone: take the GPU out of the
        cluster, preempt every job running there, and keep each DDP gang's
        surviving replicas (params + optimizer state are replicated, all at
        the last completed iteration) as its state holders — the next start
        moves / rebinds them like any preemption. A job whose only replica
        lived on ``r`` restarts from scratch."""
        s = self.sched
        if r in self.dead:
            return
        self.dead.add(r)
        for j in list(s.active):
            if j.is_running and r in gang_ranks(j.allocation, self.gpn):
                s._preempt(j, reason="rank-lost")
        s.cluster.fail_device(str(r // self.gpn + 1), r % self.gpn)
        s.max_gpus = s.cluster.num_gpus
        # every communicator that contains the dead rank is aborted on the
        # survivors (the control plane's watcher already did so asynchronously
        # to unblock them; the plan action purges the entries in lock-step)
        self._queue_aborts(self.comms.abort_rank(r))
        for j in list(s.active):
            if j.num_gpu > s.max_gpus:           # can never be placed again
                if j.is_running:
                    s._preempt(j, reason="rank-lost")
                j.state = JobState.FAILED
                s.active.remove(j)
                s.finished.append(j)
                if self.log is not None:
                    self.log.decision(self.now(), "failed", j.job_id, reason="gang larger than live GPUs")
        for jid, hold in list(self.holders.items()):
            if r not in hold:
                continue
            left = tuple(x for x in hold if x != r)
            if left and jid in self.sharded:
                # sharded state: the dead member's slices are gone with it
                self.sharded.discard(jid)
                self.holders.pop(jid)
                self._lost_all_replicas(jid)
                continue
            if left:
                self.holders[jid] = left
                self.rebind.add(jid)
                self.recovered.add(jid)
            else:
                self.holders.pop(jid)
                self._lost_all_replicas(jid)
        if self.log is not None:
            self.log.decision(self.now(), "rank-lost", str(r), gpus_left=s.cluster.num_gpus)

    def _lost_all_replicas(self, jid: str) -> None:
        """No live rank holds the job's state: restart it from its last
        durable snapshot (ckpt/snapshot.py) when there is one, else from
        scratch; the redone iterations are charged (job.csv lost_iters)."""
        j = self.sched.jobs[jid]
        snap = self.snapshots.get(jid)
        keep = snap[0] if snap is not None else 0
        lost = max(0, self.done_iters[jid] - keep)
        j.extra["lost_iters"] = j.extra.get("lost_iters", 0) + lost
        self.done_iters[jid] = keep
        j.progress = float(keep)
        if snap is not None and keep > 0:
            self.from_snap[jid] = snap
            self.snap_restored.add(jid)
        else:
            self.restarted.add(jid)
        if self.log is not None:
            self.log.decision(self.now(), "restart", jid, from_step=keep, lost_iters=lost,
                              source="snapshot" if keep > 0 else "scratch")

    def _queue_aborts(self, acts: List[dict]) -> None:
        """Abort actions go out with the next plan; held jobs whose gang
        communicator they destroy get a rebind on resume."""
        for a in acts:
            self._pending_acts.append(a)
            for jid, hold in self.holders.items():
                if tuple(hold) == tuple(a["ranks"]):
                    self.rebind.add(jid)

    def gang_failed(self, jid: str) -> None:
        """A gang step failed (collective timeout, an aborted communicator, a
        peer error): the step's gradients -- and possibly one member's
        optimizer update -- are unreliable and the communicator is dead.
        Preempt the job, abort its communicator (and any sharing one), and
        resume it from ONE replica: on restart every other member receives
        the lowest holder's state (``resync``), so the replicas agree again.
        Without this a broken gang kept stepping on the dead communicator and
        its members desynchronised (the wedge behind round 2's straggler
        test)."""
        s = self.sched
        j = s.jobs.get(jid)
        hold = self.holders.get(jid)
        self.gang_errors += 1
        if j is not None and j.is_running:
            s._preempt(j, reason="gang-error")
        if hold is not None and len(hold) > 1:
            self._queue_aborts(self.comms.abort_gang(hold))
            if jid in self.sharded:
                # no member holds the whole (consistent) state to resync from
                self.sharded.discard(jid)
                self.holders.pop(jid, None)
                self._lost_all_replicas(jid)
            else:
                self.resync.add(jid)
        if self.log is not None:
            self.log.decision(self.now(), "gang-error", jid, ranks=list(hold or ()))

    def snapshot_failed(self, jid: str) -> None:
        """A restart from the job's durable snapshot failed on some member (the
        file is missing, truncated or unreadable there; the members agreed
        and none ran it): restart the job from scratch instead, charging the
        iterations the snapshot held (job.csv lost_iters)."""
        s = self.sched
        j = s.jobs.get(jid)
        if j is None:
            return
        if j.is_running:
            s._preempt(j, reason="snapshot-failed")
        self.snapshots.pop(jid, None)
        self.from_snap.pop(jid, None)
        self.snap_restored.discard(jid)
        self.holders.pop(jid, None)
        self.last_old.pop(jid, None)
        lost = self.done_iters.get(jid, 0)
        j.extra["lost_iters"] = j.extra.get("lost_iters", 0) + lost
        j.extra["snapshot_failures"] = j.extra.get("snapshot_failures", 0) + 1
        self.done_iters[jid] = 0
        j.progress = 0.0
        self.restarted.add(jid)
        if self.log is not None:
            self.log.decision(self.now(), "restart", jid, from_step=0, lost_iters=lost,
                              source="scratch", reason="snapshot unreadable")

    def move_failed(self, jid: str) -> None:
        """A state move did not complete on every participant (a peer died
        mid-transfer): the valid replicas are on the live OLD holders. Preempt
        the job there; with no live old holder it restarts from scratch."""
        s = self.sched
        j = s.jobs.get(jid)
        if j is not None and j.is_running:
            s._preempt(j, reason="move-failed")
        old = tuple(r for r in self.last_old.get(jid, ()) if r not in self.dead)
        if old:
            self.holders[jid] = old
            self.rebind.add(jid)
        else:
            self.holders.pop(jid, None)
            self._lost_all_replicas(jid)
        if self.log is not None:
            self.log.decision(self.now(), "move-failed", jid, holders=list(old))

    # ---------------------------------------------------------------- submission
    def _poll_spool(self) -> None:
        now = self.now()
        for req in self.spool.poll():
            try:
                jid, model, g, iters, batch, clip, drop, adrop, odt, eta = self._validate(req)
                why = ""
            except (ValueError, TypeError, OverflowError) as e:
                jid = str(req.get("job_id") or "")
                why = str(e)
            if why:
                self.spool.resolve(req, False, why)
                if self.log is not None:
                    self.log.decision(now, "reject", jid or "?", reason=why)
                continue
            spec = JobSpec(job_id=jid, submit_time=now, duration=iters * self._iter_est(model, g),
                           num_gpu=g, model=model, iterations=iters, opt_dtype=odt)
            self.rjobs[jid] = ReplayJob(spec=spec, model=model, iterations=iters, batch=batch, grad_clip=clip,
                                        dropout=drop, attn_dropout=adrop, opt_dtype=odt, trust_ratio=eta)
            self.done_iters[jid] = 0
            self.sched.submit(JobSpec(**{**spec.__dict__, "duration": float(iters)}))
            self.spool.resolve(req, True)
            if self.log is not None:
                self.log.decision(now, "submit", jid, gpus=g, model=model, iterations=iters)

    def _validate(self, req: dict):
        """Untrusted spool request -> (job_id, model, num_gpu, iterations,
        batch, grad_clip, dropout, attn_dropout, opt_dtype, trust_ratio); raises
        ValueError with the rejection reason."""
        from ..models import MODELS

        jid = req.get("job_id")
        if not isinstance(jid, (str, int)) or isinstance(jid, bool) or str(jid) == "":
            raise ValueError(f"job_id must be a non-empty string, got {jid!r}")
        jid = str(jid)
        if jid in self.rjobs:
            raise ValueError(f"duplicate job id {jid!r}")
        model = req.get("model")
        if not isinstance(model, str) or model not in MODELS:
            raise ValueError(f"unknown model {model!r} (known: {sorted(MODELS)})")

        def pos_int(name, v):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v or int(v) != v or v <= 0:
                raise ValueError(f"{name} must be a positive integer, got {v!r}")
            return int(v)

        g = pos_int("num_gpu", req.get("num_gpu", 1) if req.get("num_gpu") is not None else 1)
        if g > self.world:
            raise ValueError(f"num_gpu {g} outside 1..{self.world}")
        batch = req.get("batch")
        if batch is not None:
            batch = pos_int("batch", batch)
            if batch > 4096:
                raise ValueError(f"batch {batch} too large (max 4096)")
        iters = req.get("iterations")
        if iters is None:
            dur = req.get("duration")
            if isinstance(dur, bool) or not isinstance(dur, (int, float)) or not dur > 0 or dur == float("inf"):
                raise ValueError("iterations/duration must be positive")
            iters = max(1, int(round(float(dur) / self._iter_est(model, g))))
        iters = pos_int("iterations", iters)
        clip = req.get("grad_clip")
        if clip is not None:
            if isinstance(clip, bool) or not isinstance(clip, (int, float)) or not clip > 0 or clip == float("inf"):
                raise ValueError(f"grad_clip must be a finite number > 0, got {clip!r}")
            clip = float(clip)
            if self.ddp_shard and g > 1:
                raise ValueError("grad_clip is not supported for a multi-GPU job under ddp_shard")
        drop = req.get("dropout")
        if drop is not None:
            if (isinstance(drop, bool) or not isinstance(drop, (int, float)) or not 0 <= drop < 1
                    or round(drop * 65536) >= 65536):
                raise ValueError(f"dropout must be a number p with 0 <= p < 1 (quantised to 1/65536), got {drop!r}")
            drop = float(drop)
        adrop = req.get("attn_dropout")
        if adrop is not None:
            if (isinstance(adrop, bool) or not isinstance(adrop, (int, float)) or not 0 <= adrop < 1
                    or round(adrop * 256) >= 256):
                raise ValueError(f"attn_dropout must be a number p with 0 <= p < 1 (quantised to 1/256), got {adrop!r}")
            adrop = float(adrop)
        odt = req.get("opt_dtype")
        if odt is not None and (not isinstance(odt, str) or odt not in ("fp32", "bf16")):
            raise ValueError(f"opt_dtype must be 'fp32' or 'bf16', got {odt!r}")
        eta = req.get("trust_ratio")
        if eta is not None:
            if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not eta > 0 or eta == float("inf"):
                raise ValueError(f"trust_ratio must be a finite number > 0, got {eta!r}")
            eta = float(eta)
            if self.ddp_shard and g > 1:
                raise ValueError("trust_ratio is not supported for a multi-GPU job under ddp_shard")
            if odt == "bf16":
                raise ValueError("trust_ratio is not supported with opt_dtype 'bf16'")
        return jid, model, g, iters, batch, clip, drop, adrop, odt, eta

    def status(self) -> dict:
        s = self.sched
        jobs = {}
        for jid, j in s.jobs.items():
            if j.state.name == "SUBMITTED":
                continue
            jobs[jid] = {"state": j.state.name, "model": self.rjobs[jid].model, "num_gpu": j.num_gpu,
                         "iterations_done": self.done_iters.get(jid, 0),
                         "iterations": self.rjobs[jid].iterations, "queue": j.queue,
                         "preempted": j.preempt_count,
                         "jct_s": round(j.jct, 4) if j.jct is not None else None}
        return {"time_s": round(self.now(), 3), "round": self.round, "jobs": jobs,
                "running": sum(1 for j in s.active if j.is_running),
                "pending": sum(1 for j in s.active if j.is_pending),
                "finished": len(s.finished)}

    # ---------------------------------------------------------------- planning
    def plan_round(self) -> dict:
        s = self.sched
        s.actions = []
        if self.spool is not None:
            self._poll_spool()
        t = max(self.now(), s.now)
        if s.events == 0 or t > s.now:
            s.step(t)
        else:
            s.step(s.now)
        finished = [j for j in s.finished if j.extra.get("reported") is None]
        actions: List[dict] = self._pending_acts
        self._pending_acts = []
        for j in finished:
            j.extra["reported"] = True
            if j.job_id in self.holders:
                actions.append({"op": "drop", "job": j.job_id, "ranks": self.holders.pop(j.job_id)})
        for a in s.actions:
            j = s.jobs[a["job"]]
            if a["op"] == "suspend" and j.job_id in self.sharded and j.job_id in self.holders \
                    and any(r in self.dead for r in self.holders[j.job_id]):
                self.sharded.discard(j.job_id)
                self.holders.pop(j.job_id)
                self._lost_all_replicas(j.job_id)
            if a["op"] == "suspend" and j.job_id in self.sharded and j.job_id in self.holders:
                # a suspended sharded gang gathers its full state on every
                # member first: moves, spills and snapshots read whole buffers
                actions.insert(0, {"op": "consolidate", "job": j.job_id, "ranks": self.holders[j.job_id]})
                self.sharded.discard(j.job_id)
                self.consolidations += 1
            if a["op"] == "suspend" and self.spill and j.is_pending and j.job_id in self.holders:
                actions.append({"op": "spill", "job": j.job_id, "ranks": self.holders[j.job_id]})
            if a["op"] == "start" and j.is_running:
                ranks = gang_ranks(j.allocation, self.gpn)
                if len(ranks) > 1:
                    # a gang crossing a virtual-node boundary gets the
                    # hierarchical transport (parallel/gang.py)
                    actions.extend(self.comms.ensure(ranks, self.vnode_size, self.nic_gbps))
                old = self.holders.get(j.job_id)
                rj = self.rjobs[j.job_id]
                act = {"op": "start", "job": j.job_id, "ranks": ranks, "model": rj.model,
                       "iters": max(0, rj.iterations - self.done_iters[j.job_id]),
                       "batch": rj.batch, "grad_clip": rj.grad_clip, "dropout": rj.dropout,
                       "attn_dropout": rj.attn_dropout, "opt_dtype": rj.opt_dtype, "trust_ratio": rj.trust_ratio,
                       "seed": int(j.job_id) if j.job_id.isdigit() else zlib.crc32(j.job_id.encode()) % 100000}
                if old is None and j.job_id in self.from_snap:
                    step, path = self.from_snap.pop(j.job_id)
                    act["source"] = "snapshot"
                    act["path"] = path
                    act["step"] = step
                elif old is None:
                    act["source"] = "fresh"
                elif j.job_id in self.resync and len(old) > 1:
                    # after a failed gang step: every new member except ONE
                    # holder (the lowest) receives that holder's state
                    self.resync.discard(j.job_id)
                    self.rebind.discard(j.job_id)
                    src = old[0]
                    act["source"] = "p2p"
                    act["donors"] = {r: src for r in ranks if r != src}
                    act["old"] = old
                    act["resync"] = True
                    act["step"] = self.done_iters[j.job_id]
                elif old == ranks and j.job_id not in self.rebind:
                    act["source"] = "resident"
                elif old == ranks:
                    # surviving replicas of a gang that lost a member: same
                    # ranks, new communicator (the p2p path rebinds, no donors)
                    act["source"] = "p2p"
                    act["donors"] = {}
                    act["old"] = old
                    act["step"] = self.done_iters[j.job_id]
                    self.rebind.discard(j.job_id)
                else:
                    self.rebind.discard(j.job_id)
                    # every new rank without a replica receives one from a holder
                    donors = {}
                    for i, r in enumerate(ranks):
                        if r not in old:
                            donors[r] = old[i % len(old)]
                    act["source"] = "p2p"
                    act["donors"] = donors
                    act["old"] = old
                    # receivers start with the donors' optimizer step count
                    # (Adam's bias correction), progress = completed steps
                    act["step"] = self.done_iters[j.job_id]
                if act["source"] == "p2p":
                    self.last_old[j.job_id] = tuple(old)
                self.holders[j.job_id] = ranks
                if self.ddp_shard and len(ranks) > 1 and len(vnode_parts(ranks, self.vnode_size)) <= 1:
                    self.sharded.add(j.job_id)     # steps shard the state from now on
                actions.append(act)
        # bounded communicator cache: LRU sets nobody holds state on go away
        actions.extend(self.comms.evict(set(self.holders.values())))
        # assignments: running jobs -> iterations this round; with GPU sharing
        # (pack placement) a rank can carry several jobs, run concurrently
        assign: Dict[int, List[Tuple[str, int]]] = {}
        nxt, now = s.reader.next_time(), self.now()
        for j in s.active:
            if not j.is_running:
                continue
            rj = self.rjobs[j.job_id]
            left = rj.iterations - self.done_iters[j.job_id]
            if left <= 0:
                continue
            est = self._iter_est(rj.model, j.num_gpu)
            n = max(1, int(round(self.quantum / est)))
            if j.num_gpu > 1 and math.isfinite(nxt):
                # gangs cannot cut a round at the arrival on their own (every
                # member must run the same step count), so size their share
                # to end there: the 1-GPU ranks then do not idle waiting
                n = min(n, max(1, int(math.ceil((nxt - now) / est))))
            n = min(n, left)
            for r in gang_ranks(j.allocation, self.gpn):
                assign.setdefault(r, []).append((j.job_id, n))
        if self.fill_rounds:
            fin = {jid for lst in assign.values() for jid, n in lst
                   if self.rjobs[jid].iterations - self.done_iters[jid] - n <= 0}
            if fin:
                for r, lst in assign.items():
                    if len(lst) == 1 and lst[0][0] not in fin:
                        assign[r] = [(lst[0][0], 0)]
        # iterations each assigned job has left after this round's share
        # (bounds fill-mode steps, Worker.fill)
        left = {jid: self.rjobs[jid].iterations - self.done_iters[jid] - n
                for r in assign for jid, n in assign[r]}
        for r in assign:                      # same order on every rank (gang collectives)
            if len(assign[r]) > 1:
                # co-located 1-GPU jobs each progress at 1/s of solo speed:
                # shrink their shares so the rank still ends near the quantum
                # (other ranks would otherwise idle at the round barrier)
                ms = {jid: self.rjobs[jid].model for jid, _ in assign[r]}
                shr = []
                for jid, n in assign[r]:
                    s_ = max(s.interf.pair(ms[jid], ms[o]) for o in ms if o != jid)
                    rem = self.rjobs[jid].iterations - self.done_iters[jid]
                    est = self._iter_est(ms[jid], 1)
                    shr.append((jid, max(1, min(rem, int(round(self.quantum / (est * s_)))))))
                assign[r] = shr
            assign[r].sort()
        self.round += 1
        stop = not s.active and s.reader.remaining() == 0
        if self.spool is not None:
            stop = stop and self.spool.shutdown_requested()
            if self.clock() - self._status_t > 0.5 or stop:
                self._status_t = self.clock()
                self.spool.publish(self.status())
        wait = 0.0
        if not assign and not stop:
            # idle cluster: sleep until the next arrival instead of spinning
            wait = max(0.0, min(self.quantum, s.reader.next_time() - self.now()))
        # next trace arrival as an absolute host-clock time: 1-GPU jobs end the
        # round at the first step boundary after it (Worker._run_until)
        deadline = self.t0 + nxt if math.isfinite(nxt) else None
        seen, self.plan_fill = self.plan_fill, {}
        # jobs of this round whose model runs persistent-grid recurrences (GNMT):
        # the one-GPU rehearsal's workers keep two of them off the grids at once
        persist_jobs = sorted({jid for lst in assign.values() for jid, _ in lst
                               if "gnmt" in (self.rjobs[jid].model or "")})
        plan = {"round": self.round, "actions": actions, "assign": assign, "left": left, "fill_seen": seen,
                "persist_jobs": persist_jobs,
                "stop": stop, "wait": wait,
                "deadline": deadline, "alive": [r for r in range(self.world) if r not in self.dead],
                "ckpt": getattr(self.cfg, "ckpt_policy", "none")}
        if plan["ckpt"] == "pressure":
            # suspended jobs holding state, in the policy's priority order: a
            # worker under HBM pressure spills from the END (the job the
            # scheduler will resume last), not merely the least recently run
            held = [j for j in s.active if j.is_pending and j.job_id in self.holders]
            if held:
                rank_of = {j.job_id: i for i, j in enumerate(s.policy.order(list(s.active), s.now))}
                plan["resume_order"] = sorted((j.job_id for j in held), key=lambda x: rank_of.get(x, 1 << 30))
        return plan


class Worker:
    def __init__(self, rank: int, world: int, device: torch.device, world_pg=None, use_graph=False,
                 gang_backend: Optional[str] = None, monitor_period: float = 5.0, pool_cap: int = 2,
                 hbm_budget_gb: Optional[float] = None, snapshot_s: float = 0.0, snapshot_dir: str = "",
                 ddp_shard: bool = False, ddp_wire: str = "fp32"):
        self.gang_backend = gang_backend or ("nccl" if device.type == "cuda" else "gloo")
        self.ddp_shard, self.ddp_wire = ddp_shard, ddp_wire
        self.consolidated_bytes = 0
        # warm pool: finished jobs' trainers, keyed by (model, batch, gang
        # ranks), handed to the next fresh job of the same shape after
        # Trainer.reset (new weights / batch / optimizer state in the same
        # buffers: no allocation, warm-up or graph capture on job start)
        self.pool: Dict[tuple, List[Trainer]] = {}
        self.pool_cap = pool_cap
        self.pool_hits = 0
        self.rank = rank
        self.world = world
        self.device = device
        self.world_pg = world_pg
        self.trainers: Dict[str, Trainer] = {}
        self.streams: Dict[str, object] = {}     # per-job HIP streams for co-located jobs
        # gang comms by rank set (built on the process-wide PGCache); their
        # lifecycle follows the plan's group / ungroup / abort actions, which
        # rank 0's controller decides with ``comm_registry`` (kept here so it
        # persists across replays exactly like this cache)
        self.groups: Dict[Tuple[int, ...], object] = {}
        self.comm_registry = GangRegistry()
        self._pairs: Dict[Tuple[int, int], object] = {}    # state-move communicators
        self._move_failed: set = set()
        self.plane = None                        # control plane (set by run_replay): move agreement
        self.graph_min_iters = int(os.environ.get("TAM_GRAPH_MIN_ITERS", "40"))
        # periodic durable snapshots (ckpt/snapshot.py): every snapshot_s
        # seconds of a job's run time, written by the gang's lowest rank
        self.snapshot_s = snapshot_s
        self.snap = None
        if snapshot_s > 0:
            from ..ckpt.snapshot import SnapshotWriter

            # a snapshot must outlive its writer AND be readable by whichever
            # ranks restart the job: only a directory shared by every rank
            # (never a per-process /tmp default) serves both
            if not snapshot_dir:
                raise ValueError("snapshot_s > 0 needs a snapshot_dir shared by every rank")
            self.snap = SnapshotWriter(snapshot_dir, device)
        # fill mode (fill_step): the job this rank keeps stepping after its
        # round's share while slower ranks finish, steps taken, and the
        # steps the controller's snapshot did not see (reported next round)
        self._fill: Optional[dict] = None
        self._carry: List[dict] = []
        self._fill_cap: Dict[str, int] = {}   # fill bound after a carry-capped share (run())
        self.fill_enabled = os.environ.get("TAM_FILL", "1") != "0"
        # every rank on ONE physical GPU (the one-GPU multi-rank rehearsal):
        # state moves go device to device through HIP IPC (_do_moves_ipc)
        self.shared_device = (device.type == "cuda" and self.gang_backend == "gloo"
                              and os.environ.get("TAM_SHARED_GPU") == "1"
                              and os.environ.get("TAM_IPC_MOVES", "1") != "0")
        self.fill_s_total = 0.0
        self.fill_steps_total = 0
        # host seconds of plan application per action kind (start_fresh_build /
        # _pool, start_p2p / _resident / _snapshot, p2p_transfer, move_agree,
        # group, consolidate, drop, spill, pressure_room, reclaim, prefetch)
        # and the hipGraph captures of fresh trainers' first steps
        self.apply_prof: Dict[str, float] = {}
        self.apply_count: Dict[str, int] = {}
        self._snap_failed: set = set()          # jobs whose snapshot load failed (this round)
        self.snap_reported: set = set()         # jobs with a durable snapshot the controller was told of
        self._consolidate_failed: set = set()   # sharded gangs whose consolidation failed
        self._job_ranks: Dict[str, Tuple[int, ...]] = {}
        self._snap_acc: Dict[str, float] = {}
        self.use_graph = use_graph
        self.spilled_bytes = 0
        self.restored_bytes = 0
        self._engine = None
        # HBM-pressure preemption state (ckpt policy "pressure"): suspended
        # jobs stay resident until a job that is about to start on this rank
        # needs their HBM; then the least recently run ones spill
        self.hbm_budget = hbm_budget_gb * 2 ** 30 if hbm_budget_gb else None
        self._last_run: Dict[str, int] = {}
        self._round = 0
        self._need: Dict[object, float] = {}       # model (or (model, "bf16")) -> measured HBM need of a new job
        self._ckpt: Dict[str, dict] = {}           # job -> bytes / seconds since the last report
        self.pressure_spills = 0
        self.pool_evictions = 0
        self.prefetches = 0
        # real-device sampling (HIP mem info + amd-smi) for gpu_live.csv
        self.monitor = None
        self._mon_t = -1e9
        if device.type == "cuda" and monitor_period > 0:
            from ..cluster.device import DeviceMonitor

            self.monitor = DeviceMonitor(period=monitor_period, device_index=device.index).start()

    def _ckpt_engine(self):
        if self._engine is None:
            if self.device.type == "cuda":
                self._engine = torch.classes.tam.CkptEngine(self.device.index, 1 << 30)
            else:
                self._engine = _HostEngine()
        return self._engine

    def _group(self, ranks):
        if len(ranks) <= 1:
            return None
        return self.groups[tuple(ranks)]

    @staticmethod
    def _pool_key(act) -> tuple:
        """Warm-pool key of a start action: what fixes a trainer's buffers.
        The optimizer-state format does (bf16 state buffers cannot serve a
        fp32-state job, nor the reverse), so a bf16-state job's key carries it;
        the per-job setters (clip, dropouts, trust ratio) are not part of the key."""
        key = (act["model"], act.get("batch"), tuple(act["ranks"]))
        return key + ("bf16",) if act.get("opt_dtype") == "bf16" else key

    def _make_trainer(self, act, init: bool = True) -> Trainer:
        ranks = tuple(act["ranks"])
        data_seed = act["seed"] * 1000 + ranks.index(self.rank)
        key = self._pool_key(act)
        # hipGraph capture (+ instantiation, + a private memory pool per
        # graph) costs tens of ms per fresh trainer. It pays when the
        # trainer outlives the job in the warm pool (later jobs of the shape
        # replay for free) or when the job alone is long enough; otherwise
        # run eagerly (measured on MI355X, bench without the warm pool:
        # every job capturing -> avg JCT 2.38 s, eager 0.25 s)
        long_job = int(act.get("iters", 1 << 30)) >= self.graph_min_iters
        want = self.use_graph and len(ranks) == 1 and (long_job or self.pool_cap > 0)
        free = self.pool.get(key)
        if free:
            # the key carries the state format; a pooled trainer of the other
            # format under it would run the wrong kernels silently
            want_dt = "bf16" if act.get("opt_dtype") == "bf16" else "fp32"
            if free[-1].opt_dtype != want_dt:
                raise RuntimeError(f"warm pool {key}: a {free[-1].opt_dtype}-state trainer is pooled under the "
                                   f"key of a {want_dt}-state job")
            self.pool_hits += 1
            t = free.pop().reset(act["seed"], data_seed, init=init)
            t.set_grad_clip(act.get("grad_clip"))    # per job, not part of the pool key
            t.set_dropout(act.get("dropout"))        # likewise (a change re-captures the graph)
            t.set_attn_dropout(act.get("attn_dropout"))
            t.set_trust_ratio(act.get("trust_ratio"))    # per job too: its buffers are a few KiB
            self._bind(t, ranks)
            if want and not t.use_graph and t.ddp is None:
                t.enable_graph()
            return t
        t = Trainer(act["model"], self.device, batch=act.get("batch"), group=self._group(ranks),
                    seed=act["seed"], data_seed=data_seed, use_graph=want, ddp_shard=self.ddp_shard,
                    ddp_wire=self.ddp_wire, grad_clip=act.get("grad_clip"), dropout=act.get("dropout"),
                    attn_dropout=act.get("attn_dropout"), opt_dtype=act.get("opt_dtype"),
                    trust_ratio=act.get("trust_ratio"))
        t.pool_key = key
        return t

    def _bind(self, t: Trainer, ranks) -> None:
        """A gang trainer must step on the CURRENT communicator of its rank
        set (it may have been evicted / aborted and re-created since the
        trainer last ran): rebind when it is a different object."""
        if len(ranks) > 1 and t.group is not self.groups.get(tuple(ranks)):
            t.rebind(self._group(ranks))

    def _drop_pool(self, ranks) -> None:
        for key in [k for k in self.pool if tuple(k[2]) == tuple(ranks)]:
            for t in self.pool.pop(key):
                t.release()

    # ------------------------------------------------------------ communicators
    def _open_group(self, ranks, vnode: int, nic_gbps: float, pin: bool = False):
        ranks = tuple(ranks)
        old = self.groups.pop(ranks, None)
        if old is not None:
            old.close()
        c = create_gang_comm(ranks, self.rank, vnode_size=vnode, backend=self.gang_backend,
                             device=self.device, nic_gbps=nic_gbps, pin=pin)
        if c is not None:
            c.vnode = vnode
            self.groups[ranks] = c
        return c

    def _close_group(self, ranks, abort: bool = False, dead: Optional[int] = None, purge=None) -> None:
        from ..parallel.gang import PG_CACHE

        ranks = tuple(ranks)
        c = self.groups.pop(ranks, None)
        if c is not None:
            if abort:
                abort_comm(c)
            c.close(purge=abort)
        if dead is not None:
            PG_CACHE.purge([k for k in PG_CACHE.live() if dead in k[0]])
        if purge:
            sets = {tuple(x) for x in purge}
            PG_CACHE.purge([k for k in PG_CACHE.live() if tuple(k[0]) in sets])
        self._drop_pool(ranks)

    def precreate_groups(self, sets, vnode: int = 0, nic_gbps: float = 12.5) -> int:
        """Create (and warm: the first collective builds the RCCL
        communicator) the canonical gang communicators, pinned, on every rank
        in the same order -- call it collectively outside any timed region.
        Marks them live in the controller-side registry. Returns how many
        this rank is a member of."""
        n = 0
        for r in sets:
            r = tuple(r)
            c = self._open_group(r, vnode, nic_gbps, pin=True)
            if c is not None:
                n += 1
                from ..parallel.gang import _pgs_of

                for pg in _pgs_of(c):
                    pg.warm(self.device if pg.backend == "nccl" else torch.device("cpu"))
        self.comm_registry.pin(sets, vnode)
        return n

    def prewarm(self, models) -> float:
        """Pay the per-PROCESS first-launch costs before any job runs: one
        eager step of each model family loads its kernels' code objects and
        library handles and decides GEMM routes not in the shipped table
        (measured: the first ResNet-50 step of a fresh process takes ~0.8 s
        vs 11 ms warm, profiles/r3/startup_*.jsonl). A long-lived cluster
        daemon does this once at start. Returns seconds spent."""
        t0 = time.perf_counter()
        if self.device.type != "cuda":
            return 0.0
        for m in models:
            t = Trainer(m, self.device, seed=0, use_graph=False)
            t.step()
            torch.cuda.synchronize(self.device)
            t.release()
            del t
        torch.cuda.empty_cache()
        return time.perf_counter() - t0

    def _retire(self, t: Optional[Trainer]) -> None:
        """A job left this rank: keep its trainer warm for the next job of the
        same shape (bounded per key), else free it."""
        if t is None:
            return
        key = getattr(t, "pool_key", None)
        if key is None or getattr(t, "_spilled", None) or self.pool_cap <= 0:
            t.release()
            return
        lst = self.pool.setdefault(key, [])
        if len(lst) < self.pool_cap:
            lst.append(t)
        else:
            t.release()

    def drain_pool(self) -> None:
        for lst in self.pool.values():
            for t in lst:
                t.release()
        self.pool.clear()

    # ------------------------------------------------------------ HBM pressure
    def _resident_bytes(self) -> float:
        n = 0.0
        for t in list(self.trainers.values()) + [t for lst in self.pool.values() for t in lst]:
            if not getattr(t, "_spilled", None):
                n += t.hbm_bytes()
        return n

    def _job_need(self, model: str, batch, opt_dtype: Optional[str] = None) -> float:
        """HBM a new job of ``model`` needs, in the units the budget counts
        (Trainer.hbm_bytes: state + batch): the measured growth when one was
        last created here with the same optimizer-state format, else 1.5x its
        optimizer-inclusive state (bf16 moments priced at 2 B each)."""
        nk = (model, "bf16") if opt_dtype == "bf16" else model
        if nk in self._need:
            return self._need[nk]
        from ..profiler.skew import model_profile

        try:
            st = model_profile(model).state_bytes("adam", opt_dtype)
        except KeyError:
            st = 1 << 30
        return 1.5 * st

    def _free_bytes(self) -> float:
        if self.device.type == "cuda" and self.hbm_budget is None:
            free, _ = torch.cuda.mem_get_info(self.device)
            return free + (torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device))
        budget = self.hbm_budget if self.hbm_budget is not None else float("inf")
        return budget - self._resident_bytes()

    def _make_room(self, need: float, protect: set, resume_order=None) -> None:
        """Spill least-recently-run suspended jobs of this rank (never one
        that runs or starts this round) until ``need`` bytes fit, plus a 5 %
        margin. Spills are asynchronous (Trainer.offload never waits)."""
        margin = 0.05 * (self.hbm_budget or 0.0)
        if self._free_bytes() >= need + margin:
            return
        # idle warm-pool trainers are a cache: they go first, and cost nothing
        for key in list(self.pool):
            lst = self.pool[key]
            while lst and self._free_bytes() < need + margin:
                lst.pop().release()
                self.pool_evictions += 1
            if not lst:
                del self.pool[key]
        # victims: lowest scheduler priority first (plan's resume order), then
        # least recently run
        order = {jid: i for i, jid in enumerate(resume_order or [])}
        # a sharded gang member holds only its slices of the job's state until
        # the plan's 'consolidate' action has run: never a pressure victim
        victims = sorted((jid for jid, t in self.trainers.items()
                          if jid not in protect and not getattr(t, "_spilled", None)
                          and not t.state_sharded),
                         key=lambda j: (-order.get(j, -1), self._last_run.get(j, -1)))
        for jid in victims:
            if self._free_bytes() >= need + margin:
                break
            self._spill(jid)

    def _spill(self, jid: str) -> None:
        t = self.trainers[jid]
        nb = t.offload(self._ckpt_engine())
        self.spilled_bytes += nb
        self.pressure_spills += 1
        c = self._ckpt.setdefault(jid, {"bytes": 0.0, "save_s": 0.0, "restore_s": 0.0})
        c["bytes"] += nb

    def _restore(self, jid: str) -> None:
        nb = self.trainers[jid].restore()
        self.restored_bytes += nb
        c = self._ckpt.setdefault(jid, {"bytes": 0.0, "save_s": 0.0, "restore_s": 0.0})
        c["bytes"] += nb

    def _ap(self, key: str, t0: float) -> float:
        """Charge the host seconds since ``t0`` to apply-breakdown ``key``."""
        t = time.perf_counter()
        self.apply_prof[key] = self.apply_prof.get(key, 0.0) + (t - t0)
        self.apply_count[key] = self.apply_count.get(key, 0) + 1
        return t

    def apply(self, plan: dict) -> None:
        self._round += 1
        ta = time.perf_counter()
        pressure = plan.get("ckpt") == "pressure"
        if pressure:
            # jobs this rank runs or starts this round must stay resident
            protect = {jid for jid, _ in plan["assign"].get(self.rank) or []}
            protect |= {a["job"] for a in plan["actions"] if a["op"] == "start"}
            ro = plan.get("resume_order")
            for a in plan["actions"]:
                if a["op"] != "start" or self.rank not in a["ranks"]:
                    continue
                t = self.trainers.get(a["job"])
                if t is None:
                    if self.pool.get(self._pool_key(a)):
                        continue               # a warm-pool reuse needs no new HBM
                    self._make_room(self._job_need(a["model"], a.get("batch"), a.get("opt_dtype")), protect, ro)
                elif getattr(t, "_spilled", None):
                    self._make_room(t.hbm_bytes(), protect, ro)
            ta = self._ap("pressure_room", ta)
        moves: Dict[str, tuple] = {}          # job -> ([(send|recv, buffer, peer)], action), plan order
        snap_loads: Dict[str, tuple] = {}     # job -> (local load ok, action): restarts from snapshots
        for a in plan["actions"]:
            op = a["op"]
            if op != "start":
                key = op
            elif a["source"] == "fresh" and self.rank in a["ranks"]:
                key = "start_fresh_pool" if self.pool.get((a["model"], a.get("batch"), tuple(a["ranks"]))) \
                    else "start_fresh_build"
            else:
                key = "start_" + a["source"]
            ta = self._apply_one(a, op, moves, snap_loads, ta, key)
        ta = self._finish_apply(plan, moves, snap_loads, pressure, ta)

    def _apply_one(self, a, op, moves, snap_loads, ta, key) -> float:
        """One plan action (timed into apply_prof[key])."""
        if op == "group":
            # communicators outlive a replay: every rank holds the same
            # cache (same plans, same order), so skipping is collective-safe
            c = self.groups.get(tuple(a["ranks"]))
            if c is None or getattr(c, "vnode", a.get("vnode", 0)) != a.get("vnode", 0):
                if self.rank in a["ranks"]:
                    try:
                        self._open_group(a["ranks"], a.get("vnode", 0), a.get("nic_gbps", 12.5))
                    except Exception as e:      # a member never arrived: the gang's step fails
                        from ..parallel.gang import FailedComm

                        self.groups[tuple(a["ranks"])] = FailedComm(a["ranks"], f"{type(e).__name__}: {e}")
        elif op == "consolidate":
            t = self.trainers.get(a["job"])
            if t is not None and self.rank in a["ranks"]:
                try:
                    self.consolidated_bytes += t.consolidate()
                except Exception as e:           # a member died: no one holds the whole state
                    print(f"[worker {self.rank}] job {a['job']}: consolidate over {a['ranks']} failed "
                          f"({type(e).__name__}: {e})", file=sys.stderr, flush=True)
                    abort_comm(t.group)
                    self.trainers.pop(a["job"], None)
                    t.release()
                    self._consolidate_failed.add(a["job"])
        elif op == "ungroup":
            self._close_group(a["ranks"])
        elif op == "abort":
            self._close_group(a["ranks"], abort=True, dead=a.get("dead"), purge=a.get("purge"))
        elif op == "drop":
            self.streams.pop(a["job"], None)
            self._retire(self.trainers.pop(a["job"], None))
            self._job_ranks.pop(a["job"], None)
            self._snap_acc.pop(a["job"], None)
            # the holder's lowest rank deletes the (shared) file, and so
            # does every rank whose writer ever snapshotted the job -- an
            # earlier holder's queued write must not re-create it later
            if self.snap is not None and (self.rank == min(a["ranks"]) or self.snap.wrote(a["job"])):
                self.snap.drop(a["job"])
        elif op == "spill":
            if self.trainers.get(a["job"]) is not None:
                self._spill(a["job"])
        elif op == "start":
            ranks = tuple(a["ranks"])
            src = a["source"]
            self._job_ranks[a["job"]] = ranks
            if src == "snapshot":
                # the job's only replica died: rebuild from its last
                # durable snapshot (every gang member reads the file); a
                # missing / truncated / unreadable file fails the load on
                # that member, and the members agree on the verdict below
                if self.rank in ranks:
                    from ..ckpt.snapshot import load_snapshot

                    old_t = self.trainers.pop(a["job"], None)
                    if old_t is not None:
                        old_t.release()
                    t = self._make_trainer(a, init=False)
                    ok = True
                    try:
                        load_snapshot(a["path"], t)
                    except Exception as e:
                        ok = False
                        print(f"[worker {self.rank}] job {a['job']}: snapshot {a['path']} unreadable "
                              f"({type(e).__name__}: {e}); restarting it from scratch",
                              file=sys.stderr, flush=True)
                    self.trainers[a["job"]] = t
                    self._snap_acc[a["job"]] = 0.0
                    snap_loads[a["job"]] = (ok, {**a, "old": []})
            elif src == "fresh":
                if self.rank in ranks:
                    before = torch.cuda.memory_allocated(self.device) if self.device.type == "cuda" else 0
                    self.trainers[a["job"]] = self._make_trainer(a)
                    if self.device.type == "cuda":
                        grown = torch.cuda.memory_allocated(self.device) - before
                        if grown > 0:      # a newly built trainer (not a warm-pool reuse)
                            # what _resident_bytes will count for it (state + batch)
                            nk = (a["model"], "bf16") if a.get("opt_dtype") == "bf16" else a["model"]
                            self._need[nk] = max(self._need.get(nk, 0.0), float(grown))
            elif src == "resident":
                t = self.trainers.get(a["job"])
                if t is not None and getattr(t, "_spilled", None):
                    self._restore(a["job"])
                if t is not None and self.rank in ranks:
                    self._bind(t, ranks)
            elif src == "p2p":
                donors = {int(k): v for k, v in a["donors"].items()}
                old = tuple(a["old"])
                if self.rank in old and self.trainers.get(a["job"]) is not None \
                        and getattr(self.trainers[a["job"]], "_spilled", None):
                    self._restore(a["job"])
                if self.rank in old or self.rank in ranks:
                    # every old holder and new member takes part in the
                    # move's verdict (a leaving holder frees its replica
                    # only when the move succeeded everywhere)
                    moves.setdefault(a["job"], ([], a))
                if self.rank in donors:        # receiver (state arrives by P2P)
                    t = self.trainers.get(a["job"])
                    if t is None:
                        t = self._make_trainer(a, init=False)
                        self.trainers[a["job"]] = t
                    # a resync receiver already holds a (possibly diverged) replica
                    elif t is not None and getattr(t, "_spilled", None):
                        self._restore(a["job"])
                    ops = moves.setdefault(a["job"], ([], a))[0]
                    for name, buf in sorted(t.state_tensors().items()):
                        ops.append(("recv", buf, donors[self.rank], name))
                for recv, donor in donors.items():
                    if donor == self.rank:
                        t = self.trainers[a["job"]]
                        ops = moves.setdefault(a["job"], ([], a))[0]
                        for name, buf in sorted(t.state_tensors().items()):
                            ops.append(("send", buf, recv, name))
                # replicas that stay: rebind their DDP bucketer to the new gang
                if self.rank in ranks and self.rank in old:
                    t = self.trainers[a["job"]]
                    t.rebind(self._group(ranks))
                    # (the trainer's own state format, whatever the action carries)
                    t.pool_key = self._pool_key(dict(a, opt_dtype=t.opt_dtype))
                elif self.rank in ranks:
                    self._bind(self.trainers[a["job"]], ranks)
                if self.rank in ranks and "step" in a:
                    self.trainers[a["job"]].step_count = int(a["step"])
        return self._ap(key, ta)

    def _finish_apply(self, plan, moves, snap_loads, pressure, ta) -> float:
        if any(a["op"] == "drop" for a in plan["actions"]):
            self.reclaim(64.0)
            ta = self._ap("reclaim", ta)
        failed = set()
        if moves or snap_loads:
            if moves and self.shared_device and self.plane is not None:
                ok = self._do_moves_ipc(moves, plan.get("round"))
            else:
                ok = self._do_moves(moves) if moves else {}
            ta = self._ap("p2p_transfer", ta)
            ok.update({jid: v for jid, (v, _) in snap_loads.items()})
            acts = {jid: a for jid, (_, a) in moves.items()}
            acts.update({jid: a for jid, (_, a) in snap_loads.items()})
            failed = self._agree_moves(plan.get("round"), ok, acts)
            ta = self._ap("move_agree", ta)
        for jid in [j for j in failed if j in snap_loads]:
            # some member could not read the snapshot: no member runs the job
            # on it (replicas would disagree); the controller restarts it
            # from scratch and charges the iterations the snapshot held
            failed.discard(jid)
            self._snap_failed.add(jid)
            t = self.trainers.pop(jid, None)
            if t is not None:
                t.release()
        for jid in failed:
            # every participant drops the pair communicators this move used
            # (same verdict everywhere -> same re-creation generation)
            from ..parallel.gang import PG_CACHE

            for pg in getattr(self, "_move_pgs", {}).get(jid, []):
                pg.abort()
                self._pairs.pop(pg.ranks, None)
                PG_CACHE.purge([pg.key])
            # the move did not complete everywhere: replicas on the OLD ranks
            # are the valid ones (the controller re-holds the job there);
            # whatever a receiver got is discarded, and nobody runs the job
            # this round (every participant reached the same verdict)
            a = moves[jid][1]
            self._move_failed.add(jid)
            if self.rank not in a["old"]:
                t = self.trainers.pop(jid, None)
                if t is not None:
                    t.release()
        # holders that are no longer members free their replica after sending
        for a in plan["actions"]:
            if a["op"] == "start" and a["source"] == "p2p" and a["job"] not in failed:
                if self.rank in a["old"] and self.rank not in a["ranks"]:
                    self._retire(self.trainers.pop(a["job"], None))
        if pressure:
            self._prefetch(plan.get("resume_order") or [])
            ta = self._ap("prefetch", ta)
        return ta

    # ------------------------------------------------------------ state moves
    def _pair_pg(self, peer: int):
        """State moves run on a dedicated 2-rank communicator per rank pair
        (``PG_CACHE``, pinned): never the world communicator -- an in-flight
        move with a rank that dies would poison it for every later move --
        and abortable by the control plane's watcher like any gang
        communicator. At most world-1 per rank; the bench pre-creates them."""
        from ..parallel.gang import PG_CACHE

        pair = (min(self.rank, peer), max(self.rank, peer))
        pg = self._pairs.get(pair)
        if pg is None or pg.aborted:
            # a move can meet a peer that dies in the same round: bound the
            # rendezvous by the control plane's loss detection, not 180 s
            hb = getattr(self.plane, "hb_timeout", None)
            pg = PG_CACHE.acquire(pair, self.rank, self.gang_backend, pin=True,
                                  create_s=max(15.0, 3.0 * hb) if hb else None)
            self._pairs[pair] = pg
        return pg

    def precreate_pairs(self) -> None:
        """Create + warm every pair communicator this rank belongs to, in one
        global order (no rendezvous cycle); call collectively, untimed."""
        for a in range(self.world):
            for b in range(a + 1, self.world):
                if self.rank in (a, b):
                    pg = self._pair_pg(b if self.rank == a else a)
                    pg.warm(self.device if pg.backend == "nccl" else torch.device("cpu"))

    def _do_moves(self, moves) -> Dict[str, bool]:
        """Run each job's state transfer (plan order, so every pair issues its
        sends / receives in the same sequence); returns job -> local success
        (the pair communicators used are kept in ``_move_pgs``)."""
        ok: Dict[str, bool] = {}
        cuda = self.device.type == "cuda"
        stage = cuda and self.gang_backend == "gloo"      # gloo moves host memory (one-GPU rehearsal)
        if stage:
            torch.cuda.synchronize(self.device)
        used: Dict[str, list] = {}
        for jid, (ops, _) in moves.items():
            pgs, works, staged = [], [], []
            try:
                for kind, buf, peer, _ in ops:
                    pg = self._pair_pg(peer)
                    pgs.append(pg)
                    t = buf
                    if stage:
                        t = buf.cpu() if kind == "send" else torch.empty(buf.shape, dtype=buf.dtype)
                        if kind == "recv":
                            staged.append((buf, t))
                    other = pg.ranks.index(peer)
                    works.append(pg.pg.send([t], other, 0) if kind == "send" else pg.pg.recv([t], other, 0))
                for w in works:
                    w.wait()
                for dst, h in staged:
                    dst.copy_(h)
                ok[jid] = True
            except Exception:
                ok[jid] = False
            used[jid] = pgs
        if cuda and moves:
            try:
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
        for jid, pgs in used.items():
            if any(pg.failed() for pg in pgs):
                ok[jid] = False
        self._move_pgs = used
        return ok

    def _do_moves_ipc(self, moves, rnd) -> Dict[str, bool]:
        """State moves when every rank drives the SAME physical GPU (the
        one-GPU multi-rank rehearsal, ``TAM_SHARED_GPU=1``: gloo
        communicators would stage every byte through host memory and TCP --
        0.5 s per move measured). The donor exports each state buffer as a
        HIP IPC handle through the control store; the receiver maps it and
        copies device to device, then acknowledges, and only then may the
        donor free its replica. Jobs in plan order on every rank."""
        import pickle

        from torch.multiprocessing.reductions import reduce_tensor

        plane = self.plane
        rt = plane._retry
        pre = f"{plane.prefix}/ipc/{rnd}"
        bound = max(30.0, 4.0 * plane.hb_timeout)

        def wait_key(k, peer, what):
            t0 = time.time()
            while not rt(lambda: plane.store.check([k]), what):
                if peer in plane.dead or time.time() - t0 > bound:
                    raise RuntimeError(f"{what}: rank {peer} silent")
                time.sleep(0.0005)

        ok: Dict[str, bool] = {}
        for jid, (ops, _) in moves.items():
            try:
                sends = [(buf, peer, name) for kind, buf, peer, name in ops if kind == "send"]
                if sends:
                    torch.cuda.current_stream(self.device).synchronize()   # donor state final
                    for buf, peer, name in sends:
                        data = pickle.dumps(reduce_tensor(buf))
                        rt(lambda k=f"{pre}/{jid}/{self.rank}-{peer}/{name}", d=data: plane.store.set(k, d),
                           "ipc handle")
                recvs = [(buf, peer, name) for kind, buf, peer, name in ops if kind == "recv"]
                for buf, peer, name in recvs:
                    k = f"{pre}/{jid}/{peer}-{self.rank}/{name}"
                    wait_key(k, peer, f"ipc move of {jid}")
                    fn, args = pickle.loads(rt(lambda: plane.store.get(k), "ipc handle"))
                    src = fn(*args)
                    buf.copy_(src)
                    del src
                if recvs:
                    torch.cuda.current_stream(self.device).synchronize()
                    rt(lambda: plane.store.set(f"{pre}/{jid}/ack/{self.rank}", b"1"), "ipc ack")
                for peer in sorted({p for _, p, _ in sends}):
                    wait_key(f"{pre}/{jid}/ack/{peer}", peer, f"ipc ack of {jid}")
                # the acks say every receiver read (and copied) its handles:
                # the donor, their only other reader, removes them and the
                # acks, so the store does not grow over a long replay
                for buf, peer, name in sends:
                    _store_del(plane, f"{pre}/{jid}/{self.rank}-{peer}/{name}")
                for peer in sorted({p for _, p, _ in sends}):
                    _store_del(plane, f"{pre}/{jid}/ack/{peer}")
                ok[jid] = True
            except Exception as e:
                print(f"[worker {self.rank}] ipc move of job {jid} failed ({type(e).__name__}: {e})",
                      file=sys.stderr, flush=True)
                ok[jid] = False
        self._move_pgs = {}
        return ok

    def _agree_moves(self, rnd, ok: Dict[str, bool], acts: Dict[str, dict]) -> set:
        """All participants of a job's move (old holders + new members) reach
        the SAME verdict through the control store before anyone runs the
        job: each publishes its local outcome; the lowest live participant
        decides (all published flags good -> ok; a flag that is bad, or whose
        rank died, or that stays missing past the bound -> failed) and writes
        the verdict with compare-and-set (first writer wins if a successor
        took over from a decider that died); everyone adopts the stored
        verdict. A local timeout per participant would let ranks disagree.
        Returns the failed jobs."""
        plane = self.plane
        if plane is None or rnd is None:
            return {j for j, v in ok.items() if not v}
        pre = f"{plane.prefix}/mv/{rnd}"
        # every store operation goes through the plane's reconnect-and-retry
        # (a client socket dropped under host load while a peer dies must not
        # take a surviving rank down with it)
        rt = plane._retry
        for jid, v in ok.items():
            rt(lambda: plane.store.set(f"{pre}/{jid}/{self.rank}", b"1" if v else b"0"), "move flag")
        bad = set()
        bound = max(30.0, 4.0 * plane.hb_timeout)
        for jid, a in acts.items():
            parts = sorted(set(a["old"]) | set(a["ranks"]))
            vkey = f"{pre}/{jid}/verdict"
            t0 = time.time()
            verdict = None
            while verdict is None:
                if rt(lambda: plane.store.check([vkey]), "move verdict"):
                    verdict = rt(lambda: plane.store.get(vkey), "move verdict")
                    break
                live = [r for r in parts if r not in plane.dead]
                if live and live[0] == self.rank:
                    good = True
                    for r in parts:
                        k = f"{pre}/{jid}/{r}"
                        while True:
                            if r in plane.dead:
                                good = False
                                break
                            if rt(lambda: plane.store.check([k]), "move flag"):
                                good = good and rt(lambda: plane.store.get(k), "move flag") == b"1"
                                break
                            if time.time() - t0 > bound:
                                good = False
                                break
                            time.sleep(0.001)
                        if not good:
                            break
                    verdict = rt(lambda: plane.store.compare_set(vkey, "", b"1" if good else b"0"),
                                 "move verdict")
                    break
                if time.time() - t0 > 4 * bound:      # decider silent far past its own bound
                    verdict = rt(lambda: plane.store.compare_set(vkey, "", b"0"), "move verdict")
                    break
                time.sleep(0.001)
            if verdict != b"1":
                bad.add(jid)
        return bad

    def _prefetch(self, resume_order) -> None:
        """Restore ahead: the spilled job the scheduler will resume FIRST comes
        back to HBM now, while this round's jobs compute (the H2D runs on the
        engine's side stream), when it fits without spilling anything. Its
        later resume is then a pointer swap instead of an H2D on the critical
        path."""
        for jid in resume_order[:1]:
            t = self.trainers.get(jid)
            if t is None or not getattr(t, "_spilled", None):
                continue
            margin = 0.05 * (self.hbm_budget or 0.0)
            if self._free_bytes() >= t.hbm_bytes() + margin:
                self._restore(jid)
                self.prefetches += 1

    def _dev_sample(self) -> Optional[dict]:
        """Real HBM / activity of this rank's GPU (hipMemGetInfo + amd-smi),
        at most every monitor period; None on CPU."""
        if self.monitor is None:
            return None
        now = time.monotonic()
        if now - self._mon_t < self.monitor.period:
            return None
        self._mon_t = now
        d = self.monitor.sample_own()
        if d is None:
            return None
        return {"util_pct": d.util_pct, "free_mb": round(d.free_mb, 1), "total_mb": round(d.total_mb, 1)}

    def run(self, plan: dict) -> dict:
        """Run this rank's share of the round. One job: its ``n`` steps back
        to back. Several (GPU sharing): the jobs' steps interleaved in job-id
        order, each job on its own HIP stream so their kernels overlap on the
        device; every job is charged the round's wall time (co-location
        slowdown is real, measured time)."""
        jobs = plan["assign"].get(self.rank) or []
        skipped = [{"job": jid, "iters": 0, "run_s": 0.0, "shared": False, "loss": None, "move_failed": True}
                   for jid in sorted(self._move_failed)]
        skipped += [{"job": jid, "iters": 0, "run_s": 0.0, "shared": False, "loss": None, "snap_failed": True}
                    for jid in sorted(self._snap_failed)]
        skipped += [{"job": jid, "iters": 0, "run_s": 0.0, "shared": False, "loss": None,
                     "consolidate_failed": True} for jid in sorted(self._consolidate_failed)]
        self._move_failed = set()
        self._snap_failed = set()
        self._consolidate_failed = set()
        # fill-mode steps the last plan's snapshot did not count
        carry = {}
        for r in self._carry:
            if r.get("fill"):
                carry[r["job"]] = carry.get(r["job"], 0) + int(r.get("iters") or 0)
        skipped += self._carry
        self._carry = []
        jobs = [(jid, n) for jid, n in jobs if jid not in {r["job"] for r in skipped if not r.get("fill")}]
        # those carried steps are not in the plan's done count yet (they are
        # credited with THIS report): the plan's share + left would use the
        # same remaining iterations twice. The carry is the same
        # on every gang member (equal fill steps, plan-level fill_seen), so
        # the capped share still matches across the gang.
        self._fill_cap = {}
        if carry:
            left_of = plan.get("left") or {}
            capped = []
            for jid, n in jobs:
                c = carry.get(jid, 0)
                if c > 0 and isinstance(left_of, dict) and jid in left_of:
                    rem = int(left_of[jid]) + int(n) - c     # iterations really left before the share
                    n2 = max(0, min(int(n), rem))
                    self._fill_cap[jid] = max(0, rem - n2)
                    n = n2
                capped.append((jid, n))
            jobs = capped
        if not jobs:
            return {"rank": self.rank, "job": None, "jobs": skipped, "dev": self._dev_sample(),
                    "ckpt": self._ckpt_report(), "snap": self._snap_poll()}
        for jid, _ in jobs:
            self._last_run[jid] = self._round
        cuda = self.device.type == "cuda"
        t0 = time.perf_counter()
        err = None
        if len(jobs) == 1:
            jid, n = jobs[0]
            t = self.trainers[jid]
            deadline = plan.get("deadline")
            if cuda and getattr(t.model, "persist", False):
                # alone in this worker: persistent grids unless another rank
                # of the one-GPU rehearsal runs one this round
                t.set_persist_shared(self._persist_elsewhere(plan, jid))
            if deadline is None or t.ddp is not None:
                # gang members must run the same step count (collectives)
                done = 0
                try:
                    for _ in range(n):
                        t.step()
                        done += 1
                except Exception as e:        # a gang peer died mid-collective
                    err = f"{type(e).__name__}: {e}"
                    t.broken = True
                    jobs = [(jid, done)]
            else:
                n = self._run_until(t, n, deadline, cuda)
                jobs = [(jid, n)]
        else:
            if cuda:
                # two co-located jobs' persistent LSTM grids (different kernels,
                # different per-CU footprints) cannot be guaranteed co-resident:
                # each would spin at its grid barrier waiting for workgroups the
                # other holds the CUs of. A job that shares its GPU with another
                # persistent-grid job takes the per-step recurrence from here on
                pers = [jid for jid, _ in jobs if getattr(self.trainers[jid].model, "persist", False)]
                for jid in pers:
                    self.trainers[jid].set_persist_shared(len(pers) > 1 or self._persist_elsewhere(plan, jid))
            streams = [self._stream(jid) if cuda else None for jid, _ in jobs]
            if cuda:
                # apply() ran on the default stream: fresh jobs' weight init
                # and synthetic batch, restores and P2P receives are queued
                # there; the per-job streams must not run ahead of them
                cur = torch.cuda.current_stream(self.device)
                for st in streams:
                    st.wait_stream(cur)
            for i in range(max(n for _, n in jobs)):
                for (jid, n), st in zip(jobs, streams):
                    if i >= n:
                        continue
                    if st is None:
                        self.trainers[jid].step()
                    else:
                        with torch.cuda.stream(st):
                            self.trainers[jid].step()
        if cuda:
            torch.cuda.synchronize(self.device)
        dt = time.perf_counter() - t0
        for jid, _ in jobs:
            # hipGraph captures of fresh trainers ran inside these steps
            t = self.trainers.get(jid)
            if t is not None and t.capture_s > getattr(t, "_cap_seen", 0.0):
                self.apply_prof["graph_capture_in_run"] = self.apply_prof.get("graph_capture_in_run", 0.0) + \
                    t.capture_s - getattr(t, "_cap_seen", 0.0)
                t._cap_seen = t.capture_s
        persist_err: Dict[str, str] = {}
        if cuda:
            # the persistent LSTM kernels never hang: a grid barrier that timed
            # out bumped the JOB's own timeout word, its optimizer skipped that
            # step's update and counted it -- read once per round, per job: the
            # skipped steps are not progress, and only that job falls back to
            # the per-step recurrence
            fixed = []
            for jid, n in jobs:
                t = self.trainers[jid]
                sk = t.persist_skipped(reset=True) if t.uses_persist else 0
                if sk:
                    t.disable_persist()
                    persist_err[jid] = (f"PersistTimeout: {sk} step(s) of job {jid} hit a persistent LSTM "
                                        f"barrier timeout (update skipped); it falls back to the per-step "
                                        f"recurrence")
                fixed.append((jid, max(0, n - sk)))
            jobs = fixed
        if len(jobs) == 1 and err is None:
            t = self.trainers[jobs[0][0]]
            if t.ddp is not None and comm_failed(t.group):
                # the NCCL watchdog (CleanUpOnly) or the control plane's
                # watcher aborted the communicator under this round's steps
                err = "gang communicator failed (aborted / watchdog timeout)"
        if err is not None and len(jobs) == 1 and not err.startswith("PersistTimeout"):
            t = self.trainers[jobs[0][0]]
            if t.group is not None:
                abort_comm(t.group)            # never step on it again
        if self.snap is not None and err is None:
            for jid, n in jobs:
                ranks = self._job_ranks.get(jid, (self.rank,))
                if n <= 0 or self.rank != min(ranks) or self.trainers[jid].state_sharded:
                    continue                         # (sharded gangs: state consolidated on suspension)
                acc = self._snap_acc.get(jid, 0.0) + dt
                if acc >= self.snapshot_s:
                    acc = 0.0
                    self.snap.snapshot(jid, self.trainers[jid])
                self._snap_acc[jid] = acc
        reps = []
        for jid, n in jobs:
            t = self.trainers[jid]
            rep = {"job": jid, "iters": n, "run_s": dt, "shared": len(jobs) > 1,
                   "loss": float(t.last_loss) if (t.last_loss is not None and err is None) else None}
            if t.ddp is not None:
                # hipEvent-measured gradient sync of the steps finished so far
                ct = t.ddp.poll_timing()
                if ct["steps"] or ct.get("bytes_steps"):
                    rep["comm"] = ct
            if err or jid in persist_err:
                rep["error"] = err or persist_err[jid]
            reps.append(rep)
        return {"rank": self.rank, "job": jobs[0][0], "jobs": reps + skipped, "dev": self._dev_sample(),
                "ckpt": self._ckpt_report(), "snap": self._snap_poll()}

    def _snap_poll(self):
        if self.snap is None:
            return None
        got = self.snap.poll()
        self.snap_reported.update(jid for jid, _, _ in got)
        return got

    def _persist_elsewhere(self, plan: dict, jid: str) -> bool:
        """In the one-GPU multi-rank rehearsal (TAM_SHARED_GPU=1) every rank
        drives the same device: another rank's persistent-grid job this round
        (plan["persist_jobs"], from the controller) shares the GPU with ``jid``
        (the in-worker check cannot see other ranks)."""
        if os.environ.get("TAM_SHARED_GPU") != "1" or self.world <= 1:
            return False
        others = set(plan.get("persist_jobs") or []) - {jid}
        return bool(others)

    # ------------------------------------------------------------ fill mode
    def fill_begin(self, plan: dict, rep: dict) -> None:
        """After this rank's share of the round: keep stepping its (single,
        exclusive) job until the next plan is out, instead of idling at the
        round barrier while slower ranks finish (fake backend, headline
        trace, N=8: barrier idle 20 % -> 2 % of GPU time). Bounded by the
        job's iterations left (minus any uncredited carry, ``run``); a gang
        agrees on every extra step (``_vote``).

        Gang eligibility is decided on PLAN data only (one job on this rank,
        iterations left), so every member enters the same votes: a member
        that cannot step (no trainer, a spilled or broken one, an error in
        its share) still votes -- stop -- in the first vote whenever its
        communicator is usable, and the gang stops before any fill step. A
        member without a usable communicator casts nothing; its peers' vote
        then times out (``VOTE_TIMEOUT_S``), the gang is marked broken and the
        controller recovers it, instead of the peers blocking for the
        collective timeout."""
        self._fill = None
        if not self.fill_enabled:
            return
        mine = plan["assign"].get(self.rank) or []
        if len(mine) != 1:
            return
        jid = mine[0][0]
        left_of = plan.get("left") or {}
        left = int(left_of.get(jid, 0)) if isinstance(left_of, dict) else 0
        cap = getattr(self, "_fill_cap", {})
        if jid in cap:
            left = min(left, cap[jid])
        if left <= 0:                              # plan-level (+ the gang-wide carry): same on every member
            return
        t = self.trainers.get(jid)
        gang = len(self._job_ranks.get(jid, (self.rank,))) > 1
        if t is None or (gang and t.ddp is None):
            return                                 # nothing to vote with: peers time out (bounded)
        comm_ok = not gang or (t.ddp.comm is not None and not comm_failed(t.group))
        if not comm_ok:
            return
        local_bad = (getattr(t, "broken", False) or getattr(t, "_spilled", None) or
                     any(r.get("error") for r in rep.get("jobs") or [] if r.get("job") == jid))
        if local_bad and not gang:
            return
        if (os.environ.get("TAM_SHARED_GPU") == "1" and self.world > 1 and hasattr(t.model, "shared")
                and not getattr(t, "_persist_shared", False)):
            # one-GPU rehearsal: the next round's plan can start another rank's
            # persistent LSTM grid while this rank's persistent fill step is
            # still in flight (the co-location rule only saw the round just
            # run), so such a job does not fill. The condition is plan-derived
            # (_persist_shared is set from the plan at apply): every gang
            # member takes the same branch
            return
        self._fill = {"job": jid, "left": 0 if local_bad else left, "n": 0, "sec": 0.0, "gang": gang,
                      "done": False, "prev": None, "err": None, "t": t}

    def _vote(self, t: Trainer, stop: bool) -> bool:
        """One-element SUM all-reduce over the job's gang: does ANY member
        want to stop? Every member takes the same decision, so the gang runs
        the same number of fill steps on every member (its collectives
        match).

        On the GPU the vote never drains the compute stream: it is issued on
        a side stream, so it waits for nothing on the compute stream, and on
        the communicator's own stream it queues right behind the previous
        step's gradient buckets -- it completes when that step's LAST bucket
        is reduced, while the step's optimizer still runs. The result comes
        back by a D2H copy into pinned memory and a host wait on THAT event
        (no ``.item()``, no stream synchronize): the host is throttled to one
        step ahead and the GPU never idles between fill steps (VERDICT r5
        item 6). The wait is bounded: a member that never votes makes this
        one raise, and the step is failed like a gang collective error."""
        cuda = self.device.type == "cuda"
        vb = getattr(t, "_vote_bufs", None)
        if vb is None:
            v = torch.zeros(1, dtype=torch.float32, device=self.device)
            vh = torch.zeros(1, dtype=torch.float32, pin_memory=cuda)
            side = torch.cuda.Stream(self.device) if cuda else None
            vb = t._vote_bufs = (v, vh, side)
        v, vh, side = vb
        c = t.ddp.comm
        deadline = time.perf_counter() + VOTE_TIMEOUT_S
        if not cuda:
            v.fill_(1.0 if stop else 0.0)
            h = c.start(v)
            if hasattr(h, "wait"):                 # a c10d Work (flat gang): bounded wait
                from datetime import timedelta
                h.wait(timedelta(seconds=VOTE_TIMEOUT_S))
            else:
                c.finish([h])
            return float(v[0]) > 0.0
        with torch.cuda.stream(side):
            v.fill_(1.0 if stop else 0.0)
            c.finish([c.start(v)])                 # side stream waits on the collective
            vh.copy_(v, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        while not ev.query():
            if time.perf_counter() > deadline:
                raise RuntimeError(f"fill vote timed out after {VOTE_TIMEOUT_S:.0f} s (a gang member never voted)")
            time.sleep(20e-6)
        return float(vh[0]) > 0.0

    def fill_step(self, ready: bool) -> bool:
        """One fill step when the round's next plan is not out yet
        (``ready`` False); returns False once this rank's fill is over."""
        f = self._fill
        if f is None or f["done"]:
            return False
        t = f["t"]
        cuda = self.device.type == "cuda"
        try:
            if f["gang"]:
                if self._vote(t, ready or f["n"] >= f["left"]):
                    f["done"] = True
                    return False
            elif ready or f["n"] >= f["left"]:
                f["done"] = True
                if f["prev"] is not None:
                    f["prev"].synchronize()
                return False
            t0 = time.perf_counter()
            t.step()
            if cuda and not f["gang"]:
                # keep one step queued ahead of the one waited on (the GPU
                # never drains between fill steps); a gang is throttled by
                # its next vote instead (no per-step host sync)
                ev = torch.cuda.Event()
                ev.record()
                if f["prev"] is not None:
                    f["prev"].synchronize()
                f["prev"] = ev
            f["n"] += 1
            dt = time.perf_counter() - t0
            f["sec"] += dt
            self.fill_s_total += dt
            self.fill_steps_total += 1
            return True
        except Exception as e:                    # a gang peer died mid-collective / never voted
            f["err"] = f"{type(e).__name__}: {e}"
            f["done"] = True
            t.broken = True
            if t.group is not None:
                abort_comm(t.group)
            return False

    def fill_counts(self) -> Dict[str, int]:
        f = self._fill
        return {f["job"]: f["n"]} if f is not None and f["n"] else {}

    def fill_end(self, seen: Dict[str, int]) -> None:
        """The next plan is here: the fill steps its snapshot did not count
        (``seen``: the controller's credited count per job) are reported with
        the next round."""
        f, self._fill = self._fill, None
        if f is None:
            return
        if f["prev"] is not None and not f["done"]:
            f["prev"].synchronize()
        extra = f["n"] - int(seen.get(f["job"], 0))
        if extra > 0 or f["err"]:
            e = {"job": f["job"], "iters": max(0, extra), "run_s": f["sec"] * max(0, extra) / max(1, f["n"]),
                 "shared": False, "loss": None, "fill": True}
            if f["err"]:
                e["error"] = f["err"]
            self._carry.append(e)

    def _ckpt_report(self) -> Optional[dict]:
        """Per-job spill / restore bytes and measured device copy seconds since
        the last report (polls the engine's events: never blocks)."""
        for jid, t in self.trainers.items():
            if getattr(t, "_spilled", None) or getattr(t, "_restored", None):
                got = t.ckpt_poll()
                if got["save_s"] or got["restore_s"]:
                    c = self._ckpt.setdefault(jid, {"bytes": 0.0, "save_s": 0.0, "restore_s": 0.0})
                    c["save_s"] += got["save_s"]
                    c["restore_s"] += got["restore_s"]
        if not self._ckpt:
            return None
        out, self._ckpt = self._ckpt, {}
        return out

    def _run_until(self, t: Trainer, n: int, deadline: float, cuda: bool) -> int:
        """Up to ``n`` steps of a 1-GPU job, ending the round at the first step
        boundary after ``deadline`` (the next trace arrival, host monotonic
        clock shared by every rank of the node) so the scheduler can react to
        it within ~one step instead of up to a whole quantum. One step stays
        queued ahead of the one being waited on, so the GPU never drains."""
        prev = None
        for i in range(n):
            t.step()
            if cuda:
                ev = torch.cuda.Event()
                ev.record()
                if prev is not None:
                    prev.synchronize()
                prev = ev
            if time.perf_counter() >= deadline and i + 1 < n:
                return i + 1
        return n

    def _stream(self, jid: str):
        st = self.streams.get(jid)
        if st is None:
            st = torch.cuda.Stream(self.device)
            self.streams[jid] = st
        return st

    def reclaim(self, slack_gb: float) -> bool:
        """Return cached-but-unused HBM to the driver when more than
        ``slack_gb`` is held. Finished jobs' hipGraph private pools stay
        reserved by the caching allocator until empty_cache() (a pool cannot
        be shared between jobs that may run concurrently on one GPU), so
        without this every job's pool would accumulate. Called with a small
        slack when the GPU is idle between arrivals and a large one after
        drops (a full empty_cache costs milliseconds)."""
        if self.device.type != "cuda":
            return False
        slack = torch.cuda.memory_reserved(self.device) - torch.cuda.memory_allocated(self.device)
        if slack <= slack_gb * 2 ** 30:
            return False
        torch.cuda.synchronize(self.device)
        torch.cuda.empty_cache()
        return True

    def clear(self, keep_pool: bool = True):
        for t in self.trainers.values():
            self._retire(t)
        self.trainers.clear()
        self.streams.clear()
        if not keep_pool:
            self.drain_pool()
        self.reclaim(0.0)


class _HostEngine:
    """CPU stand-in for the native engine (tests / gloo rehearsals)."""

    def __init__(self):
        self.store = {}
        self.n = 0

    def spill(self, t):
        self.n += 1
        self.store[self.n] = t.detach().clone()
        return self.n

    def wait(self, h):
        pass

    def restore(self, h, dst):
        dst.copy_(self.store[h])

    def release(self, h):
        self.store.pop(h, None)


def _abort(ctrl: "Controller", log, rounds: int, reason: str) -> dict:
    s = ctrl.sched
    lost = []
    for j in list(s.active):
        if j.job_id in ctrl.holders:
            j.state = JobState.FAILED
            lost.append(j.job_id)
    summ = s.summary()
    summ.update(aborted=True, reason=reason, rounds=rounds, lost_jobs=lost)
    if log:
        log.decision(s.now, "abort", "-", reason=reason)
        log.close()
    return summ


def _bcast(obj, src, pg):
    lst = [obj]
    dist.broadcast_object_list(lst, src=src, group=pg)
    return lst[0]


class RankLost(RuntimeError):
    pass


def run_replay(cfg: SimConfig, jobs: List[ReplayJob], rank: int, world: int, device: torch.device,
               ctrl_pg=None, world_pg=None, worker: Optional[Worker] = None, quantum: float = 0.4,
               out_dir: Optional[str] = None, use_graph: bool = False, max_rounds: int = 100000,
               fault: Optional[dict] = None, spool=None, prior: Optional[List[float]] = None,
               control: str = "store", hb_timeout: float = 6.0, hb_period: float = 1.0) -> Optional[dict]:
    """Replay ``jobs`` on the live cluster. Returns the summary on rank 0.

    ``control``: ``"store"`` (default; executor/control.py::StorePlane —
    plans and reports through the c10d store, heartbeat threads, a lost rank
    detected within ``hb_timeout`` seconds and RECOVERED in-process) or
    ``"gloo"`` (collective plane; a lost rank aborts the replay).

    Fault injection (failure-detection tests):
      ``{"rank": r, "round": k}`` / ``"kind": "crash"`` -- rank r dies at round k;
      ``{"rank": r, "round": k, "kind": "delay", "seconds": s}`` -- rank r
      stalls s seconds before its round-k work (a straggler delaying its
      gang's all-reduce): detected as slow, NOT as lost; a stall longer than
      the gang communicator timeout fails the gang step (``"where":
      "step"`` stalls after apply, in the first round the rank runs a gang,
      so its peers wait inside the collective), which the controller
      recovers (``Controller.gang_failed``: abort + resync);
      ``"kind": "hang"`` -- rank r stops heartbeating and blocks forever
      (a hung GPU / process): declared lost by rank 0's monitor thread while
      its gang peers may still be blocked in a collective with it.

    Recovery (store plane): the lost GPU leaves the cluster; every job with
    state on it is preempted. A DDP gang keeps its replicas on the surviving
    members (data parallelism replicates params + optimizer state) and
    resumes from them at its last completed iteration, re-placed on live
    ranks through the normal P2P move / communicator rebind path; a job whose
    only replica died restarts from scratch (its progress is charged back).
    """
    distributed = world > 1
    ctrl = None
    log = None
    if distributed:
        # ranks declared lost belong to the replay that lost them: bench.py
        # runs several replays per process, and a stale entry would block
        # every later communicator that includes that rank
        from ..parallel.gang import DEAD_RANKS
        DEAD_RANKS.clear()
    w = worker or Worker(rank, world, device, world_pg, use_graph=use_graph)
    if rank == 0:
        log = MetricsLogger(out_dir, node_logs=False)
        ctrl = Controller(cfg, jobs, world, quantum, logger=log, spool=spool, prior=prior,
                          comms=w.comm_registry)
        ctrl.fill_rounds = distributed and control == "store" and w.fill_enabled
    plane = None
    if distributed:
        if control == "store":
            from ..parallel.gang import PG_CACHE, note_dead
            from .control import StorePlane

            def _on_dead(r: int) -> None:
                # watcher / monitor thread: unblock this rank's training
                # thread if it is inside a collective with the dead rank, or
                # inside a communicator rendezvous that includes it
                note_dead(r)
                PG_CACHE.abort_where(lambda k: r in k[0])

            plane = StorePlane(rank, world, hb_period=hb_period, hb_timeout=hb_timeout, on_dead=_on_dead)
            w.plane = plane
        else:
            from .control import GlooPlane

            plane = GlooPlane(ctrl_pg, rank, world)
        dist.barrier(group=ctrl_pg)
    if ctrl:
        ctrl.start_clock()
    t_start = time.perf_counter()
    rounds = 0
    shared = 0                                   # rounds with co-located jobs on a GPU
    # idle_s = sleeping because no job is runnable (arrival gaps), not overhead
    prof = {"plan_s": 0.0, "bcast_s": 0.0, "apply_s": 0.0, "run_s": 0.0, "idle_s": 0.0,
            "gather_s": 0.0, "fill_s": 0.0}
    ctrl_alive = list(range(world))
    fill0 = (w.fill_s_total, w.fill_steps_total)
    ap0, apc0 = dict(w.apply_prof), dict(w.apply_count)
    lost_ranks: List[int] = []
    try:
        fill = distributed and control == "store" and w.fill_enabled
        while rounds < max_rounds:
            ta = time.perf_counter()
            if ctrl and fill and rounds > 0:
                # fill-mode steps every rank took since its last report (the
                # snapshot this plan counts; later ones come as carry)
                counts = plane.read_fill(rounds - 1, ctrl_alive)
                counts[0] = w.fill_counts()
                ctrl.plan_fill = ctrl.credit_fill(counts)
            plan = ctrl.plan_round() if ctrl else None
            tb = time.perf_counter()
            if distributed:
                plan = plane.bcast(plan, rounds)
            if fill:
                w.fill_end(plan.get("fill_seen") or {})
            tc = time.perf_counter()
            plan["round"] = rounds
            if plan["stop"]:
                w.apply(plan)                          # the last finished jobs' drops
                if plane is not None and hasattr(plane, "finish"):
                    plane.finish(plan.get("alive", range(world)))
                break
            if rank not in plan.get("alive", (rank,)):
                # declared lost (hung past the control plane's bound): this
                # rank's GPU has left the cluster -- stop participating
                break
            if fault and fault.get("rank") == rank and rounds >= fault.get("round", 0) and (
                    fault.get("when") != "snapshotted" or any(
                        jid in w.snap_reported and w._job_ranks.get(jid) == (rank,)
                        and jid in {j for j, _ in plan["assign"].get(rank) or []} for jid in w.trainers)):
                # ("when": "snapshotted" -- only once this rank holds the ONLY
                # replica of a job whose snapshot the controller knows of)
                if fault.get("kind", "crash") == "crash":
                    if fault.get("corrupt_snapshots") and worker.snap is not None:
                        # the crash also tears the shared snapshot store:
                        # every snapshot file is truncated
                        worker.snap.flush(10.0)
                        for f in os.listdir(worker.snap.dir):
                            if f.endswith(".pt"):
                                try:             # another rank's writer may drop it meanwhile
                                    with open(os.path.join(worker.snap.dir, f), "r+b") as fh:
                                        fh.truncate(16)
                                except FileNotFoundError:
                                    pass
                    os._exit(17)                     # simulated node/rank crash
                if fault.get("kind") == "hang":
                    if plane is not None:
                        plane.close()                # heartbeat stops
                    while True:
                        time.sleep(3600)
                if not fault.get("_done") and fault.get("where", "apply") == "apply":
                    fault["_done"] = True
                    time.sleep(float(fault.get("seconds", 1.0)))   # straggler
            if any(len(v) > 1 for v in plan["assign"].values()):
                shared += 1
            w.apply(plan)
            if fault and fault.get("rank") == rank and rounds >= fault.get("round", 0) \
                    and fault.get("where") == "step" and not fault.get("_done") \
                    and any(len(w.trainers[j].group.ranks) > 1 if getattr(w.trainers.get(j), "ddp", None) else False
                            for j, _ in plan["assign"].get(rank) or []):
                fault["_done"] = True                  # straggler inside a gang step: peers wait in the collective
                time.sleep(float(fault.get("seconds", 1.0)))
            td = time.perf_counter()
            rep = w.run(plan)
            te = time.perf_counter()
            prof["plan_s"] += tb - ta
            prof["bcast_s"] += tc - tb
            prof["apply_s"] += td - tc
            prof["run_s"] += te - td
            if plan.get("wait", 0) > 0 and rep["job"] is None:
                tw = time.perf_counter()
                w.reclaim(4.0)                     # idle GPU: a free moment to return dead pools
                time.sleep(max(0.0, plan["wait"] - (time.perf_counter() - tw)))
            tf = time.perf_counter()
            prof["idle_s"] += tf - te
            newly: List[int] = []
            if distributed:
                if fill:
                    w.fill_begin(plan, rep)
                try:
                    if fill and rank == 0:
                        ctrl_alive = list(plan.get("alive", range(world)))
                        reps, newly = plane.gather(rep, rounds, ctrl_alive, fill=w.fill_step)
                    else:
                        reps, newly = plane.gather(rep, rounds, plan.get("alive", range(world)))
                    if fill and rank != 0:
                        # keep stepping this rank's job until the next plan is out
                        tw = time.perf_counter()
                        nxt = rounds + 1
                        while True:
                            ready = plane.plan_ready(nxt)
                            if w.fill_step(ready):
                                plane.publish_fill(rounds, w.fill_counts())
                                continue
                            if ready:
                                break
                            time.sleep(0.0003)
                        prof["fill_s"] += time.perf_counter() - tw
                except Exception as e:                 # gloo plane: heartbeat lost
                    if ctrl:
                        return _abort(ctrl, log, rounds, f"rank lost during round {rounds}: {e}")
                    raise RankLost(str(e))
            else:
                reps = [rep]
            if ctrl:
                for r in newly:
                    lost_ranks.append(r)
                    ctrl.rank_lost(r)
                ctrl.apply_reports(reps)
            prof["gather_s"] += time.perf_counter() - tf
            rounds += 1
    finally:
        if plane is not None:
            plane.close()
        w.plane = None
    wall = time.perf_counter() - t_start
    w.clear()
    if device.type == "cuda":
        torch.cuda.synchronize(device)
    if ctrl:
        s = ctrl.sched.summary()
        s.update(rounds=rounds, shared_rounds=shared, replay_wall_s=wall, gang_errors=ctrl.gang_errors,
                 affinity_resumes=ctrl.sched.affinity_hits,
                 step_errors=list(ctrl.error_log),
                 comm_stats=dict(ctrl.comms.stats, live=len(ctrl.comms.live)),
                 iter_est={f"{k[0]}x{k[1]}": v for k, v in ctrl.est.items()},
                 runtime_breakdown={**{k: round(v, 4) for k, v in prof.items()},
                                    "fill_s": round(w.fill_s_total - fill0[0], 4)},
                 fill_steps_rank0=w.fill_steps_total - fill0[1],
                 apply_breakdown_rank0={k: round(v - ap0.get(k, 0.0), 4) for k, v in w.apply_prof.items()},
                 apply_counts_rank0={k: v - apc0.get(k, 0) for k, v in w.apply_count.items()},
                 lost_ranks=lost_ranks, recovered_jobs=sorted(ctrl.recovered),
                 restarted_jobs=sorted(ctrl.restarted), snapshot_restored_jobs=sorted(ctrl.snap_restored),
                 ddp_shard=ctrl.ddp_shard, consolidations=ctrl.consolidations,
                 # measured on the gangs' compute streams (hipEvents, lowest
                 # member): DDP reductions exposed after backward, and the
                 # deferred sharded shadow all-gather's exposed joins vs the
                 # forward window it overlapped
                 comm_totals_s={k: round(sum(j.extra.get(k, 0.0) for j in ctrl.sched.jobs.values()), 6)
                                for k in ("comm_exposed_s", "comm_span_s", "gather_exposed_s", "gather_window_s")},
                 lost_iters={j.job_id: j.extra["lost_iters"] for j in ctrl.sched.jobs.values()
                             if j.extra.get("lost_iters")})
        log.close()
        return s
    return None
