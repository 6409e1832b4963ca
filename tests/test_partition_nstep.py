"""Rank-role partitioning of the n-step driver (algos/sac1/sac_ray.py: the reference's one driver that is both n-step and sharded):
PartitionedRun on window rings — shard owners fold and send transition-shaped blocks, the learners' fold-view samplers follow the step's
plan — with the ranks of ONE GPU over gloo, like tests/test_partition.py.  Every update must have trained on exactly fold32
(tests/_nstep_fold.py) of the windows NumPy's own stream picks from the scheduled owner's ring."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = ("obs1", "obs2", "acts", "rews", "done")
N_ENVS, BATCH, CAP, PREFILL, N_UPD, LN = 64, 32, 4096, 500, 14, 8


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _prefilled_shard(d, opt, r):
    """Shard r with PREFILL windows whose first reward 1000 r + row shows the ring and row a folded transition came from; terminals at
    every position of the window (and none) over any Ln + 1 rows."""
    rb = d.ReplayBufferNStep(opt, seed=100 + r)
    rs = np.random.RandomState(r)
    n, Ln = PREFILL, LN
    rews = rs.randn(n, Ln).astype(np.float32)
    rews[:, 0] = 1000.0 * r + np.arange(n)
    done = np.zeros((n, Ln), np.float32)
    pos = np.arange(n) % (Ln + 1)
    rows = np.nonzero(pos < Ln)[0]
    done[rows, pos[rows]] = 1.0
    rb.store_batch(*(torch.from_numpy(x).cuda() for x in (rs.randn(n, Ln + 1, 8).astype(np.float32), rs.uniform(-1, 1, (n, Ln, 2)).astype(np.float32), rews, done)))
    return rb


def _folded_rows(rb, idx, gamma):
    """The packed batch [obs1 | obs2 | acts | rews | done] the ring's folded sampler hands out for indices idx: fold32 of its windows."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _nstep_fold as nf
    g = rb.rings()
    win = {k: g["buffer_" + k[0]].cpu().numpy()[idx] for k in ("obs", "acts", "rews", "done")}
    f = nf.fold32(win, gamma)
    return np.concatenate([np.ascontiguousarray(f[k]).reshape(-1) for k in NAMES])


def _gpu_worker(rank, world, port, q, num_learners):
    try:
        sys.path.insert(0, ROOT)
        os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                          DDRL_DIST_BACKEND="gloo")
        import distributed_drl_amd as d
        import torch.distributed as dist
        from distributed_drl_amd import _lib, comm, partition
        from distributed_drl_amd.agent import HyperParameters, Learner
        from distributed_drl_amd.workers import RolloutDeviceNStep
        r, w, _ = comm.init_from_env()
        torch.cuda.set_device(0)
        _lib.require_gpu()
        roles = partition.Roles(w, r, num_learners=num_learners)
        opt = HyperParameters()
        opt.num_envs, opt.batch_size, opt.seed, opt.start_steps, opt.max_ep_len, opt.push_freq = N_ENVS, BATCH, 5, -1, 50, 6
        opt.Ln, opt.buffer_size, opt.num_buffers = LN, CAP, len(roles.shard_owner)
        B, nb = opt.batch_size, opt.num_buffers
        make = (lambda: _prefilled_shard(d, opt, r), lambda rb: RolloutDeviceNStep(None, rb, opt, worker_index=r), lambda: Learner(opt, job="learner", index=0))
        with pytest.raises(ValueError, match="free-running"):      # out of scope on window rings: refused by name, before any collective
            partition.PartitionedRun(opt, roles, *make, seed=9, updates_per_graph=0, free_steps=3, nstep=True)
        run = partition.PartitionedRun(opt, roles, *make, seed=9, updates_per_graph=0, nstep=True)
        n_pi = 8 * 400 + 400 + 400 * 300 + 300 + 2 * (300 * 2 + 2)
        pi0 = run.bcast.buf[:n_pi].clone()
        if run.roll is not None:   # the learner's initial weights reached every rollout rank's actor
            assert isinstance(run.rb, d.ReplayBufferNStep)
            assert torch.equal(run.roll.actor.get_weights_flat(), pi0)
        if run.learner is not None:
            assert isinstance(run.feed_ring, d.ReplayBufferNStep) and (run.rb is not None or run.feed_ring.max_size == 1)
        sched = partition.Schedule(roles, seed=9)
        plans = [sched.next() for _ in range(N_UPD)]
        # What every ring must hand out, from NumPy's own legacy stream: the ring's sampler is np.random.seed(100 + r); the masked window
        # store keeps the row count on the device, so `size` is read back after the step (its env step is stored before its updates);
        # a shard serves learner 0's batch before learner 1's.
        rs = np.random.RandomState(100 + r)
        handed, trained, sizes = [], [], []
        for u in range(N_UPD):   # one update per step() call so that the batch of every update can be inspected
            run.step(1)
            torch.cuda.synchronize()
            if run.rb is not None:
                samples, steps, size = run.rb.get_counts()
                sizes.append(size)
                assert steps == size * nb and PREFILL <= size <= PREFILL + N_ENVS * (u + 1)
                for l, owner in plans[u]:
                    if owner == r:
                        handed.append((u, l, _folded_rows(run.rb, rs.randint(0, size, B), opt.gamma)))
            if run.learner is not None:   # the device loop gathered update u's batch into input set u & 1; data-parallel: the set just trained on
                v = run.learner.input_batch(u & 1 if run.loop is not None else run.learner._dp_last_set)
                trained.append(torch.cat([v[k].reshape(-1) for k in NAMES]).cpu().numpy().copy())
        everything = [None] * w
        dist.all_gather_object(everything, handed)
        if roles.is_learner:
            # update u trained on exactly the fold of the windows the scheduled owner's ring handed out for it (bit for bit; never a mix:
            # rews of an Ln-row without a terminal in front still carry 1000 owner + row in their first term, checked through the fold)
            want = {(u, l): rows for per_rank in everything for (u, l, rows) in per_rank}
            for u in range(N_UPD):
                assert trained[u].tobytes() == want[(u, r)].tobytes(), "update %d of learner %d" % (u, r)
            assert run.learner.opt_steps() == (N_UPD, N_UPD)
            mine = [dict(p)[r] for p in plans]
            assert run.stats["local_batches"] == mine.count(r) and run.stats["remote_batches"] == N_UPD - mine.count(r)
            if num_learners is None:
                assert 0 < mine.count(r) < N_UPD                   # config 3's roles: local AND remote entries in the run
        if run.rb is not None:
            # the shard's sampler advanced num_buffers per batch it served; the rollout's windows arrived (64 per step once the queues are full)
            served = sum(1 for p in plans for _, owner in p if owner == r)
            samples, steps, size = run.rb.get_counts()
            assert samples == served * nb and size == sizes[-1] and size > PREFILL
            assert run.stats["sent_batches"] == sum(1 for p in plans for l, owner in p if owner == r and l != r)
        assert run.stats["pushes"] == 1 + N_UPD // 6
        flat = run.bcast.buf.clone()
        if roles.is_learner:
            assert not torch.equal(flat[:n_pi], pi0)
        if run.roll is not None:   # the rollout ranks run the learner's pushed policy
            assert torch.equal(run.roll.actor.get_weights_flat(), flat[:n_pi])
        if num_learners == 2:      # synchronous data parallel: both learners hold the same parameters after every update
            ws = [None] * w
            dist.all_gather_object(ws, run.learner.get_weights_flat().cpu().numpy() if roles.is_learner else None)
            np.testing.assert_array_equal(ws[0], ws[1])
        run.check()
        comm.barrier()
        q.put((rank, "ok"))
    except Exception:  # noqa
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc()))


def _spawn(world, num_learners, timeout=300):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gpu_worker, args=(r, world, port, q, num_learners)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=timeout) for _ in procs]
    for p in procs:
        p.join(60)
    assert sorted(res) == [(r, "ok") for r in range(world)], res


@pytest.mark.gpu
def test_nstep_config3_roles_two_ranks_on_one_gpu():
    """Config 3's roles on window rings: rank 0 learns (the device loop) AND rolls out, both ranks own a window shard — local
    fold-gathers and remote folded blocks in one plan."""
    _spawn(2, None)


@pytest.mark.gpu
def test_nstep_config4_roles_three_ranks_two_learners_on_one_gpu():
    """Config 4's roles at the smallest size: two dedicated data-parallel learner ranks on one-slot feed rings + one rollout rank with
    the window shard, serving both learners' folded blocks; the learners all-reduce and stay bit-identical."""
    _spawn(3, 2)
