"""The walker's SAC-v update (agent.Model: policy + twin Q + V + target V) in the captured learner loop at 24 observations / 4 actions,
hidden (400, 300), batch 256: a wide Model (args.wide_model: ddrl_sacv_create_wide, five launches — k_dfwd_wide x 2, k_dg x 3) against
the same Model made by ddrl_sac1_create (at this shape the generic kernels, as before the wide path existed).

One process, one transition ring of 4096 random walker-shaped rows per learner.  Both loops (ddrl_loop_* on the Model's handle, 16
updates per graph: what workers.TrainDevice runs for a SAC1 Learner) run --warmup updates first; then --reps repetitions alternate
between the two, each timing --updates updates between a pair of HIP events on the current stream (sampler, noise and update:
everything the loop replays).  Reported per path: the median over the repetitions, the 5th / 95th percentile and the minimum, in
microseconds per update; then the difference of the medians beside the spread between repetitions of the generic path (p95 - p5).

    python tools/sacv_wide_probe.py [--reps 15] [--updates 1600] [--warmup 320] [--out profiles/sacv_wide_time.txt]"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OBS, ACT, BATCH, ROWS, PER_GRAPH = 24, 4, 256, 4096, 16


class Args:
    """example/dsac.py's args for Model(args), at the defaults of agent.HyperParameters."""
    obs_dim, act_dim, ac_kwargs = OBS, ACT, dict(hidden_sizes=[400, 300])
    gamma, polyak, lr, alpha, batch_size, seed, max_ep_len, act_scale = 0.997, 0.995, 5e-5, 0.1, BATCH, 0, 1000, 1.0

    def __init__(self, wide):
        self.wide_model = wide


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=15)
    p.add_argument("--updates", type=int, default=1600)
    p.add_argument("--warmup", type=int, default=320)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import numpy as np
    import torch
    import distributed_drl_amd as d
    from distributed_drl_amd import _lib
    from distributed_drl_amd.agent import Model
    arch = _lib.require_gpu()
    lib = _lib.load()
    rs = np.random.RandomState(0)
    data = [rs.randn(ROWS, OBS).astype(np.float32), rs.uniform(-1, 1, (ROWS, ACT)).astype(np.float32), rs.randn(ROWS).astype(np.float32),
            rs.randn(ROWS, OBS).astype(np.float32), (rs.rand(ROWS) < 0.05).astype(np.float32)]

    def loop(wide):
        model = Model(Args(wide))
        assert lib.ddrl_sac1_is_wide(model._h) == (1 if wide else 0) and lib.ddrl_sac1_is_fused(model._h) == (1 if wide else 0)
        rb = d.ReplayBufferSAC1(OBS, ACT, ROWS, seed=11)
        rb.store_batch(*(torch.from_numpy(x).cuda() for x in data))
        h = ctypes.c_void_p()
        _lib.check(lib.ddrl_loop_create(ctypes.byref(h), model._h, rb._h, PER_GRAPH, 1))
        return model, rb, h

    def run(h, n):
        _lib.check(lib.ddrl_loop_run(h, n, _lib.stream_ptr()))
    loops = (("generic  ddrl_sac1_create (DDRL_SAC_V)", loop(False)), ("wide     ddrl_sacv_create_wide, five launches", loop(True)))
    for _, (_, _, h) in loops:
        run(h, a.warmup)
    torch.cuda.synchronize()
    us = [[], []]
    for _ in range(a.reps):
        for j, (_, (_, _, h)) in enumerate(loops):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(h, a.updates)
            e1.record()
            e1.synchronize()
            us[j].append(e0.elapsed_time(e1) * 1e3 / a.updates)
    lines = ["sacv_wide_probe on %s: SAC-v, %d observations / %d actions, hidden (400, 300), batch %d; captured loop, %d updates per graph; %d alternating "
             "repetitions of %d updates behind %d warm-up updates, HIP events around every repetition" % (arch, OBS, ACT, BATCH, PER_GRAPH, a.reps, a.updates, a.warmup)]
    med, spread = [], []
    for j, (name, (model, _, h)) in enumerate(loops):
        u = np.array(us[j])
        med.append(float(np.median(u)))
        spread.append(float(np.percentile(u, 95) - np.percentile(u, 5)))
        lines.append("%-46s median %7.2f us per update   p5 %7.2f   p95 %7.2f   min %7.2f" % (name, med[-1], np.percentile(u, 5), np.percentile(u, 95), u.min()))
        assert model.opt_steps()[0] == a.warmup + a.reps * a.updates
        assert np.isfinite(model.get_weights_flat().cpu().numpy()).all()
        lib.ddrl_loop_destroy(h)
    diff = med[0] - med[1]
    lines.append("generic - wide = %.2f us per update (wide / generic = %.2f); spread of the generic path between repetitions %.2f us: the wide path is %s" %
                 (diff, med[1] / med[0], spread[0], "faster" if diff > spread[0] else "NOT faster by more than the spread"))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
