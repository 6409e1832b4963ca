"""Generate tests/golden/walker_hardcore.npz: the Hardcore walker's oracle (tests/walker_hardcore_oracle.py) at gym's 180 velocity /
60 position iterations from CRAFTED starts at obstacles — eight classes of tests/_walker_hardcore_scenarios.py (a foot on a stump top,
on the ground against a stump side, against each pit wall, on a stair tread up and down, the hull's nose inside a stump, standing before
a stump) — 8 envs, STEPS steps under recorded random actions, with a time limit inside the run so that every env regenerates its
terrain once.  Data only: seed, iteration counts, the start block, per step the actions, obs2, rew, done, next_obs and ended, and the
final state block.

    python tools/gen_walker_hardcore_golden.py [--out tests/golden/walker_hardcore.npz]

CPU only (NumPy); under a minute.  tests/test_walker_hardcore_cpu.py regenerates the first steps and compares bit for bit;
tests/test_gpu_walker_hardcore_scenarios.py replays the recorded actions through the HIP kernel.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SEED, N_ENVS, MAX_EP_LEN, VIT, PIT, STEPS = 23, 8, 30, 180, 60, 40
KEYS = ("actions", "obs2", "rew", "done", "next_obs", "ended")
PICK = ("stump_top", "stump_left_and_ground", "pit_left_wall", "pit_right_wall", "stair_up_tread", "stair_down_tread", "hull_in_box",
        "lidar_stump")


def run(steps=STEPS):
    """-> dict of arrays."""
    import _walker_hardcore_scenarios as sc
    from walker_hardcore_oracle import WalkerHardcoreOracle
    assert sc.SEED == SEED
    S, _ = sc.build()
    start = np.ascontiguousarray(S[:, [sc.CLASSES.index(c) for c in PICK]])
    ora = WalkerHardcoreOracle(N_ENVS, seed=SEED, max_ep_len=MAX_EP_LEN, velocity_iterations=VIT, position_iterations=PIT)
    ora.S[:] = start
    rs = np.random.RandomState(SEED)
    rec = {k: [] for k in KEYS}
    for _ in range(steps):
        a = rs.uniform(-1.0, 1.0, (N_ENVS, 4)).astype(np.float32)
        out = ora.step(a)
        for k, v in zip(KEYS, (a,) + tuple(out)):
            rec[k].append(np.array(v))
    out = {k: np.stack(v) for k, v in rec.items()}
    out.update(seed=np.int64(SEED), n_envs=np.int64(N_ENVS), max_ep_len=np.int64(MAX_EP_LEN), velocity_iterations=np.int64(VIT),
               position_iterations=np.int64(PIT), start_state=start, final_state=ora.S.copy())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "walker_hardcore.npz"))
    args = ap.parse_args()
    g = run()
    np.savez_compressed(args.out, **g)
    print("%s: %d bytes, %d steps, %d episode ends" % (args.out, os.path.getsize(args.out), g["rew"].shape[0], int(g["ended"].sum())))


if __name__ == "__main__":
    main()
