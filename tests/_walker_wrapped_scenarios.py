"""TEST INFRASTRUCTURE: crafted starts for the walker's WRAPPED step (tests/walker_wrapped_oracle.py, csrc/walker.hip) and the
census of the Wrapper's branches a run reaches.

`build()` -> (state block [286, N] float32, actions [N, 4] float32): the 96 envs of tests/_walker_scenarios.build() with their step-0
actions, followed by COPIES copies each of that module's `x_negative` stance (hull moving left at 4 m/s, 0.3 above the pad, zero action)
at the start x of BREAK_X.  The hull loses 0.08 m per physics step, so with zero action at 8 / 3 iterations `d` (x < 0) arrives at
sub-step 0, 1, 2, 3 for x = 0.04, 0.10, 0.18, 0.26: with repeat = 3 that is a break at k = 0, 1, 2 of the first wrapped step and at k = 0
of the second; with repeat = 2 a break at k = 0, 1, 0, 1.  Every env starts at EPLEN = 3, so with LIMIT = 5 the envs that are still in
their first episode at the second wrapped step end it there on the limit, without `d`.

`trajectory(repeat, vit, pit)` runs the oracle once (STEPS wrapped steps with the noise of NOISE) and is shared by
tests/test_walker_wrapped_cpu.py (the census floor: every branch the GPU test relies on IS reached) and tests/test_gpu_walker_wrapped.py
(the kernel's parity on the same run)."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _walker_scenarios as ws   # noqa: E402
import walker_oracle as W   # noqa: E402
from walker_wrapped_oracle import WalkerWrappedOracle   # noqa: E402

F = np.float32
SEED = ws.SEED
BREAK_X = (0.04, 0.10, 0.18, 0.26)
COPIES = 3
N = ws.N + COPIES * len(BREAK_X)
STEPS, LIMIT = 2, 5
NOISE = dict(act_noise=0.3, obs_noise=0.01, reward_scale=5.0)


def build():
    S0, act0 = ws.build()
    S = np.zeros((W.NFW, N), F)
    act = np.zeros((N, 4), F)
    S[:, :ws.N] = S0
    act[:ws.N] = act0[0]
    e = ws.N
    for x in BREAK_X:
        for _ in range(COPIES):
            p = ws.lift(ws.pose(x, 6.0, 0.0, 0.05, -0.15, 0.05, -0.15, vx=-4.0), ws.FLAT, 0.3)   # _walker_scenarios' x_negative stance
            for f, v in p.items():
                S[f, e] = F(v)
            S[W.T0:, e] = ws.FLAT.astype(F)
            S[W.HASP, e], S[W.EPLEN, e], S[W.PSTEP, e] = 1.0, 3.0, 3.0
            S[W.PREV, e] = F(130.0 * p[W.PX] / 30.0 - 5.0 * abs(p[W.ANG]))
            e += 1
    return S, act


def census_of(ora, outs, repeat, limit, counts=None):
    """Add the last wrapped step's branches (envs per branch) to `counts`; `ora` has just returned `outs` from step_wrapped."""
    c = {} if counts is None else counts
    add = lambda k, m: c.__setitem__(k, c.get(k, 0) + int(np.sum(m)))   # noqa: E731
    done, ended = outs[2] > 0, outs[4] > 0
    eplen = ora.last_wrapper_state[W.EPLEN] + F(1.0)
    for k in range(3):
        add("break_at_%d" % k, ora.last_break == k)
    add("ran_out", (ora.last_break < 0) & (repeat != 1))
    add("bare_step", np.full(ora.n, repeat == 1))
    add("limit_without_d", ended & ~done)
    add("d_before_limit", done & (eplen < F(limit)))
    return c


@functools.lru_cache(maxsize=None)
def trajectory(repeat, vit, pit, noisy=True):
    """-> (start block, per-step list of (action in, outputs, action out, block after, block behind the repeat loop, last_break),
    census, stats)."""
    S, act = build()
    ora = WalkerWrappedOracle(N, seed=SEED, max_ep_len=1 << 23, velocity_iterations=vit, position_iterations=pit)
    ora.S[:] = S
    kw = NOISE if noisy else dict(act_noise=0.0, obs_noise=0.0, reward_scale=1.0)
    steps, census = [], {}
    for t in range(STEPS):
        a = act.copy()
        outs = [np.array(x) for x in ora.step_wrapped(a, repeat=repeat, limit_steps=LIMIT, **kw)]
        census_of(ora, outs, repeat, LIMIT, census)
        steps.append((act.copy(), outs, a, ora.S.copy(), ora.last_wrapper_state.copy(), ora.last_break.copy()))
    return S, steps, census, ora.stats()
