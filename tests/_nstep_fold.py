"""The n-step fold (include/ddrl.h: "n-step fold") restated in NumPy — shared by tests/test_nstep_fold_cpu.py and
tests/test_gpu_nstep_learner.py.

A window row holds o[0..Ln], a[0..Ln-1], r[0..Ln-1], d[0..Ln-1] (algos/sac1/sac_ray.py:40-51) and folds into one transition:

    obs1 = o[0]   obs2 = o[Ln]   acts = a[0]
    c = 1; R = 0
    for k in 0 .. Ln-1:  R = R + c * r[k];  g = c * (1 - d[k]);  c = g * gamma
    rews = R      done = 1 - g

fold(..., np.float32) is what the device computes, bit for bit (NumPy rounds every product and every sum on its own, as the _rn
intrinsics of the kernel do); fold(..., np.float64) is the reference the float32 one is judged against.  The reference project's
learner never consumes the windows its n-step driver draws, so there is no reference implementation to pin this against: the fold
is this project's definition of the n-step backup."""
import numpy as np


def fold(win, gamma, dtype):
    """win = dict(obs[B, Ln+1, ...], acts[B, Ln, ...], rews[B, Ln], done[B, Ln]) -> dict(obs1, obs2, acts, rews, done) in `dtype`."""
    obs, acts = np.asarray(win["obs"], dtype), np.asarray(win["acts"], dtype)
    r, d = np.asarray(win["rews"], dtype), np.asarray(win["done"], dtype)
    B, Ln = r.shape
    one, gam = dtype(1), dtype(gamma)
    c, R, g = np.ones(B, dtype), np.zeros(B, dtype), np.ones(B, dtype)
    for k in range(Ln):
        R = R + c * r[:, k]
        g = c * (one - d[:, k])
        c = g * gam
    assert R.dtype == dtype and g.dtype == dtype
    return dict(obs1=obs[:, 0].reshape(B, -1), obs2=obs[:, Ln].reshape(B, -1), acts=acts[:, 0].reshape(B, -1), rews=R, done=one - g)


def fold32(win, gamma):
    return fold(win, np.float32(gamma), np.float32)


def fold64(win, gamma):
    return fold(win, gamma, np.float64)


def weighted_abs_sum(win, gamma):
    """sum_k |c_k r[k]| in float64: the scale of the rounding bound on rews."""
    r, d = np.asarray(win["rews"], np.float64), np.asarray(win["done"], np.float64)
    c, s = np.ones(r.shape[0]), np.zeros(r.shape[0])
    for k in range(r.shape[1]):
        s += np.abs(c * r[:, k])
        c = c * (1.0 - d[:, k]) * float(gamma)
    return s


def windows(rs, B, Ln, obs_dim=8, act_dim=2, terminal="some"):
    """Float32 window batch.  terminal = "some": a terminal in 40 % of the rows at a random position; "every": row b has its terminal
    at position b % (Ln + 1), where position Ln means no terminal — every position and the no-terminal case in any Ln + 1 rows;
    an int p: every row at position p (p == Ln: none)."""
    win = dict(obs=rs.randn(B, Ln + 1, obs_dim).astype(np.float32), acts=rs.uniform(-1, 1, (B, Ln, act_dim)).astype(np.float32),
               rews=rs.randn(B, Ln).astype(np.float32), done=np.zeros((B, Ln), np.float32))
    if terminal == "some":
        pos = np.where(rs.rand(B) < 0.4, rs.randint(0, Ln, B), Ln)
    elif terminal == "every":
        pos = np.arange(B) % (Ln + 1)
    else:
        pos = np.full(B, int(terminal))
    rows = np.nonzero(pos < Ln)[0]
    win["done"][rows, pos[rows]] = 1.0
    return win
