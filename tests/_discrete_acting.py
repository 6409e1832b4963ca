"""The discrete actors' selection rules and gym's discrete lander action table in NumPy: the oracle half of
tests/test_discrete_acting_cpu.py and tests/test_gpu_discrete_rollout.py.

SELECTION (ddrl_dqn_act, csrc/dqn_select.h).  Row i owns two uniforms of the counter generator, u0 = U(seed, ctr + 2 i) and
u1 = U(seed, ctr + 2 i + 1): elements of oracle/noise_oracle.uniform_fill(lo=0, hi=1).
    Double-DQN (algos/dqn/actor_learner.py:194-201)   u0 < greedy_prob: np.argmax (first maximum); else min(int(floor(u1 * A)), A - 1)
    SQN deterministic                                 np.argmax
    SQN sampling (algos/sqn/core.py:30-42)            inverse CDF in float32: p_k = exp((q_k - max q) / alpha), cumulative sums in index
                                                      order, the smallest k with u0 * total < cum_k, else the last index
TABLE (ddrl_env_step_discrete).  index = int(value) clamped to [0, 3] -> (a0, a1): noop (0, 0), left (0, -1), main (1, 0), right (0, +1)."""
import numpy as np

from oracle import noise_oracle as no

F = np.float32
ACTION_TABLE = np.array([[0.0, 0.0], [0.0, -1.0], [1.0, 0.0], [0.0, 1.0]], np.float32)


def table_actions(idx):
    """[n] indices (any float / int values) -> [n, 2] continuous actions of the table, with the clamp."""
    k = np.clip(np.trunc(np.asarray(idx, np.float64)), 0, 3).astype(np.int64)
    return ACTION_TABLE[k]


def uniforms(seed, ctr, n):
    """(u0 [n], u1 [n]) of rows 0 .. n-1 of a call at (seed, ctr)."""
    u = no.uniform_fill(2 * int(n), 0.0, 1.0, int(seed), int(ctr))
    return u[0::2].astype(F), u[1::2].astype(F)


def first_max(q):
    return np.argmax(np.asarray(q, F), axis=1)


def select_ddqn(q, greedy_prob, u0, u1):
    q = np.asarray(q, F)
    A = q.shape[1]
    rnd = np.minimum(np.floor(np.asarray(u1, F) * F(A)).astype(np.int64), A - 1)
    return np.where(np.asarray(u0, F) < F(greedy_prob), first_max(q), rnd)


def select_sqn(q, alpha, u0):
    """The float32 inverse CDF, operation for operation."""
    q = np.asarray(q, F)
    n, A = q.shape
    p = np.exp(((q - q.max(axis=1, keepdims=True)) / F(alpha)).astype(F)).astype(F)
    cum = np.zeros((n, A), F)
    run = np.zeros(n, F)
    for k in range(A):
        run = (run + p[:, k]).astype(F)
        cum[:, k] = run
    t = (np.asarray(u0, F) * run).astype(F)
    below = t[:, None] < cum
    return np.where(below.any(axis=1), np.argmax(below, axis=1), A - 1)


def select(q, family, alpha, greedy_prob, u0, u1, deterministic=False):
    if deterministic:
        return first_max(q)
    return select_sqn(q, alpha, u0) if family == "sqn" else select_ddqn(q, greedy_prob, u0, u1)


def sqn_boundaries64(q, alpha, u0):
    """(pick from the float64 inverse CDF of the float32 q rows, rows whose u0 * total lies within 1e-5 relative of a cumulative
    boundary: the only rows a float32 evaluation of the same rule may legitimately place one index off)."""
    q = np.asarray(q, F).astype(np.float64)
    A = q.shape[1]
    p = np.exp((q - q.max(axis=1, keepdims=True)) / float(F(alpha)))
    cum = np.cumsum(p, axis=1)
    t = np.asarray(u0, F).astype(np.float64) * cum[:, -1]
    below = t[:, None] < cum
    pick = np.where(below.any(axis=1), np.argmax(below, axis=1), A - 1)
    near = (np.abs(t[:, None] - cum) <= 1e-5 * np.abs(cum)).any(axis=1)
    return pick, near
