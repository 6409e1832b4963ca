"""ORACLE — TEST INFRASTRUCTURE ONLY.

`Wrapper.step` (algos/sac1/hyperparams.py:123-134) and the n-step rollout's bookkeeping (algos/sac1/sac_ray.py:212-258) on the BIPEDAL
WALKER: tests/lander3_wrapped_oracle.py restated line for line over WalkerOracle._physics / _rng / reset, statistics included, with 4
actions and 24 observations (the noise sizes hard-coded in the reference's Wrapper are this env's).  csrc/walker.hip
(k_walker_step_wrapped) mirrors it statement by statement.  Like the model itself (tests/walker_oracle.py) this is not pinned against gym.

`_physics` returns an observation per call and the Wrapper keeps only the last; `obs()` is a pure function of the state, so a kernel may
compute it once behind the last sub-step.

NOISE DRAWS.  The walker's `_rng(step, j)` hashes `step * 16 + j` (mod 2^32) under a seed of (seed, env id, episode):
    action             _rng(st0, 2 + c), c < 4                       inputs 16 st0 + 2 .. 16 st0 + 5     st0 = PSTEP before the repeat loop
    observation        _rng(OBS_NOISE_STEP0 + 2 st1, k), k < 24      inputs 0x40000000 + 32 st1 + k      st1 = PSTEP behind it
    reset observation  _rng(RESET_NOISE_STREAM, k), k < 24           inputs 0xFFFFFEF0 + k
A wrapped step draws 28 numbers, more than the 16 indices of one PSTEP value.  The one-body and articulated Wrappers' layout carried
over (observation noise at _rng(st1, 6 + k), inputs 16 st1 + 6 .. 16 st1 + 29) COLLIDES: the block reaches into the sixteen of PSTEP
st1 + 1, and an early break — `d` at sub-step 0 of the next wrapped step — draws its observation noise at st1 + 1 while the episode's
seed still holds (EPI moves behind the draw): the inputs 16 st1 + 22 .. 29 are drawn twice.  tests/test_walker_wrapped_cpu.py met this
on a live run.  So the observation noise has a range of its own with 32 inputs per PSTEP value, and no two draws of an episode share
an input (that test verifies it on live runs at repeat 1, 2 and 3, with limits and early ends):
  * walker physics draws nothing per step (only _build draws: the terrain and the initial force, under RESET_STREAM);
  * every wrapped step of an episode advances PSTEP by at least 1, so its st0 and its st1 differ from every earlier step's: the action
    inputs 16 st0 + 2 .. 5 and the observation inputs 0x40000000 + 32 st1 + 0 .. 23 are each step's own;
  * PSTEP < 2^23 (a float32 count, back to 0 at every reset), so the action inputs stay below 0x08000000 and the observation inputs
    inside [0x40000000, 0x50000000): the two ranges and the two reset ranges below never meet;
  * with repeat == 1 no observation noise is drawn at all;
  * an episode's end moves EPI, which reseeds the stream: the reset noise and the new terrain belong to the NEW episode;
  * the reset-noise inputs 0xFFFFFEF0 + k, k < 24, overlap the terrain's 0xFFFFFF00 + i (RESET_STREAM = 0xFFFFFFF0) only at i <= 7; the
    terrain draws only i > 20 and the initial force i = 200.
"""
import numpy as np

from walker_oracle import ACT, EPI, EPLEN, EPRET, OBS, PSTEP, F, WalkerOracle

RESET_NOISE_STREAM = 0xFFFFFFEF   # the value csrc/lander.hip and csrc/rollout3_nstep.hip use for the Wrapper's reset-observation noise
ACT_J0 = 2                        # first RNG index of the action noise
OBS_NOISE_STEP0 = 0x04000000      # the observation noise of PSTEP st1 is drawn at "step" OBS_NOISE_STEP0 + 2 st1, indices 0..23


class WalkerWrappedOracle(WalkerOracle):
    def step_wrapped(self, act, act_noise, obs_noise, reward_scale, repeat, limit_steps):
        S = self.S
        act = np.asarray(act, dtype=F).reshape(self.n, ACT)
        st0 = S[PSTEP].astype(np.uint32)
        a = np.empty_like(act)
        for c in range(ACT):
            a[:, c] = act[:, c] + F(act_noise) * (F(-2.0) * self._rng(st0, ACT_J0 + c) + F(1.0))
        act[...] = a   # hyperparams.py:124 `action += ...` mutates the caller's array (a float32 ndarray is updated in place)
        r = np.zeros(self.n, F)
        rew = np.zeros(self.n, F)
        obs = np.zeros((self.n, OBS), F)
        done = np.zeros(self.n, bool)
        noisy = np.ones(self.n, bool)
        active = np.ones(self.n, bool)
        self.last_break = np.full(self.n, -1, np.int64)   # RECORDING: the sub-step at which `d` broke the loop, -1: it did not
        for k in range(int(repeat)):
            if not active.any():
                break
            keep = S.copy()
            rk, dk, ok = self._physics(a)
            S[:, ~active] = keep[:, ~active]
            r = np.where(active, (r + rk).astype(F), r)
            obs[active] = ok[active]
            done = np.where(active, dk, done)
            brk_done = active & dk & (repeat != 1)
            self.last_break = np.where(brk_done, k, self.last_break)
            rew = np.where(brk_done, F(0.0), rew)
            brk_one = active & ~brk_done & (repeat == 1)
            rew = np.where(brk_one, r, rew)
            noisy = noisy & ~brk_one
            cont = active & ~brk_done & ~brk_one
            rew = np.where(cont, (F(reward_scale) * r).astype(F), rew)
            active = cont
        self.last_wrapper_state = S.copy()                # RECORDING: the block behind the repeat loop, before bookkeeping and reset
        st1 = np.uint32(OBS_NOISE_STEP0) + np.uint32(2) * S[PSTEP].astype(np.uint32)
        for j in range(OBS):
            nz = (obs[:, j] + F(obs_noise) * (F(-2.0) * self._rng(st1, j) + F(1.0))).astype(F)
            obs[:, j] = np.where(noisy, nz, obs[:, j])
        S[EPLEN] = S[EPLEN] + F(1.0)
        S[EPRET] = (S[EPRET] + rew).astype(F)
        ended = done | (S[EPLEN] >= F(limit_steps))
        self.episodes += int(ended.sum())
        self.ret_sum += float(S[EPRET][ended].astype(np.float64).sum())
        self.len_sum += int(S[EPLEN][ended].sum())
        S[EPI] = np.where(ended, S[EPI] + F(1.0), S[EPI]).astype(F)
        next_obs = obs.copy()
        if ended.any():
            ro = self.reset(ended)
            for j in range(OBS):
                nz = (ro[:, j] + F(obs_noise) * (F(-2.0) * self._rng(RESET_NOISE_STREAM, j) + F(1.0))).astype(F)
                next_obs[:, j] = np.where(ended, nz, next_obs[:, j])
        return obs, rew.astype(F), done.astype(F), next_obs, ended.astype(np.uint8)
