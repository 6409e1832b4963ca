"""Double-DQN learner / actor of the multi-node driver (algos/dqn/actor_learner.py:19-107, 175-201;
network algos/dqn/core.py:40-50) on the MI355X: `Learner(opt, job)` with set_weights / get_weights /
train(batch, cnt), `Actor(opt, job)` with get_action(o, deterministic) — same names and argument meaning — and the batched
get_actions(obs) of the device rollout (workers.RolloutDeviceDQN).
`opt` carries obs_dim, act_dim (number of discrete actions), hidden_size, gamma, lr, polyak, batch_size, seed
(algos/dqn/hyperparams.py:26-60)."""
import ctypes
import math

import numpy as np
import torch

from . import _lib


class HyperParameters:
    """Value bag of algos/dqn/hyperparams.py:10-75 (algos/sqn/hyperparams.py adds `alpha`): what the DQN / SQN driver, buffers, server and
    agents read.  `env` (anything with observation_space.shape and action_space.n) or explicit obs_dim / act_dim."""

    def __init__(self, env=None, env_name="Trading", exp_name="ddqn-trading", num_nodes=1, num_workers=6, a_l_ratio=10, weights_file="",
                 obs_dim=None, act_dim=None):
        import datetime
        import os
        self.exp_name, self.env_name, self.model = exp_name, env_name, "mlp"
        self.num_nodes, self.num_workers, self.num_learners = num_nodes, num_workers, 1
        self.push_freq = 100
        self.gamma = 0.99
        self.alpha = 0.1                  # sqn: the softmax policy's temperature (must be > 0)
        self.a_l_ratio, self.weights_file = a_l_ratio, weights_file
        self.recover = False
        self.checkpoint_freq = 21600      # seconds (6 h)
        self.hidden_size = [400, 300]
        self.obs_dim = int(env.observation_space.shape[0] if obs_dim is None else obs_dim)
        self.act_dim = int(env.action_space.n if act_dim is None else act_dim)
        self.obs_shape, self.act_shape = (self.obs_dim,), ()
        self.num_buffers = self.num_workers // 25 + 1
        self.buffer_size = int(1e6) // self.num_buffers
        self.start_steps = int(1e4) // self.num_buffers
        if self.weights_file:
            self.start_steps = self.buffer_size
        self.lr, self.polyak, self.batch_size = 1e-3, 0.995, 128
        self.Ln, self.save_freq, self.seed = 1, 1, 0
        root = os.getcwd()                # (the reference: the directory above its own source file)
        self.summary_dir, self.save_dir, self.save_interval = root + "/tboard_ray", root + "/" + exp_name, int(5e5)
        self.log_dir = "%s/%s-workers_num:%s%%%s%s-%s" % (self.summary_dir, datetime.datetime.now(), num_workers, a_l_ratio, env_name, exp_name)


def param_specs(obs_dim, n_actions, hidden_size, nets=("q1",)):
    """(name, shape) in TF variable-creation order: tf.make_template('q1', vf_mlp) [, 'q2'] under scope 'main'."""
    h1, h2 = hidden_size
    specs = []
    for q in nets:
        specs += [("main/%s/dense/kernel" % q, (obs_dim, h1)), ("main/%s/dense/bias" % q, (h1,)),
                  ("main/%s/dense_1/kernel" % q, (h1, h2)), ("main/%s/dense_1/bias" % q, (h2,)),
                  ("main/%s/dense_2/kernel" % q, (h2, n_actions)), ("main/%s/dense_2/bias" % q, (n_actions,))]
    return specs


def glorot_init(specs, seed):
    rs = np.random.RandomState(seed)
    parts = []
    for name, shape in specs:
        if name.endswith("kernel"):
            lim = math.sqrt(6.0 / (shape[0] + shape[1]))
            parts.append(rs.uniform(-lim, lim, size=shape).astype(np.float32).reshape(-1))
        else:
            parts.append(np.zeros(int(np.prod(shape)), np.float32))
    return np.concatenate(parts)


class Learner:
    NETS = ("q1",)
    VARIANT = 0  # DDRL_DDQN

    def __init__(self, opt, job="learner", batch=None):
        _lib.require_gpu()
        self._lib = _lib.load()
        self.opt = opt
        self.device = torch.device("cuda", torch.cuda.current_device())
        hs = list(opt.hidden_size)
        assert len(hs) == 2, "two hidden layers (algos/dqn/hyperparams.py:37)"
        self.specs = param_specs(opt.obs_dim, opt.act_dim, hs, self.NETS)
        self.keys = [n for n, _ in self.specs]
        self.table, off = {}, 0
        for n, s in self.specs:
            cnt = int(np.prod(s))
            self.table[n] = (off, cnt, s)
            off += cnt
        self.n_params = off
        self.cfg = _lib.DqnConfig(opt.obs_dim, opt.act_dim, hs[0], hs[1], int(opt.batch_size if batch is None else batch),
                                  gamma=opt.gamma, lr=opt.lr, polyak=opt.polyak, variant=self.VARIANT,
                                  alpha=float(getattr(opt, "alpha", 0.1)))
        h = ctypes.c_void_p()
        _lib.check(self._lib.ddrl_dqn_create(ctypes.byref(h), self.device.index, ctypes.byref(self.cfg)))
        self._h = h
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._flat_set(torch.from_numpy(glorot_init(self.specs, getattr(opt, "seed", 0))).to(self.device))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.ddrl_dqn_destroy(h)

    def _flat_set(self, flat):
        flat = flat.to(device=self.device, dtype=torch.float32).contiguous()
        _lib.check(self._lib.ddrl_dqn_set_weights(self._h, _lib.dptr(flat), _lib.stream_ptr()))

    def export(self, which=_lib.SAC1_MAIN):
        flat = torch.empty(self.n_params, dtype=torch.float32, device=self.device)
        _lib.check(self._lib.ddrl_dqn_export(self._h, which, _lib.dptr(flat), _lib.stream_ptr()))
        return flat

    def import_(self, which, flat):
        flat = flat.to(device=self.device, dtype=torch.float32).contiguous()
        assert flat.numel() == self.n_params
        _lib.check(self._lib.ddrl_dqn_import(self._h, which, _lib.dptr(flat), _lib.stream_ptr()))

    def get_weights(self):
        flat = self.export().cpu().numpy()
        return list(self.keys), [flat[o:o + n].reshape(s).copy() for (o, n, s) in (self.table[k] for k in self.keys)]

    def set_weights(self, variable_names, weights):
        # every variable given: nothing of the current parameters survives, so nothing is read back (a learner whose stream-K combine
        # timed out refuses to export — fresh parameters are exactly what it is waiting for)
        full = set(self.keys) <= set(variable_names)
        flat = torch.empty(self.n_params, dtype=torch.float32, device=self.device) if full else self.export()
        for k, w in zip(variable_names, weights):
            if k not in self.table:
                continue
            o, n, _ = self.table[k]
            w = w if torch.is_tensor(w) else torch.from_numpy(np.asarray(w, np.float32))
            flat[o:o + n] = w.to(self.device).reshape(-1)
        self._flat_set(flat)

    def _dev(self, x, shape):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        return t.to(device=self.device, dtype=torch.float32).contiguous().reshape(shape)

    def train(self, batch, cnt=0, return_outputs=False):
        """sess.run([q_loss, q, train_value_op, target_update]) (actor_learner.py:110-119)."""
        B = self.cfg.batch
        x, x2 = self._dev(batch["obs1"], (B, -1)), self._dev(batch["obs2"], (B, -1))
        a, r, d = self._dev(batch["acts"], (B,)), self._dev(batch["rews"], (B,)), self._dev(batch["done"], (B,))
        q = torch.empty(B, self.cfg.n_actions, dtype=torch.float32, device=self.device) if return_outputs else None
        _lib.check(self._lib.ddrl_dqn_step(self._h, _lib.dptr(x), _lib.dptr(x2), _lib.dptr(a), _lib.dptr(r), _lib.dptr(d),
                                           _lib.dptr(self.loss), _lib.dptr(q), _lib.stream_ptr()))
        if return_outputs:
            return self.loss, q
        return None

    def train_from(self, replay_buffer, cnt=0, return_outputs=False, with_indices=False):
        """One iteration of the learner's loop — `agent.train(replay_buffer.sample_batch(), cnt)` (algos/dqn/train.py:66-76) — with the
        layer-1 forward reading its observation rows straight out of the device ring (ddrl_dqn_step_ring): same index stream, same
        counters, bit-identical results, a quarter of the batch materialised.  Runs sample_batch_device + train itself where the fused
        call does not apply (observations narrower than 1024, a compact ring whose obs_dim is not a multiple of 16, a ring with one
        compact and one float32 observation array: DDRL_ERR_UNSUPPORTED) — and on EVERY compact (uint8) ring: ddrl_dqn_step_ring does
        take a compact ring (the forward stages the rows' bytes and converts them on chip, no float32 batch is written, bit-identical:
        tests/test_gpu_compact_ring_learner.py), but at config 5's shape it measured 565 us per iteration against the two calls' 559
        (profiles/compact_ring_learner_before_after.txt: the byte forward is no faster than the float32 one, and the batch forward
        beats both forwards on scattered ring rows by more than the 32 us gather costs), so this method keeps the faster form there."""
        B = self.cfg.batch
        q = torch.empty(B, self.cfg.n_actions, dtype=torch.float32, device=self.device) if return_outputs else None
        idx = torch.empty(B, dtype=torch.int64, device=self.device) if with_indices else None
        rc = _lib.DDRL_ERR_UNSUPPORTED
        if not getattr(replay_buffer, "compact_obs", False):
            rc = self._lib.ddrl_dqn_step_ring(self._h, replay_buffer._h, _lib.dptr(self.loss), _lib.dptr(q), _lib.dptr(idx), _lib.stream_ptr())
        if rc == _lib.DDRL_ERR_UNSUPPORTED:
            b = replay_buffer.sample_batch_device(B, with_indices=with_indices)
            out = self.train(b, cnt, return_outputs=return_outputs)
            return (out + (b["idxs"],)) if (return_outputs and with_indices) else out
        _lib.check(rc)
        if return_outputs:
            return (self.loss, q, idx) if with_indices else (self.loss, q)
        return None

    def stage_times(self, batch, reps=10):
        """Mean milliseconds per launch group of `reps` updates on `batch` (ddrl_dqn_step_timed; bench.py's config-5 roofline)."""
        B = self.cfg.batch
        x, x2 = self._dev(batch["obs1"], (B, -1)), self._dev(batch["obs2"], (B, -1))
        a, r, d = self._dev(batch["acts"], (B,)), self._dev(batch["rews"], (B,)), self._dev(batch["done"], (B,))
        ms = (ctypes.c_float * _lib.DQN_STAGES)()
        _lib.check(self._lib.ddrl_dqn_step_timed(self._h, _lib.dptr(x), _lib.dptr(x2), _lib.dptr(a), _lib.dptr(r), _lib.dptr(d), int(reps), ms,
                                                 _lib.stream_ptr()))
        return [float(v) for v in ms]

    def _q_row(self, o):
        """q of ONE host observation as a NumPy row: page-locked staging both ways, one stream synchronisation."""
        st = getattr(self, "_stage_q", None)
        if st is None:
            hi, ho = torch.empty(1, self.cfg.obs_dim, dtype=torch.float32).pin_memory(), torch.empty(1, self.cfg.n_actions, dtype=torch.float32).pin_memory()
            # the q row is written straight into its page-locked row (device-side address), and a narrow observation is read straight
            # out of its own; pixel observations (the LDS-DMA layer-1 tiles) go up with a copy first
            po, pi = ctypes.c_void_p(), ctypes.c_void_p()
            _lib.check(self._lib.ddrl_host_device_pointer(ctypes.c_void_p(ho.data_ptr()), ctypes.byref(po)))
            di = None
            if self.cfg.obs_dim < 1024:
                _lib.check(self._lib.ddrl_host_device_pointer(ctypes.c_void_p(hi.data_ptr()), ctypes.byref(pi)))
            else:
                di = torch.empty(1, self.cfg.obs_dim, dtype=torch.float32, device=self.device)
            st = self._stage_q = (hi, hi.numpy(), di, pi, ho.numpy(), po, ho)
        hi, hiv, di, pi, hov, po, _ = st
        hiv[0, :] = np.asarray(o, np.float32).reshape(-1)
        if di is not None:
            di.copy_(hi, non_blocking=True)
        _lib.check(self._lib.ddrl_dqn_q(self._h, pi if di is None else _lib.dptr(di), 1, po, _lib.stream_ptr()))
        torch.cuda.current_stream().synchronize()
        return hov[0]

    def q_values(self, obs):
        obs = self._dev(obs, (-1, self.cfg.obs_dim))
        q = torch.empty(obs.shape[0], self.cfg.n_actions, dtype=torch.float32, device=self.device)
        _lib.check(self._lib.ddrl_dqn_q(self._h, _lib.dptr(obs), obs.shape[0], _lib.dptr(q), _lib.stream_ptr()))
        return q


def _get_actions(self, obs, out=None, q_out=None, deterministic=False):
    """get_action for every row of obs[n, obs_dim] (1 <= n <= max_rows) in one stream-ordered call (ddrl_dqn_act): the main network's Q
    rows (SQN: q1) from the policy forward's MFMA kernel where the shape fits it, then one action per row — the index as float32, the
    form the replay ring stores — into `out[n]`; `q_out[n, act_dim]` (optional) receives the Q rows the selection saw.  Row i draws
    its two uniforms from the object's counter stream (self._noise_seed, self._noise_ctr + 2 i [+ 1]), which advances by 2 n per call.
    Double-DQN: argmax with probability self.greedy_prob (0.97, actor_learner.py:194-201), a uniform random action otherwise;
    SQN: one draw from softmax(q1 / alpha) (core.py:30-42); deterministic=True: the first index of the row maximum.  No host
    synchronisation; nothing a later train() reads or continues from is touched."""
    obs = self._dev(obs, (-1, self.cfg.obs_dim))
    n = int(obs.shape[0])
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=self.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.numel() >= n
    assert q_out is None or (q_out.is_cuda and q_out.is_contiguous() and q_out.dtype == torch.float32 and q_out.numel() >= n * self.cfg.n_actions)
    mode = _lib.DDRL_ACT_DETERMINISTIC if deterministic else _lib.DDRL_ACT_SAMPLE
    _lib.check(self._lib.ddrl_dqn_act(self._h, _lib.dptr(obs), n, mode, float(self.greedy_prob), self._noise_seed, self._noise_ctr,
                                      _lib.dptr(out), _lib.dptr(q_out), _lib.stream_ptr()))
    self._noise_ctr += 2 * n
    return out


EVAL_ROW = 20   # floats per step of an evaluation trace (csrc/eval_q.hip)


def _evaluate(self, n=10, seed=0, first_episode=0, max_ep_len=None, deterministic=None, greedy_prob=None, trace=False):
    """n evaluation episodes on the device as ONE launch (ddrl_dqn_eval, csrc/eval_q.hip): episode e is the (first_episode + e)-th
    episode a host `LunarLanderDiscrete(seed, max_ep_len)` plays, acted on with this actor's current main weights (SQN: q1) under
    get_actions' selection rules.  Defaults are what the class's _test_action does: Double-DQN samples with greedy_prob 0.97, SQN is
    deterministic.  Step t of episode e draws its two uniforms at self._noise_ctr + 2 (e max_ep_len + t) [+ 1] of the object's counter
    stream, which advances by 2 n max_ep_len per call, whatever the mode.
    -> dict(ret float64 [n], len int32 [n]) NumPy, and with trace=True `trace` float32 [n, max_ep_len, 20]: per step obs[8] acted on,
    the q row [8:16] (zeros beyond act_dim), the action index, rew, ended, 0; zero rows past an episode's end.
    One weight snapshot, one launch, one synchronisation; weights, Adam state and the acting forward's packed copy are untouched."""
    n = int(n)
    if max_ep_len is None:
        max_ep_len = getattr(self.opt, "max_ep_len", None)
        if max_ep_len is None:
            raise ValueError("evaluate: max_ep_len is neither given nor an attribute of the actor's options")
    max_ep_len = int(max_ep_len)
    deterministic = self._eval_deterministic if deterministic is None else bool(deterministic)
    greedy_prob = float(self.greedy_prob if greedy_prob is None else greedy_prob)
    flat = self.export(_lib.SAC1_MAIN)
    ret = torch.empty(max(n, 1), dtype=torch.float64, device=self.device)
    ln = torch.empty(max(n, 1), dtype=torch.int32, device=self.device)
    tr = torch.empty(max(n, 1), max(max_ep_len, 1), EVAL_ROW, dtype=torch.float32, device=self.device) if trace else None
    mode = _lib.DDRL_ACT_DETERMINISTIC if deterministic else _lib.DDRL_ACT_SAMPLE
    _lib.check(self._lib.ddrl_dqn_eval(ctypes.byref(self.cfg), _lib.dptr(flat), n, int(seed) & 0xFFFFFFFF, int(first_episode), max_ep_len,
                                       mode, greedy_prob, self._noise_seed, self._noise_ctr, _lib.dptr(ret), _lib.dptr(ln), _lib.dptr(tr),
                                       _lib.stream_ptr()))
    self._noise_ctr += 2 * n * max_ep_len
    torch.cuda.current_stream().synchronize()
    out = {"ret": ret.cpu().numpy(), "len": ln.cpu().numpy()}
    if trace:
        out["trace"] = tr.cpu().numpy()
    return out


def _evaluate_env(self, dev_env, n=10, first_episode=None, deterministic=None, greedy_prob=None, trace=False):
    """n evaluation episodes of `dev_env`'s model — an env.DeviceLunarLanderDiscrete of either model — as one launch fed from handles
    (ddrl_env_eval_q, csrc/eval3.hip): episode e is the (first_episode + e)-th episode a host
    `LunarLanderDiscrete(dev_env.seed, dev_env.max_ep_len, model=...)` plays (default: from dev_env.episodes_played on; the count is NOT
    advanced here), acted on with this handle's current main weights (SQN: q1), which the library reads out of the handle.  Modes,
    defaults and the noise-counter rule are `evaluate`'s: the counter advances by 2 n max_ep_len per call, whatever the mode.
    -> the dict `evaluate` returns, read from the results block the marker's handle owns."""
    n = int(n)
    first = int(dev_env.episodes_played if first_episode is None else first_episode)
    deterministic = self._eval_deterministic if deterministic is None else bool(deterministic)
    greedy_prob = float(self.greedy_prob if greedy_prob is None else greedy_prob)
    mode = _lib.DDRL_ACT_DETERMINISTIC if deterministic else _lib.DDRL_ACT_SAMPLE
    vec = dev_env.handle()
    _lib.check(self._lib.ddrl_env_eval_q(vec._h, self._h, n, first, mode, greedy_prob, self._noise_seed, self._noise_ctr,
                                         1 if trace else 0, _lib.stream_ptr()))
    self._noise_ctr += 2 * n * int(dev_env.max_ep_len)
    from .env import eval_results
    return eval_results(vec, EVAL_ROW)


# -- version store: exact per-env weight adoption of the vectorised discrete rollout worker (algos/dqn/train.py:249-252) -------------------
def _enable_versions(self, n_slots):
    """Keep `n_slots` resident copies of the acting Q network (ddrl_dqn_versions_enable): set_weights / import_ of MAIN / the repack after
    a learner step then store a NEW version (instead of replacing the one every env acts on) and the fused rollout step moves an env to
    the newest version at that env's own episode end.  get_actions keeps acting on the newest weights."""
    _lib.check(self._lib.ddrl_dqn_versions_enable(self._h, int(n_slots), _lib.stream_ptr()))
    self.n_slots = int(n_slots)


def _version_state(self, with_slots=True):
    """-> (slot of every env [max_rows] int32 device tensor or None, dict(newest, live, tiles, out_of_slots))."""
    rows = (self.max_rows + 31) & ~31      # the acting forward's rows: whole 32-row tiles
    slots = torch.empty(rows, dtype=torch.int32, device=self.device) if with_slots else None
    st = (ctypes.c_int32 * 4)()
    _lib.check(self._lib.ddrl_dqn_versions_state(self._h, _lib.dptr(slots), st, _lib.stream_ptr()))
    return (slots[:self.max_rows] if with_slots else None), {"newest": int(st[0]), "live": int(st[1]), "tiles": int(st[2]), "out_of_slots": bool(st[3])}


def _adopt_where_ended(self, ended):
    """Episode ends of steps taken outside the fused rollout step (uint8 mask of env.step): those envs pull."""
    ended = ended.to(device=self.device, dtype=torch.uint8).contiguous()
    _lib.check(self._lib.ddrl_dqn_versions_adopt(self._h, _lib.dptr(ended), int(ended.numel()), _lib.stream_ptr()))


def _noise_stream(opt, job, index=0):
    """(seed, counter) of an actor's uniform stream — the recipe agent.Actor uses for its normals."""
    import zlib
    return (int(getattr(opt, "seed", 0)) * 2654435761 + zlib.crc32(str(job).encode()) + 97 * int(index)) & 0xFFFFFFFF, 0


class Actor(Learner):
    """algos/dqn/actor_learner.py:152-201: the q network alone; get_action(o) = argmax q with probability 0.97,
    a uniform random action otherwise (actor_learner.py:193-201; np.random there, a seeded RandomState here)."""

    greedy_prob = 0.97

    def __init__(self, opt, job="worker", max_rows=1, index=0):
        super().__init__(opt, job, batch=max_rows)
        self._rs = np.random.RandomState(getattr(opt, "seed", 0))
        self.max_rows = int(max_rows)
        self._noise_seed, self._noise_ctr = _noise_stream(opt, job, index)

    get_actions = _get_actions
    enable_versions, version_state, adopt_where_ended = _enable_versions, _version_state, _adopt_where_ended

    def get_action(self, o):
        if self._rs.uniform() < 0.97:
            return int(np.argmax(self._q_row(o)))
        return int(self._rs.randint(0, self.opt.act_dim))

    def _test_action(self, o):
        return self.get_action(o)

    _eval_deterministic = False   # evaluate's default mode: what _test_action does
    evaluate, evaluate_env = _evaluate, _evaluate_env

    def test(self, test_env, n=10):
        """actor_learner.py:230-251: n episodes to their terminal with the actor's own get_action; (mean return, mean of
        test_env.rewards[0] at each episode's end — the trading env's score).
        On a test env with `on_device` (env.DeviceLunarLanderDiscrete) the n episodes run as ONE launch (evaluate) from
        test_env.episodes_played on, which then advances by n; the lander's score is its return, so (mean return, mean return).
        A marker of the articulated model runs evaluate_env (ddrl_env_eval_q, csrc/eval3.hip) instead.
        The env's max_ep_len must equal opt.max_ep_len where the options carry one (the device plays whole episodes).  Outside the
        kernel's envelope (DdrlUnsupported) the host loop below runs on test_env.host_env(): the same episode indices."""
        if getattr(test_env, "on_device", False):
            want = int(getattr(self.opt, "max_ep_len", test_env.max_ep_len))
            if int(test_env.max_ep_len) != want:
                raise ValueError("the test env's max_ep_len (%d) must equal the agent's (%d): the device plays whole episodes"
                                 % (test_env.max_ep_len, want))
            try:
                if getattr(test_env, "model", "simple") != "simple":   # the articulated lander: the handle-fed launch (ddrl_env_eval_q)
                    ret = float(np.mean(self.evaluate_env(test_env, n)["ret"]))
                else:
                    ret = float(np.mean(self.evaluate(n, test_env.seed, test_env.episodes_played, want)["ret"]))
                out = (ret, ret)
            except _lib.DdrlUnsupported:
                out = self.test(test_env.host_env(), n)
            test_env.episodes_played += n
            return out
        test_rets, scores = [], []
        for _ in range(n):
            o, r, d, ep_ret, ep_len = test_env.reset(), 0, False, 0, 0
            while True:
                o, r, d, _ = test_env.step(self._test_action(o))
                ep_ret += r
                ep_len += 1
                if d:
                    test_rets.append(ep_ret)
                    scores.append(test_env.rewards[0])
                    break
        return np.mean(test_rets), np.mean(scores)

    def write_tb(self, ave_test_reward, ave_score, alratio, update_frequency, total_learner_step):
        """actor_learner.py:203-228: the four test scalars ("Reward", "score", "a_l_ratio", "update_frequency") at step
        total_learner_step, into the run directory the reference names for job == "test" (actor_learner.py:173-176)."""
        if getattr(self, "_writer", None) is None:
            import datetime
            from .logx import SummaryWriter
            o = self.opt
            self._writer = SummaryWriter("%s/%s-%s-%s-workers_num:%s%%%s" % (getattr(o, "summary_dir", "."), datetime.datetime.now(), getattr(o, "env_name", ""),
                                                                            getattr(o, "exp_name", ""), getattr(o, "num_workers", 1), getattr(o, "a_l_ratio", "")))
        for tag, v in (("Reward", ave_test_reward), ("score", ave_score), ("a_l_ratio", alratio), ("update_frequency", update_frequency)):
            self._writer.add_scalar(tag, float(v), int(total_learner_step))
        self._writer.flush()


class LearnerSQN(Learner):
    """algos/sqn/actor_learner.py:19-131 (twin soft-Q networks main/q1, main/q2; step_ops = [q_loss, q1, q2, ...]):
    same surface as Learner; `opt.alpha` is the softmax policy's temperature (hyperparams.py:27)."""
    NETS = ("q1", "q2")
    VARIANT = 1  # DDRL_SQN


class ActorSQN(LearnerSQN):
    """algos/sqn/actor_learner.py:134-201: get_action(o, deterministic) = argmax of / a sample from
    softmax(q1(o) / alpha) (core.py:30-42; tf.random.multinomial there, a seeded RandomState here)."""

    greedy_prob = 0.97   # (unused by the SQN rules; ddrl_dqn_act takes it for both variants)

    def __init__(self, opt, job="worker", max_rows=1, index=0):
        super().__init__(opt, job, batch=max_rows)
        self._rs = np.random.RandomState(getattr(opt, "seed", 0))
        self.max_rows = int(max_rows)
        self._noise_seed, self._noise_ctr = _noise_stream(opt, job, index)

    get_actions = _get_actions
    enable_versions, version_state, adopt_where_ended = _enable_versions, _version_state, _adopt_where_ended

    def get_action(self, o, deterministic=False):
        q = self._q_row(o).astype(np.float64)
        if deterministic:
            return int(np.argmax(q))
        z = q / float(self.opt.alpha)
        p = np.exp(z - z.max())
        return int(self._rs.choice(len(p), p=p / p.sum()))

    def _test_action(self, o):
        return self.get_action(o, deterministic=True)     # algos/sqn/actor_learner.py:238

    _eval_deterministic = True
    evaluate, evaluate_env = _evaluate, _evaluate_env
    test, write_tb = Actor.test, Actor.write_tb
