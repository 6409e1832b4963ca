"""Every refusal of the eight fused rollout entry points (ddrl_rollout_begin / _step, and their _articulated, _discrete and _nstep
siblings): the status, a distinctive part of ddrl_last_error(), and nothing touched — one table, TABLE below, copied from the host code of
csrc/env.hip.  A row is (entry point, what differs from the family's good call, status, text).  All refusals return before a launch.

Untouched means: the state block of the envs of the call and the counters of its ring are bit-equal before and after every row, and the
observation rows of the family's actor survive the whole table.  Those rows have no getter; they are what the next fused step acts on, so
after the table the good call runs once, deterministically, and its action and next-observation mirrors must equal those of a twin (same
seeds, same weights, begin + step) that never saw a refused call.

The second half is the switch between the unfused and the fused path of the three rollout workers (test_switching_*)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N, CAP, LN, LIMIT = 64, 256, 4, 17
FAMILIES = ("", "_articulated", "_discrete", "_nstep")


def _pi_opt(n=N, Ln=LN):
    from distributed_drl_amd.agent import HyperParameters
    opt = HyperParameters()
    opt.hidden_sizes, opt.num_envs, opt.seed, opt.max_ep_len = (64, 64), n, 5, 50
    opt.Ln, opt.save_freq, opt.buffer_size, opt.num_buffers = Ln, 1, CAP, 1
    return opt


class _QOpt:
    obs_dim, act_dim, hidden_size, gamma, lr, polyak, batch_size, seed, alpha = 8, 4, [64, 64], 0.99, 1e-3, 0.995, 64, 5, 0.1


class _World:
    """The handles the table's rows name, each built when first asked for and kept."""

    def __init__(self):
        self.made = {}

    def __getitem__(self, name):
        if name not in self.made:
            self.made[name] = self.make(name)
        return self.made[name]

    def make(self, name, fresh=False):
        import distributed_drl_amd as ddrl
        from distributed_drl_amd import dqn
        from distributed_drl_amd.agent import Actor
        from distributed_drl_amd.env import VecLunarLander, VecLunarLanderDiscrete
        from distributed_drl_amd.replay import ReplayBuffer
        from distributed_drl_amd.workers import WindowQueue

        class Ring1D(ReplayBuffer):
            _acts_1d = True

        kind, _, arg = name.partition(":")
        art = dict(model="articulated", velocity_iterations=4, position_iterations=2)
        if kind in ("one", "art", "disc", "disc_art"):   # envs ("one:64/nstep": a family's own), a few steps into their episodes
            cls = VecLunarLanderDiscrete if kind.startswith("disc") else VecLunarLander
            env = cls(int(arg.split("/")[0]), seed=7, max_ep_len=50, **(art if kind.endswith("art") else {}))
            torch.manual_seed(1)
            for _ in range(3):
                env.step(env.sample_actions())
            return env
        if kind in ("pi", "q"):                          # actors: "pi:64", "q:128v" (v: with a version store), "pi:64/nstep" (one per family)
            rows = int(arg.split("/")[0].rstrip("v"))
            a = Actor(_pi_opt(rows), max_rows=rows) if kind == "pi" else dqn.Actor(_QOpt, "worker", max_rows=rows)
            if "v" in arg.split("/")[0]:
                a.enable_versions(8)
            return a
        if kind == "ring":
            rb = {"sac": lambda: ddrl.ReplayBufferSAC1(8, 2, CAP, seed=0), "dqn": lambda: Ring1D(8, 1, CAP),
                  "compact2": lambda: ReplayBuffer(8, 2, CAP, compact_obs=True), "compact1": lambda: Ring1D(8, 1, CAP, compact_obs=True),
                  "win": lambda: ddrl.ReplayBufferNStep(_pi_opt()), "win5": lambda: ddrl.ReplayBufferNStep(_pi_opt(Ln=5))}[arg]()
            if arg in ("sac", "dqn") and not fresh:      # some rows, so that "unchanged" is not "still empty"
                acts = torch.rand(40, 2, device="cuda") if arg == "sac" else torch.floor(torch.rand(40, device="cuda") * 4)
                rb.store_batch(torch.rand(40, 8, device="cuda"), acts, torch.rand(40, device="cuda"), torch.rand(40, 8, device="cuda"),
                               torch.zeros(40, device="cuda"))
            return rb
        if kind == "wq":                                 # window queues: "wq:64x4" = 64 envs, Ln 4
            n, Ln = (int(x) for x in arg.split("x"))
            return WindowQueue(n, Ln, 8, 2)
        raise KeyError(name)


@pytest.fixture(scope="module")
def world():
    import distributed_drl_amd as d
    d._lib.require_gpu()
    return _World()


# the good call of every family: what a row does not name
GOOD = {"": dict(env="one:64", actor="pi:64/one", ring="ring:sac"),
        "_articulated": dict(env="art:64", actor="pi:64/art", ring="ring:sac"),
        "_discrete": dict(env="disc:64", actor="q:64", ring="ring:dqn"),
        "_nstep": dict(env="one:64/nstep", actor="pi:64/nstep", ring="ring:win", winq="wq:64x4")}

U, B = "DDRL_ERR_UNSUPPORTED", "DDRL_ERR_BAD_ARG"
NO_POLICY = "no direct-operand policy"
ONE_BODY_ONLY = ": not built for the articulated lander"
ARTICULATED_ONLY = ": built for the articulated lander"
MISMATCH = "n_envs a multiple of 32 within max_rows"
MISMATCH3 = "n_envs must be a multiple of 32 within the actor's max_rows"
STORE_ROWS = "an actor with a version store steps exactly max_rows envs"
FLOAT32_ONLY = "float32 rings only (not a compact uint8 ring)"
Q_ENVELOPE = "n_envs a multiple of 32 within the handle's batch"
N_ENVELOPE = "n_envs a multiple of 32 within the actor's max_rows (all of them with a version store)"
TABLE = [
    # ---- the one-body continuous pair: DDRL_REQUIREs
    ("ddrl_rollout_begin", dict(env="art:64"), U, "ddrl_rollout_begin" + ONE_BODY_ONLY),
    ("ddrl_rollout_begin", dict(env="one:48", actor="pi:48"), B, NO_POLICY),
    ("ddrl_rollout_begin", dict(actor="pi:32"), B, "actor / env mismatch (obs_dim 8, max_rows >= n_envs, same device)"),
    ("ddrl_rollout_step", dict(env="art:64"), U, "ddrl_rollout_step" + ONE_BODY_ONLY),
    ("ddrl_rollout_step", dict(misaligned="act_out_d"), B, "act_out_d must be 8-byte aligned"),
    ("ddrl_rollout_step", dict(misaligned="next_obs_out_d"), B, "next_obs_out_d must be 16-byte aligned"),
    ("ddrl_rollout_step", dict(env="one:48", actor="pi:48"), B, NO_POLICY),
    ("ddrl_rollout_step", dict(env="one:48"), B, MISMATCH),
    ("ddrl_rollout_step", dict(actor="pi:32"), B, MISMATCH),
    ("ddrl_rollout_step", dict(ring="ring:dqn"), B, "replay row shape must be (obs1[8], obs2[8], acts[2], rews, done)"),
    ("ddrl_rollout_step", dict(ring="ring:compact2"), B, FLOAT32_ONLY),
    ("ddrl_rollout_step", dict(n_steps=0), B, "n_steps must be >= 1"),
    ("ddrl_rollout_step", dict(actor="pi:128v"), B, STORE_ROWS),
    ("ddrl_rollout_step", dict(actor="pi:128v", n_steps=0), B, "n_steps must be >= 1"),                  # two apply: the first one today
    ("ddrl_rollout_step", dict(ring="ring:compact2", misaligned="act_out_d"), B, "act_out_d must be 8-byte aligned"),
    # ---- the articulated pair: one envelope with the function's name, DDRL_ERR_UNSUPPORTED
    ("ddrl_rollout_begin_articulated", dict(env="one:64"), U, "ddrl_rollout_begin_articulated" + ARTICULATED_ONLY),
    ("ddrl_rollout_begin_articulated", dict(env="art:48", actor="pi:48"), U, NO_POLICY),
    ("ddrl_rollout_begin_articulated", dict(env="art:48"), U, "ddrl_rollout_begin_articulated: " + MISMATCH3),
    ("ddrl_rollout_begin_articulated", dict(actor="pi:32"), U, MISMATCH3),
    ("ddrl_rollout_begin_articulated", dict(actor="pi:128v"), U, STORE_ROWS),
    ("ddrl_rollout_step_articulated", dict(env="one:64"), U, "ddrl_rollout_step_articulated" + ARTICULATED_ONLY),
    ("ddrl_rollout_step_articulated", dict(misaligned="act_out_d"), B, "act_out_d must be 8-byte aligned"),
    ("ddrl_rollout_step_articulated", dict(misaligned="next_obs_out_d"), B, "next_obs_out_d must be 16-byte aligned"),
    ("ddrl_rollout_step_articulated", dict(env="art:48"), U, "ddrl_rollout_step_articulated: " + MISMATCH3),
    ("ddrl_rollout_step_articulated", dict(actor="pi:32"), U, MISMATCH3),
    ("ddrl_rollout_step_articulated", dict(actor="pi:128v"), U, STORE_ROWS + "; use ddrl_actor_act + ddrl_env_step + ddrl_replay_store"),
    ("ddrl_rollout_step_articulated", dict(ring="ring:dqn"), U, "the replay row shape must be (obs1[8], obs2[8], acts[2], rews, done)"),
    ("ddrl_rollout_step_articulated", dict(ring="ring:compact2"), U, FLOAT32_ONLY),
    ("ddrl_rollout_step_articulated", dict(n_steps=0), B, "n_steps must be >= 1"),
    ("ddrl_rollout_step_articulated", dict(actor="pi:128v", n_steps=0), U, STORE_ROWS),                  # the envelope before n_steps
    # ---- the discrete pair
    ("ddrl_rollout_begin_discrete", dict(env="disc_art:64"), U, "ddrl_rollout_begin_discrete" + ONE_BODY_ONLY),
    ("ddrl_rollout_begin_discrete", dict(env="disc:48"), U, Q_ENVELOPE),
    ("ddrl_rollout_begin_discrete", dict(actor="q:32"), U, Q_ENVELOPE),
    ("ddrl_rollout_step_discrete", dict(env="disc_art:64"), U, "ddrl_rollout_step_discrete" + ONE_BODY_ONLY),
    ("ddrl_rollout_step_discrete", dict(misaligned="next_obs_out_d"), B, "next_obs_out_d must be 16-byte aligned"),
    ("ddrl_rollout_step_discrete", dict(n_steps=0), B, "n_steps must be >= 1"),
    ("ddrl_rollout_step_discrete", dict(mode=7), B, "mode must be DDRL_ACT_SAMPLE or DDRL_ACT_DETERMINISTIC"),
    ("ddrl_rollout_step_discrete", dict(env="disc:48"), U, Q_ENVELOPE),
    ("ddrl_rollout_step_discrete", dict(actor="q:32"), U, Q_ENVELOPE),
    ("ddrl_rollout_step_discrete", dict(ring="ring:sac"), B, "replay row shape must be (obs1[8], obs2[8], acts, rews, done)"),
    ("ddrl_rollout_step_discrete", dict(ring="ring:compact1"), B, FLOAT32_ONLY),
    ("ddrl_rollout_step_discrete", dict(actor="q:128v"), B, "a handle with a version store steps exactly the acting forward's 128 rows (n_envs 64)"),
    ("ddrl_rollout_step_discrete", dict(actor="q:128v", ring="ring:sac"), B, "replay row shape must be"),  # the ring before the store's rows
    # ---- the n-step pair
    ("ddrl_rollout_begin_nstep", dict(env="art:64"), U, "ddrl_rollout_begin_nstep" + ONE_BODY_ONLY),
    ("ddrl_rollout_begin_nstep", dict(env="one:48", actor="pi:48", winq="wq:48x4"), U, "needs n_envs a multiple of 32 (n_envs 48)"),
    ("ddrl_rollout_begin_nstep", dict(actor="pi:32"), U, N_ENVELOPE),
    ("ddrl_rollout_begin_nstep", dict(actor="pi:128v"), U, N_ENVELOPE),
    ("ddrl_rollout_begin_nstep", dict(winq="wq:32x4"), U, "the window queues hold 32 envs of obs_dim 8, act_dim 2; the envs are 64 of 8 and 2"),
    ("ddrl_rollout_begin_nstep", dict(winq="wq:64x17"), U, "Ln 17 is above DDRL_NSTEP_FUSED_MAX_LN"),
    ("ddrl_rollout_step_nstep", dict(env="art:64"), U, "ddrl_rollout_step_nstep" + ONE_BODY_ONLY),
    ("ddrl_rollout_step_nstep", dict(n_steps=0), B, "n_steps, action_repeat and limit_steps must be >= 1"),
    ("ddrl_rollout_step_nstep", dict(misaligned="act"), B, "out->act must be 8-byte aligned"),
    ("ddrl_rollout_step_nstep", dict(misaligned="next_obs"), B, "out->next_obs must be 16-byte aligned"),
    ("ddrl_rollout_step_nstep", dict(env="one:48", actor="pi:48", winq="wq:48x4"), U, "needs n_envs a multiple of 32 (n_envs 48)"),
    ("ddrl_rollout_step_nstep", dict(actor="pi:32"), U, N_ENVELOPE),
    ("ddrl_rollout_step_nstep", dict(actor="pi:128v"), U, N_ENVELOPE),
    ("ddrl_rollout_step_nstep", dict(winq="wq:32x4"), U, "the window queues hold 32 envs"),
    ("ddrl_rollout_step_nstep", dict(winq="wq:64x17"), U, "Ln 17 is above DDRL_NSTEP_FUSED_MAX_LN"),
    ("ddrl_rollout_step_nstep", dict(ring="ring:sac"), U, "a four-array window ring {o, a, r, d}; this ring has 5 arrays"),
    ("ddrl_rollout_step_nstep", dict(ring="ring:compact2"), U, "a four-array window ring {o, a, r, d}; this ring has 5 arrays"),
    ("ddrl_rollout_step_nstep", dict(ring="ring:win5"), U, "are not the queues' windows {(Ln+1)*8, Ln*2, Ln, Ln} at Ln 4"),
    ("ddrl_rollout_step_nstep", dict(winq="wq:64x17", ring="ring:sac"), U, "DDRL_NSTEP_FUSED_MAX_LN"),   # the queues before the ring
]


class _Mirrors:
    """The step calls' optional device outputs; `off`: the named one 4 bytes off its grid."""

    def __init__(self, n):
        self.act, self.act1 = torch.zeros(n * 2 + 4, device="cuda"), torch.zeros(n, device="cuda")
        self.q, self.nxt = torch.zeros(n, 4, device="cuda"), torch.zeros(n * 8 + 4, device="cuda")

    def ptr(self, t, off=False):
        return ctypes.c_void_p(t.data_ptr() + (4 if off else 0))


def _call(world, entry, kw, mirrors, deterministic=0):
    from distributed_drl_amd import _lib
    lib, sp = _lib.load(), _lib.stream_ptr()
    family = entry.replace("ddrl_rollout_begin", "").replace("ddrl_rollout_step", "")
    names = dict(GOOD[family], **{k: v for k, v in kw.items() if k in ("env", "actor", "ring", "winq")})
    env, actor = world[names["env"]], world[names["actor"]]
    fn, bad, m = getattr(lib, entry), kw.get("misaligned"), mirrors
    if "begin" in entry:
        return fn(env._h, actor._h, *([world[names["winq"]]._h] if family == "_nstep" else []), sp), names
    ring, n_steps = world[names["ring"]], kw.get("n_steps", 1)
    if family in ("", "_articulated"):
        return fn(env._h, actor._h, ring._h, n_steps, 3, 0, deterministic, m.ptr(m.act, bad == "act_out_d"), m.ptr(m.nxt, bad == "next_obs_out_d"), sp), names
    if family == "_discrete":
        mode = kw.get("mode", _lib.DDRL_ACT_DETERMINISTIC if deterministic else _lib.DDRL_ACT_SAMPLE)
        return fn(env._h, actor._h, ring._h, n_steps, mode, 0.5, 3, 0, m.ptr(m.act1), m.ptr(m.q), m.ptr(m.nxt, bad == "next_obs_out_d"), sp), names
    out = _lib.RolloutNStepOut(act=m.ptr(m.act, bad == "act"), next_obs=m.ptr(m.nxt, bad == "next_obs"))
    return fn(env._h, actor._h, world[names["winq"]]._h, ring._h, n_steps, 0.0, 0.0, 1.0, 3, LIMIT, 0, 3, 0, ctypes.byref(out), sp), names


def _untouched(world, names):
    torch.cuda.synchronize()
    snap = [world[names["env"]].get_state().clone()]
    if "ring" in names:
        snap.append(torch.tensor(world[names["ring"]]._counts()))
    return snap


@pytest.mark.parametrize("family", FAMILIES, ids=lambda f: f or "_one_body")
def test_every_refusal_has_its_status_and_text_and_touches_nothing(world, family):
    from distributed_drl_amd import _lib
    lib = _lib.load()
    begin, step = "ddrl_rollout_begin" + family, "ddrl_rollout_step" + family
    rows = [r for r in TABLE if r[0] in (begin, step)]
    assert len(rows) >= 9 and {r[0] for r in rows} == {begin, step}
    mirrors = _Mirrors(N)
    rc, _ = _call(world, begin, {}, mirrors)
    assert rc == 0, lib.ddrl_last_error()        # the family's actor holds its envs' observations
    for entry, kw, status, text in rows:
        before = _untouched(world, dict(GOOD[family], **{k: v for k, v in kw.items() if k in ("env", "actor", "ring", "winq")}))
        rc, names = _call(world, entry, kw, mirrors)
        msg = lib.ddrl_last_error().decode()
        assert rc == getattr(_lib, status), (entry, kw, rc, msg)
        assert text in msg, (entry, kw, msg)
        for k, (x, y) in enumerate(zip(before, _untouched(world, names))):
            assert torch.equal(x, y), (entry, kw, k)
    assert not mirrors.act.any() and not mirrors.act1.any() and not mirrors.q.any() and not mirrors.nxt.any()
    # the actor's observation rows: the good step acts on them as its twin does, which was never refused anything
    rc, _ = _call(world, step, {}, mirrors, deterministic=1)
    assert rc == 0, lib.ddrl_last_error()
    twin, m2 = _World(), _Mirrors(N)
    twin.made["ring:dqn"], twin.made["ring:sac"] = twin.make("ring:dqn", fresh=True), twin.make("ring:sac", fresh=True)
    assert _call(twin, begin, {}, m2)[0] == 0 and _call(twin, step, {}, m2, deterministic=1)[0] == 0, lib.ddrl_last_error()
    torch.cuda.synchronize()
    assert mirrors.act.any() or mirrors.act1.any() or family == "_discrete"
    for name in ("act", "act1", "q", "nxt"):
        assert torch.equal(getattr(mirrors, name), getattr(m2, name)), (family, name)
    assert torch.equal(world[GOOD[family]["env"]].get_state(), twin[GOOD[family]["env"]].get_state())


# ---- the switch between the unfused and the fused path, the same for the three workers ------------------------------------------------
class _Counted:
    """A thin counting wrapper on a bound library function."""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self, *args):
        self.calls += 1
        return self.fn(*args)


def _switch_worker(kind):
    import distributed_drl_amd as ddrl
    from distributed_drl_amd import dqn
    from distributed_drl_amd.agent import Learner
    if kind == "discrete":
        class Opt(_QOpt):
            num_envs, max_ep_len, start_steps, adopt, a_l_ratio, num_nodes, num_buffers, push_freq, buffer_size, variant = N, 50, 2, "episode", 2, 1, 1, 50, 1024, "ddqn"
        opt = Opt()
        ps = ddrl.ParameterServer(*dqn.Learner(opt).get_weights())
        rb = ddrl.ReplayBufferDQN(opt, 0, seed=5)
        return ddrl.RolloutDeviceDQN(ps, rb, opt), rb
    opt = _pi_opt()
    opt.start_steps, opt.adopt, opt.buffer_size = 2, "episode", 1024
    ps = ddrl.ParameterServer(*Learner(opt).get_weights())
    if kind == "nstep":
        opt.action_repeat = 3
        rb = ddrl.ReplayBufferNStep(opt)
        return ddrl.RolloutDeviceNStep(ps, rb, opt), rb
    rb = ddrl.ReplayBufferSAC1(8, 2, 1024, seed=0)
    return ddrl.RolloutDevice(ps, rb, opt), rb


@pytest.mark.parametrize("kind", ["continuous", "discrete", "nstep"])
def test_switching_between_the_unfused_and_the_fused_path(kind):
    """start_steps 2, adopt "episode": the random-action steps run unfused, the policy steps fused.  Every step that stores puts the
    observations the envs showed just before it into the ring (the n-step worker: as the newest-but-one frame of the windows it stores
    Ln steps later, so its ring is read through the window queue's o rows instead); an unfused step clears _fused_live and the next
    fused step runs the begin call again; the decision itself is made once."""
    import distributed_drl_amd as d
    d._lib.require_gpu()
    lib = d._lib.load()
    begin_name = {"continuous": "ddrl_rollout_begin", "discrete": "ddrl_rollout_begin_discrete", "nstep": "ddrl_rollout_begin_nstep"}[kind]
    begin = _Counted(getattr(lib, begin_name))
    setattr(lib, begin_name, begin)
    try:
        ro, rb = _switch_worker(kind)
        assert ro.actor._lib is lib and ro._versions
        # "episode": the two transition workers decide in their constructor, the n-step worker at its first policy step — where the
        # decision's begin call stands for the refresh
        decided = 0 if kind == "nstep" else 1
        assert ro._fused is (True if decided else None) and begin.calls == decided
        stored = 0

        def one_step(want_fused):
            nonlocal stored
            obs = ro.env.obs.clone()
            ro.step()
            assert ro._fused is (True if begin.calls else None)
            assert ro._fused_live is want_fused
            if kind == "nstep":
                assert torch.equal(ro.winq.arrays[0][:, -2], obs)        # [n][Ln+1][8]: the step's o2 went in behind the frame it acted on
                size = rb._counts()[1]
                new = rb.rings()["buffer_o"][stored:size, -2]            # ... and so it stands in every window stored now
                assert (new[:, None, :] == obs[None]).all(-1).any(-1).all()
                stored = size
            else:
                rows = (stored + torch.arange(N, device="cuda")) % 1024
                assert torch.equal(rb.rings()["obs1_buf"][rows].reshape(N, 8), obs)
                stored += N

        for _ in range(1 if kind == "discrete" else 3):   # t <= start_steps = 2 (the discrete worker counts transitions): random actions, unfused
            one_step(False)
        assert begin.calls == decided
        one_step(True)                       # the first policy step: the begin call (refresh, or the n-step worker's decision), then the fused launch
        assert begin.calls == 2 - (kind == "nstep")
        one_step(True)
        assert begin.calls == 2 - (kind == "nstep")
        t_policy = ro.filling_steps if kind == "nstep" else ro.t
        if kind == "nstep":
            ro.filling_steps = 0             # back into the random-action phase for one step
        else:
            ro.t = 0
        one_step(False)
        if kind == "nstep":
            ro.filling_steps = t_policy
        else:
            ro.t = t_policy
        one_step(True)
        assert begin.calls == 3 - (kind == "nstep")                      # ... and exactly one more begin call
        assert ro._fused_ready() is True and begin.calls == 3 - (kind == "nstep")   # decided once: asking again calls nothing
        assert stored > 0
    finally:
        setattr(lib, begin_name, begin.fn)
