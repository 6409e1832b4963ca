"""The memory-contract and stream-contract rows of the handle kinds that come through another door than ddrl.h's creators:
ddrl_sac1_create_wide (include/ddrl_sac1_wide.h), ddrl_sacv_create_wide (ddrl_sacv_wide.h), ddrl_dqn_create_direct on both variants
(ddrl_dqn_direct.h) and ddrl_actor_create_wide (ddrl_actor_wide.h).  Each of those headers says that the handle is an ordinary one and
that the stream contract and the memory contract are ddrl.h's; the rows here hold the functions of ddrl.h to that on such a handle,
with the case builders of tests/_abi_contract.py behind their `door` keyword (the creator, the shape, the variant and the query that
must answer 1 — _abi_contract.Door).  tests/test_gpu_abi_handles.py runs CASES between guard bands, and CASES and STREAM_CASES on a side
stream.

CASES / STREAM_CASES / TABLE stay here, as in tests/_abi_contract_walker_nstep.py: this module enters NO row in _abi_contract's tables,
which are parsed against include/ddrl.h function by function and parametrise tests/test_gpu_abi_memory.py and test_gpu_abi_stream.py at
import.  TABLE is keyed by (kind, function); tests/test_abi_handles_table_cpu.py holds it to ddrl.h: every function with a row in
_abi_contract's tables that takes a learner or an actor handle has a row here for every kind of that handle, or stands in EXEMPT.

A REFUSAL row (the split API on a wide learner, ddrl_dqn_step_ring on a direct handle, the fused rollout entry points on a wide actor,
ddrl_env_eval_policy with an actor that is not 8 -> 2) has the shape of replay_sample-empty_ring_refused: ctx.expect_rc is the
documented code, every output is declared untouched, and the handle's state is exported before and behind the refused call into
declared outputs that are compared with the twin's by the arena and with each other, bit for bit, when the run is over."""
from ctypes import byref, c_void_p as P

import numpy as np
import torch

import _abi_contract as ac
from _abi_contract import Door, F32, I64, _f32, _ok, _rs, _tp, _weights

KINDS = ("sac1-wide", "sacv-wide", "ddqn-direct", "sqn-direct", "actor-wide")
HANDLE_KINDS = {"ddrl_sac1_t": ("sac1-wide", "sacv-wide"), "ddrl_dqn_t": ("ddqn-direct", "sqn-direct"), "ddrl_actor_t": ("actor-wide",)}

CASES = {}          # id -> (fn, (functions covered)): memory runs and S runs
STREAM_CASES = {}   # id -> (fn, (functions covered)): S runs only (host outputs, calls ahead)
TABLE = {}          # (kind, function) -> [case ids]
REFUSAL_CASES = []  # the ids of the refusal rows


def _enter(cases, cid, kind, functions):
    def deco(fn):
        assert kind in KINDS, kind
        assert cid not in CASES and cid not in STREAM_CASES and cid not in ac.CASES and cid not in ac.STREAM_CASES, cid
        cases[cid] = (fn, functions)
        for f in functions:
            TABLE.setdefault((kind, f), []).append(cid)
        return fn
    return deco


def case(cid, kind, *functions):
    return _enter(CASES, cid, kind, functions)


def stream_case(cid, kind, *functions):
    return _enter(STREAM_CASES, cid, kind, functions)


UNSUPPORTED, BAD_ARG = -5, -1     # DDRL_ERR_UNSUPPORTED, DDRL_ERR_BAD_ARG

# ---- the shapes: the smallest at which each path's branches differ ------------------------------------------------------------------
SAC_SHAPES = {
    "o12a1h36x8B5": (12, 1, 36, 8, 5),         # first shape outside the narrow envelope; element loads; one action; one ragged tile
    "o24a4h64x48B37": (24, 4, 64, 48, 37),     # whole-float4 rows and a float4 action (the walker's widths); two row tiles, the second ragged
    "o27a4h72x44B37": (27, 4, 72, 44, 37),     # D1 = 32 fills the block; the action straddles a float4 and the lane halves; hidden % 32 != 0
    "o28a3h36x8B1": (28, 3, 36, 8, 1),         # float4 observations with an element-loaded action; one row
}
WALKER = "o24a4h64x48B37"
DQN_SHAPES = {
    "o11A3h52x36B37": (11, 3, 52, 36, 37),     # odd width; three actions; ragged
    "o13A8h64x48B1": (13, 8, 64, 48, 1),       # DDRL_DQN_DIRECT_MAX_OBS_DIM; most actions; one row
    "o8A4h64x48B64": (8, 4, 64, 48, 64),       # the lander's widths (_abi_contract.DSHAPE's): versions and the fused discrete rollout step
}
LANDER = "o8A4h64x48B64"
ACTOR_SHAPES = {                               # (obs, act, hidden1, hidden2, cfg.batch), max_rows, n of ddrl_actor_act
    "o24a4h64x48": ((24, 4, 64, 48, 32), 64, (1, 5, 33)),     # vector path; n = 33 leaves a one-row tile
    "o27a4h44x36": ((27, 4, 44, 36, 32), 64, (5, 33)),        # element path; D1 = 28
    "o13a1h36x8": ((13, 1, 36, 8, 32), 32, (32,)),            # first obs width past the narrow actor's envelope (obs + act > 12)
}
ACTOR_WALKER = "o24a4h64x48"
WINDOW_LN = 3

SAC_KINDS = {"sac1-wide": ("ddrl_sac1_create_wide", 0), "sacv-wide": ("ddrl_sacv_create_wide", 1)}
DQN_KINDS = {"ddqn-direct": 0, "sqn-direct": 1}


def sac_door(kind, shape):
    create, variant = SAC_KINDS[kind]
    return Door(create, SAC_SHAPES[shape], variant, "ddrl_sac1_is_wide")


def dqn_door(kind, shape):
    return Door("ddrl_dqn_create_direct", DQN_SHAPES[shape], DQN_KINDS[kind], "ddrl_dqn_is_direct")


def actor_door(shape):
    dims, rows, _ = ACTOR_SHAPES[shape]
    assert dims[0] + dims[1] > 12        # ddrl_actor_create would not hold this policy in a direct-operand layout
    return Door("ddrl_actor_create_wide", dims, 0, None, rows)


def _with(fn, door):
    return lambda ctx: fn(ctx, door=door)


# ---- what a refused call must leave alone ---------------------------------------------------------------------------------------------
def _same_when_over(ctx):
    """Registered before any handle exists, so that it runs last: every output `before.X` equals `after.X`, bit for bit."""
    def check():
        for k in [k for k in ctx.bufs if k.startswith("before.")]:
            a, b = ctx.tensor(k).view(torch.uint8), ctx.tensor("after." + k[7:]).view(torch.uint8)
            assert torch.equal(a, b), "the refused call changed `%s`" % k[7:]
    ctx.defer(check)


def _state(ctx, export, h, n, which=(0, 1, 2, 3)):
    """Closure parts: the handle's main, target, m and v (external order) into outputs before.exportW / after.exportW."""
    outs = {t: [(w, P(ctx.out("%s.export%d" % (t, w), n, F32))) for w in which] for t in ("before", "after")}
    return [lambda t=t: [_ok(ctx, export(h, w, p, ctx.stream_arg)) for w, p in outs[t]] for t in ("before", "after")]


def refusal(cid, kind, *functions):
    REFUSAL_CASES.append(cid)
    return case(cid, kind, *functions)


# ---- sac1-wide, sacv-wide ---------------------------------------------------------------------------------------------------------------
def _mk_grad_finalize(door):
    """ddrl_sac1_grad_finalize on a wide handle launches nothing (there are no row-tile partials on the direct paths) and is not refused:
    between two updates it must change nothing that the second one or the exports see."""
    def fn(ctx):
        L = ctx.lib
        h, n = ac._sac(ctx, None, door.variant, door=door)
        ins = [P(ctx.inp(k, x)) for k, x in ac._sac_batch(None, 31, door.dims)]
        losses = P(ctx.out("losses_d", 4 if door.variant else 3, F32))
        exp = [(w, P(ctx.out("export%d" % w, n, F32))) for w in (0, 1, 2, 3)]
        s = lambda: ctx.stream_arg
        return lambda: [L.ddrl_sac1_step(h, *ins, losses, None, None, None, s()), L.ddrl_sac1_grad_finalize(h, s()),
                        L.ddrl_sac1_step(h, *ins, losses, None, None, None, s())] + [L.ddrl_sac1_export(h, w, p, s()) for w, p in exp]
    return fn


def _mk_split_refused(door, which):
    """One update (setup), then the split-API call: DDRL_ERR_UNSUPPORTED, outputs and state untouched."""
    o, a, _, _, B = door.dims

    def fn(ctx):
        L = ctx.lib
        _same_when_over(ctx)
        h, n = ac._sac(ctx, None, door.variant, door=door)
        batch = ac._sac_batch(None, 31, door.dims)
        _ok(ctx, L.ddrl_sac1_step(h, *[_tp(ctx.tmp(x)) for _, x in batch], _tp(ctx.tmp(np.zeros(4, np.float32))), None, None, None, None))
        ring = ac._sac_ring(ctx, dims=door.dims)
        ctx.expect_rc = UNSUPPORTED
        before, after = _state(ctx, L.ddrl_sac1_export, h, n)
        s = lambda: ctx.stream_arg
        if which == "compute_grads":
            ins = [P(ctx.inp(k, x)) for k, x in batch]
            outs = [P(ctx.out("losses_d", 4 if door.variant else 3, F32, untouched=True))] + [
                P(ctx.out(k, B, F32, untouched=True)) for k in ("q1_d", "q2_d", "logp_pi_d")]
            refused = lambda: L.ddrl_sac1_compute_grads(h, *ins, *outs, s())
        elif which == "apply_grads":
            refused = lambda: L.ddrl_sac1_apply_grads(h, s())
        elif which == "compute_grads_and_sample":
            refused = lambda: L.ddrl_sac1_compute_grads_and_sample(h, 0, ring, 1, s())
        else:
            refused = lambda: L.ddrl_sac1_apply_grads_and_sample(h, ring, 1, s())

        def call():
            before()
            rc = refused()
            after()
            return rc
        return call
    return fn


for _k in SAC_KINDS:
    _v = SAC_KINDS[_k][1]
    for _s in SAC_SHAPES:
        _d = sac_door(_k, _s)
        case("%s:step-%s-rows" % (_k, _s), _k, "ddrl_sac1_step", "ddrl_sac1_export")(ac._mk_sac_step(None, _v, False, True, door=_d))
        case("%s:step-%s-rows_null" % (_k, _s), _k, "ddrl_sac1_step", "ddrl_sac1_export")(ac._mk_sac_step(None, _v, False, False, door=_d))
        case("%s:step_host-%s" % (_k, _s), _k, "ddrl_sac1_step_host")(ac._mk_sac_step_host(None, door=_d))
        for _m in ("get_weights", "set_weights") + tuple("export%d" % w for w in range(5)) + tuple("import%d" % w for w in range(4)):
            _f = {"g": "ddrl_sac1_get_weights", "s": "ddrl_sac1_set_weights", "e": "ddrl_sac1_export", "i": "ddrl_sac1_import"}[_m[0]]
            case("%s:%s-%s" % (_k, _m, _s), _k, _f)(ac._mk_sac_io(None, _v, _m, door=_d))
        stream_case("%s:step_and_sample-%s" % (_k, _s), _k, "ddrl_sac1_step_and_sample", "ddrl_sac1_fill_noise")(
            ac._mk_sac_and_sample("step_and_sample", door=_d))
        stream_case("%s:step_and_sample-%s-window_ring" % (_k, _s), _k, "ddrl_sac1_step_and_sample", "ddrl_sac1_fill_noise")(
            ac._mk_sac_and_sample("step_and_sample", door=_d, window=WINDOW_LN))
    for _s in ("o12a1h36x8B5", WALKER):
        _d = sac_door(_k, _s)
        stream_case("%s:opt_state_set_get_steps-%s" % (_k, _s), _k, "ddrl_sac1_opt_state_set", "ddrl_sac1_opt_state_get",
                    "ddrl_sac1_opt_steps")(_with(ac._opt_state, _d))
        stream_case("%s:graph_sync-%s" % (_k, _s), _k, "ddrl_sac1_graph_sync")(_with(ac._graph_sync, _d))
    for _s in (WALKER, "o27a4h72x44B37"):
        for _pg in (2, 3):
            stream_case("%s:loop_run-%s-per_graph%d" % (_k, _s, _pg), _k, "ddrl_loop_run")(ac._mk_loop_run(_pg, door=sac_door(_k, _s)))
    case("%s:grad_finalize-%s" % (_k, WALKER), _k, "ddrl_sac1_grad_finalize")(_mk_grad_finalize(sac_door(_k, WALKER)))
    for _w in ("compute_grads", "apply_grads", "compute_grads_and_sample", "apply_grads_and_sample"):
        refusal("%s:%s-refused" % (_k, _w), _k, "ddrl_sac1_" + _w)(_mk_split_refused(sac_door(_k, WALKER), _w))


# ---- ddqn-direct, sqn-direct ----------------------------------------------------------------------------------------------------------
def _mk_step_ring_refused(door):
    """ddrl_dqn_step_ring takes the wide layer-1 path only (obs_dim >= 1024): it refuses a direct handle as every narrow one."""
    o, A, _, _, B = door.dims

    def fn(ctx):
        L = ctx.lib
        _same_when_over(ctx)
        h, n, _ = ac._dqn(ctx, None, door=door)
        _ok(ctx, L.ddrl_dqn_step(h, *[_tp(ctx.tmp(x)) for _, x in ac._dqn_batch(None, 61, door.dims)], None, None, None))
        ring = ac._ring5(ctx, o, 1, 0, fill=37)
        ctx.expect_rc = UNSUPPORTED
        before, after = _state(ctx, L.ddrl_dqn_export, h, n)
        loss, q, idx = P(ctx.out("loss_d", 1, F32, untouched=True)), P(ctx.out("q_d", B * A, F32, untouched=True)), P(
            ctx.out("idx_out_d", B, I64, untouched=True))

        def call():
            before()
            rc = L.ddrl_dqn_step_ring(h, ring, loss, q, idx, ctx.stream_arg)
            after()
            return rc
        return call
    return fn


for _k, _v in DQN_KINDS.items():
    for _s, (_o, _A, _h1, _h2, _B) in DQN_SHAPES.items():
        _d = dqn_door(_k, _s)
        case("%s:step-%s" % (_k, _s), _k, "ddrl_dqn_step", "ddrl_dqn_export")(ac._mk_dqn_step(None, _v, True, door=_d))
        case("%s:step-%s-outputs_null" % (_k, _s), _k, "ddrl_dqn_step", "ddrl_dqn_export")(ac._mk_dqn_step(None, _v, False, door=_d))
        for _m in ("set_weights",) + tuple("export%d" % w for w in range(5)) + tuple("import%d" % w for w in range(4)):
            _f = {"s": "ddrl_dqn_set_weights", "e": "ddrl_dqn_export", "i": "ddrl_dqn_import"}[_m[0]]
            case("%s:%s-%s" % (_k, _m, _s), _k, _f)(ac._mk_dqn_io(None, _v, _m, door=_d))
        # the acting calls behind one update: the repack of the acting forward's operands (LANDER), the refreshed generic copy (the others)
        for _n in sorted({1, min(2, _B), max(1, _B - 1)}):
            case("%s:q-%s-n%d-after_update" % (_k, _s, _n), _k, "ddrl_dqn_q")(ac._mk_dqn_q(None, _v, _n, None, door=_d, updated=True))
            case("%s:act-%s-n%d-after_update" % (_k, _s, _n), _k, "ddrl_dqn_act")(ac._mk_dqn_q(None, _v, _n, "q", door=_d, updated=True))
        case("%s:act-%s-q_null-after_update" % (_k, _s), _k, "ddrl_dqn_act")(ac._mk_dqn_q(None, _v, min(2, _B), "noq", door=_d, updated=True))
    _d = dqn_door(_k, LANDER)
    case("%s:versions_adopt_and_state" % _k, _k, "ddrl_dqn_versions_adopt", "ddrl_dqn_versions_state")(_with(ac._dqn_versions, _d))
    stream_case("%s:versions_enable" % _k, _k, "ddrl_dqn_versions_enable")(_with(ac._dqn_enable, _d))
    for _n in (1, 2):
        case("%s:rollout_step_discrete-steps%d-all_mirrors" % (_k, _n), _k, "ddrl_rollout_step_discrete")(
            ac._mk_rollout_discrete(_v, _n, ("act", "q", "obs"), door=_d))
    case("%s:rollout_step_discrete-mirrors_null" % _k, _k, "ddrl_rollout_step_discrete")(ac._mk_rollout_discrete(_v, 1, (), door=_d))
    stream_case("%s:rollout_begin_discrete" % _k, _k, "ddrl_rollout_begin_discrete")(ac._mk_rollout_begin_discrete("one_body", door=_d))
    stream_case("%s:rollout_discrete_articulated" % _k, _k, "ddrl_rollout_begin_discrete_articulated",
                "ddrl_rollout_step_discrete_articulated")(ac._mk_rollout_begin_discrete("articulated", door=_d))
    for _m in ac.MODELS:
        stream_case("%s:env_eval_q-%s" % (_k, _m), _k, "ddrl_env_eval_q")(ac._mk_env_eval(_m, True, door=_d))
    for _s in ("o11A3h52x36B37", LANDER):
        _d = dqn_door(_k, _s)
        case("%s:loop-loss-%s" % (_k, _s), _k, "ddrl_dqn_loop_create")(ac._mk_dqn_loop(_v, True, door=_d))
        case("%s:loop-loss_null-%s" % (_k, _s), _k, "ddrl_dqn_loop_create")(ac._mk_dqn_loop(_v, False, door=_d))
        for _pg in (2, 3):
            stream_case("%s:loop_run-%s-per_graph%d" % (_k, _s, _pg), _k, "ddrl_dqn_loop_run")(ac._mk_dqn_loop_run(_pg, door=_d))
    refusal("%s:step_ring-refused" % _k, _k, "ddrl_dqn_step_ring")(_mk_step_ring_refused(dqn_door(_k, "o11A3h52x36B37")))


# ---- actor-wide -------------------------------------------------------------------------------------------------------------------------
def _mk_act_set_act(door):
    """act -> set_weights -> act: the second call acts through the row-major copy that the set_weights between them made stale, rebuilt
    under the arena."""
    o, a = door.dims[:2]
    n = 33

    def fn(ctx):
        L = ctx.lib
        h, n_pi = ac._actor(ctx, door=door)
        r = _rs(n)
        obs, eps = P(ctx.inp("obs_d", _f32(r.randn(n, o)), ma=True)), P(ctx.inp("eps_d", _f32(r.randn(n, a)), ma=True))
        src = P(ctx.inp("flat_pi_d", _weights(n_pi, 79), ma=True))
        a0, a1 = P(ctx.out("act_d(first)", n * a, F32)), P(ctx.out("act_d", n * a, F32, ma=True))
        s = lambda: ctx.stream_arg
        return lambda: [L.ddrl_actor_act(h, obs, eps, n, 0, a0, s()), L.ddrl_actor_set_weights(h, src, s()),
                        L.ddrl_actor_act(h, obs, eps, n, 0, a1, s())]
    return fn


def _mk_rollout_begin_refused(door, which):
    """The fused rollout entry points read the narrow layout: they refuse a wide actor, and leave its weights and the envs alone."""
    def fn(ctx):
        L = ctx.lib
        _same_when_over(ctx)
        env, fields = ac._env(ctx, ac.RN, "articulated" if which == "begin_articulated" else "one_body", max_ep_len=3)
        ac._env_warm(ctx, env, ac.RN)
        h, n_pi = ac._actor(ctx, door=door)
        st = {t: P(ctx.out("%s.state_d" % t, fields * ac.RN, F32)) for t in ("before", "after")}
        w = {t: P(ctx.out("%s.flat_pi_d" % t, n_pi, F32)) for t in ("before", "after")}
        s = lambda: ctx.stream_arg
        if which == "begin_nstep":
            q = ac._handle(ctx, L.ddrl_winq_destroy, L.ddrl_winq_create, ac._dev(ctx), ac.RN, 4, 8, 2, 1)
            ctx.expect_rc = UNSUPPORTED
            refused = lambda: L.ddrl_rollout_begin_nstep(env, h, q, s())
        elif which == "begin_articulated":
            ctx.expect_rc = UNSUPPORTED
            refused = lambda: L.ddrl_rollout_begin_articulated(env, h, s())
        else:
            ctx.expect_rc = BAD_ARG       # the one-body pair's envelope answers DDRL_ERR_BAD_ARG (csrc/env.hip: rollout_check)
            refused = lambda: L.ddrl_rollout_begin(env, h, s())

        def both(t):
            _ok(ctx, L.ddrl_env_get_state(env, st[t], s()))
            _ok(ctx, L.ddrl_actor_get_weights(h, w[t], s()))

        def call():
            both("before")
            rc = refused()
            both("after")
            return rc
        return call
    return fn


def _mk_eval_policy_refused(door):
    """ddrl_env_eval_policy plays the lander: DDRL_ERR_BAD_ARG for an actor that is not 8 -> 2, which every shape outside the narrow
    actor's envelope is; nothing launched, allocated or changed."""
    def fn(ctx):
        L = ctx.lib
        _same_when_over(ctx)
        env, fields = ac._env(ctx, 1, "one_body", seed=5, max_ep_len=ac.EP_LEN)
        h, n_pi = ac._actor(ctx, door=door)
        ctx.expect_rc = BAD_ARG
        st = {t: P(ctx.out("%s.state_d" % t, fields, F32)) for t in ("before", "after")}
        w = {t: P(ctx.out("%s.flat_pi_d" % t, n_pi, F32)) for t in ("before", "after")}
        s = lambda: ctx.stream_arg

        def both(t):
            _ok(ctx, L.ddrl_env_get_state(env, st[t], s()))
            _ok(ctx, L.ddrl_actor_get_weights(h, w[t], s()))

        def call():
            both("before")
            rc = L.ddrl_env_eval_policy(env, h, ac.EPISODES, 2, 1, s())
            both("after")
            return rc
        return call
    return fn


_K = "actor-wide"
for _s, (_dims, _rows, _ns) in ACTOR_SHAPES.items():
    _d = actor_door(_s)
    for _n in _ns:
        case("%s:act-%s-n%d" % (_K, _s, _n), _K, "ddrl_actor_act")(ac._mk_actor_act(None, _n, 0, door=_d))
    case("%s:act-%s-deterministic" % (_K, _s), _K, "ddrl_actor_act")(ac._mk_actor_act(None, _ns[0], 1, door=_d))
    case("%s:act_one-%s" % (_K, _s), _K, "ddrl_actor_act_one")(ac._mk_actor_one(None, 0, door=_d))
    case("%s:set_weights-%s" % (_K, _s), _K, "ddrl_actor_set_weights", "ddrl_actor_get_weights")(ac._mk_actor_weights(True, door=_d))
    case("%s:get_weights-%s" % (_K, _s), _K, "ddrl_actor_get_weights")(ac._mk_actor_weights(False, door=_d))
case("%s:act_one-deterministic" % _K, _K, "ddrl_actor_act_one")(ac._mk_actor_one(None, 1, door=actor_door(ACTOR_WALKER)))
for _s in (ACTOR_WALKER, "o27a4h44x36"):      # (max_rows 64: envs 0, 3 and 40 adopt)
    _d = actor_door(_s)
    case("%s:act_versioned-%s" % (_K, _s), _K, "ddrl_actor_act_versioned")(_with(ac._act_versioned, _d))
    case("%s:versions_adopt_and_state-%s" % (_K, _s), _K, "ddrl_actor_versions_adopt", "ddrl_actor_versions_state")(
        _with(ac._versions_adopt, _d))
    stream_case("%s:versions_enable-%s" % (_K, _s), _K, "ddrl_actor_versions_enable")(_with(ac._actor_enable, _d))
    case("%s:act-set_weights-act-%s" % (_K, _s), _K, "ddrl_actor_act", "ddrl_actor_set_weights")(_mk_act_set_act(_d))
for _w, _f in (("begin", "ddrl_rollout_begin"), ("begin_articulated", "ddrl_rollout_begin_articulated"),
               ("begin_nstep", "ddrl_rollout_begin_nstep")):
    refusal("%s:rollout_%s-refused" % (_K, _w), _K, _f)(_mk_rollout_begin_refused(actor_door(ACTOR_WALKER), _w))
refusal("%s:env_eval_policy-refused" % _K, _K, "ddrl_env_eval_policy")(_mk_eval_policy_refused(actor_door(ACTOR_WALKER)))
# ... and accepts the one wide actor that is 8 -> 2 (inside ddrl_actor_create's envelope too: here the creator's return code alone says
# which layout holds the policy); the evaluation reads it through ddrl_actor_get_weights, the wide unpack
_LANDER_ACTOR = Door("ddrl_actor_create_wide", (8, 2, 64, 48, 32), 0, None, 64)
for _m in ac.MODELS:
    stream_case("%s:env_eval_policy-%s-o8a2" % (_K, _m), _K, "ddrl_env_eval_policy")(ac._mk_env_eval(_m, False, door=_LANDER_ACTOR))


# ---- what has no row, and why ---------------------------------------------------------------------------------------------------------
EXEMPT = {}
for _k in SAC_KINDS:
    EXEMPT[(_k, "ddrl_sac1_grad_buffer")] = "returns an address, writes no device memory"
    EXEMPT[(_k, "ddrl_sac1_input_buffers")] = "returns addresses, writes no device memory (the step_and_sample rows read through them)"
    EXEMPT[(_k, "ddrl_sac1_stage_time")] = "profiling entry with a host output; the kernels of ddrl_sac1_step, which has a row"
for _k in DQN_KINDS:
    EXEMPT[(_k, "ddrl_dqn_step_timed")] = "profiling entry with host outputs; it refuses a direct handle (its stage list is the generic launches')"
_STEP_WHY = "takes an actor that its begin call has accepted; the begin call refuses a wide actor and has a refusal row"
for _f in ("ddrl_rollout_step", "ddrl_rollout_step_articulated", "ddrl_rollout_step_nstep", "ddrl_rollout_step_nstep_articulated"):
    EXEMPT[(_K, _f)] = _STEP_WHY
EXEMPT[(_K, "ddrl_rollout_begin_nstep_articulated")] = "the envelope check of ddrl_rollout_begin_nstep, which has a refusal row, on the other env model"
