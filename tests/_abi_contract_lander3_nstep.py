"""The memory-contract rows of the n-step worker's three entry points on the ARTICULATED lander — ddrl_env_step_wrapped_articulated,
ddrl_rollout_begin_nstep_articulated (handles only: no row), ddrl_rollout_step_nstep_articulated — beside tests/_abi_contract.py,
whose case builders, shapes and helpers it uses.  CASES / REFUSALS have that module's form and stay here:
tests/test_gpu_abi_lander3_nstep.py runs them between guard bands (tests/_abi_arena.run_case), so tests/test_gpu_abi_memory.py's
parametrisation over _abi_contract.CASES does not depend on whether this module has been imported.
The ROWS are different: importing this module enters them in _abi_contract.TABLE, the one table tests/test_abi_table_cpu.py parses the
header against.  _abi_contract.py itself holds no row for the two functions, so that check finds them only once this module has been
imported — which every collection of the suite does (tests/test_gpu_abi_lander3_nstep.py, tests/test_lander3_wrapped_cpu.py and, for
the stream table, tests/test_abi_table_cpu.py itself import it).
tests/test_lander3_wrapped_cpu.py repeats the header check with this module imported, whatever else was collected.
The closures hand the call under test ctx.stream_arg: tests/test_gpu_abi_stream.py runs these cases on a side stream as well; the
stream row of ddrl_rollout_begin_nstep_articulated stands with the other begin calls' in _abi_contract.STREAM_CASES."""
from ctypes import byref, c_void_p as P

import torch

import _abi_contract as ac

F32, U8 = torch.float32, torch.uint8

CASES = {}   # id -> (fn, (functions covered))
TABLE = {}   # function -> [case ids]: this module's rows (also entered in ac.TABLE)


def case(cid, *functions):
    def deco(fn):
        assert cid not in CASES and cid not in ac.CASES, cid
        CASES[cid] = (fn, functions)
        for f in functions:
            TABLE.setdefault(f, []).append(cid)
            ac.TABLE.setdefault(f, []).append(cid)    # the row, where tests/test_abi_table_cpu.py looks for it
        return fn
    return deco


def _mk_env_step_wrapped(n, present):
    """ac._mk_env_step(.., "wrapped", ..) on an articulated handle: max_ep_len 2 and one step taken, limit 2 — every env goes through
    its reset; act_d is an input the call modifies."""
    def fn(ctx):
        L = ctx.lib
        h, fields = ac._env(ctx, n, "articulated")
        ac._env_warm(ctx, h, n)
        act = ctx.inp("act_d", ac._f32(ac._rs(2).uniform(-1.2, 1.2, (n, 2))), modified=True)
        outs = ac._env_outs(ctx, n, present)
        st = P(ctx.out("state_d", fields * n, F32))
        return lambda: [L.ddrl_env_step_wrapped_articulated(h, P(act), 0.3, 0.1, 5.0, 2, 2, *outs, ctx.stream_arg), L.ddrl_env_get_state(h, st, ctx.stream_arg)]
    return fn


for _n in ac.ENV_N:
    for _p in (True, False):
        case("env_step_wrapped_articulated-n%d%s" % (_n, "" if _p else "-outputs_null"),
             "ddrl_env_step_wrapped_articulated")(_mk_env_step_wrapped(_n, _p))


def _mk_rollout_nstep(n_steps, present):
    """ac._mk_rollout_nstep on an articulated handle (4 / 2 iterations, ac.MODELS)."""
    Ln = 4

    def fn(ctx):
        from distributed_drl_amd import _lib
        L = ctx.lib
        h, fields = ac._env(ctx, ac.RN, "articulated", max_ep_len=1 << 20)
        a, _ = ac._actor(ctx)
        ring = ac._wring(ctx, Ln, 8, cap=ac.RCAP)
        q = ac._handle(ctx, L.ddrl_winq_destroy, L.ddrl_winq_create, ac._dev(ctx), ac.RN, Ln, 8, 2, 1)
        obs = ctx.tmp(torch.empty(ac.RN * 8, dtype=torch.float32))
        ac._ok(ctx, L.ddrl_env_reset(h, None, ac._tp(obs), None))
        ac._ok(ctx, L.ddrl_winq_begin(q, None, ac._tp(obs), None))
        ac._ok(ctx, L.ddrl_rollout_begin_nstep_articulated(h, a, q, None))
        args = (0.3, 0.1, 5.0, 2, 3, 0, 5)
        ac._ok(ctx, L.ddrl_rollout_step_nstep_articulated(h, a, q, ring, 4, *args, 0, None, None))   # four steps: full windows, episode ends
        names = (("act", 2, F32), ("obs2", 8, F32), ("rew", 1, F32), ("done", 1, F32), ("next_obs", 8, F32), ("ended", 1, U8))
        out = ctx.keep(_lib.RolloutNStepOut(*[P(ctx.out("out->" + k, ac.RN * w, t)) if k in present else None for k, w, t in names]))
        st = P(ctx.out("state_d", fields * ac.RN, F32))
        exp = ac._export5(ctx, ring, ac._wwidths(Ln, 8), ac.RCAP)
        return lambda: [L.ddrl_rollout_step_nstep_articulated(h, a, q, ring, n_steps, *args, 4000, byref(out) if present else None, ctx.stream_arg),
                        L.ddrl_env_get_state(h, st, ctx.stream_arg)] + exp()
    return fn


_ALL6 = ac._ALL6
for _k in (1, 2):
    case("rollout_step_nstep_articulated-steps%d-all_mirrors" % _k, "ddrl_rollout_step_nstep_articulated")(_mk_rollout_nstep(_k, _ALL6))
    case("rollout_step_nstep_articulated-steps%d-out_null" % _k, "ddrl_rollout_step_nstep_articulated")(_mk_rollout_nstep(_k, ()))
for _one in _ALL6:
    case("rollout_step_nstep_articulated-only_%s" % _one, "ddrl_rollout_step_nstep_articulated")(_mk_rollout_nstep(1, (_one,)))
    case("rollout_step_nstep_articulated-without_%s" % _one,
         "ddrl_rollout_step_nstep_articulated")(_mk_rollout_nstep(1, tuple(k for k in _ALL6 if k != _one)))

# (function, pointer named by ddrl_last_error()): refused one float off its grid, on the host (tests/test_gpu_lander3_wrapped.py and
# tests/test_gpu_abi_lander3_nstep.py make the calls)
REFUSALS = [
    ("ddrl_env_step_wrapped_articulated", "act_d"), ("ddrl_env_step_wrapped_articulated", "obs2_d"),
    ("ddrl_env_step_wrapped_articulated", "next_obs_d"),
    ("ddrl_rollout_step_nstep_articulated", "out->act"), ("ddrl_rollout_step_nstep_articulated", "out->obs2"),
    ("ddrl_rollout_step_nstep_articulated", "out->next_obs"),
]
