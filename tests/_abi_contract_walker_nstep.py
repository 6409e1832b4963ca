"""The memory-contract rows of the n-step worker's entry point on the WALKER — ddrl_env_step_wrapped_walker, declared in
include/ddrl_walker.h — beside tests/_abi_contract.py, whose helpers it uses.  CASES / TABLE / REFUSALS have the form of
tests/_abi_contract_lander3_nstep.py and stay here: tests/test_gpu_abi_walker_nstep.py runs the cases between guard bands and on a
side stream.  Unlike that module this one enters NO row in _abi_contract.TABLE: that table is parsed against include/ddrl.h
(tests/test_abi_table_cpu.py), which does not declare this function — a row there would be a row for a function that header does
not have.  TABLE below is the table of include/ddrl_walker.h, and tests/test_walker_wrapped_cpu.py holds that header to it with the
same parse: every declaration with caller device memory or a stream has a row here, and no row is for a function it lacks.  So
the checks of both headers pass whichever test files are collected.
_abi_contract.MODELS has no walker, so the env helper is this module's own: [n,24] observations, [n,4] actions, 4 / 2 iterations.
The closures hand the call under test ctx.stream_arg."""
from ctypes import byref, c_void_p as P

import torch

import _abi_contract as ac

F32, U8 = torch.float32, torch.uint8
WOBS, WACT = 24, 4
ITERATIONS = (4, 2)

CASES = {}   # id -> (fn, (functions covered))
TABLE = {}   # function -> [case ids]: the rows of include/ddrl_walker.h


def case(cid, *functions):
    def deco(fn):
        assert cid not in CASES and cid not in ac.CASES and cid not in ac.STREAM_CASES, cid
        CASES[cid] = (fn, functions)
        for f in functions:
            TABLE.setdefault(f, []).append(cid)
        return fn
    return deco


def _walker(ctx, n, seed=7, max_ep_len=2):
    """ac._env for the walker: max_ep_len 2 and one step taken (_walker_warm), so the step under test ends every env's episode."""
    from distributed_drl_amd import _lib
    L = ctx.lib
    em = _lib.EnvModel(_lib.DDRL_ENV_WALKER, *ITERATIONS)
    h = ac._handle(ctx, L.ddrl_env_destroy, L.ddrl_env_create_ex, ac._dev(ctx), n, seed, max_ep_len, byref(em))
    return h, L.ddrl_env_state_fields(h)


def _walker_warm(ctx, h, n):
    ac._ok(ctx, ctx.lib.ddrl_env_step(h, ac._tp(ctx.tmp(ac._f32(ac._rs(1).uniform(-1, 1, (n, WACT))))), None, None, None, None, None, None))


def _walker_outs(ctx, n, present):
    """present: True (all five), False (all NULL) or the name of the one output that is given."""
    names = (("obs2_d", n * WOBS, F32), ("rew_d", n, F32), ("done_d", n, F32), ("next_obs_d", n * WOBS, F32), ("ended_d", n, U8))
    return [P(ctx.out(k, cnt, t)) if present is True or present == k else None for k, cnt, t in names]


def _mk_env_step_wrapped(n, present):
    """ac._mk_env_step(.., "wrapped", ..) on a walker handle: one step taken, limit 2 — every env goes through its reset (build, the
    zero-action trip, the second observation); act_d is an input the call modifies."""
    def fn(ctx):
        L = ctx.lib
        h, fields = _walker(ctx, n)
        _walker_warm(ctx, h, n)
        act = ctx.inp("act_d", ac._f32(ac._rs(2).uniform(-1.2, 1.2, (n, WACT))), modified=True)
        outs = _walker_outs(ctx, n, present)
        st = P(ctx.out("state_d", fields * n, F32))
        return lambda: [L.ddrl_env_step_wrapped_walker(h, P(act), 0.3, 0.1, 5.0, 2, 2, *outs, ctx.stream_arg),
                        L.ddrl_env_get_state(h, st, ctx.stream_arg)]
    return fn


for _n in ac.ENV_N:
    for _p in (True, False):
        case("env_step_wrapped_walker-n%d%s" % (_n, "" if _p else "-outputs_null"),
             "ddrl_env_step_wrapped_walker")(_mk_env_step_wrapped(_n, _p))
case("env_step_wrapped_walker-n33-only_next_obs", "ddrl_env_step_wrapped_walker")(_mk_env_step_wrapped(33, "next_obs_d"))

# (function, pointer named by ddrl_last_error()): refused one float off its grid, on the host (tests/test_gpu_walker_wrapped.py makes
# the calls)
REFUSALS = [
    ("ddrl_env_step_wrapped_walker", "act_d"), ("ddrl_env_step_wrapped_walker", "obs2_d"), ("ddrl_env_step_wrapped_walker", "next_obs_d"),
]
