"""The memory-contract rows of include/ddrl_walker_hardcore.h — ddrl_env_create_walker and what its Hardcore handle changes behind
the entry points of include/ddrl.h and include/ddrl_walker.h — beside tests/_abi_contract.py, whose helpers it uses.  CASES / TABLE /
REFUSALS have the form of tests/_abi_contract_walker_nstep.py and stay here: tests/test_gpu_abi_walker_hardcore.py runs the cases
between guard bands and on a side stream.  Like that module this one enters NO row in _abi_contract.TABLE, which is parsed against
include/ddrl.h.  The header's one declaration takes neither caller device memory nor a stream, so tests/test_abi_table_cpu.py's parse
finds nothing uncovered in it whatever stands here; what the header changes is the KERNELS behind ddrl_env_reset, ddrl_env_step and
ddrl_env_step_wrapped_walker on a handle it creates, and the block size of ddrl_env_get_state / ddrl_env_set_state.  TABLE's one row
is the header's function; its cases create a handle through it and hold those entry points to the contract on it
(tests/test_walker_hardcore_cpu.py: every key of TABLE is a declaration of the header, every case is in a row).
The closures hand the call under test ctx.stream_arg."""
from ctypes import c_void_p as P

import torch

import _abi_contract as ac

F32, U8 = torch.float32, torch.uint8
WOBS, WACT = 24, 4
ITERATIONS = (4, 2)
CREATE = "ddrl_env_create_walker"

CASES = {}   # id -> (fn, (functions covered))
TABLE = {}   # function -> [case ids]: the rows of include/ddrl_walker_hardcore.h


def case(cid, *functions):
    def deco(fn):
        assert cid not in CASES and cid not in ac.CASES and cid not in ac.STREAM_CASES, cid
        CASES[cid] = (fn, functions)
        for f in functions:
            TABLE.setdefault(f, []).append(cid)
        return fn
    return deco


def _walker(ctx, n, seed=7, max_ep_len=2):
    """A Hardcore handle: max_ep_len 2 and one step taken (_warm), so the step under test ends every env's episode."""
    from distributed_drl_amd import _lib
    L = ctx.lib
    h = ac._handle(ctx, L.ddrl_env_destroy, L.ddrl_env_create_walker, ac._dev(ctx), n, seed, max_ep_len, *ITERATIONS,
                   _lib.DDRL_WALKER_TERRAIN_HARDCORE)
    fields = L.ddrl_env_state_fields(h)
    assert fields == _lib.DDRL_ENVWH_STATE_FIELDS
    return h, fields


def _warm(ctx, h, n):
    ac._ok(ctx, ctx.lib.ddrl_env_step(h, ac._tp(ctx.tmp(ac._f32(ac._rs(1).uniform(-1, 1, (n, WACT))))), None, None, None, None, None, None))


def _outs(ctx, n, present):
    names = (("obs2_d", n * WOBS, F32), ("rew_d", n, F32), ("done_d", n, F32), ("next_obs_d", n * WOBS, F32), ("ended_d", n, U8))
    return [P(ctx.out(k, cnt, t)) if present else None for k, cnt, t in names]


def _mk_step(n, kind, present):
    """kind "step": ddrl_env_step at the time limit (every env resets: terrain generator, box table, the zero-action trip);
    "wrapped": ddrl_env_step_wrapped_walker likewise, act_d an input the call modifies; "reset": a masked ddrl_env_reset.
    The state block is read back through ddrl_env_get_state at the handle's own size."""
    def fn(ctx):
        L = ctx.lib
        h, fields = _walker(ctx, n)
        _warm(ctx, h, n)
        st = P(ctx.out("state_d", fields * n, F32))
        if kind == "reset":
            mask = ctx.inp("mask_d", (ac._rs(3).rand(n) < 0.5).astype("uint8"))
            obs = P(ctx.out("obs_d", n * WOBS, F32)) if present else None
            return lambda: [L.ddrl_env_reset(h, P(mask), obs, ctx.stream_arg), L.ddrl_env_get_state(h, st, ctx.stream_arg)]
        outs = _outs(ctx, n, present)
        if kind == "step":
            act = ctx.inp("act_d", ac._f32(ac._rs(2).uniform(-1.2, 1.2, (n, WACT))))
            return lambda: [L.ddrl_env_step(h, P(act), *outs, ctx.stream_arg), L.ddrl_env_get_state(h, st, ctx.stream_arg)]
        act = ctx.inp("act_d", ac._f32(ac._rs(2).uniform(-1.2, 1.2, (n, WACT))), modified=True)
        return lambda: [L.ddrl_env_step_wrapped_walker(h, P(act), 0.3, 0.1, 5.0, 2, 2, *outs, ctx.stream_arg),
                        L.ddrl_env_get_state(h, st, ctx.stream_arg)]
    return fn


def _mk_set_state(n):
    """ddrl_env_set_state of a block of the handle's size, read back."""
    def fn(ctx):
        L = ctx.lib
        h, fields = _walker(ctx, n)
        src, _ = _walker(ctx, n, seed=8)
        blk = ctx.tmp(ac._f32(ac._rs(4).rand(fields * n)))
        ac._ok(ctx, L.ddrl_env_get_state(src, ac._tp(blk), None))
        ctx.sync()
        inp = ctx.inp("state_d", blk.cpu().numpy())
        back = P(ctx.out("state_back_d", fields * n, F32))
        return lambda: [L.ddrl_env_set_state(h, P(inp), ctx.stream_arg), L.ddrl_env_get_state(h, back, ctx.stream_arg)]
    return fn


for _n in ac.ENV_N:
    for _kind in ("step", "wrapped", "reset"):
        case("hardcore_%s-n%d" % (_kind, _n), CREATE)(_mk_step(_n, _kind, True))
case("hardcore_step-n33-outputs_null", CREATE)(_mk_step(33, "step", False))
case("hardcore_wrapped-n33-outputs_null", CREATE)(_mk_step(33, "wrapped", False))
case("hardcore_set_state-n33", CREATE)(_mk_set_state(33))

# (function, pointer named by ddrl_last_error()): refused one float off its grid on a Hardcore handle, on the host
# (tests/test_gpu_walker_hardcore.py makes the calls)
REFUSALS = [
    ("ddrl_env_step", "act_d"), ("ddrl_env_step", "obs2_d"), ("ddrl_env_step", "next_obs_d"), ("ddrl_env_reset", "obs_d"),
    ("ddrl_env_step_wrapped_walker", "act_d"), ("ddrl_env_step_wrapped_walker", "obs2_d"), ("ddrl_env_step_wrapped_walker", "next_obs_d"),
]
