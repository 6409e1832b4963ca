"""The stream-contract row of the Hardcore walker's evaluation entry point — ddrl_env_eval_policy_walker_hardcore, declared in
include/ddrl_walker_hardcore_eval.h — beside tests/_abi_contract.py, whose helpers it uses, in the form of
tests/_abi_contract_walker_eval.py (the grass twin's row): STREAM_CASES / TABLE stay here, and tests/test_gpu_walker_hardcore_eval.py
runs the case on a side stream.  The function takes handles and a stream and no caller device memory, so its row is a stream row only,
and this module enters NO row in _abi_contract's tables: those are parsed against include/ddrl.h, which does not declare this function.
TABLE below is the table of include/ddrl_walker_hardcore_eval.h, and tests/test_walker_hardcore_eval_cpu.py holds that header to it with
tests/test_abi_table_cpu.py's parse.

The case is _abi_contract_walker_eval's on a Hardcore walker handle (ddrl_env_create_walker, terrain = DDRL_WALKER_TERRAIN_HARDCORE)
with that module's 24 -> 4 actor: the results live in a block of the env handle (ddrl_env_eval_results) and are copied out; a first
evaluation of the same size (setup) has allocated that block, so that the call under test only launches.  Call ahead, on the same
stream, which does not commute with the call under test: a ddrl_actor_set_weights of the actor the episodes are played with — a launch
off its stream would read the weights of the setup."""
from ctypes import byref, c_int32, c_void_p as P

import _abi_contract as ac
import _abi_contract_walker_eval as ae

F32, F64, I32 = ae.F32, ae.F64, ae.I32
ROW, ITERATIONS, EPISODES, EP_LEN = ae.ROW, ae.ITERATIONS, ae.EPISODES, ae.EP_LEN
NAME = "ddrl_env_eval_policy_walker_hardcore"

STREAM_CASES = {}   # id -> (fn, (functions covered))
TABLE = {}          # function -> [case ids]: the rows of include/ddrl_walker_hardcore_eval.h


def stream_case(cid, *functions):
    def deco(fn):
        assert cid not in STREAM_CASES and cid not in ac.CASES and cid not in ac.STREAM_CASES and cid not in ae.STREAM_CASES, cid
        STREAM_CASES[cid] = (fn, functions)
        for f in functions:
            TABLE.setdefault(f, []).append(cid)
        return fn
    return deco


def _walker_hardcore(ctx, seed=5, max_ep_len=EP_LEN):
    from distributed_drl_amd import _lib
    L = ctx.lib
    return ac._handle(ctx, L.ddrl_env_destroy, L.ddrl_env_create_walker, ac._dev(ctx), 1, seed, max_ep_len, *ITERATIONS,
                      _lib.DDRL_WALKER_TERRAIN_HARDCORE)


@stream_case("env_eval_policy_walker_hardcore", NAME)
def _env_eval_policy_walker_hardcore(ctx):
    L = ctx.lib
    h = _walker_hardcore(ctx)
    src, n = ae._walker_actor(ctx)
    flat = P(ctx.inp("ahead.flat_d", ac._weights(n, 58)))
    s = lambda: ctx.stream_arg
    ev = lambda first, st: L.ddrl_env_eval_policy_walker_hardcore(h, src, EPISODES, first, 1, st)
    ac._ok(ctx, ev(0, None))
    ctx.out("ret", EPISODES, F64), ctx.out("len", EPISODES, I32), ctx.out("trace", EPISODES * EP_LEN * ROW, F32)

    def call():
        rc = [L.ddrl_actor_set_weights(src, flat, s()), ev(2, s())]
        ret, ln, tr = P(), P(), P()
        ne, ml, tw = c_int32(), c_int32(), c_int32()
        ac._ok(ctx, L.ddrl_env_eval_results(h, byref(ret), byref(ln), byref(tr), byref(ne), byref(ml), byref(tw)))
        assert (ne.value, ml.value, tw.value) == (EPISODES, EP_LEN, ROW), (ne.value, ml.value, tw.value)
        ac._copy_out(ctx, "ret", ret.value, 2 * EPISODES)
        ac._copy_out(ctx, "len", ln.value, EPISODES)
        ac._copy_out(ctx, "trace", tr.value, EPISODES * EP_LEN * ROW)
        return rc
    return call
