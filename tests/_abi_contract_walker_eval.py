"""The stream-contract row of the walker's evaluation entry point — ddrl_env_eval_policy_walker, declared in
include/ddrl_walker_eval.h — beside tests/_abi_contract.py, whose helpers it uses.  STREAM_CASES / TABLE have the form of
tests/_abi_contract_walker_nstep.py and stay here: tests/test_gpu_abi_walker_eval.py runs the case on a side stream.  The function
takes handles and a stream and no caller device memory, so — as ddrl_env_eval_policy in tests/_abi_contract.py — its row is a stream
row only, and like tests/_abi_contract_walker_nstep.py this module enters NO row in _abi_contract's tables: those are parsed against
include/ddrl.h, which does not declare this function.  TABLE below is the table of include/ddrl_walker_eval.h, and
tests/test_walker_eval_cpu.py holds that header to it with tests/test_abi_table_cpu.py's parse.

The case is _abi_contract._mk_env_eval on a walker handle and a 24 -> 4 actor: the results live in a block of the env handle
(ddrl_env_eval_results) and are copied out; a first evaluation of the same size (setup) has allocated that block, so that the call
under test only launches.  Call ahead, on the same stream, which does not commute with the call under test: a ddrl_actor_set_weights
of the actor the episodes are played with — a launch off its stream would read the weights of the setup."""
from ctypes import byref, c_int32, c_void_p as P

import torch

import _abi_contract as ac

F32, F64, I32 = torch.float32, torch.float64, torch.int32
WOBS, WACT, ROW = 24, 4, 32
HID = (64, 48)
ITERATIONS = (4, 2)
EPISODES, EP_LEN = 3, 6

STREAM_CASES = {}   # id -> (fn, (functions covered))
TABLE = {}          # function -> [case ids]: the rows of include/ddrl_walker_eval.h


def stream_case(cid, *functions):
    def deco(fn):
        assert cid not in STREAM_CASES and cid not in ac.CASES and cid not in ac.STREAM_CASES, cid
        STREAM_CASES[cid] = (fn, functions)
        for f in functions:
            TABLE.setdefault(f, []).append(cid)
        return fn
    return deco


def _walker(ctx, seed=5, max_ep_len=EP_LEN):
    from distributed_drl_amd import _lib
    L = ctx.lib
    em = _lib.EnvModel(_lib.DDRL_ENV_WALKER, *ITERATIONS)
    return ac._handle(ctx, L.ddrl_env_destroy, L.ddrl_env_create_ex, ac._dev(ctx), 1, seed, max_ep_len, byref(em))


def _walker_actor(ctx, seed=41):
    from distributed_drl_amd import _lib
    L = ctx.lib
    cfg = _lib.Sac1Config(obs_dim=WOBS, act_dim=WACT, hidden1=HID[0], hidden2=HID[1], batch=37, variant=0, lr=1e-3)
    h = ac._handle(ctx, L.ddrl_actor_destroy, L.ddrl_actor_create, ac._dev(ctx), byref(cfg), 1)
    n_pi = ac._sac_counts(WOBS, WACT, HID[0], HID[1], 0)[0]
    ac._ok(ctx, L.ddrl_actor_set_weights(h, ac._tp(ctx.tmp(ac._weights(n_pi, seed))), None))
    return h, n_pi


@stream_case("env_eval_policy_walker", "ddrl_env_eval_policy_walker")
def _env_eval_policy_walker(ctx):
    L = ctx.lib
    h = _walker(ctx)
    src, n = _walker_actor(ctx)
    flat = P(ctx.inp("ahead.flat_d", ac._weights(n, 58)))
    s = lambda: ctx.stream_arg
    ev = lambda first, st: L.ddrl_env_eval_policy_walker(h, src, EPISODES, first, 1, st)
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
