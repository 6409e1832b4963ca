"""GPU: the C-ABI's stream contract (include/ddrl.h, "Conventions": `stream` is a hipStream_t ... all device work is enqueued on it;
no call synchronises the device except where documented; inputs are borrowed until the stream reaches the enqueued work).
Every case of the memory-contract table (tests/_abi_contract.py, tests/_abi_contract_lander3_nstep.py) and the rows of the functions
that take a stream and no caller device memory (STREAM_CASES) runs once more between guard bands, on a non-blocking side stream whose
inputs still hold decoys while a bounded gate holds the stream (tests/_abi_arena.py, "S"): work that did not go to the caller's stream
reads the decoys or is erased by the late sentinel (S-early), work left on another stream has not landed when the caller's stream is
synchronised (S-late), a host output read behind a sync of the wrong stream is stale (S-sync).  A call that touches handle memory only
has a call fed from a late-written input ahead of it in its closure, one it does not commute with (tests/_abi_contract.py, "call
ahead"): run during the gate, it acted on the state from before that call.  tests/test_abi_table_cpu.py shows on a CPU model of streams
that each of these is reported, and by that name, and that a handle-only call off its stream is reported only behind such a call.

The gate.  The slowest call of any case, timed between two events on the default stream on the build of the commit before this
suite existed: 6.084 ms, the closure of ddqn_loop-loss (ddrl_dqn_loop_run with the process's first graph capture; the next ones:
env_eval_policy-articulated 3.187 ms, dqn_loop_run-per_graph3 1.349 ms, loop_run-per_graph3 1.282 ms; everything else below 1 ms).
The gate is the larger of 10 ms and 10 x that value, 60.84 ms: a wrongly placed launch has only to start and finish inside it.
Every run measures its own gate with events; one that came out shorter fails as VOID.

A handle is ready when `create` returns (second half): the gate sits on the NULL stream while the creator runs, so whatever the
creator left unfinished there is stuck behind it, and the handle is used at once on the side stream."""
import ctypes
import os
import sys
from ctypes import byref, c_void_p as P

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_arena as aa   # noqa: E402
import _abi_contract as ac   # noqa: E402
import _abi_contract_lander3_nstep as ac3   # noqa: E402

SLOWEST_CALL_MS = 6.084
GATE_MS = max(10.0, 10.0 * SLOWEST_CALL_MS)

ALL_CASES = {}
for _d in (ac.CASES, ac3.CASES, ac.STREAM_CASES):
    for _k, _v in _d.items():
        assert _k not in ALL_CASES, _k
        ALL_CASES[_k] = _v


@pytest.fixture(scope="module")
def lib():
    from distributed_drl_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return _lib.load()


S_RUNS, VOID_RUNS = [], []      # every S run of this session, and those that came out void (case id, what the run reported)
MAX_VOID_SHARE = 0.05


@pytest.mark.parametrize("cid", sorted(ALL_CASES))
def test_stream_contract(lib, cid):
    try:
        # A run that is void and nothing else (the gate came out short, or it held the null stream too: the runtime's mapping of
        # streams onto hardware queues is not fixed for the life of a process) is made again, twice at the most, with fresh handles;
        # a third void run fails as void.  A void run never passes, any other failure is reported at once, and every void run is
        # counted: test_void_runs_stay_rare holds the session's total to a bound.
        for _ in range(3):
            checks = aa.run_stream_case(cid, ALL_CASES[cid][0], "cuda:0", lib, aa.TorchSide("cuda:0", GATE_MS))
            S_RUNS.append(cid)
            if checks.props() != ["VOID"]:
                break
            VOID_RUNS.append((cid, checks.failed))
            print("void run of %s: %s" % (cid, checks.failed))
    except RuntimeError as e:   # a HIP error out of torch (a fault is sticky: nothing that follows in this process would mean anything)
        pytest.exit("the device reported an error in case %s: %s" % (cid, e), returncode=3)
    if any(p == "RC" and "returned -3," in w for p, w in checks.failed):   # DDRL_ERR_HIP
        pytest.exit("the library reported a HIP error in case %s: %s" % (cid, checks.failed), returncode=3)
    checks.report()


def test_void_runs_stay_rare():
    """The void runs of the cases above, which a green case no longer shows.  A void run means that the gate did not do its work in
    that run: the side stream was picked once, as one that runs beside the null stream, and a run is void where that no longer held.
    The bound is not a measured figure: one run in twenty is where a case that needs three void runs in a row to fail, (1/20)^3 or
    about one in 8000, is still rarer than one per session of a few hundred cases; above it the picked stream has stopped running
    beside the null stream for good, and the suite says so here instead of hiding it behind repeats."""
    print("S runs: %d, void: %d %s" % (len(S_RUNS), len(VOID_RUNS), [c for c, _ in VOID_RUNS]))
    assert len(VOID_RUNS) <= MAX_VOID_SHARE * len(S_RUNS), "%d of %d S runs were void: %s" % (len(VOID_RUNS), len(S_RUNS), VOID_RUNS)


# ---- a handle is ready when `create` returns ----------------------------------------------------------------------------------------------
def _dev_out(n, dtype=torch.float32):
    return torch.empty(int(n), dtype=dtype, device="cuda:0")


def _ring_scn(kind):
    def scn(ctx):
        L = ctx.lib
        if kind == "create":
            widths = (8, 8, 2, 1, 1)
            create = lambda: ac._handle(ctx, L.ddrl_replay_destroy, L.ddrl_replay_create, 0, ac.CAP, 8, 2, 0)
            o1, a, r, o2, d = ac._rows5(8, 2, 7, 5, 0)
            rows = [ctx.tmp(x) for x in (o1, o2, a, r, d)]          # ring order, for ddrl_replay_store_ex
        else:
            widths = ac._wwidths(3, 5)
            w = ctx.keep((ctypes.c_int32 * 4)(*widths))
            if kind == "create_ex":
                create = lambda: ac._handle(ctx, L.ddrl_replay_destroy, L.ddrl_replay_create_ex, 0, ac.CAP, 4, w, 1, 1)
            else:
                kinds = ctx.keep((ctypes.c_uint8 * 4)(0, 0, 0, 0))
                create = lambda: ac._handle(ctx, L.ddrl_replay_destroy, L.ddrl_replay_create_typed, 0, ac.CAP, 4, w, kinds, 1, 1)
            rows = [ctx.tmp(x) for x in ac._wrows(3, 5, 7, 5)]
        src = ac._ptrs(*[t.data_ptr() for t in rows])

        def read(h, s):
            out = [_dev_out(ac.CAP * wd) for wd in widths] + [_dev_out(16, torch.int64)]
            for j, t in enumerate(out[:-1]):
                ac._ok(ctx, L.ddrl_replay_rows_export(h, j, 0, ac.CAP, ac._tp(t), s))
            ac._ok(ctx, L.ddrl_replay_sample_indices(h, 16, ac._tp(out[-1]), s))
            c = [ctypes.c_int64() for _ in range(4)]
            ac._ok(ctx, L.ddrl_replay_counts(h, *[byref(x) for x in c], s))
            return out + [torch.tensor([x.value for x in c])]
        return create, [lambda h, s: L.ddrl_replay_seed(h, 3, s), lambda h, s: L.ddrl_replay_store_ex(h, src, 7, s)], read
    return scn


def _ps_scn(ctx):
    L = ctx.lib
    src = ctx.tmp(ac._f32(ac._rs(1).randn(ac.PS_N)))

    def read(h, s):
        out = _dev_out(ac.PS_N)
        ac._ok(ctx, L.ddrl_ps_pull(h, ac._tp(out), 0, ac.PS_N, s))
        return [out]
    return (lambda: ac._handle(ctx, L.ddrl_ps_destroy, L.ddrl_ps_create, 0, ac.PS_N),
            [lambda h, s: L.ddrl_ps_push(h, ac._tp(src), 3, ac.PS_N - 3, s)], read)      # the first three floats stay as create left them


def _winq_scn(ctx):
    from distributed_drl_amd.replay import _view
    L, n, (Ln, obs) = ctx.lib, 37, ac.WINDOWS["Ln3o5"]
    r = ac._rs(3)
    o0 = ctx.tmp(ac._f32(r.randn(n, obs)))
    mask = ctx.tmp((np.arange(n) % 2).astype(np.uint8))          # every other env begins: the others stay as create left them
    ins = [ctx.tmp(ac._f32(r.randn(n, w))) for w in (obs, ac.WACT, 1, 1)]
    ready = _dev_out(n, torch.uint8)

    def read(h, s):
        arrs, tq = (P * 4)(), P()
        ac._ok(ctx, L.ddrl_winq_buffers(h, arrs, byref(tq)))
        dev = torch.device("cuda:0")
        return [_view(arrs[j], (n * w,), dev).clone() for j, w in enumerate(ac._wwidths(Ln, obs))] + [_view(tq.value, (n,), dev).clone(),
                                                                                                      ready.clone()]
    return (lambda: ac._handle(ctx, L.ddrl_winq_destroy, L.ddrl_winq_create, 0, n, Ln, obs, ac.WACT, 1),
            [lambda h, s: L.ddrl_winq_begin(h, ac._tp(mask), ac._tp(o0), s),
             lambda h, s: L.ddrl_winq_push(h, *[ac._tp(t) for t in ins], ac._tp(ready), s)], read)


def _env_scn(model):
    def scn(ctx):
        from distributed_drl_amd import _lib
        L, n = ctx.lib, 33
        other, fields = ac._env(ctx, n, model, seed=8)
        ac._env_warm(ctx, other, n)
        state = _dev_out(fields * n)
        ac._ok(ctx, L.ddrl_env_get_state(other, ac._tp(state), None))
        act = ctx.tmp(ac._f32(ac._rs(2).uniform(-1, 1, (n, 2))))
        m = ac.MODELS[model]
        em = ctx.keep(_lib.EnvModel(*m)) if m else None

        def read(h, s):
            out = _dev_out(fields * n)
            ac._ok(ctx, L.ddrl_env_get_state(h, ac._tp(out), s))
            return [out]
        return (lambda: ac._handle(ctx, L.ddrl_env_destroy, L.ddrl_env_create_ex, 0, n, 7, 2, byref(em) if em else None),
                [lambda h, s: L.ddrl_env_set_state(h, ac._tp(state), s),
                 lambda h, s: L.ddrl_env_step(h, ac._tp(act), None, None, None, None, None, s)], read)
    return scn


def _actor_scn(ctx):
    L = ctx.lib
    cfg = ctx.keep(ac._sac_cfg(ac.ACTOR_SHAPE))
    n_pi = ac._sac_counts(8, 2, 64, 48, 0)[0]
    w = ctx.tmp(ac._weights(n_pi, 41))
    obs = ctx.tmp(ac._f32(ac._rs(4).randn(5, 8)))

    def read(h, s):
        out, act = _dev_out(n_pi), _dev_out(10)
        ac._ok(ctx, L.ddrl_actor_get_weights(h, ac._tp(out), s))
        ac._ok(ctx, L.ddrl_actor_act(h, ac._tp(obs), None, 5, 1, ac._tp(act), s))
        return [out, act]
    return (lambda: ac._handle(ctx, L.ddrl_actor_destroy, L.ddrl_actor_create, 0, byref(cfg), ac.MAX_ROWS),
            [lambda h, s: L.ddrl_actor_set_weights(h, ac._tp(w), s)], read)


def _learner_scn(dqn):
    def scn(ctx):
        L = ctx.lib
        if dqn:
            cfg = ctx.keep(ac._dqn_cfg("o8A2h64x48B37", 0))
            nn = ctypes.c_int64()
            ac._ok(ctx, L.ddrl_dqn_param_count(byref(cfg), byref(nn)))
            n, scale = int(nn.value), 0.25
            create = lambda: ac._handle(ctx, L.ddrl_dqn_destroy, L.ddrl_dqn_create, 0, byref(cfg))
            setw, export = L.ddrl_dqn_set_weights, L.ddrl_dqn_export
        else:
            cfg = ctx.keep(ac._sac_cfg(ac.LSHAPE))
            n, scale = ac._sac_counts(8, 2, 64, 48, 0)[1], 1.0
            create = lambda: ac._handle(ctx, L.ddrl_sac1_destroy, L.ddrl_sac1_create, 0, byref(cfg))
            setw, export = L.ddrl_sac1_set_weights, L.ddrl_sac1_export
        w = ctx.tmp(ac._weights(n, 21) * scale)

        def read(h, s):
            out = [_dev_out(n) for _ in range(4)]
            for which, t in enumerate(out):
                ac._ok(ctx, export(h, which, ac._tp(t), s))
            return out
        return create, [lambda h, s: setw(h, ac._tp(w), s)], read
    return scn


def _loop_scn(dqn):
    def scn(ctx):
        L = ctx.lib
        if dqn:
            learner, n, _ = ac._dqn(ctx, "o8A2h64x48B37", 0)
            ring = ac._ring5(ctx, 8, 1, 0, cap=ac.LOOP_ROWS, fill=0)
            r, R = ac._rs(72), ac.LOOP_ROWS
            rows = [ac._f32(r.randn(R, 8)), ac._f32(r.randint(0, 2, (R, 1))), ac._f32(r.randn(R)), ac._f32(r.randn(R, 8)),
                    ac._f32(r.rand(R) < 0.2)]                       # the acts are action indices
            ac._ok(ctx, L.ddrl_replay_store(ring, *[ac._tp(ctx.tmp(x)) for x in rows], R, None))
            create = lambda: ac._handle(ctx, L.ddrl_dqn_loop_destroy, L.ddrl_dqn_loop_create, learner, ring, 2, None)
            run, export = L.ddrl_dqn_loop_run, L.ddrl_dqn_export
        else:
            learner, n = ac._sac(ctx, ac.LSHAPE)
            ring = ac._sac_ring(ctx, cap=ac.LOOP_ROWS, fill=ac.LOOP_ROWS)
            create = lambda: ac._handle(ctx, L.ddrl_loop_destroy, L.ddrl_loop_create, learner, ring, 2, 13)
            run, export = L.ddrl_loop_run, L.ddrl_sac1_export

        def read(h, s):
            out = [_dev_out(n) for _ in range(4)]
            for which, t in enumerate(out):
                ac._ok(ctx, export(learner, which, ac._tp(t), s))
            return out
        return create, [lambda h, s: run(h, 1, s), lambda h, s: run(h, 5, s)], read
    return scn


CREATORS = {
    "ddrl_replay_create": _ring_scn("create"), "ddrl_replay_create_ex": _ring_scn("create_ex"),
    "ddrl_replay_create_typed": _ring_scn("create_typed"), "ddrl_ps_create": _ps_scn, "ddrl_winq_create": _winq_scn,
    "ddrl_env_create_ex-one_body": _env_scn("one_body"), "ddrl_env_create_ex-articulated": _env_scn("articulated"),
    "ddrl_actor_create": _actor_scn, "ddrl_sac1_create": _learner_scn(False), "ddrl_dqn_create": _learner_scn(True),
    "ddrl_loop_create": _loop_scn(False), "ddrl_dqn_loop_create": _loop_scn(True),
}


def _created_and_used(lib, name, gated):
    """(read-back at s.synchronize(), read-back after a device sync, gate ms, whether the gate was still running when create returned);
    the twin (gated False): the same calls on the null stream with a device sync between every two."""
    ctx = aa.PlainCtx("cuda:0", lib)
    try:
        create, steps, read = CREATORS[name](ctx)
        torch.cuda.synchronize()
        if not gated:
            h = create()
            torch.cuda.synchronize()
            for st in steps:
                ac._ok(ctx, st(h, None))
                torch.cuda.synchronize()
            first = [t.cpu() for t in read(h, None)]
            torch.cuda.synchronize()
            second = [t.cpu() for t in read(h, None)]       # (a read-back may move the handle: the ring's draws advance its MT stream)
            torch.cuda.synchronize()
            return first, second, None, None
        side = aa.TorchSide("cuda:0", GATE_MS)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()                                   # the gate on the NULL stream: torch's default stream is the null stream
        torch.cuda._sleep(side.cycles)
        e1.record()
        h = create()
        held = not e1.query()
        mark = torch.cuda.Event(enable_timing=True)
        with side.on():
            torch.zeros(1, device="cuda:0")
            mark.record()                             # the side stream is not held by the gate (aa.side_stream), checked again here
            for st in steps:
                ac._ok(ctx, st(h, side_arg(side)))
            first = read(h, side_arg(side))
            side.synchronize()
            first = [t.cpu() for t in first]
        torch.cuda.synchronize()
        second = [t.cpu() for t in read(h, None)]
        torch.cuda.synchronize()
        assert held is False or mark.elapsed_time(e1) > 0.0, "the gate on the null stream held the side stream too: the run is void"
        return first, second, e0.elapsed_time(e1), held
    finally:
        ctx.finish()


def side_arg(side):
    return P(side.stream.cuda_stream)


@pytest.mark.parametrize("name", sorted(CREATORS))
def test_a_handle_is_ready_when_create_returns(lib, name):
    assert torch.cuda.default_stream().cuda_stream == 0
    want, want2, _, _ = _created_and_used(lib, name, False)
    first, second, gate_ms, held = _created_and_used(lib, name, True)
    print("%s: gate %.2f ms on the null stream, %s when create returned" % (name, gate_ms, "still running" if held else "over"))
    assert gate_ms >= GATE_MS, "the gate held the null stream for %.2f ms, %.2f ms intended: the run is void" % (gate_ms, GATE_MS)
    assert len(first) == len(second) == len(want) == len(want2)
    for i, (a, b, w, w2) in enumerate(zip(first, second, want, want2)):
        assert torch.equal(a.view(torch.uint8), w.view(torch.uint8)), \
            "%s: read-back %d on the side stream differs from the twin's: the handle was not ready when create returned" % (name, i)
        assert torch.equal(b.view(torch.uint8), w2.view(torch.uint8)), \
            "%s: read-back %d after the device drained differs from the twin's: create left work behind that landed later" % (name, i)
