"""GPU: the C-ABI's memory contract (include/ddrl.h, "Memory contract") for every entry point that takes caller device memory.
Each case of tests/_abi_contract.py runs between guard bands (tests/_abi_arena.py) and is held to four properties — P1 nothing is
written outside a buffer, P2 every output is written in full with the values the plain twin gets (or left alone where the header says
so), P3 inputs stay bit-identical, P4 the result does not depend on what surrounds the inputs — in the all-aligned variant and, where
the contract allows a pointer off the 16-byte grid, with each such pointer offset by one float (bit-equal to the aligned run: this is
what runs the ring kernels' scalar branches).  The env family's row-vector pointers are the other way round: one float off their grid
they are refused on the host, before any launch, with the pointer named and no state changed (REFUSALS)."""
import ctypes
import os
import sys
from ctypes import byref, c_void_p as P

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_arena as aa   # noqa: E402
import _abi_contract as ac   # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from distributed_drl_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return _lib.load()


@pytest.mark.parametrize("cid", sorted(ac.CASES))
def test_memory_contract(lib, cid):
    try:
        checks = aa.run_case(cid, ac.CASES[cid][0], "cuda:0", lib)
    except RuntimeError as e:   # a HIP error out of torch (a fault is sticky: nothing that follows in this process would mean anything)
        pytest.exit("the device reported an error in case %s: %s" % (cid, e), returncode=3)
    if any(p == "RC" and "returned -3," in w for p, w in checks.failed):   # DDRL_ERR_HIP
        pytest.exit("the library reported a HIP error in case %s: %s" % (cid, checks.failed), returncode=3)
    checks.report()


# ---- host-side refusals -------------------------------------------------------------------------------------------------------------
class _World:
    """Handles of one refusal call and a bit image of everything a refused call must leave alone."""

    def __init__(self, lib, function):
        self.ctx = ctx = aa.PlainCtx("cuda:0", lib)
        L = lib
        artic = function == "ddrl_rollout_step_articulated"
        self.n = n = ac.RN
        self.env, self.fields = ac._env(ctx, n, "articulated" if artic else "one_body", max_ep_len=50)
        ac._env_warm(ctx, self.env, n)
        self.ring = self.actor = self.dqn = self.winq = None
        if function in ("ddrl_rollout_step", "ddrl_rollout_step_articulated"):
            self.actor, _ = ac._actor(ctx)
            self.ring, self.widths = ac._ring5(ctx, 8, 2, cap=ac.RCAP, fill=7), (8, 8, 2, 1, 1)
            ac._ok(ctx, (L.ddrl_rollout_begin_articulated if artic else L.ddrl_rollout_begin)(self.env, self.actor, None))
        elif function == "ddrl_rollout_step_discrete":
            self.dqn, _, _ = ac._dqn(ctx, ac.DSHAPE)
            self.ring, self.widths = ac._ring5(ctx, 8, 1, cap=ac.RCAP, fill=7), (8, 8, 1, 1, 1)
            ac._ok(ctx, L.ddrl_rollout_begin_discrete(self.env, self.dqn, None))
        elif function == "ddrl_rollout_step_nstep":
            self.actor, _ = ac._actor(ctx)
            self.ring, self.widths = ac._wring(ctx, 4, 8, cap=ac.RCAP, fill=7), ac._wwidths(4, 8)
            self.winq = ac._handle(ctx, L.ddrl_winq_destroy, L.ddrl_winq_create, 0, n, 4, 8, 2, 1)
            obs = ctx.tmp(torch.empty(n * 8, dtype=torch.float32))
            ac._ok(ctx, L.ddrl_env_reset(self.env, None, ac._tp(obs), None))
            ac._ok(ctx, L.ddrl_winq_begin(self.winq, None, ac._tp(obs), None))
            ac._ok(ctx, L.ddrl_rollout_begin_nstep(self.env, self.actor, self.winq, None))
        self.buf = torch.full((n * 8 + 64,), 3.0, dtype=torch.float32, device="cuda:0")    # what the offset pointer points into

    def image(self):
        L, ctx, out = self.ctx.lib, self.ctx, []
        st = torch.empty(self.fields * self.n, dtype=torch.float32, device="cuda:0")
        ac._ok(ctx, L.ddrl_env_get_state(self.env, ac._tp(st), None))
        out.append(st)
        if self.ring is not None:
            for j, w in enumerate(self.widths):
                t = torch.empty(ac.RCAP * w, dtype=torch.float32, device="cuda:0")
                ac._ok(ctx, L.ddrl_replay_rows_export(self.ring, j, 0, ac.RCAP, ac._tp(t), None))
                out.append(t)
            c = [ctypes.c_int64() for _ in range(4)]
            ac._ok(ctx, L.ddrl_replay_counts(self.ring, *[byref(x) for x in c], None))
            out.append(torch.tensor([x.value for x in c]))
        if self.winq is not None:
            from distributed_drl_amd.replay import _view
            arrs, tq = (P * 4)(), P()
            ac._ok(ctx, L.ddrl_winq_buffers(self.winq, arrs, byref(tq)))
            for j, w in enumerate(ac._wwidths(4, 8)):
                out.append(_view(arrs[j], (self.n * w,), torch.device("cuda:0")).clone())
            out.append(_view(tq.value, (self.n,), torch.device("cuda:0")).clone())
        out.append(self.buf.clone())
        torch.cuda.synchronize()
        return [t.cpu().view(torch.uint8) if t.dtype != torch.int64 else t for t in out]


def _refused_call(w, function, pointer):
    """The call with `pointer` one float off its grid (every other pointer aligned or NULL)."""
    from distributed_drl_amd import _lib
    L, n = w.ctx.lib, w.n
    off = P(w.buf.data_ptr() + 4)
    assert w.buf.data_ptr() % 256 == 0
    pick = lambda name: off if name == pointer else None
    act = w.ctx.tmp(ac._f32(ac._rs(2).uniform(-1, 1, (n, 2))))
    if function == "ddrl_env_reset":
        return L.ddrl_env_reset(w.env, None, off, None)
    if function in ("ddrl_env_step", "ddrl_env_step_discrete"):
        a = off if pointer == "act_d" else ac._tp(act)
        return getattr(L, function)(w.env, a, pick("obs2_d"), None, None, pick("next_obs_d"), None, None)
    if function == "ddrl_env_step_wrapped":
        a = off if pointer == "act_d" else ac._tp(act)
        return L.ddrl_env_step_wrapped(w.env, a, 0.3, 0.1, 5.0, 2, 50, pick("obs2_d"), None, None, pick("next_obs_d"), None, None)
    if function in ("ddrl_rollout_step", "ddrl_rollout_step_articulated"):
        return getattr(L, function)(w.env, w.actor, w.ring, 1, 5, 0, 0, pick("act_out_d"), pick("next_obs_out_d"), None)
    if function == "ddrl_rollout_step_discrete":
        return L.ddrl_rollout_step_discrete(w.env, w.dqn, w.ring, 1, 0, 0.5, 5, 0, None, None, off, None)
    if function == "ddrl_rollout_step_nstep":
        out = _lib.RolloutNStepOut(**{pointer.split("->")[1]: off})
        return L.ddrl_rollout_step_nstep(w.env, w.actor, w.winq, w.ring, 1, 0.3, 0.1, 5.0, 2, 50, 0, 5, 0, byref(out), None)
    ret = w.ctx.tmp(torch.zeros(ac.EPISODES, dtype=torch.float64))
    ln = w.ctx.tmp(torch.zeros(ac.EPISODES, dtype=torch.int32))
    if function == "ddrl_policy_eval":
        cfg = ac._sac_cfg(ac.ACTOR_SHAPE)
        wts = w.ctx.tmp(ac._weights(ac._sac_counts(8, 2, 64, 48, 0)[0], 41))
        return L.ddrl_policy_eval(byref(cfg), ac._tp(wts), ac.EPISODES, 5, 2, ac.EP_LEN, ac._tp(ret), ac._tp(ln), off, None)
    assert function == "ddrl_dqn_eval"
    cfg = ac._dqn_cfg(ac.DSHAPE, 0)
    nq = ctypes.c_int64()
    ac._ok(w.ctx, L.ddrl_dqn_param_count(byref(cfg), byref(nq)))
    wts = w.ctx.tmp(ac._weights(nq.value, 51))
    return L.ddrl_dqn_eval(byref(cfg), ac._tp(wts), ac.EPISODES, 5, 2, ac.EP_LEN, 0, 0.5, 9, 0, ac._tp(ret), ac._tp(ln), off, None)


@pytest.mark.parametrize("function,pointer", ac.REFUSALS, ids=["%s-%s" % (f, p.replace("->", ".")) for f, p in ac.REFUSALS])
def test_a_vector_moved_pointer_off_its_grid_is_refused_on_the_host(lib, function, pointer):
    w = _World(lib, function)
    try:
        before = w.image()
        rc = _refused_call(w, function, pointer)
        msg = lib.ddrl_last_error().decode()
        after = w.image()
        assert rc == -1, (rc, msg)                                                        # DDRL_ERR_BAD_ARG
        assert pointer in msg and "aligned" in msg, msg                                   # the message names the pointer
        assert len(before) == len(after)
        for i, (b, a) in enumerate(zip(before, after)):
            assert torch.equal(b, a), "a refused call changed part %d of the handles' state" % i
    finally:
        w.ctx.finish()


def test_the_env_wrapper_never_hands_the_library_a_misaligned_action_view(lib):
    """VecLunarLander.step copies an action view that starts off the 8-byte grid (same bits as the aligned tensor); step_wrapped,
    which returns the noisy action in place, raises the library's refusal instead."""
    from distributed_drl_amd.env import VecLunarLander
    n = 33
    a = torch.from_numpy(ac._f32(ac._rs(4).uniform(-1, 1, (n, 2)))).cuda()
    flat = torch.zeros(2 * n + 1, device="cuda")
    flat[1:] = a.reshape(-1)
    view = flat[1:].view(n, 2)
    assert view.data_ptr() % 8 == 4 and view.is_contiguous()
    e1, e2 = VecLunarLander(n, seed=3), VecLunarLander(n, seed=3)
    g, w = e1.step(view), e2.step(a)
    for x, y in zip(g, w):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match="act_d"):
        e1.step_wrapped(view, 0.3, 0.1, 5.0)
    assert torch.equal(e1.get_state(), e2.get_state())
