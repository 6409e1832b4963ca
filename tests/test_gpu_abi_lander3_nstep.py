"""GPU: the C-ABI's memory contract (include/ddrl.h, "Memory contract") for the n-step worker's entry points on the ARTICULATED lander:
the cases of tests/_abi_contract_lander3_nstep.py between guard bands (tests/_abi_arena.py), held to P1-P4 as
tests/test_gpu_abi_memory.py holds the one-body twins; and the step call's mirror pointers one float off their grid, refused on the
host with the member named and nothing changed."""
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
import _abi_contract_lander3_nstep as an   # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from distributed_drl_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return _lib.load()


@pytest.mark.parametrize("cid", sorted(an.CASES))
def test_memory_contract(lib, cid):
    try:
        checks = aa.run_case(cid, an.CASES[cid][0], "cuda:0", lib)
    except RuntimeError as e:   # a HIP error out of torch (a fault is sticky: nothing that follows in this process would mean anything)
        pytest.exit("the device reported an error in case %s: %s" % (cid, e), returncode=3)
    if any(p == "RC" and "returned -3," in w for p, w in checks.failed):   # DDRL_ERR_HIP
        pytest.exit("the library reported a HIP error in case %s: %s" % (cid, checks.failed), returncode=3)
    checks.report()


@pytest.mark.parametrize("member", ["act", "obs2", "next_obs"])
def test_step_nstep_articulated_refuses_a_mirror_off_its_grid(lib, member):
    from distributed_drl_amd import _lib
    L, ctx, n, Ln = lib, aa.PlainCtx("cuda:0", lib), ac.RN, 4
    try:
        h, fields = ac._env(ctx, n, "articulated", max_ep_len=50)
        a, _ = ac._actor(ctx)
        ring = ac._wring(ctx, Ln, 8, cap=ac.RCAP, fill=7)
        q = ac._handle(ctx, L.ddrl_winq_destroy, L.ddrl_winq_create, 0, n, Ln, 8, 2, 1)
        obs = ctx.tmp(torch.empty(n * 8, dtype=torch.float32))
        ac._ok(ctx, L.ddrl_env_reset(h, None, ac._tp(obs), None))
        ac._ok(ctx, L.ddrl_winq_begin(q, None, ac._tp(obs), None))
        ac._ok(ctx, L.ddrl_rollout_begin_nstep_articulated(h, a, q, None))
        ac._ok(ctx, L.ddrl_rollout_step_nstep_articulated(h, a, q, ring, 3, 0.3, 0.1, 5.0, 2, 3, 0, 5, 0, None, None))

        def image():
            st = torch.empty(fields * n, dtype=torch.float32, device="cuda:0")
            ac._ok(ctx, L.ddrl_env_get_state(h, ac._tp(st), None))
            rows = []
            for j, w in enumerate(ac._wwidths(Ln, 8)):
                t = torch.empty(ac.RCAP * w, dtype=torch.float32, device="cuda:0")
                ac._ok(ctx, L.ddrl_replay_rows_export(ring, j, 0, ac.RCAP, ac._tp(t), None))
                rows.append(t)
            arrays, tq = (P * 4)(), P()
            ac._ok(ctx, L.ddrl_winq_buffers(q, arrays, byref(tq)))
            return [st] + rows

        buf = torch.full((n * 8 + 64,), 3.0, dtype=torch.float32, device="cuda:0")
        before = image()
        out = _lib.RolloutNStepOut(**{member: P(buf.data_ptr() + 4)})
        rc = L.ddrl_rollout_step_nstep_articulated(h, a, q, ring, 1, 0.3, 0.1, 5.0, 2, 3, 0, 5, 4000, byref(out), None)
        assert rc == _lib.DDRL_ERR_BAD_ARG and ("out->" + member).encode() in L.ddrl_last_error(), (rc, L.ddrl_last_error())
        torch.cuda.synchronize()
        assert bool((buf == 3.0).all())
        for x, y in zip(before, image()):
            assert torch.equal(x, y)
    finally:
        ctx.finish()
