"""GPU: the C-ABI's memory contract and stream contract (include/ddrl.h) on a HARDCORE walker handle
(ddrl_env_create_walker, include/ddrl_walker_hardcore.h): the cases of tests/_abi_contract_walker_hardcore.py — ddrl_env_step,
ddrl_env_step_wrapped_walker, a masked ddrl_env_reset and ddrl_env_set_state / _get_state at the handle's block size — between guard
bands (tests/_abi_arena.run_case), held to P1-P4 as tests/test_gpu_abi_walker_nstep.py holds the grass walker's wrapped step, and once
more on a non-blocking side stream behind a bounded gate (tests/_abi_arena.run_stream_case), under the policy of
tests/test_gpu_abi_stream.py: a run that is void and nothing else is made again, twice at the most, a void run never passes, and void
runs are counted against the same 5 % share.

The gate.  The slowest call of these cases is the closure that makes the process's first launch of a Hardcore kernel (its code object is
loaded then), as in tests/test_gpu_abi_walker_nstep.py, where that call took 0.409 ms; every closure here is a launch at 4 / 2
iterations plus the state read-back.  The gate is the larger of 10 ms and 10 x that value: 10 ms.  Every run measures its own gate with
events; one that came out shorter fails as VOID."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_arena as aa   # noqa: E402
import _abi_contract_walker_hardcore as ah   # noqa: E402

SLOWEST_CALL_MS = 0.409
GATE_MS = max(10.0, 10.0 * SLOWEST_CALL_MS)


@pytest.fixture(scope="module")
def lib():
    from distributed_drl_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return _lib.load()


@pytest.mark.parametrize("cid", sorted(ah.CASES))
def test_memory_contract(lib, cid):
    try:
        checks = aa.run_case(cid, ah.CASES[cid][0], "cuda:0", lib)
    except RuntimeError as e:   # a HIP error out of torch (a fault is sticky: nothing that follows in this process would mean anything)
        pytest.exit("the device reported an error in case %s: %s" % (cid, e), returncode=3)
    if any(p == "RC" and "returned -3," in w for p, w in checks.failed):   # DDRL_ERR_HIP
        pytest.exit("the library reported a HIP error in case %s: %s" % (cid, checks.failed), returncode=3)
    checks.report()


S_RUNS, VOID_RUNS = [], []      # every S run of this module, and those that came out void (case id, what the run reported)
MAX_VOID_SHARE = 0.05


@pytest.mark.parametrize("cid", sorted(ah.CASES))
def test_stream_contract(lib, cid):
    try:
        for _ in range(3):   # tests/test_gpu_abi_stream.py's policy for void runs
            checks = aa.run_stream_case(cid, ah.CASES[cid][0], "cuda:0", lib, aa.TorchSide("cuda:0", GATE_MS))
            S_RUNS.append(cid)
            if checks.props() != ["VOID"]:
                break
            VOID_RUNS.append((cid, checks.failed))
            print("void run of %s: %s" % (cid, checks.failed))
    except RuntimeError as e:
        pytest.exit("the device reported an error in case %s: %s" % (cid, e), returncode=3)
    if any(p == "RC" and "returned -3," in w for p, w in checks.failed):
        pytest.exit("the library reported a HIP error in case %s: %s" % (cid, checks.failed), returncode=3)
    checks.report()


def test_void_runs_stay_rare():
    """As tests/test_gpu_abi_stream.py::test_void_runs_stay_rare, over this module's S runs and with its bound."""
    print("S runs: %d, void: %d %s" % (len(S_RUNS), len(VOID_RUNS), [c for c, _ in VOID_RUNS]))
    assert len(VOID_RUNS) <= MAX_VOID_SHARE * len(S_RUNS), "%d of %d S runs were void: %s" % (len(VOID_RUNS), len(S_RUNS), VOID_RUNS)
