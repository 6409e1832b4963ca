"""GPU: the C-ABI's memory contract and stream contract (include/ddrl.h) for the n-step worker's entry point on the WALKER,
ddrl_env_step_wrapped_walker (include/ddrl_walker.h): the cases of tests/_abi_contract_walker_nstep.py between guard bands (tests/_abi_arena.run_case), held
to P1-P4 as tests/test_gpu_abi_memory.py holds the landers' twins, and once more on a non-blocking side stream behind a bounded gate
(tests/_abi_arena.run_stream_case), under the policy of tests/test_gpu_abi_stream.py: a run that is void and nothing else is made again,
twice at the most, a void run never passes, and void runs are counted against the same 5 % share.

The gate.  The slowest call of these cases, timed once between two events on the default stream: 0.409 ms, the closure of
env_step_wrapped_walker-n1 as the process's first launch of the kernel (its code object is loaded then; every later closure, n = 257
included — five workgroups, two action trips and the reset trip at 4 / 2 iterations, plus the state read-back — took 0.10 to 0.13 ms).
The gate is the larger of 10 ms and 10 x that value: 10 ms.  Every run measures its own gate with events; one that came out shorter fails as
VOID."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_arena as aa   # noqa: E402
import _abi_contract_walker_nstep as aw   # noqa: E402

SLOWEST_CALL_MS = 0.409
GATE_MS = max(10.0, 10.0 * SLOWEST_CALL_MS)


@pytest.fixture(scope="module")
def lib():
    from distributed_drl_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return _lib.load()


@pytest.mark.parametrize("cid", sorted(aw.CASES))
def test_memory_contract(lib, cid):
    try:
        checks = aa.run_case(cid, aw.CASES[cid][0], "cuda:0", lib)
    except RuntimeError as e:   # a HIP error out of torch (a fault is sticky: nothing that follows in this process would mean anything)
        pytest.exit("the device reported an error in case %s: %s" % (cid, e), returncode=3)
    if any(p == "RC" and "returned -3," in w for p, w in checks.failed):   # DDRL_ERR_HIP
        pytest.exit("the library reported a HIP error in case %s: %s" % (cid, checks.failed), returncode=3)
    checks.report()


S_RUNS, VOID_RUNS = [], []      # every S run of this module, and those that came out void (case id, what the run reported)
MAX_VOID_SHARE = 0.05


@pytest.mark.parametrize("cid", sorted(aw.CASES))
def test_stream_contract(lib, cid):
    try:
        # tests/test_gpu_abi_stream.py's policy: a run that is void and nothing else is made again, twice at the most, with fresh
        # handles; a third void run fails as void.  A void run never passes, any other failure is reported at once, and every void
        # run is counted: test_void_runs_stay_rare holds the module's total to a bound.
        for _ in range(3):
            checks = aa.run_stream_case(cid, aw.CASES[cid][0], "cuda:0", lib, aa.TorchSide("cuda:0", GATE_MS))
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
