"""GPU: the stream contract (include/ddrl.h) for the walker's evaluation entry point, ddrl_env_eval_policy_walker
(include/ddrl_walker_eval.h): the stream case of tests/_abi_contract_walker_eval.py — a ddrl_actor_set_weights ahead of the call under
test on the same stream, which does not commute with it — on a non-blocking side stream behind a bounded gate
(tests/_abi_arena.run_stream_case), under the policy of tests/test_gpu_abi_walker_nstep.py: a run that is void and nothing else is made
again, twice at the most, a void run never passes, and void runs are counted against the same 5 % share.  The function takes no caller
device memory, so there is no guard-band half.

The gate.  The closure of env_eval_policy_walker (set_weights, 3 episodes of up to 6 steps at 4 / 2 iterations as one launch, the three
copies out of the results block), timed once between two events on the default stream: 3.578 ms as the process's first closure (the
case's setup has launched the kernel once by then; the first device-to-device copies out of the block are made here), 0.304 and
0.272 ms for the two closures behind it.  The gate is the larger of 10 ms and 10 x the slowest: 35.78 ms.
Every run measures its own gate with events; one that came out shorter fails as VOID."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_arena as aa   # noqa: E402
import _abi_contract_walker_eval as ae   # noqa: E402

SLOWEST_CALL_MS = 3.578
GATE_MS = max(10.0, 10.0 * SLOWEST_CALL_MS)


@pytest.fixture(scope="module")
def lib():
    from distributed_drl_amd import _lib
    _lib.require_gpu()
    torch.cuda.set_device(0)
    return _lib.load()


S_RUNS, VOID_RUNS = [], []      # every S run of this module, and those that came out void (case id, what the run reported)
MAX_VOID_SHARE = 0.05


@pytest.mark.parametrize("cid", sorted(ae.STREAM_CASES))
def test_stream_contract(lib, cid):
    try:
        # tests/test_gpu_abi_stream.py's policy: a run that is void and nothing else is made again, twice at the most, with fresh
        # handles; a third void run fails as void.  A void run never passes, any other failure is reported at once, and every void
        # run is counted: test_void_runs_stay_rare holds the module's total to a bound.
        for _ in range(3):
            checks = aa.run_stream_case(cid, ae.STREAM_CASES[cid][0], "cuda:0", lib, aa.TorchSide("cuda:0", GATE_MS))
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
    """As tests/test_gpu_abi_stream.py::test_void_runs_stay_rare, over this module's S runs and with its bound."""
    print("S runs: %d, void: %d %s" % (len(S_RUNS), len(VOID_RUNS), [c for c, _ in VOID_RUNS]))
    assert len(VOID_RUNS) <= MAX_VOID_SHARE * len(S_RUNS), "%d of %d S runs were void: %s" % (len(VOID_RUNS), len(S_RUNS), VOID_RUNS)
