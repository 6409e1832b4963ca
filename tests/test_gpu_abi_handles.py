"""GPU: the C-ABI's memory contract and stream contract (include/ddrl.h) on the handles that come through another door than ddrl.h's
creators — ddrl_sac1_create_wide, ddrl_sacv_create_wide, ddrl_dqn_create_direct (both variants), ddrl_actor_create_wide, whose headers
promise an ordinary handle under ddrl.h's contracts.  The cases of tests/_abi_contract_handles.py run between guard bands
(tests/_abi_arena.run_case), held to P1-P4 and ALIGN as tests/test_gpu_abi_memory.py holds the same functions on ddrl.h's own handles,
and, with that module's stream rows, once more on a non-blocking side stream behind a bounded gate (tests/_abi_arena.run_stream_case),
under the policy of tests/test_gpu_abi_stream.py: a run that is void and nothing else is made again, twice at the most, a void run
never passes, and void runs are counted against the same 5 % share.

The gate.  The slowest call of these cases, each closure timed once between two events on the default stream on an MI355X, all in
one process in sorted order of the case ids: 3.345 ms, the closure of ddqn-direct:loop-loss-o11A3h52x36B37 (ddrl_dqn_loop_run with the
process's first graph capture; the next ones: actor-wide:env_eval_policy-articulated-o8a2 3.064 ms, sac1-wide:loop_run-o24a4h64x48B37-
per_graph3 1.271 ms, sac1-wide:loop_run-o27a4h72x44B37-per_graph3 1.169 ms, the two sacv-wide loop_run-per_graph3 rows 1.048 and
1.033 ms, sac1-wide:step_host-o12a1h36x8B5 0.912 ms; everything else below 0.75 ms).  The gate is the larger of 10 ms and 10 x that value,
33.45 ms: a wrongly placed launch has only to start and finish inside it.  Every run measures its own gate with events; one that came
out shorter fails as VOID."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_arena as aa   # noqa: E402
import _abi_contract_handles as ah   # noqa: E402

SLOWEST_CALL_MS = 3.345
GATE_MS = max(10.0, 10.0 * SLOWEST_CALL_MS)

S_CASES = {}
for _d in (ah.CASES, ah.STREAM_CASES):
    for _k, _v in _d.items():
        assert _k not in S_CASES, _k
        S_CASES[_k] = _v


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


@pytest.mark.parametrize("cid", sorted(S_CASES))
def test_stream_contract(lib, cid):
    try:
        # tests/test_gpu_abi_stream.py's policy: a run that is void and nothing else is made again, twice at the most, with fresh
        # handles; a third void run fails as void.  A void run never passes, any other failure is reported at once, and every void
        # run is counted: test_void_runs_stay_rare holds the module's total to a bound.
        for _ in range(3):
            checks = aa.run_stream_case(cid, S_CASES[cid][0], "cuda:0", lib, aa.TorchSide("cuda:0", GATE_MS))
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
