"""CPU half of the walker's evaluation-trace checks (tests/_walker_eval_trace.py): on traces built from the oracles alone —
_acting_parity.forward32 and WalkerOracle — check_env_walker and check_policy pass; each of the five planted defects of
_eval_trace.DEFECTS and a trace played with the velocity and position iteration counts swapped are seen; and the fixed inputs meet
the conditions the GPU half (tests/test_gpu_walker_eval.py) relies on: the endings and the ground contacts of the first three cases.
Also: include/ddrl_walker_eval.h declares exactly the one entry point, its ctypes table and the library name it, its stream row stands
in tests/_abi_contract_walker_eval.TABLE, the package exports the marker, and csrc/walker_eval.hip reads no handle kind."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _eval_trace as et  # noqa: E402
import _walker_eval_trace as wt  # noqa: E402

NAME = "ddrl_env_eval_policy_walker"
SMALL_CASE = wt.WalkerEvalCase("w-64x48-n2-len40", (64, 48), 2, 40)     # both episodes end on the time limit
_TRACES = {}


def _trace(case, defect=None, swapped=False):
    key = (case.id, defect, swapped)
    if key not in _TRACES:
        kw = dict(vit=case.pit, pit=case.vit) if swapped else {}
        _TRACES[key] = wt.oracle_trace_walker(case, wt.params_of(case), defect, **kw)
    return _TRACES[key]


def _fails(check, *a, **kw):
    try:
        check(*a, **kw)
    except AssertionError:
        return True
    return False


def _env_check(out, case):
    wt.check_env_walker(out, case.seed, case.first, case.max_ep_len, case.vit, case.pit, case.id)


@pytest.mark.parametrize("case", [SMALL_CASE] + wt.TRACE_CASES[:3], ids=repr)
def test_checks_pass_on_the_oracles_trace(case):
    out = _trace(case)
    _env_check(out, case)
    wt.check_policy(out, case, wt.params_of(case))


def _contact_steps(case, out):
    """Per episode, the steps whose result has a leg on the ground (observation elements 8 / 13 of o2), the recorded actions replayed."""
    env, _ = wt.oracle_at(case.seed, case.first, case.max_ep_len, case.vit, case.pit)
    counts = []
    for e in range(case.n):
        c = 0
        for t in range(int(out["len"][e])):
            o2 = env.step(out["trace"][e, t, 24:28].reshape(1, 4))[0]
            c += int(o2[0, 8] == 1 or o2[0, 13] == 1)
        counts.append(c)
    return counts


def test_inputs_reach_the_endings_and_the_contacts_the_gpu_half_relies_on():
    last = lambda out: np.array([out["trace"][e, l - 1] for e, l in enumerate(out["len"])])
    # every episode ends on a terminal at step 54, after 17 steps with a leg on the ground; the three returns differ
    case, out = wt.TERMINAL_CASE, _trace(wt.TERMINAL_CASE)
    assert out["len"].tolist() == [54, 54, 54] and (last(out)[:, wt.I_REW] == -100).all() and (last(out)[:, wt.I_END] == 1).all()
    assert _contact_steps(case, out) == [17, 17, 17] and len(set(out["ret"].tolist())) == 3
    # the full-width row: a terminal at step 79
    case, out = wt.WIDE_CASE, _trace(wt.WIDE_CASE)
    assert out["len"].tolist() == [79, 79] and (last(out)[:, wt.I_REW] == -100).all()
    # h1 and h2 off 16: the time limit, with 90 or more contact steps
    case, out = wt.LIMIT_CASE, _trace(wt.LIMIT_CASE)
    assert case.hid[0] % 16 and case.hid[1] % 16
    assert (out["len"] == case.max_ep_len).all() and (last(out)[:, wt.I_REW] != -100).all() and (last(out)[:, wt.I_END] == 1).all()
    assert min(_contact_steps(case, out)) >= 90
    # the small case of the defect tests ends on the limit too
    assert (_trace(SMALL_CASE)["len"] == SMALL_CASE.max_ep_len).all()


@pytest.mark.parametrize("defect", et.DEFECTS)
def test_planted_defect_fails_a_check(defect):
    case = SMALL_CASE
    assert case.n > 1      # episode_index_not_advanced needs a second episode
    out, params = _trace(case, defect), wt.params_of(case)
    env_fails = _fails(_env_check, out, case)
    pol_fails = _fails(wt.check_policy, out, case, params)
    # each defect is seen by the half it belongs to
    if defect in ("action_from_previous_obs", "last_hidden2_dropped"):
        assert pol_fails, defect
    else:
        assert env_fails, defect


def test_a_row_with_a_nonzero_tail_element_or_a_nonzero_row_past_the_end_is_seen():
    case = wt.WalkerEvalCase("w-64x48-n1-len60", (64, 48), 1, 60)      # ends on its terminal at step 54: six rows past the end
    out = _trace(case)
    assert out["len"][0] < case.max_ep_len
    for where in ((0, 3, 30), (0, 3, 31), (0, int(out["len"][0]), 0)):
        bad = dict(out, trace=out["trace"].copy())
        bad["trace"][where] = 1.0
        assert _fails(_env_check, bad, case), where


def test_a_trace_played_with_the_iteration_counts_swapped_is_seen():
    case = SMALL_CASE
    assert case.vit != case.pit
    out = _trace(case, swapped=True)
    wt.check_env_walker(out, case.seed, case.first, case.max_ep_len, case.pit, case.vit, case.id)      # sound for the budget it was played on
    assert _fails(_env_check, out, case)


# ---- the C ABI: name, prototype, rows ---------------------------------------------------------------------------------------------
def _headers():
    return [open(os.path.join(ROOT, "include", f)).read() for f in ("ddrl.h", "ddrl_walker.h", "ddrl_walker_eval.h")]


def test_the_new_name_in_its_header_the_ctypes_table_the_library_and_the_exports():
    import ctypes
    from distributed_drl_amd import _exports, _lib, env
    hdr, hdr_w, hdr_e = _headers()
    so = os.path.join(ROOT, "distributed-drl_amd", "libddrl_hip.so")
    assert os.path.exists(so), "libddrl_hip.so is not built"
    code = re.sub(r"/\*.*?\*/", "", hdr_e, flags=re.S)
    assert set(re.findall(r"\b(ddrl_[a-z0-9_]+)\s*\(", code)) == set(_lib.SIGNATURES_WALKER_EVAL) == {NAME}   # the header and its table, name for name
    assert not set(_lib.SIGNATURES_WALKER_EVAL) & set(_lib.SIGNATURES) and not set(_lib.SIGNATURES_WALKER_EVAL) & set(_lib.SIGNATURES_WALKER)
    assert _lib.SIGNATURES_WALKER_EVAL[NAME] == _lib.SIGNATURES["ddrl_env_eval_policy"]        # the arguments of the landers' entry point
    args = lambda f, h: [" ".join(p.split()) for p in re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % f, h, flags=re.S).group(1).split(",")]
    assert args(NAME, hdr_e) == args("ddrl_env_eval_policy", hdr)
    assert getattr(ctypes.CDLL(so), NAME) is not None
    lib = _lib.load()      # loads on the CPU; no compute call
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES_WALKER_EVAL[NAME][1]      # bound by _lib.load()
    assert re.search(r'#include "ddrl.h"', hdr_e) and NAME not in hdr and NAME not in hdr_w
    # the marker is exported, and the model table names the entry point and its trace row
    assert _exports._TABLE["DeviceBipedalWalker"] == "env" and env.DeviceBipedalWalker.on_device is True
    assert env.MODELS["walker"]["eval"] == (NAME, 32) and env.MODELS["walker"]["fused"] == {}
    for model in ("simple", "articulated"):
        assert env.MODELS[model]["eval"] == ("ddrl_env_eval_policy", 12)
    for row in env.MODELS.values():
        assert getattr(lib, row["eval"][0]) is not None


def test_the_new_declaration_has_its_stream_row():
    """tests/test_abi_table_cpu.py's checks, with its parse, on include/ddrl_walker_eval.h against tests/_abi_contract_walker_eval.TABLE:
    the declaration takes a stream and no caller device memory, it has a row, no row is for a function the header lacks, a deleted
    row or a new symbol fails the check.  And include/ddrl.h's own checks hold with the module imported."""
    import _abi_contract as ac
    import _abi_contract_walker_eval as ae
    from test_abi_table_cpu import stream_uncovered, takes_a_stream, takes_device_memory, uncovered
    hdr, _, hdr_e = _headers()
    assert takes_device_memory(hdr_e) == {} and takes_a_stream(hdr_e) == [NAME]
    assert stream_uncovered(hdr_e, ae.TABLE, {}) == [] and sorted(ae.TABLE) == [NAME]
    assert stream_uncovered(hdr_e, {}, {}) == [NAME]                                     # a deleted row fails
    grown = hdr_e.replace("#ifdef __cplusplus\n}", "int ddrl_x(float *y_d, void *stream);\n#ifdef __cplusplus\n}")
    assert grown != hdr_e and uncovered(grown, ae.TABLE, {}) == ["ddrl_x"] and stream_uncovered(grown, ae.TABLE, {}) == ["ddrl_x"]
    for f, rows in ae.TABLE.items():
        assert rows and all(cid in ae.STREAM_CASES and f in ae.STREAM_CASES[cid][1] for cid in rows), f
    assert sorted(c for rows in ae.TABLE.values() for c in rows) == sorted(ae.STREAM_CASES)
    assert not set(ae.STREAM_CASES) & set(ac.CASES) and not set(ae.STREAM_CASES) & set(ac.STREAM_CASES)
    # include/ddrl.h and its tables are as they were
    assert not set(ae.TABLE) & set(ac.STREAM_TABLE())
    assert uncovered(hdr, ac.TABLE, ac.EXEMPT) == [] and stream_uncovered(hdr, ac.STREAM_TABLE(), ac.STREAM_EXEMPT) == []


def test_walker_eval_hip_reads_no_handle_kind_and_is_a_translation_unit_of_its_own():
    from test_env_model_table_cpu import _code, _read, CSRC
    reads = re.compile(r"\bh\s*->\s*kind\b(?!\s*=[^=])|->\s*kind\s*[=!]=")
    for name in ("walker_eval.hip", "eval_host.h"):
        assert not reads.search(_code(_read(CSRC, name))), name
    code = _code(_read(CSRC, "walker_eval.hip"))
    assert re.search(r"__global__[^;{]*\bk_walker_eval\(", code) and "ddrl_env_refuse(" in code and "fmaf" not in code
    assert '#include "walker_device.h"' in _read(CSRC, "walker_eval.hip")
    # the landers' files do not see it
    for name in ("eval.hip", "eval_q.hip", "eval_episodes.h", "eval3.hip"):
        assert "k_walker_eval" not in _read(CSRC, name), name
