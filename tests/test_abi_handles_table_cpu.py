"""CPU: include/ddrl.h against the table of the handle kinds that come through another door (tests/_abi_contract_handles.py).  Every
function of ddrl.h that has a row in tests/_abi_contract.py's memory or stream table and takes a learner or an actor handle
(ddrl_sac1_t *, ddrl_dqn_t *, ddrl_actor_t *) has, for EVERY kind of that handle — sac1-wide and sacv-wide, ddqn-direct and sqn-direct,
actor-wide — a row in that module's TABLE or an entry with a reason in its EXEMPT, whose keys are a closed set written out here.  A
function added to the header later fails here for each kind of its handle until it has one or the other."""
import os
import re
import sys

import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_contract as ac   # noqa: E402
import _abi_contract_handles as ah   # noqa: E402
import _abi_contract_lander3_nstep   # noqa: E402,F401  (its rows enter ac.TABLE on import, as in tests/test_abi_table_cpu.py)
from test_abi_table_cpu import _header, takes_a_stream, takes_device_memory   # noqa: E402

_ROLLOUT_STEPS = ("ddrl_rollout_step", "ddrl_rollout_step_articulated", "ddrl_rollout_step_nstep", "ddrl_rollout_step_nstep_articulated",
                  "ddrl_rollout_begin_nstep_articulated")
ALLOWED_EXEMPTIONS = (
    {(k, f) for k in ("sac1-wide", "sacv-wide") for f in ("ddrl_sac1_grad_buffer", "ddrl_sac1_input_buffers", "ddrl_sac1_stage_time")}
    | {(k, "ddrl_dqn_step_timed") for k in ("ddqn-direct", "sqn-direct")}
    | {("actor-wide", f) for f in _ROLLOUT_STEPS})


def takes_a_handle(header_text):
    """{function: handle type} of the declarations with a parameter of type ddrl_sac1_t *, ddrl_dqn_t * or ddrl_actor_t *."""
    hdr = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    found = {}
    for m in re.finditer(r"\b(ddrl_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S):
        for t in ah.HANDLE_KINDS:
            if re.search(r"\b%s\s*\*\s*[A-Za-z_]" % t, m.group(2)):
                found[m.group(1)] = t
    return found


def needed(header_text, covered):
    """The (kind, function) pairs that need a row or a reason: the functions of `header_text` that take caller device memory or a
    stream and a handle type that has kinds, and are in `covered` (the functions with a row in _abi_contract's tables) — or in none of
    its lists yet, as a declaration added to the header is."""
    rows = set(takes_device_memory(header_text)) | set(takes_a_stream(header_text))
    exempt_there = (set(ac.EXEMPT) | set(ac.STREAM_EXEMPT)) - covered
    return sorted((k, f) for f, t in takes_a_handle(header_text).items() if f in rows and f not in exempt_there
                  for k in ah.HANDLE_KINDS[t])


def uncovered(header_text, table, exempt):
    covered = set(ac.TABLE) | set(ac.STREAM_TABLE())
    return [p for p in needed(header_text, covered) if p not in table and p not in exempt]


def test_every_handle_function_has_a_row_or_a_stated_reason_for_every_kind():
    need = needed(_header(), set(ac.TABLE) | set(ac.STREAM_TABLE()))
    assert len(need) >= 83, len(need)                      # the parse sees the header (83 such (kind, function) pairs today)
    for p in (("sac1-wide", "ddrl_sac1_step"), ("sacv-wide", "ddrl_sac1_apply_grads"), ("sqn-direct", "ddrl_dqn_loop_create"),
              ("ddqn-direct", "ddrl_env_eval_q"), ("actor-wide", "ddrl_rollout_begin_nstep")):
        assert p in need, p
    assert uncovered(_header(), ah.TABLE, ah.EXEMPT) == []
    assert set(ah.EXEMPT) <= ALLOWED_EXEMPTIONS, set(ah.EXEMPT) - ALLOWED_EXEMPTIONS     # the list is closed
    assert all(isinstance(r, str) and len(r) > 10 for r in ah.EXEMPT.values())
    assert not set(ah.EXEMPT) & set(ah.TABLE)
    declared = takes_a_handle(_header())
    for kind, f in list(ah.TABLE) + list(ah.EXEMPT):       # no row and no reason for a function the header lacks, or of another handle
        assert kind in ah.KINDS and (f in declared and kind in ah.HANDLE_KINDS[declared[f]] or f in ("ddrl_loop_run", "ddrl_dqn_loop_run")), (kind, f)
    for cases in (ah.CASES, ah.STREAM_CASES):
        for cid, (fn, functions) in cases.items():
            assert functions and callable(fn), cid
    assert not set(ah.CASES) & set(ah.STREAM_CASES)
    assert not (set(ah.CASES) | set(ah.STREAM_CASES)) & (set(ac.CASES) | set(ac.STREAM_CASES))
    assert ah.REFUSAL_CASES and set(ah.REFUSAL_CASES) <= set(ah.CASES)


def test_the_module_enters_no_row_in_the_tables_of_ddrl_h():
    """tests/test_gpu_abi_memory.py and test_gpu_abi_stream.py parametrise over _abi_contract's dicts at import: their case lists must
    not depend on whether this module was imported."""
    for cid in list(ah.CASES) + list(ah.STREAM_CASES):
        assert cid not in ac.CASES and cid not in ac.STREAM_CASES, cid
    for ids in list(ac.TABLE.values()) + list(ac.STREAM_ROWS.values()):
        assert not set(ids) & (set(ah.CASES) | set(ah.STREAM_CASES)), ids


def test_a_deleted_row_or_a_new_symbol_fails_the_table_check():
    table = dict(ah.TABLE)
    del table[("sqn-direct", "ddrl_dqn_act")]
    assert uncovered(_header(), table, ah.EXEMPT) == [("sqn-direct", "ddrl_dqn_act")]
    grown = _header().replace("#ifdef __cplusplus\n}", "int ddrl_sac1_x(ddrl_sac1_t *h, float *y_d, void *stream);\n#ifdef __cplusplus\n}")
    assert grown != _header()
    assert uncovered(grown, ah.TABLE, ah.EXEMPT) == [("sac1-wide", "ddrl_sac1_x"), ("sacv-wide", "ddrl_sac1_x")]
