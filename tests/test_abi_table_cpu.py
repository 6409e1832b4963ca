"""CPU: (1) include/ddrl.h against the memory-contract table — every declaration that takes caller device memory has a row in
tests/_abi_contract.py or stands in its closed exemption list, so a symbol added to the header later fails here until it gets one;
(2) the arena checker of tests/_abi_arena.py against NumPy stand-in "kernels" with one planted fault at a time: each defect class is
reported, and by the property that names it (the way tests/test_oracle_acting_parity.py shows that its bars see planted defects)."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import _abi_arena as aa   # noqa: E402
import _abi_contract as ac   # noqa: E402

ALLOWED_EXEMPTIONS = {
    "ddrl_comm_bcast_params", "ddrl_comm_allreduce_grads", "ddrl_comm_send_batch", "ddrl_comm_recv_batch",
    "ddrl_replay_buffers", "ddrl_replay_buffers_ex", "ddrl_ps_buffer", "ddrl_sac1_grad_buffer", "ddrl_sac1_input_buffers",
    "ddrl_winq_buffers", "ddrl_dqn_step_timed", "ddrl_sac1_stage_time"}
HOST_POINTER_ARRAYS = ("src_h", "out_h", "region_base_h")


def takes_device_memory(header_text):
    """{function: [parameters]} of the declarations with a *_d parameter, one of the host arrays of device pointers, or a
    ddrl_rollout_nstep_out_t (whose members are device pointers)."""
    hdr = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    found = {}
    for m in re.finditer(r"\b(ddrl_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S):
        name, params = m.group(1), m.group(2)
        hits = []
        for p in params.split(","):
            p = " ".join(p.split())
            ident = re.findall(r"[A-Za-z_][A-Za-z0-9_]*", p)
            if not ident:
                continue
            if ident[-1].endswith("_d") or ident[-1] in HOST_POINTER_ARRAYS or "ddrl_rollout_nstep_out_t" in ident[:-1]:
                hits.append(ident[-1])
        if hits:
            found[name] = hits
    return found


def uncovered(header_text, table, exempt):
    return sorted(f for f in takes_device_memory(header_text) if f not in table and f not in exempt)


def _header():
    return open(os.path.join(os.path.dirname(HERE), "include", "ddrl.h")).read()


def test_every_declaration_with_caller_device_memory_has_a_row_or_a_stated_reason():
    need = takes_device_memory(_header())
    assert len(need) >= 60, sorted(need)                                 # the parse sees the header (70 such declarations today)
    assert "ddrl_rollout_step_nstep" in need and "ddrl_replay_store_ex" in need and "ddrl_dqn_loop_create" in need
    assert uncovered(_header(), ac.TABLE, ac.EXEMPT) == []
    assert set(ac.EXEMPT) <= ALLOWED_EXEMPTIONS, set(ac.EXEMPT) - ALLOWED_EXEMPTIONS   # the list is closed
    assert all(isinstance(r, str) and len(r) > 10 for r in ac.EXEMPT.values())
    assert not set(ac.EXEMPT) & set(ac.TABLE)
    assert set(ac.TABLE) <= set(need), set(ac.TABLE) - set(need)                       # no row for a function that does not exist
    for cid, (fn, functions) in ac.CASES.items():
        assert functions and callable(fn), cid
    for f, p in ac.REFUSALS:
        assert f in ac.TABLE, f


def test_a_deleted_row_or_a_new_symbol_fails_the_table_check():
    table = dict(ac.TABLE)
    del table["ddrl_winq_push"]
    assert uncovered(_header(), table, ac.EXEMPT) == ["ddrl_winq_push"]
    grown = _header().replace("#ifdef __cplusplus\n}", "int ddrl_x(float *y_d, void *stream);\n#ifdef __cplusplus\n}")
    assert grown != _header()
    assert uncovered(grown, ac.TABLE, ac.EXEMPT) == ["ddrl_x"]


# ---- the checker sees each defect class ------------------------------------------------------------------------------------------
N = 37


def _stand_in(fault=None):
    """y[i] = 2 x[i] + 1 over N floats, as a "kernel" on NumPy views of the context's memory, with one planted fault."""
    def fn(ctx):
        x = ctx.inp("x_d", np.arange(N, dtype=np.float32) * 0.5 - 3.0, ma=True)
        y = ctx.out("y_d", N, torch.float32, ma=True)

        def call():
            xv, yv = ctx.view("x_d", extra=1), ctx.view("y_d", extra=1)
            n_out = N - 1 if fault == "last_unwritten" else N
            yv[:n_out] = 2.0 * xv[:n_out] + 1.0
            if fault == "one_past":
                yv[N] = 7.0
            if fault == "input_changed":
                xv[3] = -1.0
            if fault == "zero_times_neighbour":
                with np.errstate(invalid="ignore"):
                    yv[N - 1] += np.float32(0.0) * xv[N]
            if fault == "offset_path_differs" and x % 16 != 0:
                yv[0] = np.nextafter(yv[0], np.float32(np.inf))
            return 0
        return call
    return fn


def _props(fault):
    return aa.run_case("stand-in:%s" % fault, _stand_in(fault), "cpu", capacity=1 << 20).props()


def test_the_checker_passes_a_clean_stand_in():
    c = aa.run_case("stand-in:clean", _stand_in(None), "cpu", capacity=1 << 20)
    assert c.failed == []
    c.report()


@pytest.mark.parametrize("fault,prop", [("one_past", "P1"), ("last_unwritten", "P2"), ("input_changed", "P3"),
                                        ("zero_times_neighbour", "P4"), ("offset_path_differs", "ALIGN")])
def test_the_checker_reports_each_planted_fault_by_its_property(fault, prop):
    got = _props(fault)
    assert prop in got, (fault, got)
    if fault in ("one_past", "input_changed"):
        assert got == [prop], (fault, got)      # (an unwritten element, a NaN neighbour and an offset path also differ from the twin: P2 beside them)
    with pytest.raises(AssertionError, match=prop):
        aa.run_case("stand-in:%s" % fault, _stand_in(fault), "cpu", capacity=1 << 20).report()


def test_guards_are_at_least_4096_bytes_and_the_buffer_size_and_int_outputs_get_the_byte_sentinel():
    ar = aa.Arena("cpu", 1 << 20)
    small, big = ar.carve(12, name="small"), ar.carve(40000, misalign_floats=1, name="big", dtype=torch.int64, word=aa.SENT_BYTE_WORD)
    for r in (small, big):
        assert r.off - r.lo >= max(4096, r.nbytes) and r.hi - (r.off + r.nbytes) >= max(4096, r.nbytes)
    assert small.off % 256 == 0 and big.off % 256 == 4 and small.hi <= big.lo
    ar.arm()
    assert ar.guards_intact() == [] and not ar.all_overwritten(small) and not ar.all_overwritten(big)
    assert int(ar.region(small, torch.int32)[0]) == np.uint32(0x7FC0DEAD).view(np.int32)
    assert bool((ar.region(big) == 0xA5).all())
    ar.region(big, torch.uint8)[:] = 1
    ar.region(small, torch.float32)[:] = 0.0
    assert ar.all_overwritten(big) and ar.all_overwritten(small) and ar.guards_intact() == []
    ar.buf[big.off + big.nbytes] = 0                      # the first byte behind the extent
    assert ar.guards_intact() == ["big"]
