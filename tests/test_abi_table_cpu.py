"""CPU: (1) include/ddrl.h against the memory-contract table — every declaration that takes caller device memory has a row in
tests/_abi_contract.py or stands in its closed exemption list, so a symbol added to the header later fails here until it gets one;
(2) the arena checker of tests/_abi_arena.py against NumPy stand-in "kernels" with one planted fault at a time: each defect class is
reported, and by the property that names it (the way tests/test_oracle_acting_parity.py shows that its bars see planted defects)."""
import ctypes
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
import _abi_contract_lander3_nstep   # noqa: E402,F401  (its rows enter ac.TABLE on import)

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


# ---- the stream contract: (1) every function that takes `void *stream` has a row or a stated reason ------------------------------------
ALLOWED_STREAM_EXEMPTIONS = {"ddrl_comm_bcast_params", "ddrl_comm_allreduce_grads", "ddrl_comm_send_batch", "ddrl_comm_recv_batch",
                             "ddrl_dqn_step_timed", "ddrl_sac1_stage_time"}


def takes_a_stream(header_text):
    """The declarations with a `void *stream` parameter."""
    hdr = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"\b(ddrl_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr, flags=re.S)
                  if re.search(r"\bvoid\s*\*\s*stream\b", m.group(2)))


def stream_uncovered(header_text, table, exempt):
    return [f for f in takes_a_stream(header_text) if f not in table and f not in exempt]


def test_every_declaration_that_takes_a_stream_has_a_row_or_a_stated_reason():
    need = takes_a_stream(_header())
    assert len(need) >= 94, len(need)                                     # the parse sees the header (94 such declarations today)
    assert "ddrl_loop_run" in need and "ddrl_replay_seed" in need and "ddrl_env_eval_q" in need and "ddrl_replay_buffers" not in need
    table = ac.STREAM_TABLE()
    assert stream_uncovered(_header(), table, ac.STREAM_EXEMPT) == []
    assert set(ac.STREAM_EXEMPT) <= ALLOWED_STREAM_EXEMPTIONS, set(ac.STREAM_EXEMPT) - ALLOWED_STREAM_EXEMPTIONS    # the list is closed
    assert all(isinstance(r, str) and len(r) > 10 for r in ac.STREAM_EXEMPT.values())
    assert not set(ac.STREAM_EXEMPT) & set(table)
    assert set(ac.STREAM_ROWS) <= set(need), set(ac.STREAM_ROWS) - set(need)     # a stream row is for a function that takes a stream
    assert not set(ac.STREAM_CASES) & set(ac.CASES)
    for cid, (fn, functions) in ac.STREAM_CASES.items():
        assert functions and callable(fn), cid


def test_a_deleted_stream_row_or_a_new_symbol_fails_the_stream_table_check():
    for f in sorted(ac.STREAM_ROWS):                                      # every new row is needed: none hides behind a memory row
        table = ac.STREAM_TABLE()
        del table[f]
        assert stream_uncovered(_header(), table, ac.STREAM_EXEMPT) == [f]
    table = ac.STREAM_TABLE()
    del table["ddrl_winq_push"]
    assert stream_uncovered(_header(), table, ac.STREAM_EXEMPT) == ["ddrl_winq_push"]
    grown = _header().replace("#ifdef __cplusplus\n}", "int ddrl_x(ddrl_env_t *h, void *stream);\n#ifdef __cplusplus\n}")
    assert grown != _header()
    assert stream_uncovered(grown, ac.STREAM_TABLE(), ac.STREAM_EXEMPT) == ["ddrl_x"]


# ---- (2) S sees its faults: a stream is a deferred queue, the stand-ins are NumPy "kernels" on it ------------------------------------------
def _stream_stand_in(fault=None):
    """y = 2 x + 1 over N floats and total_h = sum(x) (a host output behind a stream sync), enqueued on the caller's stream ctx.stream —
    with one planted stream fault."""
    def fn(ctx):
        x = ctx.inp("x_d", np.arange(N, dtype=np.float32) * 0.5 - 3.0)
        y = ctx.out("y_d", N, torch.float32)
        total = ctx.host("total_h", 1, ctypes.c_double)
        assert x and y

        def call():
            s = ctx.stream_arg
            dev = s.device
            xv, yv = ctx.view("x_d"), ctx.view("y_d")
            acc = np.zeros(1)

            def kernel(lo=0, hi=N):
                yv[lo:hi] = 2.0 * xv[lo:hi] + 1.0

            def reduce():
                acc[0] = float(xv.astype(np.float64).sum())

            if fault == "ignores_its_stream":
                dev.null_stream().enqueue(kernel)
            elif fault == "last_write_bypasses_its_stream":
                s.enqueue(lambda: kernel(0, N - 1))
                dev.null_stream().enqueue(lambda: kernel(N - 1, N))
            elif fault == "unjoined_second_queue":
                dev.new_stream().enqueue(kernel)
            else:
                s.enqueue(kernel)
            s.enqueue(reduce)
            if fault == "syncs_the_wrong_queue":
                dev.new_stream().synchronize()
            else:
                s.synchronize()
            total[0] = acc[0]
            return 0
        return call
    return fn


def _stream_run(fault, side=None):
    twin = aa.ModelDevice(eager=True)
    return aa.run_stream_case("stream stand-in:%s" % fault, _stream_stand_in(fault), "cpu", None, side or aa.ModelSide(),
                              plain_stream=twin.null_stream(), capacity=1 << 20)


def test_the_stream_run_passes_a_clean_stand_in():
    c = _stream_run(None)
    assert c.failed == []
    c.report()


@pytest.mark.parametrize("fault,prop", [("ignores_its_stream", "S-early"), ("last_write_bypasses_its_stream", "S-early"),
                                        ("unjoined_second_queue", "S-late"), ("syncs_the_wrong_queue", "S-sync")])
def test_the_stream_run_reports_each_planted_fault_by_its_property(fault, prop):
    got = _stream_run(fault).props()
    assert prop in got, (fault, got)
    assert not {"S-early", "S-late", "S-sync"} - {prop} & set(got), (fault, got)       # and by no other S property
    assert "P1" not in got and "VOID" not in got and "RC" not in got, (fault, got)
    with pytest.raises(AssertionError, match=prop):
        _stream_run(fault).report()


def _handle_stand_in(ahead, fault=None):
    """A stand-in that touches HANDLE state only, the shape of ddrl_replay_seed or ddrl_rollout_begin: `double` doubles a handle array
    that the setup settled before the gate; `load` (a call that adds the caller's x_d to the handle, on the caller's stream) and
    `export` (handle -> y_d, on the caller's stream) stand around it.  fault: `double` ignores its stream."""
    def fn(ctx):
        assert ctx.inp("x_d", np.arange(N, dtype=np.float32) * 0.5 - 3.0) and ctx.out("y_d", N, torch.float32)
        handle = np.linspace(1.0, 2.0, N).astype(np.float32)

        def call():
            s = ctx.stream_arg
            xv, yv = ctx.view("x_d"), ctx.view("y_d")

            def load():
                handle[:] += xv

            def double():
                handle[:] *= 2.0

            def export():
                yv[:] = handle

            if ahead:
                s.enqueue(load)
            (s.device.null_stream() if fault else s).enqueue(double)
            s.enqueue(export)
            return 0
        return call
    return fn


def _handle_run(ahead, fault):
    twin = aa.ModelDevice(eager=True)
    return aa.run_stream_case("handle stand-in", _handle_stand_in(ahead, fault), "cpu", None, aa.ModelSide(),
                              plain_stream=twin.null_stream(), capacity=1 << 20)


def test_a_handle_only_call_off_its_stream_is_reported_behind_a_call_ahead_and_only_there():
    """Why every stream row of tests/_abi_contract.py puts a call that does not commute with the call under test ahead of it: a call
    that touches handle state only and ran during the gate is invisible when it is the closure's first call (the blind spot), and is
    reported as S-early once a call fed from a late-written input stands ahead of it."""
    for ahead in (False, True):
        assert _handle_run(ahead, None).failed == []
    assert _handle_run(False, "ignores_its_stream").failed == []          # the blind spot, shown so that it stays known
    got = _handle_run(True, "ignores_its_stream").props()
    assert "S-early" in got and "P2" in got and not {"S-late", "S-sync", "VOID", "P1", "RC"} & set(got), got
    with pytest.raises(AssertionError, match="S-early"):
        _handle_run(True, "ignores_its_stream").report()


def test_a_gate_that_came_out_short_makes_the_run_void():
    got = _stream_run(None, aa.ModelSide(gate_ms=10.0, measured_ms=7.5)).props()
    assert got == ["VOID"], got


def test_the_decoy_is_what_a_call_outside_its_stream_reads():
    """The S run's own premises on the model: before the late writes an input holds its elements rotated by one, the staging image holds
    the true value, and P3 compares with the true value."""
    side = aa.ModelSide()
    ctx = aa.StreamCtx("cpu", None, side, capacity=1 << 20)
    x = np.arange(N, dtype=np.float32)
    ctx.inp("x_d", x)
    ctx.out("y_d", N, torch.float32)
    ctx.arm()
    assert np.array_equal(ctx.view("x_d"), np.roll(x, 1))
    ctx.view("y_d")[:] = 5.0
    side.enqueue(ctx.late_writes)
    assert np.array_equal(ctx.view("x_d"), np.roll(x, 1))
    side.synchronize()
    assert np.array_equal(ctx.view("x_d"), x) and ctx.arena.unchanged(ctx.bufs["x_d"]["r"])
    assert not ctx.arena.all_overwritten(ctx.bufs["y_d"]["r"])
