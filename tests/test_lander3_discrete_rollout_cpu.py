"""CPU half of the articulated lander's fused DISCRETE rollout step (ddrl_rollout_begin_discrete_articulated /
ddrl_rollout_step_discrete_articulated / ddrl_env_rollout_mirrors; GPU half: tests/test_gpu_lander3_discrete_rollout.py): the header
declares the three entry points, the ctypes table binds them, the library exports them, none of them takes caller device memory, and
the opt-in flag `opt.fused_discrete_rollout_articulated` is RolloutDeviceDQN's alone."""
import inspect
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NAMES = {"ddrl_rollout_begin_discrete_articulated": 3, "ddrl_rollout_step_discrete_articulated": 9, "ddrl_env_rollout_mirrors": 6}
FLAG = "fused_discrete_rollout_articulated"


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return open(os.path.join(root, "include", "ddrl.h")).read()


def test_header_signatures_and_exports():
    from distributed_drl_amd import _lib
    header = _header()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()      # loads on the CPU; no compute call
    for name, n_args in NAMES.items():
        m = re.search(r"\bint\s+%s\s*\(([^;{}]*?)\)\s*;" % name, code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n_args, name
        assert getattr(lib, name) is not None


def test_no_entry_point_takes_caller_device_memory():
    import test_abi_table_cpu as tab
    takes = tab.takes_device_memory(_header())
    for name in NAMES:
        assert name not in takes, (name, takes.get(name))


def test_the_flag_is_the_discrete_workers_alone_and_off_by_default():
    from distributed_drl_amd import workers
    src = inspect.getsource(workers.RolloutDeviceDQN)
    assert re.search(r'getattr\(\s*self\.opt\s*,\s*"%s"\s*,\s*False\s*\)' % FLAG, src)
    assert "ddrl_rollout_begin_discrete_articulated" in src and "ddrl_rollout_step_discrete_articulated" in src
    # the continuous worker's flag is another word, and the discrete worker does not read it
    assert "fused_rollout_articulated" not in src
    for cls in (workers.RolloutDevice, workers.RolloutDeviceNStep):
        assert FLAG not in inspect.getsource(cls), cls.__name__


def test_the_sqn_cases_of_the_gpu_half_sit_off_the_cumulative_boundaries():
    """tests/_lander3_discrete.py's header: at n = 64 the boundary cap of the action check allows no excluded row, so the SQN cases are
    chosen where the CPU replay has no row within 1e-4 relative of a boundary (ten times the check's own margin)."""
    import _lander3_discrete as l3
    sqn = [x for x in l3.Q_CASES if x[0] == "sqn"]
    assert len(sqn) == 2 and l3.Q_N == 64
    for fam, hidden, seed in sqn:
        assert l3.sqn_rows_near_a_boundary(l3.q_case(fam, hidden, seed), l3.Q_ENV_SEED, l3.Q_LIMIT, l3.Q_STEPS, margin=1e-4) == 0, (hidden, seed)


def test_env_model_kw_ignores_the_flag():
    from distributed_drl_amd import workers

    class Opt:
        env_model, env_velocity_iterations, env_position_iterations = "articulated", 8, 3
    want = dict(model="articulated", velocity_iterations=8, position_iterations=3)
    assert workers._env_model_kw(Opt()) == want
    for flag in (False, True):
        o = Opt()
        setattr(o, FLAG, flag)
        o.fused_rollout_articulated = flag
        assert workers._env_model_kw(o) == want
    o = type("O", (), {})()
    setattr(o, FLAG, True)
    assert workers._env_model_kw(o) == {}
