"""The shape of the env family's host code, read from the sources (no GPU, no library):

* csrc/env.hip is host code only — no `__global__`, no `<<<`: every kernel lives in its model's own translation unit, so an edit to the
  entry points cannot change what a kernel compiles to;
* every DDRL_ENV_* kind of include/ddrl.h has exactly one row in env.hip's model table;
* the walker's reset / step / wrapped-step kernels exist once, in csrc/walker.hip, as templates over the terrain mode, with one
  put_obs24 and one put_stats, behind three launch functions that take the mode as their first argument;
* a handle's kind is read or tested (`h->kind` but on the left of an assignment, `->kind ==` / `!=`) only inside the table lookup
  (env_model_of) and the one guard function (ddrl_env_refuse) — and in eval3.hip's two choices between the Env3 evaluation launch and the one-body entry point,
  which are the evaluation family's own and are counted here so that they cannot multiply;
* the Python side picks the C entry points by model in one table (env.MODELS), whose names the library exports."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed-drl_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _code(src):
    """The source without // and /* */ comments and without string literals' contents."""
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', src)
    return re.sub(r"//[^\n]*", "", src)


def _function_body(code, head):
    """The brace-balanced body of the function whose definition starts with `head`."""
    at = code.index(head)
    start = code.index("{", at)
    depth = 0
    for i in range(start, len(code)):
        depth += {"{": 1, "}": -1}.get(code[i], 0)
        if depth == 0:
            return start, i + 1
    raise AssertionError(head)


def test_env_hip_is_host_code_only():
    code = _code(_read(CSRC, "env.hip"))
    assert "__global__" not in code and "<<<" not in code
    lander = _code(_read(CSRC, "lander.hip"))
    for kernel in ("k_env_reset", "k_env_step", "k_env_step_wrapped", "k_env_step_pi", "k_env_step_q", "k_env_obs"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, lander), kernel


def test_every_kind_has_exactly_one_table_row():
    header = re.sub(r"/\*.*?\*/", "", _read(ROOT, "include", "ddrl.h"), flags=re.S)
    kinds = dict(re.findall(r"^#define (DDRL_ENV_[A-Z_]+) (\d+)\s*$", header, flags=re.M))
    kinds = {k: v for k, v in kinds.items() if not k.endswith("_FIELDS")}
    assert set(kinds) == {"DDRL_ENV_ONE_BODY", "DDRL_ENV_ARTICULATED", "DDRL_ENV_WALKER"} and len(set(kinds.values())) == 3
    code = _code(_read(CSRC, "env.hip"))
    a, b = _function_body(code, "static const EnvModel ENV_MODELS[]")
    rows = re.findall(r"\{\s*(DDRL_ENV_[A-Z_]+)\s*,", code[a:b])
    assert sorted(rows) == sorted(kinds), rows


def test_the_walkers_step_kernels_exist_once_behind_the_terrain_mode():
    assert not os.path.exists(os.path.join(CSRC, "walker_nstep.hip")) and not os.path.exists(os.path.join(CSRC, "walker_hardcore.hip"))
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            text = _read(CSRC, name)
            assert not any(old in text for old in ("k_walker_hc_reset", "k_walker_hc_step", "ddrl_walker_hc_launch")), name
    code = _code(_read(CSRC, "walker.hip"))
    kernels = re.findall(r"(template <int HC>\s*)?__global__[^;{]*\b(k_\w+)\(", code)
    assert kernels and all(t for t, _ in kernels)
    assert sorted(k for _, k in kernels) == ["k_walker_reset", "k_walker_step", "k_walker_step_wrapped"] and code.count("__global__") == 3
    assert code.count("e.physics(") == 3
    for helper in ("put_obs24", "put_stats"):
        assert len(re.findall(r"\bvoid %s\(" % helper, code)) == 1, helper
    launches = re.findall(r"^int (ddrl_walker_launch_\w+)\(int hardcore,", _code(_read(CSRC, "env_launch.h")), flags=re.M)
    assert sorted(launches) == ["ddrl_walker_launch_reset", "ddrl_walker_launch_step", "ddrl_walker_launch_step_wrapped"]
    assert len(re.findall(r"\bddrl_walker_\w*launch_\w+\(", _code(_read(CSRC, "env_launch.h")))) == 3


def test_a_handles_kind_is_read_in_the_lookup_and_the_guard_only():
    reads = re.compile(r"\bh\s*->\s*kind\b(?!\s*=[^=])|->\s*kind\s*[=!]=")   # `h->kind` (but for `h->kind = ...`), `->kind ==`
    allowed = {"env.hip": ("static const EnvModel *env_model_of(", "int ddrl_env_refuse("), "eval3.hip": ()}
    found = {}
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        code = _code(_read(CSRC, name))
        spans = [_function_body(code, head) for head in allowed.get(name, ())]
        outside = [m.start() for m in reads.finditer(code) if not any(a <= m.start() < b for a, b in spans)]
        if outside:
            found[name] = len(outside)
    assert found == {"eval3.hip": 2}, found
    env = _code(_read(CSRC, "env.hip"))
    for macro in ("DDRL_ONE_BODY_ONLY", "DDRL_ARTICULATED_ONLY", "DDRL_REFUSE_WALKER"):
        assert all(macro not in _read(CSRC, n) for n in os.listdir(CSRC) if n.endswith((".hip", ".h"))), macro
    assert len(re.findall(r"\bddrl_env_refuse\(", env)) >= 12 and "ddrl_env_refuse(" in _code(_read(CSRC, "eval3.hip"))


def test_the_python_table_names_entry_points_that_exist():
    from distributed_drl_amd import _lib, env
    assert set(env.MODELS) == {"simple", "articulated", "walker"}
    lib = _lib.load()      # loads on the CPU; no compute call
    for model, row in env.MODELS.items():
        assert callable(getattr(row["cls"], row["wrapped"])), model
        assert getattr(lib, "ddrl_env_" + row["wrapped"]) is not None
        for family, (begin, step, opt_in, handles_only) in row["fused"].items():
            assert family in ("pi", "q", "nstep") and getattr(lib, begin) is not None and getattr(lib, step) is not None, (model, family)
            assert opt_in == (model != "simple")
    assert env.MODELS["walker"]["fused"] == {} and env.MODELS["walker"]["dims"] == (env.VecBipedalWalker.obs_dim, env.VecBipedalWalker.act_dim)
    # workers.py tests no model name outside the walker's refusal by the discrete worker (_no_walker) and the default of _env_model_kw
    src = re.sub(r'""".*?"""', "", _read(ROOT, "distributed-drl_amd", "workers.py"), flags=re.S)
    assert not re.search(r"env\.model\s*[=!]=", src)
