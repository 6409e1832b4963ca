"""CPU half of the Hardcore walker's evaluation-trace checks (tests/_walker_hardcore_eval_trace.py): on traces built from the oracles
alone — _acting_parity.forward32 and WalkerHardcoreOracle — check_env_walker_hardcore and check_policy pass; each of the five planted
defects of _eval_trace.DEFECTS and a trace played with the velocity and position iteration counts swapped are seen; and the fixed inputs
meet the conditions the GPU half (tests/test_gpu_walker_hardcore_eval.py) relies on: the endings, a lidar ray on a box edge in every
case that claims one, and a departure from the grass walker's trace in the terminal case (a kernel that built grass fails it).
Also: include/ddrl_walker_hardcore_eval.h declares exactly the one entry point, its ctypes table and the library name it with the
arguments of ddrl_env_eval_policy, its stream row stands in tests/_abi_contract_walker_hardcore_eval.TABLE, the package exports the
marker, csrc/walker_hardcore_eval.hip reads no handle kind, and the Python doors: the old ones stay shut on the Hardcore terrain, the
new flag opens the new marker.

What these inputs do NOT reach: an evaluation episode starts 4.7 m in front of its first obstacle and the test policies fall (steps
54 / 79) or stand; no leg corner or hull vertex touches a box.  The box-contact branches of WalkerT<1> stay held by the crafted-state
tests of the same text (tests/test_gpu_walker_hardcore_scenarios.py).  What is the evaluation kernel's own — the n = 1 LDS column, the
generator writing the box rows into it and the lidar reading them — is what the box-ray steps below exercise."""
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
import _walker_hardcore_eval_trace as ht  # noqa: E402

NAME = "ddrl_env_eval_policy_walker_hardcore"
GRASS_NAME = "ddrl_env_eval_policy_walker"
HARDCORE_ENV = "BipedalWalkerHardcore-v2"
SMALL_CASE = ht.WalkerEvalCase("wh-64x48-n2-len40", (64, 48), 2, 40)     # both episodes end on the time limit; a box ray in the second
_TRACES = {}


def _trace(case, defect=None, swapped=False):
    key = (case.id, defect, swapped)
    if key not in _TRACES:
        kw = dict(vit=case.pit, pit=case.vit) if swapped else {}
        _TRACES[key] = ht.oracle_trace_walker_hardcore(case, ht.params_of(case), defect, **kw)
    return _TRACES[key]


def _fails(check, *a, **kw):
    try:
        check(*a, **kw)
    except AssertionError:
        return True
    return False


def _env_check(out, case):
    ht.check_env_walker_hardcore(out, case.seed, case.first, case.max_ep_len, case.vit, case.pit, case.id)


@pytest.mark.parametrize("case", [SMALL_CASE] + ht.TRACE_CASES, ids=repr)
def test_checks_pass_on_the_oracles_trace(case):
    out = _trace(case)
    _env_check(out, case)
    ht.check_policy(out, case, ht.params_of(case))


def test_inputs_reach_the_endings_the_box_rays_and_the_departure_the_gpu_half_relies_on():
    last = lambda out: np.array([out["trace"][e, l - 1] for e, l in enumerate(out["len"])])
    # every episode ends on a terminal at step 54; the three returns differ
    out = _trace(ht.TERMINAL_CASE)
    assert out["len"].tolist() == [54, 54, 54] and (last(out)[:, ht.I_REW] == -100).all() and (last(out)[:, ht.I_END] == 1).all()
    assert len(set(out["ret"].tolist())) == 3
    # ... and the Hardcore terrain is seen: the same policy on the grass walker of the same seed acts on other observations from some
    # step before the end on (the lidar meets a box edge), so a kernel that built the grass terrain fails this case
    grass = wt.oracle_trace_walker(wt.TERMINAL_CASE, wt.params_of(wt.TERMINAL_CASE))
    assert ht.TERMINAL_CASE.policy.seed == wt.TERMINAL_CASE.policy.seed and ht.TERMINAL_CASE.seed == wt.TERMINAL_CASE.seed
    differs = (ht._bits(out["trace"][0, :, :ht.OBS]) != ht._bits(grass["trace"][0, :, :ht.OBS])).any(axis=1)
    assert differs.any() and 0 < int(np.argmax(differs)) < int(out["len"][0])
    assert _fails(wt.check_env_walker, out, 3, 0, 120, 8, 3) and _fails(_env_check, grass, ht.TERMINAL_CASE)
    # the full-width row: a terminal at step 79
    out = _trace(ht.WIDE_CASE)
    assert out["len"].tolist() == [79, 79] and (last(out)[:, ht.I_REW] == -100).all()
    # h1 and h2 off 16: the time limit
    case, out = ht.LIMIT_CASE, _trace(ht.LIMIT_CASE)
    assert case.hid[0] % 16 and case.hid[1] % 16
    assert (out["len"] == case.max_ep_len).all() and (last(out)[:, ht.I_REW] != -100).all() and (last(out)[:, ht.I_END] == 1).all()
    # the rest end on the limit; the small case of the defect tests too
    for case in [ht.ONE_STEP_CASE, ht.GYM_CASE, SMALL_CASE] + list(ht.FIRST_CASES):
        out = _trace(case)
        assert (out["len"] == case.max_ep_len).all() and (last(out)[:, ht.I_END] == 1).all() and (last(out)[:, ht.I_REW] != -100).all(), case
    # a lidar ray ends on a box edge on at least one acted-on observation of every case that claims one (the gym iteration counts
    # among them), and in more than one episode of the eight
    assert ht.GYM_CASE in ht.BOX_RAY_CASES and (ht.GYM_CASE.vit, ht.GYM_CASE.pit) == (180, 60)
    for case in ht.BOX_RAY_CASES + [SMALL_CASE]:
        assert _trace(case)["box_steps"].sum() >= 1, case
    assert (_trace(ht.FIRST_CASES[0])["box_steps"] > 0).sum() >= 2
    # the two first-episode cases overlap in episodes 5..7
    long, short = ht.FIRST_CASES
    assert (long.first, long.n, short.first, short.n) == (0, 8, 5, 3)
    assert (ht._bits(_trace(long)["trace"][5:8]) == ht._bits(_trace(short)["trace"])).all()


@pytest.mark.parametrize("defect", et.DEFECTS)
def test_planted_defect_fails_a_check(defect):
    case = SMALL_CASE
    assert case.n > 1      # episode_index_not_advanced needs a second episode
    out, params = _trace(case, defect), ht.params_of(case)
    env_fails = _fails(_env_check, out, case)
    pol_fails = _fails(ht.check_policy, out, case, params)
    # each defect is seen by the half it belongs to
    if defect in ("action_from_previous_obs", "last_hidden2_dropped"):
        assert pol_fails, defect
    else:
        assert env_fails, defect


def test_a_trace_played_with_the_iteration_counts_swapped_is_seen():
    case = SMALL_CASE
    assert case.vit != case.pit
    out = _trace(case, swapped=True)
    ht.check_env_walker_hardcore(out, case.seed, case.first, case.max_ep_len, case.pit, case.vit, case.id)      # sound for the budget it was played on
    assert _fails(_env_check, out, case)


# ---- the C ABI: name, prototype, rows ---------------------------------------------------------------------------------------------
def _hdr(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _declared(h):
    return set(re.findall(r"\b(ddrl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", h, flags=re.S)))


def test_the_new_name_in_its_header_the_ctypes_table_the_library_and_the_exports():
    import ctypes
    import distributed_drl_amd as d
    from distributed_drl_amd import _exports, _lib, env
    hdr, hdr_he = _hdr("ddrl.h"), _hdr("ddrl_walker_hardcore_eval.h")
    so = os.path.join(ROOT, "distributed-drl_amd", "libddrl_hip.so")
    assert os.path.exists(so), "libddrl_hip.so is not built"
    assert _declared(hdr_he) == set(_lib.SIGNATURES_WALKER_HARDCORE_EVAL) == {NAME}      # the header and its table, name for name
    for other in (_lib.SIGNATURES, _lib.SIGNATURES_WALKER, _lib.SIGNATURES_WALKER_EVAL, _lib.SIGNATURES_WALKER_HARDCORE):
        assert not set(_lib.SIGNATURES_WALKER_HARDCORE_EVAL) & set(other)
    assert _lib.SIGNATURES_WALKER_HARDCORE_EVAL[NAME] == _lib.SIGNATURES["ddrl_env_eval_policy"]      # the arguments of the landers' entry point
    args = lambda f, h: [" ".join(p.split()) for p in re.search(r"\bint %s\s*\(([^;]*?)\)\s*;" % f, h, flags=re.S).group(1).split(",")]
    assert args(NAME, hdr_he) == args("ddrl_env_eval_policy", hdr) == args(GRASS_NAME, _hdr("ddrl_walker_eval.h"))
    assert getattr(ctypes.CDLL(so), NAME) is not None
    lib = _lib.load()      # loads on the CPU; no compute call
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES_WALKER_HARDCORE_EVAL[NAME][1] and getattr(lib, NAME).restype is ctypes.c_int
    # the header stands beside ddrl.h, which names it and does not declare its function; the sibling headers keep their one declaration
    assert re.search(r'#include "ddrl.h"', hdr_he) and "ddrl_walker_hardcore_eval.h" in hdr and NAME not in _declared(hdr)
    assert _declared(hdr) == set(_lib.SIGNATURES)
    for sib, table in (("ddrl_walker.h", _lib.SIGNATURES_WALKER), ("ddrl_walker_eval.h", _lib.SIGNATURES_WALKER_EVAL),
                       ("ddrl_walker_hardcore.h", _lib.SIGNATURES_WALKER_HARDCORE)):
        assert _declared(_hdr(sib)) == set(table) and len(table) == 1, sib
    # the marker is exported and names its entry point and trace row itself; the model table is as it was
    assert _exports._TABLE["DeviceBipedalWalkerHardcore"] == "env" and d.DeviceBipedalWalkerHardcore is env.DeviceBipedalWalkerHardcore
    assert env.DeviceBipedalWalkerHardcore.eval_entry == (NAME, 32) and env.DeviceBipedalWalkerHardcore.on_device is True
    assert set(env.MODELS) == {"simple", "articulated", "walker"}
    assert env.MODELS["walker"]["eval"] == (GRASS_NAME, 32) and env.MODELS["walker"]["fused"] == {}
    assert not hasattr(env.DeviceBipedalWalker, "eval_entry")      # the grass marker goes through the table


def test_the_new_declaration_has_its_stream_row():
    """tests/test_abi_table_cpu.py's checks, with its parse, on include/ddrl_walker_hardcore_eval.h against
    tests/_abi_contract_walker_hardcore_eval.TABLE: the declaration takes a stream and no caller device memory, it has a row, no row is
    for a function the header lacks, a deleted row or a new symbol fails the check.  And include/ddrl.h's own checks hold with the
    module imported."""
    import _abi_contract as ac
    import _abi_contract_walker_eval as ae
    import _abi_contract_walker_hardcore_eval as ahe
    from test_abi_table_cpu import stream_uncovered, takes_a_stream, takes_device_memory, uncovered
    hdr, hdr_he = _hdr("ddrl.h"), _hdr("ddrl_walker_hardcore_eval.h")
    assert takes_device_memory(hdr_he) == {} and takes_a_stream(hdr_he) == [NAME]
    assert stream_uncovered(hdr_he, ahe.TABLE, {}) == [] and sorted(ahe.TABLE) == [NAME]
    assert stream_uncovered(hdr_he, {}, {}) == [NAME]                                     # a deleted row fails
    grown = hdr_he.replace("#ifdef __cplusplus\n}", "int ddrl_x(float *y_d, void *stream);\n#ifdef __cplusplus\n}")
    assert grown != hdr_he and uncovered(grown, ahe.TABLE, {}) == ["ddrl_x"] and stream_uncovered(grown, ahe.TABLE, {}) == ["ddrl_x"]
    for f, rows in ahe.TABLE.items():
        assert rows and all(cid in ahe.STREAM_CASES and f in ahe.STREAM_CASES[cid][1] for cid in rows), f
    assert sorted(c for rows in ahe.TABLE.values() for c in rows) == sorted(ahe.STREAM_CASES)
    assert not set(ahe.STREAM_CASES) & (set(ac.CASES) | set(ac.STREAM_CASES) | set(ae.STREAM_CASES))
    # include/ddrl.h, the grass twin's header and their tables are as they were
    assert not set(ahe.TABLE) & set(ac.STREAM_TABLE()) and not set(ahe.TABLE) & set(ae.TABLE)
    assert uncovered(hdr, ac.TABLE, ac.EXEMPT) == [] and stream_uncovered(hdr, ac.STREAM_TABLE(), ac.STREAM_EXEMPT) == []
    assert stream_uncovered(_hdr("ddrl_walker_eval.h"), ae.TABLE, {}) == []


def test_walker_hardcore_eval_hip_runs_the_hardcore_walker_and_shares_the_episode_text():
    from test_env_model_table_cpu import _code, _read, CSRC
    reads = re.compile(r"\bh\s*->\s*kind\b(?!\s*=[^=])|->\s*kind\s*[=!]=")
    names = ("walker_hardcore_eval.hip", "walker_eval.hip", "walker_eval_device.h", "walker_eval_body.h")
    for name in names:
        code = _code(_read(CSRC, name))
        assert not reads.search(code) and "fmaf" not in code, name
    src = _read(CSRC, "walker_hardcore_eval.hip")
    code = _code(src)
    assert re.search(r"__global__[^;{]*\bk_walker_hc_eval\(", code) and "ddrl_env_refuse(" in code and "WalkerHardcore" in code
    assert '#include "walker_device.h"' in src and '#include "../../include/ddrl_walker_hardcore_eval.h"' in src
    assert "eval_common_check(" in code and "h->terrain" in code
    # the episode loop and the policy row exist once: both kernels are the one body text, behind their terrain mode
    body = _code(_read(CSRC, "walker_eval_body.h"))
    assert body.count("e.physics(") == 1 and body.count("ddrl_pol::policy_row(") == 1 and "WalkerT<WE_HC" in body
    for name, mode in (("walker_eval.hip", "0"), ("walker_hardcore_eval.hip", "1")):
        text = _read(CSRC, name)
        k = _code(text)
        assert re.search(r"constexpr int WE_HC = %s;\s*#include \"\"" % mode, k), name
        assert text.count('#include "walker_eval_body.h"') == 1 and "physics(" not in k and "policy_row(" not in k, name
    dev = _code(_read(CSRC, "walker_eval_device.h"))
    assert "physics(" not in dev and "eval_reserve(" in dev      # the host half: the results block of eval_host.h
    # the one-lane instantiation packs its fields; every other kernel keeps the stride of 64 by default
    wd = _read(CSRC, "walker_device.h")
    assert "template <int HC, int LS = 64>" in wd and "using WalkerHardcoreLane = WalkerT<1, 1>;" in wd and "using WalkerHardcore = WalkerT<1>;" in wd
    # the landers' files and the walker's step kernels do not see it; the Makefile rebuilds on the new headers
    for name in ("eval.hip", "eval_q.hip", "eval_episodes.h", "eval3.hip", "walker.hip"):
        assert "k_walker_hc_eval" not in _read(CSRC, name) and "walker_eval_body.h" not in _read(CSRC, name), name
    mk = _read(CSRC, "Makefile")
    for dep in ("walker_eval_device.h", "walker_eval_body.h", "../../include/ddrl_walker_hardcore_eval.h"):
        assert dep in mk, dep
    # the compiler's report of the new kernel: no scratch, no spilled VGPRs, static LDS inside 64 KiB
    rep = _read(ROOT, "profiles", "walker_hardcore_eval_resource_usage.txt")
    mine = rep[rep.index("Function Name: _ZN12_GLOBAL__N_116k_walker_hc_evalE"):]
    mine = mine[:mine.index("LDS Size [bytes/block]")+40]
    assert "ScratchSize [bytes/lane]: 0\n" in mine and "VGPRs Spill: 0\n" in mine
    assert 0 < int(re.search(r"LDS Size \[bytes/block\]: (\d+)", mine).group(1)) <= 65536


# ---- the Python doors ----------------------------------------------------------------------------------------------------------------
def _opt(model="walker", terrain="hardcore", **flags):
    class O:
        env, seed, max_ep_len = HARDCORE_ENV, 9, 30
        env_model, env_terrain, env_velocity_iterations, env_position_iterations = model, terrain, 8, 3
    for k, v in flags.items():
        setattr(O, k, v)
    return O()


def test_python_doors_without_a_device():
    """The old doors stay shut on the Hardcore terrain and say where the open one is; the marker and the new flag."""
    from distributed_drl_amd import env as E
    from distributed_drl_amd.workers import _default_test_env
    for door in (lambda: E.make(HARDCORE_ENV, model="walker", terrain="hardcore", on_device=True),
                 lambda: E.make_device(HARDCORE_ENV, model="walker", terrain="hardcore"),
                 lambda: E.DeviceBipedalWalker(terrain="hardcore")):
        with pytest.raises(ValueError, match="evaluation kernel") as info:
            door()
        assert "DeviceBipedalWalkerHardcore" in str(info.value) and NAME in str(info.value) and "missing" not in str(info.value)
    for door in (lambda: E.make("BipedalWalker-v2", model="walker", on_device=True), lambda: E.make_device("BipedalWalker-v2", model="walker")):
        with pytest.raises(ValueError, match="DeviceBipedalWalker") as info:      # the grass name: the grass marker, as before
            door()
        assert "Hardcore" not in str(info.value)
    # the marker: the grass marker's twin
    m = E.DeviceBipedalWalkerHardcore(4, 30, velocity_iterations=8, position_iterations=3)
    assert isinstance(m, E.DeviceBipedalWalker) and (m.model, m.terrain, m.on_device) == ("walker", "hardcore", True)
    assert (m.seed, m.max_ep_len, m.velocity_iterations, m.position_iterations, m.episodes_played) == (4, 30, 8, 3, 0)
    assert m._model_kw() == dict(velocity_iterations=8, position_iterations=3, terrain="hardcore") and m._host_class is E.BipedalWalker
    d = E.DeviceBipedalWalkerHardcore()
    assert (d.seed, d.max_ep_len, d.velocity_iterations, d.position_iterations) == (0, 1600, 180, 60)
    assert m.reset().shape == (24,) and not m.reset().any() and m.action_space.shape == (4,) and m.observation_space.shape == (24,)
    with pytest.raises(RuntimeError, match="not steppable"):
        m.step(np.zeros(4))
    with pytest.raises(TypeError):
        E.DeviceBipedalWalkerHardcore(terrain="grass")      # the terrain is the class
    assert E.DeviceBipedalWalker().terrain == "grass" and E.DeviceBipedalWalker()._model_kw() == dict(velocity_iterations=180, position_iterations=60)
    # the workers' flag: read before test_on_device; the Hardcore walker only
    made = _default_test_env(HARDCORE_ENV, _opt(test_on_device_hardcore=True))
    assert type(made) is E.DeviceBipedalWalkerHardcore
    assert (made.seed, made.max_ep_len, made.velocity_iterations, made.position_iterations) == (9, 30, 8, 3)
    assert type(_default_test_env(HARDCORE_ENV, _opt(test_on_device_hardcore=True, test_on_device=True))) is E.DeviceBipedalWalkerHardcore
    for model, terrain in (("walker", "grass"), ("simple", "grass"), ("articulated", "grass")):
        with pytest.raises(ValueError, match="test_on_device_hardcore"):
            _default_test_env("BipedalWalker-v2", _opt(model, terrain, test_on_device_hardcore=True))
    with pytest.raises(ValueError, match="env_terrain"):      # _env_model_kw's own refusal comes first
        _default_test_env(HARDCORE_ENV, _opt("simple", "hardcore", test_on_device_hardcore=True))
    with pytest.raises(ValueError, match="evaluation kernel") as info:      # the old flag keeps raising, and names the new one
        _default_test_env(HARDCORE_ENV, _opt(test_on_device=True))
    assert "test_on_device_hardcore" in str(info.value)
    assert type(_default_test_env("BipedalWalker-v2", _opt("walker", "grass", test_on_device=True))) is E.DeviceBipedalWalker
    from distributed_drl_amd.agent import HyperParameters
    assert getattr(HyperParameters(obs_dim=24, act_dim=4), "test_on_device_hardcore", False) is False      # the default stays off
