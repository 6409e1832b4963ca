"""CPU: the specification of the walker's HARDCORE terrain (tests/walker_hardcore_oracle.py) held to itself and to the grass oracle —
the restated physics equals the grass walker's bit for bit with the obstacles switched off; the terrain generator's invariants; the
crafted scenarios reach every branch of the census; bounds of the wall slots; the C ABI's new header, ctypes table and contract rows;
the golden file."""
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

import walker_hardcore_oracle as H   # noqa: E402
import walker_oracle as W   # noqa: E402

F = np.float32
LIVE_SEEDS = (1, 7, 3, 11)   # the seeds of tests/test_gpu_walker_hardcore.py's live cases, (n: 64, 33, 1, 130)
LIVE_N = (64, 33, 1, 130)


def test_grass_equivalence_with_the_obstacles_switched_off():
    """16 envs, 8 / 3, max_ep_len 25 so that resets are crossed: outputs and rows 0..285 over 200 random-policy steps."""
    kw = dict(seed=3, max_ep_len=25, velocity_iterations=8, position_iterations=3)
    g, h = W.WalkerOracle(16, **kw), H.WalkerHardcoreOracle(16, obstacles=False, **kw)
    np.testing.assert_array_equal(g.S, h.S[:W.NFW])
    rs = np.random.RandomState(0)
    ended = 0
    for t in range(200):
        a = rs.uniform(-1.3, 1.3, (16, 4)).astype(F)
        wg, wh = g.step(a), h.step(a)
        for x, y in zip(wg, wh):
            np.testing.assert_array_equal(x, y, err_msg="step %d" % t)
        np.testing.assert_array_equal(g.S, h.S[:W.NFW], err_msg="step %d" % t)
        ended += int(wg[4].sum())
    assert ended >= 16 * 7
    assert (h.S[H.NB] == 0).all() and (h.S[H.BC0:H.BC0 + W.NT] == -1).all() and (h.S[H.W0:H.NB] == 0).all()
    assert g.stats() == h.stats()


def _terrains(seed, n, episode):
    ora = H.WalkerHardcoreOracle.__new__(H.WalkerHardcoreOracle)
    ora.obstacles, ora.n, ora.seed, ora.draw_log = True, n, seed, None
    ora.S = np.zeros((H.NFWH, n), F)
    ora.S[W.EPI] = F(episode)
    ora.env_ids = np.arange(n, dtype=np.uint32)
    ora._build()
    return ora


def test_generator_invariants():
    """Over 2000+ (seed, env, episode) triples: box count <= 40, no column holds two boxes, every box inside the terrain's x range
    (LAST_START keeps them there: nothing is clipped), the table behind the count empty, the column index and the table agreeing, the
    start pad flat and free of boxes; all three kinds occur in the terrains of the envs the GPU live test uses."""
    kinds = set()
    triples = 0
    cases = [(s, n, 0) for s, n in zip(LIVE_SEEDS, LIVE_N)] + [(100 + k, 64, k) for k in range(30)]
    for seed, n, ep in cases:
        ora = _terrains(seed, n, ep)
        S = ora.S
        for e in range(n):
            triples += 1
            nb = int(S[H.NB, e])
            assert 0 <= nb <= H.MAXBOX
            B = S[H.B0:H.B0 + 4 * H.MAXBOX, e].reshape(H.MAXBOX, 4)
            assert (B[nb:] == 0).all()
            col = S[H.BC0:H.BC0 + W.NT, e].astype(np.int64)
            cover = np.zeros(W.NT, np.int64)
            for b in range(nb):
                x0, x1, y0, y1 = B[b]
                i0, i1 = int(round(float(x0) / float(W.STEP))), int(round(float(x1) / float(W.STEP)))
                assert x0 == F(i0) * W.STEP and x1 == F(i1) * W.STEP and y0 < y1
                assert H.STARTPAD <= i0 < i1 <= W.NT - 1            # inside [0, 199 STEP], clear of the start pad
                cover[i0:i1] += 1
                assert (col[i0:i1] == b).all()
            assert (cover <= 1).all() and ((col >= 0) == (cover == 1)).all()
            assert (S[W.T0:W.T0 + H.STARTPAD + 1, e] == S[W.T0, e]).all() and (col[:H.STARTPAD] == -1).all()
        if ep == 0:
            for ks in ora.last_kinds:
                kinds.update(ks)
    assert triples >= 2000
    assert kinds == {H.STUMP, H.STAIRS, H.PIT}


def test_box_cap_is_a_guard_not_a_behaviour():
    """The worst case by construction is 37 boxes: the rule "stay on GRASS with fewer than 5 free slots" is never the reason a run
    stays grass in these terrains (the count never reaches 36)."""
    mx = max(int(_terrains(200 + k, 64, k).S[H.NB].max()) for k in range(12))
    assert mx <= 35, mx


def test_no_two_draws_of_an_episode_share_a_hash_input():
    """Terrain, obstacles, force, 30 wrapped steps with observation noise, the reset noise: the hash inputs (step * 16 + j) mod 2^32 of
    all draws of one episode are pairwise distinct, per env."""
    from walker_wrapped_oracle import RESET_NOISE_STREAM
    n = 4
    ora = H.WalkerHardcoreWrappedOracle(n, seed=5, max_ep_len=1 << 20, velocity_iterations=8, position_iterations=3)
    ora.S[W.EPI] = F(1.0)                           # a new episode: everything it draws is logged from here
    ora.draw_log = []
    o = ora.reset()                                # terrain, obstacles, force
    n_build = len(ora.draw_log)
    assert n_build == (W.NT - 21) + 5 * W.NT + 1
    ctl = W.WalkerHeuristic(n)
    cut = np.full(n, -1, np.int64)                 # an env whose episode ends on the way: its draws count up to the step before
    survived = np.zeros(n, np.int64)
    for t in range(30):                            # gym's walking heuristic keeps most walkers up for the 60 physics steps
        before = len(ora.draw_log)
        out = ora.step_wrapped(ctl.act(o), 0.0, 0.05, 5.0, 2, 1 << 20)
        o = out[3]
        cut = np.where((cut < 0) & (out[4] != 0), before, cut)
        survived += cut < 0
    assert len(ora.draw_log) == n_build + 30 * (4 + 24)
    assert (survived >= 10).all() and (survived == 30).any(), survived
    inputs = [((st.astype(np.uint64) * 16 + j) & 0xFFFFFFFF) for st, j in ora.draw_log]
    reset_noise = [(RESET_NOISE_STREAM * 16 + k) & 0xFFFFFFFF for k in range(24)]
    M = np.stack(inputs)                           # [draws, n]
    for e in range(n):
        mine = M[:cut[e] if cut[e] >= 0 else M.shape[0], e].tolist() + reset_noise   # ... and the reset noise's 24
        assert len(set(mine)) == len(mine), e
    assert (H.OBSTACLE_STEP0 * 16) & 0xFFFFFFFF == 0x80000000


def test_crafted_scenarios_reach_every_branch_of_the_census():
    import _walker_hardcore_scenarios as sc
    S, act, outs, final, census, recs = sc.trajectory(*sc.FAST)
    assert S.shape == (H.NFWH, sc.N) and act.shape == (sc.T, sc.N, 4)
    for b in sc.BRANCHES:
        assert census.get(b, 0) > 0, (b, census)
    r0 = recs[0]
    cls = sc.ENV_CLASS
    # what each class was built for, at the first step
    assert (r0["face"][sc.FOOT0_L][cls == "stump_top"] == H.FACE_TOP).all()
    both = cls == "stump_left_and_ground"
    assert (r0["on"][2 * sc.FOOT0_R][both] & r0["on"][2 * sc.FOOT0_R + 1][both]).all() and (r0["face"][sc.FOOT0_R][both] == H.FACE_LEFT).all()
    assert (r0["face"][sc.FOOT0_L][cls == "stump_right_and_ground"] == H.FACE_RIGHT).all()
    assert (r0["face"][sc.FOOT0_L][cls == "pit_left_wall"] == H.FACE_RIGHT).all() and (r0["face"][sc.FOOT0_R][cls == "pit_right_wall"] == H.FACE_LEFT).all()
    assert (r0["tie"][sc.FOOT0_R][cls == "tie_top_left"] == 1).all() and (r0["face"][sc.FOOT0_R][cls == "tie_top_left"] == H.FACE_TOP).all()
    assert (r0["tie"][sc.FOOT0_L][cls == "tie_top_right"] == 2).all() and (r0["face"][sc.FOOT0_L][cls == "tie_top_right"] == H.FACE_TOP).all()
    assert (r0["tie"][sc.FOOT0_L][cls == "tie_left_right"] == 3).all() and (r0["face"][sc.FOOT0_L][cls == "tie_left_right"] == H.FACE_LEFT).all()
    crash = cls == "hull_in_box"
    assert r0["box_over"][crash].all() and (outs[0][1][crash] == -100.0).all() and (outs[0][2][crash] == 1.0).all() and outs[0][4][crash].all()
    assert not r0["box_over"][~crash].any()
    miss = cls == "lidar_all_miss"
    assert (outs[0][0][miss][:, 14:] == 1.0).all()


def test_wall_slot_bounds_on_the_oracle():
    """Per slot and step: the accumulated normal impulse is never negative (along the slot's own normal); the friction bound holds as
    the solver states it — a sweep clamps the tangent impulse to MU x the normal impulse the slot holds at that moment, tangent before
    normal, so the stored tangent impulse is within the bound its last sweep used, exactly (the clamp is a min / max), and that bound is
    MU x a normal impulse >= 0; an inactive slot holds zero; and the position solve's exit guarantee includes the wall slots: a
    solved env's last sweep measured no separation below -3 slop in any slot."""
    import _walker_hardcore_scenarios as sc
    for iters in (sc.FAST, sc.GYM):
        recs = sc.trajectory(*iters)[5]
        seen_wall = 0
        for r in recs:
            an, at, on = r["an"], r["at"], r["on"]
            assert (an >= 0).all()
            assert (np.abs(at)[on] <= r["friction_limit"][on]).all() and (r["friction_limit"] >= 0).all()
            assert (an[~on] == 0).all() and (at[~on] == 0).all()
            wall = on[1::2]
            assert (np.abs(r["nx"][1::2][wall]) == 1).all() and (r["ny"][1::2][wall] == 0).all()
            seen_wall += int(wall.sum())
            solved = r["solved"]
            assert (r["minsep"][solved] >= W.SLOP3).all()
            st = r["state"]
            for q in range(8):
                np.testing.assert_array_equal(st[H.W0 + 2 * q], an[2 * q + 1])
                np.testing.assert_array_equal(st[W.K0 + 2 * q], an[2 * q])
        assert seen_wall > 0


def _hdr(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_the_new_header_its_ctypes_table_and_the_library():
    import ctypes
    from distributed_drl_amd import _lib
    hdr, hh = _hdr("ddrl.h"), _hdr("ddrl_walker_hardcore.h")
    code = re.sub(r"/\*.*?\*/", "", hh, flags=re.S)
    assert set(re.findall(r"\b(ddrl_[a-z0-9_]+)\s*\(", code)) == set(_lib.SIGNATURES_WALKER_HARDCORE) == {"ddrl_env_create_walker"}
    for other in (_lib.SIGNATURES, _lib.SIGNATURES_WALKER, _lib.SIGNATURES_WALKER_EVAL):
        assert not set(_lib.SIGNATURES_WALKER_HARDCORE) & set(other)
    so = os.path.join(ROOT, "distributed-drl_amd", "libddrl_hip.so")
    assert os.path.exists(so), "libddrl_hip.so is not built"
    assert ctypes.CDLL(so).ddrl_env_create_walker is not None and _lib.load().ddrl_env_create_walker.argtypes is not None
    args = [" ".join(p.split()) for p in re.search(r"\bint ddrl_env_create_walker\s*\(([^;]*?)\)\s*;", code, flags=re.S).group(1).split(",")]
    assert args == ["ddrl_env_t **out", "int device", "int64_t n_envs", "uint32_t seed", "int32_t max_ep_len", "int32_t velocity_iterations",
                    "int32_t position_iterations", "int32_t terrain"]
    assert len(_lib.SIGNATURES_WALKER_HARDCORE["ddrl_env_create_walker"][1]) == len(args)
    # each header names the other; the sibling headers keep their single declaration; ddrl.h's set stays closed
    assert '#include "ddrl.h"' in hh and "ddrl_walker_hardcore.h" in hdr
    assert "ddrl_walker.h" in hh and "ddrl_walker_eval.h" in hh
    for sib, table in (("ddrl_walker.h", _lib.SIGNATURES_WALKER), ("ddrl_walker_eval.h", _lib.SIGNATURES_WALKER_EVAL)):
        c = re.sub(r"/\*.*?\*/", "", _hdr(sib), flags=re.S)
        assert set(re.findall(r"\b(ddrl_[a-z0-9_]+)\s*\(", c)) == set(table) and len(table) == 1
    names = set(re.findall(r"\b(ddrl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert names == set(_lib.SIGNATURES) and "ddrl_env_create_walker" not in names
    # constants: header = _lib = oracle = the device header's enum
    defs = dict(re.findall(r"^#define (DDRL_[A-Z_]+) (\d+)", code, flags=re.M))
    assert int(defs["DDRL_WALKER_TERRAIN_GRASS"]) == _lib.DDRL_WALKER_TERRAIN_GRASS == H.TERRAIN_GRASS == 0
    assert int(defs["DDRL_WALKER_TERRAIN_HARDCORE"]) == _lib.DDRL_WALKER_TERRAIN_HARDCORE == H.TERRAIN_HARDCORE == 1
    assert int(defs["DDRL_ENVWH_STATE_FIELDS"]) == _lib.DDRL_ENVWH_STATE_FIELDS == H.NFWH == 663
    assert (H.W0, H.NB, H.B0, H.BC0) == (286, 302, 303, 463)
    dev = open(os.path.join(ROOT, "distributed-drl_amd", "csrc", "walker_device.h")).read()
    assert "WW0 = NFW, WNB = WW0 + 16, WB0 = WNB + 1, WMAXBOX = 40, WBC0 = WB0 + 4 * WMAXBOX, NFWH = WBC0 + WNT" in dev
    # the model table keeps three kinds and three keys; the terrain is no model
    from distributed_drl_amd import env
    assert set(env.MODELS) == {"simple", "articulated", "walker"} and env.MODELS["walker"]["fused"] == {}
    assert len(re.findall(r"^#define DDRL_ENV_[A-Z_]+ \d+\s*$", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M)) >= 3


def test_the_new_header_is_covered_by_its_contract_table():
    """tests/test_abi_table_cpu.py's parse on include/ddrl_walker_hardcore.h against tests/_abi_contract_walker_hardcore.TABLE: no
    declaration with caller device memory or a stream is uncovered (the header's one function takes neither), every row is for a
    declaration of the header, the rows name cases of the module, a new symbol with device memory fails the check; include/ddrl.h and
    its table are as they were with the module imported."""
    import _abi_contract as ac
    import _abi_contract_walker_hardcore as ah
    from test_abi_table_cpu import stream_uncovered, takes_a_stream, takes_device_memory, uncovered
    hdr, hh = _hdr("ddrl.h"), _hdr("ddrl_walker_hardcore.h")
    assert takes_device_memory(hh) == {} and not takes_a_stream(hh)
    assert uncovered(hh, ah.TABLE, {}) == [] and stream_uncovered(hh, ah.TABLE, {}) == []
    declared = set(re.findall(r"\b(ddrl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hh, flags=re.S)))
    assert set(ah.TABLE) == declared == {ah.CREATE}
    grown = hh.replace("#ifdef __cplusplus\n}", "int ddrl_x(float *y_d, void *stream);\n#ifdef __cplusplus\n}")
    assert grown != hh and uncovered(grown, ah.TABLE, {}) == ["ddrl_x"] and stream_uncovered(grown, ah.TABLE, {}) == ["ddrl_x"]
    for f, rows in ah.TABLE.items():
        assert rows and all(cid in ah.CASES and f in ah.CASES[cid][1] for cid in rows), f
    assert sorted(c for rows in ah.TABLE.values() for c in rows) == sorted(ah.CASES) and len(ah.CASES) >= 12
    assert not set(ah.CASES) & set(ac.CASES) and not set(ah.CASES) & set(ac.STREAM_CASES)
    assert {f for f, _ in ah.REFUSALS} == {"ddrl_env_step", "ddrl_env_reset", "ddrl_env_step_wrapped_walker"}
    assert not set(ah.TABLE) & set(ac.TABLE) and not set(ah.TABLE) & set(takes_device_memory(hdr))
    assert uncovered(hdr, ac.TABLE, ac.EXEMPT) == [] and set(ac.TABLE) <= set(takes_device_memory(hdr))
    assert stream_uncovered(hdr, ac.STREAM_TABLE(), ac.STREAM_EXEMPT) == []


def test_python_doors_without_a_device():
    """What the doors refuse before any device call."""
    from distributed_drl_amd import env as E
    from distributed_drl_amd.workers import _env_model_kw

    class O:
        env_model, env_terrain = "walker", "hardcore"
    assert _env_model_kw(O())["terrain"] == "hardcore"
    O.env_terrain = "grass"
    assert "terrain" not in _env_model_kw(O())
    O.env_model, O.env_terrain = "simple", "hardcore"
    with pytest.raises(ValueError, match="env_terrain"):
        _env_model_kw(O())
    with pytest.raises(ValueError):
        E.make("BipedalWalkerHardcore-v2", model="walker")
    with pytest.raises(ValueError, match="do not agree"):
        E.make("BipedalWalker-v2", model="walker", terrain="hardcore")
    with pytest.raises(ValueError, match="evaluation kernel"):
        E.make("BipedalWalkerHardcore-v2", model="walker", terrain="hardcore", on_device=True)
    with pytest.raises(ValueError, match="evaluation kernel"):
        E.make_device("BipedalWalkerHardcore-v2", model="walker", terrain="hardcore")
    with pytest.raises(ValueError, match="evaluation kernel"):
        E.DeviceBipedalWalker(terrain="hardcore")
    assert E.DeviceBipedalWalker(terrain="grass").model == "walker"


def test_golden_file_first_steps_regenerate_bit_for_bit():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_walker_hardcore_golden as gen
    path = os.path.join(HERE, "golden", "walker_hardcore.npz")
    assert os.path.getsize(path) < 1_000_000
    g = np.load(path)
    assert (int(g["n_envs"]), int(g["velocity_iterations"]), int(g["position_iterations"])) == (8, 180, 60)
    assert g["actions"].shape == (40, 8, 4) and g["final_state"].shape == (H.NFWH, 8) == g["start_state"].shape
    assert g["ended"].sum() >= 8                  # every env regenerated its terrain inside the recording
    r = gen.run(steps=10)
    np.testing.assert_array_equal(r["start_state"], g["start_state"])
    for k in gen.KEYS:
        np.testing.assert_array_equal(r[k], g[k][:10], err_msg=k)
