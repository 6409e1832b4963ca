"""The articulated lander's specification (tests/lander3_oracle.py) on the CPU: joint and momentum invariants in free fall, the golden
file regenerates bit for bit, and gym's heuristic controller lands the model.  No GPU; the HIP kernel is pinned to the same oracle
and the same golden file in tests/test_gpu_lander3.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import lander3_oracle as L3   # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "lander3_heuristic.npz")


from _lander3_scenarios import float64_restatement as _float64_restatement   # noqa: E402  (moved there; shared with the scenario tests)


def _momentum(S, mod=L3):
    """Total linear momentum (x, y) of hull + legs, summed in float64 from a state block, with `mod`'s masses."""
    S = S.astype(np.float64)
    mh, ml = 1.0 / float(mod.INV_MH), 1.0 / float(mod.INV_ML)
    px = mh * S[L3.VX] + ml * (S[L3.L0 + 2] + S[L3.L0 + 8])
    py = mh * S[L3.VY] + ml * (S[L3.L0 + 3] + S[L3.L0 + 9])
    return np.stack([px, py])


def _joint_errors(S):
    """-> (anchor distance [2, n], joint angle [2, n]) from a state block, in float64 with exact sin / cos."""
    S = S.astype(np.float64)
    sa, ca = np.sin(S[L3.ANG]), np.cos(S[L3.ANG])
    ax, ay = S[L3.X] + sa * float(L3.LCY), S[L3.Y] - ca * float(L3.LCY)   # hull-local (0, 0) = centre of mass - R (0, LCY)
    err, ang = [], []
    for b in range(2):
        x, y, a = S[L3.L0 + 6 * b], S[L3.L0 + 6 * b + 1], S[L3.L0 + 6 * b + 4]
        lx, ly = float(L3.SIGN[b]) * float(L3.ANCX), float(L3.ANCY)
        bx, by = x + np.cos(a) * lx - np.sin(a) * ly, y + np.sin(a) * lx + np.cos(a) * ly
        err.append(np.hypot(bx - ax, by - ay))
        ang.append(a - S[L3.ANG])
    return np.stack(err), np.stack(ang)


def test_free_fall_keeps_the_joints_closed_and_momentum_changes_by_gravity_only():
    """Zero action, no contact, 20 / 10 iterations (enough position sweeps that the step inside reset closes the legs' 0.45 rad
    start error at Box2D's 8 degrees per sweep).  Bars: Box2D's own tolerances for the joints; for the momentum twice the float32
    run's deviation from the float64 restatement of the same step, the restatement itself being exact to float64 rounding."""
    n, steps, vit, pit = 16, 50, 20, 10
    f32 = L3.Lander3Oracle(n, seed=3, velocity_iterations=vit, position_iterations=pit)
    L64 = _float64_restatement()
    f64 = L64.Lander3Oracle(n, seed=3, velocity_iterations=vit, position_iterations=pit)
    assert f64.S.dtype == np.float64
    # momentum every step adds, y only: GRAV * DT on the total mass, in exact arithmetic on the model's constants (the float32 step
    # rounds that product once: part of its rounding, not of the yardstick)
    g_step = float(L3.GRAV) * float(L3.DT) * (1.0 / float(L3.INV_MH) + 2.0 / float(L3.INV_ML))
    zero = np.zeros((n, 2), np.float32)
    p32_0, p64_0 = _momentum(f32.S), _momentum(f64.S, L64)
    worst = {"anchor": 0.0, "lo": np.inf, "hi": -np.inf, "p32": 0.0, "p64": 0.0, "dev": 0.0}
    for t in range(1, steps + 1):
        w32, w64 = f32.step(zero), f64.step(zero.astype(np.float64))
        assert not w32[4].any() and not w32[0][:, 6:].any(), "a contact or an episode end at step %d: not free fall" % t
        assert not w64[4].any() and not w64[0][:, 6:].any()
        err, ang = _joint_errors(f32.S)
        worst["anchor"] = max(worst["anchor"], float(err.max()))
        worst["lo"] = min(worst["lo"], float((ang[0] - float(L3.LIM_LO[0])).min()), float((ang[1] - float(L3.LIM_LO[1])).min()))
        worst["hi"] = max(worst["hi"], float((ang[0] - float(L3.LIM_UP[0])).max()), float((ang[1] - float(L3.LIM_UP[1])).max()))
        e32 = np.abs(_momentum(f32.S) - p32_0 - np.array([0.0, g_step * t])[:, None])
        e64 = np.abs(_momentum(f64.S, L64) - p64_0 - np.array([0.0, g_step * t])[:, None])
        dev = np.abs((_momentum(f32.S) - p32_0) - (_momentum(f64.S, L64) - p64_0))
        worst["p32"], worst["p64"], worst["dev"] = max(worst["p32"], e32.max()), max(worst["p64"], e64.max()), max(worst["dev"], dev.max())
        # float64 restatement: gravity only, to float64 rounding (|p| < 100, ~10^3 roundings per step, 50 steps: << 1e-9)
        assert e64.max() <= 1e-9, (t, e64.max())
        # float32 run: within twice its own deviation from the restatement (+ the restatement's bar)
        assert (e32 <= 2.0 * dev + 1e-9).all(), (t, e32.max(), dev.max())
    print("free fall:", worst)
    assert worst["anchor"] <= float(L3.SLOP)
    assert worst["lo"] >= -float(L3.ASLOP) and worst["hi"] <= float(L3.ASLOP)
    # the float32 deviation itself is rounding: per step at most (vit * 2 joints * 4 + 8) updates of each momentum component, each
    # within half an ulp of |m v| < 64 (2^-18), over 50 steps — a worst-case sum, two orders above what a random walk gives
    assert worst["dev"] <= steps * (vit * 8 + 8) * 2.0 ** -18


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


def test_golden_file_regenerates_bit_for_bit(golden):
    """The first 20 steps of the oracle at 180 / 60 from the recorded seed equal the file."""
    import gen_lander3_golden as gen
    g = golden
    assert (int(g["seed"]), int(g["n_envs"]), int(g["velocity_iterations"]), int(g["position_iterations"])) == (gen.SEED, 8, 180, 60)
    again = gen.run(steps=20)
    for k in ("actions", "obs2", "rew", "done", "ended"):
        assert again[k].dtype == g[k].dtype, k
        np.testing.assert_array_equal(again[k], g[k][:20], err_msg=k)
    assert g["final_state"].shape == (L3.NF3, 8) and g["final_state"].dtype == np.float32


def test_gyms_heuristic_lands_the_model(golden):
    """gym's controller lands gym's lander: more than half of the first episodes (consecutive env ids, recorded seed — no picking)
    end on the +100 rest reward with both leg flags set.  Observed in the committed file: 8 of 8, mean return 287.1
    (profiles/lander3_heuristic.txt)."""
    import gen_lander3_golden as gen
    g = golden
    assert bool(g["all_first_ended"]) and g["ended"].any(axis=0).all()
    rows = gen.first_episodes(g)
    landed = sum(r[2] for r in rows)
    print("landed %d of %d, mean first-episode return %.3f" % (landed, len(rows), np.mean([r[0] for r in rows])))
    assert landed > len(rows) // 2
    # the recorded per-episode returns and lengths are those of the recorded steps
    for k, e in enumerate(g["episode_env"]):
        ends = np.nonzero(g["ended"][:, e])[0]
        j = int(np.sum(g["episode_env"][:k] == e))
        t1, t0 = int(ends[j]), (int(ends[j - 1]) + 1 if j else 0)
        assert int(g["episode_length"][k]) == t1 - t0 + 1
        acc = np.float32(0.0)
        for r in g["rew"][t0:t1 + 1, e]:
            acc = np.float32(acc + r)
        assert acc == g["episode_return"][k]


def test_env_model_symbols_in_header_and_table():
    """The two new entry points and the model struct: declared in include/ddrl.h and present in the ctypes table with the header's
    constants (the library side of the three-way check is tests/test_workers_cpu.py's)."""
    import re
    from distributed_drl_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "ddrl.h")).read()
    for name in ("ddrl_env_create_ex", "ddrl_env_state_fields"):
        assert re.search(r"\bint %s\s*\(" % name, hdr) and name in _lib.SIGNATURES
    for name in ("DDRL_ENV_ONE_BODY", "DDRL_ENV_ARTICULATED", "DDRL_ENV3_STATE_FIELDS", "DDRL_ENV_STATE_FIELDS"):
        m = re.search(r"#define %s (\d+)" % name, hdr)
        assert m and int(m.group(1)) == getattr(_lib, name), name
    assert _lib.DDRL_ENV3_STATE_FIELDS == L3.NF3
    assert [f[0] for f in _lib.EnvModel._fields_] == ["kind", "velocity_iterations", "position_iterations"]
    m = _lib.EnvModel()
    assert (m.kind, m.velocity_iterations, m.position_iterations) == (0, 180, 60)
