"""Cases of the direct-operand Double-DQN / soft-Q learner (ddrl_dqn_create_direct), shared by tests/test_dqn_direct_cpu.py (the
oracles' side of the bars) and tests/test_gpu_dqn_direct.py (the HIP learner held to them)."""
from _state_parity import HYPER_Q, HYPER_R, Case

MAX_OBS = 13      # include/ddrl_dqn_direct.h: DDRL_DQN_DIRECT_MAX_OBS_DIM

_RD = dict(family="ddqn", obs=11, act=3, hid=(52, 36), batch=37)      # the ragged shapes
_RS = dict(family="sqn", obs=6, act=5, hid=(40, 28), batch=50)
CASES = [
    Case("dx-lander", "ddqn", 8, 4, (400, 300), 128, data_seed=310, **HYPER_Q),         # the workload's own shape (seed 300: an arg-max gap under the CPU test's)
    Case("dx-ragged", **_RD, **HYPER_R),                                                # odd width, three actions, ragged batch
    Case("dx-last-obs", "ddqn", MAX_OBS, 8, (512, 512), 1, **HYPER_Q),                  # last width, most actions, widest hidden, one row
    Case("dx-b512", "ddqn", 1, 2, (300, 300), 512, **HYPER_R),                          # the last batch the wgrad tile holds
    Case("dx-five-actions", alpha=0.2, **_RS, **HYPER_Q),
    Case("dx-sqn-aligned", "sqn", 8, 4, (128, 64), 32, alpha=0.05, **HYPER_R),
    Case("dx-ddqn-rew100", edge="rew100", **_RD, **HYPER_Q),
    Case("dx-sqn-done1", alpha=0.2, edge="done1", **_RS, **HYPER_R),
    Case("dx-ddqn-oneaction", edge="oneaction", **_RD, **HYPER_Q),
    Case("dx-sqn-oneaction", alpha=0.1, edge="oneaction", **_RS, **HYPER_R),
]
