"""Cases of the direct-operand tail of the Double-DQN / soft-Q learner (ddrl_dqn_create_direct_tail, opt.direct_learner = "tail"), shared by
tests/test_dqn_direct_tail_cpu.py (the oracles' side of the bars) and tests/test_gpu_dqn_direct_tail.py (the HIP learner held to them)."""
from _state_parity import HYPER_Q, HYPER_R, Case

MIN_OBS = 14      # include/ddrl_dqn_direct.h: DDRL_DQN_DIRECT_MAX_OBS_DIM + 1

_W = dict(obs=1024, act=4, hid=(64, 48), batch=64)                       # layer 1 on wide_l1.h (obs >= 1024, obs % 4 == 0)
CASES = [
    # layer 1 on k_gemm
    Case("tx-first-obs", "ddqn", MIN_OBS, 4, (64, 48), 64, **HYPER_Q),                  # the first width of the envelope
    Case("tx-ragged", "ddqn", 29, 3, (52, 36), 37, data_seed=310, **HYPER_R),           # ragged tiles everywhere (seed 300: an arg-max gap under the CPU test's)
    Case("tx-one-row", "ddqn", 40, 8, (512, 512), 1, **HYPER_Q),                        # most actions, widest hidden, one row
    Case("tx-b512", "ddqn", 16, 2, (300, 300), 512, **HYPER_R),                         # the last batch the wgrad tile holds
    Case("tx-sqn-five-done1", "sqn", 21, 5, (40, 28), 50, alpha=0.2, edge="done1", **HYPER_Q),
    # layer 1 on wide_l1.h
    Case("tx-wide-ddqn-oneaction", "ddqn", edge="oneaction", **_W, **HYPER_R),
    Case("tx-wide-sqn", "sqn", alpha=0.1, **_W, **HYPER_Q),
    Case("tx-wide-ragged", "ddqn", 1028, 3, (400, 300), 37, **HYPER_Q),
]
