"""ctypes binding of libddrl_hip.so (the C-ABI declared in include/ddrl.h).

The product path has no CPU fallback: if the shared library is missing, or a call fails, this
module raises.  Nothing here imports the oracle."""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint8, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# DDRL_LIB_PATH: another build of the same C-ABI (same-box A/B runs of tools/*: an older library next to the in-tree one, selected
# per process instead of copied over the package file).  Symbols an older build lacks are skipped (their call sites then fail).
LIB_PATH = os.environ.get("DDRL_LIB_PATH") or os.path.join(_HERE, "libddrl_hip.so")

DDRL_OK = 0
DDRL_ERR_BAD_ARG = -1
DDRL_ERR_EMPTY_BUFFER = -2
DDRL_ERR_HIP = -3
DDRL_ERR_NOMEM = -4
DDRL_ERR_UNSUPPORTED = -5
DDRL_ERR_NOT_REPRESENTABLE = -6
DDRL_ERR_RCCL = -7
DDRL_ACT_SAMPLE, DDRL_ACT_DETERMINISTIC = 0, 1   # ddrl_dqn_act / ddrl_rollout_step_discrete: mode
DDRL_REPLAY_ACTS_1D = 1
DDRL_REPLAY_U8_OBS = 2
DDRL_ENV_STATE_FIELDS = 32
DDRL_NSTEP_FUSED_MAX_LN = 16   # include/ddrl.h: the fused n-step rollout step stages a workgroup's windows in LDS
DDRL_ENV3_STATE_FIELDS = 66   # the articulated model's block (ddrl_env_state_fields tells which a handle holds)
DDRL_ENV_ONE_BODY, DDRL_ENV_ARTICULATED = 0, 1   # ddrl_env_model_t.kind
DDRL_ENV_WALKER = 3                              # ... the bipedal walker ([n,24] observations, [n,4] actions); 2 is not a model
DDRL_ENVW_STATE_FIELDS = 286                     # its block: bodies, joint and contact impulses, bookkeeping, 200 terrain heights
DDRL_WALKER_TERRAIN_GRASS, DDRL_WALKER_TERRAIN_HARDCORE = 0, 1   # include/ddrl_walker_hardcore.h: the walker handle's terrain mode
DDRL_ENVWH_STATE_FIELDS = 663                    # a Hardcore walker's block: the 286 rows, wall-slot impulses, box count / table / column index
SAC1_STAGES = 12
DQN_STAGES = 9   # include/ddrl.h: DDRL_DQN_STAGES
SAC1_MAIN, SAC1_TARGET, SAC1_ADAM_M, SAC1_ADAM_V, SAC1_GRAD = range(5)
SAC1, SAC_V = 0, 1  # ddrl_sac1_config_t.variant


class Sac1Config(ctypes.Structure):
    """ddrl_sac1_config_t; defaults = algos/sac1/hyperparams.py + core.py:91 at LunarLander dims."""
    _fields_ = [("obs_dim", c_int32), ("act_dim", c_int32), ("hidden1", c_int32), ("hidden2", c_int32),
                ("batch", c_int32), ("variant", c_int32), ("alpha", c_double), ("gamma", c_double),
                ("lr", c_double), ("polyak", c_double), ("beta1", c_double), ("beta2", c_double),
                ("adam_eps", c_double), ("act_scale", c_double)]

    def __init__(self, obs_dim=8, act_dim=2, hidden1=400, hidden2=300, batch=256, alpha=0.1, gamma=0.997,
                 lr=5e-5, polyak=0.995, beta1=0.9, beta2=0.999, adam_eps=1e-8, act_scale=1.0, variant=0):
        super().__init__(obs_dim, act_dim, hidden1, hidden2, batch, variant, alpha, gamma, lr, polyak, beta1, beta2,
                         adam_eps, act_scale)


class DqnConfig(ctypes.Structure):
    """ddrl_dqn_config_t; defaults = algos/dqn/hyperparams.py."""
    _fields_ = [("obs_dim", c_int32), ("n_actions", c_int32), ("hidden1", c_int32), ("hidden2", c_int32), ("batch", c_int32),
                ("variant", c_int32), ("gamma", c_double), ("lr", c_double), ("polyak", c_double), ("beta1", c_double),
                ("beta2", c_double), ("adam_eps", c_double), ("alpha", c_double)]

    def __init__(self, obs_dim, n_actions, hidden1=400, hidden2=300, batch=128, gamma=0.99, lr=1e-3, polyak=0.995, beta1=0.9,
                 beta2=0.999, adam_eps=1e-8, variant=0, alpha=0.1):
        super().__init__(obs_dim, n_actions, hidden1, hidden2, batch, variant, gamma, lr, polyak, beta1, beta2, adam_eps, alpha)


class EnvModel(ctypes.Structure):
    """ddrl_env_model_t; the iteration counts are Box2D's world.Step arguments as gym calls it (6 * 30, 2 * 30)."""
    _fields_ = [("kind", c_int32), ("velocity_iterations", c_int32), ("position_iterations", c_int32)]

    def __init__(self, kind=DDRL_ENV_ONE_BODY, velocity_iterations=180, position_iterations=60):
        super().__init__(kind, velocity_iterations, position_iterations)


_P = c_void_p  # device pointers and opaque handles cross as void*


class RolloutNStepOut(ctypes.Structure):
    """ddrl_rollout_nstep_out_t: device mirrors of ddrl_rollout_step_nstep, each nullable."""
    _fields_ = [("act", _P), ("obs2", _P), ("rew", _P), ("done", _P), ("next_obs", _P), ("ended", _P)]


# name -> (restype, argtypes).  Must list every symbol include/ddrl.h declares
# (tests/test_workers_cpu.py checks header <-> table <-> library).
SIGNATURES = {
    "ddrl_version": (c_int, []),
    "ddrl_last_error": (c_char_p, []),
    "ddrl_device_arch": (c_int, [c_int, c_char_p, c_int]),
    "ddrl_host_device_pointer": (c_int, [_P, ctypes.POINTER(ctypes.c_void_p)]),
    "ddrl_replay_create": (c_int, [POINTER(_P), c_int, c_int64, c_int, c_int, c_uint32]),
    "ddrl_replay_destroy": (c_int, [_P]),
    "ddrl_replay_seed": (c_int, [_P, c_uint32, _P]),
    "ddrl_replay_store": (c_int, [_P, _P, _P, _P, _P, _P, c_int64, _P]),
    "ddrl_replay_sample": (c_int, [_P, c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "ddrl_replay_gather": (c_int, [_P, _P, c_int64, _P, _P, _P, _P, _P, _P]),
    "ddrl_replay_create_ex": (c_int, [POINTER(_P), c_int, c_int64, c_int32, POINTER(c_int32), c_int64, c_int64]),
    "ddrl_replay_store_ex": (c_int, [_P, POINTER(_P), c_int64, _P]),
    "ddrl_replay_store_masked_ex": (c_int, [_P, POINTER(_P), _P, c_int64, _P]),
    "ddrl_replay_append_ring": (c_int, [_P, _P, _P]),
    "ddrl_replay_sample_ex": (c_int, [_P, c_int64, POINTER(_P), _P, _P]),
    "ddrl_replay_sample_many": (c_int, [_P, c_int64, c_int64, POINTER(_P), _P]),
    "ddrl_replay_set_feed": (c_int, [_P, _P, c_int32, c_int32, c_int32, POINTER(_P), POINTER(c_int32), _P]),
    "ddrl_replay_take_error": (c_int, [_P, _P, _P]),
    "ddrl_replay_gather_ex": (c_int, [_P, _P, c_int64, POINTER(_P), _P]),
    "ddrl_nstep_fold": (c_int, [_P, _P, _P, _P, c_int64, c_int32, c_int32, c_int32, c_float, _P, _P, _P, _P, _P, _P]),
    "ddrl_replay_sample_nstep": (c_int, [_P, c_int64, c_float, _P, _P, _P, _P, _P, _P, _P]),
    "ddrl_replay_sample_many_nstep": (c_int, [_P, c_int64, c_int64, c_float, POINTER(_P), _P]),
    "ddrl_replay_buffers_ex": (c_int, [_P, POINTER(_P), POINTER(c_int32), POINTER(c_int32)]),
    "ddrl_replay_counts": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64), _P]),
    "ddrl_replay_buffers": (c_int, [_P, POINTER(_P), POINTER(_P), POINTER(_P), POINTER(_P), POINTER(_P)]),
    "ddrl_replay_set_counts": (c_int, [_P, c_int64, c_int64, c_int64, c_int64, _P]),
    "ddrl_replay_sample_indices": (c_int, [_P, c_int64, _P, _P]),
    "ddrl_replay_create_typed": (c_int, [POINTER(_P), c_int, c_int64, c_int32, POINTER(c_int32), _P, c_int64, c_int64]),
    "ddrl_replay_rows_export": (c_int, [_P, c_int32, c_int64, c_int64, _P, _P]),
    "ddrl_replay_rows_import": (c_int, [_P, c_int32, c_int64, c_int64, _P, _P]),
    "ddrl_replay_mt_state": (c_int, [_P, _P, POINTER(c_int32), _P]),
    "ddrl_ps_create": (c_int, [POINTER(_P), c_int, c_int64]),
    "ddrl_ps_destroy": (c_int, [_P]),
    "ddrl_ps_push": (c_int, [_P, _P, c_int64, c_int64, _P]),
    "ddrl_ps_pull": (c_int, [_P, _P, c_int64, c_int64, _P]),
    "ddrl_ps_buffer": (c_int, [_P, POINTER(_P), POINTER(c_int64)]),
    "ddrl_ps_version": (c_int64, [_P]),
    "ddrl_sac1_param_counts": (c_int, [POINTER(Sac1Config), POINTER(c_int64), POINTER(c_int64)]),
    "ddrl_sac1_create": (c_int, [POINTER(_P), c_int, POINTER(Sac1Config)]),
    "ddrl_sac1_destroy": (c_int, [_P]),
    "ddrl_sac1_set_weights": (c_int, [_P, _P, _P]),
    "ddrl_sac1_get_weights": (c_int, [_P, _P, _P]),
    "ddrl_sac1_export": (c_int, [_P, c_int, _P, _P]),
    "ddrl_sac1_import": (c_int, [_P, c_int, _P, _P]),
    "ddrl_sac1_grad_buffer": (c_int, [_P, POINTER(_P), POINTER(c_int64)]),
    "ddrl_sac1_grad_finalize": (c_int, [_P, _P]),
    "ddrl_sac1_opt_steps": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), _P]),
    "ddrl_sac1_step": (c_int, [_P] + [_P] * 12 + [_P]),
    "ddrl_sac1_compute_grads": (c_int, [_P] + [_P] * 12 + [_P]),
    "ddrl_sac1_apply_grads": (c_int, [_P, _P]),
    "ddrl_sac1_opt_state_get": (c_int, [_P, POINTER(c_int64), POINTER(c_int64), POINTER(c_uint64), _P]),
    "ddrl_sac1_opt_state_set": (c_int, [_P, c_int64, c_int64, c_uint64, _P]),
    "ddrl_sac1_step_and_sample": (c_int, [_P, c_int, _P, c_int, _P]),
    "ddrl_sac1_compute_grads_and_sample": (c_int, [_P, c_int, _P, c_int, _P]),
    "ddrl_sac1_apply_grads_and_sample": (c_int, [_P, _P, c_int, _P]),
    "ddrl_sac1_step_host": (c_int, [_P, _P, c_int64, c_uint32, c_uint64, _P, _P]),
    "ddrl_sac1_graph_sync": (c_int, [_P, _P]),
    "ddrl_sac1_capture_begin": (c_int, [_P]),
    "ddrl_sac1_capture_abort": (c_int, [_P]),
    "ddrl_sac1_input_buffers": (c_int, [_P, c_int, POINTER(_P)]),
    "ddrl_sac1_is_fused": (c_int, [_P]),
    "ddrl_sac1_host_graphs": (c_int, [_P]),
    "ddrl_sac1_batch": (c_int, [_P]),
    "ddrl_sac1_fill_noise": (c_int, [_P, c_uint32, _P]),
    "ddrl_sac1_stage_time": (c_int, [_P, c_int, c_int, POINTER(c_float), _P]),
    "ddrl_loop_create": (c_int, [POINTER(_P), _P, _P, c_int32, c_uint32]),
    "ddrl_loop_destroy": (c_int, [_P]),
    "ddrl_loop_run": (c_int, [_P, c_int64, _P]),
    "ddrl_actor_create": (c_int, [POINTER(_P), c_int, POINTER(Sac1Config), c_int64]),
    "ddrl_actor_destroy": (c_int, [_P]),
    "ddrl_actor_set_weights": (c_int, [_P, _P, _P]),
    "ddrl_actor_get_weights": (c_int, [_P, _P, _P]),
    "ddrl_actor_act": (c_int, [_P, _P, _P, c_int64, c_int, _P, _P]),
    "ddrl_actor_act_one": (c_int, [_P, _P, c_uint32, c_uint64, c_int, _P, _P]),
    "ddrl_policy_eval": (c_int, [POINTER(Sac1Config), _P, c_int32, c_uint32, c_uint32, c_int32, _P, _P, _P, _P]),
    "ddrl_env_create": (c_int, [POINTER(_P), c_int, c_int64, c_uint32, c_int32]),
    "ddrl_env_create_ex": (c_int, [POINTER(_P), c_int, c_int64, c_uint32, c_int32, POINTER(EnvModel)]),
    "ddrl_env_state_fields": (c_int, [_P]),
    "ddrl_env_destroy": (c_int, [_P]),
    "ddrl_env_reset": (c_int, [_P, _P, _P, _P]),
    "ddrl_env_step": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "ddrl_rollout_begin": (c_int, [_P, _P, _P]),
    "ddrl_rollout_step": (c_int, [_P, _P, _P, c_int32, c_uint32, c_uint64, c_int, _P, _P, _P]),
    "ddrl_rollout_begin_articulated": (c_int, [_P, _P, _P]),
    "ddrl_rollout_step_articulated": (c_int, [_P, _P, _P, c_int32, c_uint32, c_uint64, c_int, _P, _P, _P]),
    "ddrl_env_step_wrapped": (c_int, [_P, _P, c_float, c_float, c_float, c_int32, c_int32, _P, _P, _P, _P, _P, _P]),
    "ddrl_env_step_wrapped_articulated": (c_int, [_P, _P, c_float, c_float, c_float, c_int32, c_int32, _P, _P, _P, _P, _P, _P]),
    "ddrl_env_step_discrete": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "ddrl_rollout_begin_discrete": (c_int, [_P, _P, _P]),
    "ddrl_rollout_step_discrete": (c_int, [_P, _P, _P, c_int32, c_int, c_float, c_uint32, c_uint64, _P, _P, _P, _P]),
    "ddrl_rollout_begin_discrete_articulated": (c_int, [_P, _P, _P]),
    "ddrl_rollout_step_discrete_articulated": (c_int, [_P, _P, _P, c_int32, c_int, c_float, c_uint32, c_uint64, _P]),
    "ddrl_env_rollout_mirrors": (c_int, [_P, POINTER(_P), POINTER(_P), POINTER(_P), POINTER(c_int32), POINTER(c_int32)]),
    "ddrl_env_stats": (c_int, [_P, POINTER(c_int64), POINTER(c_double), POINTER(c_int64), _P]),
    "ddrl_env_get_state": (c_int, [_P, _P, _P]),
    "ddrl_env_set_state": (c_int, [_P, _P, _P]),
    "ddrl_actor_versions_enable": (c_int, [_P, c_int32, _P]),
    "ddrl_actor_versions_state": (c_int, [_P, _P, _P, _P]),
    "ddrl_actor_versions_adopt": (c_int, [_P, _P, c_int64, _P]),
    "ddrl_actor_act_versioned": (c_int, [_P, _P, _P, c_int64, c_int, c_int32, _P, _P]),
    "ddrl_comm_unique_id": (c_int, [_P]),
    "ddrl_comm_init": (c_int, [POINTER(_P), c_int, c_int32, c_int32, _P]),
    "ddrl_comm_destroy": (c_int, [_P]),
    "ddrl_comm_bcast_params": (c_int, [_P, _P, c_int64, c_int32, _P]),
    "ddrl_comm_allreduce_grads": (c_int, [_P, _P, c_int64, _P]),
    "ddrl_comm_send_batch": (c_int, [_P, _P, c_int64, c_int32, _P]),
    "ddrl_comm_recv_batch": (c_int, [_P, _P, c_int64, c_int32, _P]),
    "ddrl_comm_group_start": (c_int, []),
    "ddrl_comm_group_end": (c_int, []),
    "ddrl_dqn_param_count": (c_int, [_P, POINTER(c_int64)]),
    "ddrl_dqn_create": (c_int, [POINTER(_P), c_int, _P]),
    "ddrl_dqn_destroy": (c_int, [_P]),
    "ddrl_dqn_set_weights": (c_int, [_P, _P, _P]),
    "ddrl_dqn_wide_sk": (c_int, [_P]),
    "ddrl_dqn_export": (c_int, [_P, c_int, _P, _P]),
    "ddrl_dqn_import": (c_int, [_P, c_int, _P, _P]),
    "ddrl_dqn_step": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "ddrl_dqn_step_timed": (c_int, [_P, _P, _P, _P, _P, _P, c_int, _P, _P]),
    "ddrl_dqn_step_ring": (c_int, [_P, _P, _P, _P, _P, _P]),
    "ddrl_dqn_loop_create": (c_int, [POINTER(_P), _P, _P, c_int32, _P]),
    "ddrl_dqn_loop_destroy": (c_int, [_P]),
    "ddrl_dqn_loop_run": (c_int, [_P, c_int64, _P]),
    "ddrl_dqn_loop_info": (c_int, [_P, POINTER(c_int32)]),
    "ddrl_dqn_q": (c_int, [_P, _P, c_int64, _P, _P]),
    "ddrl_dqn_act": (c_int, [_P, _P, c_int64, c_int, c_float, c_uint32, c_uint64, _P, _P, _P]),
    "ddrl_dqn_eval": (c_int, [POINTER(DqnConfig), _P, c_int32, c_uint32, c_uint32, c_int32, c_int, c_float, c_uint32, c_uint64, _P, _P, _P, _P]),
    "ddrl_env_eval_policy": (c_int, [_P, _P, c_int32, c_uint32, c_int32, _P]),
    "ddrl_env_eval_q": (c_int, [_P, _P, c_int32, c_uint32, c_int, c_float, c_uint32, c_uint64, c_int32, _P]),
    "ddrl_env_eval_results": (c_int, [_P, POINTER(_P), POINTER(_P), POINTER(_P), POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "ddrl_dqn_versions_enable": (c_int, [_P, c_int32, _P]),
    "ddrl_dqn_versions_state": (c_int, [_P, _P, _P, _P]),
    "ddrl_dqn_versions_adopt": (c_int, [_P, _P, c_int64, _P]),
    "ddrl_winq_create": (c_int, [POINTER(_P), c_int, c_int64, c_int32, c_int32, c_int32, c_int32]),
    "ddrl_winq_destroy": (c_int, [_P]),
    "ddrl_winq_begin": (c_int, [_P, _P, _P, _P]),
    "ddrl_winq_push": (c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "ddrl_winq_buffers": (c_int, [_P, POINTER(_P), POINTER(_P)]),
    "ddrl_rollout_begin_nstep": (c_int, [_P, _P, _P, _P]),
    "ddrl_rollout_step_nstep": (c_int, [_P, _P, _P, _P, c_int32, c_float, c_float, c_float, c_int32, c_int32, c_int32, c_uint32, c_uint64,
                                        _P, _P]),
    "ddrl_rollout_begin_nstep_articulated": (c_int, [_P, _P, _P, _P]),
    "ddrl_rollout_step_nstep_articulated": (c_int, [_P, _P, _P, _P, c_int32, c_float, c_float, c_float, c_int32, c_int32, c_int32, c_uint32,
                                                    c_uint64, _P, _P]),
    "ddrl_normal_fill": (c_int, [_P, c_int64, c_uint32, c_uint64, _P]),
    "ddrl_uniform_fill": (c_int, [_P, c_int64, c_float, c_float, c_uint32, c_uint64, _P]),
}

_lib = None


class DdrlError(RuntimeError):
    pass


class DdrlUnsupported(DdrlError):
    """DDRL_ERR_UNSUPPORTED: the call has no kernel for this shape (callers with another path catch this one)."""


# include/ddrl_walker.h: the entry points declared beside include/ddrl.h (SIGNATURES is that header's set, name for name)
SIGNATURES_WALKER = {
    "ddrl_env_step_wrapped_walker": SIGNATURES["ddrl_env_step_wrapped"],   # the arguments of its one-body twin
}
# include/ddrl_walker_eval.h, likewise
SIGNATURES_WALKER_EVAL = {
    "ddrl_env_eval_policy_walker": SIGNATURES["ddrl_env_eval_policy"],     # the arguments of the landers' entry point
}
# include/ddrl_walker_hardcore.h, likewise
SIGNATURES_WALKER_HARDCORE = {
    "ddrl_env_create_walker": (c_int, [POINTER(_P), c_int, c_int64, c_uint32, c_int32, c_int32, c_int32, c_int32]),
}
# include/ddrl_walker_hardcore_eval.h, likewise
SIGNATURES_WALKER_HARDCORE_EVAL = {
    "ddrl_env_eval_policy_walker_hardcore": SIGNATURES["ddrl_env_eval_policy"],   # the arguments of the landers' entry point
}


def load():
    """Load libddrl_hip.so; raise loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: libddrl_hip.so must bind to the HIP runtime torch has loaded (one runtime per
    # process), otherwise device pointers and streams would belong to a different runtime instance
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise DdrlError(
            "libddrl_hip.so not found at %s — build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C distributed-drl_amd/csrc`; there is no CPU fallback for the product path" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in (list(SIGNATURES.items()) + list(SIGNATURES_WALKER.items()) + list(SIGNATURES_WALKER_EVAL.items())
                              + list(SIGNATURES_WALKER_HARDCORE.items()) + list(SIGNATURES_WALKER_HARDCORE_EVAL.items())):
        try:
            fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        except AttributeError:
            if not os.environ.get("DDRL_LIB_PATH"):
                raise
            continue                 # an OLDER build selected for an A/B run: calls of what it lacks fail at the call site
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    """Map a ddrl_status to the reference's error behaviour (SURVEY §8(b) Errors)."""
    if rc == DDRL_OK:
        return
    msg = load().ddrl_last_error().decode("utf-8", "replace")
    if rc == DDRL_ERR_EMPTY_BUFFER:
        raise ValueError(msg or "high <= 0")  # what np.random.randint(0, 0, n) raises in the reference
    if rc == DDRL_ERR_BAD_ARG or rc == DDRL_ERR_NOT_REPRESENTABLE:
        raise ValueError("ddrl: " + msg)
    if rc == DDRL_ERR_NOMEM:
        raise MemoryError("ddrl: " + msg)
    raise (DdrlUnsupported if rc == DDRL_ERR_UNSUPPORTED else DdrlError)("ddrl error %d: %s" % (rc, msg))


def require_gpu():
    """Fail loudly unless torch sees a gfx950 device and the library is loadable."""
    import torch
    lib = load()
    if not torch.cuda.is_available():
        raise DdrlError("no GPU visible: the MI355X hot path has no CPU fallback")
    buf = ctypes.create_string_buffer(128)
    check(lib.ddrl_device_arch(torch.cuda.current_device(), buf, 128))
    arch = buf.value.decode()
    if not arch.startswith("gfx950"):
        raise DdrlError("libddrl_hip.so is built for gfx950 only; device reports %r" % arch)
    return arch


def stream_ptr():
    import torch
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def aligned(t, nbytes):
    """`t` (contiguous) itself when its first byte lies on the nbytes grid include/ddrl.h's memory contract asks of a pointer, else a
    copy in a fresh allocation (torch's allocator hands out 512-byte aligned blocks).  For INPUTS only: a copy cannot stand in for
    a buffer the library writes — there the library's own refusal (DDRL_ERR_BAD_ARG -> ValueError) is the right answer."""
    return t if t.data_ptr() % nbytes == 0 else t.clone()


def dptr(t):
    """Device pointer of a contiguous float32/int64/uint8 CUDA tensor (or None -> NULL)."""
    if t is None:
        return c_void_p(None)
    assert t.is_cuda and t.is_contiguous(), "expected a contiguous device tensor"
    return c_void_p(t.data_ptr())
