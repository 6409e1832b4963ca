// The env handle behind ddrl_env_* as the translation units that reach into it see it: env.hip (create / destroy, the model table, the
// step and the fused rollout entry points), eval3.hip and walker_eval.hip (the evaluation episodes, which borrow the handle's model and own
// its results block; what the two share on the host: eval_host.h).
// Host side only: never a kernel argument.
#pragma once
#include "ddrl_common.h"
#include "env_device.h"

struct ddrl_env {
    int device;
    long long n;
    uint32_t seed;
    int max_ep_len;
    float *S;
    EnvStats *stats;
    int kind, vit, pit;   // ddrl_env_model_t; the iteration counts are the articulated model's and the walker's
    int terrain;          // DDRL_WALKER_TERRAIN_* (ddrl_walker_hardcore.h): the walker's terrain mode, read where ddrl_env_create_walker
                          // chooses the handle's launches and where the walker's two evaluation entry points each refuse the other's terrain; 0 on a lander
    const struct EnvModel *model;   // the kind's row of env.hip's model table (widths, state fields, launches), set at create
    // ---- evaluation episodes (ddrl_env_eval_policy / ddrl_env_eval_q / ddrl_env_eval_results, eval3.hip; ddrl_env_eval_policy_walker,
    // walker_eval.hip).  Everything below is
    // allocated at the first evaluation, grows when a call needs more, and is freed by ddrl_env_destroy; S and stats above are
    // neither read nor written by an evaluation.
    unsigned char *ev_block;   // ret float64 [n] | len int32 [n] | trace float32 [n][max_ep_len][row], each part 256-byte aligned
    size_t ev_bytes;           // its capacity
    float *ev_w;               // the agent's weights in the flat external order, as the launch reads them
    size_t ev_w_floats;        // its capacity
    size_t ev_len_off, ev_trace_off;   // the last call's layout ...
    int ev_n, ev_row;                  // ... its episode count and trace row (0: no trace); ev_n == 0: no evaluation yet
    // ---- mirrors of the articulated discrete fused rollout step (ddrl_rollout_begin_discrete_articulated / _step_discrete_articulated /
    // ddrl_env_rollout_mirrors, env.hip; written by k_env3_step_q, rollout3_q.hip).  One allocation of n * (8 + DDRL_ROLLOUT_MIRROR_Q + 1)
    // floats made by the first begin call that passes its envelope, never resized, freed by ddrl_env_destroy:
    // next observations [n][8] (16-byte aligned: the block's start) | Q rows [n][ro_actions], n * DDRL_ROLLOUT_MIRROR_Q floats set
    // aside | action indices [n].  S and stats above are never reallocated.
    float *ro_block;           // nullptr: no begin call yet
    int ro_actions;            // n_actions of the handle the last begin / step call took: the row width of the Q mirror
};
// Which kinds an entry point takes, as the mask of 1u << DDRL_ENV_*, and the one guard behind every entry point that does not take
// them all (env.hip, beside the model table): DDRL_OK for a handle of a taken kind, else DDRL_ERR_UNSUPPORTED with `what` — the entry
// point's name — the two models and what to use instead in ddrl_last_error(), before anything is touched.  `family`: the one-body
// entry point of the same family (the handle's own model's is named from it); nullptr where only the walker is refused.
// A walker handle ([n,24] observations, [n,4] actions) is taken by reset / step / step_wrapped_walker / eval_policy_walker / eval_results /
// stats / get_state / set_state only.  Where both landers share ONE entry point of a family (ddrl_env_eval_policy), the guard names it
// without the held model's suffix.
constexpr unsigned DDRL_TAKES_LANDERS = 1u << DDRL_ENV_ONE_BODY | 1u << DDRL_ENV_ARTICULATED;
int ddrl_env_refuse(const ddrl_env *h, unsigned takes, const char *what, const char *family);
constexpr int DDRL_ROLLOUT_MIRROR_Q = 8;   // ddrl_sel::MAXQ: the widest Q row the fused discrete step takes
