// What the handle-fed evaluation entry points share on the HOST: the results block of the env handle (env_handle.h) and the argument
// check in front of every look at the agent.  Included by eval3.hip (ddrl_env_eval_policy / ddrl_env_eval_q: the landers) and
// walker_eval.hip / walker_hardcore_eval.hip (ddrl_env_eval_policy_walker / _walker_hardcore, through walker_eval_device.h).  Host code only: nothing here is part of a kernel, so neither file's device code
// depends on it.  Internal linkage throughout.
#pragma once
#include "ddrl_common.h"
#include "env_handle.h"

namespace {

size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// The results block for n episodes with a trace row of `row` floats (0: none), the weight staging for `w_floats`.  Grows by
// free + allocate (never shrinks): such a call synchronises the device and cannot be captured.
int eval_reserve(ddrl_env *h, const char *what, int n, int row, size_t w_floats) {
    const size_t len_off = up256((size_t)n * sizeof(double));
    const size_t trace_off = len_off + up256((size_t)n * sizeof(int));
    const size_t bytes = trace_off + (size_t)n * (size_t)h->max_ep_len * (size_t)row * sizeof(float);
    h->ev_n = 0;   // from here on the previous results are gone: ddrl_env_eval_results refuses until this call has launched
    if (bytes > h->ev_bytes) {
        unsigned char *p = nullptr;
        if (hipMalloc((void **)&p, bytes) != hipSuccess) {
            ddrl::set_error("%s: hipMalloc of the results block failed (%zu bytes)", what, bytes);
            return DDRL_ERR_NOMEM;
        }
        (void)hipFree(h->ev_block);
        h->ev_block = p; h->ev_bytes = bytes;
    }
    if (w_floats > h->ev_w_floats) {
        float *p = nullptr;
        if (hipMalloc((void **)&p, w_floats * sizeof(float)) != hipSuccess) {
            ddrl::set_error("%s: hipMalloc of the weight staging vector failed (%zu floats)", what, w_floats);
            return DDRL_ERR_NOMEM;
        }
        (void)hipFree(h->ev_w);
        h->ev_w = p; h->ev_w_floats = w_floats;
    }
    h->ev_len_off = len_off; h->ev_trace_off = trace_off;
    return DDRL_OK;
}

// What every entry point refuses before it looks at the agent.  kind_guard: the entry point's own call of ddrl_env_refuse
// (env_handle.h) — which kinds its kernels hold is the entry point's to say — run behind the NULL test, in front of the counts.
template <class Guard>
int eval_common_check(const char *what, ddrl_env *h, const void *agent, int32_t n_episodes, uint32_t first_episode, Guard kind_guard) {
    if (h == nullptr || agent == nullptr) {
        ddrl::set_error("%s: bad argument: NULL handle", what);
        return DDRL_ERR_BAD_ARG;
    }
    if (const int rc = kind_guard()) return rc;
    if (n_episodes < 1) {
        ddrl::set_error("%s: bad argument: n_episodes must be >= 1 (got %d)", what, (int)n_episodes);
        return DDRL_ERR_BAD_ARG;
    }
    if ((uint64_t)first_episode + (uint64_t)n_episodes > (1u << 24)) {
        ddrl::set_error("%s: bad argument: first_episode + n_episodes must stay exact in float32 (<= 2^24)", what);
        return DDRL_ERR_BAD_ARG;
    }
    return DDRL_OK;
}

}  // namespace

// What the handle-fed entry points ask of the actor handle: the configuration and the device (actor.hip)
int ddrl_actor_internal_config(ddrl_actor_t *h, ddrl_sac1_config_t *cfg_out, int *device_out);
