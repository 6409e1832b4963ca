// Evaluation episodes of the BIPEDAL WALKER on the device, fed from handles: ddrl_env_eval_policy_walker (include/ddrl_walker_eval.h),
// read back by ddrl_env_eval_results (eval3.hip).  One workgroup of 256 threads per episode, nothing crosses workgroups, as
// k_eval_episodes (eval_episodes.h) on the landers.  The kernel's body — the policy row on all threads in Actor.get_action's summation
// order, then ONE lane running Walker (walker_device.h, unchanged), one inlined physics(), the block-uniform exit — is the text of
// walker_eval_body.h with WE_HC = 0, the one text it shares with the Hardcore terrain's kernel (walker_hardcore_eval.hip:
// ddrl_env_eval_policy_walker_hardcore).  What there is to say of the loop, of the walker's pointers (n = 1, `col` in LDS) and of the
// LDS bytes the sweep fields [W_LDS_FIELDS][64] (27 KiB) share with the layer-2 slice sums stands in walker_eval_device.h.  No scratch,
// no spilled VGPRs, 55520 bytes of static LDS (profiles/walker_eval_resource_usage.txt).
// This entry point holds the GRASS terrain; a Hardcore handle is refused here and taken by the entry point of walker_hardcore_eval.hip.
// Compiled with -ffp-contract=off.  A translation unit of its own: no other file's kernels depend on it.
#include "ddrl_common.h"
#include "../../include/ddrl_walker_eval.h"
#include "../../include/ddrl_walker_hardcore.h"
#include "policy_row.h"
#include "walker_device.h"
#include "env_handle.h"
#include "eval_host.h"
#include "walker_eval_device.h"

namespace {

__global__ void __launch_bounds__(256) k_walker_eval(WalkerEvalArgs a) {
    constexpr int WE_HC = 0;
#include "walker_eval_body.h"
}

}  // namespace

extern "C" {

int ddrl_env_eval_policy_walker(ddrl_env_t *h, ddrl_actor_t *actor, int32_t n_episodes, uint32_t first_episode, int32_t want_trace,
                                void *stream) {
    const char *what = "ddrl_env_eval_policy_walker";
    if (const int rc = eval_common_check(what, h, actor, n_episodes, first_episode, [&]() -> int {
            if (const int rc = ddrl_env_refuse(h, 1u << DDRL_ENV_WALKER, what, "ddrl_env_eval_policy")) return rc;   // a lander handle: the landers' entry point
            if (h->terrain != DDRL_WALKER_TERRAIN_GRASS) {   // k_walker_eval builds the grass terrain; the Hardcore terrain's kernel has its own entry point
                ddrl::set_error("%s: this entry point holds the grass terrain; a handle of the hardcore terrain (ddrl_env_create_walker, "
                                "DDRL_WALKER_TERRAIN_HARDCORE) is taken by the evaluation kernel of that terrain — use "
                                "ddrl_env_eval_policy_walker_hardcore (include/ddrl_walker_hardcore_eval.h)", what);
                return DDRL_ERR_UNSUPPORTED;
            }
            return DDRL_OK;
        })) return rc;
    ddrl::DeviceGuard g(h->device);
    WalkerEvalArgs a;
    if (const int rc = walker_eval_prepare(what, h, actor, n_episodes, first_episode, want_trace, stream, a)) return rc;
    k_walker_eval<<<(unsigned)n_episodes, 256, 0, ddrl::as_stream(stream)>>>(a);
    DDRL_LAUNCH_CHECK();
    h->ev_n = n_episodes; h->ev_row = want_trace ? WE_ROW : 0;
    return DDRL_OK;
}

}  // extern "C"
