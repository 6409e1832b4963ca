// Evaluation episodes of the BIPEDAL WALKER on the HARDCORE terrain on the device, fed from handles:
// ddrl_env_eval_policy_walker_hardcore (include/ddrl_walker_hardcore_eval.h), read back by ddrl_env_eval_results (eval3.hip).
// k_walker_hc_eval is k_walker_eval's twin (walker_eval.hip): one workgroup of 256 threads per episode, nothing crosses workgroups; the
// policy row on all threads in Actor.get_action's summation order, then ONE lane running the Hardcore walker — WalkerT<1, 1>
// (WalkerHardcoreLane, walker_device.h: WalkerHardcore's text, the solver unchanged) with n = 1 — as k_walker_reset<1> /
// k_walker_step<1> run it (walker.hip): build() per episode with id = 0, epi = first_episode + blockIdx.x, the reset's
// zero-action trip through the one inlined physics(), the block-uniform ended flag as the loop's only exit.  The body is the text of
// walker_eval_body.h with WE_HC = 1 (see walker_eval_device.h): the episode loop and the policy row exist once, for both terrains.
// LDS: Sc / T / B / Cc point into a state-block column of NFWH = 663 floats (2652 bytes: the terrain, the box count, the box table and
// the per-column box index the generator writes).  The one lane's 172 sweep fields are packed at lane stride 1 (688 bytes, inside the
// bytes of the layer-2 slice sums): at the step kernels' stride of 64 they would be 43 KiB for one lane and the kernel about 67 KiB.
// The compiler's report — no scratch, no spilled VGPRs, the LDS bytes — is profiles/walker_hardcore_eval_resource_usage.txt.
// Compiled with -ffp-contract=off.  A translation unit of its own: no other file's kernels depend on it.
#include "ddrl_common.h"
#include "../../include/ddrl_walker_hardcore_eval.h"
#include "../../include/ddrl_walker_hardcore.h"
#include "policy_row.h"
#include "walker_device.h"
#include "env_handle.h"
#include "eval_host.h"
#include "walker_eval_device.h"

namespace {

static_assert(NFWH == DDRL_ENVWH_STATE_FIELDS, "the LDS column is a Hardcore state-block column");
static_assert(sizeof(WalkerHardcoreLane) == sizeof(WalkerHardcore), "the lane stride changes no member");

__global__ void __launch_bounds__(256) k_walker_hc_eval(WalkerEvalArgs a) {
    constexpr int WE_HC = 1;
#include "walker_eval_body.h"
}

}  // namespace

extern "C" {

int ddrl_env_eval_policy_walker_hardcore(ddrl_env_t *h, ddrl_actor_t *actor, int32_t n_episodes, uint32_t first_episode,
                                         int32_t want_trace, void *stream) {
    const char *what = "ddrl_env_eval_policy_walker_hardcore";
    if (const int rc = eval_common_check(what, h, actor, n_episodes, first_episode, [&]() -> int {
            if (const int rc = ddrl_env_refuse(h, 1u << DDRL_ENV_WALKER, what, "ddrl_env_eval_policy")) return rc;   // a lander handle: the landers' entry point
            if (h->terrain != DDRL_WALKER_TERRAIN_HARDCORE) {   // k_walker_hc_eval builds the Hardcore terrain; grass has its own entry point
                ddrl::set_error("%s: this entry point holds the hardcore terrain; a handle of the grass terrain (ddrl_env_create_ex, "
                                "kind = DDRL_ENV_WALKER) is taken by ddrl_env_eval_policy_walker (include/ddrl_walker_eval.h)", what);
                return DDRL_ERR_UNSUPPORTED;
            }
            return DDRL_OK;
        })) return rc;
    ddrl::DeviceGuard g(h->device);
    WalkerEvalArgs a;
    if (const int rc = walker_eval_prepare(what, h, actor, n_episodes, first_episode, want_trace, stream, a)) return rc;
    k_walker_hc_eval<<<(unsigned)n_episodes, 256, 0, ddrl::as_stream(stream)>>>(a);
    DDRL_LAUNCH_CHECK();
    h->ev_n = n_episodes; h->ev_row = want_trace ? WE_ROW : 0;
    return DDRL_OK;
}

}  // extern "C"
