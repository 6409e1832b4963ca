// The C ABI of the env family: every ddrl_env_* and ddrl_rollout_* entry point that takes an env handle (the evaluation episodes:
// eval3.hip, walker_eval.hip), the fused-step drivers and their envelopes, behind ONE model table — a row per DDRL_ENV_* kind with the model's widths
// and its launch functions.  Host code only: every kernel lives in its model's own translation unit (lander.hip; env3.hip,
// rollout3*.hip; walker.hip; rollout_nstep.hip) and is reached through env_launch.h, so an edit here cannot change what a kernel
// compiles to.
#include "ddrl_common.h"
#include "../../include/ddrl_walker.h"
#include "../../include/ddrl_walker_hardcore.h"
#include "policy_row.h"
#include "replay_device.h"
#include "env_handle.h"
#include "dqn_select.h"
#include "version_plan.h"
#include "rollout_nstep.h"
#include "rollout_args.h"
#include "env_launch.h"

// struct ddrl_env: env_handle.h (shared with eval3.hip and walker_eval.hip, whose evaluation entry points own the handle's results block)

// ---- the model table -----------------------------------------------------------------------------------------------------------
// One row per kind.  A launch pointer is null where the model has no such kernel (the walker's fused family).
typedef int (*EnvelopeFn)(const char *what, ddrl_env_t *h, const ddrl_actor_rollout_view &v, const ddrl_replay_dev::SamplerView *rv,
                          int32_t n_steps);
struct EnvModel {
    int kind;                 // DDRL_ENV_*
    int fields;               // rows of the state block: DDRL_ENV_STATE_FIELDS, DDRL_ENV3_STATE_FIELDS or DDRL_ENVW_STATE_FIELDS
    int obs_dim, act_dim;     // widths of an observation and of a continuous action row
    int act_align;            // bytes: a continuous action row moves as one vector (float2 on the landers, float4 on the walker)
    bool iterates;            // its solver takes the handle's velocity / position iteration counts (each >= 1)
    const char *flag, *noun;  // as the refusal texts name the model
    const char *suffix;       // of the model's own entry points: ddrl_env_step_wrapped<suffix>, ddrl_rollout_begin<suffix>, ...
    int (*reset)(float *S, long long n, uint32_t seed, int vit, int pit, const uint8_t *mask_d, float *obs_d, void *stream);
    // discrete = 1: act_d holds gym's action indices (the landers; ddrl_env_step_discrete takes no walker handle)
    int (*step)(int discrete, float *S, long long n, uint32_t seed, int max_ep_len, int vit, int pit, const float *act_d, float *obs2_d,
                float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stats_d, void *stream);
    int (*step_wrapped)(float *S, long long n, uint32_t seed, int limit_steps, int vit, int pit, float *act_d, float act_noise,
                        float obs_noise, float reward_scale, int repeat, float *obs2_d, float *rew_d, float *done_d, float *next_obs_d,
                        uint8_t *ended_d, void *stats_d, void *stream);
    // the fused rollout family: the begin calls' observation launch, the three env-step launches (`args`: env_launch.h) ...
    int (*obs)(float *S, long long n, uint32_t seed, float *obs_d, void *stream);
    int (*step_pi)(const void *args, int vit, int pit, void *stream);
    int (*step_q)(const void *args, int versioned, int vit, int pit, void *stream);
    int (*step_nstep)(const NStepLaunch &a, int vit, int pit, void *stream);
    // ... and the continuous pair's envelope (below: the two models answer in different statuses and words on purpose)
    EnvelopeFn pi_check;
};
static int rollout_check(const char *, ddrl_env_t *, const ddrl_actor_rollout_view &, const ddrl_replay_dev::SamplerView *, int32_t);
static int rollout3_check(const char *, ddrl_env_t *, const ddrl_actor_rollout_view &, const ddrl_replay_dev::SamplerView *, int32_t);
static const EnvModel ENV_MODELS[] = {
    {DDRL_ENV_ONE_BODY, DDRL_ENV_STATE_FIELDS, 8, 2, 8, false, "DDRL_ENV_ONE_BODY", "the one-body model", "",
     ddrl_lander_launch_reset, ddrl_lander_launch_step, ddrl_lander_launch_step_wrapped,
     ddrl_lander_launch_obs, ddrl_lander_launch_step_pi, ddrl_lander_launch_step_q,
     [](const NStepLaunch &a, int, int, void *stream) { return ddrl_nstep_launch_step(a, stream); }, rollout_check},
    {DDRL_ENV_ARTICULATED, DDRL_ENV3_STATE_FIELDS, 8, 2, 8, true, "DDRL_ENV_ARTICULATED", "the articulated lander", "_articulated",
     ddrl_env3_launch_reset, ddrl_env3_launch_step, ddrl_env3_launch_step_wrapped,
     [](float *S, long long n, uint32_t, float *obs_d, void *stream) { return ddrl_rollout3_launch_obs(S, n, obs_d, stream); },
     ddrl_rollout3_launch_step, ddrl_rollout3_launch_step_q, ddrl_nstep3_launch_step, rollout3_check},
    {DDRL_ENV_WALKER, DDRL_ENVW_STATE_FIELDS, 24, 4, 16, true, "DDRL_ENV_WALKER", "the walker", "_walker",
     [](auto... a) { return ddrl_walker_launch_reset(0, a...); },
     [](int, auto... a) { return ddrl_walker_launch_step(0, a...); },
     [](auto... a) { return ddrl_walker_launch_step_wrapped(0, a...); }, nullptr, nullptr, nullptr, nullptr, nullptr},
};
// The walker on the HARDCORE terrain (ddrl_walker_hardcore.h) is no kind and no row of the table: a terrain mode of the walker kind.
// Its state block's rows and its launches' terrain argument stand here, the walker row otherwise; ddrl_env_create_walker
// hands a handle this object by the handle's `terrain`, so every entry point above and below serves it through h->model unchanged.
static const EnvModel ENV_WALKER_HARDCORE = {
    DDRL_ENV_WALKER, DDRL_ENVWH_STATE_FIELDS, 24, 4, 16, true, "DDRL_ENV_WALKER", "the walker", "_walker",
    [](auto... a) { return ddrl_walker_launch_reset(1, a...); },
    [](int, auto... a) { return ddrl_walker_launch_step(1, a...); },
    [](auto... a) { return ddrl_walker_launch_step_wrapped(1, a...); }, nullptr, nullptr, nullptr, nullptr, nullptr};
// the table lookup: the row of `kind`, nullptr where no model has it
static const EnvModel *env_model_of(int kind) {
    for (const EnvModel &m : ENV_MODELS)
        if (m.kind == kind) return &m;
    return nullptr;
}

// The one guard of the family (env_handle.h).  Three texts, as the entry points have always answered:
// a walker handle at a lander's entry point; a lander handle at an entry point of the one-body model; a handle at an entry point
// built for another model than the one-body one, which names the handle's own entry point of the same family (`family` + the held
// model's suffix — or `family` as it is where both landers share that one function).
int ddrl_env_refuse(const ddrl_env *h, unsigned takes, const char *what, const char *family) {
    const EnvModel &held = *h->model;
    if (takes >> h->kind & 1u) return DDRL_OK;
    if (h->kind == DDRL_ENV_WALKER) {
        ::ddrl::set_error("%s: not built for %s (%s: %d observations, %d actions); its kernels hold a lander — "
                          "use ddrl_actor_act + ddrl_env_step + ddrl_replay_store", what, held.noun, held.flag, held.obs_dim, held.act_dim);
        return DDRL_ERR_UNSUPPORTED;
    }
    const EnvModel *built = nullptr;   // an entry point that refuses a lander is built for exactly one model
    for (const EnvModel &m : ENV_MODELS)
        if (takes == 1u << m.kind) built = &m;
    if (built->kind == DDRL_ENV_ONE_BODY)
        ::ddrl::set_error("%s: not built for %s (%s); its kernel holds %s — "
                          "use ddrl_env_step / ddrl_env_step_discrete with the unfused act and store calls", what, held.noun, held.flag, built->noun);
    else {
        // a family whose lander entry point is ONE function for both landers (eval3.hip) is named as it is, without the model's suffix
        static const char *const both_landers[] = {"ddrl_env_eval_policy"};
        const char *suffix = held.suffix;
        for (const char *f : both_landers)
            if (strcmp(family, f) == 0) suffix = "";
        ::ddrl::set_error("%s: built for %s (%s); this handle holds %s — use %s%s", what, built->noun, built->flag, held.noun, family, suffix);
    }
    return DDRL_ERR_UNSUPPORTED;
}

// Memory contract (include/ddrl.h): the env family's kernels move an observation row as float4s and a continuous action row as one
// vector — float2 on the landers, float4 on the walker — so caller pointers to observations must be 16-byte aligned and to actions
// 8-byte (landers) or 16-byte (walker) aligned.  Checked here, before any launch: a pointer off that grid is refused with its name in
// ddrl_last_error() and nothing is touched.  (NULL passes: optional.)
#define DDRL_REQUIRE_ALIGNED(p, bytes) \
    DDRL_REQUIRE((reinterpret_cast<uintptr_t>(p) & (uintptr_t)((bytes) - 1)) == 0, #p " must be " #bytes "-byte aligned")
#define DDRL_REQUIRE_ACT_ALIGNED(p, model)                                                           \
    DDRL_REQUIRE((reinterpret_cast<uintptr_t>(p) & (uintptr_t)((model)->act_align - 1)) == 0,        \
                 (model)->act_align == 16 ? #p " must be 16-byte aligned" : #p " must be 8-byte aligned")

// ---- what the fused rollout entry points below share on the host.  (The kernels are kept apart on purpose.)
// "A five-array float32 transition ring (obs1[8], obs2[8], acts[w], rews, done)": what a ring is not, for the caller to report in its own
// status and words.
enum RingFault { RING_FITS = 0, RING_ROW_SHAPE, RING_COMPACT };
static RingFault transition_ring_fault(const ddrl_replay_dev::RingPtrs &r, int w) {
    if (r.n_arr != 5 || r.w[0] != 8 || r.w[1] != 8 || r.w[2] != w || r.w[3] != 1 || r.w[4] != 1) return RING_ROW_SHAPE;
    return (r.kind[0] || r.kind[1]) ? RING_COMPACT : RING_FITS;
}
static const char *const RING_COMPACT_MSG = "the fused rollout step stores into float32 rings only (not a compact uint8 ring)";

// the observations of the envs' present state into the forward's rows (the begin calls)
static int launch_env_obs(ddrl_env_t *h, float *obs, void *stream) {
    ddrl::DeviceGuard g(h->device);
    return h->model->obs(h->S, h->n, h->seed, obs, stream);
}

// The version store's side of ONE vector step of every fused loop, around `step(versioned, fused_plan)` — the entry point's own forward,
// argument patch and launch.  versioned: the store's own answer (ddrl_actor_internal_step_begin with the horizon max_ep_len, or the
// wrapped step's limit_steps).  fused_plan: the next forward's plan rides in this launch (base offsets of the row lists must fit the
// records' int); behind the launch the store is told whether that tail has planned for the envs the launch's episode ends moved to
// the newest version, or the next forward has to.
template <class Step>
static int rollout_versioned_step(const ddrl_version_view &ver, long long n, long long horizon, Step step) {
    const bool versioned = ver.n_slots > 0 && ddrl_actor_internal_step_begin(ver.owner, horizon) != 0;
    const bool fused_plan = versioned && ver.vcnt != nullptr && ver.perm2d_off + (long long)ver.n_slots * n < (1ll << 31) && n / 32 <= 1024;
    if (const int rc = step(versioned, fused_plan)) return rc;
    if (versioned) ddrl_actor_internal_step_end(ver.owner, fused_plan ? 1 : 0);
    return DDRL_OK;
}
// ... and the plan's tables as the launch takes them: k_env_step_q as they stand, the other argument structs field by field
static VerPlan ver_plan_of(const ddrl_version_view &ver, bool fused_plan, int col_tiles) {
    return VerPlan{fused_plan ? ver.vcnt : nullptr, ver.perm, ver.perm2d_off, ver.vtiles, ver.vs, ver.n_slots, col_tiles, ver.wg_slots, ver.vt_cap};
}
template <class Args>
static void set_ver_plan(Args &a, const VerPlan &p) {
    a.vcnt = p.vcnt; a.perm = p.perm; a.perm2d_off = p.perm2d_off; a.vtiles = p.vtiles; a.vs = p.vs;
    a.n_slots = p.n_slots; a.col_tiles = p.col_tiles; a.wg_slots = p.wg_slots; a.vt_cap = p.vt_cap;
}

// The continuous pair's envelopes (EnvModel::pi_check; rv: the step's ring, nullptr in the begin call, which has no n_steps either).
// The one-body pair's: DDRL_ERR_BAD_ARG
static int rollout_check(const char *, ddrl_env_t *h, const ddrl_actor_rollout_view &v, const ddrl_replay_dev::SamplerView *rv, int32_t n_steps) {
    DDRL_REQUIRE(v.ok, "actor has no direct-operand policy (shape outside the envelope): use ddrl_actor_act + ddrl_env_step + ddrl_replay_store");
    if (!rv) {
        DDRL_REQUIRE(v.obs_dim == 8 && h->n <= v.max_rows && v.device == h->device, "actor / env mismatch (obs_dim 8, max_rows >= n_envs, same device)");
        return DDRL_OK;
    }
    DDRL_REQUIRE(v.obs_dim == 8 && v.act <= 2 && h->n <= v.max_rows && h->n % 32 == 0 && v.device == h->device,
                 "actor / env mismatch (obs_dim 8, act_dim <= 2, n_envs a multiple of 32 within max_rows, same device)");
    const RingFault rf = transition_ring_fault(rv->ring, 2);
    DDRL_REQUIRE(rf != RING_ROW_SHAPE, "replay row shape must be (obs1[8], obs2[8], acts[2], rews, done)");
    DDRL_REQUIRE(rf != RING_COMPACT, RING_COMPACT_MSG);
    DDRL_REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    DDRL_REQUIRE(v.ver.n_slots == 0 || h->n == v.max_rows, "an actor with a version store steps exactly max_rows envs");
    return DDRL_OK;
}
// the articulated pair's: DDRL_ERR_UNSUPPORTED with the function's name (n_steps behind it, as a bad argument)
static int rollout3_check(const char *what, ddrl_env_t *h, const ddrl_actor_rollout_view &v, const ddrl_replay_dev::SamplerView *rv,
                          int32_t n_steps) {
    const char *why = nullptr;
    if (!v.ok) why = "the actor has no direct-operand policy (shape outside the envelope)";
    else if (v.obs_dim != 8 || v.act > 2) why = "the actor must have obs_dim 8 and act_dim <= 2";
    else if (h->n % 32 != 0 || h->n > v.max_rows) why = "n_envs must be a multiple of 32 within the actor's max_rows";
    else if (v.ver.n_slots > 0 && h->n != v.max_rows) why = "an actor with a version store steps exactly max_rows envs";
    else if (v.device != h->device) why = "actor and envs must live on one device";
    else if (rv) {
        const RingFault rf = transition_ring_fault(rv->ring, 2);
        if (rf == RING_ROW_SHAPE) why = "the replay row shape must be (obs1[8], obs2[8], acts[2], rews, done)";
        else if (rf == RING_COMPACT) why = RING_COMPACT_MSG;
        else if (rv->device != h->device) why = "the replay ring lives on another device than the envs";
    }
    if (why) {
        ddrl::set_error("%s: %s; use ddrl_actor_act + ddrl_env_step + ddrl_replay_store", what, why);
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(!rv || n_steps >= 1, "n_steps must be >= 1");
    return DDRL_OK;
}

// The continuous fused step behind ddrl_rollout_step (lander.hip: k_env_step_pi) and ddrl_rollout_step_articulated (rollout3.hip:
// k_env3_step_pi), behind the entry point's own envelope: n_steps times the loop body of worker_rollout — the forward, the env-step
// kernel of the handle's model on the filled RolloutArgs, the host's bookkeeping.
static int rollout_step_loop(ddrl_env_t *h, ddrl_actor_t *actor, const ddrl_actor_rollout_view &v, ddrl_replay_t *replay,
                             const ddrl_replay_dev::SamplerView &rv, int32_t n_steps, uint32_t noise_seed, uint64_t noise_ctr,
                             int deterministic, float *act_out_d, float *next_obs_out_d, void *stream) {
    ddrl::DeviceGuard g(h->device);
    RolloutArgs a{};
    a.S = h->S; a.n = h->n; a.seed = h->seed; a.max_ep_len = (float)h->max_ep_len; a.stats = h->stats;
    a.obs = v.obs; a.hp = v.hp; a.act = v.act; a.nt2 = v.nt2; a.scale = v.scale;
    a.deterministic = deterministic; a.noise_seed = noise_seed; a.vstride = v.ver.vstride;
    a.rs = rv.state; a.ring = rv.ring; a.act_out = act_out_d; a.next_obs_out = next_obs_out_d;
    for (int k = 0; k < n_steps; ++k) {  // the loop body of worker_rollout, n_steps times with the weights the actor holds
        const int rc = rollout_versioned_step(v.ver, h->n, h->max_ep_len, [&](bool versioned, bool fused_plan) -> int {
            a.slot = versioned ? v.ver.slot : nullptr;
            a.newest = versioned ? &v.ver.vs->newest : nullptr;
            a.bmu = versioned ? v.vbmu : v.bmu; a.bls = versioned ? v.vbls : v.bls;
            set_ver_plan(a, ver_plan_of(v.ver, fused_plan, v.nt2));
            if (const int frc = ddrl_actor_internal_forward(actor, h->n, stream, versioned ? 1 : 0)) return frc;
            a.noise_ctr = noise_ctr + (uint64_t)k * (uint64_t)h->n * (uint64_t)v.act;
            return h->model->step_pi(&a, h->vit, h->pit, stream);
        });
        if (rc != DDRL_OK) return rc;
        ddrl_replay_note_store(replay, h->n);
    }
    return DDRL_OK;
}

// The discrete fused step behind ddrl_rollout_step_discrete (lander.hip: k_env_step_q) and ddrl_rollout_step_discrete_articulated
// (rollout3_q.hip: k_env3_step_q), behind the entry point's own envelope: n_steps times the loop body of worker_rollout_dqn — the
// pending repack, the forward, the env-step kernel of the handle's model on the filled RolloutQArgs, the host's bookkeeping.
static int rollout_discrete_step_loop(ddrl_env_t *h, ddrl_dqn_t *dqn, const ddrl_dqn_rollout_view &v, ddrl_replay_t *replay,
                                      const ddrl_replay_dev::SamplerView &rv, int32_t n_steps, int mode, float greedy_prob, uint32_t seed,
                                      uint64_t ctr, float *act_out_d, float *q_out_d, float *next_obs_out_d, void *stream) {
    ddrl::DeviceGuard g(h->device);
    RolloutQArgs a{};
    a.S = h->S; a.n = h->n; a.seed = h->seed; a.max_ep_len = (float)h->max_ep_len; a.stats = h->stats;
    a.obs = v.obs; a.hp = v.hp; a.b_lo = v.b_lo; a.b_hi = v.b_hi; a.A = v.n_actions; a.half = v.half; a.nt2 = v.nt2; a.sqn = v.sqn;
    a.deterministic = mode == DDRL_ACT_DETERMINISTIC; a.greedy_prob = greedy_prob; a.alpha = v.alpha; a.noise_seed = seed;
    a.rs = rv.state; a.ring = rv.ring; a.act_out = act_out_d; a.q_out = q_out_d; a.next_obs_out = next_obs_out_d;
    for (int k = 0; k < n_steps; ++k) {   // ddrl_rollout_step's loop body
        // a learner step's pending repack is an install: before the store is asked whether this step is versioned
        if (const int rc = ddrl_dqn_internal_repack(dqn, stream)) return rc;
        const int rc = rollout_versioned_step(v.ver, h->n, h->max_ep_len, [&](bool versioned, bool fused_plan) -> int {
            if (const int frc = ddrl_dqn_internal_forward(dqn, h->n, stream, versioned ? 1 : 0)) return frc;
            a.noise_ctr = ctr + (uint64_t)k * 2ull * (uint64_t)h->n;
            if (versioned) {
                a.b_lo = v.vb_lo; a.b_hi = v.vb_hi; a.slot = v.ver.slot; a.newest = &v.ver.vs->newest; a.vstride = v.ver.vstride;
                a.vp = ver_plan_of(v.ver, fused_plan, v.nt2);
            } else {
                a.b_lo = v.b_lo; a.b_hi = v.b_hi;
            }
            return h->model->step_q(&a, versioned ? 1 : 0, h->vit, h->pit, stream);
        });
        if (rc != DDRL_OK) return rc;
        ddrl_replay_note_store(replay, h->n);
    }
    return DDRL_OK;
}

// ---- one body behind each family's exports: `kind` is the model the entry point `what` is built for, and the only one it takes ----
// ddrl_env_step_wrapped / _articulated / _walker (no_pointer, no_count: the entry point's own words for its two argument refusals)
static int env_step_wrapped(int kind, const char *what, const char *no_pointer, const char *no_count, ddrl_env_t *h, float *act_d,
                            float act_noise, float obs_noise, float reward_scale, int32_t action_repeat, int32_t limit_steps, float *obs2_d,
                            float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && act_d != nullptr, no_pointer);
    if (const int rc = ddrl_env_refuse(h, 1u << kind, what, "ddrl_env_step_wrapped")) return rc;
    DDRL_REQUIRE_ACT_ALIGNED(act_d, h->model);
    DDRL_REQUIRE_ALIGNED(obs2_d, 16);
    DDRL_REQUIRE_ALIGNED(next_obs_d, 16);
    DDRL_REQUIRE(action_repeat >= 1 && limit_steps >= 1, no_count);
    ddrl::DeviceGuard g(h->device);
    return h->model->step_wrapped(h->S, h->n, h->seed, limit_steps, h->vit, h->pit, act_d, act_noise, obs_noise, reward_scale,
                                  action_repeat, obs2_d, rew_d, done_d, next_obs_d, ended_d, h->stats, stream);
}
// ddrl_rollout_begin / _articulated
static int rollout_begin(int kind, const char *what, ddrl_env_t *h, ddrl_actor_t *actor, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr, "NULL handle");
    if (const int rc = ddrl_env_refuse(h, 1u << kind, what, "ddrl_rollout_begin")) return rc;
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    if (const int rc = h->model->pi_check(what, h, v, nullptr, 0)) return rc;
    return launch_env_obs(h, v.obs, stream);
}
// ddrl_rollout_step / _articulated
static int rollout_step(int kind, const char *what, ddrl_env_t *h, ddrl_actor_t *actor, ddrl_replay_t *replay, int32_t n_steps,
                        uint32_t noise_seed, uint64_t noise_ctr, int deterministic, float *act_out_d, float *next_obs_out_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr && replay != nullptr, "NULL handle");
    if (const int rc = ddrl_env_refuse(h, 1u << kind, what, "ddrl_rollout_step")) return rc;
    DDRL_REQUIRE_ALIGNED(act_out_d, 8);
    DDRL_REQUIRE_ALIGNED(next_obs_out_d, 16);
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    if (const int rc = h->model->pi_check(what, h, v, &rv, n_steps)) return rc;
    return rollout_step_loop(h, actor, v, replay, rv, n_steps, noise_seed, noise_ctr, deterministic, act_out_d, next_obs_out_d, stream);
}

extern "C" {

int ddrl_env_create(ddrl_env_t **out, int device, int64_t n_envs, uint32_t seed, int32_t max_ep_len) {
    return ddrl_env_create_ex(out, device, n_envs, seed, max_ep_len, nullptr);
}

// ddrl_env_create_ex and ddrl_env_create_walker: `terrain` is the handle's terrain mode, which picks the walker's launches
static int env_create(ddrl_env_t **out, int device, int64_t n_envs, uint32_t seed, int32_t max_ep_len, const ddrl_env_model_t *model,
                      int terrain) {
    DDRL_REQUIRE(out != nullptr && n_envs > 0 && max_ep_len > 0, "bad out/n_envs/max_ep_len");
    DDRL_REQUIRE(max_ep_len < (1 << 24), "max_ep_len must stay exact in float32");
    const EnvModel *m = env_model_of(model ? model->kind : DDRL_ENV_ONE_BODY);
    DDRL_REQUIRE(m != nullptr, "model kind must be DDRL_ENV_ONE_BODY, DDRL_ENV_ARTICULATED or DDRL_ENV_WALKER");
    DDRL_REQUIRE(!m->iterates || (model->velocity_iterations >= 1 && model->position_iterations >= 1),
                 "the articulated model and the walker need velocity_iterations >= 1 and position_iterations >= 1");
    if (terrain == DDRL_WALKER_TERRAIN_HARDCORE) m = &ENV_WALKER_HARDCORE;
    ddrl::DeviceGuard g(device);
    if (!g.ok) { ddrl::set_error("cannot select device %d", device); return DDRL_ERR_HIP; }
    ddrl_env *h = new ddrl_env();
    h->device = device; h->n = n_envs; h->seed = seed; h->max_ep_len = max_ep_len; h->S = nullptr; h->stats = nullptr;
    h->kind = m->kind; h->model = m; h->terrain = terrain;
    h->vit = m->iterates ? model->velocity_iterations : 0;
    h->pit = m->iterates ? model->position_iterations : 0;
    if (hipMalloc((void **)&h->S, (size_t)m->fields * n_envs * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&h->stats, sizeof(EnvStats)) != hipSuccess) {
        ddrl::set_error("hipMalloc failed for %lld envs", (long long)n_envs);
        ddrl_env_destroy(h);
        return DDRL_ERR_NOMEM;
    }
    DDRL_HIP_CHECK(hipMemset(h->S, 0, (size_t)m->fields * n_envs * sizeof(float)));
    DDRL_HIP_CHECK(hipMemset(h->stats, 0, sizeof(EnvStats)));
    if (const int rc = m->reset(h->S, h->n, h->seed, h->vit, h->pit, nullptr, nullptr, nullptr)) return rc;
    DDRL_HIP_CHECK(hipStreamSynchronize(nullptr));
    *out = h;
    return DDRL_OK;
}

int ddrl_env_create_ex(ddrl_env_t **out, int device, int64_t n_envs, uint32_t seed, int32_t max_ep_len, const ddrl_env_model_t *model) {
    return env_create(out, device, n_envs, seed, max_ep_len, model, DDRL_WALKER_TERRAIN_GRASS);
}

// ddrl_walker_hardcore.h: a walker handle with a terrain mode (GRASS: ddrl_env_create_ex's walker handle itself)
int ddrl_env_create_walker(ddrl_env_t **out, int device, int64_t n_envs, uint32_t seed, int32_t max_ep_len, int32_t velocity_iterations,
                           int32_t position_iterations, int32_t terrain) {
    DDRL_REQUIRE(terrain == DDRL_WALKER_TERRAIN_GRASS || terrain == DDRL_WALKER_TERRAIN_HARDCORE,
                 "ddrl_env_create_walker: terrain must be DDRL_WALKER_TERRAIN_GRASS or DDRL_WALKER_TERRAIN_HARDCORE");
    const ddrl_env_model_t model = {DDRL_ENV_WALKER, velocity_iterations, position_iterations};
    return env_create(out, device, n_envs, seed, max_ep_len, &model, terrain);
}

int ddrl_env_destroy(ddrl_env_t *h) {
    if (!h) return DDRL_OK;
    ddrl::DeviceGuard g(h->device);
    (void)hipFree(h->S); (void)hipFree(h->stats);
    (void)hipFree(h->ev_block); (void)hipFree(h->ev_w);   // the evaluation results block and weight staging (eval3.hip)
    (void)hipFree(h->ro_block);                           // the articulated discrete rollout step's mirrors
    delete h;
    return DDRL_OK;
}

int ddrl_env_reset(ddrl_env_t *h, const uint8_t *mask_d, float *obs_d, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    DDRL_REQUIRE_ALIGNED(obs_d, 16);
    ddrl::DeviceGuard g(h->device);
    return h->model->reset(h->S, h->n, h->seed, h->vit, h->pit, mask_d, obs_d, stream);
}

int ddrl_env_step(ddrl_env_t *h, const float *act_d, float *obs2_d, float *rew_d, float *done_d, float *next_obs_d,
                  uint8_t *ended_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && act_d != nullptr, "NULL handle or action pointer");
    DDRL_REQUIRE_ALIGNED(act_d, 8);
    DDRL_REQUIRE_ALIGNED(obs2_d, 16);
    DDRL_REQUIRE_ALIGNED(next_obs_d, 16);
    ddrl::DeviceGuard g(h->device);
    DDRL_REQUIRE_ACT_ALIGNED(act_d, h->model);   // the walker's [n,4] action row moves as one float4
    return h->model->step(0, h->S, h->n, h->seed, h->max_ep_len, h->vit, h->pit, act_d, obs2_d, rew_d, done_d, next_obs_d, ended_d,
                          h->stats, stream);
}

int ddrl_env_step_discrete(ddrl_env_t *h, const float *act_idx_d, float *obs2_d, float *rew_d, float *done_d, float *next_obs_d,
                           uint8_t *ended_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && act_idx_d != nullptr, "NULL handle or action pointer");
    if (const int rc = ddrl_env_refuse(h, DDRL_TAKES_LANDERS, "ddrl_env_step_discrete", nullptr)) return rc;
    DDRL_REQUIRE_ALIGNED(obs2_d, 16);
    DDRL_REQUIRE_ALIGNED(next_obs_d, 16);
    ddrl::DeviceGuard g(h->device);
    return h->model->step(1, h->S, h->n, h->seed, h->max_ep_len, h->vit, h->pit, act_idx_d, obs2_d, rew_d, done_d, next_obs_d, ended_d,
                          h->stats, stream);
}

int ddrl_env_step_wrapped(ddrl_env_t *h, float *act_d, float act_noise, float obs_noise, float reward_scale, int32_t action_repeat,
                          int32_t limit_steps, float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d,
                          void *stream) {
    return env_step_wrapped(DDRL_ENV_ONE_BODY, "ddrl_env_step_wrapped", "NULL pointer", "action_repeat and limit_steps must be >= 1", h,
                            act_d, act_noise, obs_noise, reward_scale, action_repeat, limit_steps, obs2_d, rew_d, done_d, next_obs_d, ended_d, stream);
}
// ... on the articulated lander (kernel: rollout3_nstep.hip, k_env3_step_wrapped); the iteration counts are the handle's
int ddrl_env_step_wrapped_articulated(ddrl_env_t *h, float *act_d, float act_noise, float obs_noise, float reward_scale,
                                      int32_t action_repeat, int32_t limit_steps, float *obs2_d, float *rew_d, float *done_d,
                                      float *next_obs_d, uint8_t *ended_d, void *stream) {
    return env_step_wrapped(DDRL_ENV_ARTICULATED, "ddrl_env_step_wrapped_articulated", "NULL pointer", "action_repeat and limit_steps must be >= 1", h,
                            act_d, act_noise, obs_noise, reward_scale, action_repeat, limit_steps, obs2_d, rew_d, done_d, next_obs_d, ended_d, stream);
}
// ... on the walker (kernel: walker.hip, k_walker_step_wrapped): [n,4] actions as one float4, [n,24] observations as six
int ddrl_env_step_wrapped_walker(ddrl_env_t *h, float *act_d, float act_noise, float obs_noise, float reward_scale, int32_t action_repeat,
                                 int32_t limit_steps, float *obs2_d, float *rew_d, float *done_d, float *next_obs_d, uint8_t *ended_d,
                                 void *stream) {
    return env_step_wrapped(DDRL_ENV_WALKER, "ddrl_env_step_wrapped_walker", "ddrl_env_step_wrapped_walker: NULL handle or act_d",
                            "ddrl_env_step_wrapped_walker: action_repeat and limit_steps must be >= 1", h,
                            act_d, act_noise, obs_noise, reward_scale, action_repeat, limit_steps, obs2_d, rew_d, done_d, next_obs_d, ended_d, stream);
}

int ddrl_rollout_begin(ddrl_env_t *h, ddrl_actor_t *actor, void *stream) {
    return rollout_begin(DDRL_ENV_ONE_BODY, "ddrl_rollout_begin", h, actor, stream);
}
int ddrl_rollout_step(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_replay_t *replay, int32_t n_steps, uint32_t noise_seed, uint64_t noise_ctr,
                      int deterministic, float *act_out_d, float *next_obs_out_d, void *stream) {
    return rollout_step(DDRL_ENV_ONE_BODY, "ddrl_rollout_step", h, actor, replay, n_steps, noise_seed, noise_ctr, deterministic, act_out_d,
                        next_obs_out_d, stream);
}
// ---- the same pair on the articulated lander (kernels: rollout3.hip)
int ddrl_rollout_begin_articulated(ddrl_env_t *h, ddrl_actor_t *actor, void *stream) {
    return rollout_begin(DDRL_ENV_ARTICULATED, "ddrl_rollout_begin_articulated", h, actor, stream);
}
int ddrl_rollout_step_articulated(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_replay_t *replay, int32_t n_steps, uint32_t noise_seed,
                                  uint64_t noise_ctr, int deterministic, float *act_out_d, float *next_obs_out_d, void *stream) {
    return rollout_step(DDRL_ENV_ARTICULATED, "ddrl_rollout_step_articulated", h, actor, replay, n_steps, noise_seed, noise_ctr, deterministic,
                        act_out_d, next_obs_out_d, stream);
}

// the discrete fused step's envelope: 0, or the status with the reason in ddrl_last_error()
static int rollout_discrete_check(ddrl_env_t *h, const ddrl_dqn_rollout_view &v) {
    if (!v.ok) {
        ddrl::set_error("fused discrete rollout step: %s; use ddrl_dqn_act + ddrl_env_step_discrete + ddrl_replay_store", v.why ? v.why : "no acting forward");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (v.obs_dim != 8 || v.n_actions > ddrl_sel::MAXQ || h->n % 32 != 0 || h->n > v.batch) {
        ddrl::set_error("fused discrete rollout step needs obs_dim 8, n_actions <= 8 and n_envs a multiple of 32 within the handle's batch "
                        "(obs_dim %d, n_actions %d, n_envs %lld, batch %d); use ddrl_dqn_act + ddrl_env_step_discrete + ddrl_replay_store",
                        v.obs_dim, v.n_actions, h->n, v.batch);
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(v.device == h->device, "the learner / actor handle lives on another device than the envs");
    return DDRL_OK;
}

int ddrl_rollout_begin_discrete(ddrl_env_t *h, ddrl_dqn_t *dqn, void *stream) {
    DDRL_REQUIRE(h != nullptr && dqn != nullptr, "NULL handle");
    if (const int rc = ddrl_env_refuse(h, 1u << DDRL_ENV_ONE_BODY, "ddrl_rollout_begin_discrete", nullptr)) return rc;
    const ddrl_dqn_rollout_view v = ddrl_dqn_internal_view(dqn);
    if (const int rc = rollout_discrete_check(h, v)) return rc;
    return launch_env_obs(h, v.obs, stream);
}

int ddrl_rollout_step_discrete(ddrl_env_t *h, ddrl_dqn_t *dqn, ddrl_replay_t *replay, int32_t n_steps, int mode, float greedy_prob,
                               uint32_t seed, uint64_t ctr, float *act_out_d, float *q_out_d, float *next_obs_out_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && dqn != nullptr && replay != nullptr, "NULL handle");
    if (const int rc = ddrl_env_refuse(h, 1u << DDRL_ENV_ONE_BODY, "ddrl_rollout_step_discrete", nullptr)) return rc;
    DDRL_REQUIRE_ALIGNED(next_obs_out_d, 16);
    DDRL_REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    DDRL_REQUIRE(mode == DDRL_ACT_SAMPLE || mode == DDRL_ACT_DETERMINISTIC, "mode must be DDRL_ACT_SAMPLE or DDRL_ACT_DETERMINISTIC");
    const ddrl_dqn_rollout_view v = ddrl_dqn_internal_view(dqn);
    if (const int rc = rollout_discrete_check(h, v)) return rc;
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    DDRL_REQUIRE(rv.device == h->device, "the replay ring lives on another device than the envs");
    const RingFault rf = transition_ring_fault(rv.ring, 1);
    DDRL_REQUIRE(rf != RING_ROW_SHAPE, "replay row shape must be (obs1[8], obs2[8], acts, rews, done)");
    DDRL_REQUIRE(rf != RING_COMPACT, RING_COMPACT_MSG);
    if (v.ver.n_slots > 0 && h->n != v.rows) {
        ddrl::set_error("fused discrete rollout step: a handle with a version store steps exactly the acting forward's %lld rows (n_envs %lld)", v.rows, h->n);
        return DDRL_ERR_BAD_ARG;
    }
    return rollout_discrete_step_loop(h, dqn, v, replay, rv, n_steps, mode, greedy_prob, seed, ctr, act_out_d, q_out_d, next_obs_out_d, stream);
}

// ---- the same pair on the articulated lander (kernel: rollout3_q.hip).  Handles only: the step's mirrors are a block the env handle
// owns (env_handle.h), allocated by the first begin call that passes the envelope and handed out by ddrl_env_rollout_mirrors.
// The envelope (rv: the step's ring): DDRL_ERR_UNSUPPORTED with the function's name
static int rollout3_discrete_check(const char *what, ddrl_env_t *h, const ddrl_dqn_rollout_view &v, const ddrl_replay_dev::SamplerView *rv) {
    const char *why = nullptr;
    if (!v.ok) why = v.why ? v.why : "no acting forward";
    else if (v.obs_dim != 8 || v.n_actions > ddrl_sel::MAXQ) why = "the handle must have obs_dim 8 and n_actions <= 8";
    else if (h->n % 32 != 0 || h->n > v.batch) why = "n_envs must be a multiple of 32 within the handle's batch";
    else if (v.ver.n_slots > 0 && h->n != v.rows) why = "a handle with a version store steps exactly the acting forward's rows";
    else if (v.device != h->device) why = "the learner / actor handle lives on another device than the envs";
    else if (rv) {
        const RingFault rf = transition_ring_fault(rv->ring, 1);
        if (rf == RING_ROW_SHAPE) why = "the replay row shape must be (obs1[8], obs2[8], acts, rews, done)";
        else if (rf == RING_COMPACT) why = RING_COMPACT_MSG;
        else if (rv->device != h->device) why = "the replay ring lives on another device than the envs";
    }
    if (!why) return DDRL_OK;
    ddrl::set_error("%s: %s; use ddrl_dqn_act + ddrl_env_step_discrete + ddrl_replay_store", what, why);
    return DDRL_ERR_UNSUPPORTED;
}

int ddrl_rollout_begin_discrete_articulated(ddrl_env_t *h, ddrl_dqn_t *dqn, void *stream) {
    DDRL_REQUIRE(h != nullptr && dqn != nullptr, "NULL handle");
    if (const int rc = ddrl_env_refuse(h, 1u << DDRL_ENV_ARTICULATED, "ddrl_rollout_begin_discrete_articulated", "ddrl_rollout_begin_discrete")) return rc;
    const ddrl_dqn_rollout_view v = ddrl_dqn_internal_view(dqn);
    if (const int rc = rollout3_discrete_check("ddrl_rollout_begin_discrete_articulated", h, v, nullptr)) return rc;
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    const size_t n = (size_t)h->n;
    if (!h->ro_block) {   // the first begin call inside the envelope: the mirror block, zeroed
        float *p = nullptr;
        if (hipMalloc((void **)&p, n * (8 + DDRL_ROLLOUT_MIRROR_Q + 1) * sizeof(float)) != hipSuccess) {
            ddrl::set_error("ddrl_rollout_begin_discrete_articulated: hipMalloc failed for the mirrors of %lld envs", h->n);
            return DDRL_ERR_NOMEM;
        }
        DDRL_HIP_CHECK(hipMemsetAsync(p, 0, n * (8 + DDRL_ROLLOUT_MIRROR_Q + 1) * sizeof(float), s));
        h->ro_block = p;
    }
    h->ro_actions = v.n_actions;
    // the envs' current observations into the forward's rows and into the next-observation mirror: what the next step acts on
    if (const int rc = h->model->obs(h->S, h->n, h->seed, v.obs, stream)) return rc;
    DDRL_HIP_CHECK(hipMemcpyAsync(h->ro_block, v.obs, n * 8 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return DDRL_OK;
}

int ddrl_rollout_step_discrete_articulated(ddrl_env_t *h, ddrl_dqn_t *dqn, ddrl_replay_t *replay, int32_t n_steps, int mode,
                                           float greedy_prob, uint32_t seed, uint64_t ctr, void *stream) {
    DDRL_REQUIRE(h != nullptr && dqn != nullptr && replay != nullptr, "NULL handle");
    if (const int rc = ddrl_env_refuse(h, 1u << DDRL_ENV_ARTICULATED, "ddrl_rollout_step_discrete_articulated", "ddrl_rollout_step_discrete")) return rc;
    DDRL_REQUIRE(n_steps >= 1, "n_steps must be >= 1");
    DDRL_REQUIRE(mode == DDRL_ACT_SAMPLE || mode == DDRL_ACT_DETERMINISTIC, "mode must be DDRL_ACT_SAMPLE or DDRL_ACT_DETERMINISTIC");
    const ddrl_dqn_rollout_view v = ddrl_dqn_internal_view(dqn);
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(replay);
    if (const int rc = rollout3_discrete_check("ddrl_rollout_step_discrete_articulated", h, v, &rv)) return rc;
    DDRL_REQUIRE(h->ro_block != nullptr, "ddrl_rollout_step_discrete_articulated: no ddrl_rollout_begin_discrete_articulated on this env handle yet");
    h->ro_actions = v.n_actions;
    const long long n = h->n;
    float *next_obs = h->ro_block, *q = next_obs + n * 8, *act = q + n * DDRL_ROLLOUT_MIRROR_Q;
    return rollout_discrete_step_loop(h, dqn, v, replay, rv, n_steps, mode, greedy_prob, seed, ctr, act, q, next_obs, stream);
}

int ddrl_env_rollout_mirrors(ddrl_env_t *h, const float **act, const float **q, const float **next_obs, int32_t *n_envs, int32_t *n_actions) {
    DDRL_REQUIRE(h != nullptr, "ddrl_env_rollout_mirrors: handle is NULL");
    if (const int rc = ddrl_env_refuse(h, DDRL_TAKES_LANDERS, "ddrl_env_rollout_mirrors", nullptr)) return rc;
    DDRL_REQUIRE(h->ro_block != nullptr, "ddrl_env_rollout_mirrors: no ddrl_rollout_begin_discrete_articulated on this env handle yet");
    const float *b = h->ro_block;
    if (next_obs) *next_obs = b;
    if (q) *q = b + h->n * 8;
    if (act) *act = b + h->n * (8 + DDRL_ROLLOUT_MIRROR_Q);
    if (n_envs) *n_envs = (int32_t)h->n;
    if (n_actions) *n_actions = h->ro_actions;
    return DDRL_OK;
}

// the fused n-step step's envelope (kernel: rollout_nstep.hip): 0, or the status with the reason in ddrl_last_error().  Nothing is
// launched or written before it has passed.
static int rollout_nstep_check(ddrl_env_t *h, const ddrl_actor_rollout_view &v, const ddrl_winq_view &q) {
    if (h->n % 32 != 0) {   // (first: an actor for such a row count has no direct-operand policy either, which says less)
        ddrl::set_error("fused n-step rollout step needs n_envs a multiple of 32 (n_envs %lld); use the unfused calls", h->n);
        return DDRL_ERR_UNSUPPORTED;
    }
    if (!v.ok) {
        ddrl::set_error("fused n-step rollout step: the actor has no direct-operand policy (shape outside the envelope); use "
                        "ddrl_actor_act + ddrl_env_step_wrapped + ddrl_winq_push + ddrl_replay_store_masked_ex");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (v.obs_dim != 8 || v.act != 2 || h->n % 32 != 0 || h->n > v.max_rows || (v.ver.n_slots > 0 && h->n != v.max_rows)) {
        ddrl::set_error("fused n-step rollout step needs obs_dim 8, act_dim 2 and n_envs a multiple of 32 within the actor's max_rows (all of "
                        "them with a version store): obs_dim %d, act_dim %d, n_envs %lld, max_rows %lld", v.obs_dim, v.act, h->n, v.max_rows);
        return DDRL_ERR_UNSUPPORTED;
    }
    if (q.n != h->n || q.obs != 8 || q.act != 2) {
        ddrl::set_error("fused n-step rollout step: the window queues hold %lld envs of obs_dim %d, act_dim %d; the envs are %lld of 8 and 2",
                        q.n, q.obs, q.act, h->n);
        return DDRL_ERR_UNSUPPORTED;
    }
    if (q.Ln > DDRL_NSTEP_FUSED_MAX_LN) {
        ddrl::set_error("fused n-step rollout step: Ln %d is above DDRL_NSTEP_FUSED_MAX_LN (%d: the workgroup's windows are staged in LDS); use "
                        "the unfused calls", q.Ln, DDRL_NSTEP_FUSED_MAX_LN);
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(v.device == h->device && q.device == h->device, "actor, window queues and envs must live on one device");
    return DDRL_OK;
}
static int rollout_nstep_ring_check(ddrl_env_t *h, const ddrl_winq_view &q, const ddrl_replay_dev::SamplerView &rv) {
    const ddrl_replay_dev::RingPtrs &r = rv.ring;
    if (r.n_arr != 4) {
        ddrl::set_error("fused n-step rollout step stores into a four-array window ring {o, a, r, d}; this ring has %d arrays", r.n_arr);
        return DDRL_ERR_UNSUPPORTED;
    }
    if (r.kind[0] || r.kind[1] || r.kind[2] || r.kind[3]) {
        ddrl::set_error("fused n-step rollout step stores into float32 rings only (not a compact uint8 ring)");
        return DDRL_ERR_UNSUPPORTED;
    }
    if (r.w[0] != (q.Ln + 1) * 8 || r.w[1] != q.Ln * 2 || r.w[2] != q.Ln || r.w[3] != q.Ln) {
        ddrl::set_error("fused n-step rollout step: the ring's rows {%d, %d, %d, %d} are not the queues' windows {(Ln+1)*8, Ln*2, Ln, Ln} at Ln %d",
                        r.w[0], r.w[1], r.w[2], r.w[3], q.Ln);
        return DDRL_ERR_UNSUPPORTED;
    }
    const unsigned long long al_o = reinterpret_cast<unsigned long long>(r.a[0]) | reinterpret_cast<unsigned long long>(q.o);
    const unsigned long long al_a = reinterpret_cast<unsigned long long>(r.a[1]) | reinterpret_cast<unsigned long long>(q.a);
    if (r.capacity >= (1ll << 31) || (al_o & 15ull) || (al_a & 7ull)) {
        ddrl::set_error("fused n-step rollout step: ring capacity must be below 2^31 and the window arrays vector-aligned");
        return DDRL_ERR_UNSUPPORTED;
    }
    DDRL_REQUIRE(rv.device == h->device, "the window ring lives on another device than the envs");
    return DDRL_OK;
}

// ---- the one body behind each of the two n-step pairs (one-body: rollout_nstep.hip; articulated: rollout3_nstep.hip), like
// rollout_begin / rollout_step above: the begin call — guard, envelope, then the observation rows and the readiness bytes from the queues
// (no env state is read) ...
static int rollout_nstep_begin(int kind, const char *what, ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr && winq != nullptr, "NULL handle");
    if (const int rc = ddrl_env_refuse(h, 1u << kind, what, "ddrl_rollout_begin_nstep")) return rc;
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    const ddrl_winq_view q = ddrl_winq_internal_view(winq);
    if (const int rc = rollout_nstep_check(h, v, q)) return rc;
    ddrl::DeviceGuard g(h->device);
    return ddrl_nstep_launch_begin(q.o, h->n, q.Ln, v.obs, q.t, q.save_freq, q.rdy[*q.parity], stream);
}
// ... and the step driver: guard, argument checks, envelope, then n_steps times the loop body of worker_rollout — the versioned / plain
// forward choice, the env-step kernel of the handle's model on the filled NStepLaunch, the parity flip
static int rollout_nstep_step_loop(int kind, const char *what, ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, ddrl_replay_t *window_ring, int32_t n_steps,
                                   float act_noise, float obs_noise, float reward_scale, int32_t action_repeat, int32_t limit_steps,
                                   int32_t adopt_at_episode_end, uint32_t noise_seed, uint64_t noise_ctr,
                                   const ddrl_rollout_nstep_out_t *out, void *stream) {
    DDRL_REQUIRE(h != nullptr && actor != nullptr && winq != nullptr && window_ring != nullptr, "NULL handle");
    if (const int rc = ddrl_env_refuse(h, 1u << kind, what, "ddrl_rollout_step_nstep")) return rc;
    DDRL_REQUIRE(n_steps >= 1 && action_repeat >= 1 && limit_steps >= 1, "n_steps, action_repeat and limit_steps must be >= 1");
    if (out) {
        DDRL_REQUIRE_ALIGNED(out->act, 8);
        DDRL_REQUIRE_ALIGNED(out->obs2, 16);
        DDRL_REQUIRE_ALIGNED(out->next_obs, 16);
    }
    const ddrl_actor_rollout_view v = ddrl_actor_internal_view(actor);
    const ddrl_winq_view q = ddrl_winq_internal_view(winq);
    if (const int rc = rollout_nstep_check(h, v, q)) return rc;
    const ddrl_replay_dev::SamplerView rv = ddrl_replay_sampler_view(window_ring);
    if (const int rc = rollout_nstep_ring_check(h, q, rv)) return rc;
    ddrl::DeviceGuard g(h->device);
    NStepLaunch a{};
    a.S = h->S; a.n = h->n; a.seed = h->seed; a.stats = h->stats;
    a.limit_steps = (float)limit_steps; a.act_noise = act_noise; a.obs_noise = obs_noise; a.reward_scale = reward_scale;
    a.repeat = action_repeat; a.adopt = adopt_at_episode_end ? 1 : 0;
    a.obs = v.obs; a.hp = v.hp; a.nt2 = v.nt2; a.scale = v.scale; a.noise_seed = noise_seed;
    const bool store = v.ver.n_slots > 0;
    a.slot = store ? v.ver.slot : nullptr;
    a.newest = store ? &v.ver.vs->newest : nullptr;
    a.vstride = v.ver.vstride;
    a.qo = q.o; a.qa = q.a; a.qr = q.r; a.qd = q.d; a.qt = q.t; a.Ln = q.Ln; a.save_freq = q.save_freq;
    a.rs = rv.state; a.ring = rv.ring;
    if (out) {
        a.act_out = out->act; a.obs2_out = out->obs2; a.rew_out = out->rew; a.done_out = out->done; a.next_obs_out = out->next_obs;
        a.ended_out = out->ended;
    }
    for (int k = 0; k < n_steps; ++k) {   // the loop body of worker_rollout, n_steps times with the weights the actor holds
        // the horizon is the wrapped step's limit (as ddrl_actor_act_versioned's horizon_steps)
        const int rc = rollout_versioned_step(v.ver, h->n, limit_steps, [&](bool versioned, bool fused_plan) -> int {
            a.versioned = versioned ? 1 : 0;
            a.bmu = versioned ? v.vbmu : v.bmu; a.bls = versioned ? v.vbls : v.bls;
            set_ver_plan(a, ver_plan_of(v.ver, fused_plan, v.nt2));
            if (const int frc = ddrl_actor_internal_forward(actor, h->n, stream, versioned ? 1 : 0)) return frc;
            a.noise_ctr = noise_ctr + (uint64_t)k * (uint64_t)h->n * 2ull;
            a.rdy_in = q.rdy[*q.parity]; a.rdy_out = q.rdy[1 - *q.parity];
            if (const int lrc = h->model->step_nstep(a, h->vit, h->pit, stream)) return lrc;
            *q.parity = 1 - *q.parity;
            if (!versioned && store && a.adopt) ddrl_actor_internal_step_end(actor, 0);   // an unplanned launch moved envs: the next forward plans
            return DDRL_OK;
        });
        if (rc != DDRL_OK) return rc;
        ddrl_replay_note_masked_store(window_ring);   // the row count is known on the device only
    }
    return DDRL_OK;
}

int ddrl_rollout_begin_nstep(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, void *stream) {
    return rollout_nstep_begin(DDRL_ENV_ONE_BODY, "ddrl_rollout_begin_nstep", h, actor, winq, stream);
}
int ddrl_rollout_step_nstep(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, ddrl_replay_t *window_ring, int32_t n_steps,
                            float act_noise, float obs_noise, float reward_scale, int32_t action_repeat, int32_t limit_steps,
                            int32_t adopt_at_episode_end, uint32_t noise_seed, uint64_t noise_ctr, const ddrl_rollout_nstep_out_t *out,
                            void *stream) {
    return rollout_nstep_step_loop(DDRL_ENV_ONE_BODY, "ddrl_rollout_step_nstep", h, actor, winq, window_ring, n_steps, act_noise, obs_noise, reward_scale,
                                   action_repeat, limit_steps, adopt_at_episode_end, noise_seed, noise_ctr, out, stream);
}
// ---- the same pair on the articulated lander (kernel: rollout3_nstep.hip)
int ddrl_rollout_begin_nstep_articulated(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, void *stream) {
    return rollout_nstep_begin(DDRL_ENV_ARTICULATED, "ddrl_rollout_begin_nstep_articulated", h, actor, winq, stream);
}
int ddrl_rollout_step_nstep_articulated(ddrl_env_t *h, ddrl_actor_t *actor, ddrl_winq_t *winq, ddrl_replay_t *window_ring, int32_t n_steps,
                                        float act_noise, float obs_noise, float reward_scale, int32_t action_repeat, int32_t limit_steps,
                                        int32_t adopt_at_episode_end, uint32_t noise_seed, uint64_t noise_ctr, const ddrl_rollout_nstep_out_t *out,
                                        void *stream) {
    return rollout_nstep_step_loop(DDRL_ENV_ARTICULATED, "ddrl_rollout_step_nstep_articulated", h, actor, winq, window_ring, n_steps, act_noise, obs_noise, reward_scale,
                                   action_repeat, limit_steps, adopt_at_episode_end, noise_seed, noise_ctr, out, stream);
}

int ddrl_env_stats(ddrl_env_t *h, int64_t *episodes_h, double *ret_sum_h, int64_t *len_sum_h, void *stream) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    ddrl::DeviceGuard g(h->device);
    hipStream_t s = ddrl::as_stream(stream);
    EnvStats st;
    DDRL_HIP_CHECK(hipMemcpyAsync(&st, h->stats, sizeof(st), hipMemcpyDeviceToHost, s));
    DDRL_HIP_CHECK(hipMemsetAsync(h->stats, 0, sizeof(EnvStats), s));
    DDRL_HIP_CHECK(hipStreamSynchronize(s));
    if (episodes_h) *episodes_h = st.episodes;
    if (ret_sum_h) *ret_sum_h = st.ret_sum;
    if (len_sum_h) *len_sum_h = st.len_sum;
    return DDRL_OK;
}

int ddrl_env_state_fields(ddrl_env_t *h) {
    DDRL_REQUIRE(h != nullptr, "handle is NULL");
    return h->model->fields;
}

int ddrl_env_get_state(ddrl_env_t *h, float *state_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && state_d != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    DDRL_HIP_CHECK(hipMemcpyAsync(state_d, h->S, (size_t)h->model->fields * h->n * sizeof(float), hipMemcpyDeviceToDevice, ddrl::as_stream(stream)));
    return DDRL_OK;
}

int ddrl_env_set_state(ddrl_env_t *h, const float *state_d, void *stream) {
    DDRL_REQUIRE(h != nullptr && state_d != nullptr, "NULL pointer");
    ddrl::DeviceGuard g(h->device);
    DDRL_HIP_CHECK(hipMemcpyAsync(h->S, state_d, (size_t)h->model->fields * h->n * sizeof(float), hipMemcpyDeviceToDevice, ddrl::as_stream(stream)));
    return DDRL_OK;
}

}  // extern "C"
