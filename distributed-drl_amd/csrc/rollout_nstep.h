// The fused n-step rollout step (rollout_nstep.hip) as env.hip's entry points reach it: the kernel lives in a translation unit of its
// own — like the articulated model's (env3.hip) — so that env.hip's kernels compile exactly as they did.  Internal to libddrl_hip.so.
#pragma once
#include "ddrl_common.h"
#include "replay_device.h"
#include "policy_row.h"

// What the fused step needs from a window-queue handle (winq.hip).  rdy[2]: one readiness byte per env (padded with zeros to a
// multiple of 1024), double-buffered: the launch of parity p reads rdy[p] — ready = t_queue >= Ln and t_queue % save_freq == 0 of
// the t_queue BEFORE that launch — and writes rdy[1 - p] for the next one; *parity is flipped by the host per launch.
struct ddrl_winq_view {
    float *o, *a, *r, *d;   // [n][(Ln+1)*obs], [n][Ln*act], [n][Ln], [n][Ln]
    int *t;
    long long n;
    int Ln, obs, act, save_freq, device;
    uint8_t *rdy[2];
    int *parity;
};
ddrl_winq_view ddrl_winq_internal_view(ddrl_winq_t *h);
// replay.hip, beside ddrl_replay_note_store: host mirror bookkeeping for a store whose row count only the device knows (the counters
// are re-read from the device at the next host look, as behind ddrl_replay_store_masked_ex)
void ddrl_replay_note_masked_store(ddrl_replay_t *h);

// One launch's arguments, in plain pointers (the env state block, the stats words and the version-store tables are the handles' own)
struct NStepLaunch {
    // env (ddrl_env)
    float *S;
    long long n;
    uint32_t seed;
    void *stats;            // EnvStats
    // Wrapper + episode bookkeeping
    float limit_steps, act_noise, obs_noise, reward_scale;
    int repeat, adopt;
    // policy head
    float *obs;             // [n][8] the forward's buffer: in (acted on by the forward in front) / out (the next observation)
    const float *hp;        // [8][n][16]
    const float *bmu, *bls; // head biases (slot 0's when versioned; slot s: + s * vstride)
    int nt2, versioned;
    float scale;
    uint32_t noise_seed;
    unsigned long long noise_ctr;
    int *slot;              // nullable: the actor has no version store
    const int *newest;
    long long vstride;
    // the next versioned forward's plan (vcnt nullable), version_plan.h
    int *vcnt, *perm;
    long long perm2d_off;
    VerTile *vtiles;
    VerState *vs;
    int n_slots, col_tiles, wg_slots, vt_cap;
    // window queues
    float *qo, *qa, *qr, *qd;
    int *qt;
    int Ln, save_freq;
    const uint8_t *rdy_in;
    uint8_t *rdy_out;
    // window ring
    ddrl_replay_dev::RingState *rs;
    ddrl_replay_dev::RingPtrs ring;
    // mirrors (each nullable)
    float *act_out, *obs2_out, *rew_out, *done_out, *next_obs_out;
    uint8_t *ended_out;
};
// (ddrl_nstep_launch_step / ddrl_nstep_launch_begin and the articulated lander's ddrl_nstep3_launch_step: env_launch.h.)
