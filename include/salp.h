/*
 * salp.h — C ABI of the MI355X-native batched SALP simulator (libsalp.so).
 *
 * Drop-in boundary.  The reference (Avielstein/GRASP_LAB_SALP) exposes the hot
 * path only as Python objects:
 *
 *   SalpRobotEnv(render_mode, width, height, robot, num_obstacles, obstacle_radius)
 *       src/salp_robot_env.py:35          -> salp_create / SalpParams
 *   SalpRobotEnv.reset(seed, options) -> (obs, {})
 *       src/salp_robot_env.py:114-155     -> salp_reset / salp_reset_to
 *   SalpRobotEnv.step(action) -> (obs, reward, terminated, truncated, info)
 *       src/salp_robot_env.py:196-299     -> salp_step
 *   Robot(dry_mass, init_length, init_width, max_contraction, nozzle),
 *   Nozzle(length1, length2, length3, area, mass), Robot.set_environment,
 *   Nozzle.set_angles        src/robot.py:20-21, 261-262, 443-449, 50-60
 *                                         -> SalpParams fields
 *   Robot / Nozzle state attributes (src/robot.py:261-412)
 *                                         -> salp_get_state / salp_set_state
 *   SB3 VecEnv rollout collection around env.step (src/train_robot.py:26,
 *   src/train_robot_recurrent_ppo.py:65)  -> salp_rollout (rollout-buffer fill)
 *
 * The Python host layer (grasp_lab_salp_amd/) binds these with ctypes; the
 * reference-side binding a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - Every array argument is a caller-owned DEVICE pointer (e.g. a torch
 *    tensor's data_ptr()) on the handle's device; `stream` is a hipStream_t
 *    (NULL = the legacy default stream).  Calls only enqueue work: nothing
 *    synchronises and nothing allocates after salp_create.
 *  - Return value: 0 on success, a negative SALP_E* code on error; the
 *    message is available from salp_last_error(h) (h may be NULL for errors
 *    raised by salp_create).  No C++ exception crosses this boundary.
 *  - A handle is not thread-safe: one handle per GPU per process.
 *  - Physics is fp64 end to end (the reference is NumPy fp64); observations
 *    are float32 exactly as the reference returns them; rewards are fp64.
 */
#ifndef SALP_H
#define SALP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SALP_ABI_VERSION 14

#define SALP_MAX_OBSTACLES 4
#define SALP_OBS_DIM_MAX (6 + 2 * SALP_MAX_OBSTACLES)
/* info_out row: 7 reward components, 16 episode metrics, ep return, ep length,
 * has_metrics flag, terminal hit_obstacle flag (see SALP_INFO_* below). */
#define SALP_INFO_DIM 27

#define SALP_OK 0
#define SALP_EINVAL -1
#define SALP_EHIP -2
#define SALP_ENOMEM -3

/* Constructor arguments of the reference objects.  Constants that the
 * reference hard-codes (dt=0.01, drag/added-mass coefficients, the polynomial
 * cycle-time fits, masses of buoy/skin/tube) are not parameters there and are
 * not parameters here either. */
typedef struct SalpParams {
    /* Nozzle(length1, length2, length3, area, mass)   src/robot.py:20-21 */
    double nozzle_length1, nozzle_length2, nozzle_length3, nozzle_area, nozzle_mass;
    /* Robot(dry_mass, init_length, init_width, max_contraction, nozzle)
     *                                                  src/robot.py:261-262 */
    double dry_mass, init_length, init_width, max_contraction;
    /* Robot.set_environment(density)                  src/robot.py:443-449 */
    double density;
    /* Nozzle.set_angles(angle1, angle2) done by make_env before the env is
     * built (src/train_robot.py:16)                   src/robot.py:50-60 */
    double init_angle1, init_angle2;
    /* SalpRobotEnv(width, height, num_obstacles, obstacle_radius)
     *                                                  src/salp_robot_env.py:35 */
    double obstacle_radius;
    int32_t width, height, num_obstacles;
    int32_t max_cycles; /* timeout, hard-coded 500 at src/salp_robot_env.py:274 */
    /* Randomisation switches, all off in every reference script (0 = off):
     *   Robot.enable_dynamic_randomization  src/robot.py:436-438, 594-628
     *   Robot.enable_disturbances           src/robot.py:440-441, 796-800, 834-838
     *   SalpRobotEnv.enable_action_randomization / enable_observation_randomization /
     *   enable_latency                      src/salp_robot_env.py:157-194, 293-297
     * Draws come from the device Philox stream (grasp_lab_salp_amd/csrc/
     * salp_random.h), not NumPy's MT19937: distributional parity only. */
    int32_t dynamics_randomization, disturbances, action_randomization, observation_randomization,
        latency, reserved0;
} SalpParams;

typedef struct SalpEnv SalpEnv; /* opaque handle */

/* Rollout-buffer fill targets for salp_rollout (all device pointers, rows
 * indexed [slot][env], slot = completed-step counter of that env modulo
 * `capacity`).  Any pointer may be NULL to skip that output. */
typedef struct SalpRolloutBuffers {
    int64_t capacity;      /* slots per env                                  */
    float* obs;            /* [capacity][n_envs][obs_dim]  obs AFTER the step  */
    float* actions;        /* [capacity][n_envs][3]                            */
    float* rewards;        /* [capacity][n_envs]  (float32, SB3 buffer dtype)  */
    uint8_t* dones;        /* [capacity][n_envs]  bit0 terminated, bit1 truncated */
    int64_t* steps_done;   /* [n_envs] completed env-steps counter (in/out)    */
    int64_t max_steps;     /* >0: a lane starts no env-step once steps_done
                            * reaches it (fixed-length rollouts, n_steps)     */
    int32_t chunk;         /* ticks between env-step boundaries (0 = 64)      */
    int32_t reserved;
    float* obs_before;     /* [capacity][n_envs][obs_dim]  the observation the
                            * step's action was taken from (SB3 RolloutBuffer
                            * "obs"): the previous step's obs, or the reset obs
                            * after an episode end (ABI 4)                     */
} SalpRolloutBuffers;

/* ------------------------------------------------------------ lifecycle */
int salp_abi_version(void);
void salp_default_params(SalpParams* p); /* canonical make_env config */
int salp_create(const SalpParams* p, int64_t n_envs, uint64_t seed, int64_t env_id_offset,
                int device, SalpEnv** out);
int salp_destroy(SalpEnv* h);
const char* salp_last_error(const SalpEnv* h);
int64_t salp_num_envs(const SalpEnv* h);
int salp_obs_dim(const SalpEnv* h);

/* -------------------------------------------------------------- env API */
/* reset(): per masked env (mask NULL = all) draw target + obstacles from the
 * env's Philox stream, Robot.reset(), episode trackers; writes obs rows of
 * masked envs.  obs_out [n_envs][obs_dim] (NULL allowed). */
int salp_reset(SalpEnv* h, const uint8_t* mask, float* obs_out, void* stream);
/* reset() with the target / obstacles given by the caller (the reference
 * draws them from the global np.random; parity tests inject them).
 * targets [n][2], obstacles [n][SALP_MAX_OBSTACLES][2], n_obstacles [n]. */
int salp_reset_to(SalpEnv* h, const uint8_t* mask, const float* targets, const float* obstacles,
                  const int32_t* n_obstacles, float* obs_out, void* stream);
/* One SalpRobotEnv.step per env (one breathing cycle each).
 * actions [n][3] float32 in the action box; outputs may be NULL.
 * auto_reset != 0: envs that end are reset (SB3 VecEnv semantics); their
 * obs_out row is then the reset observation and terminal_obs_out [n][obs_dim]
 * receives the final observation.  info_out [n][SALP_INFO_DIM] fp64. */
int salp_step(SalpEnv* h, const float* actions, float* obs_out, double* reward_out,
              uint8_t* terminated_out, uint8_t* truncated_out, int auto_reset,
              float* terminal_obs_out, double* info_out, void* stream);
/* Synthetic random-action rollout, chained per lane: every env runs up to
 * `tick_budget` physics ticks (dt=0.01 each) in chunks of buf->chunk ticks,
 * completing as many env-steps as fit, with actions ~ U(action box) from
 * Philox(seed; env id, step index) and auto-reset (Philox targets/obstacles).
 * Env-steps end and start only at chunk boundaries (a lane waits < chunk
 * ticks); a cycle cut by the budget resumes on the next call.  Per-env results
 * do not depend on how the work is split. */
int salp_rollout(SalpEnv* h, int64_t tick_budget, const SalpRolloutBuffers* buf, void* stream);
/* Same random actions, lock-step: every env performs exactly n_steps
 * env-steps (one full cycle each) with auto-reset.  rewards_out [n] = sum. */
int salp_step_random(SalpEnv* h, int32_t n_steps, double* reward_sum_out, void* stream);

/* ------------------------------------------------ policy-in-the-loop collection
 * PPO's collect_rollouts (stable-baselines3 OnPolicyAlgorithm.collect_rollouts,
 * around the env.step calls of the reference's on-policy learner,
 * src/train_robot_recurrent_ppo.py:65, 85-107) inside the chained kernel: every env
 * runs `n_steps` env-steps back to back; at each env-step boundary the lane
 * evaluates the policy on the env's observation and draws its action there, so
 * no env waits for the slowest cycle of the batch between steps.
 *
 * Policy: SB3 MlpPolicy with net_arch pi=[64, 64], vf=[64, 64], tanh, a
 * state-independent log_std (diagonal Gaussian).  float32 weights packed in
 * one array (torch nn.Linear weights are [out][in]; the first layer's input
 * columns are zero-padded to SALP_OBS_DIM_MAX), offsets in floats:          */
#define SALP_POLICY_HIDDEN 64
#define SALP_POLICY_PI_W1 0
#define SALP_POLICY_PI_B1 (SALP_POLICY_PI_W1 + SALP_POLICY_HIDDEN * SALP_OBS_DIM_MAX)
#define SALP_POLICY_PI_W2 (SALP_POLICY_PI_B1 + SALP_POLICY_HIDDEN)
#define SALP_POLICY_PI_B2 (SALP_POLICY_PI_W2 + SALP_POLICY_HIDDEN * SALP_POLICY_HIDDEN)
#define SALP_POLICY_ACT_W (SALP_POLICY_PI_B2 + SALP_POLICY_HIDDEN)       /* [3][64] */
#define SALP_POLICY_ACT_B (SALP_POLICY_ACT_W + 3 * SALP_POLICY_HIDDEN)   /* [3] */
#define SALP_POLICY_LOG_STD (SALP_POLICY_ACT_B + 3)                     /* [3] */
#define SALP_POLICY_VF_W1 (SALP_POLICY_LOG_STD + 3)
#define SALP_POLICY_VF_B1 (SALP_POLICY_VF_W1 + SALP_POLICY_HIDDEN * SALP_OBS_DIM_MAX)
#define SALP_POLICY_VF_W2 (SALP_POLICY_VF_B1 + SALP_POLICY_HIDDEN)
#define SALP_POLICY_VF_B2 (SALP_POLICY_VF_W2 + SALP_POLICY_HIDDEN * SALP_POLICY_HIDDEN)
#define SALP_POLICY_VAL_W (SALP_POLICY_VF_B2 + SALP_POLICY_HIDDEN)       /* [1][64] */
#define SALP_POLICY_VAL_B (SALP_POLICY_VAL_W + SALP_POLICY_HIDDEN)       /* [1] */
#define SALP_POLICY_SIZE (SALP_POLICY_VAL_B + 1)

/* Per env-step of env i, row t (its t-th step of this call):
 *   obs[t][i]      the observation the action is taken on;
 *   actions[t][i]  a = mean + exp(log_std) * z, z ~ N(0, 1) from
 *                  Philox(noise_seed; global env id, step counter); the env
 *                  receives clamp(a, Box low, Box high) (SB3 clips, buffers a);
 *   values, log_probs: V(obs), log N(a; mean, std) summed over the 3 dims;
 *   episode_starts[t][i]: 1 if obs starts an episode (in: episode_start[i]);
 *   rewards[t][i]  float32 reward; + gamma * V(terminal obs) where the episode
 *                  was truncated, not terminated (SB3's timeout bootstrap);
 *                  0 and a fresh episode where the divergence guard fires
 *                  (|obs| > diverged_obs_abs, |reward| > diverged_reward_abs or
 *                  non-finite; guard off when diverged_obs_abs <= 0);
 * last_obs[i] is in/out: on entry the observation env i's first step of this
 * call is taken on (the reset observation, or the previous call's last_obs);
 * on return episode_start[i] (next step starts an episode) and last_obs[i]
 * (the obs after the last step, the reset obs where it ended an episode).
 * ep_stats[0..3] += (return, 1, target reached (terminated), length) per
 * episode that ended by the task's rules;
 * diverged[0] += envs reset by the guard. */
typedef struct SalpPolicyRollout {
    const float* weights;  /* [SALP_POLICY_SIZE] */
    uint64_t noise_seed;
    double gamma;
    double diverged_obs_abs;
    double diverged_reward_abs;
    int64_t n_steps;
    float* obs;            /* [n_steps][n_envs][obs_dim] */
    float* actions;        /* [n_steps][n_envs][3]        */
    float* rewards;        /* [n_steps][n_envs]           */
    float* episode_starts; /* [n_steps][n_envs]           */
    float* values;         /* [n_steps][n_envs]           */
    float* log_probs;      /* [n_steps][n_envs]           */
    float* episode_start;  /* [n_envs] in/out             */
    float* last_obs;       /* [n_envs][obs_dim] in/out    */
    double* ep_stats;      /* [4] accumulated             */
    int64_t* diverged;     /* [1] accumulated             */
} SalpPolicyRollout;
int salp_collect(SalpEnv* h, const SalpPolicyRollout* r, void* stream);

/* salp_collect that also records the episodes it finishes (added under ABI 14
 * without a new number: a library without the feature lacks the symbol).  The
 * caller owns a per-env log; salp_collect is this call with a NULL log, and a
 * call with a log leaves every salp_collect output (buffers, state, ep_stats,
 * diverged) as the call without one does.
 *
 * A row is written exactly where ep_stats is updated: for an episode that
 * ended by the task's rules (terminated or truncated) in an env-step the
 * divergence guard did not drop; an env the guard reset logs nothing (the
 * lock-step callback's skip = diverged).  The row is the episode-window row
 * (SalpEpisodeWindow below, SALP_EPWIN_COLS = 20 doubles): ep_return, ep_len,
 * success = terminated, truncation = truncated and not terminated, then info
 * columns SALP_INFO_PATH_LENGTH .. SALP_INFO_AVG_R_OBSTACLE of that env-step,
 * bit for bit what salp_step's info_out holds for the same step.  Env i's e-th
 * episode of the call (0-based) goes to slot e % per_env of its own ring, with
 * step = the buffer row t it ended in; count[i] is the number of episodes env i
 * finished in this call, however many are still kept.  count is zeroed and
 * rewritten by every call; slots a call does not reach keep their contents.
 * An env is owned by one lane at a time: no atomics, two runs give the same bits.
 * SALP_EINVAL, with a message and no GPU work: per_env < 1, or a NULL rows /
 * step / count in a non-NULL log (and everything salp_collect rejects). */
typedef struct SalpEpisodeLog {
    int64_t per_env;       /* K >= 1: episodes kept per env, its latest K of the call */
    double* rows;          /* [n_envs][K][SALP_EPWIN_COLS] */
    int32_t* step;         /* [n_envs][K] */
    int32_t* count;        /* [n_envs] written by every call, not accumulated */
} SalpEpisodeLog;
int salp_collect_episodes(SalpEnv* h, const SalpPolicyRollout* r, const SalpEpisodeLog* log, void* stream);

/* Launch order of the lock-step calls (salp_step, salp_step_random): a
 * launch lasts as long as its slowest wave.  mode 1: envs run sorted by the
 * predicted length of the cycle each is about to run (longest first): the
 * waves of short cycles finish early, which lets the chip clock the long ones
 * higher, and beyond one wave per SIMD the rounds pack; 0: env order;
 * -1 (default): sorted from 1 024 envs on.  Results per env are identical in
 * every mode. */
int salp_set_lockstep_order(SalpEnv* h, int mode);

/* Kernel of the chained calls (salp_rollout, salp_collect, salp_step_random
 * from 32 env-steps on; ABI 9).  mode 0: one env per lane (k_rollout); 1: each
 * env on two waves that split its physics tick and meet once per tick through
 * LDS (k_rollout_pair: twice the waves, so an env count that leaves SIMDs idle
 * with one env per lane fills the chip); 2 (round 6): two waves per env with
 * the tick split along its one-way dependences, the B wave's angle chain
 * following the A wave's forces through an LDS ring (k_rollout_split);
 * -1 (default): a two-wave kernel while n_envs <= 128 x compute units.  The
 * two-wave kernels have no randomised instance: with a randomisation switch
 * on the chained calls use k_rollout.  Results per env are identical in every
 * mode. */
int salp_set_rollout_kernel(SalpEnv* h, int mode);
/* Partner waits of k_rollout_pair that gave up (ABI 10): the two waves of an
 * env meet once per tick; a wave that polls for its partner ~56 ms in vain
 * stops waiting, so that the kernel always ends, and that env's results of the
 * launch are then invalid.  Reads (synchronising `stream`) and clears the
 * count of such waits since the previous call, over every launch of the
 * process; 0 is the only good answer (the Python layer raises otherwise).
 * k_step_wave (salp_step) also marks such an env invalid in place: its motion
 * state is set to NaN, the state of a diverged env, so a caller that never
 * reads this count still cannot take the unfinished cycle for a result.
 * Diagnostic with no reference counterpart. */
int salp_pair_timeouts(SalpEnv* h, uint64_t* count_out, void* stream);
/* Kernel of salp_step (ABI 11): -1 auto (default), 0 one env per lane
 * (k_step, lock-step), 1 one env per wave (k_step_wave: the wave's lanes
 * compute the geometry of 64 ticks at once, then run their dynamics; a cycle's
 * latency drops to about its steady ticks').  Auto: one env per wave up to
 * 1 024 envs (the per-env SalpRobotEnv.step, src/salp_robot_env.py:196-299,
 * and small vector envs).  Recording (salp_set_trace) always uses k_step.
 * Results per env are identical in every mode.  No reference counterpart. */
int salp_set_step_kernel(SalpEnv* h, int mode);

/* GAE / returns over a rollout buffer: stable_baselines3's
 * RolloutBuffer.compute_returns_and_advantage (stable-baselines3 >= 2.0,
 * requirements.txt:6-7), which RecurrentPPO runs with gamma 0.99 and
 * gae_lambda 0.95 (src/train_robot_recurrent_ppo.py:94-95).  All buffers are
 * float32 device arrays, [n_steps][n_envs] row-major as in SB3:
 * rewards, values, episode_starts (1.0 where the step began an episode);
 * last_values / last_dones [n_envs] are the value estimate and done flag after
 * the last step.  Outputs advantages, returns [n_steps][n_envs].  Float32 with
 * SB3's operation order and NumPy 2 promotion (float32(gamma),
 * float32(gamma * gae_lambda)): bit-identical to the NumPy code. */
int salp_gae(int64_t n_steps, int64_t n_envs, const float* rewards, const float* values,
             const float* episode_starts, const float* last_values, const float* last_dones,
             double gamma, double gae_lambda, float* advantages, float* returns, void* stream);

/* Fused PPO loss head (stable_baselines3 PPO.train's clipped surrogate, value
 * MSE and entropy for a diagonal Gaussian with state-independent log-std) and
 * its gradient, for one minibatch of B rows.  Device float32 arrays: mu [B][3]
 * (policy mean), log_std [3], value [B], actions [B][3], old_logp [B],
 * advantages [B], returns [B].  normalize_advantage: SB3's per-minibatch
 * (adv - mean) / (std + 1e-8).  workspace: SALP_PPO_WORKSPACE_DOUBLES doubles.
 * Outputs: out [8] = loss, pg_loss, vf_loss, entropy, clip_fraction,
 * d loss / d log_std [3]; dmu [B][3] = d loss / d mu; dvalue [B] = d loss /
 * d value.  Float32 row math with fp64 sums (agrees with the torch expression
 * to float32 rounding).  Not part of the reference's API: it is the loss of
 * the SB3 learner the reference trains with (grasp_lab_salp_amd/ppo.py). */
#define SALP_PPO_WORKSPACE_DOUBLES 2048
int salp_ppo_loss(int64_t batch, const float* mu, const float* log_std, const float* value,
                  const float* actions, const float* old_logp, const float* advantages, const float* returns,
                  double clip_range, double ent_coef, double vf_coef, int normalize_advantage,
                  double* workspace, float* out, float* dmu, float* dvalue, void* stream);

/* One PPO minibatch step of the built-in MlpPolicy, fused (stable_baselines3
 * PPO.train's inner loop for SB3's MlpPolicy with net_arch pi = vf = [64, 64],
 * tanh: forward, the loss of salp_ppo_loss, backward, clip_grad_norm_, Adam).
 * The policy's tensors, torch.nn.Linear row-major [out][in], in this order
 * (obs_dim D <= SALP_OBS_DIM_MAX): */
enum SalpMlpTensor {
    SALP_MLP_PI_W1,   /* [64][D] */
    SALP_MLP_PI_B1,   /* [64]    */
    SALP_MLP_PI_W2,   /* [64][64] */
    SALP_MLP_PI_B2,   /* [64]    */
    SALP_MLP_ACT_W,   /* [3][64] action mean head */
    SALP_MLP_ACT_B,   /* [3]     */
    SALP_MLP_LOG_STD, /* [3]     */
    SALP_MLP_VF_W1,   /* [64][D] */
    SALP_MLP_VF_B1,   /* [64]    */
    SALP_MLP_VF_W2,   /* [64][64] */
    SALP_MLP_VF_B2,   /* [64]    */
    SALP_MLP_VAL_W,   /* [1][64] value head */
    SALP_MLP_VAL_B,   /* [1]     */
    SALP_MLP_N_TENSORS
};
/* The flat gradient / Adam-state vectors hold the tensors back to back in
 * that order: salp_ppo_mlp_offset(D, t) floats in, salp_ppo_mlp_num_params(D)
 * in all. */
int64_t salp_ppo_mlp_num_params(int obs_dim);
int64_t salp_ppo_mlp_offset(int obs_dim, int tensor);
int64_t salp_ppo_mlp_workspace_doubles(int64_t batch, int obs_dim);
/* Gradient of the loss over rows idx[0..batch) of the rollout buffer
 * (obs [N][D], actions [N][3], old_log_prob, advantages, returns [N]) into
 * grads (flat, overwritten); stats [4] += pg_loss, vf_loss, entropy,
 * clip_fraction.  Deterministic (no atomics), float32 rows, fp64 sums. */
typedef struct SalpPpoMinibatch {
    int64_t batch;
    int32_t obs_dim;
    int32_t normalize_advantage;
    const int64_t* idx;
    const float* obs;
    const float* actions;
    const float* old_log_prob;
    const float* advantages;
    const float* returns;
    float* params[SALP_MLP_N_TENSORS];
    float* grads;
    double clip_range;
    double ent_coef;
    double vf_coef;
    double* workspace;     /* salp_ppo_mlp_workspace_doubles(batch, obs_dim) */
    float* stats;          /* [4] accumulated, or NULL */
    const double* adv_part; /* ABI 12: this minibatch's advantage partials from
                               salp_ppo_mlp_adv_partials, or NULL (computed here) */
    double* norm_part;     /* ABI 13: or NULL.  The squared norm's partials of the final gradient (one per
                              64 parameters), written by the reduction: pass SalpPpoAdam.workspace here and
                              set SalpPpoAdam.norm_ready when nothing changes grads between the two calls
                              (one rank; a multi-GPU learner's all-reduce does) */
} SalpPpoMinibatch;
int salp_ppo_mlp_grads(const SalpPpoMinibatch* m, void* stream);
/* The advantage normalisation's partial sums (sum, sum of squares in fp64;
 * SALP_PPO_ADV_PARTIAL_DOUBLES per minibatch) of n_minibatches consecutive
 * minibatches of `batch` rows each (minibatch k: idx[k * batch ...]), in one
 * launch, exactly as salp_ppo_mlp_grads computes them for one minibatch; pass
 * out + k * SALP_PPO_ADV_PARTIAL_DOUBLES as minibatch k's adv_part (ABI 12:
 * one launch per epoch instead of one per minibatch).  No reference
 * counterpart (SB3 PPO.train's advantage normalisation). */
#define SALP_PPO_ADV_PARTIAL_DOUBLES 512
int salp_ppo_mlp_adv_partials(int64_t batch, int64_t n_minibatches, const int64_t* idx, const float* advantages,
                              double* out, void* stream);
/* clip_grad_norm_(max_grad_norm; <= 0: no clipping) of the flat gradient,
 * then torch.optim.Adam (no weight decay / amsgrad) on the tensors; exp_avg
 * and exp_avg_sq are flat like grads, step [1] is Adam's step count (float32,
 * incremented here), grad_norm [1] (or NULL) receives the pre-clip norm.  A
 * multi-GPU learner all-reduces grads between the two calls. */
typedef struct SalpPpoAdam {
    int32_t obs_dim;
    int32_t norm_ready;    /* ABI 13: 1 = workspace already holds the norm partials of grads
                              (SalpPpoMinibatch.norm_part); 0 = computed here (k_mlp_norm) */
    float* params[SALP_MLP_N_TENSORS];
    const float* grads;
    float* exp_avg;
    float* exp_avg_sq;
    float* step;
    float* grad_norm;
    double lr;
    double beta1;
    double beta2;
    double eps;
    double max_grad_norm;
    double* workspace;     /* ABI 13: SALP_PPO_APPLY_WORKSPACE_DOUBLES, zero-filled once by the caller and
                              then left to these calls (the norm's partials and a block-arrival count):
                              clip + Adam run over many blocks (k_mlp_adam, after k_mlp_norm unless
                              norm_ready); NULL: one block does both (k_mlp_apply) */
} SalpPpoAdam;
#define SALP_PPO_APPLY_WORKSPACE_DOUBLES 256
int salp_ppo_mlp_apply(const SalpPpoAdam* a, void* stream);
/* One step of that policy on `rows` observations in one launch on the
 * caller's stream (ActorCritic.act / .value, grasp_lab_salp_amd/ppo.py: predict,
 * evaluate and the lock-step collection): mean = actor(obs),
 * a = mean + exp(log_std) eps (eps NULL: a = mean, bit for bit; not clipped),
 * log_prob = sum -(a - mean)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi),
 * value = critic(obs).  The actor is present when action is given, the critic
 * when value is.  float32, in the operation order of salp_collect's in-kernel
 * policy: on the same observations the values are the collection's, bit for
 * bit.  A row's result depends on nothing but the row and the parameters (not
 * on rows, its position, or the networks present).  No atomics, nothing
 * allocated or synchronised; capturable in a HIP graph.  The parameter pointers
 * are the torch tensors as they are.  Rows >= rows and outputs whose pointer is
 * NULL are never written.  SALP_EINVAL before any launch for: a NULL struct,
 * rows < 0, obs_dim outside 1 .. SALP_OBS_DIM_MAX, obs NULL, both networks
 * absent, log_prob or eps without action, and a NULL tensor among those a
 * present network needs (actor: PI_W1 .. LOG_STD; critic: VF_W1 .. VAL_B).
 * rows == 0 is SALP_OK without a launch.  Added under ABI 14 without a new
 * version number: a library built before it is recognised by the missing
 * symbol.  No reference counterpart (its learners are stable-baselines3). */
typedef struct SalpPpoMlpAct {
    int64_t rows;
    int32_t obs_dim;                           /* 1 .. SALP_OBS_DIM_MAX */
    int32_t reserved;                          /* 0 */
    const float* params[SALP_MLP_N_TENSORS];   /* the policy's own tensors, SalpMlpTensor order */
    const float* obs;                          /* [rows][obs_dim] */
    const float* eps;                          /* [rows][3] N(0,1); NULL: action = mean */
    float* action;                             /* [rows][3] unclipped; NULL: actor absent */
    float* log_prob;                           /* [rows] or NULL (needs action) */
    float* value;                              /* [rows]; NULL: critic absent */
} SalpPpoMlpAct;
int salp_ppo_mlp_act(const SalpPpoMlpAct* a, void* stream);

/* The LSTM cell of RecurrentPPO's MlpLstmPolicy (sb3-contrib RecurrentPPO,
 * src/train_robot_recurrent_ppo.py:85-107; grasp_lab_salp_amd/recurrent_ppo.py),
 * elementwise part of one torch.nn.LSTM step with sb3-contrib's episode-start
 * reset: gates [rows][4 hidden] = x W_ih^T + b + (h keep) W_hh^T (i, f, g, o),
 * c_prev [rows][hidden], keep [rows] (1 - episode_start);
 * c = sigmoid(f) c_prev keep + sigmoid(i) tanh(g), h = sigmoid(o) tanh(c);
 * act [rows][4 hidden] receives the activated gates for the backward, which
 * turns dh (and dc, or NULL) into dgates and dc_prev.  float32, caller's
 * stream; not part of the reference's own API (its learner is sb3-contrib). */
int salp_lstm_cell_forward(int64_t rows, int32_t hidden, const float* gates, const float* c_prev, const float* keep,
                           float* h, float* c, float* act, void* stream);
int salp_lstm_cell_backward(int64_t rows, int32_t hidden, const float* act, const float* c_prev, const float* keep,
                            const float* c, const float* dh, const float* dc, float* dgates, float* dc_prev,
                            void* stream);
/* One step of a whole-sequence pass (the training pass of both LSTMs,
 * recurrent_ppo._LSTMPairSeqFn).  Forward: the cell of gates + gx (gx, the
 * input projection with the bias, may be NULL), and hk_next = h keep_next (the
 * next step's recurrent GEMM operand; keep_next and hk_next both NULL or
 * both set).  Backward: the cell's backward for dh = d_out + dhk_next keep_next
 * (dhk_next = d hk_next; dhk_next and keep_next both NULL or both set). */
int salp_lstm_step_forward(int64_t rows, int32_t hidden, const float* gates, const float* gx, const float* c_prev,
                           const float* keep, const float* keep_next, float* h, float* c, float* act, float* hk_next,
                           void* stream);
int salp_lstm_step_backward(int64_t rows, int32_t hidden, const float* act, const float* c_prev, const float* keep,
                            const float* c, const float* d_out, const float* dhk_next, const float* keep_next,
                            const float* dc, float* dgates, float* dc_prev, void* stream);

/* One step of the whole recurrent policy (RecurrentActorCritic.act /
 * predict_values, grasp_lab_salp_amd/recurrent_ppo.py) for `rows` envs:
 * observation and LSTM state in; action, log-prob, value and new state out.
 * Per network (actor, critic; either may be absent: all its pointers NULL):
 *   hk = h keep, ck = c keep
 *   gates = x W_ih^T + b_ih + b_hh + hk W_hh^T          (i, f, g, o)
 *   c' = sigmoid(f) ck + sigmoid(i) tanh(g), h' = sigmoid(o) tanh(c')   (the cell above)
 *   y = head(tanh(W2 tanh(W1 h' + b1) + b2))            (64-64 tanh MLP)
 * actor: mean = y [3], a = mean + exp(log_std) eps (eps NULL: a = mean),
 * log_prob = sum -(a - mean)^2 / (2 sigma^2) - log sigma - log sqrt(2 pi);
 * critic: value = y [1].  The action is not clipped.
 *
 * Two launches on the caller's stream: k_lstm_policy_cell (the gate products
 * of [hk | x | 1] on v_mfma_f32_32x32x2_f32, exact f32, K split over four
 * accumulators; a workgroup owns 32 units of one network and keeps their
 * weights in registers over its row tiles) and k_lstm_policy_head (MLP, head
 * and Gaussian on the VALU).  float32, no atomics (two calls give identical
 * bits), nothing allocated or synchronised.  The parameter pointers are the
 * torch tensors as they are (weight_hh_l0, mlp weights 16-byte aligned).
 * Rows >= rows and outputs whose pointer is NULL are never written.
 * SALP_EINVAL before any launch for: bad sizes, a needed pointer that is NULL,
 * a network given in part, both networks absent, an output of an absent
 * network, nothing to compute, state_out == NULL without latent, and
 * state_out overlapping state_in (a row's units are spread over workgroups:
 * an in-place update would race; the caller double-buffers).  rows == 0 is
 * SALP_OK.  Added under ABI 14 without a new version number: a library built
 * before it is recognised by the missing symbol. */
#define SALP_LSTM_POLICY_HIDDEN 256
#define SALP_LSTM_POLICY_MLP 64
#define SALP_LSTM_POLICY_OBS_MAX 16
#define SALP_LSTM_POLICY_ACT_DIM 3
typedef struct SalpLstmPolicyNet {
    const float* weight_ih;   /* [1024][obs_dim]  torch weight_ih_l0 */
    const float* weight_hh;   /* [1024][256]      torch weight_hh_l0 */
    const float* bias_ih;     /* [1024] */
    const float* bias_hh;     /* [1024] */
    const float* mlp_w1;      /* [64][256] */
    const float* mlp_b1;      /* [64] */
    const float* mlp_w2;      /* [64][64] */
    const float* mlp_b2;      /* [64] */
    const float* head_w;      /* actor [3][64], critic [1][64] */
    const float* head_b;      /* actor [3], critic [1] */
} SalpLstmPolicyNet;
typedef struct SalpLstmPolicyStep {
    int64_t rows;
    int32_t obs_dim;          /* 1 .. SALP_LSTM_POLICY_OBS_MAX */
    int32_t act_dim;          /* SALP_LSTM_POLICY_ACT_DIM */
    const float* obs;         /* [rows][obs_dim] */
    const float* keep;        /* [rows] 1 - episode start; NULL: all 1 */
    const float* state_in;    /* [4][rows][256]: actor h, actor c, critic h, critic c */
    float* state_out;         /* the same shape; NULL: the state is not advanced */
    float* latent;            /* [2][rows][256] h' of (actor, critic) between the launches;
                                 needed only when state_out is NULL */
    SalpLstmPolicyNet actor;
    SalpLstmPolicyNet critic;
    const float* log_std;     /* [3] */
    const float* eps;         /* [rows][3] N(0, 1) noise; NULL: deterministic */
    float* action;            /* [rows][3] or NULL */
    float* log_prob;          /* [rows] or NULL */
    float* value;             /* [rows] or NULL */
} SalpLstmPolicyStep;
int salp_lstm_policy_step(const SalpLstmPolicyStep* s, void* stream);

/* ------------------------------------------------ SAC (ABI 14)
 * The off-policy learner of src/train_robot.py:62-69 (stable_baselines3 SAC,
 * "MlpPolicy", buffer_size 100 000, batch_size 256, tau 0.005, gamma 0.99;
 * grasp_lab_salp_amd/sac.py): its replay buffer and the elementwise heads
 * around its GEMMs.  float32 like SB3; scalar sums are fp64 partials added in
 * a fixed order (no atomics: two calls give identical bits).  Not part of the
 * reference's own API: these are the SB3 functions its learner runs.
 *
 * Replay ring, SB3 ReplayBuffer's arrays with per-env cursors: row
 * [slot][env], slot < capacity.  pos[env] is the slot env writes next,
 * size[env] <= capacity the slots it has filled (both zero at the start). */
typedef struct SalpReplay {
    int64_t capacity;      /* slots per env: max(buffer_size / n_envs, 1) as SB3 */
    int64_t n_envs;
    int32_t obs_dim;
    int32_t reserved;
    float* obs;            /* [capacity][n_envs][obs_dim] the obs the action was taken on */
    float* next_obs;       /* [capacity][n_envs][obs_dim] */
    float* actions;        /* [capacity][n_envs][3] policy-scaled to [-1, 1] */
    float* rewards;        /* [capacity][n_envs] */
    float* dones;          /* [capacity][n_envs] 1.0 where terminated */
    int64_t* pos;          /* [n_envs] */
    int64_t* size;         /* [n_envs] */
} SalpReplay;
/* One lock-step env-step of every env into the ring: SB3 ReplayBuffer.add as
 * OffPolicyAlgorithm._store_transition calls it.  Inputs are what salp_step
 * with auto_reset wrote: next_obs is terminal_obs where the episode ended
 * (terminated or truncated), else obs_after; dones is 1.0 only where
 * terminated (SB3's handle_timeout_termination: a truncation does not cut the
 * bootstrap); rewards is the reward rounded to float32.  Divergence guard as
 * SalpPolicyRollout's (off when diverged_obs_abs <= 0): an env whose next_obs
 * or float32 reward is non-finite or beyond the bounds is not stored, its
 * cursors stay, and diverged_out[env] (or NULL) is 1, else 0. */
typedef struct SalpReplayAdd {
    const float* obs;            /* [n_envs][obs_dim] */
    const float* actions;        /* [n_envs][3] */
    const float* obs_after;      /* [n_envs][obs_dim] */
    const float* terminal_obs;   /* [n_envs][obs_dim] */
    const double* reward;        /* [n_envs] */
    const uint8_t* terminated;   /* [n_envs] */
    const uint8_t* truncated;    /* [n_envs] */
    double diverged_obs_abs;
    double diverged_reward_abs;
    uint8_t* diverged_out;       /* [n_envs] */
} SalpReplayAdd;
int salp_replay_add(const SalpReplay* rb, const SalpReplayAdd* a, void* stream);
/* SB3 ReplayBuffer.sample: `batch` transitions gathered into contiguous
 * arrays.  Row b draws v = Philox4x32-10(counter (lo32(update[0]),
 * hi32(update[0]), b, 0x52504C59), key (lo32(seed), hi32(seed))), update read
 * on the device:  env = (v0 * n_envs) >> 32, moved on to the next env (mod
 * n_envs) while size[env] == 0;  slot = (v1 * size[env]) >> 32  (64-bit
 * products; integer-only, so a host restatement agrees bit for bit).  At least
 * one env must have stored a transition.  env_out / slot_out [batch] (or
 * NULL) receive the pairs. */
typedef struct SalpReplaySample {
    int64_t batch;
    uint64_t seed;
    const int64_t* update; /* [1] device */
    float* obs;            /* [batch][obs_dim] */
    float* next_obs;       /* [batch][obs_dim] */
    float* actions;        /* [batch][3] */
    float* rewards;        /* [batch] */
    float* dones;          /* [batch] */
    int64_t* env_out;
    int64_t* slot_out;
} SalpReplaySample;
int salp_replay_sample(const SalpReplay* rb, const SalpReplaySample* s, void* stream);

/* SB3 SquashedDiagGaussianDistribution (proba_distribution + rsample +
 * log_prob) of SAC's actor, whose log-std is clamped to [-20, 2]
 * (sac/policies.py LOG_STD_MIN / LOG_STD_MAX).  mu, log_std (raw), eps
 * (N(0, 1) noise) [batch][3]:
 *   ls = clamp(log_std, -20, 2);  u = fmaf(exp(ls), eps, mu);  a = tanh(u);
 *   logp = sum_j(-eps^2 / 2 - ls - log(2 pi) / 2) - sum_j log(1 - a^2 + 1e-6)
 * with 1 - a^2 = fmaf(-a, a, 1).  Outputs act [batch][3], logp [batch].
 * Backward, from da [batch][3] and dlogp [batch] (either may be NULL: zero):
 *   du = da (1 - a^2) + dlogp 2 a (1 - a^2) / (1 - a^2 + 1e-6);  dmu = du;
 *   dls = du exp(ls) eps - dlogp, 0 where log_std lies outside [-20, 2]. */
int salp_sac_actor_head_forward(int64_t batch, const float* mu, const float* log_std, const float* eps,
                                float* act, float* logp, void* stream);
int salp_sac_actor_head_backward(int64_t batch, const float* log_std, const float* eps, const float* act,
                                 const float* da, const float* dlogp, float* dmu, float* dls, void* stream);

/* SB3 SAC.train's target and critic loss, and its entropy-coefficient loss.
 * alpha = exp(log_alpha[0]) is read on the device and written to
 * alpha_used[0] (SB3 uses the pre-step coefficient for the whole gradient
 * step).  Rows [batch]:
 *   target = rewards + (1 - dones) gamma (min(q1_target, q2_target) - alpha logp_next)
 *            as fmaf((1 - dones) gamma, fmaf(-alpha, logp_next, min), rewards)
 *   dq_i   = (q_i - target) / batch        (d critic_loss / d q_i)
 * out[0] = critic_loss = (mean((q1 - target)^2) + mean((q2 - target)^2)) / 2
 * out[1] = ent_coef_loss = -mean(log_alpha (logp + target_entropy)), logp the
 *          current observations' log-probability
 * out[2] = d ent_coef_loss / d log_alpha = -mean(logp + target_entropy) */
#define SALP_SAC_WORKSPACE_DOUBLES 256
typedef struct SalpSacTd {
    int64_t batch;
    const float* rewards;
    const float* dones;
    const float* q1_target;
    const float* q2_target;
    const float* logp_next;
    const float* q1;
    const float* q2;
    const float* logp;
    const float* log_alpha;  /* [1] */
    double gamma;
    double target_entropy;
    double* workspace;       /* SALP_SAC_WORKSPACE_DOUBLES */
    float* target;           /* [batch] */
    float* dq1;              /* [batch] */
    float* dq2;              /* [batch] */
    float* out;              /* [3] */
    float* alpha_used;       /* [1] */
} SalpSacTd;
int salp_sac_td_head(const SalpSacTd* t, void* stream);
/* SB3 SAC.train's actor loss: out[0] = mean(alpha_used logp - min(q1_pi,
 * q2_pi)); dlogp [batch] = alpha_used / batch; -1 / batch goes to the
 * smaller Q of each row (dq1, dq2 [batch]; the other gets 0), on a tie to q1
 * (torch.min over a dimension takes the first). */
typedef struct SalpSacPi {
    int64_t batch;
    const float* alpha_used; /* [1] as salp_sac_td_head wrote it */
    const float* logp;
    const float* q1_pi;
    const float* q2_pi;
    double* workspace;       /* SALP_SAC_WORKSPACE_DOUBLES */
    float* out;              /* [1] */
    float* dlogp;
    float* dq1;
    float* dq2;
} SalpSacPi;
int salp_sac_pi_head(const SalpSacPi* p, void* stream);
/* SB3 polyak_update on flat float32 vectors of n elements:
 * target = fmaf(tau, params, target (1 - tau)), 1 - tau formed in double and
 * then rounded to float32. */
int salp_sac_polyak(int64_t n, const float* params, float* target, double tau, void* stream);

/* SAC's networks (csrc/salp_sac_mlp.hip): one 3-layer float32 ReLU network
 *   out = W3 relu(W2 relu(W1 x + b1) + b2) + b3,   in -> 256 -> 256 -> out,
 * forward and backward, the 256 x 256 products on the f32-input matrix cores
 * (exact f32).  It is the actor (in = obs_dim, out = 6: rows 0-2 of the head
 * are mu, rows 3-5 the raw log-std) and each critic (in = obs_dim + 3, out =
 * 1).  These entry points were added under ABI 14 without a new version
 * number: nothing that existed changed, and a library of ABI 14 built before
 * them is recognised by the missing symbol salp_sac_net_forward.
 *
 * A network's parameters are one flat float32 vector, the six tensors in
 * torch Linear shapes ([out][in] row-major) back to back in SalpSacNetTensor
 * order; gradients use the same layout.  1 <= in_dim <= SALP_SAC_NET_IN_MAX,
 * 1 <= out_dim <= SALP_SAC_NET_OUT_MAX.  salp_sac_net_offset(in, out, t) is
 * the offset of tensor t (t = SALP_SAC_NET_N_TENSORS: the total, which
 * salp_sac_net_num_params returns too); -1 for a bad argument. */
#define SALP_SAC_HIDDEN 256
#define SALP_SAC_NET_IN_MAX 17
#define SALP_SAC_NET_OUT_MAX 6
#define SALP_SAC_NET_MAX_NETS 4
typedef enum SalpSacNetTensor {
    SALP_SAC_NET_W1 = 0,   /* [256][in] */
    SALP_SAC_NET_B1,       /* [256] */
    SALP_SAC_NET_W2,       /* [256][256] */
    SALP_SAC_NET_B2,       /* [256] */
    SALP_SAC_NET_W3,       /* [out][256] */
    SALP_SAC_NET_B3,       /* [out] */
    SALP_SAC_NET_N_TENSORS
} SalpSacNetTensor;
int64_t salp_sac_net_num_params(int in_dim, int out_dim);
int64_t salp_sac_net_offset(int in_dim, int out_dim, int tensor);
/* Rows per tile of the kernels, and the most row blocks the backward runs per
 * network (a block takes tiles bx, bx + blocks, ...), so a batch of
 * tile_rows * max_blocks + 1 is the smallest at which a block takes two tiles. */
int salp_sac_net_tile_rows(void);
int salp_sac_net_max_blocks(void);
/* One launch evaluates n_nets <= 4 networks of the same shape on `batch` rows.
 * Network i reads the row concat(x0[i][:, :d0], x1[i][:, :d1]) (in_dim = d0 +
 * d1; d1 = 0: x1 unused), so critic(obs, action) needs no concatenation.
 * out[i] [batch][out_dim].  h1[i], h2[i] [batch][256] receive the post-ReLU
 * activations for the backward; both NULL: not kept (out has the same bits). */
typedef struct SalpSacNetForward {
    int64_t batch;
    int32_t d0;
    int32_t d1;
    int32_t out_dim;
    int32_t n_nets;
    const float* params[4];
    const float* x0[4];     /* [batch][d0] */
    const float* x1[4];     /* [batch][d1] */
    float* out[4];
    float* h1[4];
    float* h2[4];
} SalpSacNetForward;
int salp_sac_net_forward(const SalpSacNetForward* f, void* stream);
/* The backward of the same launch from dout[i] [batch][out_dim] and the kept
 * h1[i], h2[i]:  dz2 = (dout W3) (h2 > 0),  dz1 = (dz2 W2) (h1 > 0)  (zero
 * gradient where the stored activation is exactly 0, torch's
 * threshold_backward).  dparams[i] (all set or all NULL) receive the flat
 * parameter gradient, overwritten: every row block accumulates its tiles in
 * registers and writes one float32 partial, the partials are summed in fp64
 * in a fixed order.  dx1 [batch][d1] (or NULL; needs d1 > 0) receives
 * (dz1 W1)[:, d0:] summed over the networks in index order: the action's
 * gradient through both critics.  At least one of the two is set.  No
 * floating-point atomics: two calls give identical bits.  The workspace size
 * takes the struct's own fields (d0 and d1 apart: the dx1 partials are
 * [n_nets][batch][d1]); it is fully written before it is read. */
typedef struct SalpSacNetBackward {
    int64_t batch;
    int32_t d0;
    int32_t d1;
    int32_t out_dim;
    int32_t n_nets;
    const float* params[4];
    const float* x0[4];
    const float* x1[4];
    const float* h1[4];
    const float* h2[4];
    const float* dout[4];
    float* dparams[4];
    float* dx1;
    float* workspace;       /* salp_sac_net_workspace_floats(batch, d0, d1, out_dim, n_nets) */
} SalpSacNetBackward;
int64_t salp_sac_net_workspace_floats(int64_t batch, int d0, int d1, int out_dim, int n_nets);
int salp_sac_net_backward(const SalpSacNetBackward* b, void* stream);

/* ------------------------------------------------ Episode metrics and evaluation
 * (csrc/salp_metrics.hip; recognised by their symbols, the ABI number stays.)
 * The per-env-step work of the reference's training callbacks
 * (src/train_robot.py:71-122) without a host copy: all three enqueue on the
 * caller's stream, allocate nothing, never touch the host and use no
 * floating-point atomic, so two runs on the same inputs give the same bits.
 *
 * Episode window: the device form of src/tensorboard_callback.py:36-61's
 * deque(maxlen=100) per metric.  Episode e (0-based, counted since creation in
 * count[0]) lives in row e % window.  Row layout:
 *   0 ep_return   1 ep_len   2 success = terminated != 0 (only reaching the
 *   target terminates: the reference's "terminated and not TimeLimit.truncated")
 *   3 truncation = truncated != 0 && terminated == 0
 *   4 .. 19  info columns SALP_INFO_PATH_LENGTH .. SALP_INFO_AVG_R_OBSTACLE in
 *            enum order, copied bit for bit. */
#define SALP_EPWIN_COLS 20
#define SALP_EPWIN_MAX_WINDOW 1024
#define SALP_EPSUM_DIM 84
typedef struct SalpEpisodeWindow {
    int32_t window;          /* 1 .. SALP_EPWIN_MAX_WINDOW */
    int32_t reserved;
    double* rows;            /* [window][SALP_EPWIN_COLS] */
    int64_t* count;          /* [1] episodes pushed since creation */
} SalpEpisodeWindow;
/* One lock-step env-step as salp_step wrote it. */
typedef struct SalpEpisodePush {
    int64_t n_envs;
    const double* info;          /* [n_envs][SALP_INFO_DIM] */
    const uint8_t* terminated;   /* [n_envs] */
    const uint8_t* truncated;    /* [n_envs] */
    const uint8_t* skip;         /* [n_envs] or NULL */
} SalpEpisodePush;
/* An env finishes when (terminated | truncated) != 0 and its skip byte, if
 * given, is 0 (the learner passes its diverged mask: a dropped transition logs
 * no episode).  Finishers are appended in ascending env index (the reference's
 * `for idx, info in enumerate(infos)`): with D finishers the r-th (0-based)
 * becomes episode count + r, then count += D.  If D > window only the last
 * `window` of them are written, so no two finishers of a push write one row.
 * One workgroup; any n_envs >= 1. */
int salp_episode_window_push(const SalpEpisodeWindow* w, const SalpEpisodePush* p, void* stream);
/* Merge one salp_collect_episodes log into the window: afterwards rows and
 * count equal what n_steps calls of salp_episode_window_push would have left,
 * one per buffer row t = 0, 1, ... in turn, each pushing the envs whose episode
 * ended in row t in ascending env index.  With D = sum of count[i] (dropped
 * episodes included) and c = count[0] on entry, the episode of rank r in
 * (t, i) order becomes episode c + r in row (c + r) % window; only the last
 * min(window, D) are written; count[0] += D.
 * An env with count[i] > per_env has dropped its older episodes.  If that
 * env's oldest kept episode is among the last `window` kept episodes (by
 * (t, i)), one of its dropped ones might have belonged to the window: lost[0]
 * += 1 for that env.  lost unchanged guarantees the window is exact; either
 * way the result depends on the log's contents alone.  One workgroup, any
 * n_envs >= 1 and per_env >= 1, no floating-point atomics, rows copied as
 * 64-bit integers.  SALP_EINVAL with no GPU work: window outside 1 ..
 * SALP_EPWIN_MAX_WINDOW, n_envs < 1, per_env < 1, a NULL pointer. */
int salp_episode_window_push_log(const SalpEpisodeWindow* w, const SalpEpisodeLog* log, int64_t n_envs,
                                 int64_t* lost, void* stream);
/* What src/tensorboard_callback.py:131-205 computes.  out [SALP_EPSUM_DIM]:
 *   out[0] = n = min(count, window)
 *   out[1 + 4 c + {0, 1, 2, 3}] = mean, population standard deviation (two-pass,
 *            as np.std), min, max of column c over the n rows
 *   out[81] = mean(path_length / ep_len)   out[82] = mean ep_len over success
 *   rows (NaN if none)   out[83] = number of success rows
 * With n = 0, out[0] = 0 and the rest is NaN.  fp64 sums in one fixed order. */
int salp_episode_window_summary(const SalpEpisodeWindow* w, double* out, void* stream);
/* stable_baselines3 evaluate_policy's bookkeeping over a vector env: env i
 * contributes target[i] = (n_eval_episodes + i) / n_envs episodes
 * (episode_count_targets), into slots offset[i] .. (offset the exclusive prefix
 * of target).  An env that finishes (terminated | truncated; skip is ignored)
 * with done_count[i] < target[i] writes slot offset[i] + done_count[i],
 * increments its count and decrements remaining[0] (an integer atomic); its
 * later episodes are ignored. */
typedef struct SalpEvalState {
    int64_t n_envs;
    const int32_t* target;   /* [n_envs] */
    const int64_t* offset;   /* [n_envs] */
    int32_t* done_count;     /* [n_envs] */
    double* ep_return;       /* [n_eval_episodes] */
    double* ep_len;          /* [n_eval_episodes] */
    uint8_t* success;        /* [n_eval_episodes] */
    int64_t* remaining;      /* [1] starts at n_eval_episodes */
} SalpEvalState;
int salp_eval_account(const SalpEvalState* s, const SalpEpisodePush* p, void* stream);

/* ------------------------------------------------ Robot / Nozzle level */
/* The reference's Robot API for callers that drive the robot directly,
 * without the task env (src/compare_trajectories.py:120-168,
 * src/robot.py:1103-1158): per env, in the reference's call order
 *   nozzle.set_yaw_angle(yaw); nozzle.solve_angles()   -> salp_nozzle_solve
 *   robot.set_control(contraction, coast_time, angles)  -> salp_robot_set_control
 *   robot.step_through_cycle()                          -> salp_robot_step_through_cycle
 * Python floats are float64; the *_f32 flags say that the argument is an
 * np.float32 instead (NumPy 2 then computes some of the geometry in float32,
 * as on the env path).  All arrays are device pointers with n_envs rows. */
/* Robot.reset() (src/robot.py:452-501); mask NULL = all envs */
int salp_robot_reset(SalpEnv* h, const uint8_t* mask, void* stream);
/* Nozzle.set_angles(angle1, angle2) (src/robot.py:50-60); angles [n][2] */
int salp_nozzle_set_angles(SalpEnv* h, const double* angles, void* stream);
/* Nozzle.set_yaw_angle(yaw) + Nozzle.solve_angles() (src/robot.py:62-98); yaw [n] */
int salp_nozzle_solve(SalpEnv* h, const double* yaw, int yaw_is_f32, void* stream);
/* Robot.set_control(contraction, coast_time, [angle1, angle2])
 * (src/robot.py:544-592); control [n][4] */
int salp_robot_set_control(SalpEnv* h, const double* control, int contraction_is_f32, void* stream);
/* Robot.step_through_cycle() (src/robot.py:740-777) */
int salp_robot_step_through_cycle(SalpEnv* h, void* stream);

/* Per-tick history recording (Robot.enable_history_recording, record=True:
 * the *_history lists of src/robot.py:687-738).  While a trace buffer is set,
 * salp_step and salp_robot_step_through_cycle write, for every env, sample 0
 * (the state before the cycle's first tick) and one sample per tick:
 *   rows[(t * SALP_TRACE_DIM + col) * n_envs + env],  t < max_samples
 * n_samples[env] receives the number of samples of the last cycle (ticks + 1;
 * more than max_samples means the tail was not recorded).  Force columns of
 * sample 0 are NaN (the reference's force histories are one shorter), and so
 * are its euler_angle_rate and nozzle_yaw (there the reference holds stale
 * values left by the previous cycle's last tick).  asymmetry_torque (always
 * [0, 0, 0.00*|v|] == 0) and position_front (= [length/2, 0, 0]) are not
 * recorded.  The bench paths (salp_rollout, salp_step_random) never record. */
typedef struct SalpTraceBuffer {
    int64_t max_samples;
    double* rows;          /* [max_samples][SALP_TRACE_DIM][n_envs] */
    int64_t* n_samples;    /* [n_envs] */
} SalpTraceBuffer;
/* buf NULL disables recording; the struct is copied, the arrays are not */
int salp_set_trace(SalpEnv* h, const SalpTraceBuffer* buf);

/* Switch the randomisation features of SalpParams on or off for subsequent
 * calls (the reference's enable_* methods can be called at any time). */
int salp_set_randomization(SalpEnv* h, int dynamics, int disturbances, int actions, int observations,
                           int latency);

/* --------------------------------------------------------- state access */
/* State is a struct-of-arrays of SALP_NUM_FIELDS fp64 rows of n_envs each:
 * state[field * n_envs + env].  Integer and float32 quantities are stored
 * exactly as doubles.  With every randomisation switch off the coefficient
 * fields hold the reference's means and the OU fields zero; the kernels then
 * use the constants and leave those fields alone, so a state written with
 * salp_set_state should keep them that way. */
int salp_num_fields(void);
const char* salp_field_name(int field);
int salp_trace_dim(void);   /* SALP_TRACE_DIM */
int salp_get_state(SalpEnv* h, double* state_out, void* stream);
int salp_set_state(SalpEnv* h, const double* state_in, void* stream);
/* Diagnostic: n_ticks physics ticks on every env with no env-step boundaries
 * (a cycle that ends simply continues in REST); times the tick body alone.
 * Leaves the envs in a state no reference call sequence produces. */
int salp_bench_ticks(SalpEnv* h, int32_t n_ticks, void* stream);
/* Device address of the handle's state buffer.  Its layout is internal
 * (field-major rows plus an env-major block of the fields only env-step
 * boundaries touch, grasp_lab_salp_amd/csrc/salp_device.h "state layout");
 * use salp_get_state / salp_set_state for the field-major view. */
int64_t salp_state_ptr(SalpEnv* h);
/* Device-side self-test of salp_math.h: out[r * n + i] for the rows
 * {0 sin, 1 cos, 2 tan, 3 atan2(x, y), 4 asin, 5 acos, 6 cube, 7 np_cosf,
 * 8 np_sinf, 9-10 sin and cos of the branch-free sincos, 11 x / y by the
 * tick's shared-reciprocal division, 12-13 sin and cos of the tick's yaw
 * function, 14-17 sin x, cos x, sin y, cos y of the tick's roll / pitch pair
 * function at (x, y), 18-20 the tick's world-frame rotation of (y, x, 1) by
 * the angles (x, y, x + y), 21 atan (select form), 22 atan (fdlibm's branches),
 * 23 log (under the Box-Muller draws of the disturbance and policy noise)},
 * x, y [n]; out [SALP_MATH_SELFTEST_ROWS][n]. */
#define SALP_MATH_SELFTEST_ROWS 24
int salp_math_selftest(const double* x, const double* y, int64_t n, double* out, void* stream);

/* State fields.  Names follow the reference attribute they hold. */
enum SalpField {
    /* Robot vectors (src/robot.py:358-374), body frame unless noted */
    SALP_F_V0 = 0, SALP_F_V1, SALP_F_V2,                  /* velocity */
    SALP_F_W0, SALP_F_W1, SALP_F_W2,                      /* angular_velocity */
    SALP_F_ACC0, SALP_F_ACC1, SALP_F_ACC2,                /* acceleration */
    SALP_F_ALPHA0, SALP_F_ALPHA1, SALP_F_ALPHA2,          /* angular_acceleration */
    SALP_F_ETA0, SALP_F_ETA1, SALP_F_ETA2,                /* euler_angle (world) */
    SALP_F_PW0, SALP_F_PW1, SALP_F_PW2,                   /* position_world */
    SALP_F_POS0, SALP_F_POS1, SALP_F_POS2,                /* position */
    SALP_F_ANG0, SALP_F_ANG1, SALP_F_ANG2,                /* angle */
    SALP_F_PPOS0, SALP_F_PPOS1, SALP_F_PPOS2,             /* prev_position */
    SALP_F_PANG0, SALP_F_PANG1, SALP_F_PANG2,             /* prev_angle */
    SALP_F_AVGV0, SALP_F_AVGV1, SALP_F_AVGV2,             /* avg_cycle_velocity */
    SALP_F_AVGW0, SALP_F_AVGW1, SALP_F_AVGW2,             /* avg_cycle_angular_velocity */
    /* body geometry / mass properties (src/robot.py:325-339) */
    SALP_F_LENGTH, SALP_F_WIDTH, SALP_F_VOLUME, SALP_F_PREV_VOLUME,
    SALP_F_COM, SALP_F_COM_RATE, SALP_F_COM_ACC,          /* x components (y,z == 0) */
    SALP_F_PREV_I0, SALP_F_PREV_I1, SALP_F_PREV_I2,       /* diag(prev_I) */
    /* NumPy dtype of length/width/volume (1 = np.float32, see DESIGN.md
     * §NEP 50) and of prev_water_volume */
    SALP_F_GEOM32, SALP_F_PVOL32,
    /* cycle (src/robot.py:311-322) */
    SALP_F_CYCLE_TIME, SALP_F_TIME, SALP_F_REFILL_TIME, SALP_F_JET_TIME, SALP_F_COAST_TIME,
    SALP_F_CONTRACTION, SALP_F_CONTRACT_RATE, SALP_F_RELEASE_RATE, SALP_F_PHASE, SALP_F_CYCLE,
    /* 1 if `contraction` is an np.float32 (always on the env path, where it
     * comes from the float32 action; 0 for a Python float passed to
     * Robot.set_control): selects float32 vs float64 body geometry */
    SALP_F_CONTR32,
    /* nozzle (src/robot.py:30-44) */
    SALP_F_ANGLE1, SALP_F_ANGLE2, SALP_F_PREV_ANGLE1, SALP_F_PREV_ANGLE2,
    SALP_F_YAW, SALP_F_PREV_YAW, SALP_F_TURN_TIME,
    /* env (src/salp_robot_env.py:114-155) */
    SALP_F_TARGET0, SALP_F_TARGET1,
    SALP_F_OBST0, SALP_F_OBST_END = SALP_F_OBST0 + 2 * SALP_MAX_OBSTACLES - 1,
    SALP_F_N_OBST, SALP_F_PREV_DIST, SALP_F_PREV_A2,
    /* episode trackers (src/salp_robot_env.py:145-153, 399-447) */
    SALP_F_EP_LEN, SALP_F_EP_RETURN, SALP_F_PATH_LEN, SALP_F_LAST_PX, SALP_F_LAST_PY,
    SALP_F_SUM_A0, SALP_F_SUM_A1, SALP_F_SUM_ABS_A2, SALP_F_SUM_VEL, SALP_F_INIT_DIST,
    SALP_F_SUM_R0, SALP_F_SUM_R_END = SALP_F_SUM_R0 + 6,
    /* in-flight env-step (action of the cycle being simulated) + RNG counters */
    SALP_F_ACT0, SALP_F_ACT1, SALP_F_ACT2, SALP_F_PENDING,
    SALP_F_STEP_COUNT, SALP_F_EPISODE,
    /* coefficients of the current cycle (src/robot.py:300-306 means, or the
     * Robot._randomize_parameters draw): discharge coefficient, drag force /
     * torque ratios, diag of the added-mass (rate) coefficient matrices */
    SALP_F_CD, SALP_F_DFR, SALP_F_DTR,
    SALP_F_AMF0, SALP_F_AMF1, SALP_F_AMF2, SALP_F_AMRF0, SALP_F_AMRF1, SALP_F_AMRF2,
    SALP_F_AMT0, SALP_F_AMT1, SALP_F_AMT2, SALP_F_AMRT0, SALP_F_AMRT1, SALP_F_AMRT2,
    /* OUDisturbance states (force, torque) and the randomisation counters */
    SALP_F_OUF0, SALP_F_OUF1, SALP_F_OUF2, SALP_F_OUT0, SALP_F_OUT1, SALP_F_OUT2,
    SALP_F_RNG_CTL, SALP_F_RNG_TICK,
    SALP_NUM_FIELDS
};

/* info_out columns */
enum SalpInfo {
    SALP_INFO_R_TRACK = 0, SALP_INFO_R_HEADING, SALP_INFO_R_SMOOTH, SALP_INFO_R_YAW,
    SALP_INFO_R_TIME, SALP_INFO_R_SIDESLIP, SALP_INFO_R_OBSTACLE,
    SALP_INFO_PATH_LENGTH, SALP_INFO_DIRECT_DISTANCE, SALP_INFO_PATH_EFFICIENCY,
    SALP_INFO_FINAL_DISTANCE, SALP_INFO_INITIAL_DISTANCE, SALP_INFO_AVG_COMPRESSION,
    SALP_INFO_AVG_COAST_TIME, SALP_INFO_AVG_NOZZLE_ANGLE, SALP_INFO_AVG_VELOCITY,
    SALP_INFO_AVG_R_TRACK, SALP_INFO_AVG_R_HEADING, SALP_INFO_AVG_R_SMOOTH, SALP_INFO_AVG_R_YAW,
    SALP_INFO_AVG_R_TIME, SALP_INFO_AVG_R_SIDESLIP, SALP_INFO_AVG_R_OBSTACLE,
    SALP_INFO_EP_RETURN, SALP_INFO_EP_LEN, SALP_INFO_HAS_METRICS, SALP_INFO_HIT_OBSTACLE
};

/* trace columns (src/robot.py:687-738 history names without "_history") */
enum SalpTraceCol {
    SALP_T_STATE = 0,                                   /* phase value */
    SALP_T_PW0, SALP_T_PW1, SALP_T_PW2,                 /* position_world */
    SALP_T_V0, SALP_T_V1, SALP_T_V2,                    /* velocity */
    SALP_T_ACC0, SALP_T_ACC1, SALP_T_ACC2,              /* acceleration */
    SALP_T_ETA0, SALP_T_ETA1, SALP_T_ETA2,              /* euler_angle */
    SALP_T_ETAR0, SALP_T_ETAR1, SALP_T_ETAR2,           /* euler_angle_rate */
    SALP_T_W0, SALP_T_W1, SALP_T_W2,                    /* angular_velocity */
    SALP_T_ALPHA0, SALP_T_ALPHA1, SALP_T_ALPHA2,        /* angular_acceleration */
    SALP_T_LENGTH, SALP_T_WIDTH,
    SALP_T_AREA0, SALP_T_AREA1, SALP_T_AREA2,
    SALP_T_VOLUME, SALP_T_MASS, SALP_T_MASS_RATE,       /* mass[0,0], mass_rate[0,0] */
    SALP_T_NOZZLE_YAW,                                  /* nozzle.current_yaw */
    SALP_T_I0, SALP_T_I1, SALP_T_I2,                    /* inertia_tensor (diag) */
    SALP_T_TCD0, SALP_T_TCD1, SALP_T_TCD2,              /* trans_drag_coefficient */
    SALP_T_RCD0, SALP_T_RCD1, SALP_T_RCD2,              /* rot_drag_coefficient */
    SALP_T_COM, SALP_T_COM_RATE, SALP_T_COM_ACC,        /* x components (y, z == 0) */
    SALP_T_FRONT_W0, SALP_T_FRONT_W1, SALP_T_FRONT_W2,  /* position_front_world */
    /* force values (NaN in sample 0) */
    SALP_T_JETV0, SALP_T_JETV1, SALP_T_JETV2,           /* jet_velocity */
    SALP_T_JETF0, SALP_T_JETF1, SALP_T_JETF2,           /* jet_force */
    SALP_T_JETT0, SALP_T_JETT1, SALP_T_JETT2,           /* jet_torque */
    SALP_T_DRAGF0, SALP_T_DRAGF1, SALP_T_DRAGF2,        /* drag_force */
    SALP_T_DRAGT0, SALP_T_DRAGT1, SALP_T_DRAGT2,        /* drag_torque */
    SALP_T_CORF0, SALP_T_CORF1, SALP_T_CORF2,           /* coriolis_force */
    SALP_T_CORT0, SALP_T_CORT1, SALP_T_CORT2,           /* coriolis_torque */
    SALP_T_AMF0, SALP_T_AMF1, SALP_T_AMF2,              /* added_mass_force */
    SALP_T_AMT0, SALP_T_AMT1, SALP_T_AMT2,              /* added_mass_torque */
    SALP_T_DEFT0, SALP_T_DEFT1, SALP_T_DEFT2,           /* deform_torque */
    SALP_T_ACCF0, SALP_T_ACCF1, SALP_T_ACCF2,           /* acceleration_force */
    SALP_TRACE_DIM
};
#define SALP_T_FIRST_FORCE SALP_T_JETV0

#ifdef __cplusplus
}
#endif
#endif /* SALP_H */
