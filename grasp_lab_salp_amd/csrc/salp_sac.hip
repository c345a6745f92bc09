// salp_sac.hip — replay buffer and loss heads of the on-device SAC learner (gfx950).
//
// What it restates: stable_baselines3 (>= 2.0, requirements.txt:6-7) SAC as
// src/train_robot.py:62-69 configures it, minus the GEMMs (those stay library
// calls, grasp_lab_salp_amd/sac.py):
//
//   k_replay_add     ReplayBuffer.add + OffPolicyAlgorithm._store_transition
//                    (terminal observation as next_obs, timeouts do not cut
//                    the bootstrap), with the learner's divergence guard
//   k_replay_sample  ReplayBuffer.sample: a uniform (env, slot) draw per row
//                    from Philox, and the gather
//   k_actor_fwd/bwd  SquashedDiagGaussianDistribution: rsample, tanh, log_prob
//   k_td_rows/final  SAC.train: entropy-regularised TD target, critic MSE and
//                    its gradient, the entropy coefficient's loss
//   k_pi_rows/final  SAC.train: actor loss and its gradient
//   k_polyak         polyak_update on flat vectors
//
// float32 row math like SB3; sums are fp64 block partials in a workspace, added
// in a fixed order by one block (no atomics: two runs give the same bits).
// Everything is enqueued on the caller's stream, nothing allocates or
// synchronises, and values that change between gradient steps (the update
// counter, log alpha) are read from device memory, so a captured graph of the
// step can be replayed.  -ffp-contract=off holds: a fused multiply-add is
// written fmaf where one rounding is wanted.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/salp.h"
#include "salp_host.h"
#include "salp_philox.h"

using salp::check_hip;
using salp::fail;

/* Stream tag (Philox counter word 3) of the replay sampler, "RPLY".  The
 * tags of salp_philox.h are small integers or-ed with bits of the env id's
 * high word (SP_STREAM_RESET | hi32(env_id) << 1 equals this tag for hi32 =
 * 0x29282626): the tag cannot collide with them for env ids below 2^32, and
 * beyond that only if the other counter words and the key matched too. */
#define SP_STREAM_REPLAY 0x52504C59u

namespace {

constexpr int kBlock = 256;
constexpr int kGrid = SALP_SAC_WORKSPACE_DOUBLES / 4;   // row blocks at most; 4 partials per block
constexpr float kHalfLog2Pi = 0.91893853320467274178f;
constexpr float kSquashEps = 1e-6f;                      // SB3 SquashedDiagGaussianDistribution.epsilon
constexpr float kLogStdMin = -20.0f, kLogStdMax = 2.0f;  // SB3 sac.policies LOG_STD_MIN / LOG_STD_MAX

__device__ __forceinline__ double block_sum(double v, double* sh) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int w = threadIdx.x / 64, l = threadIdx.x % 64;
    __syncthreads();
    if (l == 0) sh[w] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int k = 0; k < kBlock / 64; ++k) t += sh[k];
    return t;   // valid in thread 0
}

__device__ __forceinline__ bool beyond(float x, float bound) { return !isfinite(x) || fabsf(x) > bound; }

// One thread per env: a row is at most 2 x 14 + 5 floats.
__global__ __launch_bounds__(kBlock) void k_replay_add(SalpReplay rb, SalpReplayAdd a) {
    const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= rb.n_envs) return;
    const int D = rb.obs_dim;
    const bool term = a.terminated[e] != 0;
    const bool done = term || a.truncated[e] != 0;
    const float* nxt = (done ? a.terminal_obs : a.obs_after) + e * D;
    const float rew = (float)a.reward[e];
    bool bad = false;
    if (a.diverged_obs_abs > 0) {
        const float ob = (float)a.diverged_obs_abs, rb_ = (float)a.diverged_reward_abs;
        bad = beyond(rew, rb_);
        for (int k = 0; k < D; ++k) bad |= beyond(nxt[k], ob);
    }
    if (a.diverged_out) a.diverged_out[e] = bad ? 1 : 0;
    if (bad) return;   // not stored: the env's cursor stays
    const int64_t p = rb.pos[e];
    const int64_t row = p * rb.n_envs + e;
    const float* cur = a.obs + e * D;
    for (int k = 0; k < D; ++k) {
        rb.obs[row * D + k] = cur[k];
        rb.next_obs[row * D + k] = nxt[k];
    }
    for (int k = 0; k < 3; ++k) rb.actions[row * 3 + k] = a.actions[e * 3 + k];
    rb.rewards[row] = rew;
    rb.dones[row] = term ? 1.0f : 0.0f;
    rb.pos[e] = p + 1 == rb.capacity ? 0 : p + 1;
    const int64_t s = rb.size[e];
    if (s < rb.capacity) rb.size[e] = s + 1;
}

// 32 lanes per row (2 D + 5 <= 33 columns): each lane repeats the row's
// integer draw (10 Philox rounds) and copies its columns.
__global__ __launch_bounds__(kBlock) void k_replay_sample(SalpReplay rb, SalpReplaySample s) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t b = t >> 5;
    const int j = (int)(t & 31);
    if (b >= s.batch) return;
    const uint64_t upd = (uint64_t)s.update[0];
    const sp_u32x4 r = sp_philox4x32_10((uint32_t)upd, (uint32_t)(upd >> 32), (uint32_t)b, SP_STREAM_REPLAY,
                                        (uint32_t)s.seed, (uint32_t)(s.seed >> 32));
    const int64_t n = rb.n_envs;
    int64_t env = (int64_t)(((uint64_t)r.v[0] * (uint64_t)n) >> 32);
    int64_t sz = rb.size[env];
    for (int64_t tries = 1; sz == 0 && tries < n; ++tries) {   // an env that never stored
        env = env + 1 == n ? 0 : env + 1;
        sz = rb.size[env];
    }
    // an empty buffer (the caller's error) reads slot 0, which exists
    const int64_t slot = (int64_t)(((uint64_t)r.v[1] * (uint64_t)sz) >> 32);
    const int64_t row = slot * n + env;
    const int D = rb.obs_dim;
    for (int k = j; k < 2 * D + 5; k += 32) {
        if (k < D) s.obs[b * D + k] = rb.obs[row * D + k];
        else if (k < 2 * D) s.next_obs[b * D + (k - D)] = rb.next_obs[row * D + (k - D)];
        else if (k < 2 * D + 3) s.actions[b * 3 + (k - 2 * D)] = rb.actions[row * 3 + (k - 2 * D)];
        else if (k == 2 * D + 3) s.rewards[b] = rb.rewards[row];
        else s.dones[b] = rb.dones[row];
    }
    if (j == 0 && s.env_out) s.env_out[b] = env;
    if (j == 0 && s.slot_out) s.slot_out[b] = slot;
}

// a = tanh(mu + exp(ls) eps), logp = log N(u; mu, exp(ls)) - sum log(1 - a^2 + 1e-6)
__global__ __launch_bounds__(kBlock) void k_actor_fwd(int64_t B, const float* __restrict__ mu,
                                                      const float* __restrict__ log_std,
                                                      const float* __restrict__ eps, float* __restrict__ act,
                                                      float* __restrict__ logp) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    float gauss = 0.0f, squash = 0.0f;
    for (int j = 0; j < 3; ++j) {
        const float ls = fminf(fmaxf(log_std[3 * b + j], kLogStdMin), kLogStdMax);
        const float e = eps[3 * b + j];
        const float a = tanhf(fmaf(expf(ls), e, mu[3 * b + j]));
        act[3 * b + j] = a;
        gauss += -0.5f * (e * e) - ls - kHalfLog2Pi;
        squash += logf(fmaf(-a, a, 1.0f) + kSquashEps);   // 1 - a^2 in one rounding
    }
    logp[b] = gauss - squash;
}

// da, dlogp may be null (no gradient through that output)
__global__ __launch_bounds__(kBlock) void k_actor_bwd(int64_t B, const float* __restrict__ log_std,
                                                      const float* __restrict__ eps, const float* __restrict__ act,
                                                      const float* __restrict__ da, const float* __restrict__ dlogp,
                                                      float* __restrict__ dmu, float* __restrict__ dls) {
    const int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (b >= B) return;
    const float dl = dlogp ? dlogp[b] : 0.0f;
    for (int j = 0; j < 3; ++j) {
        const float raw = log_std[3 * b + j];
        const float ls = fminf(fmaxf(raw, kLogStdMin), kLogStdMax);
        const float a = act[3 * b + j];
        const float om = fmaf(-a, a, 1.0f);
        const float du = (da ? da[3 * b + j] : 0.0f) * om + dl * (2.0f * a * om / (om + kSquashEps));
        dmu[3 * b + j] = du;
        // torch's clamp passes the gradient on the closed interval
        dls[3 * b + j] = (raw >= kLogStdMin && raw <= kLogStdMax) ? du * expf(ls) * eps[3 * b + j] - dl : 0.0f;
    }
}

// Rows in float32, each product-and-add of the target in one rounding; the
// squared errors and the entropy term are formed in double from the float32
// row values (exact), so the scalars carry the target's rounding only.
__global__ __launch_bounds__(kBlock) void k_td_rows(SalpSacTd t, float gamma) {
    __shared__ double sh[kBlock / 64];
    const float alpha = expf(t.log_alpha[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) t.alpha_used[0] = alpha;
    const float invB = 1.0f / (float)t.batch;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < t.batch; b += (int64_t)gridDim.x * kBlock) {
        const float nq = fmaf(-alpha, t.logp_next[b], fminf(t.q1_target[b], t.q2_target[b]));
        const float tg = fmaf((1.0f - t.dones[b]) * gamma, nq, t.rewards[b]);
        t.target[b] = tg;
        const double e1 = (double)t.q1[b] - (double)tg, e2 = (double)t.q2[b] - (double)tg;
        t.dq1[b] = (float)e1 * invB;
        t.dq2[b] = (float)e2 * invB;
        acc[0] += e1 * e1;
        acc[1] += e2 * e2;
        acc[2] += (double)t.logp[b] + t.target_entropy;
    }
    for (int k = 0; k < 3; ++k) {
        const double v = block_sum(acc[k], sh);
        if (threadIdx.x == 0) t.workspace[4 * blockIdx.x + k] = v;
    }
}

__global__ __launch_bounds__(kBlock) void k_td_final(SalpSacTd t, int blocks) {
    __shared__ double sh[kBlock / 64];
    double s[3];
    for (int k = 0; k < 3; ++k)
        s[k] = block_sum((int)threadIdx.x < blocks ? t.workspace[4 * threadIdx.x + k] : 0.0, sh);
    if (threadIdx.x == 0) {
        const double B = (double)t.batch;
        const double m = s[2] / B;                          // mean(logp + target_entropy)
        t.out[0] = (float)(0.5 * (s[0] / B + s[1] / B));    // critic_loss
        t.out[1] = (float)(-(double)t.log_alpha[0] * m);    // ent_coef_loss
        t.out[2] = (float)(-m);                             // d ent_coef_loss / d log_alpha
    }
}

__global__ __launch_bounds__(kBlock) void k_pi_rows(SalpSacPi p) {
    __shared__ double sh[kBlock / 64];
    const float alpha = p.alpha_used[0];
    const float invB = 1.0f / (float)p.batch;
    const float dl = alpha * invB;
    double acc = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * kBlock + threadIdx.x; b < p.batch; b += (int64_t)gridDim.x * kBlock) {
        const float a1 = p.q1_pi[b], a2 = p.q2_pi[b];
        const bool first = a1 <= a2;   // a tie goes to q1: torch.min(dim) takes the first
        acc += (double)alpha * (double)p.logp[b] - (double)(first ? a1 : a2);   // exact product
        p.dlogp[b] = dl;
        p.dq1[b] = first ? -invB : 0.0f;
        p.dq2[b] = first ? 0.0f : -invB;
    }
    const double v = block_sum(acc, sh);
    if (threadIdx.x == 0) p.workspace[4 * blockIdx.x] = v;
}

__global__ __launch_bounds__(kBlock) void k_pi_final(SalpSacPi p, int blocks) {
    __shared__ double sh[kBlock / 64];
    const double s = block_sum((int)threadIdx.x < blocks ? p.workspace[4 * threadIdx.x] : 0.0, sh);
    if (threadIdx.x == 0) p.out[0] = (float)(s / (double)p.batch);
}

__global__ __launch_bounds__(kBlock) void k_polyak(int64_t n, const float* __restrict__ params,
                                                   float* __restrict__ target, float tau, float one_minus_tau) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
        target[i] = fmaf(tau, params[i], target[i] * one_minus_tau);
}

static_assert(kGrid <= kBlock, "the final kernels reduce one partial per thread");

inline unsigned blocks_for(int64_t n, int64_t cap) {
    const int64_t b = (n + kBlock - 1) / kBlock;
    return (unsigned)(b < cap ? b : cap);
}

bool replay_ok(const SalpReplay* rb) {
    // row indices stay far inside int64: capacity x n_envs x obs_dim elements are allocated by the caller
    return rb && rb->capacity > 0 && rb->n_envs > 0 && rb->obs_dim > 0 && rb->obs_dim <= SALP_OBS_DIM_MAX &&
           rb->n_envs <= INT32_MAX && rb->obs && rb->next_obs && rb->actions && rb->rewards && rb->dones && rb->pos &&
           rb->size;
}

}  // namespace

extern "C" {

// The launch status of each: one hipGetLastError() right after the launches (salp_ppo.hip explains why).
int salp_replay_add(const SalpReplay* rb, const SalpReplayAdd* a, void* stream) {
    if (!replay_ok(rb)) return fail(SALP_EINVAL, "salp_replay_add: bad replay buffer");
    if (!a || !a->obs || !a->actions || !a->obs_after || !a->terminal_obs || !a->reward || !a->terminated ||
        !a->truncated)
        return fail(SALP_EINVAL, "salp_replay_add: null buffer");
    hipLaunchKernelGGL(k_replay_add, dim3(blocks_for(rb->n_envs, INT32_MAX)), dim3(kBlock), 0, (hipStream_t)stream,
                       *rb, *a);
    return check_hip(hipGetLastError(), "k_replay_add");
}

int salp_replay_sample(const SalpReplay* rb, const SalpReplaySample* s, void* stream) {
    if (!replay_ok(rb)) return fail(SALP_EINVAL, "salp_replay_sample: bad replay buffer");
    if (!s || s->batch <= 0 || s->batch > (int64_t)1 << 32)   // the row index is a 32-bit Philox counter word
        return fail(SALP_EINVAL, "salp_replay_sample: batch must be in 1 .. 2^32");
    if (!s->update || !s->obs || !s->next_obs || !s->actions || !s->rewards || !s->dones)
        return fail(SALP_EINVAL, "salp_replay_sample: null buffer");
    hipLaunchKernelGGL(k_replay_sample, dim3(blocks_for(s->batch * 32, INT32_MAX)), dim3(kBlock), 0,
                       (hipStream_t)stream, *rb, *s);
    return check_hip(hipGetLastError(), "k_replay_sample");
}

int salp_sac_actor_head_forward(int64_t batch, const float* mu, const float* log_std, const float* eps,
                                float* act, float* logp, void* stream) {
    if (batch <= 0) return fail(SALP_EINVAL, "salp_sac_actor_head_forward: batch must be positive");
    if (!mu || !log_std || !eps || !act || !logp)
        return fail(SALP_EINVAL, "salp_sac_actor_head_forward: null buffer");
    hipLaunchKernelGGL(k_actor_fwd, dim3(blocks_for(batch, INT32_MAX)), dim3(kBlock), 0, (hipStream_t)stream, batch,
                       mu, log_std, eps, act, logp);
    return check_hip(hipGetLastError(), "k_actor_fwd");
}

int salp_sac_actor_head_backward(int64_t batch, const float* log_std, const float* eps, const float* act,
                                 const float* da, const float* dlogp, float* dmu, float* dls, void* stream) {
    if (batch <= 0) return fail(SALP_EINVAL, "salp_sac_actor_head_backward: batch must be positive");
    if (!log_std || !eps || !act || !dmu || !dls)
        return fail(SALP_EINVAL, "salp_sac_actor_head_backward: null buffer");
    hipLaunchKernelGGL(k_actor_bwd, dim3(blocks_for(batch, INT32_MAX)), dim3(kBlock), 0, (hipStream_t)stream, batch,
                       log_std, eps, act, da, dlogp, dmu, dls);
    return check_hip(hipGetLastError(), "k_actor_bwd");
}

int salp_sac_td_head(const SalpSacTd* t, void* stream) {
    if (!t || t->batch <= 0) return fail(SALP_EINVAL, "salp_sac_td_head: batch must be positive");
    if (!t->rewards || !t->dones || !t->q1_target || !t->q2_target || !t->logp_next || !t->q1 || !t->q2 || !t->logp ||
        !t->log_alpha || !t->workspace || !t->target || !t->dq1 || !t->dq2 || !t->out || !t->alpha_used)
        return fail(SALP_EINVAL, "salp_sac_td_head: null buffer");
    const unsigned g = blocks_for(t->batch, kGrid);
    hipLaunchKernelGGL(k_td_rows, dim3(g), dim3(kBlock), 0, (hipStream_t)stream, *t, (float)t->gamma);
    hipLaunchKernelGGL(k_td_final, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, *t, (int)g);
    return check_hip(hipGetLastError(), "k_td");
}

int salp_sac_pi_head(const SalpSacPi* p, void* stream) {
    if (!p || p->batch <= 0) return fail(SALP_EINVAL, "salp_sac_pi_head: batch must be positive");
    if (!p->alpha_used || !p->logp || !p->q1_pi || !p->q2_pi || !p->workspace || !p->out || !p->dlogp || !p->dq1 ||
        !p->dq2)
        return fail(SALP_EINVAL, "salp_sac_pi_head: null buffer");
    const unsigned g = blocks_for(p->batch, kGrid);
    hipLaunchKernelGGL(k_pi_rows, dim3(g), dim3(kBlock), 0, (hipStream_t)stream, *p);
    hipLaunchKernelGGL(k_pi_final, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, *p, (int)g);
    return check_hip(hipGetLastError(), "k_pi");
}

int salp_sac_polyak(int64_t n, const float* params, float* target, double tau, void* stream) {
    if (n <= 0 || !params || !target) return fail(SALP_EINVAL, "salp_sac_polyak: bad argument");
    if (!(tau >= 0 && tau <= 1)) return fail(SALP_EINVAL, "salp_sac_polyak: tau must be in [0, 1]");
    // 1 - tau in double, then rounded: 1.0f - (float)0.005 is 1.1e-8 away from it
    hipLaunchKernelGGL(k_polyak, dim3(blocks_for(n, 1024)), dim3(kBlock), 0, (hipStream_t)stream, n, params, target,
                       (float)tau, (float)(1.0 - tau));
    return check_hip(hipGetLastError(), "k_polyak");
}

}  // extern "C"
