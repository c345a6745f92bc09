// salp_ppo_act.hip — salp_ppo_mlp_act (include/salp.h): one step of PPO's
// 64-64 tanh MlpPolicy on a batch of observations in one launch, for predict,
// evaluate and the lock-step collection's _act / _terminal_value /
// _last_values (grasp_lab_salp_amd/ppo.py FusedMlpAct).
//
// The arithmetic restates the in-kernel policy of salp_collect
// (salp_kernels.hip policy_layer1 / policy_mlp / policy_act) operation for
// operation, so that what evaluates a policy is, bit for bit, the function that
// collected its data (tests/test_gpu_ppo_act.py; every action, log-prob and
// value of a collection: tests/test_gpu_collect_policy.py):
//   layer 1   acc = b1[j]; acc = fma(W1[j][k], x[k], acc), k ascending over the
//             SALP_OBS_DIM_MAX zero-padded inputs; salp_tanhf
//   layer 2   even-k products summed from b2[j], odd-k products from 0, each
//             with fma in ascending k; salp_tanhf(even + odd)
//   head      out[c] = fmaf(Wh[c][j], t_j, out[c]), j ascending from 0; + bh[c]
//   Gaussian  policy_act's expressions, eps in the place of the Philox noise
//
// Shape: grid (row tiles of 64, networks present), 256 threads.  Thread
// (j = tid & 63, g = tid >> 6) owns hidden unit j of its network for the 16
// rows of quarter g: the unit's first- and second-layer weight rows stay in
// registers, the tile's inputs and activations in LDS (read as wave-wide
// broadcasts: a wave's lanes share the row), 8 rows interleaved per thread.
// The 64-step head chains run one per (row, output) on up to 192 threads, the
// Gaussian on one wave.  A row is computed by one thread per unit whatever the
// row count or the networks present: its bits do not depend on either.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "salp_host.h"
#include "salp_tanh.h"

using namespace salp;

namespace {

constexpr int AH = SALP_POLICY_HIDDEN;   // hidden units per layer
constexpr int AIN = SALP_OBS_DIM_MAX;    // first-layer inputs, zero-padded as in the packed policy
constexpr int ATR = 64;                  // rows per workgroup
constexpr int AXS = 16;                  // floats per input row in LDS (16-byte reads)
constexpr int AHS = AH + 1;              // second activation / head weight stride: the head reads a row per lane
constexpr int ARI = 8;                   // rows interleaved in the second layer
constexpr int AROWS = ATR / 4;           // rows per wave
static_assert(AH == 64 && AIN <= AXS && AROWS % ARI == 0, "k_ppo_mlp_act's thread layout");

typedef float ActF2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void k_ppo_mlp_act(const SalpPpoMlpAct a, const int first_net) {
    __shared__ __attribute__((aligned(16))) float s_x[ATR * AXS];
    __shared__ __attribute__((aligned(16))) float s_h1[ATR * AH];
    __shared__ float s_h2[ATR * AHS];
    __shared__ float s_wh[3 * AHS];
    __shared__ float s_mean[ATR * 3];

    const int tid = (int)threadIdx.x, j = tid & 63, g = tid >> 6;
    const bool critic = first_net + (int)blockIdx.y != 0;
    const int64_t row0 = (int64_t)blockIdx.x * ATR;
    const int D = a.obs_dim;
    const float* const W1 = critic ? a.params[SALP_MLP_VF_W1] : a.params[SALP_MLP_PI_W1];
    const float* const B1 = critic ? a.params[SALP_MLP_VF_B1] : a.params[SALP_MLP_PI_B1];
    const float* const W2 = critic ? a.params[SALP_MLP_VF_W2] : a.params[SALP_MLP_PI_W2];
    const float* const B2 = critic ? a.params[SALP_MLP_VF_B2] : a.params[SALP_MLP_PI_B2];
    const float* const WH = critic ? a.params[SALP_MLP_VAL_W] : a.params[SALP_MLP_ACT_W];
    const float* const BH = critic ? a.params[SALP_MLP_VAL_B] : a.params[SALP_MLP_ACT_B];
    const int nout = critic ? 1 : 3;

    // the tile's observations (zero beyond obs_dim and beyond the last row) and the head's weights
    for (int i = tid; i < ATR * AXS; i += 256) {
        const int r = i / AXS, k = i % AXS;
        const int64_t row = row0 + r;
        s_x[i] = (k < D && row < a.rows) ? a.obs[row * D + k] : 0.0f;
    }
    if (tid < nout * AH) s_wh[(tid >> 6) * AHS + j] = WH[tid];
    // this unit's weights
    float w1[AIN], w2[AH];
#pragma unroll
    for (int k = 0; k < AIN; ++k) w1[k] = k < D ? W1[j * D + k] : 0.0f;
#pragma unroll
    for (int k = 0; k < AH; ++k) w2[k] = W2[j * AH + k];
    const float b1 = B1[j], b2 = B2[j];
    __syncthreads();

    // first layer
#pragma unroll 4
    for (int rr = 0; rr < AROWS; ++rr) {
        const int r = g * AROWS + rr;
        const float4* const xp = reinterpret_cast<const float4*>(s_x + r * AXS);
        const float4 x0 = xp[0], x1 = xp[1], x2 = xp[2], x3 = xp[3];
        const float x[AXS] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w,
                              x2.x, x2.y, x2.z, x2.w, x3.x, x3.y, x3.z, x3.w};
        float acc = b1;
#pragma unroll
        for (int k = 0; k < AIN; ++k) acc = fmaf(w1[k], x[k], acc);
        s_h1[r * AH + j] = salp_tanhf(acc);
    }
    __syncthreads();

    // second layer: even and odd inputs in the two halves of a packed sum
#pragma unroll 1
    for (int rb = 0; rb < AROWS; rb += ARI) {
        const float* const h1 = s_h1 + (g * AROWS + rb) * AH;
        ActF2 acc[ARI];
#pragma unroll
        for (int i = 0; i < ARI; ++i) acc[i] = ActF2{b2, 0.0f};
#pragma unroll
        for (int k = 0; k < AH; k += 4) {
#pragma unroll
            for (int i = 0; i < ARI; ++i) {
                const float4 h = *reinterpret_cast<const float4*>(h1 + i * AH + k);
                acc[i] = __builtin_elementwise_fma(ActF2{w2[k], w2[k + 1]}, ActF2{h.x, h.y}, acc[i]);
                acc[i] = __builtin_elementwise_fma(ActF2{w2[k + 2], w2[k + 3]}, ActF2{h.z, h.w}, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < ARI; ++i) s_h2[(g * AROWS + rb + i) * AHS + j] = salp_tanhf(acc[i].x + acc[i].y);
    }
    __syncthreads();

    // heads: thread (row j, output g)
    const int64_t row = row0 + j;
    if (g < nout) {
        float out = 0.0f;
#pragma unroll 8
        for (int k = 0; k < AH; ++k) out = fmaf(s_wh[g * AHS + k], s_h2[j * AHS + k], out);
        out += BH[g];
        if (critic) {
            if (row < a.rows) a.value[row] = out;
        } else {
            s_mean[j * 3 + g] = out;
        }
    }
    if (critic) return;   // (uniform over the workgroup)
    __syncthreads();
    if (g != 0 || row >= a.rows) return;
    const float* const log_std = a.params[SALP_MLP_LOG_STD];
    float lp = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float mean = s_mean[j * 3 + c];
        const float sd = expf(log_std[c]);
        const float act = a.eps ? mean + sd * a.eps[row * 3 + c] : mean;
        const float d = act - mean;
        lp += -(d * d) / (2.0f * (sd * sd)) - logf(sd) - 0.91893853320467274f;
        a.action[row * 3 + c] = act;
    }
    if (a.log_prob) a.log_prob[row] = lp;
}

}  // namespace

extern "C" {

int salp_ppo_mlp_act(const SalpPpoMlpAct* a, void* stream) {
    const char* const me = "salp_ppo_mlp_act: ";
    if (!a) return fail(SALP_EINVAL, std::string(me) + "null argument");
    if (a->rows < 0 || a->rows > (int64_t)INT32_MAX * ATR)
        return fail(SALP_EINVAL, std::string(me) + "rows must be in 0 .. 64 (2^31 - 1)");
    if (a->obs_dim < 1 || a->obs_dim > SALP_OBS_DIM_MAX)
        return fail(SALP_EINVAL, std::string(me) + "obs_dim must be in 1 .. " + std::to_string(SALP_OBS_DIM_MAX));
    if (!a->obs) return fail(SALP_EINVAL, std::string(me) + "null obs");
    const bool actor = a->action != nullptr, critic = a->value != nullptr;
    if (!actor && !critic)
        return fail(SALP_EINVAL, std::string(me) + "both networks are absent (action and value are NULL)");
    if (!actor && (a->log_prob || a->eps))
        return fail(SALP_EINVAL, std::string(me) + "log_prob and eps need the actor network (action is NULL)");
    if (actor)
        for (int t = SALP_MLP_PI_W1; t <= SALP_MLP_LOG_STD; ++t)
            if (!a->params[t])
                return fail(SALP_EINVAL, std::string(me) + "the actor needs params[" + std::to_string(t) + "] (NULL)");
    if (critic)
        for (int t = SALP_MLP_VF_W1; t <= SALP_MLP_VAL_B; ++t)
            if (!a->params[t])
                return fail(SALP_EINVAL, std::string(me) + "the critic needs params[" + std::to_string(t) + "] (NULL)");
    if (a->rows == 0) return SALP_OK;
    const unsigned tiles = (unsigned)((a->rows + ATR - 1) / ATR);
    hipLaunchKernelGGL(k_ppo_mlp_act, dim3(tiles, (unsigned)actor + (unsigned)critic), dim3(256), 0,
                       (hipStream_t)stream, *a, actor ? 0 : 1);
    return check_hip(hipGetLastError(), "k_ppo_mlp_act");
}

}  // extern "C"
