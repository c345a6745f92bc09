// salp_lstm.hip — the LSTM cell of RecurrentPPO's MlpLstmPolicy (gfx950).
//
// What it replaces: the elementwise part of one torch.nn.LSTM step (gates
// i, f, g, o in torch's order; c' = f c + i g, h' = o tanh(c')), with
// sb3-contrib's episode-start reset folded in (c is multiplied by keep =
// 1 - episode_start before the step, as sb3-contrib's _process_sequence
// zeroes the state), and its backward.  The gate pre-activations
// G = x W_ih^T + b + (h keep) W_hh^T stay library GEMMs (grasp_lab_salp_amd/
// recurrent_ppo.py); what these kernels fuse is the ~8 elementwise torch
// kernels of a step forward and ~12 backward, which at 2 048 sequences x 16
// steps x 2 LSTMs made RecurrentPPO's update launch-bound.
//
// One thread per (row, unit): the four gate columns of a row are H apart, so
// each gate's loads are coalesced across the wave.  float32 like torch.
//
// salp_lstm_policy_step (further down) is the whole policy step of the
// collection, of evaluate and of predict in two launches: there the gate
// products run in the kernel too, on the f32 matrix cores.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "salp_host.h"

using salp::check_hip;
using salp::fail;

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// One cell from the gate pre-activations (i, f, g, o) and ck = c_prev keep: the
// arithmetic k_lstm_fwd and k_lstm_policy_cell share, so that the update's pass
// over a stored sequence recomputes what the collection's step computed.
struct Cell {
    float ig, fg, gg, og, cn, hn;
};
__device__ __forceinline__ Cell lstm_cell(float gi, float gf, float gc, float go, float ck) {
    Cell o;
    o.ig = sigm(gi);
    o.fg = sigm(gf);
    o.gg = tanhf(gc);
    o.og = sigm(go);
    o.cn = o.fg * ck + o.ig * o.gg;
    o.hn = o.og * tanhf(o.cn);
    return o;
}

// act [m][4H]: the activated gates (i, f, g, o) for the backward pass
// Sequence steps (salp_lstm_step_forward): GX (the input projection, or null)
// is added to G here instead of by a copy before the GEMM, and hk = h keep_next
// (the next step's GEMM operand, when keep_next is not null) is written too.
__global__ __launch_bounds__(256) void k_lstm_fwd(int64_t m, int H, const float* __restrict__ G,
                                                  const float* __restrict__ GX,
                                                  const float* __restrict__ c_prev, const float* __restrict__ keep,
                                                  const float* __restrict__ keep_next,
                                                  float* __restrict__ h, float* __restrict__ c,
                                                  float* __restrict__ act, float* __restrict__ hk) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * H) return;
    const int64_t r = e / H;
    const int u = (int)(e - r * H);
    const float* g = G + r * 4 * H;
    float gi = g[u], gf = g[H + u], gc = g[2 * H + u], go = g[3 * H + u];
    if (GX) {
        const float* x = GX + r * 4 * H;
        gi = x[u] + gi;
        gf = x[H + u] + gf;
        gc = x[2 * H + u] + gc;
        go = x[3 * H + u] + go;
    }
    const Cell o = lstm_cell(gi, gf, gc, go, c_prev[e] * keep[r]);
    c[e] = o.cn;
    h[e] = o.hn;
    if (keep_next) hk[e] = o.hn * keep_next[r];
    float* a = act + r * 4 * H;
    a[u] = o.ig;
    a[H + u] = o.fg;
    a[2 * H + u] = o.gg;
    a[3 * H + u] = o.og;
}

// dh, dc: gradients of the step's h and c outputs (dc may be null: zero);
// dG [m][4H] the gate pre-activations' gradient, dc_prev [m][H] c_prev's
// Sequence steps (salp_lstm_step_backward): dh = d_out + dhk_next keep_next
// (the gradient through the next step's GEMM operand, when dhk_next is not null).
__global__ __launch_bounds__(256) void k_lstm_bwd(int64_t m, int H, const float* __restrict__ act,
                                                  const float* __restrict__ c_prev, const float* __restrict__ keep,
                                                  const float* __restrict__ c, const float* __restrict__ dh,
                                                  const float* __restrict__ dhk_next,
                                                  const float* __restrict__ keep_next,
                                                  const float* __restrict__ dc, float* __restrict__ dG,
                                                  float* __restrict__ dc_prev) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * H) return;
    const int64_t r = e / H;
    const int u = (int)(e - r * H);
    const float* a = act + r * 4 * H;
    const float ig = a[u], fg = a[H + u], gg = a[2 * H + u], og = a[3 * H + u];
    const float kp = keep[r];
    const float ck = c_prev[e] * kp;
    const float tc = tanhf(c[e]);
    const float dhe = dhk_next ? dh[e] + dhk_next[e] * keep_next[r] : dh[e];
    const float dcn = (dc ? dc[e] : 0.0f) + dhe * og * (1.0f - tc * tc);
    float* d = dG + r * 4 * H;
    d[u] = dcn * gg * ig * (1.0f - ig);
    d[H + u] = dcn * ck * fg * (1.0f - fg);
    d[2 * H + u] = dcn * ig * (1.0f - gg * gg);
    d[3 * H + u] = dhe * tc * og * (1.0f - og);
    dc_prev[e] = dcn * fg * kp;
}

// The cell and the sequence step share a kernel: the cell is the step without GX, keep_next and hk.
int launch_fwd(int64_t m, int H, const float* G, const float* GX, const float* c_prev, const float* keep,
               const float* keep_next, float* h, float* c, float* act, float* hk, void* stream) {
    const int64_t n = m * H;
    hipLaunchKernelGGL(k_lstm_fwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, H, G, GX,
                       c_prev, keep, keep_next, h, c, act, hk);
    return check_hip(hipGetLastError(), "k_lstm_fwd");
}

int launch_bwd(int64_t m, int H, const float* act, const float* c_prev, const float* keep, const float* c,
               const float* dh, const float* dhk_next, const float* keep_next, const float* dc, float* dG,
               float* dc_prev, void* stream) {
    const int64_t n = m * H;
    hipLaunchKernelGGL(k_lstm_bwd, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, m, H,
                       act, c_prev, keep, c, dh, dhk_next, keep_next, dc, dG, dc_prev);
    return check_hip(hipGetLastError(), "k_lstm_bwd");
}

// ------------------------------------------------------------------------
// salp_lstm_policy_step: one step of the whole recurrent policy in two launches.
//
//   k_lstm_policy_cell  grid (8 groups of 32 units, networks, row splits), four
//                       waves: wave g owns gate g of the block's 32 units.  A lane
//                       keeps its B operand W[gate][unit lc][k] in 140 registers
//                       for the block's whole life: the 256 recurrent columns,
//                       then W_ih's obs_dim columns, then b_ih + b_hh against a
//                       column of ones, zeros up to K = 280.  Per tile of 32 rows:
//                       [hk | x | 1 | 0] is staged in LDS, 140 MFMAs per wave
//                       (v_mfma_f32_32x32x2_f32, chunk q of 8 columns into
//                       accumulator q & 3: no chain longer than 36 terms), the
//                       four gate tiles meet in LDS, the cell runs on the VALU.
//   k_lstm_policy_head  grid (tiles of 32 rows, networks): 256 -> 64 -> 64 tanh
//                       MLP (thread: one unit, eight rows, four interleaved
//                       chains each), the head, the Gaussian.
constexpr int PH = SALP_LSTM_POLICY_HIDDEN;
constexpr int PM = SALP_LSTM_POLICY_MLP;
constexpr int PXK = 24;                 // columns after the recurrent ones: x (<= 16), the ones column, zeros
constexpr int PKT = PH + PXK;           // K of the gate product
constexpr int PKS = PKT + 4;            // LDS row stride: rows 16-B aligned, 16 rows on 16 different 16-B slots
constexpr int PNQ = PKT / 8;            // chunks of 8 columns: a float4 per lane half
constexpr int PTR = 32;                 // rows per tile: one MFMA tile high
constexpr int PSPLIT = 32;              // row splits of the cell kernel at most
constexpr int PMS = PM + 4;             // LDS row stride of the 64-wide tiles
static_assert(SALP_LSTM_POLICY_OBS_MAX + 1 <= PXK && PKT % 8 == 0, "x and the ones column fit the padded K");
static_assert(PM == 64 && PH % PM == 0, "the head's thread layout");

typedef float f32x16 __attribute__((ext_vector_type(16)));
// row of accumulator register r of a 32x32 result, lane half h (the column is the lane & 31)
__device__ __forceinline__ int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__global__ __launch_bounds__(256) void k_lstm_policy_cell(SalpLstmPolicyStep a, int net0, int64_t tiles) {
    const int tid = threadIdx.x, ug = blockIdx.x, net = net0 + blockIdx.y;
    const SalpLstmPolicyNet n = net ? a.critic : a.actor;
    const int64_t rows = a.rows;
    const int od = a.obs_dim;
    const int w = tid >> 6, l = tid & 63, lc = l & 31, lh = l >> 5;
    __shared__ __attribute__((aligned(16))) float sA[PTR][PKS];
    __shared__ float sG[4][PTR][PTR + 1];

    // B operand: row `wrow` of the stacked weights, columns 8 q + 4 lh + e
    const int wrow = w * PH + PTR * ug + lc;
    float wreg[4 * PNQ];
#pragma unroll
    for (int q = 0; q < PH / 8; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(n.weight_hh + (int64_t)wrow * PH + 8 * q + 4 * lh);
        wreg[4 * q] = v.x;
        wreg[4 * q + 1] = v.y;
        wreg[4 * q + 2] = v.z;
        wreg[4 * q + 3] = v.w;
    }
    const float bias = n.bias_ih[wrow] + n.bias_hh[wrow];
#pragma unroll
    for (int q = PH / 8; q < PNQ; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int kx = 8 * q + 4 * lh + e - PH;
            wreg[4 * q + e] = kx < od ? n.weight_ih[(int64_t)wrow * od + kx] : (kx == od ? bias : 0.0f);
        }

    const float* const h_in = a.state_in + (int64_t)(2 * net) * rows * PH;
    const float* const c_in = h_in + rows * PH;
    float* const h_out = a.state_out ? a.state_out + (int64_t)(2 * net) * rows * PH : a.latent + (int64_t)net * rows * PH;
    float* const c_out = a.state_out ? a.state_out + (int64_t)(2 * net + 1) * rows * PH : nullptr;

    for (int64_t t = blockIdx.z; t < tiles; t += gridDim.z) {
        const int64_t row0 = t * PTR;
        // ---- [hk | x | 1 | 0] of the tile; rows >= rows are zero
        for (int e = tid; e < PTR * PKT; e += 256) {
            const int r = e / PKT, k = e - r * PKT;
            const int64_t row = row0 + r;
            float v = 0.0f;
            if (row < rows) {
                if (k < PH) v = h_in[row * PH + k] * (a.keep ? a.keep[row] : 1.0f);
                else if (k < PH + od) v = a.obs[row * od + (k - PH)];
                else if (k == PH + od) v = 1.0f;
            }
            sA[r][k] = v;
        }
        __syncthreads();   // (every wave is past the cell of the tile before: it read sG)
        // ---- this wave's gate of the block's units: lane A = [hk | x | 1][row lc][k], B = wreg
        f32x16 acc[4] = {};
#pragma unroll
        for (int q = 0; q < PNQ; ++q) {
            const float4 x = *reinterpret_cast<const float4*>(&sA[lc][8 * q + 4 * lh]);
            acc[q & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.x, wreg[4 * q], acc[q & 3], 0, 0, 0);
            acc[q & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.y, wreg[4 * q + 1], acc[q & 3], 0, 0, 0);
            acc[q & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.z, wreg[4 * q + 2], acc[q & 3], 0, 0, 0);
            acc[q & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(x.w, wreg[4 * q + 3], acc[q & 3], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) sG[w][crow(r, lh)][lc] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
        __syncthreads();   // the gates are there; every read of sA is done
        // ---- the cell: thread (unit tid & 31, rows tid >> 5, + 8, ...)
        const int u = tid & 31;
#pragma unroll
        for (int i = 0; i < PTR / 8; ++i) {
            const int r = (tid >> 5) + 8 * i;
            const int64_t row = row0 + r;
            if (row < rows) {
                const int64_t e = row * PH + PTR * ug + u;
                const Cell o = lstm_cell(sG[0][r][u], sG[1][r][u], sG[2][r][u], sG[3][r][u],
                                         c_in[e] * (a.keep ? a.keep[row] : 1.0f));
                h_out[e] = o.hn;
                if (c_out) c_out[e] = o.cn;
            }
        }
    }
}

// One tanh layer of the head kernel: out[r][j] = tanh(in[r][:] W[j][:] + b[j]) for the tile's 32 rows.
// W [64][K] comes through LDS in chunks of 64 columns.  Opens with a barrier (the input is written,
// the readers of sW are done) and leaves without one.
template <int K>
__device__ __forceinline__ void policy_mlp_layer(const float* sIn, int in_stride, float (*sW)[PMS],
                                                 const float* __restrict__ W, const float* __restrict__ b,
                                                 float* sOut, int out_stride, int tid) {
    const int j = tid & 63, rg = tid >> 6;
    float acc[8][4];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][e] = 0.0f;
    for (int c = 0; c < K / PM; ++c) {
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = (tid >> 4) + 16 * i, col = (tid & 15) * 4;
            *reinterpret_cast<float4*>(&sW[row][col]) =
                *reinterpret_cast<const float4*>(W + (int64_t)row * K + c * PM + col);
        }
        __syncthreads();
#pragma unroll 4
        for (int k4 = 0; k4 < PM / 4; ++k4) {
            const float4 wv = *reinterpret_cast<const float4*>(&sW[j][4 * k4]);
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                const float4 x = *reinterpret_cast<const float4*>(&sIn[(rg * 8 + r) * in_stride + c * PM + 4 * k4]);
                acc[r][0] = fmaf(x.x, wv.x, acc[r][0]);
                acc[r][1] = fmaf(x.y, wv.y, acc[r][1]);
                acc[r][2] = fmaf(x.z, wv.z, acc[r][2]);
                acc[r][3] = fmaf(x.w, wv.w, acc[r][3]);
            }
        }
    }
    const float bias = b[j];
#pragma unroll
    for (int r = 0; r < 8; ++r)
        sOut[(rg * 8 + r) * out_stride + j] = tanhf(((acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3])) + bias);
}

__global__ __launch_bounds__(256) void k_lstm_policy_head(SalpLstmPolicyStep a, int net0) {
    const int tid = threadIdx.x, net = net0 + blockIdx.y;
    const SalpLstmPolicyNet n = net ? a.critic : a.actor;
    const int64_t rows = a.rows, row0 = (int64_t)blockIdx.x * PTR;
    const float* const h = a.state_out ? a.state_out + (int64_t)(2 * net) * rows * PH
                                       : a.latent + (int64_t)net * rows * PH;
    __shared__ __attribute__((aligned(16))) float sH[PTR][PH + 4];   // h', then the second layer's output
    __shared__ __attribute__((aligned(16))) float sW[PM][PMS];
    __shared__ __attribute__((aligned(16))) float sM[PTR][PMS];      // the first layer's output
    for (int e = tid; e < PTR * (PH / 4); e += 256) {
        const int r = e / (PH / 4), k = 4 * (e % (PH / 4));
        float4 v = {0.0f, 0.0f, 0.0f, 0.0f};
        if (row0 + r < rows) v = *reinterpret_cast<const float4*>(h + (row0 + r) * PH + k);
        *reinterpret_cast<float4*>(&sH[r][k]) = v;
    }
    policy_mlp_layer<PH>(&sH[0][0], PH + 4, sW, n.mlp_w1, n.mlp_b1, &sM[0][0], PMS, tid);
    policy_mlp_layer<PM>(&sM[0][0], PMS, sW, n.mlp_w2, n.mlp_b2, &sH[0][0], PH + 4, tid);
    __syncthreads();
    // ---- head: 8 threads per row, units p, p + 8, ... each, then a xor tree
    const int r = tid >> 3, p = tid & 7, nout = net ? 1 : SALP_LSTM_POLICY_ACT_DIM;
    float s[SALP_LSTM_POLICY_ACT_DIM] = {0.0f, 0.0f, 0.0f};
    for (int q = 0; q < PM / 8; ++q) {
        const int u = p + 8 * q;
        const float x = sH[r][u];
#pragma unroll
        for (int o = 0; o < SALP_LSTM_POLICY_ACT_DIM; ++o)
            if (o < nout) s[o] = fmaf(x, n.head_w[o * PM + u], s[o]);
    }
    for (int x = 1; x < 8; x <<= 1)
#pragma unroll
        for (int o = 0; o < SALP_LSTM_POLICY_ACT_DIM; ++o) s[o] += __shfl_xor(s[o], x, 64);
    const int64_t row = row0 + r;
    if (p != 0 || row >= rows) return;
    if (net) {
        a.value[row] = s[0] + n.head_b[0];
        return;
    }
    // torch.distributions.Normal(mean, exp(log_std)): a = mean + std eps, log_prob summed over the action
    float lp = 0.0f;
#pragma unroll
    for (int o = 0; o < SALP_LSTM_POLICY_ACT_DIM; ++o) {
        const float mean = s[o] + n.head_b[o];
        const float sd = expf(a.log_std[o]);
        const float act = a.eps ? mean + sd * a.eps[row * SALP_LSTM_POLICY_ACT_DIM + o] : mean;
        const float d = act - mean;
        lp += -(d * d) / (2.0f * (sd * sd)) - logf(sd) - 0.91893853320467274178f;
        if (a.action) a.action[row * SALP_LSTM_POLICY_ACT_DIM + o] = act;
    }
    if (a.log_prob) a.log_prob[row] = lp;
}

// a network is absent (every pointer NULL), whole, or given in part (an error)
enum NetState { NET_ABSENT, NET_WHOLE, NET_PARTIAL };
NetState net_state(const SalpLstmPolicyNet& n) {
    const float* const p[10] = {n.weight_ih, n.weight_hh, n.bias_ih, n.bias_hh, n.mlp_w1,
                                n.mlp_b1,    n.mlp_w2,    n.mlp_b2,  n.head_w,  n.head_b};
    int set = 0;
    for (const float* q : p) set += q != nullptr;
    return set == 0 ? NET_ABSENT : (set == 10 ? NET_WHOLE : NET_PARTIAL);
}
bool aligned16(const SalpLstmPolicyNet& n) {
    return ((uintptr_t)n.weight_hh | (uintptr_t)n.mlp_w1 | (uintptr_t)n.mlp_w2) % 16 == 0;
}

}  // namespace

extern "C" {

int salp_lstm_policy_step(const SalpLstmPolicyStep* s, void* stream) {
    const char* const me = "salp_lstm_policy_step: ";
    if (!s) return fail(SALP_EINVAL, std::string(me) + "null argument");
    if (s->rows < 0 || s->rows > INT32_MAX) return fail(SALP_EINVAL, std::string(me) + "rows must be in 0 .. 2^31 - 1");
    if (s->obs_dim < 1 || s->obs_dim > SALP_LSTM_POLICY_OBS_MAX || s->act_dim != SALP_LSTM_POLICY_ACT_DIM)
        return fail(SALP_EINVAL, std::string(me) + "obs_dim must be in 1 .. 16 and act_dim 3");
    const NetState sa = net_state(s->actor), sc = net_state(s->critic);
    if (sa == NET_PARTIAL || sc == NET_PARTIAL)
        return fail(SALP_EINVAL, std::string(me) + "a network has all its pointers or none (NULL parameter)");
    if (sa == NET_ABSENT && sc == NET_ABSENT) return fail(SALP_EINVAL, std::string(me) + "both networks are absent");
    const bool actor = sa == NET_WHOLE, critic = sc == NET_WHOLE;
    if ((actor && !aligned16(s->actor)) || (critic && !aligned16(s->critic)))
        return fail(SALP_EINVAL, std::string(me) + "weight_hh, mlp_w1 and mlp_w2 must be 16-byte aligned");
    if (!s->obs || !s->state_in) return fail(SALP_EINVAL, std::string(me) + "null obs or state_in");
    if (!s->state_out && !s->latent)
        return fail(SALP_EINVAL, std::string(me) + "state_out is NULL: latent must hold h between the launches");
    if (!actor && (s->action || s->log_prob))
        return fail(SALP_EINVAL, std::string(me) + "action / log_prob need the actor network");
    if (!critic && s->value) return fail(SALP_EINVAL, std::string(me) + "value needs the critic network");
    const bool actor_head = actor && (s->action || s->log_prob), critic_head = critic && s->value;
    if (actor_head && !s->log_std) return fail(SALP_EINVAL, std::string(me) + "null log_std");
    if (!s->state_out && !actor_head && !critic_head)
        return fail(SALP_EINVAL, std::string(me) + "nothing to compute: no state_out and no output");
    if (s->state_out) {
        const uintptr_t bytes = (uintptr_t)4 * (uintptr_t)s->rows * PH * sizeof(float);
        const uintptr_t i0 = (uintptr_t)s->state_in, o0 = (uintptr_t)s->state_out;
        if (s->rows > 0 ? (i0 < o0 + bytes && o0 < i0 + bytes) : i0 == o0)
            return fail(SALP_EINVAL, std::string(me) + "state_out overlaps state_in: the step is not in place");
    }
    if (s->rows == 0) return SALP_OK;
    hipStream_t st = (hipStream_t)stream;
    const int64_t tiles = (s->rows + PTR - 1) / PTR;
    const unsigned splits = (unsigned)(tiles < PSPLIT ? tiles : PSPLIT);
    hipLaunchKernelGGL(k_lstm_policy_cell, dim3(PH / PTR, (unsigned)actor + (unsigned)critic, splits), dim3(256), 0, st,
                       *s, actor ? 0 : 1, tiles);
    // the heads are not enqueued behind a cell that did not launch
    if (const int rc = check_hip(hipGetLastError(), "k_lstm_policy_cell")) return rc;
    if (!actor_head && !critic_head) return SALP_OK;
    hipLaunchKernelGGL(k_lstm_policy_head, dim3((unsigned)tiles, (unsigned)actor_head + (unsigned)critic_head),
                       dim3(256), 0, st, *s, actor_head ? 0 : 1);
    return check_hip(hipGetLastError(), "k_lstm_policy_head");
}

int salp_lstm_cell_forward(int64_t rows, int32_t hidden, const float* gates, const float* c_prev, const float* keep,
                           float* h, float* c, float* act, void* stream) {
    if (rows < 0 || hidden <= 0) return fail(SALP_EINVAL, "salp_lstm_cell_forward: bad size");
    if (!gates || !c_prev || !keep || !h || !c || !act)
        return fail(SALP_EINVAL, "salp_lstm_cell_forward: null buffer");
    if (rows == 0) return SALP_OK;
    return launch_fwd(rows, hidden, gates, nullptr, c_prev, keep, nullptr, h, c, act, nullptr, stream);
}

int salp_lstm_step_forward(int64_t rows, int32_t hidden, const float* gates, const float* gx, const float* c_prev,
                           const float* keep, const float* keep_next, float* h, float* c, float* act, float* hk_next,
                           void* stream) {
    if (rows < 0 || hidden <= 0) return fail(SALP_EINVAL, "salp_lstm_step_forward: bad size");
    if (!gates || !c_prev || !keep || !h || !c || !act)
        return fail(SALP_EINVAL, "salp_lstm_step_forward: null buffer");
    if (!keep_next != !hk_next)
        return fail(SALP_EINVAL, "salp_lstm_step_forward: keep_next and hk_next go together");
    if (rows == 0) return SALP_OK;
    return launch_fwd(rows, hidden, gates, gx, c_prev, keep, keep_next, h, c, act, hk_next, stream);
}

int salp_lstm_cell_backward(int64_t rows, int32_t hidden, const float* act, const float* c_prev, const float* keep,
                            const float* c, const float* dh, const float* dc, float* dgates, float* dc_prev,
                            void* stream) {
    if (rows < 0 || hidden <= 0) return fail(SALP_EINVAL, "salp_lstm_cell_backward: bad size");
    if (!act || !c_prev || !keep || !c || !dh || !dgates || !dc_prev)
        return fail(SALP_EINVAL, "salp_lstm_cell_backward: null buffer");
    if (rows == 0) return SALP_OK;
    return launch_bwd(rows, hidden, act, c_prev, keep, c, dh, nullptr, nullptr, dc, dgates, dc_prev, stream);
}

int salp_lstm_step_backward(int64_t rows, int32_t hidden, const float* act, const float* c_prev, const float* keep,
                            const float* c, const float* d_out, const float* dhk_next, const float* keep_next,
                            const float* dc, float* dgates, float* dc_prev, void* stream) {
    if (rows < 0 || hidden <= 0) return fail(SALP_EINVAL, "salp_lstm_step_backward: bad size");
    if (!act || !c_prev || !keep || !c || !d_out || !dgates || !dc_prev)
        return fail(SALP_EINVAL, "salp_lstm_step_backward: null buffer");
    if (!dhk_next != !keep_next)
        return fail(SALP_EINVAL, "salp_lstm_step_backward: dhk_next and keep_next go together");
    if (rows == 0) return SALP_OK;
    return launch_bwd(rows, hidden, act, c_prev, keep, c, d_out, dhk_next, keep_next, dc, dgates, dc_prev, stream);
}

}  // extern "C"
