// salp_sac_mlp.hip — SAC's 256-256 ReLU networks, forward and backward (gfx950).
//
// What it replaces: the torch.nn.Linear / ReLU chains of stable_baselines3's
// SAC MlpPolicy (actor: obs -> 256 -> 256 -> (mu, log_std); each critic:
// cat(obs, action) -> 256 -> 256 -> 1) as grasp_lab_salp_amd/sac.py ran them
// through torch: addmm, relu, threshold_backward, cat and bias-sum launches,
// eleven network evaluations per gradient step.  Here a pass over up to four
// networks of one shape is one launch each way (include/salp.h "SAC"):
//
//   k_sac_net_fwd     blockIdx.y = network, blockIdx.x = tile of 32 rows.
//                     Layer 1 (K <= 17) and the head (out <= 6) on the VALU,
//                     layer 2 on v_mfma_f32_32x32x2_f32: wave w owns hidden
//                     units 32 w .. 32 w + 31 of the tile, W2 streams through
//                     LDS in chunks of 32 input columns
//   k_sac_net_bwd     blockIdx.y = network; at most 64 row blocks of four
//                     waves, block bx takes tiles bx, bx + blocks, ...: dz2,
//                     the weight gradient dz2^T h1 (wave w owns rows 64 w .. of
//                     dW2: sixteen 32 x 32 accumulator tiles, kept over the
//                     block's tiles), dz1 = (dz2 W2)(h1 > 0) with W2 streamed
//                     in chunks of 16 rows, then dW1, the bias sums (fp64) and
//                     the action columns of dz1 W1.  A block writes one float32
//                     partial per parameter; <WG = false> computes no weight
//                     gradient
//   k_sac_net_reduce  the partials summed in fp64 in block order into the
//                     flat gradients, and dx1 over the networks in index order
//
// The matrix-core products are exact f32: one fmaf chain per output in the
// order its k arrive.  K = 256 is split over independent accumulators (four
// forward, two backward) that are added at the end, so no chain is longer than
// 128 terms.  No floating-point atomics.  Everything is enqueued on the
// caller's stream; nothing allocates or synchronises.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/salp.h"
#include "salp_host.h"

using salp::check_hip;
using salp::fail;

namespace {

constexpr int H = SALP_SAC_HIDDEN;          // hidden units per layer
constexpr int KP = SALP_SAC_NET_IN_MAX;     // input columns in LDS; columns >= in_dim are zero (odd: no bank conflicts)
constexpr int OM = SALP_SAC_NET_OUT_MAX;    // head rows in LDS; rows >= out_dim are zero
constexpr int TR = 32;                      // rows per tile: one MFMA tile high
constexpr int NT = 512;                     // threads per block of the forward: 8 waves, one per 32 hidden units
constexpr int MAXB = 64;                    // row blocks of the backward per network at most
constexpr int HS = H + 4;                   // LDS row stride: rows 16-B aligned, 16 rows on 16 different 16-B slots
constexpr int KC = 32;                      // W2 columns per LDS chunk of the forward
constexpr int NCH = H / KC;                 // chunks
constexpr int CS = KC + 4;                  // row stride of the forward's chunk
constexpr int NPRE = H * KC / NT;           // chunk elements per thread
static_assert(H == 32 * (NT / 64), "one wave per 32 hidden units");
static_assert(NT == 2 * H && TR == 32, "a thread takes one unit and half the tile's rows");
static_assert(NT == TR * 16, "16 threads per row in the head");
static_assert(NPRE * NT == H * KC, "whole staging rounds");

typedef float f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ f32x16 mfma32(float a, float b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of accumulator register r of a 32x32 result, lane half h (the column is the lane & 31)
__device__ __forceinline__ int crow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// torch's relu: NaN stays NaN
__device__ __forceinline__ float relu(float s) { return s <= 0.0f ? 0.0f : s; }

struct Net {
    const float *W1, *b1, *W2, *b2, *W3, *b3;
};
__device__ __forceinline__ Net net_of(const float* p, int in, int od) {
    Net n;
    n.W1 = p;
    n.b1 = n.W1 + H * in;
    n.W2 = n.b1 + H;
    n.b2 = n.W2 + H * H;
    n.W3 = n.b2 + H;
    n.b3 = n.W3 + od * H;
    return n;
}
__host__ __device__ inline int64_t num_params(int in, int od) {
    return (int64_t)H * in + H + (int64_t)H * H + H + (int64_t)od * H + od;
}

// the tile's input rows, [TR][KP]: x0's d0 columns, x1's d1 columns, zeros; rows >= B are zero
__device__ __forceinline__ void stage_x(float (*sX)[KP], const float* x0, const float* x1, int d0, int d1,
                                        int64_t row0, int64_t B) {
    for (int e = threadIdx.x; e < TR * KP; e += NT) {
        const int r = e / KP, k = e % KP;
        const int64_t row = row0 + r;
        float v = 0.0f;
        if (row < B) {
            if (k < d0) v = x0[row * d0 + k];
            else if (k < d0 + d1) v = x1[row * d1 + (k - d0)];
        }
        sX[r][k] = v;
    }
}

__global__ __launch_bounds__(NT) void k_sac_net_fwd(SalpSacNetForward a) {
    const int net = blockIdx.y, tid = threadIdx.x;
    const int d0 = a.d0, d1 = a.d1, in = d0 + d1, od = a.out_dim;
    const int64_t B = a.batch, row0 = (int64_t)blockIdx.x * TR;
    const Net n = net_of(a.params[net], in, od);
    float* const h1g = a.h1[net];
    float* const h2g = a.h2[net];
    __shared__ float sX[TR][KP];
    __shared__ __attribute__((aligned(16))) float sH[TR][HS];   // h1, then h2
    __shared__ __attribute__((aligned(16))) float sW[H][CS];    // W2[unit][32 c + k] of chunk c
    __shared__ float sW3[OM][H];

    // the first chunk of W2 is in flight while layer 1 runs
    float pre[NPRE];
#pragma unroll
    for (int q = 0; q < NPRE; ++q) {
        const int e = tid + q * NT;
        pre[q] = n.W2[(e / KC) * H + e % KC];
    }
    stage_x(sX, a.x0[net], a.x1[net], d0, d1, row0, B);
    for (int e = tid; e < OM * H; e += NT) sW3[e / H][e % H] = e < od * H ? n.W3[e] : 0.0f;
    const int j = tid % H, rg = tid / H;
    float w1[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) w1[k] = k < in ? n.W1[j * in + k] : 0.0f;
    const float bias1 = n.b1[j];
    __syncthreads();
    // ---- layer 1: h1 = relu(x W1^T + b1); thread (unit j, row half rg)
    for (int rr = 0; rr < TR / 2; ++rr) {
        const int r = rg * (TR / 2) + rr;
        float s = bias1;
#pragma unroll
        for (int k = 0; k < KP; ++k) s = fmaf(sX[r][k], w1[k], s);
        s = relu(s);
        sH[r][j] = s;
        if (h1g && row0 + r < B) h1g[(row0 + r) * H + j] = s;
    }
    // ---- layer 2: h2 = relu(h1 W2^T + b2); lane: A = h1[row lc][k], B = W2[unit 32 w + lc][k],
    //      k = 32 c + 16 lh + 4 s4 + e; chunk c adds into accumulator c & 3
    const int w = tid / 64, l = tid % 64, lc = l & 31, lh = l >> 5;
    f32x16 acc[4] = {};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        __syncthreads();   // h1 is written (c = 0); every wave is done with the chunk before
#pragma unroll
        for (int q = 0; q < NPRE; ++q) {
            const int e = tid + q * NT;
            sW[e / KC][e % KC] = pre[q];
        }
        __syncthreads();
        if (c + 1 < NCH) {
#pragma unroll
            for (int q = 0; q < NPRE; ++q) {
                const int e = tid + q * NT;
                pre[q] = n.W2[(e / KC) * H + (c + 1) * KC + e % KC];
            }
        }
#pragma unroll
        for (int s4 = 0; s4 < KC / 8; ++s4) {
            const float4 x = *reinterpret_cast<const float4*>(&sH[lc][c * KC + (KC / 2) * lh + 4 * s4]);
            const float4 y = *reinterpret_cast<const float4*>(&sW[32 * w + lc][(KC / 2) * lh + 4 * s4]);
            acc[c & 3] = mfma32(x.x, y.x, acc[c & 3]);
            acc[c & 3] = mfma32(x.y, y.y, acc[c & 3]);
            acc[c & 3] = mfma32(x.z, y.z, acc[c & 3]);
            acc[c & 3] = mfma32(x.w, y.w, acc[c & 3]);
        }
    }
    __syncthreads();   // every read of h1 is done: h2 replaces it
    {
        const float bias2 = n.b2[32 * w + lc];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = crow(r, lh);
            const float v = relu(((acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r])) + bias2);
            sH[row][32 * w + lc] = v;
            if (h2g && row0 + row < B) h2g[(row0 + row) * H + 32 * w + lc] = v;
        }
    }
    __syncthreads();
    // ---- head: out = h2 W3^T + b3; 16 threads per row, units p, p + 16, ... each, then a xor tree
    {
        const int r = tid / 16, p = tid % 16;
        float s[OM];
#pragma unroll
        for (int o = 0; o < OM; ++o) s[o] = 0.0f;
        for (int q = 0; q < H / 16; ++q) {
            const int u = p + 16 * q;
            const float h = sH[r][u];
#pragma unroll
            for (int o = 0; o < OM; ++o) s[o] = fmaf(h, sW3[o][u], s[o]);
        }
        for (int x = 1; x < 16; x <<= 1)
#pragma unroll
            for (int o = 0; o < OM; ++o) s[o] += __shfl_xor(s[o], x, 64);
        if (p == 0 && row0 + r < B) {
            float* const out = a.out[net] + (row0 + r) * od;
#pragma unroll
            for (int o = 0; o < OM; ++o)
                if (o < od) out[o] = s[o] + n.b3[o];
        }
    }
}

// part: [n_nets][nb][P] block partials of the parameter gradients (WG);
// dxp: [n_nets][B][d1] the networks' dx1 (a.dx1 set).  Four waves, so that a
// wave may hold the 16 accumulator tiles of its 64 rows of dW2 (256 registers
// of the 512 a lane has at one wave per SIMD): wave w owns hidden units
// 64 w .. 64 w + 63, thread tid the unit tid on the VALU.
constexpr int NTB = 256;                    // threads per block of the backward
constexpr int KCB = 16;                     // W2 rows per LDS chunk
constexpr int NCHB = H / KCB;
constexpr int NPREB = H * KCB / NTB;        // chunk elements per thread
constexpr int NKB = H / 32;                 // 32-column blocks of a row of dW2
static_assert(NTB == H && H == 64 * (NTB / 64), "a thread per unit, a wave per 64 units");
static_assert(NTB * 2 == TR * 16, "dx1: 16 threads per row, two rows each");

template <bool WG>
__global__ __launch_bounds__(NTB) void k_sac_net_bwd(SalpSacNetBackward a, int64_t tiles, int64_t P, float* part,
                                                     float* dxp) {
    const int net = blockIdx.y, tid = threadIdx.x, nb = gridDim.x;
    const int d0 = a.d0, d1 = a.d1, in = d0 + d1, od = a.out_dim;
    const int64_t B = a.batch;
    const Net n = net_of(a.params[net], in, od);
    const float* const h1g = a.h1[net];
    const float* const h2g = a.h2[net];
    const float* const dog = a.dout[net];
    const bool want_dx = a.dx1 != nullptr;
    __shared__ float sX[TR][KP];
    __shared__ float sDo[TR][OM];                                // dout of the tile; columns >= out_dim zero
    __shared__ __attribute__((aligned(16))) float sH1[TR][HS];
    __shared__ __attribute__((aligned(16))) float sDz[TR][HS];   // dz2, then dz1
    __shared__ float sW[KCB][HS];                                // W2[16 c + row][k] of chunk c
    __shared__ float sW1[H][KP];                                 // W1, columns >= in_dim zero

    const int j = tid;
    const int w = tid / 64, l = tid % 64, lc = l & 31, lh = l >> 5;
    for (int e = tid; e < H * KP; e += NTB) sW1[e / KP][e % KP] = e % KP < in ? n.W1[(e / KP) * in + e % KP] : 0.0f;
    float w3[OM];
#pragma unroll
    for (int o = 0; o < OM; ++o) w3[o] = o < od ? n.W3[o * H + j] : 0.0f;
    // gradient accumulators, kept over the block's tiles
    f32x16 gW2[WG ? 2 : 1][WG ? NKB : 1] = {};   // dW2[64 w + 32 jb + crow(r, lh)][32 kb + lc]
    float gW1[KP], gW3[OM];                    // unit j
    double gB1 = 0.0, gB2 = 0.0, gB3 = 0.0;    // the bias sums have no products: fp64, rounded once (gB3: tid < out_dim)
#pragma unroll
    for (int k = 0; k < KP; ++k) gW1[k] = 0.0f;
#pragma unroll
    for (int o = 0; o < OM; ++o) gW3[o] = 0.0f;

    for (int64_t t = blockIdx.x; t < tiles; t += nb) {
        const int64_t row0 = t * TR;
        const int nrows = (int)(B - row0 < TR ? B - row0 : TR);
        // the first chunk of W2 is in flight while dz2 is formed
        float pre[NPREB];
#pragma unroll
        for (int q = 0; q < NPREB; ++q) pre[q] = n.W2[tid + q * NTB];
        for (int e = tid; e < TR * KP; e += NTB) {
            const int r = e / KP, k = e % KP;
            float v = 0.0f;
            if (r < nrows) {
                if (k < d0) v = a.x0[net][(row0 + r) * d0 + k];
                else if (k < in) v = a.x1[net][(row0 + r) * d1 + (k - d0)];
            }
            sX[r][k] = v;
        }
        if (tid < TR * OM) {
            const int r = tid / OM, o = tid % OM;
            sDo[r][o] = (r < nrows && o < od) ? dog[(row0 + r) * od + o] : 0.0f;
        }
        __syncthreads();
        // ---- dz2 = (dout W3) (h2 > 0); dW3 += dout^T h2, db2 += dz2, db3 += dout; h1 into LDS
#pragma unroll 8
        for (int r = 0; r < TR; ++r) {
            const bool ok = r < nrows;
            const float h2 = ok ? h2g[(row0 + r) * H + j] : 0.0f;
            sH1[r][j] = ok ? h1g[(row0 + r) * H + j] : 0.0f;
            float dh = 0.0f;
#pragma unroll
            for (int o = 0; o < OM; ++o) {
                const float d = sDo[r][o];
                dh = fmaf(d, w3[o], dh);
                if (WG) gW3[o] = fmaf(d, h2, gW3[o]);
            }
            const float z = h2 > 0.0f ? dh : 0.0f;
            if (WG) gB2 += (double)z;
            sDz[r][j] = z;
        }
        if (WG && tid < OM)
            for (int r = 0; r < TR; ++r) gB3 += (double)sDo[r][tid];
        __syncthreads();
        // ---- dW2 += dz2^T h1: K = the tile's rows, r = 16 lh + s
        if (WG) {
#pragma unroll 2
            for (int s = 0; s < TR / 2; ++s) {
                const int r = (TR / 2) * lh + s;
                const float z0 = sDz[r][64 * w + lc], z1 = sDz[r][64 * w + 32 + lc];
#pragma unroll
                for (int kb = 0; kb < NKB; ++kb) {
                    const float h = sH1[r][32 * kb + lc];
                    gW2[0][WG ? kb : 0] = mfma32(z0, h, gW2[0][WG ? kb : 0]);
                    gW2[WG ? 1 : 0][WG ? kb : 0] = mfma32(z1, h, gW2[WG ? 1 : 0][WG ? kb : 0]);
                }
            }
        }
        // ---- dh1 = dz2 W2: lane: A = dz2[row lc][u], B = W2[u][64 w + 32 jb + lc], u = 16 c + 8 lh + 4 s4 + e;
        //      chunk c adds into accumulator c & 1
        f32x16 dh[2][2] = {};
#pragma unroll 2
        for (int c = 0; c < NCHB; ++c) {
            if (c) __syncthreads();   // every wave is done with the chunk before
#pragma unroll
            for (int q = 0; q < NPREB; ++q) sW[q][tid] = pre[q];
            __syncthreads();
            if (c + 1 < NCHB) {
#pragma unroll
                for (int q = 0; q < NPREB; ++q) pre[q] = n.W2[(c + 1) * KCB * H + tid + q * NTB];
            }
#pragma unroll
            for (int s4 = 0; s4 < KCB / 8; ++s4) {
                const int u = (KCB / 2) * lh + 4 * s4;
                const float4 z = *reinterpret_cast<const float4*>(&sDz[lc][c * KCB + u]);
                const float zz[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    dh[0][c & 1] = mfma32(zz[e], sW[u + e][64 * w + lc], dh[0][c & 1]);
                    dh[1][c & 1] = mfma32(zz[e], sW[u + e][64 * w + 32 + lc], dh[1][c & 1]);
                }
            }
        }
        __syncthreads();   // every read of dz2 is done: dz1 replaces it
#pragma unroll
        for (int jb = 0; jb < 2; ++jb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = crow(r, lh), col = 64 * w + 32 * jb + lc;
                sDz[row][col] = sH1[row][col] > 0.0f ? dh[jb][0][r] + dh[jb][1][r] : 0.0f;
            }
        __syncthreads();
        // ---- dW1 += dz1^T x, db1 += dz1
        if (WG) {
#pragma unroll 2
            for (int r = 0; r < TR; ++r) {
                const float z = sDz[r][j];
                gB1 += (double)z;
#pragma unroll
                for (int k = 0; k < KP; ++k) gW1[k] = fmaf(z, sX[r][k], gW1[k]);
            }
        }
        // ---- dx1 = (dz1 W1)[:, d0:]: thread (rows r and r + 16, column c), four interleaved chains over the units
        if (want_dx) {
            const int c = tid % 16;
            for (int r = tid / 16; r < nrows; r += TR / 2) {
                if (c < d1) {
                    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 2
                    for (int u = 0; u < H; u += 4)
#pragma unroll
                        for (int e = 0; e < 4; ++e) s[e] = fmaf(sDz[r][u + e], sW1[u + e][d0 + c], s[e]);
                    dxp[((int64_t)net * B + row0 + r) * d1 + c] = (s[0] + s[1]) + (s[2] + s[3]);
                }
            }
        }
        __syncthreads();   // the next tile's staging overwrites sX, sDo, sH1, sDz
    }

    if (!WG) return;
    // ---- this block's partials, in the flat gradient layout
    float* const Pn = part + ((int64_t)net * nb + blockIdx.x) * P;
    const int64_t oB1 = (int64_t)H * in, oW2 = oB1 + H, oB2 = oW2 + (int64_t)H * H, oW3 = oB2 + H,
                  oB3 = oW3 + (int64_t)od * H;
#pragma unroll
    for (int jb = 0; jb < (WG ? 2 : 1); ++jb)
#pragma unroll
        for (int kb = 0; kb < (WG ? NKB : 1); ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                Pn[oW2 + (64 * w + 32 * jb + crow(r, lh)) * H + 32 * kb + lc] = gW2[jb][kb][r];
#pragma unroll
    for (int k = 0; k < KP; ++k)
        if (k < in) Pn[j * in + k] = gW1[k];
#pragma unroll
    for (int o = 0; o < OM; ++o)
        if (o < od) Pn[oW3 + o * H + j] = gW3[o];
    Pn[oB1 + j] = (float)gB1;
    Pn[oB2 + j] = (float)gB2;
    if (tid < od) Pn[oB3 + tid] = (float)gB3;
}

// blockIdx.y < n_nets: that network's flat gradient = the sum of its nb block
// partials, in block order, in fp64.  blockIdx.y == n_nets: dx1 = the sum of
// the networks' dx1, in index order.
constexpr int NT_RED = 256;
__global__ __launch_bounds__(NT_RED) void k_sac_net_reduce(SalpSacNetBackward a, int nb, int64_t P,
                                                           const float* __restrict__ part,
                                                           const float* __restrict__ dxp) {
    const int64_t i = (int64_t)blockIdx.x * NT_RED + threadIdx.x;
    const int y = blockIdx.y;
    if (y < a.n_nets) {
        if (!a.dparams[0] || i >= P) return;
        const float* p = part + (int64_t)y * nb * P + i;
        double s = 0.0;
#pragma unroll 8
        for (int b = 0; b < nb; ++b) s += (double)p[(int64_t)b * P];
        a.dparams[y][i] = (float)s;
    } else {
        const int64_t n = a.batch * a.d1;
        if (!a.dx1 || i >= n) return;
        double s = 0.0;
        for (int k = 0; k < a.n_nets; ++k) s += (double)dxp[k * n + i];
        a.dx1[i] = (float)s;
    }
}

inline int64_t tiles_of(int64_t B) { return (B + TR - 1) / TR; }
inline int blocks_of(int64_t B) {
    const int64_t t = tiles_of(B);
    return (int)(t < MAXB ? t : MAXB);
}

bool sac_net_dims_ok(int in, int od) {
    return in >= 1 && in <= SALP_SAC_NET_IN_MAX && od >= 1 && od <= SALP_SAC_NET_OUT_MAX;
}
// the part SalpSacNetForward and SalpSacNetBackward share; nullptr if it is sound, else what is wrong
const char* sac_net_bad(int64_t batch, int d0, int d1, int od, int n_nets, const float* const* params,
                        const float* const* x0, const float* const* x1) {
    if (batch <= 0 || batch > INT32_MAX) return "batch must be in 1 .. 2^31 - 1";
    if (d0 < 1 || d1 < 0 || !sac_net_dims_ok(d0 + d1, od)) return "d0 >= 1, d1 >= 0, d0 + d1 <= 17 and out_dim in 1 .. 6";
    if (n_nets < 1 || n_nets > SALP_SAC_NET_MAX_NETS) return "n_nets must be in 1 .. 4";
    for (int i = 0; i < n_nets; ++i)
        if (!params[i] || !x0[i] || (d1 > 0 && !x1[i])) return "null params, x0 or x1";
    return nullptr;
}

}  // namespace

extern "C" {

int64_t salp_sac_net_num_params(int in_dim, int out_dim) {
    return salp_sac_net_offset(in_dim, out_dim, SALP_SAC_NET_N_TENSORS);
}

int64_t salp_sac_net_offset(int in_dim, int out_dim, int tensor) {
    if (!sac_net_dims_ok(in_dim, out_dim) || tensor < 0 || tensor > SALP_SAC_NET_N_TENSORS) {
        fail(SALP_EINVAL, "salp_sac_net_offset: in_dim in 1 .. 17, out_dim in 1 .. 6, tensor in 0 .. 6");
        return -1;
    }
    const int64_t size[SALP_SAC_NET_N_TENSORS] = {(int64_t)H * in_dim, H, (int64_t)H * H, H, (int64_t)out_dim * H,
                                                  out_dim};
    int64_t off = 0;
    for (int t = 0; t < tensor; ++t) off += size[t];
    return off;
}

int salp_sac_net_tile_rows(void) { return TR; }
int salp_sac_net_max_blocks(void) { return MAXB; }

int64_t salp_sac_net_workspace_floats(int64_t batch, int d0, int d1, int out_dim, int n_nets) {
    if (batch <= 0 || batch > INT32_MAX || d0 < 1 || d1 < 0 || !sac_net_dims_ok(d0 + d1, out_dim) || n_nets < 1 ||
        n_nets > SALP_SAC_NET_MAX_NETS) {
        fail(SALP_EINVAL, "salp_sac_net_workspace_floats: bad argument");
        return -1;
    }
    // [n_nets][blocks][P] parameter partials, then [n_nets][batch][d1] dx1 partials
    return (int64_t)n_nets * blocks_of(batch) * num_params(d0 + d1, out_dim) + (int64_t)n_nets * batch * d1;
}

// The launch status of each: one hipGetLastError() right after the launches (salp_ppo.hip explains why).
int salp_sac_net_forward(const SalpSacNetForward* f, void* stream) {
    if (!f) return fail(SALP_EINVAL, "salp_sac_net_forward: null argument");
    if (const char* bad = sac_net_bad(f->batch, f->d0, f->d1, f->out_dim, f->n_nets, f->params, f->x0, f->x1))
        return fail(SALP_EINVAL, std::string("salp_sac_net_forward: ") + bad);
    for (int i = 0; i < f->n_nets; ++i) {
        if (!f->out[i]) return fail(SALP_EINVAL, "salp_sac_net_forward: null out");
        if (!f->h1[i] != !f->h2[i])
            return fail(SALP_EINVAL, "salp_sac_net_forward: h1 and h2 are both NULL or both set");
    }
    hipLaunchKernelGGL(k_sac_net_fwd, dim3((unsigned)tiles_of(f->batch), (unsigned)f->n_nets), dim3(NT), 0,
                       (hipStream_t)stream, *f);
    return check_hip(hipGetLastError(), "k_sac_net_fwd");
}

int salp_sac_net_backward(const SalpSacNetBackward* b, void* stream) {
    if (!b) return fail(SALP_EINVAL, "salp_sac_net_backward: null argument");
    if (const char* bad = sac_net_bad(b->batch, b->d0, b->d1, b->out_dim, b->n_nets, b->params, b->x0, b->x1))
        return fail(SALP_EINVAL, std::string("salp_sac_net_backward: ") + bad);
    for (int i = 0; i < b->n_nets; ++i) {
        if (!b->h1[i] || !b->h2[i] || !b->dout[i])
            return fail(SALP_EINVAL, "salp_sac_net_backward: null h1, h2 or dout");
        if (!b->dparams[i] != !b->dparams[0])
            return fail(SALP_EINVAL, "salp_sac_net_backward: dparams are all NULL or all set");
    }
    if (!b->dparams[0] && !b->dx1) return fail(SALP_EINVAL, "salp_sac_net_backward: neither dparams nor dx1 is set");
    if (b->dx1 && b->d1 == 0) return fail(SALP_EINVAL, "salp_sac_net_backward: dx1 needs d1 > 0");
    if (!b->workspace) return fail(SALP_EINVAL, "salp_sac_net_backward: null workspace");
    hipStream_t s = (hipStream_t)stream;
    const int nb = blocks_of(b->batch);
    const int64_t P = num_params(b->d0 + b->d1, b->out_dim), tiles = tiles_of(b->batch);
    float* const part = b->workspace;
    float* const dxp = part + (int64_t)b->n_nets * nb * P;
    const bool wg = b->dparams[0] != nullptr;
    const dim3 grid((unsigned)nb, (unsigned)b->n_nets);
    if (wg) hipLaunchKernelGGL(k_sac_net_bwd<true>, grid, dim3(NTB), 0, s, *b, tiles, P, part, dxp);
    else hipLaunchKernelGGL(k_sac_net_bwd<false>, grid, dim3(NTB), 0, s, *b, tiles, P, part, dxp);
    // the reduction is not enqueued behind a backward that did not launch
    if (const int rc = check_hip(hipGetLastError(), "k_sac_net_bwd")) return rc;
    const int64_t nx = b->dx1 ? b->batch * b->d1 : 0, n = wg && P > nx ? P : nx;
    hipLaunchKernelGGL(k_sac_net_reduce, dim3((unsigned)((n + NT_RED - 1) / NT_RED), (unsigned)b->n_nets + 1),
                       dim3(NT_RED), 0, s, *b, nb, P, part, dxp);
    return check_hip(hipGetLastError(), "k_sac_net_bwd");
}

}  // extern "C"
