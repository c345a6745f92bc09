// salp_metrics.hip — episode metrics and evaluation bookkeeping on the device (gfx950).
//
// What it restates: the per-env-step host work of the reference's callbacks,
// which walk a Python list of info dicts after every vec-env step:
//
//   k_epwin_push      src/tensorboard_callback.py:36-123: a deque(maxlen=window)
//                     per metric, appended to for every env whose episode ended,
//                     in env order — here one ring of rows and one counter
//   k_epwin_summary   :131-205: mean / np.std / min / max of every deque, the
//                     distance per cycle and the cycles to success
//   k_eval_account    stable_baselines3 evaluate_policy over a vector env: env i
//                     contributes its first target[i] episodes
//
// Everything is enqueued on the caller's stream, nothing allocates or
// synchronises, and there is no floating-point atomic: the push ranks its
// finishers with ballots and an integer scan, the summary adds in one fixed
// order, and the only atomic is the integer countdown of the evaluation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/salp.h"
#include "salp_host.h"

using salp::check_hip;
using salp::fail;

namespace {

constexpr int kPushBlock = 1024;              // one workgroup walks all envs
constexpr int kPushWaves = kPushBlock / 64;
constexpr int kSumBlock = 64;                 // one wave per statistic
constexpr int kEvalBlock = 256;
constexpr int kInfoCols = SALP_EPWIN_COLS - 4;   // SALP_INFO_PATH_LENGTH .. SALP_INFO_AVG_R_OBSTACLE

static_assert(SALP_INFO_AVG_R_OBSTACLE - SALP_INFO_PATH_LENGTH + 1 == kInfoCols, "row layout");
static_assert(SALP_EPSUM_DIM == 1 + 4 * SALP_EPWIN_COLS + 3, "summary layout");
static_assert(SALP_EPWIN_MAX_WINDOW <= INT32_MAX, "window is an int32");

__device__ __forceinline__ bool finishes(const SalpEpisodePush& p, int64_t e) {
    return (p.terminated[e] | p.truncated[e]) != 0 && !(p.skip && p.skip[e] != 0);
}

// Pass 1 counts the finishers D; pass 2 walks the envs again in chunks of one
// env per thread, ranks each chunk's finishers (ballot inside a wave, the 16
// wave totals through LDS) on top of the chunks before it, and the r-th
// finisher writes episode count + r into row (count + r) % window — unless
// D > window and it is not among the last `window`, whose rows are all distinct.
__global__ __launch_bounds__(kPushBlock) void k_epwin_push(SalpEpisodeWindow w, SalpEpisodePush p) {
    __shared__ int64_t tot[2][kPushWaves];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int64_t n = p.n_envs;
    const int64_t chunks = (n + kPushBlock - 1) / kPushBlock;
    const int64_t count0 = w.count[0];

    int64_t mine = 0;
    for (int64_t e = threadIdx.x; e < n; e += kPushBlock) mine += finishes(p, e) ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if (lane == 0) tot[0][wave] = mine;
    __syncthreads();
    int64_t D = 0;
    for (int k = 0; k < kPushWaves; ++k) D += tot[0][k];
    __syncthreads();   // tot[0] is written again by chunk 0
    if (D == 0) return;
    const int64_t first = D > w.window ? D - w.window : 0;   // finishers before this rank are overwritten: skipped

    int64_t before = 0;   // finishers in the chunks already walked
    for (int64_t c = 0; c < chunks; ++c) {
        const int64_t e = c * kPushBlock + threadIdx.x;
        const bool fin = e < n && finishes(p, e);
        const unsigned long long m = __ballot(fin);
        int64_t* t = tot[c & 1];
        if (lane == 0) t[wave] = __popcll(m);
        __syncthreads();   // the other buffer is next written after the next barrier, when every read of it is over
        int64_t below = 0, all = 0;
        for (int k = 0; k < kPushWaves; ++k) {
            const int64_t v = t[k];
            below += k < wave ? v : 0;
            all += v;
        }
        if (fin) {
            const int64_t r = before + below + __popcll(m & ((1ull << lane) - 1ull));
            if (r >= first) {
                const int64_t ep = count0 + r;
                double* row = w.rows + (ep % w.window) * SALP_EPWIN_COLS;
                const double* info = p.info + e * SALP_INFO_DIM;
                const bool term = p.terminated[e] != 0;
                // bit copies: through integers, so a NaN keeps its payload
                const uint64_t* src = reinterpret_cast<const uint64_t*>(info);
                uint64_t* dst = reinterpret_cast<uint64_t*>(row);
                dst[0] = src[SALP_INFO_EP_RETURN];
                dst[1] = src[SALP_INFO_EP_LEN];
                row[2] = term ? 1.0 : 0.0;
                row[3] = (!term && p.truncated[e] != 0) ? 1.0 : 0.0;
                for (int k = 0; k < kInfoCols; ++k) dst[4 + k] = src[SALP_INFO_PATH_LENGTH + k];
            }
        }
        before += all;
    }
    // every thread read count[0] before the first barrier
    if (threadIdx.x == 0) w.count[0] = count0 + D;
}

// ---------------------------------------------------------------- k_epwin_push_log
// One salp_collect_episodes log into the window, in the order the lock-step
// pushes would have used: by (step, env).  A candidate is a kept slot of an
// env's ring; its key is step * n_envs + env, and keys are distinct (an env
// ends at most one episode per step).
struct LogCand {
    bool kept;
    bool oldest_of_dropper;   // the env dropped episodes and this is the oldest it kept
    int64_t key;
};
__device__ __forceinline__ LogCand log_candidate(const SalpEpisodeLog& l, int64_t n_envs, int64_t idx) {
    const int64_t K = l.per_env;
    // most logs have fewer than 2^32 slots: the 32-bit division is several times cheaper
    const int64_t i = ((uint64_t)(n_envs * K) >> 32) == 0 ? (int64_t)((uint32_t)idx / (uint32_t)K) : idx / K;
    const int64_t slot = idx - i * K;
    const int64_t cnt = l.count[i] > 0 ? l.count[i] : 0;
    LogCand c{slot < cnt, false, 0};
    if (c.kept) {
        c.key = (int64_t)l.step[idx] * n_envs + i;
        if (cnt > K) {   // the ring wrapped: slot holds the env's latest episode e with e % K == slot
            int64_t e = (cnt - 1) / K * K + slot;
            if (e > cnt - 1) e -= K;
            c.oldest_of_dropper = e == cnt - K;
        }
    }
    return c;
}

// The block's sum of v; every thread gets it.  One barrier: the caller alternates buf.
__device__ __forceinline__ int64_t block_sum(int64_t v, int64_t* buf) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (threadIdx.x % 64 == 0) buf[threadIdx.x / 64] = v;
    __syncthreads();
    int64_t s = 0;
    for (int k = 0; k < kPushWaves; ++k) s += buf[k];
    return s;
}

// Pass 1: D (all episodes), M (kept ones) and the largest key.  Then a
// bisection on the key finds the threshold T with exactly min(window, M) kept
// keys >= T (one pass over the candidates per bit of the key range), the
// selected candidates go to LDS (an integer counter hands out the places:
// their order does not matter), and each is ranked against the others: with
// g selected keys above it, it is episode count + D - 1 - g.
__global__ __launch_bounds__(kPushBlock) void k_epwin_push_log(SalpEpisodeWindow w, SalpEpisodeLog l, int64_t n_envs,
                                                               int64_t* lost) {
    __shared__ int64_t tot[3][kPushWaves];
    __shared__ int64_t s_key[SALP_EPWIN_MAX_WINDOW];
    __shared__ int64_t s_loc[SALP_EPWIN_MAX_WINDOW];   // slot index, bit 62: oldest_of_dropper
    __shared__ int s_n, s_lost;
    const int64_t K = l.per_env, total = n_envs * K;
    const int64_t count0 = w.count[0];
    if (threadIdx.x == 0) s_n = s_lost = 0;

    int64_t d = 0, m = 0, top = -1;
    for (int64_t i = threadIdx.x; i < n_envs; i += kPushBlock) {
        const int64_t cnt = l.count[i] > 0 ? l.count[i] : 0;
        d += cnt;
        m += cnt < K ? cnt : K;
    }
    for (int64_t idx = threadIdx.x; idx < total; idx += kPushBlock) {
        const LogCand c = log_candidate(l, n_envs, idx);
        if (c.kept && c.key > top) top = c.key;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t u = __shfl_xor(top, o, 64);
        top = u > top ? u : top;
    }
    if (threadIdx.x % 64 == 0) tot[2][threadIdx.x / 64] = top;
    const int64_t D = block_sum(d, tot[0]);
    const int64_t M = block_sum(m, tot[1]);   // its barrier covers tot[2] and s_n too
    for (int k = 0; k < kPushWaves; ++k) top = tot[2][k] > top ? tot[2][k] : top;
    if (D == 0) return;   // uniform
    const int64_t sel = M < w.window ? M : w.window;   // >= 1: an env with an episode keeps one

    int64_t lo = 0, hi = top + 1;   // kept keys >= lo: at least sel; >= hi: fewer
    for (int it = 0; hi - lo > 1; ++it) {
        const int64_t mid = lo + (hi - lo) / 2;
        int64_t above = 0;
        for (int64_t idx = threadIdx.x; idx < total; idx += kPushBlock) {
            const LogCand c = log_candidate(l, n_envs, idx);
            above += c.kept && c.key >= mid ? 1 : 0;
        }
        // tot[0] and tot[1] in turn: a buffer is written again two barriers after its reads
        if (block_sum(above, tot[it & 1]) >= sel) lo = mid; else hi = mid;
    }
    for (int64_t idx = threadIdx.x; idx < total; idx += kPushBlock) {
        const LogCand c = log_candidate(l, n_envs, idx);
        if (c.kept && c.key >= lo) {
            const int at = atomicAdd(&s_n, 1);   // integer, LDS: exactly sel of them
            if (at < SALP_EPWIN_MAX_WINDOW) {
                s_key[at] = c.key;
                s_loc[at] = idx | (c.oldest_of_dropper ? (int64_t)1 << 62 : 0);
            }
        }
    }
    __syncthreads();
    const int n_sel = s_n < SALP_EPWIN_MAX_WINDOW ? s_n : SALP_EPWIN_MAX_WINDOW;
    if ((int)threadIdx.x < n_sel) {
        const int64_t key = s_key[threadIdx.x];
        int64_t g = 0;
        for (int k = 0; k < n_sel; ++k) g += s_key[k] > key ? 1 : 0;
        const int64_t ep = count0 + D - 1 - g;
        const int64_t loc = s_loc[threadIdx.x];
        if (loc >> 62) atomicAdd(&s_lost, 1);
        const uint64_t* src = reinterpret_cast<const uint64_t*>(l.rows) + (loc & (((int64_t)1 << 62) - 1)) * SALP_EPWIN_COLS;
        uint64_t* dst = reinterpret_cast<uint64_t*>(w.rows) + (ep % w.window) * SALP_EPWIN_COLS;
        for (int k = 0; k < SALP_EPWIN_COLS; ++k) dst[k] = src[k];   // bit copies
    }
    __syncthreads();
    // every thread read count[0] before the first barrier
    if (threadIdx.x == 0) {
        w.count[0] = count0 + D;
        if (s_lost) lost[0] += s_lost;
    }
}

// A wave's sum in one fixed order: each lane adds its rows in ascending order, then the butterfly.
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_min(double v) {
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) {
        const double u = __shfl_xor(v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

// Block c < SALP_EPWIN_COLS: column c's mean, two-pass population standard
// deviation, min and max.  Block SALP_EPWIN_COLS: mean(path_length / ep_len).
// Block SALP_EPWIN_COLS + 1: mean ep_len over success rows and their number.
__global__ __launch_bounds__(kSumBlock) void k_epwin_summary(SalpEpisodeWindow w, double* __restrict__ out) {
    const int lane = threadIdx.x;
    const int c = blockIdx.x;
    const int64_t cnt = w.count[0];
    const int n = (int)(cnt < w.window ? cnt : w.window);   // rows 0 .. n - 1 hold episodes
    const double nan = __longlong_as_double(0x7FF8000000000000ll);
    const double* rows = w.rows;
    if (c == 0 && lane == 0) out[0] = (double)n;
    if (c < SALP_EPWIN_COLS) {
        double s = 0.0, lo = INFINITY, hi = -INFINITY;
        for (int r = lane; r < n; r += 64) {
            const double v = rows[(int64_t)r * SALP_EPWIN_COLS + c];
            s += v;
            lo = v < lo ? v : lo;
            hi = v > hi ? v : hi;
        }
        const double mean = wave_sum(s) / (double)n;
        double q = 0.0;
        for (int r = lane; r < n; r += 64) {
            const double d = rows[(int64_t)r * SALP_EPWIN_COLS + c] - mean;
            q += d * d;
        }
        const double var = wave_sum(q) / (double)n;
        lo = wave_min(lo);
        hi = wave_max(hi);
        if (lane == 0) {
            double* o = out + 1 + 4 * c;
            o[0] = n ? mean : nan;
            o[1] = n ? sqrt(var) : nan;
            o[2] = n ? lo : nan;
            o[3] = n ? hi : nan;
        }
    } else if (c == SALP_EPWIN_COLS) {
        double s = 0.0;
        for (int r = lane; r < n; r += 64)
            s += rows[(int64_t)r * SALP_EPWIN_COLS + 4] / rows[(int64_t)r * SALP_EPWIN_COLS + 1];
        s = wave_sum(s);
        if (lane == 0) out[1 + 4 * SALP_EPWIN_COLS] = n ? s / (double)n : nan;
    } else {
        double s = 0.0, k = 0.0;
        for (int r = lane; r < n; r += 64) {
            const bool ok = rows[(int64_t)r * SALP_EPWIN_COLS + 2] == 1.0;
            s += ok ? rows[(int64_t)r * SALP_EPWIN_COLS + 1] : 0.0;
            k += ok ? 1.0 : 0.0;
        }
        s = wave_sum(s);
        k = wave_sum(k);   // whole numbers <= 1024: exact
        if (lane == 0) {
            out[2 + 4 * SALP_EPWIN_COLS] = k > 0.0 ? s / k : nan;
            out[3 + 4 * SALP_EPWIN_COLS] = n ? k : nan;
        }
    }
}

// One thread per env; an env only ever touches its own slots.
__global__ __launch_bounds__(kEvalBlock) void k_eval_account(SalpEvalState s, SalpEpisodePush p) {
    const int64_t i = (int64_t)blockIdx.x * kEvalBlock + threadIdx.x;
    if (i >= s.n_envs) return;
    if ((p.terminated[i] | p.truncated[i]) == 0) return;
    const int32_t d = s.done_count[i];
    if (d >= s.target[i]) return;   // SB3 ignores an env's episodes past its target
    const int64_t slot = s.offset[i] + d;
    const double* info = p.info + i * SALP_INFO_DIM;
    s.ep_return[slot] = info[SALP_INFO_EP_RETURN];
    s.ep_len[slot] = info[SALP_INFO_EP_LEN];
    s.success[slot] = p.terminated[i] != 0 ? 1 : 0;
    s.done_count[i] = d + 1;
    atomicAdd(reinterpret_cast<unsigned long long*>(s.remaining), ~0ull);   // integer: the order does not matter
}

bool epwin_ok(const SalpEpisodeWindow* w) {
    return w && w->window >= 1 && w->window <= SALP_EPWIN_MAX_WINDOW && w->rows && w->count;
}

bool eppush_ok(const SalpEpisodePush* p) {
    return p && p->n_envs >= 1 && p->info && p->terminated && p->truncated;
}

}  // namespace

extern "C" {

// The launch status of each: one hipGetLastError() right after the launch (salp_ppo.hip explains why).
int salp_episode_window_push(const SalpEpisodeWindow* w, const SalpEpisodePush* p, void* stream) {
    if (!epwin_ok(w))
        return fail(SALP_EINVAL, "salp_episode_window_push: window must be in 1 .. 1024, rows and count set");
    if (!eppush_ok(p))
        return fail(SALP_EINVAL, "salp_episode_window_push: n_envs >= 1 and info, terminated, truncated set");
    hipLaunchKernelGGL(k_epwin_push, dim3(1), dim3(kPushBlock), 0, (hipStream_t)stream, *w, *p);
    return check_hip(hipGetLastError(), "k_epwin_push");
}

int salp_episode_window_push_log(const SalpEpisodeWindow* w, const SalpEpisodeLog* log, int64_t n_envs,
                                 int64_t* lost, void* stream) {
    if (!epwin_ok(w))
        return fail(SALP_EINVAL, "salp_episode_window_push_log: window must be in 1 .. 1024, rows and count set");
    if (!log || log->per_env < 1 || n_envs < 1)
        return fail(SALP_EINVAL, "salp_episode_window_push_log: a log, per_env >= 1 and n_envs >= 1 are required");
    if (!log->rows || !log->step || !log->count || !lost)
        return fail(SALP_EINVAL, "salp_episode_window_push_log: rows, step, count and lost must be set");
    if (n_envs > INT64_MAX / ((int64_t)1 << 25) || log->per_env > INT64_MAX / ((int64_t)1 << 25) / n_envs)
        return fail(SALP_EINVAL, "salp_episode_window_push_log: n_envs * per_env too large");
    hipLaunchKernelGGL(k_epwin_push_log, dim3(1), dim3(kPushBlock), 0, (hipStream_t)stream, *w, *log, n_envs, lost);
    return check_hip(hipGetLastError(), "k_epwin_push_log");
}

int salp_episode_window_summary(const SalpEpisodeWindow* w, double* out, void* stream) {
    if (!epwin_ok(w))
        return fail(SALP_EINVAL, "salp_episode_window_summary: window must be in 1 .. 1024, rows and count set");
    if (!out) return fail(SALP_EINVAL, "salp_episode_window_summary: null out");
    hipLaunchKernelGGL(k_epwin_summary, dim3(SALP_EPWIN_COLS + 2), dim3(kSumBlock), 0, (hipStream_t)stream, *w, out);
    return check_hip(hipGetLastError(), "k_epwin_summary");
}

int salp_eval_account(const SalpEvalState* s, const SalpEpisodePush* p, void* stream) {
    static_assert(kEvalBlock == 256, "the bound below is INT32_MAX blocks of kEvalBlock envs");
    if (!s || s->n_envs < 1 || s->n_envs > INT32_MAX * (int64_t)256)
        return fail(SALP_EINVAL, "salp_eval_account: n_envs must be positive");
    if (!s->target || !s->offset || !s->done_count || !s->ep_return || !s->ep_len || !s->success || !s->remaining)
        return fail(SALP_EINVAL, "salp_eval_account: null state buffer");
    if (!eppush_ok(p) || p->n_envs != s->n_envs)
        return fail(SALP_EINVAL, "salp_eval_account: the step must be of the state's n_envs, buffers set");
    const int64_t blocks = (s->n_envs + kEvalBlock - 1) / kEvalBlock;
    hipLaunchKernelGGL(k_eval_account, dim3((unsigned)blocks), dim3(kEvalBlock), 0, (hipStream_t)stream, *s, *p);
    return check_hip(hipGetLastError(), "k_eval_account");
}

}  // extern "C"
