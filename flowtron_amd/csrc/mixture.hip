// Gaussian-mixture prior (flowtron.py:217-231, 312-363, 437-439): mixture negative log-likelihood forward / backward, the
// mel encoder's time pooling, the component softmax and a component sampler (gfx950, fp32, no float atomics).
//
// Likelihood layout.  One workgroup owns utterance b and a chunk of R * FPT frames (R = 256 / M frame rows in flight, thread
// = (row r, channel m), FPT frames per thread, fully unrolled so z, the log-sum-exp and dz stay in registers).  The per-
// (channel, component) constants -- mean, a = -exp(-log_var) / 2, h = -log_var / 2 -- and log prob / prob of the utterance are
// formed ONCE per workgroup in LDS, component-major ([c][m]: the lanes of a wave read consecutive banks).  The element chain is
// pinned with explicit roundings (the error bounds of tests/gm_ref64.py follow it operation by operation):
//     d = z - mean ; u_c = fma(a_c, d * d, h_c) ; e_c = log prob_c + u_c ; l = max_c e_c + log(sum_c exp(e_c - max))
// Reductions are two-stage and ordered: a workgroup leaves ONE partial per output it touches in `work`, a second kernel adds the
// partials of an utterance's chunks in chunk order.  Nothing depends on arrival order: two launches give identical bits.
#include "common.h"
#include <math.h>

namespace {

constexpr int NT = 256;
constexpr int FPT = 8;                    // frames per thread
constexpr int MAX_LS = 8;
struct LsPtrs { const float* p[MAX_LS]; };

__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < NT / 64; ++i) r += red[i];
    return r;
}

inline int rows_in_flight(int M) { return NT / M; }
inline int chunk_frames(int M) { return rows_in_flight(M) * FPT; }
inline size_t consts_bytes(int M, int C) { return ((size_t)3 * C * M + 2 * C) * sizeof(float); }
constexpr size_t LDS_CONSTS_MAX = 64 * 1024 - 2304;   // a workgroup's 64 KB less the backward's static reduction arrays (M 80 x C 64 fits)

struct Consts { const float *mu, *a, *h, *lp, *pr; };

// mean / log_var rows [M][C] of utterance bm -> LDS [c][m]; prob row b
__device__ __forceinline__ Consts load_consts(float* sm, const float* __restrict__ mean, const float* __restrict__ log_var,
                                              const float* __restrict__ prob, int b, int bm, int M, int C) {
    float *mu = sm, *a = sm + C * M, *h = sm + 2 * C * M, *lp = sm + 3 * C * M, *pr = lp + C;
    const float* mb = mean + (long)bm * M * C;
    const float* vb = log_var + (long)bm * M * C;
    for (int i = threadIdx.x; i < M * C; i += NT) {
        const int m = i / C, c = i - m * C;
        const float lv = vb[i];
        mu[c * M + m] = mb[i];
        a[c * M + m] = __fmul_rn(-0.5f, expf(-lv));
        h[c * M + m] = __fmul_rn(-0.5f, lv);
    }
    for (int c = threadIdx.x; c < C; c += NT) {
        const float p = prob[(long)b * C + c];
        pr[c] = p;
        lp[c] = logf(p);
    }
    __syncthreads();
    return Consts{mu, a, h, lp, pr};
}

__device__ __forceinline__ float comp_u(float z, float mu, float a, float h, float& d, float& d2) {
    d = __fsub_rn(z, mu);
    d2 = __fmul_rn(d, d);
    return __fmaf_rn(a, d2, h);
}

// log sum_c prob_c N(z; mean_c, exp(log_var_c)) without the 2 pi term, shifted by the largest exponent
__device__ __forceinline__ float mixture_lse(float z, const Consts& k, int m, int M, int C) {
    float mx = -INFINITY;
    for (int c = 0; c < C; ++c) {
        float d, d2;
        mx = fmaxf(mx, __fadd_rn(k.lp[c], comp_u(z, k.mu[c * M + m], k.a[c * M + m], k.h[c * M + m], d, d2)));
    }
    float s = 0.f;
    for (int c = 0; c < C; ++c) {
        float d, d2;
        s = __fadd_rn(s, expf(__fsub_rn(__fadd_rn(k.lp[c], comp_u(z, k.mu[c * M + m], k.a[c * M + m], k.h[c * M + m], d, d2)), mx)));
    }
    return __fadd_rn(mx, logf(s));
}

__device__ __forceinline__ int clamp_len(int l, int T) { return l < 0 ? 0 : (l > T ? T : l); }

// part[chunk * B + b] = - sum over the chunk's valid (t, m) of (l + sum_f log_s_f)
__global__ void __launch_bounds__(NT) mixture_nll_fwd_k(const float* __restrict__ z, const float* __restrict__ mean,
                                                        const float* __restrict__ log_var, const float* __restrict__ prob, LsPtrs ls,
                                                        int n_ls, long ld_ls, const int* __restrict__ lens, float* __restrict__ part,
                                                        int T, int B, int M, int C, int Bm) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[NT / 64];
    const int b = blockIdx.y, R = NT / M, CH = R * FPT;
    const int t0 = blockIdx.x * CH, len = clamp_len(lens[b], T);
    float nl = 0.f;
    if (t0 < len) {                                             // (uniform over the workgroup)
        const Consts k = load_consts(sm, mean, log_var, prob, b, Bm == 1 ? 0 : b, M, C);
        const int r = threadIdx.x / M, m = threadIdx.x - r * M;
        if (r < R) {
#pragma unroll
            for (int j = 0; j < FPT; ++j) {
                const int t = t0 + j * R + r;
                if (t < len) {
                    const long row = (long)t * B + b;
                    float v = mixture_lse(z[row * M + m], k, m, M, C);
                    for (int f = 0; f < n_ls; ++f) v += ls.p[f][row * ld_ls + m];
                    nl -= v;
                }
            }
        }
    }
    nl = block_sum(nl, red);
    if (threadIdx.x == 0) part[(long)blockIdx.x * B + b] = nl;
}

// acc: [0] the sum, [4] 1 / (n M), [6] n -- n counts the frames the sums visited (lengths clamped to 0 ..= T)
__global__ void __launch_bounds__(NT) mixture_nll_finalize_k(const float* __restrict__ part, int n_part, const int* __restrict__ lens,
                                                             int T, int B, int M, float* __restrict__ acc, float* __restrict__ loss_out) {
    __shared__ float red[NT / 64];
    float s = 0.f, n = 0.f;
    for (int i = threadIdx.x; i < n_part; i += NT) s += part[i];
    for (int b = threadIdx.x; b < B; b += NT) n += (float)clamp_len(lens[b], T);
    s = block_sum(s, red);
    n = block_sum(n, red);
    if (threadIdx.x == 0) {
        const float nm = n * (float)M;
        loss_out[0] = s / nm;
        acc[0] = s;
        acc[4] = 1.f / nm;
        acc[6] = n;
    }
}

// dz, dls for every frame of the chunk (0 at padded ones); with WANT, per (m, c) the chunk's unscaled sums of
//   d nll / d mean_c = -r_c d / var_c ,  d nll / d log_var_c = r_c (1/2 + a_c d^2) ,  d nll / d prob_c = -q_c   (r_c = prob_c q_c)
// into pm / pv [chunk][B][M][C] and pp [chunk][B][C]
template <bool WANT>
__global__ void __launch_bounds__(NT) mixture_nll_bwd_k(const float* __restrict__ z, const float* __restrict__ mean,
                                                        const float* __restrict__ log_var, const float* __restrict__ prob,
                                                        const int* __restrict__ lens, const float* __restrict__ acc,
                                                        const float* __restrict__ g, float* __restrict__ dz, float* __restrict__ dls,
                                                        float* __restrict__ pm, float* __restrict__ pv, float* __restrict__ pp,
                                                        int T, int B, int M, int C, int Bm) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[2][NT];
    __shared__ float redp[NT / 64];
    const int b = blockIdx.y, R = NT / M, CH = R * FPT;
    const int t0 = blockIdx.x * CH, len = clamp_len(lens[b], T);
    const int r = threadIdx.x / M, m = threadIdx.x - r * M;
    const bool active = r < R;
    if (t0 >= len) {                                            // a chunk of padded frames only: zeros, no partials (the reduction skips it)
        if (active)
            for (int j = 0; j < FPT; ++j) {
                const int t = t0 + j * R + r;
                if (t < T) {
                    const long i = ((long)t * B + b) * M + m;
                    dz[i] = 0.f;
                    if (dls) dls[i] = 0.f;
                }
            }
        return;
    }
    const Consts k = load_consts(sm, mean, log_var, prob, b, Bm == 1 ? 0 : b, M, C);
    const float sc = g[0] * acc[4];
    float zv[FPT], lse[FPT], dza[FPT];
#pragma unroll
    for (int j = 0; j < FPT; ++j) {
        const int t = t0 + j * R + r;
        const bool valid = active && t < len;
        zv[j] = valid ? z[((long)t * B + b) * M + m] : 0.f;
        lse[j] = valid ? mixture_lse(zv[j], k, m, M, C) : INFINITY;      // +inf: q = exp(-inf) = 0, the frame adds nothing below
        dza[j] = 0.f;
    }
    const int mi = active ? m : 0;
    for (int c = 0; c < C; ++c) {
        const float mu = k.mu[c * M + mi], a = k.a[c * M + mi], h = k.h[c * M + mi], p = k.pr[c];
        const float inv = __fmul_rn(-2.f, a);
        float dm = 0.f, dv = 0.f, dp = 0.f;
#pragma unroll
        for (int j = 0; j < FPT; ++j) {
            float d, d2;
            const float u = comp_u(zv[j], mu, a, h, d, d2);
            const float q = expf(__fsub_rn(u, lse[j]));
            const float rc = p > 0.f ? __fmul_rn(p, q) : 0.f;
            const float w = __fmul_rn(__fmul_rn(rc, d), inv);
            dza[j] = __fadd_rn(dza[j], w);
            if (WANT) {
                dm = __fsub_rn(dm, w);
                dv = __fadd_rn(dv, __fmul_rn(rc, __fmaf_rn(a, d2, 0.5f)));
                dp = __fsub_rn(dp, q);
            }
        }
        if (WANT) {
            // the R frame rows of a channel and the workgroup's waves are added in index order
            dp = wave_sum(dp);
            __syncthreads();
            red[0][threadIdx.x] = active ? dm : 0.f;
            red[1][threadIdx.x] = active ? dv : 0.f;
            if ((threadIdx.x & 63) == 0) redp[threadIdx.x >> 6] = dp;
            __syncthreads();
            if (threadIdx.x < M) {
                float s0 = 0.f, s1 = 0.f;
                for (int rr = 0; rr < R; ++rr) { s0 += red[0][rr * M + threadIdx.x]; s1 += red[1][rr * M + threadIdx.x]; }
                const long o = (((long)blockIdx.x * B + b) * M + threadIdx.x) * C + c;
                pm[o] = s0;
                pv[o] = s1;
            }
            if (threadIdx.x == 0) {
                float s = 0.f;
                for (int w = 0; w < NT / 64; ++w) s += redp[w];
                pp[((long)blockIdx.x * B + b) * C + c] = s;
            }
        }
    }
    if (active) {
#pragma unroll
        for (int j = 0; j < FPT; ++j) {
            const int t = t0 + j * R + r;
            if (t < T) {
                const long i = ((long)t * B + b) * M + m;
                const bool valid = t < len;
                dz[i] = valid ? __fmul_rn(sc, dza[j]) : 0.f;
                if (dls) dls[i] = valid ? -sc : 0.f;
            }
        }
    }
}

// out[b][i] = sc * sum over the utterance's chunks (those that hold a valid frame), in chunk order
__global__ void mixture_bwd_reduce_k(const float* __restrict__ pm, const float* __restrict__ pv, const float* __restrict__ pp,
                                     const int* __restrict__ lens, const float* __restrict__ acc, const float* __restrict__ g,
                                     float* __restrict__ dmean, float* __restrict__ dlog_var, float* __restrict__ dprob,
                                     int T, int B, int M, int C, int CH) {
    const float sc = g[0] * acc[4];
    const long per = (long)M * C, n_mc = (long)B * per, n_p = (long)B * C;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n_mc + n_p; i += (long)gridDim.x * blockDim.x) {
        const bool is_p = i >= n_mc;
        const long e = is_p ? i - n_mc : i;
        const int b = (int)(is_p ? e / C : e / per);
        const int nk = (clamp_len(lens[b], T) + CH - 1) / CH;
        if (is_p) {
            if (!dprob) continue;
            float s = 0.f;
            for (int k = 0; k < nk; ++k) s += pp[k * n_p + e];
            dprob[e] = sc * s;
        } else {
            float s0 = 0.f, s1 = 0.f;
            for (int k = 0; k < nk; ++k) { s0 += pm[k * n_mc + e]; s1 += pv[k * n_mc + e]; }
            if (dmean) dmean[e] = sc * s0;
            if (dlog_var) dlog_var[e] = sc * s1;
        }
    }
}

// ---------------- time pooling (flowtron.py:437-439): the divisor is the batch's longest length ----------------
__device__ __forceinline__ int block_max_len(const int* __restrict__ lens, int T, int B, int* red) {
    int v = 0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) { const int l = clamp_len(lens[b], T); v = l > v ? l : v; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    int r = 0;
    for (int i = 0; i < (int)(blockDim.x + 63) / 64; ++i) r = red[i] > r ? red[i] : r;
    return r;
}

// grid (ceil(W / 64), B), 64 channels x 4 time slices per workgroup; the slices are added in slice order
__global__ void __launch_bounds__(NT) time_pool_fwd_k(const float* __restrict__ x, const int* __restrict__ lens, float* __restrict__ y,
                                                      int T, int B, int W) {
    __shared__ int redi[NT / 64];
    __shared__ float red[4][64];
    const int mx = block_max_len(lens, T, B, redi);
    const int b = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63), s = threadIdx.x >> 6;
    const int len = clamp_len(lens[b], T);
    float v = 0.f;
    if (c < W)
        for (int t = s; t < len; t += 4) v += x[((long)t * B + b) * W + c];
    red[s][threadIdx.x & 63] = v;
    __syncthreads();
    if (s == 0 && c < W) {
        const float sum = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
        y[(long)b * W + c] = mx > 0 ? sum / (float)mx : 0.f;
    }
}

__global__ void __launch_bounds__(NT) time_pool_bwd_k(const float* __restrict__ dy, const int* __restrict__ lens, float* __restrict__ dx,
                                                      int T, int B, int W) {
    __shared__ int redi[NT / 64];
    const int mx = block_max_len(lens, T, B, redi);
    const long total = (long)T * B * W;
    for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const long row = i / W;
        const int c = (int)(i - row * W);
        const int t = (int)(row / B), b = (int)(row - (long)t * B);
        dx[i] = t < clamp_len(lens[b], T) ? dy[(long)b * W + c] / (float)mx : 0.f;
    }
}

// ---------------- softmax over the C <= 64 components of a row: one wave per row ----------------
__global__ void __launch_bounds__(NT) softmax_rows_fwd_k(const float* __restrict__ x, float* __restrict__ y, int B, int C) {
    const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const float v = lane < C ? x[(long)row * C + lane] : -INFINITY;
    const float mx = wave_max(v);
    const float e = lane < C ? expf(__fsub_rn(v, mx)) : 0.f;
    const float s = wave_sum(e);
    if (lane < C) y[(long)row * C + lane] = e / s;
}

// dx = y (dy - sum_c y_c dy_c)
__global__ void __launch_bounds__(NT) softmax_rows_bwd_k(const float* __restrict__ y, const float* __restrict__ dy, float* __restrict__ dx,
                                                         int B, int C) {
    const int row = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B) return;
    const float yv = lane < C ? y[(long)row * C + lane] : 0.f;
    const float gv = lane < C ? dy[(long)row * C + lane] : 0.f;
    const float s = wave_sum(__fmul_rn(yv, gv));
    if (lane < C) dx[(long)row * C + lane] = __fmul_rn(yv, __fsub_rn(gv, s));
}

// ---------------- component sampler ----------------
// out[s][m][t] = mean[row_s][m][k_s] + sigma exp(log_var[row_s][m][k_s] / 2) eps[s][m][t]; a row or component outside its range
// (they live on the device: the host cannot check them) gives NaN and reads nothing
__global__ void __launch_bounds__(NT) mixture_sample_k(const float* __restrict__ mean, const float* __restrict__ log_var,
                                                       const int* __restrict__ rows, const int* __restrict__ comp,
                                                       const float* __restrict__ eps, float* __restrict__ out, long total, int M,
                                                       int n_frames, int C, int Bm, float sigma) {
    for (long i = blockIdx.x * (long)NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const long sm_ = i / n_frames;
        const int s = (int)(sm_ / M), m = (int)(sm_ - (long)s * M);
        const int row = rows ? rows[s] : 0, k = comp[s];
        float v = NAN;
        if (row >= 0 && row < Bm && k >= 0 && k < C) {
            const long o = ((long)row * M + m) * C + k;
            v = mean[o];
            if (eps) v = __fmaf_rn(__fmul_rn(sigma, expf(__fmul_rn(0.5f, log_var[o]))), eps[i], v);
        }
        out[i] = v;
    }
}

inline int grid_for(int64_t n, int cap = 256 * 16) {
    int64_t g = (n + NT - 1) / NT;
    return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

// every check of the likelihood's geometry, on the host, before any device call
inline int mixture_geometry(const char* fn, int T, int B, int M, int C, int Bm) {
    if (!(T >= 1 && B >= 1 && B <= 65535 && M >= 1 && M <= NT)) return ft_fail(FT_EINVAL, "%s: invalid argument: T >= 1, 1 <= B <= 65535, 1 <= M <= %d", fn, NT);
    if (!(C >= 2 && C <= FT_MIXTURE_MAX_C)) return ft_fail(FT_EINVAL, "%s: invalid argument: 2 <= C <= %d, got %d", fn, FT_MIXTURE_MAX_C, C);
    if (!(Bm == 1 || Bm == B)) return ft_fail(FT_EINVAL, "%s: invalid argument: mean / log_var rows Bm must be 1 or B = %d, got %d", fn, B, Bm);
    if (consts_bytes(M, C) > LDS_CONSTS_MAX) return ft_fail(FT_EINVAL, "%s: invalid argument: M * C = %d: the constants need %zu bytes of LDS, %zu are there", fn, M * C, consts_bytes(M, C), LDS_CONSTS_MAX);
    return FT_OK;
}

}  // namespace

#define ST(s) reinterpret_cast<hipStream_t>(s)

extern "C" size_t ft_mixture_nll_work_floats(int T, int B, int M, int C) {
    if (T < 1 || B < 1 || M < 1 || M > NT || C < 1) return 0;
    const size_t nk = (size_t)cdiv(T, chunk_frames(M));
    return nk * B * ((size_t)2 * M * C + C);
}

extern "C" int ft_mixture_nll_fwd(const float* z, const float* mean, const float* log_var, const float* prob, const float* const* log_s,
                                  int n_ls, int64_t ld_ls, const int32_t* out_lens, float* acc, float* work, float* loss_out,
                                  int T, int B, int M, int C, int Bm, void* stream) {
    FT_CHECK_ARG(z && mean && log_var && prob && out_lens && acc && work && loss_out);
    if (int rc = mixture_geometry(__func__, T, B, M, C, Bm)) return rc;
    FT_CHECK_ARG(n_ls >= 0 && n_ls <= MAX_LS && (n_ls == 0 || (log_s && ld_ls >= M)));
    LsPtrs ls{};
    for (int f = 0; f < n_ls; ++f) { FT_CHECK_ARG(log_s[f] != nullptr); ls.p[f] = log_s[f]; }
    const int nk = cdiv(T, chunk_frames(M));
    hipLaunchKernelGGL(mixture_nll_fwd_k, dim3(nk, B), dim3(NT), consts_bytes(M, C), ST(stream), z, mean, log_var, prob, ls, n_ls,
                       (long)ld_ls, out_lens, work, T, B, M, C, Bm);
    hipLaunchKernelGGL(mixture_nll_finalize_k, dim3(1), dim3(NT), 0, ST(stream), work, nk * B, out_lens, T, B, M, acc, loss_out);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_mixture_nll_bwd(const float* z, const float* mean, const float* log_var, const float* prob, const int32_t* out_lens,
                                  const float* acc, const float* g, float* dz, float* dls, float* dmean, float* dlog_var, float* dprob,
                                  float* work, int T, int B, int M, int C, int Bm, void* stream) {
    FT_CHECK_ARG(z && mean && log_var && prob && out_lens && acc && g && dz);
    if (int rc = mixture_geometry(__func__, T, B, M, C, Bm)) return rc;
    const bool want = dmean || dlog_var || dprob;
    FT_CHECK_ARG(!want || work);
    const int nk = cdiv(T, chunk_frames(M));
    const size_t n_mc = (size_t)nk * B * M * C;
    float *pm = work, *pv = work ? work + n_mc : nullptr, *pp = work ? work + 2 * n_mc : nullptr;
    if (want) {
        hipLaunchKernelGGL(mixture_nll_bwd_k<true>, dim3(nk, B), dim3(NT), consts_bytes(M, C), ST(stream), z, mean, log_var, prob,
                           out_lens, acc, g, dz, dls, pm, pv, pp, T, B, M, C, Bm);
        hipLaunchKernelGGL(mixture_bwd_reduce_k, dim3(grid_for((int64_t)B * M * C + (int64_t)B * C)), dim3(NT), 0, ST(stream), pm, pv, pp,
                           out_lens, acc, g, dmean, dlog_var, dprob, T, B, M, C, chunk_frames(M));
    } else {
        hipLaunchKernelGGL(mixture_nll_bwd_k<false>, dim3(nk, B), dim3(NT), consts_bytes(M, C), ST(stream), z, mean, log_var, prob,
                           out_lens, acc, g, dz, dls, pm, pv, pp, T, B, M, C, Bm);
    }
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_time_pool_fwd(const float* x, const int32_t* lens, float* y, int T, int B, int W, void* stream) {
    FT_CHECK_ARG(x && lens && y && T >= 1 && B >= 1 && B <= 65535 && W >= 1);
    hipLaunchKernelGGL(time_pool_fwd_k, dim3(cdiv(W, 64), B), dim3(NT), 0, ST(stream), x, lens, y, T, B, W);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_time_pool_bwd(const float* dy, const int32_t* lens, float* dx, int T, int B, int W, void* stream) {
    FT_CHECK_ARG(dy && lens && dx && T >= 1 && B >= 1 && B <= 65535 && W >= 1);
    hipLaunchKernelGGL(time_pool_bwd_k, dim3(grid_for((int64_t)T * B * W)), dim3(NT), 0, ST(stream), dy, lens, dx, T, B, W);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_softmax_rows_fwd(const float* x, float* y, int B, int C, void* stream) {
    FT_CHECK_ARG(x && y && B >= 1);
    FT_CHECK_ARG(C >= 2 && C <= FT_MIXTURE_MAX_C);
    hipLaunchKernelGGL(softmax_rows_fwd_k, dim3(cdiv(B, NT / 64)), dim3(NT), 0, ST(stream), x, y, B, C);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_softmax_rows_bwd(const float* y, const float* dy, float* dx, int B, int C, void* stream) {
    FT_CHECK_ARG(y && dy && dx && B >= 1);
    FT_CHECK_ARG(C >= 2 && C <= FT_MIXTURE_MAX_C);
    hipLaunchKernelGGL(softmax_rows_bwd_k, dim3(cdiv(B, NT / 64)), dim3(NT), 0, ST(stream), y, dy, dx, B, C);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_mixture_sample(const float* mean, const float* log_var, const int32_t* rows, const int32_t* component, const float* eps,
                                 float* out, int S, int M, int n_frames, int C, int Bm, float sigma, void* stream) {
    FT_CHECK_ARG(mean && log_var && component && out);
    FT_CHECK_ARG(S >= 1 && M >= 1 && n_frames >= 1 && Bm >= 1);
    FT_CHECK_ARG(C >= 2 && C <= FT_MIXTURE_MAX_C);
    FT_CHECK_ARG(rows || Bm == 1);
    FT_CHECK_ARG(eps || sigma == 0.f);
    FT_CHECK_ARG(sigma >= 0.f);
    const int64_t total = (int64_t)S * M * n_frames;
    hipLaunchKernelGGL(mixture_sample_k, dim3(grid_for(total)), dim3(NT), 0, ST(stream), mean, log_var, rows, component, eps, out,
                       (long)total, M, n_frames, C, Bm, sigma);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
