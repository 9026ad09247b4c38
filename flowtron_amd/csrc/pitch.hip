// F0 tracking (YIN) and F0 error along a warping path (additive: the reference has no pitch tracker and no metric).
//
// ft_f0_yin_ragged: per utterance b, T_b = n_samples[b] / hop + 1 frames; frame t reads x[t hop - W/2 + j], 0 <= j < W + tau_max + 1,
// zero outside 0 .. n_samples[b] - 1 (that memory is never touched):
//     d(tau) = sum_{j < W} (x[j] - x[j + tau])^2        tau = 0 .. tau_max + 1; j ascending; sub, mul, add: one fp32 rounding each
//     s(tau) = s(tau - 1) + d(tau), s(0) = 0;   d'(0) = 1, d'(tau) = (d(tau) * float(tau)) / s(tau) where s(tau) > 0, else 1
//     tau = the lowest lag in tau_min ..= tau_max with d'(tau) < threshold, then upwards while d'(tau + 1) < d'(tau)
//     voiced: f0 = sr / (float(tau) + shift), the parabola through d'(tau - 1), d'(tau), d'(tau + 1); aperiodicity d'(tau)
//     unvoiced: f0 = 0, aperiodicity = the least d' in tau_min ..= tau_max
//   * a workgroup owns FPW consecutive frames of one utterance; each frame's window waits in LDS at a 16-byte aligned base.
//     G = ceil((tau_max + 2) / 4) threads share a frame, thread g owns the lags 4 g .. 4 g + 3 and walks j in ascending order
//     four at a time: one broadcast 16-byte read of x[j .. j + 3] and one 16-byte read of x[j + 4 g + 4 .. + 7] (the four
//     before it stay in registers from the step before) feed 16 difference / square / add triples.
//   * the running sum s is 369 dependent adds at the default lags: thread 0 of every frame does it from LDS while the other
//     waves of the CU work on other frames; it is not a parallel scan, whose sums would round differently.  d' is formed by
//     every thread from the d it still holds in registers.
//   * the search is a wave's: lanes stride over the lags, first-below-threshold and the least d' are index / value minima
//     over lanes, the walk to the local minimum is uniform.
//   * a frame whose window holds a non-finite sample is flagged while it is staged and gives f0 = 0, aperiodicity 1.
//   * n_samples is clamped to 1 ..= N in the kernel, every sample index is bounded by it, addressing with B, N is 64-bit.
//     No atomics, no scratch, no communication between workgroups.
//
// ft_f0_path_stats: per pair, over the cells (i, j) of a warping path: how many have both frames voiced (f0 > 0), how many
// exactly one, and the float64 sum of (1200 log2(f0_a[i] / f0_b[j]))^2 over the former.  One workgroup per pair, a thread
// sums its cells in ascending order and the partial sums meet in a fixed tree: the same bits on every call.
#include "common.h"

// the float32 replay on the host rounds every operation on its own (dtw.hip)
#pragma clang fp contract(off)

namespace {

constexpr int YIN_MAX_W = 2048;
constexpr int YIN_MAX_LAG = 1022;               // tau_max: tau_max + 2 lags, four to a thread, at most 256 threads a frame
constexpr int YIN_MAX_FPW = 16;
constexpr int YIN_LDS_BYTES = 60 * 1024;
constexpr int STATS_THREADS = 256;

struct YinArgs {
    const float* audio;
    int64_t sb, sn;                             // element strides of (utterance, sample)
    const int32_t* n_samples;
    float* f0;                                  // [B][T]
    float* ap;                                  // [B][T]
    float sr, threshold;
    int N, T, hop, W, tau_min, tau_max;
    int G, FPW, FS, DS;                         // threads and frames of the layout; floats per staged window and per lag array
};

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// NJ values of j from j0 on: x[j0 .. j0 + 3] against the seven values x[j0 + tau0 .. j0 + tau0 + 6]
template <int NJ>
__device__ __forceinline__ void yin_step(const f32x4 a, const f32x4 lo, const f32x4 hi, float (&acc)[4]) {
    const float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const float df = a[jj] - v[jj + l];
            acc[l] = acc[l] + df * df;
        }
    }
}

__global__ __launch_bounds__(1024) void yin_k(YinArgs p) {
    extern __shared__ __align__(16) float smem[];
    float* xs_all = smem;                                           // [FPW][FS] the windows
    float* dp_all = xs_all + p.FPW * p.FS;                          // [FPW][DS] d, then d'
    float* ss_all = dp_all + p.FPW * p.DS;                          // [FPW][DS] s
    int* flag = reinterpret_cast<int*>(ss_all + p.FPW * p.DS);      // [FPW] the window holds a non-finite sample

    const int b = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x;
    const int n = min(max(p.n_samples[b], 1), p.N);
    const int Tb = n / p.hop + 1;
    const int t0 = blockIdx.x * p.FPW;                              // this workgroup's first frame (< T by the grid)
    float* f0 = p.f0 + (int64_t)b * p.T;
    float* ap = p.ap + (int64_t)b * p.T;
    if (t0 >= Tb) {                                                 // (uniform over the workgroup) behind the utterance
        if (tid < p.FPW && t0 + tid < p.T) { f0[t0 + tid] = 0.f; ap[t0 + tid] = 0.f; }
        return;
    }

    if (tid < p.FPW) flag[tid] = 0;
    __syncthreads();
    const int span = p.W + p.tau_max + 1;
    const float* x = p.audio + b * p.sb;
    for (int e = tid; e < p.FPW * p.FS; e += nthr) {
        const int f = e / p.FS, i = e - f * p.FS;
        const int t = t0 + f;
        float v = 0.f;
        if (t < Tb && i < span) {
            const int64_t k = (int64_t)t * p.hop - p.W / 2 + i;
            if (k >= 0 && k < n) {
                v = x[k * p.sn];
                if (!(fabsf(v) < INFINITY)) flag[f] = 1;            // (every writer stores the same value)
            }
        }
        xs_all[e] = v;
    }
    __syncthreads();

    const int f = tid / p.G, g = tid - f * p.G;
    const bool mine = f < p.FPW && t0 + f < Tb;                     // this thread has a frame and four lags of it
    const int tau0 = 4 * g;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    if (mine) {
        const float* xs = xs_all + f * p.FS;
        const f32x4* xa = reinterpret_cast<const f32x4*>(xs);
        const f32x4* xv = reinterpret_cast<const f32x4*>(xs + tau0);
        const int W4 = p.W >> 2;
        f32x4 lo = xv[0];
        for (int q = 0; q < W4; ++q) {
            const f32x4 a = xa[q], hi = xv[q + 1];
            yin_step<4>(a, lo, hi, acc);
            lo = hi;
        }
        if (p.W & 2) yin_step<2>(xa[W4], lo, xv[W4 + 1], acc);      // W is even
        *reinterpret_cast<f32x4*>(dp_all + f * p.DS + tau0) = f32x4{acc[0], acc[1], acc[2], acc[3]};
    }
    __syncthreads();

    if (mine && g == 0) {                                           // the running sum, in order, on one thread a frame
        const float* dp = dp_all + f * p.DS;
        float* ss = ss_all + f * p.DS;
        float s = 0.f;
        ss[0] = 0.f;
        for (int q = 0; q < p.DS; q += 4) {
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(dp + q);
            f32x4 s4;
            if (q == 0) s4[0] = 0.f; else { s = s + d4[0]; s4[0] = s; }
            s = s + d4[1]; s4[1] = s;
            s = s + d4[2]; s4[2] = s;
            s = s + d4[3]; s4[3] = s;
            *reinterpret_cast<f32x4*>(ss + q) = s4;
        }
    }
    __syncthreads();

    if (mine) {
        const f32x4 s4 = *reinterpret_cast<const f32x4*>(ss_all + f * p.DS + tau0);
        f32x4 r;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const int tau = tau0 + l;
            r[l] = (tau > 0 && s4[l] > 0.f) ? (acc[l] * (float)tau) / s4[l] : 1.f;
        }
        *reinterpret_cast<f32x4*>(dp_all + f * p.DS + tau0) = r;
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
    for (int fr = wave; fr < p.FPW; fr += nw) {                     // (uniform over the wave) a wave searches a frame
        const int t = t0 + fr;
        if (t >= p.T) break;
        float out_f = 0.f, out_a = 0.f;
        if (t < Tb) {
            const float* dp = dp_all + fr * p.DS;
            int first = 0x7fffffff;
            float least = INFINITY;
            for (int tau = p.tau_min + lane; tau <= p.tau_max; tau += 64) {
                const float v = dp[tau];
                if (v < p.threshold) first = min(first, tau);
                least = v < least ? v : least;
            }
            first = wave_min_i(first);
            least = wave_min_f(least);
            out_a = least;
            if (first != 0x7fffffff) {
                int tau = first;
                while (tau < p.tau_max && dp[tau + 1] < dp[tau]) ++tau;
                const float a = dp[tau - 1], bb = dp[tau], c = dp[tau + 1];
                const float den = (a + c) - 2.f * bb;
                float shift = 0.f;
                if (a >= bb && c >= bb && den > 0.f) shift = (0.5f * (a - c)) / den;
                out_f = p.sr / ((float)tau + shift);
                out_a = bb;
            }
            if (flag[fr]) { out_f = 0.f; out_a = 1.f; }
        }
        if (lane == 0) { f0[t] = out_f; ap[t] = out_a; }
    }
}

struct StatsArgs {
    const float* fa;
    int64_t sab, sat;
    const float* fb;
    int64_t sbb, sbt;
    const int32_t* path;                        // [B][P][2]
    const int32_t* path_len;                    // [B]
    int32_t* n_both;                            // [B]
    int32_t* n_mismatch;                        // [B]
    double* sum_sq;                             // [B]
    int Ta, Tb, P;
};

__global__ __launch_bounds__(STATS_THREADS) void f0_path_stats_k(StatsArgs p) {
    __shared__ double sq[STATS_THREADS];
    __shared__ int nb[STATS_THREADS], nm[STATS_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int len = min(max(p.path_len[b], 0), p.P);
    const int32_t* path = p.path + (int64_t)b * p.P * 2;
    const float* fa = p.fa + b * p.sab;
    const float* fb = p.fb + b * p.sbb;
    double acc = 0.0;
    int both = 0, mism = 0;
    for (int c = tid; c < len; c += STATS_THREADS) {
        const int i = min(max(path[2 * c], 0), p.Ta - 1), j = min(max(path[2 * c + 1], 0), p.Tb - 1);
        const float va = fa[i * p.sat], vb = fb[j * p.sbt];
        const bool a_on = va > 0.f, b_on = vb > 0.f;
        if (a_on && b_on) {
            const double cents = 1200.0 * log2((double)va / (double)vb);
            acc = acc + cents * cents;
            ++both;
        } else if (a_on != b_on) {
            ++mism;
        }
    }
    sq[tid] = acc;
    nb[tid] = both;
    nm[tid] = mism;
    __syncthreads();
    for (int h = STATS_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) {
            sq[tid] = sq[tid] + sq[tid + h];
            nb[tid] += nb[tid + h];
            nm[tid] += nm[tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) { p.sum_sq[b] = sq[0]; p.n_both[b] = nb[0]; p.n_mismatch[b] = nm[0]; }
}

}  // namespace

extern "C" int ft_f0_yin_ragged(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, float* f0,
                                float* aperiodicity, int B, int N, float sampling_rate, int hop, int W, int tau_min, int tau_max,
                                float threshold, void* stream) {
    FT_CHECK_ARG(audio && n_samples && f0 && aperiodicity);
    FT_CHECK_ARG(B >= 1 && N >= 1 && hop >= 1 && W >= 1);
    FT_CHECK_ARG(stride_b >= 0 && stride_n >= 0);
    FT_CHECK_ARG(B <= 65535 && N / hop < 0x7fffffff);
    FT_CHECK_ARG(sampling_rate > 0.f);
    FT_CHECK_ARG(tau_min >= 2);
    FT_CHECK_ARG(tau_max >= tau_min);
    FT_CHECK_ARG(threshold > 0.f && threshold <= 1.f);
    if (W > YIN_MAX_W || (W & 1) || tau_max > YIN_MAX_LAG)
        return ft_fail(FT_EUNSUPPORTED, "%s: window %d, lags up to %d: the tracker holds an even window of at most %d samples and lags up to %d",
                       __func__, W, tau_max, YIN_MAX_W, YIN_MAX_LAG);
    YinArgs p{audio, stride_b, stride_n, n_samples, f0, aperiodicity, sampling_rate, threshold, N, N / hop + 1, hop, W, tau_min, tau_max,
              0, 0, 0, 0};
    p.G = cdiv(tau_max + 2, 4);
    p.DS = 4 * p.G;
    p.FS = ((W + 3) & ~3) + 4 * p.G + 8;                            // the last step reads x[j + 4 g + 4 .. + 7] with j + 4 <= W + 2
    const int per_frame = (p.FS + 2 * p.DS) * (int)sizeof(float) + (int)sizeof(int);
    p.FPW = min(min(YIN_MAX_FPW, 1024 / p.G), min(YIN_LDS_BYTES / per_frame, p.T));
    if (p.FPW < 1) return ft_fail(FT_EUNSUPPORTED, "%s: a window of %d samples with %d lags does not fit the workgroup", __func__, W, tau_max + 2);
    const int threads = cdiv(p.FPW * p.G, 64) * 64;
    const size_t lds = (size_t)p.FPW * per_frame;
    hipLaunchKernelGGL(yin_k, dim3(cdiv(p.T, p.FPW), B), dim3(threads), lds, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_f0_path_stats(const float* f0_a, int64_t a_stride_b, int64_t a_stride_t, const float* f0_b, int64_t b_stride_b,
                                int64_t b_stride_t, const int32_t* path, const int32_t* path_len, int32_t* n_both, int32_t* n_mismatch,
                                double* sum_sq, int B, int Ta, int Tb, int P, void* stream) {
    FT_CHECK_ARG(f0_a && f0_b && path && path_len && n_both && n_mismatch && sum_sq);
    FT_CHECK_ARG(B >= 1 && Ta >= 1 && Tb >= 1 && P >= 1);
    FT_CHECK_ARG(a_stride_b >= 0 && a_stride_t >= 0 && b_stride_b >= 0 && b_stride_t >= 0);
    FT_CHECK_ARG(P <= Ta + Tb - 1);                                 // a monotone path has no more cells: a longer one leaves the tensors
    const StatsArgs p{f0_a, a_stride_b, a_stride_t, f0_b, b_stride_b, b_stride_t, path, path_len, n_both, n_mismatch, sum_sq, Ta, Tb, P};
    hipLaunchKernelGGL(f0_path_stats_k, dim3(B), dim3(STATS_THREADS), 0, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
