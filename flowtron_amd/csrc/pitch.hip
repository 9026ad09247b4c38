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
//
// ft_f0_candidates_ragged, ft_f0_viterbi_ragged: probabilistic YIN (Mauch & Dixon 2014) in two launches; include/flowtron_hip.h
// states the rule.  The first shares yin_k's front (yin_dprime) and gives every frame its candidate mass per pitch bin, the
// second takes one path through a voiced / unvoiced state per bin, one workgroup an utterance.  The notes stand at the kernels.
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

// The front both trackers share: stages the windows of the workgroup's frames t0 .. t0 + FPW - 1 of utterance b (n samples, Tb
// frames) and leaves d' in dp_all, s in ss_all and the non-finite flags in flag, behind a barrier.
__device__ __forceinline__ void yin_dprime(const YinArgs& p, float* xs_all, float* dp_all, float* ss_all, int* flag, int b, int n,
                                           int Tb, int t0) {
    const int tid = threadIdx.x, nthr = blockDim.x;
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
    yin_dprime(p, xs_all, dp_all, ss_all, flag, b, n, Tb, t0);

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

// ---- probabilistic YIN: candidates per frame, then one path through a voiced / unvoiced pitch HMM ----------------------------
constexpr int PYIN_MAX_BINS = 512;              // two states a bin, a lane a state
constexpr int PYIN_MAX_BAND = 63;               // 2 band + 1 offsets and the voicing share a byte
constexpr int PYIN_THRESHOLDS = 100;
constexpr float PYIN_FLOOR = 9.5367431640625e-07f;          // 2^-20: the least observation
constexpr float PYIN_CUT = 5.421010862427522e-20f;          // 2^-64: scores below it are 0, so nothing ever reaches a denormal
constexpr float PYIN_MIN_SWITCH = 9.5367431640625e-07f;     // 2^-20 <= switch_prob <= 1 - 2^-20, for the same reason

struct PyinArgs {
    YinArgs y;                                  // the windows and the layout (f0, ap and threshold are not used)
    const float* cum;                           // [101] the Beta prior summed up to threshold i / 100
    const float* edges;                         // [n_bins + 1] the bins' edges as lags, descending
    float* prob;                                // [B][T][n_bins]
    float* freq;                                // [B][T][n_bins]
    float* voiced;                              // [B][T]
    float amp;                                  // absolute_min_prob
    int n_bins;
};

// how many of the thresholds float(i) / 100, i = 1 .. 100, lie at or below v (v >= 0, +inf included)
__device__ __forceinline__ int thresholds_at_or_below(float v) {
    int k = (int)fminf(v * 100.f, 100.f);
    while (k < PYIN_THRESHOLDS && (float)(k + 1) / 100.f <= v) ++k;
    while (k > 0 && (float)k / 100.f > v) --k;
    return k;
}

// bin k holds edges[k + 1] < lag <= edges[k]; -1 outside the bins
__device__ __forceinline__ int lag_bin(const float* edges, int n_bins, float lag) {
    if (!(lag <= edges[0]) || !(lag > edges[n_bins])) return -1;
    int lo = 0, hi = n_bins;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (lag <= edges[mid]) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ float refined_lag(const float* dp, int tau) {
    const float a = dp[tau - 1], bb = dp[tau], c = dp[tau + 1];
    const float den = (a + c) - 2.f * bb;
    float shift = 0.f;
    if (a >= bb && c >= bb && den > 0.f) shift = (0.5f * (a - c)) / den;
    return (float)tau + shift;
}

__device__ __forceinline__ bool is_trough(const float* dp, int tau) {
    const float v = dp[tau];
    return v <= dp[tau - 1] && v < dp[tau + 1];
}

// The front is yin_k's (same layout, same LDS).  Then a wave owns a frame: lane l walks the C = ceil(lags / 64) consecutive lags
// from tau_min + l C, so "lower than every earlier trough" is an exclusive prefix minimum over the lanes (a minimum is exact in
// any order) followed by each lane's own walk.  The candidates go, in lag order, into a list that overlays the frame's window
// and s (both dead by then), the global minimum behind them; then lane l sums the list into the bins l, l + 64, ..: every
// bin has one owner, so there is nothing to make atomic, and the lanes' partial sums are the 64 terms of the voiced mass.
__global__ __launch_bounds__(1024) void pyin_candidates_k(PyinArgs q) {
    const YinArgs& p = q.y;
    extern __shared__ __align__(16) float smem[];
    float* xs_all = smem;
    float* dp_all = xs_all + p.FPW * p.FS;
    float* ss_all = dp_all + p.FPW * p.DS;
    int* flag = reinterpret_cast<int*>(ss_all + p.FPW * p.DS);

    const int b = blockIdx.y, tid = threadIdx.x, nthr = blockDim.x, nb = q.n_bins;
    const int n = min(max(p.n_samples[b], 1), p.N);
    const int Tb = n / p.hop + 1;
    const int t0 = blockIdx.x * p.FPW;
    float* prob = q.prob + (int64_t)b * p.T * nb;
    float* freq = q.freq + (int64_t)b * p.T * nb;
    float* voiced = q.voiced + (int64_t)b * p.T;
    if (t0 >= Tb) {                                                 // (uniform over the workgroup) behind the utterance
        const int nf = min(p.FPW, p.T - t0);
        for (int e = tid; e < nf * nb; e += nthr) { prob[(int64_t)t0 * nb + e] = 0.f; freq[(int64_t)t0 * nb + e] = 0.f; }
        if (tid < nf) voiced[t0 + tid] = 0.f;
        return;
    }
    yin_dprime(p, xs_all, dp_all, ss_all, flag, b, n, Tb, t0);

    const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
    const int nl = p.tau_max - p.tau_min + 1, C = (nl + 63) >> 6;
    const int EM = nl / 2 + 2;                                      // no two troughs are neighbours: ceil(nl / 2) candidates and the global minimum
    for (int fr0 = 0; fr0 < p.FPW; fr0 += nw) {                     // (uniform over the workgroup: every wave meets the barriers)
        const int fr = min(fr0 + wave, p.FPW - 1), t = t0 + fr0 + wave;
        const bool have = fr0 + wave < p.FPW && t < p.T;
        const float* dp = dp_all + fr * p.DS;
        float* ew = ss_all + fr * p.DS;                             // [EM] weights
        float* ef = xs_all + fr * p.FS;                             // [EM] frequencies
        int* eb = reinterpret_cast<int*>(ef + EM);                  // [EM] bins, -1 = dropped
        // mass only for a frame of the utterance with finite samples that is not digital silence (s is ascending)
        const bool ok = have && t < Tb && !flag[fr] && ss_all[fr * p.DS + p.tau_max + 1] > 0.f;
        const int lo = p.tau_min + lane * C, hi = min(lo + C - 1, p.tau_max);

        float tmin = INFINITY, least = INFINITY;
        int glag = 0x7fffffff;
        if (ok) {
            for (int tau = lo; tau <= hi; ++tau) {
                const float v = dp[tau];
                if (is_trough(dp, tau)) tmin = v < tmin ? v : tmin;
                if (v < least) { least = v; glag = tau; }
            }
        }
        float inc = tmin;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float o = __shfl_up(inc, off, 64);
            if (lane >= off && o < inc) inc = o;
        }
        float rec = __shfl_up(inc, 1, 64);                          // the lowest trough of the lanes before this one
        if (lane == 0) rec = INFINITY;
        const float gmin = wave_min_f(least);
        const int gtau = wave_min_i(least == gmin ? glag : 0x7fffffff);   // its lowest lag

        int cnt = 0;
        if (ok) {
            float r = rec;
            for (int tau = lo; tau <= hi; ++tau)
                if (is_trough(dp, tau) && dp[tau] < r) { r = dp[tau]; ++cnt; }
        }
        int pos = cnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(pos, off, 64);
            if (lane >= off) pos += o;
        }
        int E = __shfl(pos, 63, 64);
        pos -= cnt;
        __syncthreads();                                            // s has been read: its place takes the list

        if (ok) {
            float r = rec;
            for (int tau = lo; tau <= hi; ++tau) {
                const float v = dp[tau];
                if (is_trough(dp, tau) && v < r) {
                    const float w = q.cum[thresholds_at_or_below(r)] - q.cum[thresholds_at_or_below(v)];
                    const float lag = refined_lag(dp, tau);
                    ew[pos] = w;
                    ef[pos] = p.sr / lag;
                    eb[pos] = w > 0.f ? lag_bin(q.edges, nb, lag) : -1;
                    ++pos;
                    r = v;
                }
            }
            if (gtau != 0x7fffffff) {
                if (lane == 0) {
                    const float w = q.amp * q.cum[thresholds_at_or_below(gmin)];
                    const float lag = refined_lag(dp, gtau);
                    ew[E] = w;
                    ef[E] = p.sr / lag;
                    eb[E] = w > 0.f ? lag_bin(q.edges, nb, lag) : -1;
                }
                ++E;
            }
        }
        __syncthreads();

        if (have) {
            float psum = 0.f;
            for (int k = lane; k < nb; k += 64) {
                float sum = 0.f, bw = 0.f, bf = 0.f;
                for (int e = 0; e < E; ++e) {
                    if (eb[e] == k) {
                        const float w = ew[e];
                        sum = sum + w;
                        if (w > bw) { bw = w; bf = ef[e]; }
                    }
                }
                prob[(int64_t)t * nb + k] = sum;
                freq[(int64_t)t * nb + k] = bf;
                psum = psum + sum;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) psum = psum + __shfl_down(psum, off, 64);
            if (lane == 0) voiced[t] = psum;
        }
    }
}

struct ViterbiArgs {
    const float* prob;                          // [B][T][n_bins]
    const float* freq;                          // [B][T][n_bins]
    const float* voiced;                        // [B][T]
    const int32_t* n_samples;
    const float* tri;                           // [2 band + 1]
    const float* centre;                        // [n_bins]
    float* f0;                                  // [B][T]
    uint8_t* bp;                                // [B][T][2 n_bins] (offset << 1 | voicing) of the predecessor
    float stay, sw;
    int N, T, hop, n_bins, band, SPs;
};

// One workgroup an utterance, lane 2 k + x the state (bin k, x = 1 voiced).  The scores of two frames alternate in LDS, each
// voicing's row padded with band zeros on both sides (row stride = 32 mod 64 floats: the two rows a wave reads lie in
// different banks); the frame's power-of-two scale is applied a frame late, from the waves' maxima that went to LDS before
// the barrier, so one barrier a frame is enough.  A pair of lanes shares the two band maxima of its bin through a shuffle.
__global__ __launch_bounds__(1024) void pyin_viterbi_k(ViterbiArgs p) {
    extern __shared__ __align__(16) float smem[];
    const int SPs = p.SPs, band = p.band, nb = p.n_bins, no = 2 * band + 1;
    float* S = smem;                                                // [2 frames][2 voicings][SPs]
    float* tri = S + 4 * SPs;                                       // [128]
    float* wm = tri + 128;                                          // [2 frames][16 waves] maxima
    int* wi = reinterpret_cast<int*>(wm + 32);                      // [16]

    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
    const int n = min(max(p.n_samples[b], 1), p.N);
    const int Tb = n / p.hop + 1;
    const int x = tid & 1;
    const bool live = (tid >> 1) < nb;
    const int k = live ? tid >> 1 : 0;
    const float* prob = p.prob + (int64_t)b * p.T * nb;
    const float* freq = p.freq + (int64_t)b * p.T * nb;
    const float* voiced = p.voiced + (int64_t)b * p.T;
    uint8_t* bp = p.bp + (int64_t)b * p.T * 2 * nb;
    float* f0 = p.f0 + (int64_t)b * p.T;

    for (int i = tid; i < 4 * SPs; i += nthr) S[i] = 0.f;
    for (int i = tid; i < 128; i += nthr) tri[i] = i < no ? p.tri[i] : 0.f;
    __syncthreads();

    float nxt_p = x ? prob[k] : 0.f, nxt_v = voiced[0];
    float raw = 0.f;
    for (int t = 0; t < Tb; ++t) {
        const int cur = t & 1;
        const float pv = nxt_p, vp = nxt_v;
        if (t + 1 < Tb) {                                           // the next frame's observation is under way during this one
            nxt_p = x ? prob[(int64_t)(t + 1) * nb + k] : 0.f;
            nxt_v = voiced[t + 1];
        }
        float obs = pv;
        if (!x) {
            float u = 1.f - vp;
            u = u < 0.f ? 0.f : u;
            obs = u / (float)nb;
        }
        obs = obs < PYIN_FLOOR ? PYIN_FLOOR : obs;
        if (t == 0) {
            raw = obs;
        } else {
            const float* wmp = wm + 16 * (cur ^ 1);
            float m = wmp[0];
            for (int i = 1; i < nw; ++i) m = wmp[i] > m ? wmp[i] : m;
            const float scale = __int_as_float((254 - ((__float_as_int(m) >> 23) & 0xff)) << 23);   // m in [2^e, 2^(e + 1)): 2^-e
            const float* sp = S + ((cur ^ 1) * 2 + x) * SPs + k;    // sp[o]: bin k + o - band
            // eight offsets at a time: a multiply and a maximum each (a maximum is exact), one compare per eight; then the
            // lowest offset of the winning eight whose product is the maximum.  Behind 2 band the triangle is 0 and the row
            // holds zeros: such a product is 0 and takes no maximum from a real one (the products are >= 0)
            float A = -1.f;
            int bc = 0;
            for (int c0 = 0; c0 < no; c0 += 8) {
                float m = sp[c0] * tri[c0];
#pragma unroll
                for (int i = 1; i < 8; ++i) m = __builtin_fmaxf(m, sp[c0 + i] * tri[c0 + i]);
                if (m > A) { A = m; bc = c0; }
            }
            int bo = bc + 7;
#pragma unroll
            for (int i = 6; i >= 0; --i)
                if (sp[bc + i] * tri[bc + i] == A) bo = bc + i;
            const float Ao = __shfl_xor(A, 1, 64);
            const int boo = __shfl_xor(bo, 1, 64);
            const float keep = A * p.stay, chg = Ao * p.sw;
            const bool change = chg > keep;
            raw = ((change ? chg : keep) * scale) * obs;
            if (raw < PYIN_CUT) raw = 0.f;
            if (live) bp[(int64_t)t * 2 * nb + tid] = (uint8_t)(((change ? boo : bo) << 1) | (change ? x ^ 1 : x));
        }
        if (!live) raw = 0.f;
        if (live) S[(cur * 2 + x) * SPs + band + k] = raw;
        float wmax = raw;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float o = __shfl_xor(wmax, off, 64);
            wmax = o > wmax ? o : wmax;
        }
        if (lane == 0) wm[16 * cur + wave] = wmax;
        __syncthreads();
    }

    // the best final state, the lowest of equals; then one thread walks back and leaves the states where the F0 will stand
    const float* wml = wm + 16 * ((Tb - 1) & 1);
    float m = wml[0];
    for (int i = 1; i < nw; ++i) m = wml[i] > m ? wml[i] : m;
    const int mine = wave_min_i(live && raw == m ? tid : 0x7fffffff);
    if (lane == 0) wi[wave] = mine;
    __syncthreads();
    if (tid == 0) {
        int j = wi[0];
        for (int i = 1; i < nw; ++i) j = min(j, wi[i]);
        j = min(j, 2 * nb - 1);
        for (int t = Tb - 1;; --t) {
            f0[t] = __int_as_float(j);
            if (t == 0) break;
            const int code = bp[(int64_t)t * 2 * nb + j];
            const int kk = min(max((j >> 1) + (code >> 1) - band, 0), nb - 1);
            j = 2 * kk + (code & 1);
        }
    }
    __syncthreads();
    for (int t = tid; t < p.T; t += nthr) {
        float out = 0.f;
        if (t < Tb) {
            const int j = __float_as_int(f0[t]);
            if (j & 1) {
                const float fr = freq[(int64_t)t * nb + (j >> 1)];
                out = fr > 0.f ? fr : p.centre[j >> 1];
            }
        }
        f0[t] = out;
    }
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

extern "C" int ft_f0_candidates_ragged(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, const float* cum,
                                       const float* lag_edges, float* prob, float* freq, float* voiced_prob, int B, int N,
                                       float sampling_rate, int hop, int W, int tau_min, int tau_max, int n_bins,
                                       float absolute_min_prob, void* stream) {
    FT_CHECK_ARG(audio && n_samples && cum && lag_edges && prob && freq && voiced_prob);
    FT_CHECK_ARG(B >= 1 && N >= 1 && hop >= 1 && W >= 1 && n_bins >= 1);
    FT_CHECK_ARG(stride_b >= 0 && stride_n >= 0);
    FT_CHECK_ARG(B <= 65535 && N / hop < 0x7fffffff);
    FT_CHECK_ARG(sampling_rate > 0.f);
    FT_CHECK_ARG(tau_min >= 2);
    FT_CHECK_ARG(tau_max >= tau_min);
    FT_CHECK_ARG(absolute_min_prob >= 0.f && absolute_min_prob <= 1.f);
    if (W > YIN_MAX_W || (W & 1) || tau_max > YIN_MAX_LAG || n_bins > PYIN_MAX_BINS)
        return ft_fail(FT_EUNSUPPORTED, "%s: window %d, lags up to %d, %d bins: the tracker holds an even window of at most %d samples, lags up to %d and %d bins",
                       __func__, W, tau_max, n_bins, YIN_MAX_W, YIN_MAX_LAG, PYIN_MAX_BINS);
    PyinArgs q{{audio, stride_b, stride_n, n_samples, nullptr, nullptr, sampling_rate, 0.f, N, N / hop + 1, hop, W, tau_min, tau_max, 0, 0, 0, 0},
               cum, lag_edges, prob, freq, voiced_prob, absolute_min_prob, n_bins};
    YinArgs& p = q.y;                                               // the layout of ft_f0_yin_ragged
    p.G = cdiv(tau_max + 2, 4);
    p.DS = 4 * p.G;
    p.FS = ((W + 3) & ~3) + 4 * p.G + 8;
    const int per_frame = (p.FS + 2 * p.DS) * (int)sizeof(float) + (int)sizeof(int);
    p.FPW = min(min(YIN_MAX_FPW, 1024 / p.G), min(YIN_LDS_BYTES / per_frame, p.T));
    if (p.FPW < 1) return ft_fail(FT_EUNSUPPORTED, "%s: a window of %d samples with %d lags does not fit the workgroup", __func__, W, tau_max + 2);
    const int threads = cdiv(p.FPW * p.G, 64) * 64;
    const size_t lds = (size_t)p.FPW * per_frame;
    hipLaunchKernelGGL(pyin_candidates_k, dim3(cdiv(p.T, p.FPW), B), dim3(threads), lds, reinterpret_cast<hipStream_t>(stream), q);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" size_t ft_f0_viterbi_workspace_bytes(int B, int T, int n_bins) {
    if (B < 1 || T < 1 || n_bins < 1) return 0;
    return (size_t)B * (size_t)T * 2 * (size_t)n_bins;
}

extern "C" int ft_f0_viterbi_ragged(const float* prob, const float* freq, const float* voiced_prob, const int32_t* n_samples,
                                    const float* transition, const float* centres, float* f0, void* work, size_t work_bytes, int B,
                                    int N, int hop, int n_bins, int band, float switch_prob, void* stream) {
    FT_CHECK_ARG(prob && freq && voiced_prob && n_samples && transition && centres && f0 && work);
    FT_CHECK_ARG(B >= 1 && N >= 1 && hop >= 1 && n_bins >= 1 && band >= 0);
    FT_CHECK_ARG(B <= 65535 && N / hop < 0x7fffffff);
    FT_CHECK_ARG(switch_prob >= PYIN_MIN_SWITCH && switch_prob <= 1.f - PYIN_MIN_SWITCH);
    if (n_bins > PYIN_MAX_BINS || band > PYIN_MAX_BAND)
        return ft_fail(FT_EUNSUPPORTED, "%s: %d bins, a band of %d: the path search holds %d bins (a lane a state) and a band of %d (a byte a backpointer)",
                       __func__, n_bins, band, PYIN_MAX_BINS, PYIN_MAX_BAND);
    const int T = N / hop + 1;
    FT_CHECK_ARG(work_bytes >= ft_f0_viterbi_workspace_bytes(B, T, n_bins));
    const int SPs = cdiv(n_bins + 2 * band, 64) * 64 + 32;
    const ViterbiArgs p{prob, freq, voiced_prob, n_samples, transition, centres, f0, static_cast<uint8_t*>(work), 1.f - switch_prob, switch_prob,
                        N, T, hop, n_bins, band, SPs};
    const size_t lds = (size_t)(4 * SPs + 128 + 32 + 16) * sizeof(float);
    hipLaunchKernelGGL(pyin_viterbi_k, dim3(B), dim3(cdiv(2 * n_bins, 64) * 64), lds, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
