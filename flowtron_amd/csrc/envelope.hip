// F0-adaptive spectral envelope (CheapTrick, Morise 2015) and its mel-cepstrum of a zero-padded batch of utterances, one launch
// (additive: the reference has no metric).  include/flowtron_hip.h states the rule; tests/envelope_ref.py replays it in float64.
//
// envelope_k<LOGN>: one workgroup per frame, grid (T, B), fft_size = 2^LOGN = 512, 1024 or 2048.  The frame lives in LDS from the
// first sample load to the last store; nothing goes to global memory between the steps.
//   1. the integers of the rule (half, ul, n_w, ..) from the frame's fp32 F0, the same in every thread
//   2. the window: w_i and x w_i into the two frame buffers, their three sums in float64 (wave butterfly, then the four waves in
//      order), s_i = (x w_i - w_i sum(x w) / sum(w)) / sqrt(sum(w^2)) zero-padded into buffer A
//   3. transform 1 -> P[k] = |X[k]|^2 as floats in the free buffer; the DC correction there (read, barrier, add)
//   4. the direct-sum smoothing reads P through the mirror index and writes log S, evenly extended, as transform 2's input
//   5. transform 2 -> c2[q] = Re / fft_size, q = 0 .. H; the lifter in place, evenly extended, as transform 3's input
//   6. the mel-cepstrum: coefficient m by wave m mod 4, lane l adds A[m][q] c^[q] for q = l, l + 64, .. ascending, the lanes meet
//      in the xor butterfly (A is read from L2: 135 KB at order 32 and H = 1024)
//   7. transform 3 -> env[k] = exp(Re), skipped altogether where no envelope is asked for
// The transform is a plain complex Stockham FFT, radix 4 with one closing radix-2 stage where LOGN is odd: thread i of a stage
// reads elements i, i + N/4, i + N/2, i + 3N/4 (consecutive lanes, consecutive 8-byte words: no bank conflict) and writes
// q + s (4 p + r), which for the first stage (s = 1) is a 32-byte stride: by the bank rule those stores conflict (the later
// stages' runs of s consecutive words less and less); not measured, and not what a call costs (profiles/envelope_prof.txt: the
// mel-cepstrum's matrix from L2 and the envelope store are).  The three real transforms are run as complex ones with a zero imaginary part; the even symmetry of the
// second and third is not exploited.  Twiddles e^{-2 pi i j / N}, j < 3N/4, come from a host table (float64 rounded once) and sit
// in LDS.  LDS: 2 N + 3N/4 complex words = 11, 22, 44 KB.  Window and lifter phases are formed in float64 and reduced to one
// period before cospif / sinpif, logf and expf are the accurate ones.  No atomics, no scratch.
// Nothing at or behind n_samples[b] is read: every sample index is clamped to 0 ..= n - 1.
#include "common.h"
#include <cfloat>

namespace {

#include "stft_common.h"

constexpr int EV_THREADS = 256;
constexpr float EV_FLOOR = 1e-20f;
constexpr float EV_F0_CEIL = 1000.f;
constexpr float EV_F0_DEFAULT = 500.f;

static_assert(FT_ENVELOPE_MAX_ORDER == 32, "the header names the order limit");

struct EnvArgs {
    const float* audio;
    int64_t sb, sn;
    const int32_t* n_samples;
    const float* f0;
    int64_t fsb, fst;
    const float* twiddle;                       // [3 N / 4][2]
    const float* freqt;                         // [order + 1][H + 1], or nullptr with mc
    float* env;                                 // [B][T][H + 1] or nullptr
    float* mc;                                  // [B][T][order + 1] or nullptr
    int N, T, hop, order;
    float sr, sr15, df, f0_floor, q1;
};

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

// one radix-4 Stockham stage: sub-transforms of length N >> SL at stride s = 1 << SL
template <int N, int SL>
__device__ __forceinline__ void r4_stage(const cpx* __restrict__ x, cpx* __restrict__ y, const cpx* __restrict__ tw, int tid) {
    constexpr int S = 1 << SL;
#pragma unroll
    for (int i = tid; i < N / 4; i += EV_THREADS) {
        const int q = i & (S - 1), p = i >> SL, k = p << SL;
        const cpx a = x[i], b = x[i + N / 4], c = x[i + N / 2], d = x[i + 3 * N / 4];
        const cpx apc = cadd(a, c), amc = csub(a, c), bpd = cadd(b, d), bmd = csub(b, d);
        const cpx jbmd = {-bmd.im, bmd.re};
        const int o = q + ((4 * p) << SL);
        y[o] = cadd(apc, bpd);
        y[o + S] = cmul(tw[k], csub(amc, jbmd));
        y[o + 2 * S] = cmul(tw[2 * k], csub(apc, bpd));
        y[o + 3 * S] = cmul(tw[3 * k], cadd(amc, jbmd));
    }
}

template <int N>
__device__ __forceinline__ void r2_last(const cpx* __restrict__ x, cpx* __restrict__ y, int tid) {
#pragma unroll
    for (int i = tid; i < N / 2; i += EV_THREADS) {
        const cpx a = x[i], b = x[i + N / 2];
        y[i] = cadd(a, b);
        y[i + N / 2] = csub(a, b);
    }
}

template <int N, int SL>
__device__ __forceinline__ cpx* fft_from(cpx* a, cpx* b, const cpx* tw, int tid) {
    if constexpr ((N >> SL) >= 4) {
        r4_stage<N, SL>(a, b, tw, tid);
        __syncthreads();
        return fft_from<N, SL + 2>(b, a, tw, tid);
    } else if constexpr ((N >> SL) == 2) {
        r2_last<N>(a, b, tid);
        __syncthreads();
        return b;
    } else {
        return a;
    }
}

// forward DFT of the N complex words in a (every thread has written its part; the barrier is taken here) -> the buffer, a or b,
// that holds the result in natural order; the other one is free
template <int N>
__device__ __forceinline__ cpx* fft(cpx* a, cpx* b, const cpx* tw, int tid) {
    __syncthreads();
    return fft_from<N, 0>(a, b, tw, tid);
}

template <int LOGN>
__global__ __launch_bounds__(EV_THREADS) void envelope_k(EnvArgs p) {
    constexpr int N = 1 << LOGN, H = N / 2;
    __shared__ cpx buf0[N];
    __shared__ cpx buf1[N];
    __shared__ cpx tw[3 * N / 4];
    __shared__ double red[EV_THREADS / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.x, b = blockIdx.y;
    const int n = min(max(p.n_samples[b], 1), p.N);
    float* env = p.env ? p.env + ((int64_t)b * p.T + t) * (H + 1) : nullptr;
    float* mc = p.mc ? p.mc + ((int64_t)b * p.T + t) * (p.order + 1) : nullptr;
    if (t > n / p.hop) {                        // (uniform over the workgroup; no barrier has been met)
        if (env) for (int k = tid; k <= H; k += EV_THREADS) env[k] = 0.f;
        if (mc) for (int m = tid; m <= p.order; m += EV_THREADS) mc[m] = 0.f;
        return;
    }
    for (int j = tid; j < 3 * N / 4; j += EV_THREADS) tw[j] = (cpx){p.twiddle[2 * j], p.twiddle[2 * j + 1]};

    // 1. the frame's integers: fp32 operations, each rounded on its own, as the header writes them out
    float f = p.f0[b * p.fsb + t * p.fst];
    if (!(f >= p.f0_floor && f <= EV_F0_CEIL)) f = EV_F0_DEFAULT;           // NaN, infinities, 0 and negatives fail the test
    const int half = min((int)floorf(__fadd_rn(__fdiv_rn(p.sr15, f), 0.5f)), H - 1);
    const float wq = __fdiv_rn(f, p.df);
    const int ul = min(2 + (int)wq, H);
    const float wb = __fdiv_rn(__fdiv_rn(__fmul_rn(2.f, f), 3.f), p.df);
    const float hw = __fadd_rn(__fmul_rn(0.5f, wb), 0.5f);
    const int nw = min((int)hw, H);
    const float fr = __fsub_rn(hw, (float)nw);
    const float wd = __fsub_rn(__fmul_rn(2.f, hw), 1.f);                     // exact: the width, in bins, that n_w and fr stand for

    // 2. window and frame
    const float* x = p.audio + b * p.sb;
    const int64_t c0 = (int64_t)t * p.hop - half;
    const double wstep = (double)f / (double)p.sr15;                         // w_i = 0.5 cos(pi i wstep) + 0.5, |i wstep| < 1.01
    float* wbuf = reinterpret_cast<float*>(buf1);
    double s_ww = 0.0, s_w = 0.0, s_xw = 0.0;
    for (int i = tid; i < N; i += EV_THREADS) {
        float w = 0.f, xw = 0.f;
        if (i <= 2 * half) {
            w = 0.5f * cospif((float)((double)(i - half) * wstep)) + 0.5f;
            const int64_t idx = min(max(c0 + i, (int64_t)0), (int64_t)n - 1);
            xw = x[idx * p.sn] * w;
            s_ww += (double)w * (double)w;
            s_w += (double)w;
            s_xw += (double)xw;
        }
        wbuf[i] = w;
        buf0[i] = (cpx){xw, 0.f};
    }
    s_ww = wave_sum_d(s_ww);
    s_w = wave_sum_d(s_w);
    s_xw = wave_sum_d(s_xw);
    if (lane == 0) { red[wave][0] = s_ww; red[wave][1] = s_w; red[wave][2] = s_xw; }
    __syncthreads();
    s_ww = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    s_w = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    s_xw = ((red[0][2] + red[1][2]) + red[2][2]) + red[3][2];
    const float mean = (float)(s_xw / s_w), rnorm = (float)(1.0 / sqrt(s_ww));
    for (int i = tid; i < N; i += EV_THREADS) buf0[i].re = (buf0[i].re - wbuf[i] * mean) * rnorm;    // (its own elements)

    // 3. power spectrum and DC correction
    cpx* X = fft<N>(buf0, buf1, tw, tid);
    cpx* O = X == buf0 ? buf1 : buf0;
    float* P = reinterpret_cast<float*>(O);
    for (int k = tid; k <= H; k += EV_THREADS) { const cpx v = X[k]; P[k] = v.re * v.re + v.im * v.im; }
    __syncthreads();
    float add = 0.f;                            // ul - 1 < EV_THREADS (the entry point refuses a df that small): thread k takes bin k
    if (tid < ul - 1) {
        const float pos = __fsub_rn(wq, (float)tid);                        // exact; 0 <= pos <= wq < ul - 1
        const int j = min(max((int)pos, 0), H - 1);
        const float g = pos - (float)j;
        add = P[j] + g * (P[j + 1] - P[j]);
    }
    __syncthreads();                            // every read of the uncorrected P comes before the first write
    if (tid < ul - 1) P[tid] += add;
    __syncthreads();

    // 4. smoothing -> log S, evenly extended
    for (int k = tid; k <= H; k += EV_THREADS) {
        float S;
        if (nw == 0) {
            S = P[k];
        } else {
            float acc = 0.f;
            for (int j = k - nw + 1; j <= k + nw - 1; ++j) {
                const int m = j < 0 ? -j : (j > H ? 2 * H - j : j);
                acc += P[min(max(m, 0), H)];
            }
            const int lo = k - nw, hi = k + nw;
            const int ml = lo < 0 ? -lo : lo, mh = hi > H ? 2 * H - hi : hi;
            acc += fr * (P[min(ml, H)] + P[max(mh, 0)]);
            S = __fdiv_rn(acc, wd);
        }
        const float Lg = logf(S + EV_FLOOR);
        X[k] = (cpx){Lg, 0.f};
        if (k > 0 && k < H) X[N - k] = (cpx){Lg, 0.f};
    }

    // 5. cepstrum and lifter
    cpx* C = fft<N>(X, O, tw, tid);
    cpx* D = C == buf0 ? buf1 : buf0;
    const double fq = (double)f / (double)p.sr;
    for (int q = tid; q <= H; q += EV_THREADS) {
        float c2 = C[q].re * (1.f / (float)N);
        if (q > 0) {
            const double xd = fq * (double)q;                                // f0 tau, up to ~130 periods
            const float xr = (float)(xd - 2.0 * floor(0.5 * xd));            // one period of sin(pi x) and of cos(2 pi x)
            const float sinc = sinpif(xr) / (3.14159265358979323846f * (float)xd);
            c2 *= sinc * ((1.f - 2.f * p.q1) + 2.f * p.q1 * cospif(2.f * xr));
        }
        C[q] = (cpx){c2, 0.f};
        if (q > 0 && q < H) C[N - q] = (cpx){c2, 0.f};
    }
    __syncthreads();

    // 6. mel-cepstrum
    if (mc) {
        for (int m = wave; m <= p.order; m += EV_THREADS / 64) {
            const float* A = p.freqt + (int64_t)m * (H + 1);
            float acc = 0.f;
            for (int q = lane; q <= H; q += 64) {
                const float ch = (q == 0 || q == H) ? 0.5f * C[q].re : C[q].re;
                acc += A[q] * ch;
            }
            acc = wave_sum(acc);
            if (lane == 0) mc[m] = acc;
        }
    }
    if (!env) return;                           // (uniform)

    // 7. the envelope
    const cpx* E = fft<N>(C, D, tw, tid);
    for (int k = tid; k <= H; k += EV_THREADS) env[k] = expf(E[k].re);
}

template <int LOGN>
void envelope_launch(const EnvArgs& p, int B, hipStream_t st) {
    hipLaunchKernelGGL(envelope_k<LOGN>, dim3(p.T, B), dim3(EV_THREADS), 0, st, p);
}

inline bool finite_f(float v) { return v == v && v <= FLT_MAX && v >= -FLT_MAX; }

}  // namespace

extern "C" int ft_spectral_envelope(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, const float* f0,
                                    int64_t f0_stride_b, int64_t f0_stride_t, const float* twiddle, const float* freqt, float* env,
                                    float* mc, int B, int N, int T_f0, int hop, int fft_size, int order, float sr, float sr15,
                                    float f0_floor, float q1, void* stream) {
    FT_CHECK_ARG(audio && n_samples && f0 && twiddle && (env || mc));
    FT_CHECK_ARG(!mc || freqt);
    FT_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1 && hop >= 1);
    FT_CHECK_ARG(stride_b >= 0 && stride_n >= 0 && f0_stride_b >= 0 && f0_stride_t >= 0);
    FT_CHECK_ARG(T_f0 >= N / hop + 1);
    FT_CHECK_ARG(finite_f(sr) && sr > 0.f && finite_f(sr15) && sr15 > 0.f && finite_f(q1));
    FT_CHECK_ARG(finite_f(f0_floor) && f0_floor > 0.f && f0_floor <= EV_F0_CEIL);
    if (fft_size != 512 && fft_size != 1024 && fft_size != 2048)
        return ft_fail(FT_EUNSUPPORTED, "%s: fft_size %d: the kernels hold 512, 1024 and 2048", __func__, fft_size);
    const int H = fft_size / 2;
    FT_CHECK_ARG(!mc || (order >= 1 && order <= FT_ENVELOPE_MAX_ORDER && order < H));
    const float df = sr / (float)fft_size;
    // the widest window fits the transform, and the DC correction and the mirror stay inside the spectrum
    FT_CHECK_ARG(2.0 * floor(1.5 * (double)sr / (double)f0_floor + 0.5) + 1.0 <= (double)fft_size);
    FT_CHECK_ARG((double)EV_F0_CEIL / (double)df + 2.0 <= (double)(H < 250 ? H : 250));
    EnvArgs p{};
    p.audio = audio; p.sb = stride_b; p.sn = stride_n; p.n_samples = n_samples;
    p.f0 = f0; p.fsb = f0_stride_b; p.fst = f0_stride_t;
    p.twiddle = twiddle; p.freqt = freqt; p.env = env; p.mc = mc;
    p.N = N; p.T = N / hop + 1; p.hop = hop; p.order = mc ? order : 0;
    p.sr = sr; p.sr15 = sr15; p.df = df; p.f0_floor = f0_floor; p.q1 = q1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (fft_size == 512) envelope_launch<9>(p, B, st);
    else if (fft_size == 1024) envelope_launch<10>(p, B, st);
    else envelope_launch<11>(p, B, st);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
