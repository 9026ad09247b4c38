// Endpoints and loudness of a zero-padded batch of utterances (additive: the reference only divides by the peak at the end of
// inference.py).  include/flowtron_hip.h states every rule and summation order; tests/level_ref.py replays them bit for bit.
//
// ft_level_bounds: frame powers (librosa.effects.trim's framing), the peak, and the first / last active frame.
//   * level_frames_k: one wave per frame, LV_FPW frames to a workgroup.  Lane l adds the squares of the frame's samples l, l + 64, ..
//     ascending in float64 (the square of an fp32 is exact there), the lanes meet in the xor butterfly, and the mean is rounded
//     once to fp32.  The same wave takes max |x| over the hop samples from the frame's centre on (the frames' hops tile [0, n)).
//   * level_bounds_k: one workgroup per utterance: the largest power, the peak, then the first and last frame above the limit.
// ft_level_loudness: ITU-R BS.1770-4 gated loudness of the span [start, end) of every utterance, mono.  The K-weighting is two
// biquads in series, a serial recurrence; it runs as a chunked linear recurrence in float64, four launches:
//   * level_filter_k<1>: a lane filters its chunk of LV_CHUNK samples from a zero state and keeps the four end-state values.
//   * level_carry_k: one wave per utterance walks the chunks, s[c + 1] = z[c] + M s[c], M the host-made matrix of LV_CHUNK
//     zero-input steps.  Lane r forms row r; the four state values travel through v_readlane.
//   * level_filter_k<3>: the lane filters its chunk again from s[c], adds the squared outputs to the (at most two) 100 ms steps the
//     chunk touches, and keeps the chunk's max |x|.  The filtered signal is never stored.
//   * level_gate_k: one workgroup per utterance: step sums in ascending chunk order, 400 ms blocks, both gates, the mean.
//   A lane walking LV_CHUNK consecutive samples would read global memory LV_CHUNK words apart.  A wave (= a workgroup) stages
//   LV_SUB samples of each of its 64 chunks at a time: 64 runs of 128 contiguous bytes, two to a load instruction, into an LDS
//   tile of pitch LV_SUB + 1 words, so lane l reading word l (LV_SUB + 1) + j meets 32 distinct banks per half-wave (a pitch of
//   LV_SUB, like a pitch of LV_CHUNK, would put all 64 lanes on one bank).  8.4 KB of LDS a wave: the waves a SIMD holds are set
//   by its wave slots, not by LDS.
// ft_level_gather: [start, end) of every utterance to the front of a new batch, times an optional gain, zeros behind.
// Nothing at or behind n_samples[b] is read; every index is bounded by the clamped lengths.  No atomics, no scratch.
#include "common.h"

// the float64 replay on the host rounds every operation on its own (score.hip, dtw.hip)
#pragma clang fp contract(off)

namespace {

constexpr int LV_MAX_FRAME = 4096;
constexpr int LV_FPW = 4;                       // frames (= waves) of a workgroup
constexpr int LV_THREADS = 256;
constexpr int LV_CHUNK = 256;                   // samples a lane filters (FT_LEVEL_CHUNK)
constexpr int LV_SUB = 32;                      // samples of every chunk in the LDS tile
constexpr int LV_PITCH = LV_SUB + 1;
constexpr int LV_MAX_STEPS = 4096;              // 100 ms steps of an utterance the gate kernel holds in LDS
constexpr int LV_CARRY_TILE = 16;               // chunks whose end states the carry kernel stages at a time
constexpr int LV_GATHER = 4;                    // samples a thread of the gather copies

static_assert(LV_CHUNK == FT_LEVEL_CHUNK, "the header names the chunk length");
static_assert(LV_MAX_STEPS == FT_LEVEL_MAX_STEPS, "the header names the step limit");
static_assert(LV_MAX_FRAME == FT_LEVEL_MAX_FRAME, "the header names the frame limit");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double lane_bcast(double v, int l) {                // (l is a constant: v_readlane_b32 twice)
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}

struct FrameArgs {
    const float* audio;
    int64_t sb, sn;
    const int32_t* n_samples;
    float* power;                               // [B][T]
    float* frame_peak;                          // [B][T]
    int N, T, F, hop;
};

__global__ __launch_bounds__(LV_FPW * 64) void level_frames_k(FrameArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int t = blockIdx.x * LV_FPW + wave;
    if (t >= p.T) return;                       // (uniform over the wave; no barrier follows)
    const int n = min(max(p.n_samples[b], 1), p.N);
    const int64_t o = (int64_t)b * p.T + t;
    if (t > n / p.hop) {
        if (lane == 0) { p.power[o] = 0.f; p.frame_peak[o] = 0.f; }
        return;
    }
    const float* x = p.audio + b * p.sb;
    const int64_t s0 = (int64_t)t * p.hop - p.F / 2;
    double q = 0.0;
    for (int j = lane; j < p.F; j += 64) {
        const int64_t i = s0 + j;
        if (i >= 0 && i < n) { const double v = (double)x[i * p.sn]; q = q + v * v; }
    }
    const double Q = wave_sum_f64(q);
    const int64_t h0 = (int64_t)t * p.hop;
    float pk = 0.f;
    for (int j = lane; j < p.hop; j += 64) {
        const int64_t i = h0 + j;
        if (i < n) pk = fmaxf(pk, fabsf(x[i * p.sn]));
    }
    pk = wave_max(pk);
    if (lane == 0) { p.power[o] = (float)(Q / (double)p.F); p.frame_peak[o] = pk; }
}

__global__ __launch_bounds__(LV_THREADS) void level_bounds_k(const float* __restrict__ power, const float* __restrict__ frame_peak,
                                                             const int32_t* __restrict__ n_samples, float* __restrict__ peak,
                                                             int32_t* __restrict__ start, int32_t* __restrict__ end, int N, int T,
                                                             int hop, float thr, float ref_power, int pad) {
    __shared__ float smax[LV_THREADS / 64], spk[LV_THREADS / 64];
    __shared__ int sfirst[LV_THREADS / 64], slast[LV_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(max(n_samples[b], 1), N);
    const int Tb = n / hop + 1;                 // <= T = N / hop + 1
    const float* pw = power + (int64_t)b * T;
    const float* fp = frame_peak + (int64_t)b * T;
    float m = 0.f, pk = 0.f;
    for (int t = tid; t < Tb; t += LV_THREADS) { m = fmaxf(m, pw[t]); pk = fmaxf(pk, fp[t]); }
    m = wave_max(m);
    pk = wave_max(pk);
    if (lane == 0) { smax[wave] = m; spk[wave] = pk; }
    __syncthreads();
    m = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    pk = fmaxf(fmaxf(spk[0], spk[1]), fmaxf(spk[2], spk[3]));
    const double lim = (double)thr * (double)(ref_power > 0.f ? ref_power : m);          // exact: two fp32 factors
    int first = 0x7fffffff, last = -1;
    for (int t = tid; t < Tb; t += LV_THREADS)
        if ((double)pw[t] > lim) { first = min(first, t); last = max(last, t); }
    first = wave_min_i(first);
    last = wave_max_i(last);
    if (lane == 0) { sfirst[wave] = first; slast[wave] = last; }
    __syncthreads();
    if (tid == 0) {
        first = min(min(sfirst[0], sfirst[1]), min(sfirst[2], sfirst[3]));
        last = max(max(slast[0], slast[1]), max(slast[2], slast[3]));
        int64_t s = 0, e = n;
        if (last >= 0) {
            s = max((int64_t)first * hop - pad, (int64_t)0);
            e = min(((int64_t)last + 1) * hop + pad, (int64_t)n);
            if (s >= e) { s = 0; e = n; }       // the one active frame is centred on the utterance's end
        }
        peak[b] = pk;
        start[b] = (int32_t)s;
        end[b] = (int32_t)e;
    }
}

struct FilterArgs {
    const float* audio;
    int64_t sb, sn;
    const int32_t* n_samples;
    const int32_t* start;                       // or nullptr: 0
    const int32_t* end;                         // or nullptr: n_samples
    double* z;                                  // [B][NC][4] chunk end states from a zero state (v1, v2, y1, y2)
    double* s;                                  // [B][NC][4] chunk start states
    double* part;                               // [B][NC][2] squared outputs of the chunk's first and second step
    float* chunk_peak;                          // [B][NC]
    double b0, b1, b2, a1, a2, h1, h2;          // shelf b and a, high-pass a (its b is 1, -2, 1)
    double m[16];                               // M, row-major
    int N, NC, step;
};

// the span [s0, s0 + len) of utterance b: 1 <= len, inside [0, n)
__device__ __forceinline__ void level_span(const int32_t* n_samples, const int32_t* start, const int32_t* end, int b, int N, int& s0,
                                           int& len) {
    const int n = min(max(n_samples[b], 1), N);
    s0 = start ? min(max(start[b], 0), n - 1) : 0;
    const int e = end ? min(max(end[b], s0 + 1), n) : n;
    len = e - s0;
}

template <int PASS>
__global__ __launch_bounds__(64) void level_filter_k(FilterArgs p) {
    __shared__ float tile[64 * LV_PITCH];
    const int lane = threadIdx.x, b = blockIdx.y;
    int s0, len;
    level_span(p.n_samples, p.start, p.end, b, p.N, s0, len);
    const int64_t w0 = (int64_t)blockIdx.x * 64 * LV_CHUNK;                 // the wave's first sample, counted from s0
    if (w0 >= len) return;                      // (uniform: the workgroup is this one wave)
    const float* x = p.audio + b * p.sb + (int64_t)s0 * p.sn;
    const int c = blockIdx.x * 64 + lane;
    const int64_t my0 = (int64_t)c * LV_CHUNK;
    const bool mine = my0 < len;
    const int64_t cell = (int64_t)b * p.NC + c;
    double x1 = 0.0, x2 = 0.0, v1 = 0.0, v2 = 0.0, y1 = 0.0, y2 = 0.0;
    if (mine) {
        if (my0 >= 1) x1 = (double)x[(my0 - 1) * p.sn];
        if (my0 >= 2) x2 = (double)x[(my0 - 2) * p.sn];
        if (PASS == 3) {
            const double* st = p.s + cell * 4;
            v1 = st[0]; v2 = st[1]; y1 = st[2]; y2 = st[3];
        }
    }
    const int64_t next_step = (my0 / p.step + 1) * p.step;                  // step >= LV_CHUNK: a chunk crosses at most one boundary
    double acc = 0.0, acc0 = 0.0;
    bool crossed = false;
    float pk = 0.f;
    for (int sub = 0; sub < LV_CHUNK / LV_SUB; ++sub) {
        if (w0 + sub * LV_SUB >= len) break;    // (uniform: lane 0 holds the earliest chunk)
        __syncthreads();                        // the previous tile has been read
#pragma unroll 8
        for (int k = 0; k < LV_SUB; ++k) {
            const int idx = lane + 64 * k, ch = idx / LV_SUB, o = idx % LV_SUB;
            const int64_t i = w0 + (int64_t)ch * LV_CHUNK + sub * LV_SUB + o;
            tile[ch * LV_PITCH + o] = i < len ? x[i * p.sn] : 0.f;
        }
        __syncthreads();
        const int todo = (int)min((int64_t)LV_SUB, (int64_t)len - (my0 + sub * LV_SUB));   // <= 0: nothing of this chunk is left
        for (int j = 0; j < todo; ++j) {
            const float xf = tile[lane * LV_PITCH + j];
            const double u = (double)xf;
            const double v = (((p.b0 * u + p.b1 * x1) + p.b2 * x2) - p.a1 * v1) - p.a2 * v2;
            const double y = (((v - 2.0 * v1) + v2) - p.h1 * y1) - p.h2 * y2;
            x2 = x1; x1 = u;
            v2 = v1; v1 = v;
            y2 = y1; y1 = y;
            if (PASS == 3) {
                if (my0 + sub * LV_SUB + j == next_step) { acc0 = acc; acc = 0.0; crossed = true; }
                acc = acc + y * y;
                pk = fmaxf(pk, fabsf(xf));
            }
        }
    }
    if (!mine) return;
    if (PASS == 1) {
        double* zo = p.z + cell * 4;
        zo[0] = v1; zo[1] = v2; zo[2] = y1; zo[3] = y2;
    } else {
        p.part[cell * 2] = crossed ? acc0 : acc;
        p.part[cell * 2 + 1] = crossed ? acc : 0.0;
        p.chunk_peak[cell] = pk;
    }
}

__global__ __launch_bounds__(64) void level_carry_k(FilterArgs p) {
    __shared__ double zt[LV_CARRY_TILE * 4];
    const int lane = threadIdx.x, b = blockIdx.x, r = lane & 3;
    int s0, len;
    level_span(p.n_samples, p.start, p.end, b, p.N, s0, len);
    const int nc = (int)(((int64_t)len + LV_CHUNK - 1) / LV_CHUNK);                           // <= NC
    const double* z = p.z + (int64_t)b * p.NC * 4;
    double* s = p.s + (int64_t)b * p.NC * 4;
    const double m0 = p.m[r * 4], m1 = p.m[r * 4 + 1], m2 = p.m[r * 4 + 2], m3 = p.m[r * 4 + 3];
    double cur = 0.0;                           // element r of the running start state; lanes 4 .. 63 repeat lanes 0 .. 3
    for (int c0 = 0; c0 < nc; c0 += LV_CARRY_TILE) {                         // (uniform trip counts)
        __syncthreads();
        {
            const int c = c0 + (lane >> 2);
            zt[lane] = c < nc ? z[(int64_t)c * 4 + r] : 0.0;
        }
        __syncthreads();
        const int kn = min(LV_CARRY_TILE, nc - c0);
        for (int k = 0; k < kn; ++k) {
            if (lane < 4) s[(int64_t)(c0 + k) * 4 + r] = cur;
            const double e0 = lane_bcast(cur, 0), e1 = lane_bcast(cur, 1), e2 = lane_bcast(cur, 2), e3 = lane_bcast(cur, 3);
            cur = zt[k * 4 + r] + (((m0 * e0 + m1 * e1) + m2 * e2) + m3 * e3);
        }
    }
}

__global__ __launch_bounds__(LV_THREADS) void level_gate_k(FilterArgs p, double* __restrict__ step_sums, double* __restrict__ power,
                                                           float* __restrict__ peak, int S, double abs_gate) {
    __shared__ double ss[LV_MAX_STEPS];
    __shared__ double zz[LV_MAX_STEPS];
    __shared__ float spk[LV_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int s0, len;
    level_span(p.n_samples, p.start, p.end, b, p.N, s0, len);
    const int nc = (int)(((int64_t)len + LV_CHUNK - 1) / LV_CHUNK);
    const int ns = len / p.step;                // whole steps: <= S <= LV_MAX_STEPS
    const double* part = p.part + (int64_t)b * p.NC * 2;
    for (int k = tid; k < S; k += LV_THREADS) {
        double a = 0.0;
        if (k < ns) {
            const int lo = (int)(((int64_t)k * p.step) / LV_CHUNK), hi = (int)((((int64_t)k + 1) * p.step - 1) / LV_CHUNK);   // hi < nc
            for (int c = lo; c <= hi; ++c) {
                const int slot = ((int64_t)c * LV_CHUNK) / p.step == k ? 0 : 1;
                a = a + part[(int64_t)c * 2 + slot];
            }
            ss[k] = a;
        }
        step_sums[(int64_t)b * S + k] = a;
    }
    float pk = 0.f;
    const float* cp = p.chunk_peak + (int64_t)b * p.NC;
    for (int c = tid; c < nc; c += LV_THREADS) pk = fmaxf(pk, cp[c]);
    pk = wave_max(pk);
    if (lane == 0) spk[wave] = pk;
    __syncthreads();
    const int nb = max(0, ns - 3);
    const double den = (double)(4 * (int64_t)p.step);
    for (int j = tid; j < nb; j += LV_THREADS) zz[j] = ((ss[j] + ss[j + 1]) + (ss[j + 2] + ss[j + 3])) / den;
    __syncthreads();
    if (tid == 0) {
        peak[b] = fmaxf(fmaxf(spk[0], spk[1]), fmaxf(spk[2], spk[3]));
        double out;
        if (nb == 0) {
            out = __builtin_nan("");
        } else {
            double sum = 0.0;
            int cnt = 0;
            for (int j = 0; j < nb; ++j)
                if (zz[j] > abs_gate) { sum = sum + zz[j]; ++cnt; }
            if (cnt == 0) {
                out = 0.0;
            } else {
                const double rel = 0.1 * (sum / (double)cnt);
                sum = 0.0;
                cnt = 0;
                for (int j = 0; j < nb; ++j)
                    if (zz[j] > abs_gate && zz[j] > rel) { sum = sum + zz[j]; ++cnt; }
                out = cnt ? sum / (double)cnt : 0.0;
            }
        }
        power[b] = out;
    }
}

__global__ __launch_bounds__(LV_THREADS) void level_gather_k(const float* __restrict__ audio, int64_t sb, int64_t sn,
                                                             const int32_t* __restrict__ n_samples, const int32_t* __restrict__ start,
                                                             const int32_t* __restrict__ end, const float* __restrict__ gain,
                                                             float* __restrict__ out, int32_t* __restrict__ n_out, int N) {
    const int b = blockIdx.y;
    int s0, len;
    level_span(n_samples, start, end, b, N, s0, len);
    const float* x = audio + b * sb + (int64_t)s0 * sn;
    float* o = out + (int64_t)b * N;
    const float g = gain ? gain[b] : 1.f;
    const int64_t i0 = (int64_t)blockIdx.x * (LV_THREADS * LV_GATHER) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < LV_GATHER; ++k) {
        const int64_t i = i0 + k * LV_THREADS;
        if (i < N) {
            float v = 0.f;
            if (i < len) { v = x[i * sn]; if (gain) v = g * v; }
            o[i] = v;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) n_out[b] = len;
}

inline bool finite_d(double v) { return v == v && v <= 1.7976931348623157e308 && v >= -1.7976931348623157e308; }

}  // namespace

extern "C" int ft_level_bounds(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, float* power,
                               float* frame_peak, float* peak, int32_t* start, int32_t* end, int B, int N, int frame_length, int hop,
                               float threshold, float ref_power, int pad, void* stream) {
    FT_CHECK_ARG(audio && n_samples && power && frame_peak && peak && start && end);
    FT_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1);
    FT_CHECK_ARG(stride_b >= 0 && stride_n >= 0);
    FT_CHECK_ARG(frame_length >= 2 && frame_length % 2 == 0);
    FT_CHECK_ARG(hop >= 1 && hop <= frame_length);
    FT_CHECK_ARG(threshold >= 0.f && threshold <= 3.4028234663852886e38f);
    FT_CHECK_ARG(ref_power >= 0.f && ref_power <= 3.4028234663852886e38f);
    FT_CHECK_ARG(pad >= 0);
    if (frame_length > LV_MAX_FRAME)
        return ft_fail(FT_EUNSUPPORTED, "%s: frame_length %d: a frame holds at most %d samples", __func__, frame_length, LV_MAX_FRAME);
    const int T = N / hop + 1;
    const FrameArgs p{audio, stride_b, stride_n, n_samples, power, frame_peak, N, T, frame_length, hop};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(level_frames_k, dim3(cdiv(T, LV_FPW), B), dim3(LV_FPW * 64), 0, st, p);
    hipLaunchKernelGGL(level_bounds_k, dim3(B), dim3(LV_THREADS), 0, st, power, frame_peak, n_samples, peak, start, end, N, T, hop,
                       threshold, ref_power, pad);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" size_t ft_level_loudness_workspace_bytes(int B, int N) {
    if (B < 1 || N < 1) return 0;
    const size_t cells = (size_t)B * (size_t)cdiv(N, LV_CHUNK);
    return cells * (10 * sizeof(double) + sizeof(float));
}

extern "C" int ft_level_loudness(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples,
                                 const int32_t* start, const int32_t* end, const double* coef, const double* carry, double abs_gate,
                                 double* step_sums, double* power, float* peak, void* work, size_t work_bytes, int B, int N, int step,
                                 void* stream) {
    FT_CHECK_ARG(audio && n_samples && coef && carry && step_sums && power && peak && work);
    FT_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1 && step >= 1);
    FT_CHECK_ARG(stride_b >= 0 && stride_n >= 0);
    FT_CHECK_ARG(abs_gate >= 0.0 && finite_d(abs_gate));
    FT_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 7) == 0);
    FT_CHECK_ARG(work_bytes >= ft_level_loudness_workspace_bytes(B, N));
    for (int i = 0; i < 7; ++i) FT_CHECK_ARG(finite_d(coef[i]));
    for (int i = 0; i < 16; ++i) FT_CHECK_ARG(finite_d(carry[i]));
    const int S = max(N / step, 1);
    if (step < LV_CHUNK || S > LV_MAX_STEPS)
        return ft_fail(FT_EUNSUPPORTED, "%s: a step of %d samples, %d steps: a step holds at least %d samples and an utterance at most %d steps",
                       __func__, step, S, LV_CHUNK, LV_MAX_STEPS);
    const int NC = cdiv(N, LV_CHUNK);
    const size_t cells = (size_t)B * NC;
    FilterArgs p{};
    p.audio = audio; p.sb = stride_b; p.sn = stride_n;
    p.n_samples = n_samples; p.start = start; p.end = end;
    p.z = static_cast<double*>(work);
    p.s = p.z + cells * 4;
    p.part = p.s + cells * 4;
    p.chunk_peak = reinterpret_cast<float*>(p.part + cells * 2);
    p.b0 = coef[0]; p.b1 = coef[1]; p.b2 = coef[2]; p.a1 = coef[3]; p.a2 = coef[4]; p.h1 = coef[5]; p.h2 = coef[6];
    for (int i = 0; i < 16; ++i) p.m[i] = carry[i];
    p.N = N; p.NC = NC; p.step = step;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(cdiv(NC, 64), B);
    hipLaunchKernelGGL(level_filter_k<1>, grid, dim3(64), 0, st, p);
    hipLaunchKernelGGL(level_carry_k, dim3(B), dim3(64), 0, st, p);
    hipLaunchKernelGGL(level_filter_k<3>, grid, dim3(64), 0, st, p);
    hipLaunchKernelGGL(level_gate_k, dim3(B), dim3(LV_THREADS), 0, st, p, step_sums, power, peak, S, abs_gate);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_level_gather(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, const int32_t* start,
                               const int32_t* end, const float* gain, float* out, int32_t* n_out, int B, int N, void* stream) {
    FT_CHECK_ARG(audio && n_samples && out && n_out);
    FT_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1);
    FT_CHECK_ARG(stride_b >= 0 && stride_n >= 0);
    hipLaunchKernelGGL(level_gather_k, dim3(cdiv(N, LV_THREADS * LV_GATHER), B), dim3(LV_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), audio, stride_b, stride_n, n_samples, start, end, gain, out, n_out, N);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
