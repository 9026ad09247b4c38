// Scoring utterances: the exact log-density of every mel frame, and the health of attention maps (additive: the reference
// exposes the likelihood only as the batch-mean loss and has no attention measure).
//
// ft_frame_loglik: with n_b = min(max(out_lens[b], 0), T), for t < n_b
//     ll[b][t] = -sum_m z[t][b][m]^2 / (2 sigma^2) - (M / 2) ln(2 pi sigma^2) + sum_f sum_m log_s_f[tau_f(t)][b][m]
//     tau_f(t) = reversed[f] ? n_b - 1 - t : t          (an odd flow hands log_s back in its own, reversed time; z is natural)
//   * one wave per frame, LL_FPW frames to a workgroup.  Lane l owns the channels m = l and m = l + 64 (M <= 128) and forms, in
//     float64 from the exactly converted fp32 inputs, every operation rounded on its own,
//         q_l = (0 + z[l]^2) + z[l + 64]^2                                       (channels at or behind M contribute +0)
//         s_l = 0, then for f ascending: s_l = s_l + log_s_f[l], s_l = s_l + log_s_f[l + 64]
//     the 64 lanes meet in the xor butterfly v_l = v_l + v_{l ^ off}, off = 32, 16, 8, 4, 2, 1 (addition commutes, so every lane
//     ends with the same bits): Q from q, S from s, and
//         ll = ((-(Q * inv)) - c) + S         inv = 1 / (2 sigma^2) and c = (M / 2) ln(2 pi sigma^2): doubles from the host
//     z^2 of an fp32 is exact in float64; nothing else could be contracted, and contraction is off for the whole file.
//   * total[b] comes from a second launch, one workgroup per utterance: thread i adds ll[b][i], ll[b][i + 256], ... ascending
//     from 0, and the 256 partial sums meet in the tree p_i = p_i + p_{i + h}, h = 128, 64, .., 1.  Both orders depend on n_b
//     and M alone -- not on B, T, the grid or the utterance's place in the batch.
//   * every index is bounded by n_b <= T: nothing at or behind out_lens[b] is read.  No atomics, no scratch.
//
// ft_attn_diagnostics: one launch, one workgroup of AD_THREADS per (flow, utterance), n = out_lens[b] and l = in_lens[b] clamped
// to 1 ..= T and 1 ..= L.
//   * peaks: waves take frames (wave w the frames w, w + AD_WAVES, ..), lanes take tokens (lane i the tokens i, i + 64, ..
//     ascending: coalesced along L where the token stride is 1).  A lane keeps (value, index) and replaces only on `>`, from
//     value -inf and no index; lanes meet in a butterfly that takes the other pair when its value is larger, or equal with a
//     lower index.  A NaN never enters, the lowest index wins a tie; a row with nothing above -inf peaks at 0.  pmax is the value
//     AT the peak.  The wave adds pmax of its frames in float64, ascending; the AD_WAVES partial sums are added by one thread in
//     wave order from 0.
//   * counters: integer arithmetic over peaks (read back after a workgroup barrier).  Tiles of AD_THREADS frames: a running
//     max-scan of "the frame my run started at" (wave scan + carry, as align.hip scans durations) gives every frame its run's
//     length so far; backward steps and skipped tokens are sums over neighbouring frames; attended tokens are bits set with
//     integer atomic-or in the workgroup's own words of the caller's workspace, counted afterwards.
//   * nothing at or behind the lengths is read; addressing is 64-bit.  No float atomics, no scratch.
#include "common.h"

// the float64 replay on the host rounds every operation on its own (dtw.hip)
#pragma clang fp contract(off)

namespace {

constexpr int LL_MAX_FLOWS = 8;
constexpr int LL_MAX_M = 128;
constexpr int LL_FPW = 4;                       // frames (= waves) of a workgroup
constexpr int LL_TOTAL_THREADS = 256;
constexpr int AD_THREADS = 1024;
constexpr int AD_WAVES = AD_THREADS / 64;

struct LlArgs {
    const float* z;                             // [T][B][M]
    const float* ls[LL_MAX_FLOWS];              // [T][B][M] views, row stride ld
    int64_t ld;
    const int32_t* out_lens;
    double* frame_ll;                           // [B][T]
    double inv, c;
    int n_ls, rev_mask, T, B, M;
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(LL_FPW * 64) void frame_ll_k(LlArgs p) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const int64_t t = (int64_t)blockIdx.x * LL_FPW + wave;
    if (t >= p.T) return;                       // (uniform over the wave; no barrier follows)
    const int n = min(max(p.out_lens[b], 0), p.T);
    double* out = p.frame_ll + (int64_t)b * p.T + t;
    if (t >= n) {
        if (lane == 0) *out = 0.0;
        return;
    }
    const bool m0 = lane < p.M, m1 = lane + 64 < p.M;
    const float* zr = p.z + (t * p.B + b) * p.M;
    double q = 0.0;
    if (m0) { const double v = (double)zr[lane]; q = q + v * v; }
    if (m1) { const double v = (double)zr[lane + 64]; q = q + v * v; }
    double s = 0.0;
#pragma unroll
    for (int f = 0; f < LL_MAX_FLOWS; ++f) {
        if (f < p.n_ls) {                       // (uniform)
            const int64_t tau = ((p.rev_mask >> f) & 1) ? (int64_t)n - 1 - t : t;
            const float* r = p.ls[f] + (tau * p.B + b) * p.ld;
            if (m0) s = s + (double)r[lane];
            if (m1) s = s + (double)r[lane + 64];
        }
    }
    const double Q = wave_sum_f64(q), S = wave_sum_f64(s);
    if (lane == 0) *out = (-(Q * p.inv) - p.c) + S;
}

__global__ __launch_bounds__(LL_TOTAL_THREADS) void total_ll_k(const double* __restrict__ frame_ll, const int32_t* __restrict__ out_lens,
                                                               double* __restrict__ total, int T) {
    __shared__ double part[LL_TOTAL_THREADS];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int n = min(max(out_lens[b], 0), T);
    const double* ll = frame_ll + (int64_t)b * T;
    double acc = 0.0;
    for (int t = tid; t < n; t += LL_TOTAL_THREADS) acc = acc + ll[t];
    part[tid] = acc;
    __syncthreads();
    for (int h = LL_TOTAL_THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] = part[tid] + part[tid + h];
        __syncthreads();
    }
    if (tid == 0) total[b] = part[0];
}

struct AdArgs {
    const float* attn;
    int64_t sf, sb, st, sl;                     // element strides of (flow, utterance, frame, token)
    const int32_t* in_lens;
    const int32_t* out_lens;
    int32_t* peaks;                             // [F][B][T]
    int32_t* counters;                          // [F][B][6]
    double* focus_sum;                          // [F][B]
    unsigned int* bits;                         // [F][B][W]
    int B, T, L, W;
};

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(AD_THREADS) void attn_diag_k(AdArgs p) {
    __shared__ double fpart[AD_WAVES];
    __shared__ int wmax[AD_WAVES];
    __shared__ long long red[3][AD_WAVES];
    __shared__ int redmax[AD_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.y, b = blockIdx.x;
    const int n = min(max(p.out_lens[b], 1), p.T), l = min(max(p.in_lens[b], 1), p.L);
    const int64_t fb = (int64_t)f * p.B + b;
    const float* a = p.attn + f * p.sf + b * p.sb;
    int32_t* peaks = p.peaks + fb * p.T;
    unsigned int* bits = p.bits + fb * p.W;
    const int words = (l + 31) >> 5;            // the words that hold this utterance's tokens

    for (int w = tid; w < words; w += AD_THREADS) bits[w] = 0u;
    for (int t = n + tid; t < p.T; t += AD_THREADS) peaks[t] = -1;

    // peaks and the focus sum
    double focus = 0.0;
    for (int t = wave; t < n; t += AD_WAVES) {  // (uniform over the wave)
        const float* row = a + t * p.st;
        float bv = -INFINITY, first = 0.f;
        int bj = 0x7fffffff;
        for (int j = lane; j < l; j += 64) {
            const float v = row[j * p.sl];
            if (j == 0) first = v;
            if (v > bv) { bv = v; bj = j; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (ov > bv || (ov == bv && oj < bj)) { bv = ov; bj = oj; }
        }
        first = __shfl(first, 0, 64);
        const bool none = bj == 0x7fffffff;     // nothing above -inf: the peak is token 0, whatever it holds
        const float pmax = none ? first : bv;
        if (lane == 0) peaks[t] = none ? 0 : bj;
        focus = focus + (double)pmax;
    }
    if (lane == 0) fpart[wave] = focus;
    __syncthreads();                            // peaks and the zeroed words have landed (vmcnt(0) + barrier)

    // counters
    long long backward = 0, skipped = 0;
    int best = 0, carry = -1;
    for (int t0 = 0; t0 < n; t0 += AD_THREADS) {                            // (uniform trip count)
        const int t = t0 + tid;
        int start = -1;
        if (t < n) {
            const int pk = peaks[t];
            start = t;
            if (t > 0) {
                const int pv = peaks[t - 1];
                if (pk == pv) start = -1;
                if (pk < pv) ++backward;
                if (pk > pv + 1) skipped += pk - pv - 1;
            }
            atomicOr(&bits[pk >> 5], 1u << (pk & 31));
        }
        int s = start;                          // inclusive max-scan: the frame at which the run through t started
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int u = __shfl_up(s, off, 64);
            if (lane >= off) s = max(s, u);
        }
        if (lane == 63) wmax[wave] = s;
        __syncthreads();
        int before = carry;
        for (int w = 0; w < wave; ++w) before = max(before, wmax[w]);
        s = max(s, before);
        if (t < n) best = max(best, t - s + 1);
        for (int w = 0; w < AD_WAVES; ++w) carry = max(carry, wmax[w]);
        __syncthreads();
    }
    __syncthreads();                            // every bit is set
    long long attended = 0;
    // (an agent-scope load: the bits were set by atomics at the L2, a plain load may be served by this CU's L1)
    for (int w = tid; w < words; w += AD_THREADS)
        attended += __popc(__hip_atomic_load(&bits[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    backward = wave_sum_ll(backward);
    skipped = wave_sum_ll(skipped);
    attended = wave_sum_ll(attended);
    best = wave_max_i(best);
    if (lane == 0) { red[0][wave] = backward; red[1][wave] = skipped; red[2][wave] = attended; redmax[wave] = best; }
    __syncthreads();
    if (tid == 0) {
        long long r0 = 0, r1 = 0, r2 = 0;
        int rm = 0;
        double fs = 0.0;
        for (int w = 0; w < AD_WAVES; ++w) {
            r0 += red[0][w]; r1 += red[1][w]; r2 += red[2][w];
            rm = max(rm, redmax[w]);
            fs = fs + fpart[w];
        }
        int32_t* c = p.counters + fb * 6;
        c[0] = (int32_t)r2;                                                 // n_attended
        c[1] = (int32_t)r0;                                                 // n_backward
        c[2] = (int32_t)(r1 < 2147483647LL ? r1 : 2147483647LL);            // n_skipped
        c[3] = rm;                                                          // longest_run
        c[4] = peaks[0];                                                    // first_peak
        c[5] = peaks[n - 1];                                                // last_peak
        p.focus_sum[fb] = fs;
    }
}

}  // namespace

extern "C" int ft_frame_loglik(const float* z, const float* const* log_s, const int32_t* reversed, int n_ls, int64_t ld_ls,
                               const int32_t* out_lens, double sigma, double* frame_ll, double* total, int T, int B, int M,
                               void* stream) {
    FT_CHECK_ARG(z && log_s && reversed && out_lens && frame_ll && total);
    FT_CHECK_ARG(n_ls >= 1 && n_ls <= LL_MAX_FLOWS);
    FT_CHECK_ARG(M >= 1 && M <= LL_MAX_M && ld_ls >= M);
    FT_CHECK_ARG(T >= 1 && B >= 1 && B <= 65535);
    FT_CHECK_ARG(sigma > 0.0 && sigma <= 1.7976931348623157e308);
    LlArgs p{};
    p.z = z;
    for (int f = 0; f < n_ls; ++f) {
        FT_CHECK_ARG(log_s[f] != nullptr);
        p.ls[f] = log_s[f];
        if (reversed[f]) p.rev_mask |= 1 << f;
    }
    p.ld = ld_ls;
    p.out_lens = out_lens;
    p.frame_ll = frame_ll;
    p.inv = 1.0 / (2.0 * sigma * sigma);
    p.c = (double)M * 0.5 * log(6.283185307179586 * sigma * sigma);
    FT_CHECK_ARG(p.inv > 0.0 && p.inv <= 1.7976931348623157e308);           // (a sigma whose square leaves the doubles)
    p.n_ls = n_ls; p.T = T; p.B = B; p.M = M;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(frame_ll_k, dim3(cdiv(T, LL_FPW), B), dim3(LL_FPW * 64), 0, st, p);
    hipLaunchKernelGGL(total_ll_k, dim3(B), dim3(LL_TOTAL_THREADS), 0, st, frame_ll, out_lens, total, T);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" size_t ft_attn_diagnostics_workspace_bytes(int F, int B, int L) {
    if (F < 1 || B < 1 || L < 1) return 0;
    return (size_t)F * (size_t)B * (size_t)cdiv(L, 32) * sizeof(unsigned int);
}

extern "C" int ft_attn_diagnostics(const float* attn, int64_t stride_f, int64_t stride_b, int64_t stride_t, int64_t stride_l,
                                   const int32_t* in_lens, const int32_t* out_lens, int32_t* peaks, int32_t* counters,
                                   double* focus_sum, void* work, size_t work_bytes, int F, int B, int T, int L, void* stream) {
    FT_CHECK_ARG(attn && in_lens && out_lens && peaks && counters && focus_sum && work);
    FT_CHECK_ARG(F >= 1 && B >= 1 && T >= 1 && L >= 1);
    FT_CHECK_ARG(F <= 65535);
    FT_CHECK_ARG(stride_f >= 0 && stride_b >= 0 && stride_t >= 0 && stride_l >= 0);
    FT_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 3) == 0);
    FT_CHECK_ARG(work_bytes >= ft_attn_diagnostics_workspace_bytes(F, B, L));
    const AdArgs p{attn, stride_f, stride_b, stride_t, stride_l, in_lens, out_lens, peaks, counters, focus_sum,
                   static_cast<unsigned int*>(work), B, T, L, cdiv(L, 32)};
    hipLaunchKernelGGL(attn_diag_k, dim3(B, F), dim3(AD_THREADS), 0, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
