// Bandlimited sample-rate conversion of a (ragged) batch in ONE launch: x [B,N] at `orig` Hz -> y [B,N_out] at `new` Hz,
//   y[m] = sum_k h(k / orig - m / new) x[k],   h = Hann-windowed sinc (width 6 zero crossings, rolloff 0.99),
// samples outside the utterance counting as zero.  With g = gcd(orig, new), og = orig / g and ng = new / g the filter is
// polyphase: output m = q ng + p reads the K inputs k = q og + start[p] + i (i = 0 .. K-1) with the taps of phase p.  The caller
// builds taps [ng][K] and start [ng] once per rate pair (float64 on the host, rounded to fp32; flowtron_amd/audio.py).
//
//   * streaming and memory-bound: a workgroup stages the whole tap table in LDS once (row stride K | 1 words, so consecutive
//     phases fall on different banks) and then walks tiles of TILE = 1024 consecutive outputs of one utterance, grid-stride,
//     so the table's load is paid once per workgroup, not once per 4 KB of output;
//   * per tile the input span [first tap of the first output, last tap of the last output] is staged in LDS with coalesced
//     loads -- zero outside 0 <= k < n_samples[b], so whatever lies behind an utterance's end (or NaNs) never enters a sum --
//     and every lane computes 4 outputs m = m0 + tid + 256 r: coalesced stores, no atomics;
//   * every output is one fmaf chain over its K taps in ascending k, in the dense and the ragged case alike and whatever tile
//     or workgroup it falls in: utterance b of a ragged batch equals that utterance resampled alone bit for bit;
//   * outputs behind n_out(n_samples[b]) = ceil(n_samples[b] new / orig) are written as zeros up to N_out.
#include "common.h"

namespace {

constexpr int TILE = 1024;
constexpr int THREADS = 256;
constexpr int MAX_GRID = 1024;                  // 4 workgroups per CU at the table sizes of the common rates
constexpr int LDS_MAX = 160 * 1024;

struct ResampleP {
    const float* x;
    const int32_t* n_samples;                   // NULL: every row holds N samples
    const float* taps;                          // [ng][K]
    const int32_t* start;                       // [ng]
    float* y;
    int N, N_out, og, ng, K, KS, tiles;
    int64_t total;                              // B * tiles
};

__global__ __launch_bounds__(THREADS) void resample_k(ResampleP p) {
    extern __shared__ float lds[];
    float* tp = lds;                                                   // [ng][KS]
    int* st = reinterpret_cast<int*>(lds + p.ng * p.KS);               // [ng]
    float* xs = lds + p.ng * p.KS + p.ng;                              // the tile's input span
    const int tid = threadIdx.x;
    for (int i = tid; i < p.ng * p.K; i += THREADS) tp[(i / p.K) * p.KS + i % p.K] = p.taps[i];
    for (int i = tid; i < p.ng; i += THREADS) st[i] = p.start[i];

    for (int64_t w = blockIdx.x; w < p.total; w += gridDim.x) {
        const int b = (int)(w / p.tiles);
        const int m0 = (int)(w % p.tiles) * TILE;
        int n = p.n_samples ? p.n_samples[b] : p.N;
        n = min(max(n, 0), p.N);
        const int n_out = (int)min(((int64_t)n * p.ng + p.og - 1) / p.og, (int64_t)p.N_out);
        const int m_end = min(m0 + TILE, p.N_out);
        const float* xb = p.x + (int64_t)b * p.N;
        float* yb = p.y + (int64_t)b * p.N_out;
        __syncthreads();                                               // the table is staged; the last tile's span has been read
        int lo = 0;
        if (m0 < n_out) {                                              // uniform over the workgroup
            const int m_last = min(m_end, n_out) - 1;
            lo = (m0 / p.ng) * p.og + st[m0 % p.ng];
            const int len = (m_last / p.ng) * p.og + st[m_last % p.ng] + p.K - lo;
            for (int i = tid; i < len; i += THREADS) {
                const int k = lo + i;
                xs[i] = (k >= 0 && k < n) ? xb[k] : 0.f;
            }
            __syncthreads();
        }
#pragma unroll
        for (int r = 0; r < TILE / THREADS; ++r) {
            const int m = m0 + tid + THREADS * r;
            if (m >= m_end) break;
            float acc = 0.f;
            if (m < n_out) {
                const int q = m / p.ng, ph = m - q * p.ng;
                const float* h = tp + ph * p.KS;
                const float* xv = xs + (q * p.og + st[ph] - lo);
                for (int i = 0; i < p.K; ++i) acc = __fmaf_rn(h[i], xv[i], acc);
            }
            yb[m] = acc;
        }
    }
}

}  // namespace

extern "C" int64_t ft_resample_out_len(int64_t n, int orig, int new_rate) {
    if (n < 0 || orig < 1 || new_rate < 1) return -1;
    return (int64_t)(((__int128)n * new_rate + orig - 1) / orig);
}

// x [B,N] -> y [B,N_out], utterance b holding n_samples[b] samples (device int32; NULL = N each): y[b, m] for
// m < ceil(n_samples[b] new_g / orig_g) as above, zeros behind.  taps [new_g][K] and phase_start [new_g] on the device.
extern "C" int ft_resample_ragged(const float* x, const int32_t* n_samples, const float* taps, const int32_t* phase_start,
                                  float* y, int B, int N, int N_out, int orig_g, int new_g, int K, void* stream) {
    FT_CHECK_ARG(x && taps && phase_start && y);
    FT_CHECK_ARG(B >= 1 && N >= 1 && N_out >= 1 && orig_g >= 1 && new_g >= 1 && K >= 1);
    if (new_g > FT_RESAMPLE_MAX_PHASES || (int64_t)new_g * K > FT_RESAMPLE_MAX_TAPS)
        return ft_fail(FT_EUNSUPPORTED, "ft_resample_ragged: %d phases x %d taps exceed the table the kernel holds in LDS "
                       "(at most %d phases and %d taps in all)", new_g, K, FT_RESAMPLE_MAX_PHASES, FT_RESAMPLE_MAX_TAPS);
    FT_CHECK_ARG((int64_t)N + orig_g + K < INT32_MAX && (int64_t)N_out + TILE < INT32_MAX);
    const int KS = K | 1;
    const int64_t span = ((int64_t)(TILE - 1) * orig_g) / new_g + 2 + K;      // inputs under one tile's outputs
    const int64_t lds = ((int64_t)new_g * KS + new_g + span) * 4;
    if (lds > LDS_MAX)
        return ft_fail(FT_EUNSUPPORTED, "ft_resample_ragged: %d / %d with %d taps needs %lld B of LDS", orig_g, new_g, K,
                       (long long)lds);
    ResampleP p{x, n_samples, taps, phase_start, y, N, N_out, orig_g, new_g, K, KS, cdiv(N_out, TILE), 0};
    p.total = (int64_t)B * p.tiles;
    FT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(resample_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     LDS_MAX));
    const int grid = (int)(p.total < MAX_GRID ? p.total : MAX_GRID);
    hipLaunchKernelGGL(resample_k, dim3(grid), dim3(THREADS), (size_t)lds, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
