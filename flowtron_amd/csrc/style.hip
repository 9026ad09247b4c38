// Style transfer (the reference's inference_style_transfer.ipynb): the posterior over z given the latents of a set of reference
// utterances, accumulated batch by batch, and samples from it.  K utterances z_b [M][len_b], prior N(0, 1), lambd the assumed
// variance of an observation:  ratio = K / lambd,  mu = ratio / (ratio + 1) * mean_b(...)  with
//   FT_STYLE_BATCH            mean over b of z_b tiled along time to n_frames: z_b[m][t mod len_b]       -> mu [M][n_frames]
//   FT_STYLE_TIME_AND_BATCH   mean over b of the utterance's own time mean (1 / len_b) sum_t z_b[m][t]   -> mu [M]
//
//   * the sums live in a float64 accumulator the caller owns (zeroed once), so a reference set of any size is added in as
//     many calls as it takes.  No floating-point atomics: every accumulator element belongs to ONE thread, which adds the
//     utterances in order of b; a time mean is 16 strided partial sums (t = j, j + 16, ... ascending) folded by one fixed
//     tree, an order that depends on len_b alone.  The result is therefore the same bit for bit however the set is split
//     into calls and whatever width T the batch is padded to.
//   * z comes with element strides (b, m, t): the forward's time-major [T][B][M] and a [B][M][T] tensor are read in place.
//     A workgroup is a 16 x 16 tile of (m, t); its lanes walk whichever of the two has the smaller stride first, so a wave
//     reads runs of 16 consecutive floats in either layout.
//   * len_b is clamped to 1 ..= T inside the kernels and only frames t < len_b are addressed: nothing behind an utterance's
//     end (padding, NaNs) is ever read, and no length can send a read out of bounds.
//   * sampling: out[s][m][t] = mu + sigma eps[s][m][t], formed in float64 and rounded to fp32 once.
#include "common.h"

namespace {

constexpr int TM = 16, TT = 16;                 // the (m, t) tile of a workgroup
constexpr int THREADS = TM * TT;
constexpr int SAMPLE_MAX_GRID = 4096;

struct StyleZ {
    const float* z;
    int64_t sb, sm, st;                         // element strides of (utterance, mel, frame)
    const int32_t* lens;
    int B, M, T;
};

__device__ __forceinline__ int style_len(const StyleZ& p, int b) { return min(max(p.lens[b], 1), p.T); }

template <bool MFAST>
__global__ __launch_bounds__(THREADS) void style_acc_batch_k(StyleZ p, double* acc, int n_frames) {
    const int mi = MFAST ? threadIdx.x % TM : threadIdx.x / TT;
    const int ti = MFAST ? threadIdx.x / TM : threadIdx.x % TT;
    const int m = blockIdx.y * TM + mi;
    const int64_t t = (int64_t)blockIdx.x * TT + ti;
    if (m >= p.M || t >= n_frames) return;
    double* dst = acc + (int64_t)m * n_frames + t;
    double a = *dst;
    const float* zm = p.z + m * p.sm;
    for (int b = 0; b < p.B; ++b) {
        const int len = style_len(p, b);
        a += (double)zm[b * p.sb + (t % len) * p.st];
    }
    *dst = a;
}

template <bool MFAST>
__global__ __launch_bounds__(THREADS) void style_acc_time_k(StyleZ p, double* acc) {
    __shared__ double part[TM][TT + 1];
    const int mi = MFAST ? threadIdx.x % TM : threadIdx.x / TT;
    const int ti = MFAST ? threadIdx.x / TM : threadIdx.x % TT;
    const int m = blockIdx.x * TM + mi;
    const bool live = m < p.M;
    const bool owner = live && ti == 0;
    double a = owner ? acc[m] : 0.0;
    const float* zm = p.z + (live ? m : 0) * p.sm;
    for (int b = 0; b < p.B; ++b) {
        const int len = style_len(p, b);                               // uniform over the workgroup
        double s = 0.0;
        if (live)
            for (int t = ti; t < len; t += TT) s += (double)zm[b * p.sb + t * p.st];
        part[mi][ti] = s;
        __syncthreads();
#pragma unroll
        for (int w = TT / 2; w > 0; w >>= 1) {
            if (ti < w) part[mi][ti] += part[mi][ti + w];
            __syncthreads();
        }
        if (owner) a += part[mi][0] / (double)len;
        __syncthreads();                                               // part[mi][0] is read before the next utterance overwrites it
    }
    if (owner) acc[m] = a;
}

// per = M * n_frames elements per sample; bcast: acc is [M] and element (m, t) reads acc[m]
__global__ __launch_bounds__(256) void style_sample_k(const double* acc, const float* eps, float* out, int64_t per, int64_t total,
                                                      int n_frames, int bcast, double c, double K, double sigma) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i % per;
        const double mu = c * acc[bcast ? r / n_frames : r] / K;
        out[i] = (float)(eps ? mu + sigma * (double)eps[i] : mu);
    }
}

}  // namespace

extern "C" int ft_style_accumulate(const float* z, int64_t stride_b, int64_t stride_m, int64_t stride_t, const int32_t* lens,
                                   double* acc, int B, int M, int T, int n_frames, int mode, void* stream) {
    FT_CHECK_ARG(z && lens && acc);
    FT_CHECK_ARG(B >= 1 && M >= 1 && T >= 1 && n_frames >= 1);
    FT_CHECK_ARG(mode == FT_STYLE_BATCH || mode == FT_STYLE_TIME_AND_BATCH);
    FT_CHECK_ARG(stride_b >= 0 && stride_m >= 0 && stride_t >= 0);
    FT_CHECK_ARG((reinterpret_cast<uintptr_t>(acc) & 7) == 0);
    FT_CHECK_ARG(cdiv(M, TM) <= 65535);
    const StyleZ p{z, stride_b, stride_m, stride_t, lens, B, M, T};
    const bool mfast = stride_m <= stride_t;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (mode == FT_STYLE_BATCH) {
        const dim3 grid(cdiv(n_frames, TT), cdiv(M, TM));
        if (mfast) hipLaunchKernelGGL(style_acc_batch_k<true>, grid, dim3(THREADS), 0, st, p, acc, n_frames);
        else hipLaunchKernelGGL(style_acc_batch_k<false>, grid, dim3(THREADS), 0, st, p, acc, n_frames);
    } else {
        const dim3 grid(cdiv(M, TM));
        if (mfast) hipLaunchKernelGGL(style_acc_time_k<true>, grid, dim3(THREADS), 0, st, p, acc);
        else hipLaunchKernelGGL(style_acc_time_k<false>, grid, dim3(THREADS), 0, st, p, acc);
    }
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_style_sample(const double* acc, const float* eps, float* out, int S, int M, int n_frames, int K, double lambd,
                               double sigma, int mode, void* stream) {
    FT_CHECK_ARG(acc && out);
    FT_CHECK_ARG(S >= 1 && M >= 1 && n_frames >= 1 && K >= 1);
    FT_CHECK_ARG(lambd > 0.0);
    FT_CHECK_ARG(mode == FT_STYLE_BATCH || mode == FT_STYLE_TIME_AND_BATCH);
    FT_CHECK_ARG(eps || S == 1);
    FT_CHECK_ARG((reinterpret_cast<uintptr_t>(acc) & 7) == 0);
    const double ratio = (double)K / lambd;
    const double c = ratio / (ratio + 1.0);
    const int64_t per = (int64_t)M * n_frames, total = per * S;
    const int64_t blocks = (total + 255) / 256;
    const int grid = (int)(blocks < SAMPLE_MAX_GRID ? blocks : SAMPLE_MAX_GRID);
    hipLaunchKernelGGL(style_sample_k, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), acc, eps, out, per, total,
                       n_frames, mode == FT_STYLE_TIME_AND_BATCH ? 1 : 0, c, (double)K, sigma);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
