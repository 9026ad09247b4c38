// Mel -> waveform helpers (additive: the reference has neither): non-negative least-squares mel inversion and the
// momentum step of fast Griffin-Lim (Perraudin, Balazs, Soendergaard 2013).
//
// ft_mel_nnls: per frame, min ||W m - s||^2 over m >= 0 by Lee-Seung multiplicative updates, started from the caller's
// estimate m0 (relu(pinv(W) s) in TacotronSTFT.mel_to_magnitude).  The arithmetic rule is in include/flowtron_hip.h; a float32
// replay on the host gives the same bits.
//   * a workgroup owns FT (a power of two, <= 16) consecutive frames of one utterance: T is the contiguous axis of s, m0 and
//     m, so a tile's loads and stores are runs of FT floats.  Everything a frame needs waits in LDS with the frame as the fast
//     index: m [nb][FT], Wt s [nb][FT], r [n_mel][FT], s [n_mel][FT], the CSR weights and the clamped band ranges.
//   * r = W m: one thread per (band, frame) adds the band's bins in ascending order; the FT lanes of a band read FT consecutive
//     LDS words and one broadcast weight.  d = Wt r and the update: one thread per (bin, frame), lower band first; the per-bin
//     table (16 bytes a bin) is read from global memory, where the FT lanes of a bin share one address.
//   * bins that no band covers are skipped after the start (they hold 0), frames behind n_frames[b] are staged as zeros and
//     never read; a tile wholly behind the utterance only writes zeros.
//   * every band range is clamped to the bins and to the weights, every band of the per-bin table to 0 .. n_mel - 1 (or "none"),
//     so a bad table reads nothing out of bounds.  No atomics, no scratch, no communication between workgroups.
//
// ft_gl_momentum: one thread per cell of [B][n_bins][T]: c = M (cos phi, sin phi), t = c + alpha (c - c_prev),
// phi <- atan2(t.im, t.re), c_prev <- c; the first call of a loop stores c_prev only.  Rows of T floats need not be 16-byte
// aligned and sincosf + atan2f dominate the 28 bytes a cell moves, so the accesses are plain coalesced 4-byte ones.
#include "common.h"

// the float32 replay on the host rounds every operation on its own (dtw.hip, pitch.hip)
#pragma clang fp contract(off)

namespace {

constexpr int NNLS_THREADS = 256;
constexpr int NNLS_MAX_FT = 16;                 // frames of a tile
constexpr int NNLS_PARTS = 16;                  // partial sums of the start's mean, per frame
constexpr int NNLS_LDS_BYTES = 60 * 1024;
constexpr float NNLS_TINY = 1e-30f;
constexpr float NNLS_FLOOR = 1e-3f;
constexpr int GLM_THREADS = 256;

struct NnlsArgs {
    const float* s;                             // [B][n_mel][T]
    const float* m0;                            // [B][nb][T]
    float* m;                                   // [B][nb][T] (may be m0)
    const int32_t* n_frames;                    // [B] or NULL
    const int32_t* fb_bin0;                     // [n_mel]
    const int32_t* fb_ptr;                      // [n_mel + 1]
    const float* fb_w;                          // [nnz]
    const int32_t* bin_band;                    // [nb][2], -1 = none
    const float* bin_w;                         // [nb][2]
    int n_mel, nb, T, nnz, n_iters, shift;      // FT = 1 << shift
};

__host__ __device__ inline size_t nnls_lds_bytes(int nb, int n_mel, int nnz, int FT) {
    return ((size_t)FT * (2 * nb + 2 * n_mel + NNLS_PARTS + 1) + nnz) * sizeof(float) + (size_t)3 * n_mel * sizeof(int);
}

__global__ __launch_bounds__(NNLS_THREADS) void mel_nnls_k(NnlsArgs p) {
    extern __shared__ __align__(16) float smem[];
    const int FT = 1 << p.shift, fmask = FT - 1, nb = p.nb, nm = p.n_mel, T = p.T;
    float* ms = smem;                                               // [nb][FT]    m
    float* qs = ms + nb * FT;                                       // [nb][FT]    Wt s
    float* rs = qs + nb * FT;                                       // [n_mel][FT] W m
    float* ss = rs + nm * FT;                                       // [n_mel][FT] s
    float* part = ss + nm * FT;                                     // [NNLS_PARTS][FT]
    float* lowest = part + NNLS_PARTS * FT;                         // [FT] the start's floor
    float* ws = lowest + FT;                                        // [nnz] CSR weights
    int* band_k0 = reinterpret_cast<int*>(ws + p.nnz);              // [n_mel] first bin, first weight, bins of a band
    int* band_p0 = band_k0 + nm;
    int* band_len = band_p0 + nm;

    const int b = blockIdx.y, tid = threadIdx.x;
    const int t0 = blockIdx.x * FT;                                 // (< T by the grid)
    const int n = p.n_frames ? min(max(p.n_frames[b], 0), T) : T;
    const int live = min(n - t0, FT);                               // frames of the tile inside the utterance
    const int wide = min(T - t0, FT);                               // frames of the tile inside the tensors
    float* mo = p.m + (int64_t)b * nb * T + t0;
    if (live <= 0) {                                                // (uniform over the workgroup) behind the utterance
        for (int e = tid; e < nb * FT; e += NNLS_THREADS) {
            const int k = e >> p.shift, f = e & fmask;
            if (f < wide) mo[(int64_t)k * T + f] = 0.f;
        }
        return;
    }

    const float* mi = p.m0 + (int64_t)b * nb * T + t0;
    const float* sg = p.s + (int64_t)b * nm * T + t0;
    for (int e = tid; e < nb * FT; e += NNLS_THREADS) {
        const int k = e >> p.shift, f = e & fmask;
        ms[e] = f < live ? mi[(int64_t)k * T + f] : 0.f;
    }
    for (int e = tid; e < nm * FT; e += NNLS_THREADS) {
        const int j = e >> p.shift, f = e & fmask;
        ss[e] = f < live ? sg[(int64_t)j * T + f] : 0.f;
    }
    for (int e = tid; e < p.nnz; e += NNLS_THREADS) ws[e] = p.fb_w[e];
    for (int j = tid; j < nm; j += NNLS_THREADS) {
        const int k0 = min(max(p.fb_bin0[j], 0), nb);
        const int p0 = min(max(p.fb_ptr[j], 0), p.nnz);
        const int len = min(max(p.fb_ptr[j + 1] - p.fb_ptr[j], 0), min(nb - k0, p.nnz - p0));
        band_k0[j] = k0;
        band_p0[j] = p0;
        band_len[j] = len;
    }
    __syncthreads();

    // the start: covered bins are raised to 1e-3 of the frame's mean estimate, the others are 0
    if (tid < NNLS_PARTS * FT) {
        const int l = tid >> p.shift, f = tid & fmask;
        float acc = 0.f;
        for (int k = l; k < nb; k += NNLS_PARTS) acc = acc + ms[k * FT + f];
        part[l * FT + f] = acc;
    }
    __syncthreads();
    if (tid < FT) {
        float acc = 0.f;
        for (int l = 0; l < NNLS_PARTS; ++l) acc = acc + part[l * FT + tid];
        lowest[tid] = NNLS_FLOOR * (acc / (float)nb);
    }
    __syncthreads();
    for (int e = tid; e < nb * FT; e += NNLS_THREADS) {
        const int k = e >> p.shift, f = e & fmask;
        const int b0 = min(p.bin_band[2 * k], nm - 1), b1 = min(p.bin_band[2 * k + 1], nm - 1);
        float v = 0.f, q = 0.f;
        if (b0 >= 0) {
            const float lo = lowest[f];
            v = ms[e];
            v = v < lo ? lo : v;
            q = p.bin_w[2 * k] * ss[b0 * FT + f];
            if (b1 >= 0) q = q + p.bin_w[2 * k + 1] * ss[b1 * FT + f];
        }
        ms[e] = v;
        qs[e] = q;
    }
    __syncthreads();

    for (int it = 0; it < p.n_iters; ++it) {
        for (int e = tid; e < nm * FT; e += NNLS_THREADS) {         // r = W m
            const int j = e >> p.shift, f = e & fmask;
            const float* w = ws + band_p0[j];
            const float* mm = ms + band_k0[j] * FT + f;
            const int len = band_len[j];
            float acc = 0.f;
            for (int i = 0; i < len; ++i) acc = acc + w[i] * mm[i * FT];
            rs[e] = acc;
        }
        __syncthreads();
        for (int e = tid; e < nb * FT; e += NNLS_THREADS) {         // d = Wt r;  m <- (m Wt s) / d
            const int k = e >> p.shift, f = e & fmask;
            const int b0 = min(p.bin_band[2 * k], nm - 1), b1 = min(p.bin_band[2 * k + 1], nm - 1);
            if (b0 < 0) continue;
            float d = p.bin_w[2 * k] * rs[b0 * FT + f];
            if (b1 >= 0) d = d + p.bin_w[2 * k + 1] * rs[b1 * FT + f];
            float v = 0.f;
            if (d > 0.f) v = (ms[e] * qs[e]) / d;
            if (v < NNLS_TINY) v = 0.f;
            ms[e] = v;
        }
        __syncthreads();
    }

    for (int e = tid; e < nb * FT; e += NNLS_THREADS) {
        const int k = e >> p.shift, f = e & fmask;
        if (f < wide) mo[(int64_t)k * T + f] = f < live ? ms[e] : 0.f;
    }
}

__global__ __launch_bounds__(GLM_THREADS) void gl_momentum_k(const float* mag, float* phase, float* prev_re, float* prev_im,
                                                             const int32_t* n_frames, int cells, int T, float alpha, int first) {
    const int j = blockIdx.x * GLM_THREADS + threadIdx.x;           // cell of utterance blockIdx.y: bin * T + frame
    if (j >= cells) return;
    if (n_frames) {
        const int n = min(max(n_frames[blockIdx.y], 0), T);
        if (j % T >= n) return;                                     // behind the utterance: neither read nor written
    }
    const int64_t i = (int64_t)blockIdx.y * cells + j;
    float sn, cs;
    sincosf(phase[i], &sn, &cs);
    const float M = mag[i];
    const float re = M * cs, im = M * sn;
    if (!first) {
        const float tr = re + alpha * (re - prev_re[i]);
        const float ti = im + alpha * (im - prev_im[i]);
        phase[i] = atan2f(ti, tr);
    }
    prev_re[i] = re;
    prev_im[i] = im;
}

}  // namespace

extern "C" int ft_mel_nnls(const float* s, const float* m0, float* m, const int32_t* n_frames, const int32_t* fb_bin0,
                           const int32_t* fb_ptr, const float* fb_w, const int32_t* bin_band, const float* bin_w, int B, int n_mel,
                           int n_fft, int T, int nnz, int n_iters, void* stream) {
    FT_CHECK_ARG(s && m0 && m && fb_bin0 && fb_ptr && fb_w && bin_band && bin_w);
    FT_CHECK_ARG(B >= 1 && n_mel >= 1 && T >= 1 && nnz >= 1 && n_iters >= 0);
    FT_CHECK_ARG(B <= 65535);
    if (n_fft < 256 || n_fft > 4096 || (n_fft & (n_fft - 1)) || n_mel > 128)
        return ft_fail(FT_EUNSUPPORTED, "%s: n_fft %d with %d mel bands: the solver takes a power-of-two n_fft in 256 .. 4096 and at most 128 bands",
                       __func__, n_fft, n_mel);
    const int nb = n_fft / 2 + 1;
    int shift = 4;                                                  // the widest tile of at most NNLS_MAX_FT frames that fits
    while (shift > 0 && ((1 << shift) > NNLS_MAX_FT || nnls_lds_bytes(nb, n_mel, nnz, 1 << shift) > (size_t)NNLS_LDS_BYTES)) --shift;
    const size_t lds = nnls_lds_bytes(nb, n_mel, nnz, 1 << shift);
    if (lds > (size_t)NNLS_LDS_BYTES)
        return ft_fail(FT_EUNSUPPORTED, "%s: %d filterbank weights over %d bins do not fit the workgroup's %d bytes", __func__, nnz, nb,
                       NNLS_LDS_BYTES);
    const NnlsArgs p{s, m0, m, n_frames, fb_bin0, fb_ptr, fb_w, bin_band, bin_w, n_mel, nb, T, nnz, n_iters, shift};
    hipLaunchKernelGGL(mel_nnls_k, dim3(cdiv(T, 1 << shift), B), dim3(NNLS_THREADS), lds, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_gl_momentum(const float* magnitude, float* phase, float* prev_re, float* prev_im, const int32_t* n_frames, int B,
                              int n_bins, int T, float alpha, int first, void* stream) {
    FT_CHECK_ARG(magnitude && phase && prev_re && prev_im);
    FT_CHECK_ARG(B >= 1 && n_bins >= 1 && T >= 1);
    FT_CHECK_ARG(B <= 65535 && (int64_t)n_bins * T <= 0x7fffffff - GLM_THREADS);
    FT_CHECK_ARG(alpha >= 0.f && alpha < 1.f);
    const int cells = n_bins * T;
    hipLaunchKernelGGL(gl_momentum_k, dim3(cdiv(cells, GLM_THREADS), B), dim3(GLM_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       magnitude, phase, prev_re, prev_im, n_frames, cells, T, alpha, first);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
