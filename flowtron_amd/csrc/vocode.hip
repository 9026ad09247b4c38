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
//
// ft_spsi_phase: the single-pass phase start (Beauregard, Harish, Wyse 2015) by the rule in include/flowtron_hip.h; a float32
// replay on the host gives the same bits.  One workgroup of 16 waves per utterance walks the frames in tiles of FT (16; 8 at
// n_fft 4096) frames; T is the contiguous axis, so a tile is staged in and out as runs of FT floats per bin.  In LDS a frame is
// a row of K + 3 words (the rows of a tile then start 4 banks apart): A [FT][K + 3] fp32 holds the magnitudes, then per bin the
// increment of its owner, then the angle; O [FT][K + 3] the owner as 16 bits; phi [2][K] the accumulator, double-buffered.
//   * analysis, one wave per frame, a lane owns ceil(K / 64) consecutive bins (an odd count: no bank conflicts) and walks them
//     with a, b, c in registers.  Pass 1 only reads: the lane's first bin that stops a walk to the right, its last bin that stops
//     a walk to the left, each with "is a peak", and the neighbours' edge magnitudes; a suffix minimum / prefix maximum over the
//     lanes (6 shuffles each) hands every lane the nearest stop outside its bins.  Behind a barrier the forward sweep writes the
//     owners of peaks and of left walks and a peak's increment over its magnitude (nobody reads that any more), the backward
//     sweep the owners of right walks from the owners alone.  Behind another barrier every owned bin copies its peak's increment.
//     No walk is longer than a lane's bins, whatever the slopes.
//   * the recurrence, one thread per bin: owner and increment from the thread's own cell, one gather phi[owner], the wraps, the
//     new phi and the angle; one barrier per frame.
//   * frames at or behind n_frames[b] are not staged; their cells get 0.  No atomics, no scratch, no communication between
//     workgroups.
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
constexpr int SPSI_THREADS = 1024;              // 16 waves: one per frame of a tile
constexpr int SPSI_MAX_FT = SPSI_THREADS / 64;
constexpr int SPSI_LDS_BYTES = 128 * 1024;
constexpr int SPSI_NONE = 0xffff;               // owner codes beside a bin number (<= 2048)
constexpr int SPSI_RIGHT = 0xfffe;              // between the two sweeps: the stop of the walk to the right
constexpr int SPSI_NO_STOP = 0x7fffffff;

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

__host__ __device__ inline size_t spsi_lds_bytes(int K, int FT) {
    return (size_t)FT * (K + 3) * (sizeof(float) + sizeof(uint16_t)) + (size_t)2 * K * sizeof(float);
}

__global__ __launch_bounds__(SPSI_THREADS) void spsi_phase_k(const float* mag, float* phase, const int32_t* n_frames, int K, int T,
                                                             int n_fft, int hop, int shift) {
    extern __shared__ __align__(16) float smem[];
    const int FT = 1 << shift, fmask = FT - 1, KP = K + 3;
    float* A = smem;                                                // [FT][KP] magnitude -> owner's increment -> angle
    float* phi = A + FT * KP;                                       // [2][K]   the accumulator, in turns
    uint16_t* O = reinterpret_cast<uint16_t*>(phi + 2 * K);         // [FT][KP] owner
    const int b = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n = n_frames ? min(max(n_frames[b], 0), T) : T;
    const float* mi = mag + (int64_t)b * K * T;
    float* po = phase + (int64_t)b * K * T;
    const int C = (K + 63) >> 6;                                    // bins of a lane
    const int j0 = min(lane * C, K), j1 = min(j0 + C, K);
    const float step = (float)hop / (float)n_fft, size = (float)n_fft;
    for (int j = tid; j < 2 * K; j += SPSI_THREADS) phi[j] = 0.f;
    int cur = 0;

    for (int t0 = 0; t0 < n; t0 += FT) {
        const int live = min(n - t0, FT);                           // frames of the tile inside the utterance
        const int wide = min(T - t0, FT);                           // frames of the tile inside the tensors
        for (int e = tid; e < K * FT; e += SPSI_THREADS) {
            const int k = e >> shift, f = e & fmask;
            if (f < live) A[f * KP + k] = mi[(int64_t)k * T + t0 + f];
        }
        __syncthreads();

        // pass 1 (reads only): the lane's own stops and what lies beside its bins
        const bool active = wave < live;                            // (uniform over the wave)
        float* m = A + wave * KP;
        uint16_t* o = O + wave * KP;
        float left = 0.f, right = 0.f;
        int stop_r = SPSI_NO_STOP, stop_l = -1;                     // 2 q + (0 peak, 1 not) / 2 q + (1 peak, 0 not)
        if (active) {
            if (j0 < j1) {
                left = j0 > 0 ? m[j0 - 1] : 0.f;
                right = j1 < K ? m[j1] : 0.f;
                float a = left, bb = m[j0];
                for (int j = j0; j < j1; ++j) {
                    const float c = j + 1 < j1 ? m[j + 1] : right;
                    const bool asc = j < K - 1 && bb < c, desc = j > 0 && bb < a;
                    const bool peak = j >= 1 && j <= K - 2 && bb > a && bb > c;
                    if (!asc && stop_r == SPSI_NO_STOP) stop_r = 2 * j + (peak ? 0 : 1);
                    if (!desc) stop_l = 2 * j + (peak ? 1 : 0);
                    a = bb;
                    bb = c;
                }
            }
            for (int d = 1; d < 64; d <<= 1) {                      // nearest stop in this lane or beyond it
                const int r = __shfl_down(stop_r, d), l = __shfl_up(stop_l, d);
                if (lane + d < 64) stop_r = min(stop_r, r);
                if (lane >= d) stop_l = max(stop_l, l);
            }
            const int r = __shfl_down(stop_r, 1), l = __shfl_up(stop_l, 1);
            stop_r = lane < 63 ? r : SPSI_NO_STOP;                  // ... beyond it only
            stop_l = lane > 0 ? l : -1;
        }
        __syncthreads();

        if (active && j0 < j1) {
            float a = left, bb = m[j0];
            int carry = stop_l;
            for (int j = j0; j < j1; ++j) {                         // forward: peaks, walks to the left
                const float c = j + 1 < j1 ? m[j + 1] : right;
                const bool asc = j < K - 1 && bb < c, desc = j > 0 && bb < a;
                const bool peak = j >= 1 && j <= K - 2 && bb > a && bb > c;
                int own = SPSI_NONE;
                if (peak) {
                    const float den = (a - bb) + (c - bb);
                    float p = (0.5f * (a - c)) / den;
                    if (!(fabsf(p) <= 0.5f)) p = 0.f;
                    m[j] = (float)((hop * j) & (n_fft - 1)) / size + step * p;
                    own = j;
                } else if (asc) {
                    own = SPSI_RIGHT;
                } else if (desc && carry >= 0 && (carry & 1)) {
                    own = carry >> 1;
                }
                o[j] = (uint16_t)own;
                if (!desc) carry = 2 * j + (peak ? 1 : 0);
                a = bb;
                bb = c;
            }
            carry = stop_r;
            for (int j = j1 - 1; j >= j0; --j) {                    // backward: walks to the right
                const int own = o[j];
                if (own == SPSI_RIGHT)
                    o[j] = (uint16_t)((carry & 1) ? SPSI_NONE : carry >> 1);
                else
                    carry = 2 * j + (own == j ? 0 : 1);
            }
        }
        __syncthreads();
        if (active)
            for (int j = lane; j < K; j += 64) {                    // every owned bin takes its peak's increment
                const int own = o[j];
                if (own < K && own != j) m[j] = m[own];
            }
        __syncthreads();

        for (int f = 0; f < live; ++f) {                            // the walk over the frames
            const float* pc = phi + cur * K;
            float* pn = phi + (cur ^ 1) * K;
            for (int j = tid; j < K; j += SPSI_THREADS) {
                const int own = O[f * KP + j];
                float v;
                if (own >= K) {
                    v = pc[j];
                } else {
                    v = pc[own] + A[f * KP + j];
                    v = v - rintf(v);
                    if (own != j) {
                        const float w = v + (((j - own) & 1) ? 0.5f : 0.0f);
                        v = w - rintf(w);
                    }
                }
                pn[j] = v;
                A[f * KP + j] = 6.2831855f * v;
            }
            __syncthreads();
            cur ^= 1;
        }

        for (int e = tid; e < K * FT; e += SPSI_THREADS) {
            const int k = e >> shift, f = e & fmask;
            if (f < wide) po[(int64_t)k * T + t0 + f] = f < live ? A[f * KP + k] : 0.f;
        }
        __syncthreads();
    }

    const int t_done = min((int)(((int64_t)n + FT - 1) >> shift << shift), T);      // whole tiles behind the utterance
    const int behind = T - t_done;
    for (int64_t e = tid; e < (int64_t)K * behind; e += SPSI_THREADS) po[(e / behind) * T + t_done + e % behind] = 0.f;
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

extern "C" int ft_spsi_phase(const float* magnitude, float* phase, const int32_t* n_frames, int B, int n_fft, int hop, int T,
                             void* stream) {
    FT_CHECK_ARG(magnitude && phase);
    FT_CHECK_ARG(B >= 1 && T >= 1 && hop >= 1 && hop <= n_fft);
    FT_CHECK_ARG(B <= 65535);
    if (n_fft < 256 || n_fft > 4096 || (n_fft & (n_fft - 1)))
        return ft_fail(FT_EUNSUPPORTED, "%s: n_fft %d: the phase start takes a power-of-two n_fft in 256 .. 4096", __func__, n_fft);
    const int K = n_fft / 2 + 1;
    FT_CHECK_ARG((int64_t)K * T <= 0x7fffffff - GLM_THREADS);
    int shift = 4;                                                  // the widest tile of at most SPSI_MAX_FT frames that fits
    while (shift > 0 && ((1 << shift) > SPSI_MAX_FT || spsi_lds_bytes(K, 1 << shift) > (size_t)SPSI_LDS_BYTES)) --shift;
    const size_t lds = spsi_lds_bytes(K, 1 << shift);
    FT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(spsi_phase_k), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     SPSI_LDS_BYTES));
    hipLaunchKernelGGL(spsi_phase_k, dim3(B), dim3(SPSI_THREADS), lds, reinterpret_cast<hipStream_t>(stream), magnitude, phase,
                       n_frames, K, T, n_fft, hop, shift);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
