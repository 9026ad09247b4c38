// STFT magnitude / phase / mel and the inverse STFT for every power-of-two analysis size n_fft = 256 .. 4096 and any hop
// (1 <= hop <= win_length <= n_fft): the settings of data_config at other sample rates (16 kHz 512 / 128, 24 kHz 2048 / 300,
// 44.1 / 48 kHz 2048 / 512, ...).  The design of stft_r8.hip (n_fft = 1024, hop <= 256) generalised:
//
//   * rFFT-N = ONE H-point complex FFT (H = N / 2) of z[m] = x[2m] + i x[2m+1] plus the split step
//       X[k] = (Z[k] + conj Z[H-k]) / 2  -  i e^{-2 pi i k / N} (Z[k] - conj Z[H-k]) / 2,   k = 0 .. H.
//   * one WAVE per frame, 4 waves per workgroup.  The H-point FFT is a Stockham autosort transform held in the wave's own LDS
//     buffer: one radix-2 / -4 pass where log2 H is not a multiple of 3, then radix-8 passes (H = 128: 2.8.8, 256: 4.8.8,
//     512: 8.8.8, 1024: 2.8.8.8, 2048: 4.8.8.8).  A pass loads a lane's butterflies (H / 64 points, 2 .. 32) into registers,
//     twiddles them from an LDS table of e^{-2 pi i j / N}, runs the DFT in registers and writes them back in place: the LDS
//     operations of one wave execute in order, so no workgroup barrier is needed inside a frame.
//   * the workgroup's audio span ((4 FPW - 1) hop + N samples) is staged in LDS once.  FPW (frames per wave) is chosen at run
//     time from (hop, N): 4, 2 or 1, the largest whose LDS fits two workgroups per CU (80 KiB), else 1 (at most 155 KiB).
//   * filterbank in CSR form (as ft_stft_r8): band b = weights band_w[ptr[b] .. ptr[b+1]) over consecutive bins from bin0[b];
//     staged in LDS when nnz <= BWMAX, read from global memory otherwise (4096 with fmax = sr / 2: ~4 000 non-zeros).
//   * the inverse: the IFFT of the conjugate split spectrum on the same FFT, window, and an overlap-add without atomics in which
//     a workgroup owns 4 096 output samples whatever the hop and recomputes the halo frames it shares with its neighbours.
#include "common.h"

#include <cfloat>

namespace {

constexpr int WAVES = 4;
constexpr int LDS_TWO_PER_CU = 80 * 1024;              // forward: prefer an LDS footprint that leaves room for two workgroups
constexpr int LDS_MAX = 160 * 1024;

#include "stft_common.h"

// tw[j] = e^{-2 pi i j / N}, j = 0 .. H (N = 2H): the split twiddles, and W_H^j = tw[2j] for the FFT passes
template <int H>
__device__ __forceinline__ void fill_twiddles(cpx* tw, int tid) {
    for (int i = tid; i <= H; i += 256) {
        float s, c;
        sincospif(-2.0f * ((float)i / (float)(2 * H)), &s, &c);                                 // exact argument: N is 2^k
        tw[i] = (cpx){c, s};
    }
}

// One Stockham pass of radix R over an H-point sequence in T (natural order in, natural order out after the last pass); NS =
// the product of the radices before it.  Butterfly j (0 <= j < H/R) reads T[j + r H/R], twiddles point r by W_{NS R}^{r k}
// (k = j mod NS), and writes T[(j - k) R + k + r NS].  Every lane reads all its points before any lane writes (one wave).
template <int H, int R, int NS>
__device__ __forceinline__ void fft_pass(cpx* T, const cpx* tw, int lane) {
    constexpr int NBF = H / R, PER = NBF >= 64 ? NBF / 64 : 1;
    const bool on = NBF >= 64 || lane < NBF;
    cpx v[PER][R];
    if (on) {
#pragma unroll
        for (int i = 0; i < PER; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) v[i][r] = T[lane + 64 * i + r * NBF];
    }
    lds_order();
    if (on) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = lane + 64 * i, k = j & (NS - 1);
            if constexpr (NS > 1) {
#pragma unroll
                for (int r = 1; r < R; ++r) {
                    const int idx = r * k * (2 * H / (NS * R));                                // W_{NS R}^{r k} = e^{-2 pi i idx / N}
                    const cpx w = idx <= H ? tw[idx] : (cpx){-tw[idx - H].re, -tw[idx - H].im};
                    v[i][r] = cmul(v[i][r], w);
                }
            }
            dft(v[i]);
            const int d = (j - k) * R + k;
#pragma unroll
            for (int r = 0; r < R; ++r) T[d + r * NS] = v[i][r];
        }
    }
    lds_order();
}

template <int H, int NS>
__device__ __forceinline__ void fft_r8_passes(cpx* T, const cpx* tw, int lane) {
    if constexpr (NS < H) {
        fft_pass<H, 8, NS>(T, tw, lane);
        fft_r8_passes<H, NS * 8>(T, tw, lane);
    }
}

// forward H-point DFT (H = 2^LH) of T[0 .. H) in place, one wave
template <int LH>
__device__ __forceinline__ void fft_wave(cpx* T, const cpx* tw, int lane) {
    constexpr int H = 1 << LH, R0 = 1 << (LH % 3 == 0 ? 3 : LH % 3);
    fft_pass<H, R0, 1>(T, tw, lane);
    fft_r8_passes<H, R0>(T, tw, lane);
}

// dynamic LDS of the forward kernel: tw [H+1] cpx | T [WAVES][H] cpx | mo [n_mel][FPG+1] | bw [BWMAX] | xs [span]
size_t stft_lds_bytes(int n_fft, int hop, int n_mel, bool mel, int fpw) {
    const size_t H = n_fft / 2, fpg = (size_t)WAVES * fpw;
    size_t b = sizeof(cpx) * ((H + 1) + WAVES * H);
    if (mel) b += sizeof(float) * ((size_t)n_mel * (fpg + 1) + BWMAX);
    return b + sizeof(float) * ((fpg - 1) * hop + n_fft);
}

template <int LH>
__global__ __launch_bounds__(256) void stft_pow2_k(StftP p) {
    constexpr int H = 1 << LH, N = 2 * H, PL = H / 64;                   // PL: complex points per lane
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int FPG = WAVES * p.fpw;
    cpx* tw = reinterpret_cast<cpx*>(smem);
    cpx* tr = tw + (H + 1);
    float* mo = reinterpret_cast<float*>(tr + WAVES * H);
    float* bw = mo + (p.mel ? p.n_mel * (FPG + 1) : 0);
    float* xs = bw + (p.mel ? BWMAX : 0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, f0 = blockIdx.x * FPG;
    const float* yb = p.y + (size_t)b * p.N;
    const int Nb = p.n_samples ? min(max(p.n_samples[b], 1), p.N) : p.N;   // this utterance's own length: the reflection is about ITS end
    const int nfb = p.n_samples ? Nb / p.hop + 1 : p.n_frames;
    const int span = (FPG - 1) * p.hop + N;
#pragma unroll 4
    for (int j = tid; j < span; j += 256) {
        int n = f0 * p.hop + j - H;                                       // reflect padding (audio_processing.py:210-214)
        if (n < 0) n = -n;
        if (n >= Nb) n = 2 * (Nb - 1) - n;
        xs[j] = (n >= 0 && n < Nb) ? yb[n] : 0.f;
    }
    int bk0[2] = {0, 0}, bw0[2] = {0, 0}, bn[2] = {0, 0};
    bool w_lds = false;
    if (p.mel) {
        const int nnz = p.band_ptr[p.n_mel];
        w_lds = nnz <= BWMAX;
        if (w_lds) for (int j = tid; j < nnz; j += 256) bw[j] = p.band_w[j];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int mb = lane + 64 * h;
            if (mb < p.n_mel) { bk0[h] = p.band_bin0[mb]; bw0[h] = p.band_ptr[mb]; bn[h] = p.band_ptr[mb + 1] - bw0[h]; }
        }
    }
    fill_twiddles<H>(tw, tid);
    __syncthreads();
    cpx* T = tr + wave * H;
    float* M = reinterpret_cast<float*>(T);                               // the magnitudes replace the spectrum after the split
    for (int fi = 0; fi < p.fpw; ++fi) {
        const int t = f0 + wave * p.fpw + fi;
        if (t >= nfb) break;                                              // wave-uniform
        const float* xf = xs + (wave * p.fpw + fi) * p.hop;
        // ---- z[m] = w[2m] x[2m] + i w[2m+1] x[2m+1]  (xf is 4-byte aligned only: hop may be odd)
#pragma unroll
        for (int j = 0; j < PL; ++j) {
            const int m = lane + 64 * j;
            const float2 w2 = *reinterpret_cast<const float2*>(p.window + 2 * m);
            T[m] = (cpx){xf[2 * m] * w2.x, xf[2 * m + 1] * w2.y};
        }
        lds_order();
        fft_wave<LH>(T, tw, lane);
        // ---- split: X[k], k = lane + 64 r (r = 0 .. PL), k <= H
        float mk[PL + 1];
#pragma unroll
        for (int r = 0; r <= PL; ++r) {
            const int k = lane + 64 * r;
            mk[r] = 0.f;
            if (k <= H) {
                const cpx zk = T[k & (H - 1)], zc = T[(H - k) & (H - 1)];
                const cpx e = {0.5f * (zk.re + zc.re), 0.5f * (zk.im - zc.im)};    // (Z[k] + conj Z[H-k]) / 2
                const cpx o = {0.5f * (zk.re - zc.re), 0.5f * (zk.im + zc.im)};    // (Z[k] - conj Z[H-k]) / 2
                const cpx w = cmul(tw[k], mul_mi(o));                              // -i e^{-2 pi i k / N} o
                const float re = e.re + w.re, im = e.im + w.im;
                mk[r] = sqrtf(re * re + im * im);
                if (p.phase) {
                    if (p.mag) p.mag[((size_t)b * (H + 1) + k) * p.ldt + t] = mk[r];
                    p.phase[((size_t)b * (H + 1) + k) * p.ldt + t] = atan2f(im, re);
                }
            }
        }
        lds_order();                                                      // every lane has read Z before M overwrites it
        if (p.mel) {
#pragma unroll
            for (int r = 0; r <= PL; ++r) if (lane + 64 * r <= H) M[lane + 64 * r] = mk[r];
            lds_order();
            // ---- sparse triangular filterbank + log compression (audio_processing.py:132-133, :81-82)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int mb = lane + 64 * h;
                if (mb >= p.n_mel) continue;
                const int k0 = bk0[h], w0 = bw0[h], n = bn[h];
                float s = 0.f;                                             // one accumulator, bins in ascending order
                if (w_lds) {
                    for (int i = 0; i < n; i += 8) {
                        float wv[8], mv[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) {
                            const int j = i + u < n ? i + u : n - 1;
                            wv[u] = bw[w0 + j];
                            mv[u] = M[k0 + j];
                        }
#pragma unroll
                        for (int u = 0; u < 8; ++u) if (i + u < n) s += wv[u] * mv[u];
                    }
                } else {
                    for (int i = 0; i < n; ++i) s += p.band_w[w0 + i] * M[k0 + i];
                }
                mo[mb * (FPG + 1) + wave * p.fpw + fi] = logf(fmaxf(s, 1e-5f));
            }
            lds_order();
        }
    }
    if (p.phase && p.n_samples) {                                         // a ragged spectrum is zero behind the utterance's last frame
        const int te = min(f0 + (wave + 1) * p.fpw, p.n_frames);
        for (int t = max(f0 + wave * p.fpw, nfb); t < te; ++t)
            for (int k = lane; k <= H; k += 64) {
                if (p.mag) p.mag[((size_t)b * (H + 1) + k) * p.ldt + t] = 0.f;
                p.phase[((size_t)b * (H + 1) + k) * p.ldt + t] = 0.f;
            }
    }
    if (p.mel) {                                                          // [band][FPG consecutive frames]
        __syncthreads();
        const int nf = min(FPG, p.n_frames - f0);
        for (int idx = tid; idx < p.n_mel * FPG; idx += 256) {
            const int mb = idx / FPG, f = idx - mb * FPG;
            if (f < nf) p.mel[((size_t)b * p.n_mel + mb) * p.ldt + f0 + f] = (f0 + f < nfb) ? mo[mb * (FPG + 1) + f] : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Inverse: (magnitude, phase) [B,H+1,T] -> y [B, hop (T-1)],
//   y[n] = sum_t w[u - t hop] irfft(X_t)[u - t hop] / wss[u]   (only where wss[u] > FLT_MIN),   u = n + H,
//   wss[u] = sum_t w^2[u - t hop],   X_t[k] = M[k,t] e^{i phase[k,t]}   (Im X[0] and Im X[H] ignored, as irfft does).
//   * irfft-N = ONE H-point complex inverse FFT plus the inverse split step: with X' = conj X[H - k],
//       Z[k] = (X[k] + X') + i e^{+2 pi i k / N} (X[k] - X'),   z = IFFT_H(Z) / 2,   x[2m] = Re z[m], x[2m+1] = Im z[m];
//     the IFFT is fft_wave on conj Z, conjugated back.  The result lands in the wave's buffer as the N real samples of the frame
//     in natural order (cpx m = samples 2m, 2m+1), windowed in place.
//   * overlap-add without atomics: a workgroup owns OWN = 4 096 consecutive output samples (16 per thread) whatever the hop and
//     computes every frame that covers them, its neighbours' halo frames included; 4 frames (one per wave) per round, then each
//     thread adds them into its samples' registers in ascending t together with the window's square -- fixed order, so the
//     result does not depend on the launch.
constexpr int SPT = 16, OWN = 256 * SPT;

// dynamic LDS of the inverse kernel: tw [H+1] cpx | X [WAVES][H+1] cpx | wl [N]
size_t istft_lds_bytes(int n_fft) {
    const size_t H = n_fft / 2;
    return sizeof(cpx) * ((H + 1) + WAVES * (H + 1)) + sizeof(float) * n_fft;
}

template <int LH>
__global__ __launch_bounds__(256) void istft_pow2_k(IstftP p) {
    constexpr int H = 1 << LH, N = 2 * H, PL = H / 64;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    cpx* tw = reinterpret_cast<cpx*>(smem);
    cpx* tr = tw + (H + 1);
    float* wl = reinterpret_cast<float*>(tr + WAVES * (H + 1));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, hop = p.hop, ldt = p.T;
    const int T = p.n_frames ? min(max(p.n_frames[b], 1), ldt) : ldt;    // this utterance's own frame count (uniform: SGPRs)
    const int n0 = blockIdx.x * OWN;
    const int nz1 = min(n0 + OWN, p.n_out);                               // the workgroup stores [n0, nz1): zeros from hop (T - 1) on
    float* yb = p.y + (size_t)b * p.n_out;
    if (n0 >= hop * (T - 1)) {                                            // wholly behind the utterance's end (ragged batch only)
        for (int n = n0 + tid; n < nz1; n += 256) yb[n] = 0.f;
        return;
    }
    const int u0 = n0 + H, u1 = min(n0 + OWN, hop * (T - 1)) + H;         // untrimmed sample range [u0, u1) of this workgroup
    const int t_lo = u0 - (N - 1) <= 0 ? 0 : (u0 - (N - 1) + hop - 1) / hop;
    const int t_hi = min(T - 1, (u1 - 1) / hop);                          // frames t_lo .. t_hi cover [u0, u1)
    fill_twiddles<H>(tw, tid);
    for (int i = tid; i < N; i += 256) wl[i] = p.window[i];
    __syncthreads();
    float acc[SPT], wss[SPT];
#pragma unroll
    for (int i = 0; i < SPT; ++i) acc[i] = wss[i] = 0.f;
    cpx* X = tr + wave * (H + 1);
    const float* magb = p.mag + (size_t)b * (H + 1) * ldt;
    const float* phb = p.phase + (size_t)b * (H + 1) * ldt;
    for (int c0 = t_lo; c0 <= t_hi; c0 += WAVES) {
        const int t = c0 + wave;
        if (t <= t_hi) {                                                  // wave-uniform
            // ---- X[k] = M e^{i phase}, k = lane + 64 j (j = 0 .. PL, k <= H); the raw pairs are parked first so that all loads
            // are in flight together while the accurate sincosf runs one bin at a time
#pragma unroll
            for (int j = 0; j <= PL; ++j) {
                const int k = lane + 64 * j;
                if (k <= H) X[k] = (cpx){magb[(size_t)k * ldt + t], phb[(size_t)k * ldt + t]};
            }
            lds_order();
            polar_to_cpx(X, H, lane);
            lds_order();
            // ---- inverse split: conj Z[k], k = lane + 64 j < H; all reads before the in-place writes
            cpx v[PL];
#pragma unroll
            for (int j = 0; j < PL; ++j) {
                const int k = lane + 64 * j;
                const cpx a = X[k], c = X[H - k], w = tw[k];
                const cpx s = {a.re + c.re, a.im - c.im};                                // X[k] + conj X[H-k]
                const cpx d = {a.re - c.re, a.im + c.im};                                // X[k] - conj X[H-k]
                const cpx e = cmul((cpx){w.re, -w.im}, d);                              // e^{+2 pi i k / N} d
                v[j] = (cpx){s.re - e.im, -(s.im + e.re)};                               // conj(s + i e)
            }
            lds_order();
#pragma unroll
            for (int j = 0; j < PL; ++j) X[lane + 64 * j] = v[j];
            lds_order();
            fft_wave<LH>(X, tw, lane);
            // ---- X[m] = conj(N z[m]): x[2m] = Re, x[2m+1] = -Im, scaled by 1/N (exact) and windowed, in place
#pragma unroll
            for (int j = 0; j < PL; ++j) {
                const int m = lane + 64 * j;
                const cpx c = X[m];
                const float2 w2 = *reinterpret_cast<const float2*>(wl + 2 * m);
                X[m] = (cpx){w2.x * (c.re * (1.0f / N)), w2.y * (-c.im * (1.0f / N))};
            }
            lds_order();
        }
        __syncthreads();
        // ---- overlap-add of this round's frames, ascending t
        const int nf = min(WAVES, t_hi - c0 + 1);
        for (int f = 0; f < nf; ++f) {
            const float* F = reinterpret_cast<const float*>(tr + f * (H + 1));
            const int m0 = u0 + tid - (c0 + f) * hop;
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const int m = m0 + 256 * i;
                if (m >= 0 && m < N && u0 + tid + 256 * i < u1) {
                    const float w = wl[m];
                    acc[i] += F[m];
                    wss[i] += w * w;
                }
            }
        }
        __syncthreads();
    }
    // ---- divide by the window's sum-square envelope where it is > FLT_MIN (the reference's tiny(float32) rule), store
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int u = u0 + tid + 256 * i;
        if (u < u1) yb[u - H] = wss[i] > FLT_MIN ? acc[i] / wss[i] : acc[i];
        else if (u - H < nz1) yb[u - H] = 0.f;                            // behind the utterance's end (ragged batch only)
    }
}

template <int LH>
int launch_stft(const StftP& p, int B, hipStream_t s) {
    const int fpg = WAVES * p.fpw;
    const size_t lds = stft_lds_bytes(2 << LH, p.hop, p.n_mel, p.mel != nullptr, p.fpw);
    FT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(stft_pow2_k<LH>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     LDS_MAX));
    hipLaunchKernelGGL(stft_pow2_k<LH>, dim3(cdiv(p.n_frames, fpg), B), dim3(256), lds, s, p);
    return FT_OK;
}

int stft_dispatch(StftP p, int B, int n_fft, hipStream_t s) {
    int fpw = 4;
    while (fpw > 1 && stft_lds_bytes(n_fft, p.hop, p.n_mel, p.mel != nullptr, fpw) > LDS_TWO_PER_CU) fpw /= 2;
    const size_t lds = stft_lds_bytes(n_fft, p.hop, p.n_mel, p.mel != nullptr, fpw);
    if (lds > LDS_MAX) return ft_fail(FT_EUNSUPPORTED, "stft_pow2: n_fft=%d hop=%d needs %zu B of LDS", n_fft, p.hop, lds);
    p.fpw = fpw;
    switch (log2_pow2_nfft(n_fft)) {
        case 8: return launch_stft<7>(p, B, s);
        case 9: return launch_stft<8>(p, B, s);
        case 10: return launch_stft<9>(p, B, s);
        case 11: return launch_stft<10>(p, B, s);
        default: return launch_stft<11>(p, B, s);
    }
}

template <int LH>
int launch_istft(const IstftP& p, int B, hipStream_t s) {
    const size_t lds = istft_lds_bytes(2 << LH);
    FT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(istft_pow2_k<LH>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     LDS_MAX));
    hipLaunchKernelGGL(istft_pow2_k<LH>, dim3(cdiv(p.n_out, OWN), B), dim3(256), lds, s, p);
    return FT_OK;
}

int istft_dispatch(const IstftP& p, int B, int n_fft, hipStream_t s) {
    switch (log2_pow2_nfft(n_fft)) {
        case 8: return launch_istft<7>(p, B, s);
        case 9: return launch_istft<8>(p, B, s);
        case 10: return launch_istft<9>(p, B, s);
        case 11: return launch_istft<10>(p, B, s);
        default: return launch_istft<11>(p, B, s);
    }
}

// the entries below are the shared launch path (stft_common.h); hop <= win_length <= n_fft is the only limit on the hop
const StftFamily POW2 = {stft_dispatch, istft_dispatch, 4096, OWN};

}  // namespace

// y [B,N] -> any of mel [B,n_mel,T] (needs the CSR filterbank), mag [B,n_fft/2+1,T], phase [B,n_fft/2+1,T] (both or neither);
// T = N / hop + 1.  n_fft = 256 .. 4096 (a power of two), 1 <= hop <= win_length <= n_fft, window: hann [n_fft] (win_length
// zero-padded by the caller), N > n_fft / 2 (the reflect padding).
extern "C" int ft_stft_pow2(const float* y, const float* window, const int32_t* band_bin0, const int32_t* band_ptr,
                            const float* band_w, float* mel, float* mag, float* phase, int B, int N, int n_fft, int hop,
                            int win_length, int n_mel, void* stream) {
    return stft_forward(__func__, POW2, y, nullptr, false, window, band_bin0, band_ptr, band_w, mel, mag, phase, B, N, n_fft, hop,
                        win_length, n_mel, nullptr, stream);
}

// The collated batch of the data path, as ft_stft_r8_ragged: y [B,N] zero-padded audio, utterance b holds n_samples[b] samples
// (device int32) -> mel [B,n_mel,T_out]: frames < n_samples[b] / hop + 1 exactly as ft_stft_pow2 computes them for that
// utterance alone (reflection about ITS last sample), zeros beyond.  T_out >= max_b (n_samples[b] / hop + 1).
extern "C" int ft_stft_pow2_ragged(const float* y, const int32_t* n_samples, const float* window, const int32_t* band_bin0,
                                   const int32_t* band_ptr, const float* band_w, float* mel, int B, int N, int n_fft, int hop,
                                   int win_length, int n_mel, int T_out, void* stream) {
    return stft_forward(__func__, POW2, y, n_samples, true, window, band_bin0, band_ptr, band_w, mel, nullptr, nullptr, B, N, n_fft,
                        hop, win_length, n_mel, &T_out, stream);
}

// The spectrum of a ragged batch, as ft_stft_r8_ragged_phase: y [B,N], utterance b holds n_samples[b] samples (device int32) ->
// mag (NULL = skip the store) and phase [B,n_fft/2+1,T_out], T_out = N / hop + 1: frames < n_samples[b] / hop + 1 exactly as
// ft_stft_pow2 computes them for y[b, :n_samples[b]] alone (reflection about ITS last sample), zeros beyond in every output
// that is written.  Same preconditions as ft_stft_pow2.
extern "C" int ft_stft_pow2_ragged_phase(const float* y, const int32_t* n_samples, const float* window, float* mag, float* phase,
                                         int B, int N, int n_fft, int hop, int win_length, void* stream) {
    return stft_forward(__func__, POW2, y, n_samples, true, window, nullptr, nullptr, nullptr, nullptr, mag, phase, B, N, n_fft, hop,
                        win_length, 0, nullptr, stream);
}

// (mag, phase) [B,n_fft/2+1,T] -> y [B, hop (T-1)]: STFT.inverse (audio_processing.py:237-263) for n_fft = 256 .. 4096 (a power
// of two), 1 <= hop <= win_length <= n_fft; window: hann [n_fft] (win_length zero-padded by the caller), as ft_stft_pow2.
extern "C" int ft_istft_pow2(const float* mag, const float* phase, const float* window, float* y, int B, int T, int n_fft,
                             int hop, int win_length, void* stream) {
    return stft_inverse(__func__, POW2, mag, phase, nullptr, false, window, y, B, T, n_fft, hop, win_length, stream);
}

// The inverse of a ragged batch, as ft_istft_r8_ragged: (mag, phase) [B,n_fft/2+1,T] with row stride T, utterance b holds
// n_frames[b] frames (device int32, 1 <= n_frames[b] <= T) -> y [B, hop (T-1)]: the samples n < hop (n_frames[b] - 1) exactly as
// ft_istft_pow2 computes them for mag[b, :, :n_frames[b]] alone, zeros behind; frames t >= n_frames[b] are never read.  ONE
// launch for the batch, no atomics, launch-independent.  Same preconditions as ft_istft_pow2.
extern "C" int ft_istft_pow2_ragged(const float* mag, const float* phase, const int32_t* n_frames, const float* window, float* y,
                                    int B, int T, int n_fft, int hop, int win_length, void* stream) {
    return stft_inverse(__func__, POW2, mag, phase, n_frames, true, window, y, B, T, n_fft, hop, win_length, stream);
}
