// STFT magnitude / phase / mel for the reference's analysis setting n_fft = 1024 (audio_processing.py:207-235, :117-134;
// config.json:32-34) as the north star words it: a real FFT + sparse triangular filterbank, HBM-bound.
//
//   * rFFT-1024 = ONE 512-point complex FFT of z[m] = x[2m] + i x[2m+1] plus the split step
//       X[k] = (Z[k] + conj Z[512-k]) / 2  -  i e^{-2 pi i k / 1024} (Z[k] - conj Z[512-k]) / 2,   k = 0 .. 512
//     -- half the butterflies of the complex radix-2 transform in stft.hip.
//   * one WAVE per frame, 4 frames of a workgroup in flight at once: the 512-point FFT is three radix-8 passes with the 8 points
//     of a lane in REGISTERS (n = 64 j + 8 a + b, k = k1 + 8 k2 + 64 k3: DFT_8 over j, twiddle W512^{l k1}, transpose through
//     LDS, DFT_8 over a, twiddle W64^{b k2}, transpose, DFT_8 over b) -- 2 LDS transposes instead of 9 radix-2 LDS stages,
//     no workgroup barrier inside a frame (LDS operations of one wave execute in order).
//   * filterbank: the Slaney triangles overlap at most pairwise, so the dense [80][513] matrix has ~1 000 non-zeros; the host
//     hands them over as CSR (band -> first bin, weights) and a lane accumulates its band over 2 .. 60 consecutive bins.
//   * the audio span of the workgroup's 16 frames (4 864 samples) is staged in LDS once: 256 new samples in + 80 floats out
//     per frame = 1 344 B of HBM traffic.
#include "common.h"

#include <cfloat>

namespace {

constexpr int NFFT = 1024, NH = 512, NB = 513;
constexpr int FPW = 4, FPG = 4 * FPW;                  // frames per wave / per workgroup
constexpr int SPAN = (FPG - 1) * 256 + NFFT;           // hop is a runtime argument <= 256 in the reference; sized for 256

#include "stft_common.h"

// The per-lane twiddle constants of fft512_r8 and the split step depend on (lane, k) only; a workgroup evaluates each once into
// LDS (1 152 sincospif over 256 threads): tw[0, 512) = W512^{l k}, tw[512, 576) = W64^{b k}, tw[576, 1152) = W1024^{k}.
__device__ __forceinline__ void fill_twiddles(cpx* tw, int tid) {
    for (int i = tid; i < 512 + 64 + 576; i += 256) {
        float s, c, a;
        if (i < 512) a = (float)((i >> 3) * (i & 7)) / 512.0f;
        else if (i < 576) a = (float)(((i - 512) >> 3) * ((i - 512) & 7)) / 64.0f;
        else a = (float)(i - 576) / 1024.0f;
        sincospif(-2.0f * a, &s, &c);
        tw[i] = (cpx){c, s};
    }
}

// 512-point forward DFT held by one wave: on entry lane l holds v[j] = z[l + 64 j]; on exit v[k3] = Z[k1 + 8 k2 + 64 k3] with
// (k1, k2) = (lane >> 3, lane & 7).  Three radix-8 passes (n = 64 j + 8 a + b: DFT_8 over j, twiddle w1 = W512^{l k1}, transpose
// through LDS, DFT_8 over a, twiddle w2 = W64^{b k2}, transpose, DFT_8 over b).  T: the wave's own 512-entry LDS buffer; the
// LDS operations of one wave execute in order, so no barrier is needed.
__device__ __forceinline__ void fft512_r8(cpx (&v)[8], cpx* T, const cpx (&w1)[8], const cpx (&w2)[8], int lane) {
    dft(v);
#pragma unroll
    for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], w1[k]);
    // transpose 1: element (l = 8 a + b2, k1) -> lane (k1, b2), register a
    {
        const int a = lane >> 3, b2 = lane & 7;
#pragma unroll
        for (int k1 = 0; k1 < 8; ++k1) T[(k1 * 8 + b2) * 8 + a] = v[k1];
    }
    lds_order();
#pragma unroll
    for (int a = 0; a < 8; ++a) v[a] = T[lane * 8 + a];
    lds_order();
    // pass 2: DFT over a; twiddle W64^{b2 k2}
    dft(v);
#pragma unroll
    for (int k = 1; k < 8; ++k) v[k] = cmul(v[k], w2[k]);
    // transpose 2: element (k1, b2, k2) -> lane (k1, k2), register b2
    {
        const int k1 = lane >> 3, b2 = lane & 7;
#pragma unroll
        for (int k2 = 0; k2 < 8; ++k2) T[(k1 * 8 + k2) * 8 + b2] = v[k2];
    }
    lds_order();
#pragma unroll
    for (int b2 = 0; b2 < 8; ++b2) v[b2] = T[lane * 8 + b2];
    lds_order();
    // pass 3: DFT over b2
    dft(v);
}

__global__ __launch_bounds__(256) void stft_r8_k(StftP p) {
    __shared__ __attribute__((aligned(16))) float xs[SPAN];
    __shared__ __attribute__((aligned(16))) cpx tr[4][NH];               // per-wave transpose buffer
    __shared__ float mg[4][NB + 3];                                      // per-wave magnitudes
    __shared__ float mo[128][FPG + 1];                                   // mel tile of the workgroup's frames [band][frame]
    __shared__ float bw[BWMAX];                                          // the filterbank's non-zero weights (CSR values)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, f0 = blockIdx.x * FPG;
    const float* yb = p.y + (size_t)b * p.N;
    const int Nb = p.n_samples ? min(max(p.n_samples[b], 1), p.N) : p.N;   // this utterance's own length: the reflection is about ITS end
    const int nfb = p.n_samples ? Nb / p.hop + 1 : p.n_frames;
    const int span = (FPG - 1) * p.hop + NFFT;
    {                                                                     // all of a thread's loads in flight before the first LDS write
        constexpr int NL = (SPAN + 255) / 256;
        float xv[NL];
#pragma unroll
        for (int u = 0; u < NL; ++u) {
            const int j = tid + 256 * u;
            int n = f0 * p.hop + j - NH;                                  // reflect padding (audio_processing.py:210-214)
            if (n < 0) n = -n;
            if (n >= Nb) n = 2 * (Nb - 1) - n;
            xv[u] = (j < span && n >= 0 && n < Nb) ? yb[n] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NL; ++u) if (tid + 256 * u < span) xs[tid + 256 * u] = xv[u];
    }
    // filterbank: this lane's bands (lane, lane + 64) and, when they fit, the CSR values in LDS -- the band loop below then reads
    // weight and magnitude from LDS eight bins at a time (one global load per bin, un-unrolled, was ~60 dependent L1 round trips
    // on the lanes that hold the widest bands: most of a frame's time)
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
    // per-lane constants for all frames: twiddles W512^{l k1} (l = lane), W64^{b2 k2} (b2 = lane & 7), the split twiddles
    // W1024^{k} of this lane's bins k = lane + 64 r, and the window taps of its 8 complex input points
    // The three twiddle tables depend on (lane, k) only: the workgroup evaluates each entry ONCE into LDS (1 089 sincospif over 256
    // threads instead of 25 per lane of every wave) and a lane then picks its 25 constants up; the table aliases the per-wave
    // transpose buffers, which are not in use yet.
    cpx w1[8], w2[8], w3[9];
    float2 win[8];
    {
        cpx* tw = &tr[0][0];
        fill_twiddles(tw, tid);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            w1[k] = tw[lane * 8 + k];
            w2[k] = tw[512 + (lane & 7) * 8 + k];
            win[k] = *reinterpret_cast<const float2*>(p.window + 2 * (lane + 64 * k));
        }
#pragma unroll
        for (int r = 0; r < 9; ++r) w3[r] = tw[576 + lane + 64 * r];
    }
    __syncthreads();
    cpx* T = tr[wave];
    float* M = mg[wave];
    for (int fi = 0; fi < FPW; ++fi) {
        const int t = f0 + wave * FPW + fi;
        if (t >= nfb) break;                                              // wave-uniform
        const float* xf = xs + (wave * FPW + fi) * p.hop;
        // ---- lane l holds z[l + 64 j]; 512-point FFT -> Z[k], k = k1 + 8 k2 + 64 k3 with (k1, k2) = (lane >> 3, lane & 7)
        cpx v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = lane + 64 * j;
            const float2 x2 = *reinterpret_cast<const float2*>(xf + 2 * m);
            v[j] = (cpx){x2.x * win[j].x, x2.y * win[j].y};
        }
        fft512_r8(v, T, w1, w2, lane);
        {
            const int q = (lane >> 3) + 8 * (lane & 7);
#pragma unroll
            for (int k3 = 0; k3 < 8; ++k3) T[q + 64 * k3] = v[k3];
        }
        lds_order();
        // ---- split: X[k], k = lane + 64 r (r = 0 .. 7), and k = 512 on lane 0
#pragma unroll
        for (int r = 0; r <= 8; ++r) {
            const int k = lane + 64 * r;
            if (k <= NH) {
                const cpx zk = T[k & (NH - 1)], zc = T[(NH - k) & (NH - 1)];
                const cpx e = {0.5f * (zk.re + zc.re), 0.5f * (zk.im - zc.im)};    // (Z[k] + conj Z[512-k]) / 2
                const cpx o = {0.5f * (zk.re - zc.re), 0.5f * (zk.im + zc.im)};    // (Z[k] - conj Z[512-k]) / 2
                const cpx tw = cmul(w3[r], mul_mi(o));                              // -i e^{-2 pi i k / 1024} o
                const float re = e.re + tw.re, im = e.im + tw.im;
                const float m = sqrtf(re * re + im * im);
                M[k] = m;
                if (p.phase) {
                    if (p.mag) p.mag[((size_t)b * NB + k) * p.ldt + t] = m;
                    p.phase[((size_t)b * NB + k) * p.ldt + t] = atan2f(im, re);
                }
            }
        }
        lds_order();
        // ---- sparse triangular filterbank + log compression (audio_processing.py:132-133, :81-82)
        if (p.mel) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int mb = lane + 64 * h;
                if (mb >= p.n_mel) continue;
                const int k0 = bk0[h], w0 = bw0[h], n = bn[h];
                float s = 0.f;                                             // one accumulator, bins in ascending order (as before)
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
                mo[mb][wave * FPW + fi] = logf(fmaxf(s, 1e-5f));
            }
        }
        lds_order();
    }
    if (p.phase && p.n_samples) {                                         // a ragged spectrum is zero behind the utterance's last frame
        const int te = min(f0 + (wave + 1) * FPW, p.n_frames);
        for (int t = max(f0 + wave * FPW, nfb); t < te; ++t)
            for (int k = lane; k <= NH; k += 64) {
                if (p.mag) p.mag[((size_t)b * NB + k) * p.ldt + t] = 0.f;
                p.phase[((size_t)b * NB + k) * p.ldt + t] = 0.f;
            }
    }
    if (p.mel) {                                                          // [band][16 consecutive frames]: 64-byte row pieces
        __syncthreads();
        const int nf = min(FPG, p.n_frames - f0);
        for (int idx = tid; idx < p.n_mel * FPG; idx += 256) {
            const int mb = idx / FPG, f = idx - mb * FPG;
            if (f < nf) p.mel[((size_t)b * p.n_mel + mb) * p.ldt + f0 + f] = (f0 + f < nfb) ? mo[mb][f] : 0.f;   // zero padding of DataCollate
        }
    }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------------
// Inverse STFT (audio_processing.py:237-263, STFT.inverse) for the same setting: (magnitude, phase) [B,513,T] -> y [B,hop*(T-1)],
//
//   y[n] = sum_t  w[u - t hop] irfft(X_t)[u - t hop] / wss[u]   (only where wss[u] > FLT_MIN),   u = n + 512,
//   wss[u] = sum_t w^2[u - t hop],   X_t[k] = M[k,t] e^{i phase[k,t]}
//
// which is what the reference's conv_transpose1d with pinv(scale F)^T * window, the window_sumsquare division, the scale and the
// 512-sample trims compute (the pseudo-inverse of the half-spectrum DFT basis is irfft: Im X[0] and Im X[512] are ignored).
//   * irfft-1024 = ONE 512-point complex inverse FFT plus the inverse split step: with X' = conj X[512 - k],
//       Z[k] = (X[k] + X') + i e^{+2 pi i k / 1024} (X[k] - X'),   z = IFFT_512(Z) / 2,   x[2m] = Re z[m], x[2m+1] = Im z[m];
//     the IFFT is fft512_r8 on conj Z, conjugated back (one wave per frame, as in the forward kernel).
//   * overlap-add without atomics: a workgroup owns 16 hop consecutive output samples and computes every frame that covers
//     them, its neighbours' halo frames included (ceil(1024 / hop) - 1 of them: 3 of 19 at hop 256).  The windowed frames go
//     to LDS FC at a time, then each thread adds them into its samples' registers in ascending t -- fixed order, so the result
//     does not depend on the launch.  No workgroup waits for another.
//   * 256 threads, 53 KB of LDS, 234 VGPRs without spills: two workgroups per CU (two waves per SIMD, as the forward kernel);
//     three would need <= 168 VGPRs, and at that budget the compiler spills.
namespace {

constexpr int FC = 8;                                  // frames staged in LDS per round: 2 per wave
constexpr int SPT = 16;                                // owned samples per thread: 16 hop <= 4 096 = 256 threads x 16

__global__ __launch_bounds__(256) void istft_r8_k(IstftP p) {
    __shared__ __attribute__((aligned(16))) float fr[FC][NFFT];          // windowed irfft of the round's frames
    __shared__ __attribute__((aligned(16))) cpx tr[4][NH + 1];           // per-wave spectrum / transpose buffer
    __shared__ float wl[NFFT];                                            // the window (for wss)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, hop = p.hop, ldt = p.T;
    const int T = p.n_frames ? min(max(p.n_frames[b], 1), ldt) : ldt;    // this utterance's own frame count (uniform: SGPRs)
    const int S = 16 * hop;
    const int n0 = blockIdx.x * S;
    const int nz1 = min(n0 + S, p.n_out);                                 // the workgroup stores [n0, nz1): zeros from hop (T - 1) on
    float* yb = p.y + (size_t)b * p.n_out;
    if (n0 >= hop * (T - 1)) {                                            // wholly behind the utterance's end (ragged batch only)
        for (int n = n0 + tid; n < nz1; n += 256) yb[n] = 0.f;
        return;
    }
    const int u0 = n0 + NH, u1 = min(n0 + S, hop * (T - 1)) + NH;        // untrimmed sample range [u0, u1) of this workgroup
    const int t_lo = u0 - (NFFT - 1) <= 0 ? 0 : (u0 - (NFFT - 1) + hop - 1) / hop;
    const int t_hi = min(T - 1, (u1 - 1) / hop);                          // frames t_lo .. t_hi cover [u0, u1)
    // per-lane constants: w1 = W512^{l k1}, w2 = W64^{b2 k2}, w3[j] = W1024^{k} of the lane's bins k = lane + 64 j, and the window
    // taps of the lane's 8 output pairs (2m, 2m + 1), m = q + 64 k3
    const int q = (lane >> 3) + 8 * (lane & 7);
    cpx w1[8], w2[8], w3[8];
    float2 win[8];
    {
        cpx* tw = &tr[0][0];
        fill_twiddles(tw, tid);
        for (int i = tid; i < NFFT; i += 256) wl[i] = p.window[i];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            w1[k] = tw[lane * 8 + k];
            w2[k] = tw[512 + (lane & 7) * 8 + k];
            w3[k] = tw[576 + lane + 64 * k];
            win[k] = *reinterpret_cast<const float2*>(wl + 2 * (q + 64 * k));
        }
    }
    __syncthreads();
    float acc[SPT];
#pragma unroll
    for (int i = 0; i < SPT; ++i) acc[i] = 0.f;
    cpx* X = tr[wave];
    const float* magb = p.mag + (size_t)b * NB * ldt;
    const float* phb = p.phase + (size_t)b * NB * ldt;
    for (int c0 = t_lo; c0 <= t_hi; c0 += FC) {
        for (int f = wave; f < FC; f += 4) {
            const int t = c0 + f;
            if (t > t_hi) break;                                          // wave-uniform
            // ---- X[k] = M e^{i phase}, k = lane + 64 j, and k = 512 on lane 0; Im X[0] and Im X[512] dropped (irfft ignores them).
            // The raw (M, phase) pairs are parked in X first so that all loads are in flight together while the accurate
            // sincosf (full range reduction, many registers) runs one bin at a time.
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const size_t o = (size_t)(lane + 64 * j) * ldt + t;
                X[lane + 64 * j] = (cpx){magb[o], phb[o]};
            }
            if (lane == 0) X[NH] = (cpx){magb[(size_t)NH * ldt + t], phb[(size_t)NH * ldt + t]};
            lds_order();
            polar_to_cpx(X, NH, lane);
            lds_order();
            // ---- inverse split: conj Z[k] for k = lane + 64 j (the input layout of fft512_r8)
            cpx v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = lane + 64 * j;
                const cpx a = X[k], c = X[NH - k];
                const cpx s = {a.re + c.re, a.im - c.im};                                // X[k] + conj X[512-k]
                const cpx d = {a.re - c.re, a.im + c.im};                                // X[k] - conj X[512-k]
                const cpx e = cmul((cpx){w3[j].re, -w3[j].im}, d);                      // e^{+2 pi i k / 1024} d
                v[j] = (cpx){s.re - e.im, -(s.im + e.re)};                               // conj(s + i e)
            }
            lds_order();
            fft512_r8(v, X, w1, w2, lane);
            // ---- v[k3] = conj(2 * 512 z[m]), m = q + 64 k3: x[2m] = Re, x[2m+1] = -Im, scaled by 1/1024 (exact) and windowed
            float* F = fr[f];
#pragma unroll
            for (int k3 = 0; k3 < 8; ++k3) {
                const int m = q + 64 * k3;
                *reinterpret_cast<float2*>(F + 2 * m) =
                    make_float2(win[k3].x * (v[k3].re * (1.0f / 1024.0f)), win[k3].y * (-v[k3].im * (1.0f / 1024.0f)));
            }
            lds_order();
        }
        __syncthreads();
        // ---- overlap-add of this round's frames, ascending t
        const int nf = min(FC, t_hi - c0 + 1);
        for (int f = 0; f < nf; ++f) {
            const int m0 = u0 + tid - (c0 + f) * hop;
#pragma unroll
            for (int i = 0; i < SPT; ++i) {
                const int m = m0 + 256 * i;
                if (m >= 0 && m < NFFT && u0 + tid + 256 * i < u1) acc[i] += fr[f][m];
            }
        }
        __syncthreads();
    }
    // ---- divide by the window's sum-square envelope where it is > FLT_MIN (the reference's tiny(float32) rule), store
#pragma unroll
    for (int i = 0; i < SPT; ++i) {
        const int u = u0 + tid + 256 * i;
        if (u >= u1) {
            if (u - NH < nz1) yb[u - NH] = 0.f;                           // behind the utterance's end (ragged batch only)
        } else {
            const int ta = u - (NFFT - 1) <= 0 ? 0 : (u - (NFFT - 1) + hop - 1) / hop, tb = min(T - 1, u / hop);
            float wss = 0.f;
            for (int t = ta; t <= tb; ++t) {
                const float w = wl[u - t * hop];
                wss += w * w;
            }
            yb[u - NH] = wss > FLT_MIN ? acc[i] / wss : acc[i];
        }
    }
}

int launch_stft_r8(StftP p, int B, int, hipStream_t s) {
    hipLaunchKernelGGL(stft_r8_k, dim3(cdiv(p.n_frames, FPG), B), dim3(256), 0, s, p);
    return FT_OK;
}

int launch_istft_r8(const IstftP& p, int B, int, hipStream_t s) {
    hipLaunchKernelGGL(istft_r8_k, dim3(cdiv(p.n_out, 16 * p.hop), B), dim3(256), 0, s, p);
    return FT_OK;
}

// the entries below are the shared launch path (stft_common.h) at n_fft = win_length = 1024 with hop <= 256
const StftFamily R8 = {launch_stft_r8, launch_istft_r8, 256, 0};

}  // namespace

// y [B,N] -> any of mel [B,n_mel,T] (needs the CSR filterbank), mag [B,513,T], phase [B,513,T] (both or neither); T = N / hop + 1.
// n_fft = 1024 (hann window [1024] passed in, any win_length zero-padded by the caller), hop <= 256.
extern "C" int ft_stft_r8(const float* y, const float* window, const int32_t* band_bin0, const int32_t* band_ptr,
                          const float* band_w, float* mel, float* mag, float* phase, int B, int N, int hop, int n_mel,
                          void* stream) {
    return stft_forward(__func__, R8, y, nullptr, false, window, band_bin0, band_ptr, band_w, mel, mag, phase, B, N, NFFT, hop, NFFT,
                        n_mel, nullptr, stream);
}

// The collated batch of the data path (data.py:207-229 pads every mel with zeros to the longest one): y [B,N] zero-padded audio,
// utterance b holds n_samples[b] samples (device int32) -> mel [B,n_mel,T_out]: frames < n_samples[b] / hop + 1 as ft_stft_r8
// computes them for that utterance alone (reflection about ITS last sample), zeros beyond.  ONE launch for the batch instead of
// one per utterance (each ~35 us of latency for <= 862 frames).  T_out >= max_b (n_samples[b] / hop + 1).
extern "C" int ft_stft_r8_ragged(const float* y, const int32_t* n_samples, const float* window, const int32_t* band_bin0,
                                 const int32_t* band_ptr, const float* band_w, float* mel, int B, int N, int hop, int n_mel,
                                 int T_out, void* stream) {
    return stft_forward(__func__, R8, y, n_samples, true, window, band_bin0, band_ptr, band_w, mel, nullptr, nullptr, B, N, NFFT, hop,
                        NFFT, n_mel, &T_out, stream);
}

// The spectrum of a ragged batch (the analysis step of griffin_lim_ragged): y [B,N], utterance b holds n_samples[b] samples
// (device int32) -> mag (NULL = skip the store: Griffin-Lim keeps the phase only) and phase [B,513,T_out], T_out = N / hop + 1:
// frames < n_samples[b] / hop + 1 exactly as ft_stft_r8 computes them for y[b, :n_samples[b]] alone (reflection about ITS last
// sample, so the samples behind it are never read), zeros beyond in every output that is written.  ONE launch for the batch.
extern "C" int ft_stft_r8_ragged_phase(const float* y, const int32_t* n_samples, const float* window, float* mag, float* phase,
                                       int B, int N, int hop, void* stream) {
    return stft_forward(__func__, R8, y, n_samples, true, window, nullptr, nullptr, nullptr, nullptr, mag, phase, B, N, NFFT, hop,
                        NFFT, 0, nullptr, stream);
}

// (mag, phase) [B,513,T] -> y [B, hop (T-1)]: STFT.inverse (audio_processing.py:237-263) for n_fft = 1024, hop <= 256;
// window: hann [1024] (win_length zero-padded by the caller), as ft_stft_r8.
extern "C" int ft_istft_r8(const float* mag, const float* phase, const float* window, float* y, int B, int T, int hop,
                           void* stream) {
    return stft_inverse(__func__, R8, mag, phase, nullptr, false, window, y, B, T, NFFT, hop, NFFT, stream);
}

// The inverse of a ragged batch (the synthesis step of griffin_lim_ragged): (mag, phase) [B,513,T] with row stride T, utterance b
// holds n_frames[b] frames (device int32, 1 <= n_frames[b] <= T) -> y [B, hop (T-1)]: the samples n < hop (n_frames[b] - 1)
// exactly as ft_istft_r8 computes them for mag[b, :, :n_frames[b]] alone (the covering frames, the wss sum and both 512-sample
// trims use ITS frame count; the same ascending-t overlap-add and > FLT_MIN rule), zeros behind.  Frames t >= n_frames[b] are
// never read.  ONE launch for the batch, no atomics, launch-independent.  Same preconditions as ft_istft_r8.
extern "C" int ft_istft_r8_ragged(const float* mag, const float* phase, const int32_t* n_frames, const float* window, float* y,
                                  int B, int T, int hop, void* stream) {
    return stft_inverse(__func__, R8, mag, phase, n_frames, true, window, y, B, T, NFFT, hop, NFFT, stream);
}
