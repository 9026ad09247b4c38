// What the two STFT kernel families share (csrc/stft_r8.hip: n_fft = 1024, hop <= 256; csrc/stft_pow2.hip: every power-of-two
// n_fft = 256 .. 4096): complex arithmetic and the small DFTs, the parameter blocks, the polar step of the inverse, and the host
// side of the ten entry points (validation, parameter block, launch).  Each file keeps its FFT engine, twiddle tables, LDS
// layout, span staging and overlap-add scheme -- and, for now, its own text of the reflect rule, the split steps, the CSR
// filterbank, the ragged tail and the mel tile store: hipcc optimises a helper before it inlines it, and for each of these the
// kernels came out with other instructions than from the same text written in place.  A piece moves here only when all 12
// kernels (stft_r8_k, istft_r8_k, stft_pow2_k<7..11>, istft_pow2_k<7..11>) keep their instruction streams.
// Included inside the anonymous namespace of stft_r8.hip and stft_pow2.hip (after common.h and <cfloat>).
#pragma once

constexpr int BWMAX = 2048;                            // CSR values staged in LDS when they fit (Slaney, 80 bands at 1024: ~1 000)

struct cpx { float re, im; };
__device__ __forceinline__ cpx cmul(cpx a, cpx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cpx cadd(cpx a, cpx b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cpx csub(cpx a, cpx b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cpx mul_mi(cpx a) { return {a.im, -a.re}; }                       // a * (-i)

// the LDS operations of one wave execute in order: waiting for them is all a wave needs between its own writes and reads
__device__ __forceinline__ void lds_order() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// in-place forward DFT of R = 2, 4, 8 points (e^{-2 pi i jk/R}), natural order in and out
__device__ __forceinline__ void dft(cpx (&v)[2]) {
    const cpx a = v[0];
    v[0] = cadd(a, v[1]);
    v[1] = csub(a, v[1]);
}
__device__ __forceinline__ void dft(cpx (&v)[4]) {
    const cpx a0 = cadd(v[0], v[2]), a1 = csub(v[0], v[2]), a2 = cadd(v[1], v[3]), a3 = mul_mi(csub(v[1], v[3]));
    v[0] = cadd(a0, a2); v[2] = csub(a0, a2);
    v[1] = cadd(a1, a3); v[3] = csub(a1, a3);
}
__device__ __forceinline__ void dft(cpx (&v)[8]) {
    const float r = 0.70710678118654752f;
    cpx a0 = cadd(v[0], v[4]), a1 = csub(v[0], v[4]), a2 = cadd(v[2], v[6]), a3 = mul_mi(csub(v[2], v[6]));
    cpx a4 = cadd(v[1], v[5]), a5 = csub(v[1], v[5]), a6 = cadd(v[3], v[7]), a7 = mul_mi(csub(v[3], v[7]));
    cpx b0 = cadd(a0, a2), b2 = csub(a0, a2), b1 = cadd(a1, a3), b3 = csub(a1, a3);
    cpx b4 = cadd(a4, a6), b6 = mul_mi(csub(a4, a6)), b5 = cadd(a5, a7), b7 = csub(a5, a7);
    b5 = (cpx){r * (b5.re + b5.im), r * (b5.im - b5.re)};                                     // * e^{-i pi/4}
    b7 = (cpx){r * (b7.im - b7.re), -r * (b7.re + b7.im)};                                    // * e^{-3 i pi/4}
    v[0] = cadd(b0, b4); v[4] = csub(b0, b4);
    v[1] = cadd(b1, b5); v[5] = csub(b1, b5);
    v[2] = cadd(b2, b6); v[6] = csub(b2, b6);
    v[3] = cadd(b3, b7); v[7] = csub(b3, b7);
}

// ---- forward: y [B,N] -> mel / mag / phase.  H = n_fft / 2 below; a spectrum has H + 1 bins.
struct StftP {
    const float* y; const float* window;
    const int* band_bin0; const int* band_ptr; const float* band_w;      // CSR of the filterbank: band b covers bins
    float* mel; float* mag; float* phase;                                // [bin0[b], bin0[b] + ptr[b+1] - ptr[b])
    int N, hop, n_mel, n_frames;
    const int* n_samples;            // ragged batch: utterance b holds n_samples[b] <= N samples and n_samples[b] / hop + 1
    int ldt;                         // frames; frames beyond that are written as zeros; ldt = output row stride
    int fpw;                         // frames per wave (stft_pow2_k; stft_r8_k has FPW)
};                                   // phase without mag (ft_stft_*_ragged_phase): the magnitude store is skipped

// ---- inverse: (magnitude, phase) [B,H+1,T] -> y [B, hop (T-1)]
struct IstftP {
    const float* mag; const float* phase; const float* window;
    float* y;
    int T, hop, n_out;               // T: frames per spectrum row (the row stride), n_out = hop (T - 1): samples per output row
    const int* n_frames;             // ragged batch (ft_istft_*_ragged): utterance b holds n_frames[b] <= T frames; later frames are
};                                   // never read and the samples from hop (n_frames[b] - 1) on are written as zeros

// X[k] = M e^{i phase} in place over the raw (M, phase) pairs parked in X[0 .. H]; Im X[0] and Im X[H] dropped (irfft ignores
// them).  The accurate sincosf (full range reduction, many registers) runs one bin at a time.
__device__ __forceinline__ void polar_to_cpx(cpx* X, int H, int lane) {
#pragma unroll 1
    for (int k = lane; k <= H; k += 64) {
        const cpx mp = X[k];
        float s, c;
        sincosf(mp.im, &s, &c);
        X[k] = (cpx){mp.re * c, (k & (H - 1)) == 0 ? 0.f : mp.re * s};
    }
}

// ---- host: one launch path per direction for the ten entry points ft_stft_{r8,pow2}{,_ragged,_ragged_phase} and
// ft_istft_{r8,pow2}{,_ragged}.  A family is its two launchers and the two numbers its scope differs in.
struct StftFamily {
    int (*stft)(StftP p, int B, int n_fft, hipStream_t s);
    int (*istft)(const IstftP& p, int B, int n_fft, hipStream_t s);
    int hop_max;                     // r8: 256 (16 hop owned samples in 256 x 16 registers, the span in static LDS)
    int own_pad;                     // samples past n_out + 2 n_fft the inverse's indices reach: a workgroup's owned span when it
};                                   // does not shrink with the hop (pow2: OWN)

int log2_pow2_nfft(int n_fft) {                        // 8 .. 12 for n_fft = 256 .. 4096, -1 otherwise
    for (int l = 8; l <= 12; ++l) if (n_fft == (1 << l)) return l;
    return -1;
}

// FT_CHECK_ARG and FT_CHECK_LAUNCH under the name of the entry point that was called (__func__ would name the helper)
#define FT_ENTRY_ARG(cond)                                                            \
    do {                                                                              \
        if (!(cond)) return ft_fail(FT_EINVAL, "%s: invalid argument: %s", fn, #cond); \
    } while (0)

int stft_launched(const char* fn, int rc) {
    if (rc != FT_OK) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return ft_fail(FT_EHIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return FT_OK;
}

// Forward.  fn: the entry point's name.  ragged: n_samples is required (a dense entry passes NULL and false).  T_out: the row
// stride and frame count of a collated mel batch (ft_stft_*_ragged), NULL = N / hop + 1.  The r8 entries are n_fft = win_length
// = 1024 under fam.hop_max = 256.
int stft_forward(const char* fn, const StftFamily& fam, const float* y, const int32_t* n_samples, bool ragged, const float* window,
                 const int32_t* band_bin0, const int32_t* band_ptr, const float* band_w, float* mel, float* mag, float* phase,
                 int B, int N, int n_fft, int hop, int win_length, int n_mel, const int* T_out, void* stream) {
    FT_ENTRY_ARG(y && window && (n_samples || !ragged));
    FT_ENTRY_ARG((mel || phase) && (phase || !mag));                      // phase alone: the ragged analysis step of Griffin-Lim
    FT_ENTRY_ARG(ragged || (mag == nullptr) == (phase == nullptr));
    FT_ENTRY_ARG(!mel || (band_bin0 && band_ptr && band_w && n_mel >= 1 && n_mel <= 128));
    FT_ENTRY_ARG(log2_pow2_nfft(n_fft) > 0 && hop >= 1 && hop <= win_length && win_length <= n_fft && hop <= fam.hop_max);
    FT_ENTRY_ARG(B >= 1 && B <= 65535 && N > n_fft / 2 && (!T_out || *T_out >= 1));
    const int n_frames = T_out ? *T_out : N / hop + 1;
    const StftP p{y, window, band_bin0, band_ptr, band_w, mel, mag, phase, N, hop, mel ? n_mel : 0, n_frames, n_samples, n_frames, 1};
    return stft_launched(fn, fam.stft(p, B, n_fft, reinterpret_cast<hipStream_t>(stream)));
}

// Inverse.  ragged: n_frames is required (a dense entry passes NULL and false).
int stft_inverse(const char* fn, const StftFamily& fam, const float* mag, const float* phase, const int32_t* n_frames, bool ragged,
                 const float* window, float* y, int B, int T, int n_fft, int hop, int win_length, void* stream) {
    FT_ENTRY_ARG(mag && phase && window && y && (n_frames || !ragged));
    FT_ENTRY_ARG(log2_pow2_nfft(n_fft) > 0 && hop >= 1 && hop <= win_length && win_length <= n_fft && hop <= fam.hop_max);
    FT_ENTRY_ARG(B >= 1 && B <= 65535 && T >= 2);
    FT_ENTRY_ARG((int64_t)hop * (T - 1) <= INT32_MAX - 2 * n_fft - fam.own_pad);
    const IstftP p{mag, phase, window, y, T, hop, hop * (T - 1), n_frames};
    return stft_launched(fn, fam.istft(p, B, n_fft, reinterpret_cast<hipStream_t>(stream)));
}
