// Mel-cepstral distortion along a dynamic-time-warping path (additive: the reference has no metric of its own).
//
// ft_mel_cepstra: cep[b][t][k-1] = sum_m mel[b][m][t] * D[k-1][m], k = 1 .. K (c0 left out), m ascending, every product and
// every sum rounded to fp32 on its own.  D is the caller's fp32 DCT-II table.  A thread owns one frame and all K sums; the
// table sits in LDS and is read as broadcasts.
//
// ft_dtw_ragged: per pair b, A = x_lens[b] and N = y_lens[b] frames of K features:
//     d[i][j] = sqrt(sum_k (x[i][k] - y[j][k])^2)                  k ascending; sub, mul, add, sqrt: one fp32 rounding each
//     C[0][0] = d[0][0];  i == 0: move 2 (from (i, j-1));  j == 0: move 1 (from (i-1, j))
//     else best = C[i-1][j-1], move 0;  if C[i-1][j] < best: move 1;  if C[i][j-1] < best: move 2      (strict)
//     C[i][j] = d[i][j] + best;  backtrack from (A-1, N-1)
//   * the sibling of mas_k (align.hip): one workgroup per pair, thread j = column j, A + N - 1 dependent anti-diagonal steps
//     s = i + j.  At step s a thread needs its own last value (up), its left neighbour's value of step s - 1 (left) and the
//     neighbour's value of step s - 2 (diagonal).  The last is what the thread read as `left` one step earlier, so it stays
//     in a register: one LDS read and one LDS write per step into two lines in rotation, one LDS-only barrier per step.
//   * distances come from the features on the fly: x's rows wait in LDS (row stride odd, so the 64 rows a wave reads at one
//     step fall on 64 different banks), a thread keeps its own y row in registers.  The K of a launch is rounded up to the
//     next compiled width with zero features: (0 - 0)^2 adds +0 to a non-negative sum, which changes no bit.  The distance of
//     step s + 1 does not depend on step s and is computed while the line's write drains.
//   * backpointers are two bits per cell: the ballots of the compares combine, as scalar mask arithmetic, into the words of
//     `move == 1` and `move == 2`, two 64-bit words per wave and step, [B][ceil(Tb / 64)][Ta + Tb - 1][2] in the caller's
//     workspace.  Lane (s mod 64) of the wave keeps step s's pair in registers and every 64 steps the wave stores its 1 KiB as
//     whole lines, so a step issues no store.  A wave none of whose columns has a cell at a step or the next sleeps
//     through it, barrier apart.  The backtrack is the first wave's: 64 anti-diagonals per memory round trip (the path
//     loses at most one column per anti-diagonal, so two waves' words cover them), every lane picks the move of ITS
//     anti-diagonal at the path's current column and one lane read fetches the one that counts; the walk's state is
//     scalar.  The cells go to LDS last to first and leave in ascending order as whole lines.
//   * lengths are clamped to 1 ..= Ta and 1 ..= Tb in the kernel and every index is bounded by the clamped lengths; all
//     addressing that involves B, Ta, Tb is 64-bit.  No atomics, no communication between workgroups.
//   * diagonal: cells i == j only, cost = running sum of d[i][i]; a pair with A != N: path_len 0, cost +inf.
#include "common.h"

// the float32 replay on the host multiplies, adds and subtracts one rounding at a time: hipcc would otherwise contract
// acc + d * d into v_fmac_f32 (the _rn intrinsics do not prevent it)
#pragma clang fp contract(off)

namespace {

constexpr int DTW_MAX_T = 1024;                 // frames per side: one thread per column of y, the rows of x in LDS
constexpr int DTW_MAX_K = 32;
constexpr int CEP_MAX_M = 128;
constexpr int CEP_THREADS = 256;

__device__ __forceinline__ void lds_barrier() {                     // align.hip: drains LDS traffic only
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// KP: the compiled number of sums, >= the launch's K; the table's rows behind K are zero and their sums are not stored
template <int KP>
__global__ __launch_bounds__(CEP_THREADS) void mel_cepstra_k(const float* __restrict__ mel, int64_t sb, int64_t sm, int64_t st,
                                                            const int32_t* __restrict__ lens, const float* __restrict__ dct,
                                                            float* __restrict__ cep, int M, int T, int K) {
    __shared__ float D[CEP_MAX_M * KP];                             // [m][k]
    const int b = blockIdx.y, t = blockIdx.x * CEP_THREADS + threadIdx.x;
    const int Tb = lens ? min(max(lens[b], 1), T) : T;
    if (blockIdx.x * CEP_THREADS >= Tb) return;                     // (uniform over the workgroup)
    for (int e = threadIdx.x; e < M * KP; e += CEP_THREADS) {
        const int m = e / KP, k = e - m * KP;
        D[e] = k < K ? dct[k * M + m] : 0.f;
    }
    __syncthreads();
    if (t >= Tb) return;
    const float* src = mel + b * sb + t * st;
    float acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.f;
    for (int m = 0; m < M; ++m) {
        const float v = src[m * sm];
#pragma unroll
        for (int k = 0; k < KP; ++k) acc[k] = acc[k] + v * D[m * KP + k];
    }
    float* out = cep + ((int64_t)b * T + t) * K;
#pragma unroll
    for (int k = 0; k < KP; ++k)
        if (k < K) out[k] = acc[k];
}

struct DtwArgs {
    const float* x;
    int64_t sxb, sxt, sxk;                      // element strides of (pair, frame, feature)
    const float* y;
    int64_t syb, syt, syk;
    const int32_t* x_lens;
    const int32_t* y_lens;
    float* cost;                                // [B]
    int32_t* path_len;                          // [B]
    int32_t* path;                              // [B][Ta + Tb - 1][2]
    unsigned long long* bits;                   // [B][W][Ta + Tb - 1][2]
    int Ta, Tb, K, W, diagonal;
};

// KP: the compiled feature width, >= the launch's K
template <int KP>
__global__ __launch_bounds__(1024) void dtw_k(DtwArgs p) {
    constexpr int KS = KP | 1;                                      // row stride of x in LDS: odd
    constexpr int XS_FLOATS = DTW_MAX_T * KS > 4 * DTW_MAX_T ? DTW_MAX_T * KS : 4 * DTW_MAX_T;
    __shared__ float xs[XS_FLOATS];                                 // x's rows; after the DP the path's cells, last to first
    __shared__ float line[2][DTW_MAX_T + 1];                        // [.][0] stands in front of column 0 (never selected)
    __shared__ int n_cells;
    const int b = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6;
    const int A = min(max(p.x_lens[b], 1), p.Ta), N = min(max(p.y_lens[b], 1), p.Tb);
    const int P = p.Ta + p.Tb - 1;
    int32_t* path = p.path + (int64_t)b * P * 2;
    int2* cells = reinterpret_cast<int2*>(xs);

    if (p.diagonal && A != N) {                                     // (uniform over the workgroup)
        for (int n = j; n < 2 * P; n += blockDim.x) path[n] = -1;
        if (j == 0) { p.cost[b] = INFINITY; p.path_len[b] = 0; }
        return;
    }

    const float* x = p.x + b * p.sxb;
    for (int e = j; e < A * KP; e += blockDim.x) {
        const int i = e / KP, k = e - i * KP;
        xs[i * KS + k] = k < p.K ? x[i * p.sxt + k * p.sxk] : 0.f;
    }
    const bool col = j < N;
    float yk[KP];
    {
        const float* y = p.y + b * p.syb + (col ? j : 0) * p.syt;
#pragma unroll
        for (int k = 0; k < KP; ++k) yk[k] = (col && k < p.K) ? y[k * p.syk] : 0.f;
    }
    if (j == 0) { line[0][0] = 0.f; line[1][0] = 0.f; }
    // y's row has arrived HERE: left to itself hipcc waits for it at its first use, inside the step loop, and that wait
    // (vmcnt(0)) would also wait for the backpointer words just stored, a memory round trip per step
#pragma unroll
    for (int k = 0; k < KP; ++k) asm volatile("" : "+v"(yk[k]));
    __syncthreads();

    auto dist = [&](int i) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const float df = xs[i * KS + k] - yk[k];
            acc = acc + df * df;
        }
        return sqrtf(acc);
    };

    if (p.diagonal) {
        if (col) line[0][j] = dist(j);                              // d[j][j]
        __syncthreads();
        if (j == 0) {
            float c = line[0][0];
            for (int i = 1; i < A; ++i) c = line[0][i] + c;
            p.cost[b] = c;
            p.path_len[b] = A;
        }
        for (int n = j; n < P; n += blockDim.x) {
            const int v = n < A ? n : -1;
            path[2 * n] = v;
            path[2 * n + 1] = v;
        }
        return;
    }

    unsigned long long* bits = p.bits + (int64_t)b * P * p.W * 2;
    const int S = A + N - 1;
    // step 0 is cell (0, 0) alone; its move is never followed
    float c = 0.f, diag = 0.f;
    float d = 0.f;                                                  // the distance of the step to come
    if (j == 0) {
        c = dist(0);
        line[1][1] = c;
        if (A > 1) d = dist(1);
    } else if (j == 1 && col) {
        d = dist(0);
    }
    __syncthreads();
    const int j_lo = wave * 64, j_hi = min(j_lo + 63, N - 1);       // this wave's columns
    const bool top_col = j == 0;
    const unsigned long long edge = wave == 0 ? 1ull : 0ull;        // the lanes of column 0, as a ballot
    unsigned long long w1 = 0ull, w2 = 0ull;                        // the backpointer words this lane keeps
    bool dirty = false;
    int cur = 1;
    for (int s = 1; s < S; ++s) {
        // (uniform over the wave) a wave whose columns all lie outside rows 0 .. A-1 at this step and the next only keeps the
        // barrier: its first cell is its first column's at s = j_lo, and the `left` a cell needs as its diagonal one step
        // later is read from the step before its column's first on, when the wave is already awake
        if (j_lo <= j_hi && s + 1 >= j_lo && s - j_hi < A) {
            const int i = s - j;
            const bool on = col && (unsigned)i < (unsigned)A;
            const float left = line[cur][j];                        // C[i][j-1]: the neighbour's value of step s - 1
            // without branches: the three-way choice, then the borders over it; the moves as whole-wave masks
            const bool up = c < diag;
            float best = up ? c : diag;
            const bool lf = left < best;
            best = lf ? left : best;
            best = i == 0 ? left : (top_col ? c : best);
            const unsigned long long m_on = __builtin_amdgcn_ballot_w64(on), m_top = __builtin_amdgcn_ballot_w64(i == 0);
            const unsigned long long m_up = __builtin_amdgcn_ballot_w64(up), m_lf = __builtin_amdgcn_ballot_w64(lf);
            if (on) {
                c = d + best;
                line[cur ^ 1][j + 1] = c;
            }
            diag = left;
            // lane (s mod 64) keeps this step's two words; a chunk of 64 steps leaves as whole lines below
            const bool keeper = lane == (s & 63);
            w1 = keeper ? m_on & ~m_top & (edge | (m_up & ~m_lf)) : w1;     // move 1
            w2 = keeper ? m_on & (m_top | (~edge & m_lf)) : w2;             // move 2
            dirty = true;
            const int in = i + 1;                                   // this column's row at step s + 1
            if (col && (unsigned)in < (unsigned)A && s + 1 < S) d = dist(in);
        }
        if (dirty && ((s & 63) == 63 || s == S - 1)) {              // (uniform over the wave)
            const int sl = (s & ~63) + lane;
            if (sl <= s) *reinterpret_cast<ulonglong2*>(bits + ((int64_t)wave * P + sl) * 2) = make_ulonglong2(w1, w2);
            dirty = false;
        }
        lds_barrier();
        cur ^= 1;
    }
    if (j == N - 1) p.cost[b] = c;
    __syncthreads();                            // every wave's backpointer words have landed; xs is free

    if (wave == 0) {
        // the walk's state is the same in every lane: held in scalar registers, so that its loop control is scalar and the
        // move comes through a lane read, not through LDS
        int i = __builtin_amdgcn_readfirstlane(A - 1), jj = __builtin_amdgcn_readfirstlane(N - 1), total = 0;
        bool done = false;
        while (!done) {
            const int s0 = i + jj, w = jj >> 6; // the path stays in waves w and w - 1 over these 64 anti-diagonals
            const int sq = s0 - lane;
            unsigned long long h1 = 0ull, h2 = 0ull, l1 = 0ull, l2 = 0ull;
            if (sq >= 0) {
                const unsigned long long* src = bits + ((int64_t)w * P + sq) * 2;
                h1 = src[0];
                h2 = src[1];
                if (w > 0) { l1 = src[-2 * (int64_t)P]; l2 = src[-2 * (int64_t)P + 1]; }
            }
            int cnt = 0, mi = 0, mj = 0;
            for (;;) {
                const int q = s0 - (i + jj);
                if (q >= 64) break;
                if (lane == cnt) { mi = i; mj = jj; }
                ++cnt;
                if (i + jj == 0) { done = true; break; }
                const bool upper = (jj >> 6) == w;
                const int bit = jj & 63;
                const int mine = (int)(((upper ? h1 : l1) >> bit) & 1ull) | ((int)(((upper ? h2 : l2) >> bit) & 1ull) << 1);
                const int m = __builtin_amdgcn_readlane(mine, q);
                // move 1 leaves the column, move 2 the row, move 0 neither; the border moves are structural, as in the
                // forward pass
                const int di = i == 0 ? 0 : (jj == 0 ? 1 : ((m & 1) | ((m >> 1) ^ 1)));
                const int dj = i == 0 ? 1 : (jj == 0 ? 0 : ((m & 1) ^ 1));
                i -= di;
                jj -= dj;
            }
            if (lane < cnt) cells[total + lane] = make_int2(mi, mj);
            total += cnt;
        }
        if (lane == 0) { n_cells = total; p.path_len[b] = total; }
    }
    __syncthreads();
    const int total = n_cells;
    for (int n = j; n < P; n += blockDim.x) {
        int2 v = make_int2(-1, -1);
        if (n < total) v = cells[total - 1 - n];
        path[2 * n] = v.x;
        path[2 * n + 1] = v.y;
    }
}

template <int KP>
void dtw_launch(const DtwArgs& p, int B, hipStream_t st) {
    hipLaunchKernelGGL(dtw_k<KP>, dim3(B), dim3(p.W * 64), 0, st, p);
}

// the compiled widths: the smallest one that holds K features
#define DTW_WIDTHS(K, CALL)     \
    do {                        \
        if (K <= 1) CALL(1);    \
        else if (K <= 4) CALL(4);   \
        else if (K <= 8) CALL(8);   \
        else if (K <= 13) CALL(13); \
        else if (K <= 16) CALL(16); \
        else if (K <= 24) CALL(24); \
        else CALL(32);          \
    } while (0)

}  // namespace

extern "C" int ft_mel_cepstra(const float* mel, int64_t stride_b, int64_t stride_m, int64_t stride_t, const int32_t* lens,
                              const float* dct, float* cep, int B, int M, int T, int K, void* stream) {
    FT_CHECK_ARG(mel && dct && cep);
    FT_CHECK_ARG(B >= 1 && M >= 1 && T >= 1 && K >= 1);
    FT_CHECK_ARG(stride_b >= 0 && stride_m >= 0 && stride_t >= 0);
    FT_CHECK_ARG(B <= 65535);
    if (K > DTW_MAX_K || K >= M || M > CEP_MAX_M)
        return ft_fail(FT_EUNSUPPORTED, "%s: K = %d of M = %d, the transform holds 1 <= K <= %d, K < M <= %d", __func__, K, M,
                       DTW_MAX_K, CEP_MAX_M);
#define CEP_LAUNCH(KP)                                                                                                            \
    hipLaunchKernelGGL(mel_cepstra_k<KP>, dim3(cdiv(T, CEP_THREADS), B), dim3(CEP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), \
                       mel, stride_b, stride_m, stride_t, lens, dct, cep, M, T, K)
    DTW_WIDTHS(K, CEP_LAUNCH);
#undef CEP_LAUNCH
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" size_t ft_dtw_workspace_bytes(int B, int Ta, int Tb, int K) {
    if (B < 1 || Ta < 1 || Tb < 1 || K < 1) return 0;
    return (size_t)B * ((size_t)Ta + (size_t)Tb - 1) * (size_t)cdiv(Tb, 64) * 2 * sizeof(unsigned long long);
}

extern "C" int ft_dtw_ragged(const float* x, int64_t x_stride_b, int64_t x_stride_t, int64_t x_stride_k, const float* y,
                             int64_t y_stride_b, int64_t y_stride_t, int64_t y_stride_k, const int32_t* x_lens, const int32_t* y_lens,
                             float* cost, int32_t* path_len, int32_t* path, void* work, size_t work_bytes, int B, int Ta, int Tb, int K,
                             int diagonal, void* stream) {
    FT_CHECK_ARG(x && y && x_lens && y_lens && cost && path_len && path && work);
    FT_CHECK_ARG(B >= 1 && Ta >= 1 && Tb >= 1 && K >= 1);
    FT_CHECK_ARG(x_stride_b >= 0 && x_stride_t >= 0 && x_stride_k >= 0 && y_stride_b >= 0 && y_stride_t >= 0 && y_stride_k >= 0);
    FT_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 15) == 0);
    if (Ta > DTW_MAX_T || Tb > DTW_MAX_T)
        return ft_fail(FT_EUNSUPPORTED, "%s: %d x %d frames, the warp holds at most %d per side", __func__, Ta, Tb, DTW_MAX_T);
    if (K > DTW_MAX_K) return ft_fail(FT_EUNSUPPORTED, "%s: K = %d features, the warp holds at most %d", __func__, K, DTW_MAX_K);
    FT_CHECK_ARG(work_bytes >= ft_dtw_workspace_bytes(B, Ta, Tb, K));
    const int W = cdiv(Tb, 64);
    const DtwArgs p{x, x_stride_b, x_stride_t, x_stride_k, y, y_stride_b, y_stride_t, y_stride_k, x_lens, y_lens, cost, path_len,
                    path, static_cast<unsigned long long*>(work), Ta, Tb, K, W, diagonal != 0 ? 1 : 0};
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define DTW_LAUNCH(KP) dtw_launch<KP>(p, B, st)
    DTW_WIDTHS(K, DTW_LAUNCH);
#undef DTW_LAUNCH
    FT_CHECK_LAUNCH();
    return FT_OK;
}
