// Token durations from attention, and alignments from durations (additive: the reference has no alignment search).
//
// ft_mas_ragged: monotonic alignment search, the Viterbi counterpart of the alpha recursion of ctc.hip over the same [T, L]
// grid.  Per utterance b, T_b = out_lens[b] frames, L_b = in_lens[b] <= T_b tokens, s = its fp32 scores:
//     Q[0][0] = s[0][0]
//     Q[t][l] = s[t][l] + (adv[t][l] ? Q[t-1][l-1] : Q[t-1][l])              l <= min(t, L_b - 1)
//     adv[t][l] = l > 0 && (l == t || Q[t-1][l-1] > Q[t-1][l])               (strict: a tie stays)
//     backtrack from (T_b - 1, L_b - 1):  path[t] = l;  l -= adv[t][l]
//   * one fp32 add and one compare per cell, nothing the compiler can contract: a float32 replay on the host gives the same
//     bits.  Among the best paths the rule picks the one that advances earliest; the `l == t` clause keeps the path valid
//     (path[0] = 0, path[T_b-1] = L_b-1, steps of 0 or 1) even when every score is -inf.
//   * one workgroup per utterance, thread l = token l, T_b dependent row steps; the row lives in a double-buffered LDS line
//     (one LDS-only barrier per step, as in ctc.hip), the scores of the next four rows are requested before the current four
//     are used.
//   * backpointers are ONE BIT per cell: each wave's ballot of adv is one 64-bit word, stored by its first lane into the
//     caller's workspace [B][T][ceil(L/64)].  The backtrack is the first wave's: 64 rows at a time, lane i loads the two words
//     of row t0 - i that the path can still reach (it moves by at most one token per row), the walk itself runs over lanes'
//     registers -- one memory round trip per 64 rows, not per row.
//   * durations need no atomics: the path is monotone, so token l starts at the first frame whose path entry is l.
//   * lengths are clamped to 1 ..= L and 1 ..= T in the kernel and every index is bounded by the clamped lengths: nothing
//     behind an utterance's frames or tokens is read, and no length can send an access out of bounds.  L_b > T_b (no monotone
//     path exists): path -1, durations 0, score -inf.
//
// ft_durations_to_rows: rows[b][n][l] = 1 where cum[l-1] <= n < cum[l] and l < L_b (cum = running sum of max(d, 0)), else 0;
// reverse: utterance b's rows in reversed time (n -> total_b - 1 - n), the orientation odd flows decode in.  A workgroup
// writes DR_ROWS rows of one utterance: it scans the durations (wave scan + carry, any L) and notes, for each of its rows,
// the token that owns it; then the rows are written as whole lines.
#include "common.h"

namespace {

constexpr int MAS_MAX_L = 1024;
constexpr int MAS_AHEAD = 4;                    // score rows requested ahead of the dependent chain
constexpr int DR_THREADS = 256;
constexpr int DR_ROWS = 32;

// workgroup barrier that drains LDS traffic only (ctc.hip): __syncthreads() would also wait for the prefetched score rows
// and the backpointer words just stored, a memory round trip per DP step
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

struct MasArgs {
    const float* logp;
    int64_t sb, st, sl;                         // element strides of (utterance, frame, token)
    const int32_t* in_lens;
    const int32_t* out_lens;
    unsigned long long* bits;                   // [B][T][W]
    int32_t* path;                              // [B][T]
    int32_t* dur;                               // [B][L]
    float* score;                               // [B] | NULL
    int T, L, W;
};

__global__ __launch_bounds__(1024) void mas_k(MasArgs p) {
    __shared__ float qrow[2][MAS_MAX_L + 1];    // [.][0] is the guard in front of token 0 (never selected: l > 0 in adv)
    __shared__ int start[MAS_MAX_L + 1];
    const int b = blockIdx.x, l = threadIdx.x, lane = l & 63, wave = l >> 6;
    const int Lb = min(max(p.in_lens[b], 1), p.L), Tb = min(max(p.out_lens[b], 1), p.T);
    int32_t* path = p.path + (int64_t)b * p.T;
    int32_t* dur = p.dur + (int64_t)b * p.L;
    for (int t = Tb + l; t < p.T; t += blockDim.x) path[t] = -1;
    for (int k = Lb + l; k < p.L; k += blockDim.x) dur[k] = 0;
    if (Lb > Tb) {                              // (uniform over the workgroup)
        for (int t = l; t < Tb; t += blockDim.x) path[t] = -1;
        for (int k = l; k < Lb; k += blockDim.x) dur[k] = 0;
        if (p.score && l == 0) p.score[b] = -INFINITY;
        return;
    }
    const bool tok = l < Lb;
    const float* s = p.logp + b * p.sb + (tok ? l : 0) * p.sl;
    unsigned long long* bits = p.bits + (int64_t)b * p.T * p.W;

    // row 0, and the first rows of scores
    float q = (l == 0) ? s[0] : -INFINITY;
    qrow[0][l + 1] = q;
    if (l == 0) { qrow[0][0] = -INFINITY; qrow[1][0] = -INFINITY; }
    if (lane == 0 && wave < p.W) bits[wave] = 0ull;
    float sc[MAS_AHEAD], scn[MAS_AHEAD];
#pragma unroll
    for (int u = 0; u < MAS_AHEAD; ++u) {
        const int t = 1 + u;
        sc[u] = (tok && t < Tb && l <= t) ? s[t * p.st] : 0.f;
    }
    __syncthreads();
    int cur = 0;
    for (int tb = 1; tb < Tb; tb += MAS_AHEAD) {
#pragma unroll
        for (int u = 0; u < MAS_AHEAD; ++u) {
            const int t = tb + MAS_AHEAD + u;
            scn[u] = (tok && t < Tb && l <= t) ? s[t * p.st] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < MAS_AHEAD; ++u) {
            const int t = tb + u;
            if (t < Tb) {                       // (uniform over the workgroup)
                const bool on = tok && l <= t;
                const float left = qrow[cur][l];                      // Q[t-1][l-1]
                const bool adv = on && l > 0 && (l == t || left > q);
                if (on) q = sc[u] + (adv ? left : q);
                qrow[cur ^ 1][l + 1] = q;
                const unsigned long long word = __ballot(adv);
                if (lane == 0 && wave < p.W) bits[(int64_t)t * p.W + wave] = word;
                lds_barrier();
                cur ^= 1;
            }
        }
#pragma unroll
        for (int u = 0; u < MAS_AHEAD; ++u) sc[u] = scn[u];
    }
    if (p.score && l == Lb - 1) p.score[b] = q;
    __syncthreads();                            // every wave's backpointer words have landed (vmcnt(0) + barrier)

    if (wave == 0) {
        int at = Lb - 1;                        // the same in every lane
        for (int t0 = Tb - 1; t0 >= 0; t0 -= 64) {
            const int t = t0 - lane;
            const int w = at >> 6;              // the path stays in words w and w - 1 over these 64 rows
            unsigned long long hi = 0ull, lo = 0ull;
            if (t >= 0) {
                hi = bits[(int64_t)t * p.W + w];
                if (w > 0) lo = bits[(int64_t)t * p.W + w - 1];
            }
            const int n = min(64, t0 + 1);
            int mine = 0;
            for (int i = 0; i < n; ++i) {
                const unsigned h0 = __shfl((unsigned)hi, i, 64), h1 = __shfl((unsigned)(hi >> 32), i, 64);
                const unsigned l0 = __shfl((unsigned)lo, i, 64), l1 = __shfl((unsigned)(lo >> 32), i, 64);
                if (lane == i) mine = at;
                const bool upper = (at >> 6) == w;
                const unsigned long long word = upper ? ((unsigned long long)h1 << 32 | h0) : ((unsigned long long)l1 << 32 | l0);
                at -= (int)((word >> (at & 63)) & 1ull);
            }
            if (t >= 0) path[t] = mine;
        }
    }
    __syncthreads();
    // token k starts at the first frame whose path entry is k (every token owns at least one frame)
    for (int t = l; t < Tb; t += blockDim.x) {
        const int k = path[t];
        if (t == 0 || path[t - 1] != k) start[k] = t;
    }
    if (l == 0) start[Lb] = Tb;
    __syncthreads();
    if (tok) dur[l] = start[l + 1] - start[l];
}

__device__ __forceinline__ long long wave_scan_incl(long long v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long u = __shfl_up(v, off, 64);
        if (lane >= off) v += u;
    }
    return v;
}

__global__ __launch_bounds__(DR_THREADS) void dur_rows_k(const int32_t* __restrict__ durations, const int32_t* __restrict__ in_lens,
                                                         float* __restrict__ rows, int N, int L, int chunks, int reverse) {
    __shared__ long long wsum[DR_THREADS / 64];
    __shared__ int owner[DR_ROWS];
    const int b = blockIdx.x / chunks, n0 = (blockIdx.x - b * chunks) * DR_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int Lb = min(max(in_lens[b], 1), L);
    const int32_t* d = durations + (int64_t)b * L;
    long long total = 0;
    if (reverse) {                              // the utterance's frames, before any row can be placed
        long long v = 0;
        for (int k = tid; k < Lb; k += DR_THREADS) v += max(d[k], 0);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (lane == 0) wsum[wave] = v;
        __syncthreads();
        total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid < DR_ROWS) owner[tid] = -1;
    __syncthreads();
    long long carry = 0;
    for (int k0 = 0; k0 < Lb; k0 += DR_THREADS) {                          // (uniform trip count)
        const int k = k0 + tid;
        const long long dk = k < Lb ? max(d[k], 0) : 0;
        const long long incl = wave_scan_incl(dk, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        long long before = carry;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        const long long end = before + incl, beg = end - dk;               // token k owns frames beg .. end - 1
        carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (dk > 0) {
            const long long o0 = reverse ? total - end : beg, o1 = reverse ? total - beg : end;      // its rows as written
            const long long r0 = o0 > n0 ? o0 : n0;
            const long long r1 = o1 < (long long)n0 + DR_ROWS ? o1 : (long long)n0 + DR_ROWS;
            for (long long r = r0; r < r1; ++r) owner[(int)(r - n0)] = k;   // (at most DR_ROWS, each row has one owner)
        }
        __syncthreads();
    }
    const int nr = min(DR_ROWS, N - n0);
    float* out = rows + ((int64_t)b * N + n0) * L;
    for (int64_t i = tid; i < (int64_t)nr * L; i += DR_THREADS) {
        const int r = (int)(i / L), k = (int)(i - (int64_t)r * L);
        out[i] = owner[r] == k ? 1.f : 0.f;
    }
}

}  // namespace

extern "C" size_t ft_mas_workspace_bytes(int B, int T, int L) {
    if (B < 1 || T < 1 || L < 1) return 0;
    return (size_t)B * (size_t)T * (size_t)cdiv(L, 64) * sizeof(unsigned long long);
}

extern "C" int ft_mas_ragged(const float* logp, int64_t stride_b, int64_t stride_t, int64_t stride_l, const int32_t* in_lens,
                             const int32_t* out_lens, int32_t* path, int32_t* durations, float* score, void* work,
                             size_t work_bytes, int B, int T, int L, void* stream) {
    FT_CHECK_ARG(logp && in_lens && out_lens && path && durations && work);
    FT_CHECK_ARG(B >= 1 && T >= 1 && L >= 1);
    FT_CHECK_ARG(stride_b >= 0 && stride_t >= 0 && stride_l >= 0);
    FT_CHECK_ARG((reinterpret_cast<uintptr_t>(work) & 7) == 0);
    if (L > MAS_MAX_L) return ft_fail(FT_EUNSUPPORTED, "%s: L = %d tokens, the search holds at most %d", __func__, L, MAS_MAX_L);
    FT_CHECK_ARG(work_bytes >= ft_mas_workspace_bytes(B, T, L));
    const int W = cdiv(L, 64);
    const MasArgs p{logp, stride_b, stride_t, stride_l, in_lens, out_lens, static_cast<unsigned long long*>(work), path, durations,
                    score, T, L, W};
    hipLaunchKernelGGL(mas_k, dim3(B), dim3(W * 64), 0, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_durations_to_rows(const int32_t* durations, const int32_t* in_lens, float* rows, int B, int N, int L, int reverse,
                                    void* stream) {
    FT_CHECK_ARG(durations && in_lens && rows);
    FT_CHECK_ARG(B >= 1 && N >= 1 && L >= 1);
    const int chunks = cdiv(N, DR_ROWS);
    FT_CHECK_ARG((int64_t)B * chunks <= 2147483647LL);
    hipLaunchKernelGGL(dur_rows_k, dim3(B * chunks), dim3(DR_THREADS), 0, reinterpret_cast<hipStream_t>(stream), durations, in_lens,
                       rows, N, L, chunks, reverse != 0 ? 1 : 0);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
