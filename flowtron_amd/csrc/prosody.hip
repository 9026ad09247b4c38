// Pitch and pace of a zero-padded batch of utterances by time-domain pitch-synchronous overlap-add on the F0 track (additive:
// the reference has no F0 input).  include/flowtron_hip.h states the rule; tests/prosody_ref.py replays it bit for bit.
//
// ft_psola_marks: psola_marks_k, one wave (= one workgroup) per utterance, one launch for the batch.  Both recurrences are
//   serial chains of a few thousand dependent steps, so a step must not go to L2: the wave first forms per[t] and step[t] of the
//   utterance's frames, 64 frames at a time, and keeps the first PS_LDS_FRAMES of them in LDS (32 KB: 47 s at 22,050 Hz and a hop
//   of 256); a frame behind them is formed again from global memory where it is met.  The frame of a position is not divided out
//   per step: positions only grow, so a counter follows them (exactly floor(((p >> 8) + hop / 2) / hop)).  The walk runs
//   uniformly on all 64 lanes; lane 0 writes the marks with plain stores that nothing waits for.  The second walk forms the
//   analysis marks again beside the synthesis marks and never reads back what the first one stored.
// ft_psola_synth: psola_synth_k, one workgroup per tile of PS_TILE consecutive output samples of one utterance, a sample a lane.
//   The grains' centres ascend, so a binary search finds the first grain that can reach the tile (half-widths are at most 1024);
//   from there the workgroup stages PS_TILE grains at a time in LDS (centre, source centre, half-width and its reciprocal) and
//   every lane walks them upward, in ascending j as the rule demands, until a centre lies more than 1024 behind the tile.  The
//   grain is uniform over the workgroup (an LDS broadcast), the source reads x[m + d] are consecutive across the lanes, the
//   window table sits in LDS.  (|d| 1024) / half is not divided: q = int(float(|d| 1024) * (1.f / half)) is the quotient or one
//   below it (|d| 1024 < 2^20 and the quotient < 1024, so the product is within 2^-12 of the true value, which is an integer or
//   at least 2^-10 below the next one), and q += ((q + 1) half <= |d| 1024) makes it exact for every |d| < half <= 1024.
// ft_psola_marks_warp: psola_marks_warp_k, the same wave per utterance, the synthesis marks walking a time map instead of
//   s pace.  What the serial chain reads per step beyond per[] is staged too: the first PS_LDS_FRAMES entries of the map's row
//   and, for a ratio on the output's axis, of the clamped ratio (64 KB of LDS in all; an entry behind them comes from global
//   memory).  The output frame u of a mark is a counter like the input's (s only grows), the input frame of ta too, because the
//   rule's running maximum keeps ta from descending.  Each step adds at least 8 Q to s, so the walk ends at n_out whatever the
//   map, the ratio and F0 hold; u + 1 <= TM - 1 is held by a clamp besides the entry's refusal.
// ft_psola_time_map: psola_time_map_k, a workgroup per utterance.  mid[] lives in LDS (FT_PSOLA_MAX_PATH entries): the first
//   cell of a reference frame stores lo, after a barrier the last cell turns it into 128 hop (lo + hi) -- one writer per entry
//   in either pass, no atomics -- and after another barrier every thread averages 2 w + 1 entries for the map entries it owns.
// Every index is bounded by the clamped lengths and by the row capacities passed in; nothing at or behind n_samples[b] is read.
// No atomics, no scratch.
#include "common.h"

// the replay on the host rounds every operation on its own
#pragma clang fp contract(off)

namespace {

constexpr int PS_Q = 256;                       // positions are integers in 1 / 256 sample
constexpr int PS_MIN_PERIOD = 16;               // samples
constexpr int PS_MAX_PERIOD = 1024;
constexpr int PS_MAX_SAMPLES = 1 << 22;
constexpr int PS_HANN = 1024;
constexpr int PS_LDS_FRAMES = 4096;             // frames whose per / step the marks kernel keeps in LDS
constexpr int PS_TILE = 256;                    // output samples (= threads) of a workgroup of the synthesis
constexpr int PS_MIN_PACE_Q = 65536 / 4, PS_MAX_PACE_Q = 65536 * 4;
constexpr int PS_MAX_PATH = 4096;               // cells of a warping path (and reference frames) the time map kernel holds
constexpr int PS_MAX_SMOOTH = 32;
constexpr int PS_MAP_THREADS = 256;

static_assert(PS_Q == FT_PSOLA_Q && PS_MIN_PERIOD == FT_PSOLA_MIN_PERIOD && PS_MAX_PERIOD == FT_PSOLA_MAX_PERIOD,
              "the header names the units");
static_assert(PS_MAX_SAMPLES == FT_PSOLA_MAX_SAMPLES && PS_HANN == FT_PSOLA_HANN, "the header names the limits");
static_assert(PS_MAX_PATH == FT_PSOLA_MAX_PATH && PS_MAX_SMOOTH == FT_PSOLA_MAX_SMOOTH, "the header names the limits");

struct MarksArgs {
    const float* f0;
    int64_t f_sb, f_st;
    const float* ratio;
    int64_t r_sb, r_st;
    const int32_t* n_samples;
    const int32_t* pace_q;
    int32_t* amarks;                            // [B][KA]
    int32_t* n_amarks;                          // [B]
    int32_t* smarks;                            // [B][KS]
    int32_t* src;                               // [B][KS]
    int32_t* half;                              // [B][KS]
    int32_t* n_smarks;                          // [B]
    int32_t* n_out;                             // [B]
    int N, N_out, T, hop, KA, KS, unvoiced;
    float sr256;
};

// per[t] and step[t] of frame t of utterance b, in 1 / 256 sample
__device__ __forceinline__ void psola_frame(const MarksArgs& p, int b, int t, int& per, int& step) {
    const float f = p.f0[b * p.f_sb + t * p.f_st];
    if (f > 0.f && f <= 3.4028234663852886e38f) {                           // NaN, inf, 0 and below: unvoiced
        float q = rintf(p.sr256 / f);
        q = fminf(fmaxf(q, (float)(PS_MIN_PERIOD * PS_Q)), (float)(PS_MAX_PERIOD * PS_Q));
        per = (int)q;
        float r = p.ratio[b * p.r_sb + t * p.r_st];
        r = r >= 0.625f ? r : 0.625f;
        r = r <= 2.0f ? r : 2.0f;
        step = max(PS_MIN_PERIOD / 2 * PS_Q, (int)rintf((float)per / r));
    } else {
        per = step = p.unvoiced * PS_Q;
    }
}

// per[t] alone, for a ratio that does not live on the input's frames: step = 0 on a voiced frame (the step is formed at the
// mark, where its ratio is known), unvoiced_period Q otherwise
__device__ __forceinline__ void psola_period(const MarksArgs& p, int b, int t, int& per, int& step) {
    const float f = p.f0[b * p.f_sb + t * p.f_st];
    if (f > 0.f && f <= 3.4028234663852886e38f) {
        float q = rintf(p.sr256 / f);
        q = fminf(fmaxf(q, (float)(PS_MIN_PERIOD * PS_Q)), (float)(PS_MAX_PERIOD * PS_Q));
        per = (int)q;
        step = 0;
    } else {
        per = step = p.unvoiced * PS_Q;
    }
}

__global__ __launch_bounds__(64) void psola_marks_k(MarksArgs p) {
    __shared__ int per_s[PS_LDS_FRAMES], step_s[PS_LDS_FRAMES];
    const int lane = threadIdx.x, b = blockIdx.x;
    const int n = min(max(p.n_samples[b], 1), p.N);
    const int pq = min(max(p.pace_q[b], PS_MIN_PACE_Q), PS_MAX_PACE_Q);
    const int no = (int)min((int64_t)p.N_out, max((int64_t)1, ((int64_t)n << 16) / pq));
    const int last = min(p.T - 1, n / p.hop);                               // the highest frame a position below n 256 maps to
    for (int t = lane; t <= min(last, PS_LDS_FRAMES - 1); t += 64) {
        int per, step;
        psola_frame(p, b, t, per, step);
        per_s[t] = per;
        step_s[t] = step;
    }
    __syncthreads();
    const int h2 = p.hop / 2;
    auto fetch = [&](int t, int& per, int& step) {                          // t <= last
        if (t < PS_LDS_FRAMES) { per = per_s[t]; step = step_s[t]; }
        else psola_frame(p, b, t, per, step);
    };
    int32_t* am = p.amarks + (int64_t)b * p.KA;
    int32_t* sm = p.smarks + (int64_t)b * p.KS;
    int32_t* so = p.src + (int64_t)b * p.KS;
    int32_t* ha = p.half + (int64_t)b * p.KS;

    // analysis marks: a_0 = 0, a_{k+1} = a_k + per[frame(a_k)] while (a_k >> 8) < n
    int K = 0;
    {
        int a = 0, t = 0;
        int64_t edge = p.hop;                                               // (t + 1) hop: frame(a) = t while (a >> 8) + h2 < edge
        while ((a >> 8) < n && K < p.KA) {
            if (lane == 0) am[K] = a;
            ++K;
            while ((a >> 8) + h2 >= edge) { ++t; edge += p.hop; }
            int per, step;
            fetch(min(t, last), per, step);
            a += per;
        }
    }
    // synthesis marks, the analysis marks formed again beside them (a = a_k, an = a_{k+1})
    int J = 0;
    {
        int s = 0, k = 0, a = 0, ta_t = 0, a_t = 0, per, step;
        int64_t ta_edge = p.hop, a_edge = p.hop;
        fetch(0, per, step);                                                // frame(0) = 0
        int an = per;
        while ((s >> 8) < no && J < p.KS) {
            const int ta = (int)(((int64_t)s * pq) >> 16);                  // < n 256
            while (k + 1 < K && abs(an - ta) <= abs(a - ta)) {
                a = an;
                ++k;
                while ((a >> 8) + h2 >= a_edge) { ++a_t; a_edge += p.hop; }
                fetch(min(a_t, last), per, step);
                an = a + per;
            }
            while ((ta >> 8) + h2 >= ta_edge) { ++ta_t; ta_edge += p.hop; }
            int tper, tstep;
            fetch(min(ta_t, last), tper, tstep);
            if (lane == 0) { sm[J] = s; so[J] = k; ha[J] = (an - a + 128) >> 8; }
            ++J;
            s += tstep;
        }
    }
    if (lane == 0) { p.n_amarks[b] = K; p.n_smarks[b] = J; p.n_out[b] = no; }
}

struct WarpArgs {
    MarksArgs m;                                // (pace_q is not used; ratio is [B][RT])
    const int32_t* n_out_in;                    // [B]
    const int32_t* tmap;                        // [B][TM]
    int RT, TM, hop_out, axis;
};

// the ratio as step 1 clamps it (NaN counts as 0.625)
__device__ __forceinline__ float psola_clamp_ratio(float r) {
    r = r >= 0.625f ? r : 0.625f;
    return r <= 2.0f ? r : 2.0f;
}

// (d fr) / den toward zero, exactly, without the 64-bit division (a subroutine of some 150 instructions in every step of a
// serial chain): |d| <= 2^32, 0 <= fr < den <= 2^30, inv = 1.0 / den.  |d fr| < 2^62 and the quotient is below 2^32, so the
// double product is within 2^-19 of the true quotient: truncated it is the quotient or one off, and the remainder says which.
__device__ __forceinline__ int64_t psola_muldiv(int64_t d, int64_t fr, int64_t den, double inv) {
    const int64_t num = d * fr, mag = num < 0 ? -num : num;
    int64_t q = (int64_t)((double)mag * inv);
    const int64_t r = mag - q * den;
    q += r >= den ? 1 : (r < 0 ? -1 : 0);
    return num < 0 ? -q : q;
}

__global__ __launch_bounds__(64) void psola_marks_warp_k(WarpArgs w) {
    // step_s[t]: ratio_axis 0 -- step[t] as in psola_marks_k (psola_frame); ratio_axis 1 -- psola_period's
    __shared__ int per_s[PS_LDS_FRAMES], step_s[PS_LDS_FRAMES], map_s[PS_LDS_FRAMES];
    __shared__ float rat_s[PS_LDS_FRAMES];
    const MarksArgs& p = w.m;
    const int lane = threadIdx.x, b = blockIdx.x;
    const int n = min(max(p.n_samples[b], 1), p.N);
    const int no = min(max(w.n_out_in[b], 1), p.N_out);
    const int last = min(p.T - 1, n / p.hop);
    const int u_last = min(w.TM - 2, (no - 1) / w.hop_out);                 // the highest u a mark below no 256 has
    const int o_last = min(w.RT - 1, no / w.hop_out);                       // and the highest output frame
    const int32_t* tm = w.tmap + (int64_t)b * w.TM;
    const float* rrow = p.ratio + b * p.r_sb;
    auto frame = [&](int t, int& per, int& step) {
        if (w.axis == 1) psola_period(p, b, t, per, step); else psola_frame(p, b, t, per, step);
    };
    for (int t = lane; t <= min(last, PS_LDS_FRAMES - 1); t += 64) {
        int per, step;
        frame(t, per, step);
        per_s[t] = per;
        step_s[t] = step;
    }
    for (int u = lane; u <= min(u_last + 1, PS_LDS_FRAMES - 1); u += 64) map_s[u] = tm[u];
    if (w.axis == 1)
        for (int t = lane; t <= min(o_last, PS_LDS_FRAMES - 1); t += 64) rat_s[t] = psola_clamp_ratio(rrow[t * p.r_st]);
    __syncthreads();
    const int h2 = p.hop / 2;
    auto fetch = [&](int t, int& per, int& step) {                          // t <= last
        if (t < PS_LDS_FRAMES) { per = per_s[t]; step = step_s[t]; }
        else frame(t, per, step);
    };
    auto map_at = [&](int u) { return u < PS_LDS_FRAMES ? map_s[u] : tm[u]; };                        // u <= TM - 1
    auto ratio_at = [&](int t) { return t < PS_LDS_FRAMES ? rat_s[t] : psola_clamp_ratio(rrow[t * p.r_st]); };   // t <= RT - 1
    int32_t* am = p.amarks + (int64_t)b * p.KA;
    int32_t* sm = p.smarks + (int64_t)b * p.KS;
    int32_t* so = p.src + (int64_t)b * p.KS;
    int32_t* ha = p.half + (int64_t)b * p.KS;

    // analysis marks: psola_marks_k's walk
    int K = 0;
    {
        int a = 0, t = 0;
        int64_t edge = p.hop;
        while ((a >> 8) < n && K < p.KA) {
            if (lane == 0) am[K] = a;
            ++K;
            while ((a >> 8) + h2 >= edge) { ++t; edge += p.hop; }
            int per, step;
            fetch(min(t, last), per, step);
            a += per;
        }
    }
    // synthesis marks along the map
    int J = 0;
    {
        const int64_t den = (int64_t)w.hop_out * PS_Q;
        const double inv_den = 1.0 / (double)den;
        const int ho2 = w.hop_out / 2, ta_max = n * PS_Q - 1;
        int s = 0, k = 0, a = 0, ta = 0, ta_t = 0, a_t = 0, per, step;
        int u = 0, o_t = 0;
        int64_t ta_edge = p.hop, a_edge = p.hop, u_edge = w.hop_out, o_edge = w.hop_out, u_base = 0;
        fetch(0, per, step);
        int an = per;
        while ((s >> 8) < no && J < p.KS) {
            while ((s >> 8) >= u_edge) { ++u; u_edge += w.hop_out; u_base += den; }         // u = (s >> 8) / hop_out
            const int uc = min(u, u_last);
            const int64_t m0 = map_at(uc), m1 = map_at(uc + 1);
            const int64_t lin = m0 + psola_muldiv(m1 - m0, (int64_t)s - u_base, den, inv_den);
            ta = (int)min(max(lin, (int64_t)ta), (int64_t)ta_max);                          // ta starts at 0: never below it
            while (k + 1 < K && abs(an - ta) <= abs(a - ta)) {
                a = an;
                ++k;
                while ((a >> 8) + h2 >= a_edge) { ++a_t; a_edge += p.hop; }
                fetch(min(a_t, last), per, step);
                an = a + per;
            }
            while ((ta >> 8) + h2 >= ta_edge) { ++ta_t; ta_edge += p.hop; }
            int tper, tstep;
            fetch(min(ta_t, last), tper, tstep);
            if (w.axis == 1 && tstep == 0) {
                while ((s >> 8) + ho2 >= o_edge) { ++o_t; o_edge += w.hop_out; }            // ((s >> 8) + hop_out / 2) / hop_out
                tstep = max(PS_MIN_PERIOD / 2 * PS_Q, (int)rintf((float)tper / ratio_at(min(o_t, o_last))));
            }
            if (lane == 0) { sm[J] = s; so[J] = k; ha[J] = (an - a + 128) >> 8; }
            ++J;
            s += tstep;
        }
    }
    if (lane == 0) { p.n_amarks[b] = K; p.n_smarks[b] = J; p.n_out[b] = no; }
}

struct MapArgs {
    const int32_t* path;                        // [B][P][2]
    const int32_t* path_len;                    // [B]
    int32_t* tmap;                              // [B][TM]
    int P, TM, hop, w;
};

__global__ __launch_bounds__(PS_MAP_THREADS) void psola_time_map_k(MapArgs p) {
    __shared__ int mid[PS_MAX_PATH];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Pb = min(max(p.path_len[b], 1), p.P);
    const int32_t* cells = p.path + (int64_t)b * p.P * 2;
    const int i_max = (PS_MAX_SAMPLES - 1) / p.hop, j_max = p.P - 1;
    auto jc = [&](int c) { return min(max(cells[2 * c + 1], 0), j_max); };
    auto ic = [&](int c) { return min(max(cells[2 * c], 0), i_max); };
    const int Jb = jc(Pb - 1) + 1;
    for (int j = tid; j < Jb; j += PS_MAP_THREADS) mid[j] = 0;
    __syncthreads();
    for (int c = tid; c < Pb; c += PS_MAP_THREADS) {
        const int j = jc(c);
        if (j < Jb && (c == 0 || jc(c - 1) != j)) mid[j] = ic(c);           // lo_j
    }
    __syncthreads();
    for (int c = tid; c < Pb; c += PS_MAP_THREADS) {
        const int j = jc(c);
        if (j < Jb && (c == Pb - 1 || jc(c + 1) != j)) mid[j] = 128 * p.hop * (mid[j] + ic(c));   // hop i <= 2^22 - 1: below 2^30
    }
    __syncthreads();
    int32_t* row = p.tmap + (int64_t)b * p.TM;
    const int64_t taps = 2 * p.w + 1;
    for (int u = tid; u < p.TM; u += PS_MAP_THREADS) {
        int64_t sum = 0;
        for (int d = -p.w; d <= p.w; ++d) sum += mid[min(max(u + d, 0), Jb - 1)];
        row[u] = (int32_t)(sum / taps);
    }
}

struct SynthArgs {
    const float* audio;
    int64_t sb, sn;
    const int32_t* n_samples;
    const int32_t* amarks;
    const int32_t* smarks;
    const int32_t* src;
    const int32_t* half;
    const int32_t* n_smarks;
    const int32_t* n_out;
    const float* hann;                          // [PS_HANN + 1]
    float* out;                                 // [B][N_out]
    int N, N_out, KA, KS;
};

__global__ __launch_bounds__(PS_TILE) void psola_synth_k(SynthArgs p) {
    __shared__ float H[PS_HANN + 1];
    __shared__ int gc[PS_TILE], gm[PS_TILE], gh[PS_TILE];
    __shared__ float gr[PS_TILE];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int o0 = blockIdx.x * PS_TILE, o = o0 + tid;
    const int n = min(max(p.n_samples[b], 1), p.N);
    const int no = min(max(p.n_out[b], 1), p.N_out);
    const int J = min(max(p.n_smarks[b], 0), p.KS);
    float* row = p.out + (int64_t)b * p.N_out;
    if (o0 >= no) {                             // (uniform: the tile lies behind the utterance)
        if (o < p.N_out) row[o] = 0.f;
        return;
    }
    for (int i = tid; i <= PS_HANN; i += PS_TILE) H[i] = p.hann[i];
    const float* x = p.audio + b * p.sb;
    const int32_t* sm = p.smarks + (int64_t)b * p.KS;
    const int32_t* so = p.src + (int64_t)b * p.KS;
    const int32_t* ha = p.half + (int64_t)b * p.KS;
    const int32_t* am = p.amarks + (int64_t)b * p.KA;
    int lo = 0, hi = J;                         // the first grain with c_j + 1024 > o0 (uniform)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (((sm[mid] + 128) >> 8) + PS_MAX_PERIOD > o0) hi = mid; else lo = mid + 1;
    }
    float y = 0.f, ws = 0.f;
    for (int j0 = lo; j0 < J; j0 += PS_TILE) {  // (uniform trip counts)
        __syncthreads();                        // H is written; the previous grains have been read
        const int j = j0 + tid;
        if (j < J) {
            const int h = min(max(ha[j], 1), PS_MAX_PERIOD);
            gc[tid] = (sm[j] + 128) >> 8;
            gm[tid] = (am[min(max(so[j], 0), p.KA - 1)] + 128) >> 8;
            gh[tid] = h;
            gr[tid] = 1.f / (float)h;
        }
        __syncthreads();
        const int cnt = min(PS_TILE, J - j0);
        bool behind = false;
        for (int g = 0; g < cnt; ++g) {
            const int c = gc[g];
            if (c - PS_MAX_PERIOD >= o0 + PS_TILE) { behind = true; break; }   // (uniform) no later grain reaches the tile
            const int h = gh[g], d = o - c, ad = abs(d);
            if (ad < h) {
                const int num = ad * PS_HANN;
                int q = (int)((float)num * gr[g]);
                q += ((q + 1) * h <= num);
                const float w = H[q];
                const int64_t i = (int64_t)gm[g] + d;
                const float xv = (i >= 0 && i < n) ? x[i * p.sn] : 0.f;
                ws = ws + w;
                y = y + w * xv;
            }
        }
        if (behind) break;
    }
    if (o < p.N_out) row[o] = (o < no && ws >= 0.0009765625f) ? y / ws : 0.f;
}

}  // namespace

extern "C" int ft_psola_marks(const float* f0, int64_t f0_stride_b, int64_t f0_stride_t, const float* ratio, int64_t ratio_stride_b,
                              int64_t ratio_stride_t, const int32_t* n_samples, const int32_t* pace_q, int32_t* analysis,
                              int32_t* n_analysis, int32_t* synthesis, int32_t* source, int32_t* half, int32_t* n_synthesis,
                              int32_t* n_out, int B, int N, int N_out, int T, int hop, int KA, int KS, float sr256,
                              int unvoiced_period, void* stream) {
    FT_CHECK_ARG(f0 && ratio && n_samples && pace_q && analysis && n_analysis && synthesis && source && half && n_synthesis && n_out);
    FT_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1 && N_out >= 1 && T >= 1 && hop >= 1);
    FT_CHECK_ARG(f0_stride_b >= 0 && f0_stride_t >= 0 && ratio_stride_b >= 0 && ratio_stride_t >= 0);
    FT_CHECK_ARG(sr256 > 0.f && sr256 <= 3.4028234663852886e38f);
    if (N > PS_MAX_SAMPLES || N_out > PS_MAX_SAMPLES)
        return ft_fail(FT_EUNSUPPORTED, "%s: N %d, N_out %d: an utterance holds at most %d samples", __func__, N, N_out, PS_MAX_SAMPLES);
    if (unvoiced_period < PS_MIN_PERIOD || unvoiced_period > PS_MAX_PERIOD)
        return ft_fail(FT_EUNSUPPORTED, "%s: unvoiced_period %d: a period holds %d .. %d samples", __func__, unvoiced_period,
                       PS_MIN_PERIOD, PS_MAX_PERIOD);
    FT_CHECK_ARG(T >= N / hop + 1);
    FT_CHECK_ARG(KA >= cdiv(N, PS_MIN_PERIOD) && KS >= cdiv(N_out, PS_MIN_PERIOD / 2));
    MarksArgs p{};
    p.f0 = f0; p.f_sb = f0_stride_b; p.f_st = f0_stride_t;
    p.ratio = ratio; p.r_sb = ratio_stride_b; p.r_st = ratio_stride_t;
    p.n_samples = n_samples; p.pace_q = pace_q;
    p.amarks = analysis; p.n_amarks = n_analysis; p.smarks = synthesis; p.src = source; p.half = half; p.n_smarks = n_synthesis;
    p.n_out = n_out;
    p.N = N; p.N_out = N_out; p.T = T; p.hop = hop; p.KA = KA; p.KS = KS; p.unvoiced = unvoiced_period; p.sr256 = sr256;
    hipLaunchKernelGGL(psola_marks_k, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_psola_marks_warp(const float* f0, int64_t f0_stride_b, int64_t f0_stride_t, const float* ratio, int64_t ratio_stride_b,
                                   int64_t ratio_stride_t, const int32_t* n_samples, const int32_t* n_out_in, const int32_t* tmap,
                                   int32_t* analysis, int32_t* n_analysis, int32_t* synthesis, int32_t* source, int32_t* half,
                                   int32_t* n_synthesis, int32_t* n_out, int B, int N, int N_out, int T, int RT, int TM, int hop,
                                   int hop_out, int ratio_axis, int KA, int KS, float sr256, int unvoiced_period, void* stream) {
    FT_CHECK_ARG(f0 && ratio && n_samples && n_out_in && tmap && analysis && n_analysis && synthesis && source && half && n_synthesis &&
                 n_out);
    FT_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1 && N_out >= 1 && T >= 1 && RT >= 1 && TM >= 1 && hop >= 1);
    FT_CHECK_ARG(hop_out >= 1 && hop_out <= PS_MAX_SAMPLES);
    FT_CHECK_ARG(ratio_axis == 0 || ratio_axis == 1);
    FT_CHECK_ARG(f0_stride_b >= 0 && f0_stride_t >= 0 && ratio_stride_b >= 0 && ratio_stride_t >= 0);
    FT_CHECK_ARG(sr256 > 0.f && sr256 <= 3.4028234663852886e38f);
    if (N > PS_MAX_SAMPLES || N_out > PS_MAX_SAMPLES)
        return ft_fail(FT_EUNSUPPORTED, "%s: N %d, N_out %d: an utterance holds at most %d samples", __func__, N, N_out, PS_MAX_SAMPLES);
    if (unvoiced_period < PS_MIN_PERIOD || unvoiced_period > PS_MAX_PERIOD)
        return ft_fail(FT_EUNSUPPORTED, "%s: unvoiced_period %d: a period holds %d .. %d samples", __func__, unvoiced_period,
                       PS_MIN_PERIOD, PS_MAX_PERIOD);
    FT_CHECK_ARG(T >= N / hop + 1);
    FT_CHECK_ARG(TM >= N_out / hop_out + 2);
    FT_CHECK_ARG(RT >= (ratio_axis == 0 ? N / hop : N_out / hop_out) + 1);
    FT_CHECK_ARG(KA >= cdiv(N, PS_MIN_PERIOD) && KS >= cdiv(N_out, PS_MIN_PERIOD / 2));
    WarpArgs w{};
    MarksArgs& p = w.m;
    p.f0 = f0; p.f_sb = f0_stride_b; p.f_st = f0_stride_t;
    p.ratio = ratio; p.r_sb = ratio_stride_b; p.r_st = ratio_stride_t;
    p.n_samples = n_samples; p.pace_q = nullptr;
    p.amarks = analysis; p.n_amarks = n_analysis; p.smarks = synthesis; p.src = source; p.half = half; p.n_smarks = n_synthesis;
    p.n_out = n_out;
    p.N = N; p.N_out = N_out; p.T = T; p.hop = hop; p.KA = KA; p.KS = KS; p.unvoiced = unvoiced_period; p.sr256 = sr256;
    w.n_out_in = n_out_in; w.tmap = tmap; w.RT = RT; w.TM = TM; w.hop_out = hop_out; w.axis = ratio_axis;
    hipLaunchKernelGGL(psola_marks_warp_k, dim3(B), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), w);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_psola_time_map(const int32_t* path, const int32_t* path_len, int32_t* tmap, int B, int P, int TM, int hop, int w,
                                 void* stream) {
    FT_CHECK_ARG(path && path_len && tmap);
    FT_CHECK_ARG(B >= 1 && B <= 65535 && P >= 1 && TM >= 1 && hop >= 1 && hop <= PS_MAX_SAMPLES);
    FT_CHECK_ARG(w >= 0 && w <= PS_MAX_SMOOTH);
    if (P > PS_MAX_PATH)
        return ft_fail(FT_EUNSUPPORTED, "%s: P %d: a path holds at most %d cells", __func__, P, PS_MAX_PATH);
    MapArgs p{};
    p.path = path; p.path_len = path_len; p.tmap = tmap; p.P = P; p.TM = TM; p.hop = hop; p.w = w;
    hipLaunchKernelGGL(psola_time_map_k, dim3(B), dim3(PS_MAP_THREADS), 0, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int ft_psola_synth(const float* audio, int64_t stride_b, int64_t stride_n, const int32_t* n_samples, const int32_t* analysis,
                              const int32_t* synthesis, const int32_t* source, const int32_t* half, const int32_t* n_synthesis,
                              const int32_t* n_out, const float* hann, float* out, int B, int N, int N_out, int KA, int KS,
                              void* stream) {
    FT_CHECK_ARG(audio && n_samples && analysis && synthesis && source && half && n_synthesis && n_out && hann && out);
    FT_CHECK_ARG(B >= 1 && B <= 65535 && N >= 1 && N_out >= 1 && KA >= 1 && KS >= 1);
    FT_CHECK_ARG(stride_b >= 0 && stride_n >= 0);
    if (N > PS_MAX_SAMPLES || N_out > PS_MAX_SAMPLES)
        return ft_fail(FT_EUNSUPPORTED, "%s: N %d, N_out %d: an utterance holds at most %d samples", __func__, N, N_out, PS_MAX_SAMPLES);
    SynthArgs p{};
    p.audio = audio; p.sb = stride_b; p.sn = stride_n;
    p.n_samples = n_samples; p.amarks = analysis; p.smarks = synthesis; p.src = source; p.half = half; p.n_smarks = n_synthesis;
    p.n_out = n_out; p.hann = hann; p.out = out;
    p.N = N; p.N_out = N_out; p.KA = KA; p.KS = KS;
    hipLaunchKernelGGL(psola_synth_k, dim3(cdiv(N_out, PS_TILE), B), dim3(PS_TILE), 0, reinterpret_cast<hipStream_t>(stream), p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
