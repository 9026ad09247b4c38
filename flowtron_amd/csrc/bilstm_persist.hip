// Persistent bidirectional LSTM for the text encoder (flowtron.py:488, :505-512: nn.LSTM(512, 256, bidirectional=True)):
// ONE launch per pass for both directions and all time steps, instead of one launch per step (lstm.hip lstm_*_pair, 4.4 / 4.9 us
// per step at the launch floor).
//
// H = 256 is small enough for a much simpler organisation than lstm_persist.hip.
//   group      = (XCD x, direction d): batch rows [4x, 4x + 4) of that direction, for the whole sequence; formed at run time from
//                the workgroups' XCC ids (census, as in lstm_persist.hip), hand-off through that XCD's own L2; 16 workgroups per
//                group in both passes, so all 32 CUs of an XCD work;
//   forward    every WAVE is an independent agent that owns 4 hidden units (one 16-column MFMA tile = 4 units x 4 gates) with
//                the whole K = 256: 8 MFMAs per step, no K split, hence no LDS reduction and no barrier -- the four gates of a
//                unit are gathered into one lane with three DPP row shifts.  64 waves per group;
//   backward   a WORKGROUP owns 16 hidden units (one column tile of W_hh^T, K = 4H = 1024) and splits K over its four waves: wave g
//                polls and multiplies the dgates of gate g (a quarter of the hand-off bytes, 8 of the 32 MFMAs), the partials are
//                summed through LDS in a fixed order behind one barrier per step (see bilstm_bwd_body);
//   hand-off   h_t / dgates_s as 8-byte {epoch, 16-bit pair} granules in the packed layout of lstm_persist.hip (one 16-byte load
//                per lane fetches four k-chunks of the group's four rows; DPP row shifts move them into the MFMA row positions),
//                plain stores, nt loads, two parity buffers, bounded spins with a status word;
//   HBM rows   (gx; saved gates, cell, dy) are fetched one step ahead into registers right after a step's poll has completed, so
//                that they have a whole step of slack before the next poll queues up behind them (vmcnt retires in order).
// The time index is uniform per group: forward direction t = s, reverse direction t = tg - 1 - s (tg = the longest of the group's
// four rows), a row takes part while t < len -- a row of the reverse direction simply starts late, with zero state.
// y / dgx rows of padded frames are zeroed by the launcher (memset), the kernels write valid frames only.
// Not bit-identical to the launch-per-step pair kernels (those split K over waves); same operand rounding, fp32 accumulation.
#include "common.h"
#include "lstm_images.h"

namespace {

typedef __attribute__((address_space(1))) unsigned long long gu64;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

constexpr int BH = 256;                  // hidden size this file is built for
constexpr int NWG = 256;                 // workgroups launched: one per CU, 32 per XCD
constexpr int GRAN_F = 4 * BH / 2;       // granules of one forward state vector (4 rows x 256): 512
constexpr int GRAN_B = 4 * 4 * BH / 2;   // granules of one dgates vector (4 rows x 1024): 2048

template <int N>
__device__ __forceinline__ unsigned row_shl(unsigned v) {          // lane l <- lane l + N of the same 16-lane row
    if constexpr (N == 0) return v;
    else return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x100 + N, 0xf, 0xf, true);
}
template <int N>
__device__ __forceinline__ float row_shl_f(float v) { return __uint_as_float(row_shl<N>(__float_as_uint(v))); }
template <int S>
__device__ __forceinline__ u32x4 shl4(u32x4 v) {
    return (u32x4){row_shl<S>(v[0]), row_shl<S>(v[1]), row_shl<S>(v[2]), row_shl<S>(v[3])};
}
// member j (0..3) of a load group = k-chunk 4 lg + j: its four rows moved to lanes li < 4 of every 16-lane row
__device__ __forceinline__ u32x4 member(u32x4 v, int j) {
    switch (j) {
        case 0: return v;
        case 1: return shl4<4>(v);
        case 2: return shl4<8>(v);
        default: return shl4<12>(v);
    }
}
// granule index of the operand pair (k, k + 1), k even, of row b (0..3): chunk c = k / 32 -> load group lg = c / 4, member j = c % 4,
// lane = kg 16 + j 4 + b; a lane's two 16-byte loads (halves) of a load group hold its eight k-values {v, tag, v, tag} x 2
__device__ __forceinline__ int gran_index(int b, int k) {
    const int c = k >> 5, kg = (k >> 3) & 3, e = k & 7;
    const int lg = c >> 2, j = c & 3, lane = kg * 16 + j * 4 + b;
    return ((((lg * 2 + (e >> 2)) * 64 + lane)) << 1) + ((e >> 1) & 1);
}

struct BiFwdP {
    const float* gx[2]; const int* lens; float* y; long ldy; float* gates[2]; float* cell[2];
    const unsigned short* wfrag[2];      // make_wfrag_fwd images of W_hh (forward, reverse)
    unsigned long long* gran;            // [2 parity][8 xcd][2 dir][GRAN_F]
    int* status; unsigned* census; int T, B; long timeout_ticks;
};
struct BiBwdP {
    const float* dy; long ldy; const int* lens; const float* gates[2]; const float* cell[2]; float* dgx[2];
    const unsigned short* wTfrag[2];     // make_wfrag_bwd images
    unsigned long long* gran;            // [2 parity][8 xcd][2 dir][GRAN_B]
    int* status; unsigned* census; int T, B; long timeout_ticks; long* prof;
};

// XCD census: group = this workgroup's XCC id, slot = arrival order inside that XCD (lstm_persist.hip)
__device__ __forceinline__ bool join(unsigned* census, int* status, int tid, int& xcd, int& q) {
    __shared__ int slot[2];
    if (tid == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
        slot[0] = (int)(xcc & 7u);
        slot[1] = (int)__hip_atomic_fetch_add(census + (xcc & 7u), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    xcd = __builtin_amdgcn_readfirstlane(slot[0]);
    q = __builtin_amdgcn_readfirstlane(slot[1]);
    if (q >= 32) {
        if (tid == 0) atomicExch(status, 2);
        return false;
    }
    return true;
}

// poll NL load groups (two 16-byte loads each) of this group's vector, from the wave-uniform byte offset `soff` on, until every tag
// shows `epoch`; false = timed out
template <int NL>
__device__ __forceinline__ bool poll(u32x4 (&ld)[NL][2], __amdgpu_buffer_rsrc_t rs, int voff, unsigned epoch, long t_start,
                                     long timeout_ticks, int* status, int soff = 0) {
    auto issue = [&](int g) {
#pragma unroll
        for (int h = 0; h < 2; ++h) ld[g][h] = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff + (g * 2 + h) * 1024, 2);   // nt
    };
#pragma unroll
    for (int g = 0; g < NL; ++g) issue(g);
    unsigned ready = 0;
    for (unsigned spins = 0;; ++spins) {
#pragma unroll
        for (int g = 0; g < NL; ++g) {
            if (!((ready >> g) & 1u)) {
                const bool ok = (ld[g][0][1] == epoch) & (ld[g][0][3] == epoch) & (ld[g][1][1] == epoch) & (ld[g][1][3] == epoch);
                if (__all(ok)) ready |= 1u << g;
            }
        }
        if (ready == (1u << NL) - 1u) return true;
        if ((spins & 15) == 15) {
            if (wall_clock64() - t_start > timeout_ticks || __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)
                return false;
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int g = 0; g < NL; ++g) {
            if (!((ready >> g) & 1u)) issue(g);
        }
    }
}

__global__ __launch_bounds__(256) void bilstm_persist_fwd_k(BiFwdP p) {
    extern __shared__ float occupancy_pad[];             // sized by the launcher so that one workgroup fills a CU
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, kg = lane >> 4;
    int xcd, q;
    if (!join(p.census, p.status, tid, xcd, q)) return;
    const int dir = q >> 4, m = q & 15;                  // 16 workgroups per (XCD, direction)
    const int B = p.B, T = p.T, b0 = xcd * 4;
    const int jb = m * 4 + wave;                         // this wave's tile: units jb*4 .. jb*4 + 3
    int len[4], tg = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        len[r] = (b0 + r < B) ? min(p.lens[b0 + r], T) : 0;
        tg = len[r] > tg ? len[r] : tg;
    }
    bf16x8 w[8];
    {
        const bf16x8* wf = reinterpret_cast<const bf16x8*>(p.wfrag[dir]);
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c] = wf[((size_t)jb * 8 + c) * 64 + lane];
    }
    // The MFMA leaves row r of the tile in register r of lanes 0..15 (lane li <-> gate li / 4, unit li % 4).  One shuffle per row
    // hands row r to the 16-lane group kg = r, so that every lane group finishes ONE row: one gx load, one cell update and one
    // store of each kind per lane and step instead of four (the vector-memory instruction count is what a step costs here).
    const int mylen = kg == 0 ? len[0] : kg == 1 ? len[1] : kg == 2 ? len[2] : len[3];
    const int gcol = (li >> 2) * BH + jb * 4 + (li & 3);                 // column of gx of this lane: gate li / 4, unit li % 4
    const float* gxp = p.gx[dir];
    auto load_gx = [&](int t) { return (t >= 0 && t < mylen) ? gxp[((size_t)t * B + b0 + kg) * 4 * BH + gcol] : 0.f; };
    unsigned long long* gbase = p.gran + ((size_t)xcd * 2 + dir) * GRAN_F;          // + parity * 16 * GRAN_F
    __amdgpu_buffer_rsrc_t rs[2];
#pragma unroll
    for (int par = 0; par < 2; ++par) rs[par] = __builtin_amdgcn_make_buffer_rsrc(gbase + (size_t)par * 16 * GRAN_F, 0, GRAN_F * 8, 0x00020000);
    const int voff = lane * 16;
    const long t_start = wall_clock64();
    float c_state = 0.f, h_state = 0.f;
    float gxv = load_gx(dir ? tg - 1 : 0), gxn;
    const int u = jb * 4 + (li & 3);                     // (lanes li < 4 of every group own unit li)
    bool dead = false;
    for (int s = 0; s < tg; ++s) {
        const int t = dir ? tg - 1 - s : s;
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
        u32x4 ld[2][2];
        if (s > 0) {
            if (!poll<2>(ld, rs[(s - 1) & 1], voff, (unsigned)s, t_start, p.timeout_ticks, p.status)) { dead = true; break; }
        }
        gxn = load_gx(dir ? t - 1 : t + 1);              // next step's row: a whole step ahead of the poll that queues behind it
        if (s > 0) {
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const u32x4 pay = (u32x4){ld[c >> 2][0][0], ld[c >> 2][0][2], ld[c >> 2][1][0], ld[c >> 2][1][2]};
                acc = mfma16(__builtin_bit_cast(bf16x8, member(pay, c & 3)), w[c], acc);
            }
        }
        const float x1 = __shfl(acc[1], li, 64), x2 = __shfl(acc[2], li, 64), x3 = __shfl(acc[3], li, 64);
        const float pre_i = (kg == 0 ? acc[0] : kg == 1 ? x1 : kg == 2 ? x2 : x3) + gxv;     // (row kg, gate li / 4, unit li % 4)
        float pre[4] = {pre_i, row_shl_f<4>(pre_i), row_shl_f<8>(pre_i), row_shl_f<12>(pre_i)};   // lanes li < 4: the four gates of unit li
        float ig, fg, gg, og, c_new, h_new;
        lstm_cell<true>(pre, c_state, ig, fg, gg, og, c_new, h_new);
        const bool active = t < mylen;
        if (active) { c_state = c_new; h_state = h_new; }
        const float hn = row_shl_f<1>(h_state);          // the odd unit of the pair
        if (li < 4) {
            if ((li & 1) == 0) {
                // publish h_t: one {epoch, pair} granule (a row that does not take part publishes its frozen / zero state)
                const unsigned long long gran = ((unsigned long long)(unsigned)(s + 1) << 32) | pack_op16x2(h_state, hn);
                unsigned long long* dst = gbase + (size_t)(s & 1) * 16 * GRAN_F + gran_index(kg, u);
                __hip_atomic_store((gu64*)dst, gran, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            if (active) {
                const size_t row = (size_t)t * B + b0 + kg;
                p.y[row * p.ldy + dir * BH + u] = h_state;
                float* gp = p.gates[dir] + row * 4 * BH + u;
                gp[0] = ig; gp[BH] = fg; gp[2 * BH] = gg; gp[3 * BH] = og;
                p.cell[dir][row * BH + u] = c_state;
            }
        }
        gxv = gxn;
    }
    if (dead && lane == 0) atomicExch(p.status, 1);
}

// Backward step, K split inside the workgroup.  A workgroup owns one column tile of W_hh^T (16 hidden units) of its group, its four
// waves the four k-quarters of the sum over k = gate * 256 + unit -- wave g polls and multiplies the dgates of gate g only: two load
// groups (4 KB of granules), 8 weight fragments, 8 MFMAs in two independent chains.  The four 4 x 16 fp32 partials meet in LDS
// (`part`, two parity buffers) behind ONE barrier per step and are summed in the fixed order 0, 1, 2, 3 by wave 0, which finishes
// the 64 (row, unit) elements: row loads, cell backward, four granule and four dgx stores per lane.  Waves 1..3 carry nothing but
// their poll in the vector-memory queue.  (All four waves finishing redundantly and each publishing one gate -- one store of each
// kind per lane behind the next poll -- measured 5 us per launch SLOWER at T 157: profiles/bilstm_bwd_split_variants.log.)
//
// Parity buffers and the one barrier: a wave writes part[s & 1] again at step s + 2, which it reaches only through the barrier of step
// s + 1; wave 0 arrives there after its reads of step s have returned (they feed the cell backward in front of it).
//
// Leaving: a wave whose poll gives up (time-out, or another workgroup's status) does NOT leave on its own.  It raises quit[s & 1]
// and arrives at the step's barrier like everybody else, and the other waves read that flag BEHIND the barrier: the decision is
// the same for the whole workgroup, nobody is left waiting at a barrier.  The flag has the partials' parity for the partials'
// reason: a wave that is already in step s + 1 raises quit[(s + 1) & 1], which a slower wave still reading the flag of step s does
// not look at, and it cannot reach step s + 2 before that wave has read.  A raised flag is never lowered.
// PROF: stage stamps (100 MHz wall clock) of workgroup (XCD 0, slot 0): prof[(s * 4 + wave) * 6 + {top, polled, partial written,
// reduced, cell done, published}], s < 1024; waves 1..3 stamp the first four.
template <bool PROF>
__device__ __forceinline__ void bilstm_bwd_body(const BiBwdP& p) {
    __shared__ f32x4 part[2][4][16];                     // [parity][k-quarter][unit]: rows 0..3 of the quarter's partial of dh_rec
    __shared__ int quit[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 15, kg = lane >> 4;
    if (tid < 2) quit[tid] = 0;                          // (join's barrier stands between this and the first read)
    int xcd, q;
    if (!join(p.census, p.status, tid, xcd, q)) return;
    const int dir = q >> 4, jt = q & 15;                 // 16 workgroups per (XCD, direction); column tile jt: units jt*16 .. jt*16 + 15
    const int B = p.B, T = p.T, b0 = xcd * 4;
    const int u = jt * 16 + li;
    int len[4], tg = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        len[r] = (b0 + r < B) ? min(p.lens[b0 + r], T) : 0;
        tg = len[r] > tg ? len[r] : tg;
    }
    tg = __builtin_amdgcn_readfirstlane(tg);
    bf16x8 w[8];                                         // k-chunks 8 wave .. 8 wave + 7 of the tile's 32
    {
        const bf16x8* wf = reinterpret_cast<const bf16x8*>(p.wTfrag[dir]);
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c] = wf[((size_t)jt * 32 + wave * 8 + c) * 64 + lane];
    }
    // ONE descriptor over both parity buffers of the group, built from scalars; parity and k-quarter select a scalar byte offset
    unsigned long long* gbase = p.gran + ((size_t)xcd * 2 + dir) * GRAN_B;
    constexpr int PAROFF = 16 * GRAN_B * 8;              // bytes between a group's two parity buffers
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(gbase, 0, PAROFF + GRAN_B * 8, 0x00020000);
    const int voff = lane * 16;
    const int soff_w = wave * 4096;                      // load groups 2 wave, 2 wave + 1
    const long t_start = wall_clock64();
    // wave 0: lane (kg, li) finishes element (row kg, unit u) of the tile
    const bool fin = wave == 0;
    const int mylen = kg == 0 ? len[0] : kg == 1 ? len[1] : kg == 2 ? len[2] : len[3];
    const float* gp = p.gates[dir];
    const float* cp = p.cell[dir];
    struct Rows { float g[4]; float dy; float cprev; };
    // saved gates i f g o, dy, and the cell of the recurrence's previous step.  The loads are unconditional, from clamped (always
    // valid) addresses -- a load under a lane mask comes with a default value in its register, and the copies the compiler makes of
    // those wait for loads that were only just issued.  What a row reads outside [0, len) is masked where it is used (see step).
    const int brow = min(b0 + kg, B - 1);
    auto load_rows = [&](int t, Rows& v) {
        const int tp = dir ? t + 1 : t - 1;              // the recurrence's previous step in time
        const size_t row = (size_t)min(max(t, 0), T - 1) * B + brow;
#pragma unroll
        for (int g = 0; g < 4; ++g) v.g[g] = gp[row * 4 * BH + g * BH + u];
        v.dy = p.dy[row * p.ldy + dir * BH + u];
        v.cprev = cp[((size_t)min(max(tp, 0), T - 1) * B + brow) * BH + u];
    };
    const bool prof = PROF && p.prof != nullptr && xcd == 0 && q == 0 && lane == 0;
    // backward walks the recurrence the other way round: forward direction t = tg-1 .. 0, reverse direction t = 0 .. tg-1.
    // The rows of step s + 1 are in flight while step s runs.  They live in two register sets that swap roles from step to step (the
    // loop below is written out for two steps): a copy from one set to the other would have to wait for the loads it copies.
    Rows ra, rb;
    const int t0 = dir ? 0 : tg - 1;
    float c_t = 0.f, dc_carry = 0.f;
    if (fin) {
        load_rows(t0, ra);
        if (t0 >= 0 && t0 < mylen) c_t = cp[((size_t)t0 * B + b0 + kg) * BH + u];
    }
    bool dead = false;
    auto stamp = [&](int s, const long (&st)[6]) {
        if constexpr (PROF) {
            if (prof && s < 1024) {
#pragma unroll
                for (int i = 0; i < 6; ++i) p.prof[((size_t)s * 4 + wave) * 6 + i] = st[i];
            }
        }
    };
    auto step = [&](int s, Rows& cur, Rows& nxt) __attribute__((always_inline)) -> bool {      // false: the workgroup leaves
        const int t = dir ? s : tg - 1 - s;
        long st[6] = {0, 0, 0, 0, 0, 0};
        if (prof) st[0] = wall_clock64();
        float dh_rec = 0.f;
        if (s > 0) {
            const int par = s & 1;
            u32x4 ld[2][2];
            if (!poll<2>(ld, rs, voff, (unsigned)s, t_start, p.timeout_ticks, p.status, soff_w + (par ^ 1) * PAROFF)) {
                dead = true;
                quit[par] = 1;
                __syncthreads();                         // the step's barrier, on this path: the others read the flag behind theirs
                return false;
            }
            // Every poll load has returned: its tags were just compared, and vmcnt retires in order, so nothing at all is in flight.
            // Said in a form the compiler's wait-count pass sees -- the spin loop's exit shares a block with its back edge, which
            // re-issues loads, and without this the pass waits for the row loads below wherever a register of the poll is reused: in
            // front of the MFMAs and in the cell phase.  (The time-out path above stays apart for the same reason.)
            __builtin_amdgcn_s_waitcnt(0x0F70);
            if (prof) st[1] = wall_clock64();
            if (fin && s + 1 < tg) load_rows(dir ? t + 1 : t - 1, nxt);   // a whole step ahead of the poll that queues behind it
            f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const u32x4 pay = (u32x4){ld[c >> 2][0][0], ld[c >> 2][0][2], ld[c >> 2][1][0], ld[c >> 2][1][2]};
                acc[c & 1] = mfma16(__builtin_bit_cast(bf16x8, member(pay, c & 3)), w[c], acc[c & 1]);
            }
            if (kg == 0) part[par][wave][li] = acc[0] + acc[1];      // rows 0..3 of column li sit in lanes 0..15
            if (prof) st[2] = wall_clock64();
            __syncthreads();
            if (quit[par]) return false;                 // the same answer in all four waves (see above)
            if (fin) {
                const float* pp = reinterpret_cast<const float*>(&part[par][0][li]) + kg;
                dh_rec = ((pp[0] + pp[64]) + pp[128]) + pp[192];     // k-quarters 0, 1, 2, 3 of (row kg, unit u)
            }
        } else if (fin && tg > 1) {
            load_rows(dir ? t + 1 : t - 1, nxt);
        }
        if (prof) st[3] = wall_clock64();
        if (!fin) {
            stamp(s, st);
            return true;
        }
        // the masks of the unconditional row loads: an inactive row's gates and dy only reach values that are dropped right here;
        // the cell of the recurrence's previous step is zero where that step does not exist (also for a row that only joins at the
        // walk's NEXT step: this value becomes its c_t there)
        const int tp = dir ? t + 1 : t - 1;
        const float c_prev = (tp >= 0 && tp < mylen) ? cur.cprev : 0.f;
        float da[4], carry;
        lstm_cell_bwd<true>(dh_rec + cur.dy, dc_carry, cur.g[0], cur.g[1], cur.g[2], cur.g[3], c_t, c_prev, da, carry);
        const bool active = t < mylen;
        if (active) {
            dc_carry = carry;
        } else {
#pragma unroll
            for (int g = 0; g < 4; ++g) da[g] = 0.f;     // (a row that does not take part publishes zeros)
        }
        if (prof) st[4] = wall_clock64();
        // publish dgates_s: k = gate * H + unit, one granule per unit pair (even lanes)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float nb = row_shl_f<1>(da[g]);
            if ((li & 1) == 0) {
                const unsigned long long gran = ((unsigned long long)(unsigned)(s + 1) << 32) | pack_op16x2(da[g], nb);
                unsigned long long* dst = gbase + (size_t)(s & 1) * 16 * GRAN_B + gran_index(kg, g * BH + u);
                __hip_atomic_store((gu64*)dst, gran, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
        if (active) {
            float* dg = p.dgx[dir] + ((size_t)t * B + b0 + kg) * 4 * BH + u;
            dg[0] = da[0]; dg[BH] = da[1]; dg[2 * BH] = da[2]; dg[3 * BH] = da[3];
        }
        c_t = c_prev;                                    // the cell of the step the walk visits next
        if (prof) st[5] = wall_clock64();
        stamp(s, st);
        return true;
    };
    if (tg > 0) {
        step(0, ra, rb);
        for (int s = 1; s < tg; s += 2) {
            if (!step(s, rb, ra)) break;
            if (s + 1 >= tg) break;
            if (!step(s + 1, ra, rb)) break;
        }
    }
    if (dead && lane == 0) atomicExch(p.status, 1);
}

__global__ __launch_bounds__(256) void bilstm_persist_bwd_k(BiBwdP p) {
    extern __shared__ float occupancy_pad[];
    bilstm_bwd_body<false>(p);
}
__global__ __launch_bounds__(256) void bilstm_persist_bwd_prof_k(BiBwdP p) {
    extern __shared__ float occupancy_pad[];
    bilstm_bwd_body<true>(p);
}

}  // namespace

static inline size_t al256b(size_t v) { return (v + 255) & ~size_t(255); }
constexpr size_t BI_WFRAG = (size_t)4 * BH * BH * 2;               // one direction's fragment image
constexpr size_t BI_GRAN = (size_t)2 * 16 * GRAN_B * 8;            // the larger (backward) hand-off region
constexpr size_t BI_LDS = 96 * 1024;                               // one workgroup per CU: the census expects 32 per XCD
constexpr size_t BI_LDS_STATIC = 2 * 4 * 16 * 16 + 2 * 4 + 2 * 4;  // backward: part, quit; join: slot
static_assert(BI_LDS + BI_LDS_STATIC <= 160 * 1024 && 2 * BI_LDS > 160 * 1024, "exactly one workgroup fits a CU's 160 KB of LDS");

#if FT_OPFMT == 0
extern "C" int ft_lstm_persist_supported(int B, int H);
extern "C" int ft_bilstm_persist_supported(int B, int H) {
    if (H != BH || B < 1 || B > 32) return 0;
    return ft_lstm_persist_supported(B, 1024);                     // the same 256-CU device test
}
extern "C" size_t ft_bilstm_persist_workspace_bytes(int B, int H) {
    (void)B; (void)H;
    return 2 * al256b(BI_WFRAG) + al256b(BI_GRAN) + 256;
}
long* ftint_bilstm_prof = nullptr;                   // shared with the fp16 build of this file
extern "C" int ft_bilstm_persist_debug_prof(void* dev_buf) { ftint_bilstm_prof = reinterpret_cast<long*>(dev_buf); return FT_OK; }
#else
extern "C" int ft_bilstm_persist_supported(int B, int H);
extern long* ftint_bilstm_prof;
#endif

extern "C" int FT_OPNAME(ft_bilstm_persist_fwd)(const float* gx_f, const float* gx_r, const float* w_hh_f, const float* w_hh_r,
                                             const int32_t* lens, float* y, int64_t ldy, float* gates_f, float* gates_r,
                                             float* cell_f, float* cell_r, void* work, int32_t* status, int T, int B, int H,
                                             void* stream) {
    FT_CHECK_ARG(gx_f && gx_r && w_hh_f && w_hh_r && lens && y && gates_f && gates_r && cell_f && cell_r && work && status);
    FT_CHECK_ARG(T >= 0 && ldy >= 2 * (int64_t)H && reinterpret_cast<uintptr_t>(work) % 256 == 0);
    if (!ft_bilstm_persist_supported(B, H))
        return ft_fail(FT_EUNSUPPORTED, "ft_bilstm_persist_fwd: needs H == 256, B <= 32 and a 256-CU device (H=%d B=%d)", H, B);
    if (T == 0) return FT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(work);
    unsigned short* wf[2] = {reinterpret_cast<unsigned short*>(base), reinterpret_cast<unsigned short*>(base + al256b(BI_WFRAG))};
    unsigned long long* gran = reinterpret_cast<unsigned long long*>(base + 2 * al256b(BI_WFRAG));
    unsigned* census = reinterpret_cast<unsigned*>(base + 2 * al256b(BI_WFRAG) + al256b(BI_GRAN));
    FT_CHECK_HIP(hipMemset2DAsync(y, (size_t)ldy * 4, 0, (size_t)2 * H * 4, (size_t)T * B, st));   // padded frames: zeros
    // tags 0: no epoch matches (epochs start at 1); preset, with the census counters, by the fragment kernel (WfragAux): ONE launch
    // for both directions' images, in front of every recurrence launch
    static_assert(((size_t)2 * 16 * GRAN_F * 8) % 16 == 0, "granule buffer in 16-byte pieces");
    const WfragAux aux{reinterpret_cast<uint4*>(gran), (unsigned long)((size_t)2 * 16 * GRAN_F * 8 / 16), 0u, census};
    hipLaunchKernelGGL(make_wfrag_pair<false>, dim3(512), dim3(256), 0, st, w_hh_f, w_hh_r, wf[0], wf[1], H, aux);
    BiFwdP p{{gx_f, gx_r}, lens, y, (long)ldy, {gates_f, gates_r}, {cell_f, cell_r}, {wf[0], wf[1]}, gran, status, census, T, B,
             100000000L / 2};
    FT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(bilstm_persist_fwd_k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BI_LDS));
    hipLaunchKernelGGL(bilstm_persist_fwd_k, dim3(NWG), dim3(256), BI_LDS, st, p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}

extern "C" int FT_OPNAME(ft_bilstm_persist_bwd)(const float* dy, int64_t ldy, const float* w_hh_f, const float* w_hh_r, const int32_t* lens,
                                             const float* gates_f, const float* gates_r, const float* cell_f, const float* cell_r,
                                             float* dgx_f, float* dgx_r, void* work, int32_t* status, int T, int B, int H,
                                             void* stream) {
    FT_CHECK_ARG(dy && w_hh_f && w_hh_r && lens && gates_f && gates_r && cell_f && cell_r && dgx_f && dgx_r && work && status);
    FT_CHECK_ARG(T >= 0 && ldy >= 2 * (int64_t)H && reinterpret_cast<uintptr_t>(work) % 256 == 0);
    if (!ft_bilstm_persist_supported(B, H))
        return ft_fail(FT_EUNSUPPORTED, "ft_bilstm_persist_bwd: needs H == 256, B <= 32 and a 256-CU device (H=%d B=%d)", H, B);
    if (T == 0) return FT_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    char* base = reinterpret_cast<char*>(work);
    unsigned short* wf[2] = {reinterpret_cast<unsigned short*>(base), reinterpret_cast<unsigned short*>(base + al256b(BI_WFRAG))};
    unsigned long long* gran = reinterpret_cast<unsigned long long*>(base + 2 * al256b(BI_WFRAG));
    unsigned* census = reinterpret_cast<unsigned*>(base + 2 * al256b(BI_WFRAG) + al256b(BI_GRAN));
    FT_CHECK_HIP(hipMemsetAsync(dgx_f, 0, (size_t)T * B * 4 * H * 4, st));
    FT_CHECK_HIP(hipMemsetAsync(dgx_r, 0, (size_t)T * B * 4 * H * 4, st));
    static_assert(BI_GRAN % 16 == 0, "granule buffer in 16-byte pieces");
    const WfragAux aux{reinterpret_cast<uint4*>(gran), (unsigned long)(BI_GRAN / 16), 0u, census};
    hipLaunchKernelGGL(make_wfrag_pair<true>, dim3(512), dim3(256), 0, st, w_hh_f, w_hh_r, wf[0], wf[1], H, aux);
    BiBwdP p{dy, (long)ldy, lens, {gates_f, gates_r}, {cell_f, cell_r}, {dgx_f, dgx_r}, {wf[0], wf[1]}, gran, status, census, T, B,
             100000000L / 2, ftint_bilstm_prof};
    auto kern = p.prof ? bilstm_persist_bwd_prof_k : bilstm_persist_bwd_k;
    FT_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)BI_LDS));
    hipLaunchKernelGGL(kern, dim3(NWG), dim3(256), BI_LDS, st, p);
    FT_CHECK_LAUNCH();
    return FT_OK;
}
