// The batched persistent decode kernel: free-running (dec_persist_batch_k<F32, false>, csrc/decode_batch.hip) and along given alignment
// rows (dec_persist_batch_k<F32, true>, csrc/decode_forced.hip).  One template, so the two forms cannot drift apart; two translation units, so
// neither form's instantiations meet the other's in the optimiser (decode_batch.hip:1-5).
// Included inside the anonymous namespace of both, behind decode_dev.h and decode_persist.h.
#pragma once

// ---- Batched persistent decode: ONE launch per flow for 2 .. DEC_NBMAX utterances (dec_persist_batch_k; the forced form: 1 .. DEC_NBMAX).
// A frame of dec_persist_k is hand-off latency, not arithmetic: nine dependent hops, each a relay + gather of a stage vector.  Here
// every hop carries the vectors of all utterances still decoding, so the hops are paid once per frame for the whole group.  Same
// geometry (256 workgroups, one per CU, XCD census and relay, small stages replicated per XCD), same weight residency, and for each
// utterance the same floating-point operations in the same order (the dot helpers, wsum, cell_update, softmax, context and coupling
// above): every utterance comes out bit for bit as dec_persist_k decodes it alone.  Differences, none of them arithmetic:
//   - the utterance loop sits OUTSIDE the resident-weight dot: the weight registers are shared, one utterance's accumulators live
//   - key rows and value columns come from the XCD's L2 for each utterance and frame (dec_persist_k holds the first 128 / 256
//     positions in registers for the whole utterance), loaded into the same register arrays and used in the same unrolled code
//   - fp32 mode reads layer-1 W_ih and the context columns of layer-0 W_ih from the L2 (dec_persist_k<true>: 104 KB of LDS, which the
//     batch's activations take here), in the loop shape of dec_persist_k's dot_lds (dot_l2 below)
//   - the recurrent vectors are single-buffered: a barrier in front of the gather that overwrites a vector the previous stage read
// Granules: stage-major, stage X of utterance b at nb * G_X + b * (size of X); the stop flag of b behind its conv output.
constexpr int DEC_NBMAX = 4;

struct DecPB {
    DecP p;                       // p.d: the per-utterance operands are nb-strided (K, V [nb][L][A], residual, mel_out [nb][N][M],
    const int* n_lim;             //   attn_out [nb][N][L], n_done_dev [nb]); n_lim [nb]: frame limit of each utterance (<= N)
    const int* n_keys;            // [nb] or null: text positions of each utterance (1 ..= L; null = L for all)
    int nb;
};

// the key count of utterance b: its own text length inside the padded L (read where it is used: a scalar load, no live register)
__device__ __forceinline__ int keys_of(const int* n_keys, int b, int L) { return n_keys ? min(max(n_keys[b], 1), L) : L; }

// gather() for the live utterances of a batched launch: segment k < nlive is utterance b = byte k of `live`, granules [0, n_b) at
// off + b * seg -> dst + b * dst_stride, n_b = keys_of(n_keys, b, n) (n_keys null: n for every segment; no one publishes a granule
// past n_b, so none is waited for).  The same protocol: 16 lanes of wave 0 per segment relay [relay_lo, n_b) (n - relay_lo <= 1024),
// every thread re-reads its granule pairs 2 tid and 2 tid + 512 of every segment while stale.
__device__ __forceinline__ bool gather_b(const Relay& R, int off, int seg, int n, int relay_lo, unsigned live, int nlive, unsigned epoch,
                                         float* dst, int dst_stride, const DecP& p, long t_start, const int* n_keys = nullptr) {
    const int npad = (n + 1) & ~1;
    bool ok_all = true;
    if (relay_lo < n && (int)threadIdx.x < 16 * nlive) {
        const int k = threadIdx.x >> 4, t = threadIdx.x & 15;
        const int b = (int)((live >> (8 * k)) & 255u), nk = keys_of(n_keys, b, n);
        const int o = off + b * seg;
        const int S = 2 * ((n - relay_lo + 63) >> 6);
        const int j = relay_lo + R.q * S + 2 * t;
        if (2 * t < S && j < nk) {
            __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(R.glob + o, 0, npad * 8, 0x00020000);
            for (unsigned spins = 0;; ++spins) {
                const du32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rg, j * 8, 0, 16);
                if (v[1] == epoch && (j + 1 >= nk || v[3] == epoch)) {
                    __hip_atomic_store((dgu64*)(R.loc + o + j), ((unsigned long long)v[1] << 32) | v[0], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (j + 1 < nk)
                        __hip_atomic_store((dgu64*)(R.loc + o + j + 1), ((unsigned long long)v[3] << 32) | v[2], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                    break;
                }
                if ((spins & 63) == 63 && (wall_clock64() - t_start > p.timeout_ticks ||
                                           __hip_atomic_load(p.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
                    ok_all = false;
                    break;
                }
                asm volatile("" ::: "memory");
            }
        }
    }
    const int j0 = threadIdx.x * 2, j1 = j0 + 512;
    // bit 2k: pair j0 of segment k, bit 2k + 1: pair j1; need: the pair starts in the segment, pair: both of its granules are in it
    unsigned need = 0, pair = 0;
#pragma unroll
    for (int k = 0; k < DEC_NBMAX; ++k)
        if (k < nlive) {
            const int nk = keys_of(n_keys, (int)((live >> (8 * k)) & 255u), n);
            need |= ((j0 < nk ? 1u : 0u) | (j1 < nk ? 2u : 0u)) << (2 * k);
            pair |= ((j0 + 1 < nk ? 1u : 0u) | (j1 + 1 < nk ? 2u : 0u)) << (2 * k);
        }
    for (unsigned spins = 0; ok_all && need; ++spins) {
        du32x4 v[DEC_NBMAX][2];
#pragma unroll
        for (int k = 0; k < DEC_NBMAX; ++k) {
            __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(R.loc + off + (int)((live >> (8 * k)) & 255u) * seg, 0, npad * 8, 0x00020000);
            if (need & (1u << (2 * k))) v[k][0] = __builtin_amdgcn_raw_buffer_load_b128(rs, j0 * 8, 0, DEC_LAUX);
            if (need & (2u << (2 * k))) v[k][1] = __builtin_amdgcn_raw_buffer_load_b128(rs, j1 * 8, 0, DEC_LAUX);
        }
#pragma unroll
        for (int k = 0; k < DEC_NBMAX; ++k) {
            float* const d = dst + (int)((live >> (8 * k)) & 255u) * dst_stride;
            if ((need & (1u << (2 * k))) && v[k][0][1] == epoch && (!(pair & (1u << (2 * k))) || v[k][0][3] == epoch)) {
                d[j0] = __uint_as_float(v[k][0][0]);
                if (pair & (1u << (2 * k))) d[j0 + 1] = __uint_as_float(v[k][0][2]);
                need &= ~(1u << (2 * k));
            }
            if ((need & (2u << (2 * k))) && v[k][1][1] == epoch && (!(pair & (2u << (2 * k))) || v[k][1][3] == epoch)) {
                d[j1] = __uint_as_float(v[k][1][0]);
                if (pair & (2u << (2 * k))) d[j1 + 1] = __uint_as_float(v[k][1][2]);
                need &= ~(2u << (2 * k));
            }
        }
        if ((spins & 63) == 63 && (wall_clock64() - t_start > p.timeout_ticks ||
                                   __hip_atomic_load(p.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0)) {
            ok_all = false;
            break;
        }
        asm volatile("" ::: "memory");
    }
    if (!ok_all && (threadIdx.x & 63) == 0) atomicExch(p.status, 1);
    return __syncthreads_and(ok_all ? 1 : 0) != 0;
}

// FORCED: the attention row of every frame is GIVEN (P.forced [nb][N][L], rows in the flow's own time order) -- no query
// projection, no scores, no softmax: S2 only gathers h_att, S3a is gone with its hop, S3b takes the row as it is (dec_ctx_k's
// treatment of a forced row: no max, exp or division) and computes the context with the free form's code.
template <bool F32, bool FORCED>
__global__ __launch_bounds__(256, 1) void dec_persist_batch_k(const DecPB pb) {
    const DecP& p = pb.p;
    const DecodeDev& P = p.d;
    constexpr int H = 1024, A = 640, M = 80, LMAX = 1024, NB = DEC_NBMAX;
    // per-utterance activations: 30 KB each (the scores tile at the largest L), 132 KB in all with the shared rows (forced form: 120 KB, no s_q)
    __shared__ __attribute__((aligned(16))) float s_prev[NB][M + 16], s_cat[NB][H + A], s_q[NB][A], s_pr[NB][LMAX], s_h0[NB][H],
        s_h1[NB][H], s_u1[NB][H], s_u2[NB][H], s_o[NB][2 * M + 16], s_v[A], s_gw[H + A];
    __shared__ float s_red[8], s_cell[3][NB][4], s_gdone[NB];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), c = blockIdx.x;
    const int u = c * 4 + wave;
    const int L = P.L, N = P.N, nb = pb.nb;
    const long t_start = wall_clock64();
    __shared__ int s_slot[2];
    if (tid == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
        s_slot[0] = (int)(xcc & 7u);
        s_slot[1] = (int)__hip_atomic_fetch_add(p.census + (xcc & 7u), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int k = tid; k < NB * H; k += 256) { s_cat[k / H][k % H] = 0.f; s_h0[k / H][k % H] = 0.f; s_h1[k / H][k % H] = 0.f; }
    if (tid < 3 * NB * 4) (&s_cell[0][0][0])[tid] = 0.f;
    __syncthreads();
    Relay R;
    R.glob = p.gran;
    R.loc = p.gran + (size_t)G_TOTAL * nb * (1 + __builtin_amdgcn_readfirstlane(s_slot[0]));
    R.q = __builtin_amdgcn_readfirstlane(s_slot[1]);
    if (R.q >= 32) {
        if (tid == 0) atomicExch(p.status, 2);
        return;
    }
    // the utterances still decoding: byte k of `live` = utterance id, k < nlive (wave-uniform; every workgroup derives the same set
    // from the same stop flags)
    unsigned live = 0;
    int nlive = 0;
    for (int b = 0; b < nb; ++b)
        if (pb.n_lim[b] > 0) { live |= (unsigned)b << (8 * nlive); ++nlive; }
    auto lv = [&](int k) { return (int)((live >> (8 * k)) & 255u); };
    int i = 0;
    typedef typename std::conditional<F32, float, bf16_t>::type wt_t;
    const wt_t* rows4[4];
    auto gate_rows = [&](const wt_t* W, int K, int col0 = 0) {
#pragma unroll
        for (int g = 0; g < 4; ++g) rows4[g] = W + ((size_t)g * H + u) * K + col0;
    };
    auto wsel = [](const bf16_t* w16, const float* w32) -> const wt_t* {
        if constexpr (F32) return w32; else return w16;
    };
    template_rows<4, 1, F32> wa_ih;  template_rows<4, 2, F32> wa_hh;  template_rows<5, 2, F32> wq;
    template_rows<4, F32 ? 2 : 4, F32> w0_ih;                     // (fp32 mode: the h_att columns; the ctx columns: dot_l2 below)
    // fp32 mode: layer-1 W_ih and layer-0 W_ih[:, H:] -- the rows dec_persist_k<true> keeps in LDS -- read from the L2 inside the
    // same loop as its dot_lds (hipcc forms and packs the FMAs of a loop body by its shape: multiplying rows issued into registers
    // beforehand, the same expressions came out in a different order of roundings); four rows of stride rs floats times x
    auto dot_l2 = [&](const float* wl, size_t rs, const float* x, int K, float (&acc)[4]) {
        const float4* x4 = reinterpret_cast<const float4*>(x);
        for (int kk = lane; kk < (K >> 3); kk += 64) {
            const float4 xa = x4[2 * kk], xb = x4[2 * kk + 1];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float4 a = reinterpret_cast<const float4*>(wl + (size_t)r * rs)[2 * kk], b = reinterpret_cast<const float4*>(wl + (size_t)r * rs)[2 * kk + 1];
                acc[r] += (a.x * xa.x + a.y * xa.y + a.z * xa.z + a.w * xa.w) + (b.x * xb.x + b.y * xb.y + b.z * xb.z + b.w * xb.w);
            }
        }
    };
    template_rows<4, 2, F32> w0_hh, w1_ih, w1_hh;              // (w1_ih: 16-bit mode only)
    template_rows<1, 2, F32> wd0, wd1;  template_rows<2, 2, F32> wcv;
    const int slot = R.q * 4 + wave;
    // the streamed rows' addresses are formed at each request (kept across the frame loop, they were the registers that spilled)
    auto issue_q = [&]() {
        const wt_t* r5[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) r5[k] = wsel(P.w_query16, P.w_query) + (size_t)(slot + 128 * k) * H;
        wq.issue(r5, H, lane);
    };
    auto issue_cv = [&]() {
        const wt_t* r2[2] = {wsel(P.conv_w16, P.conv_w) + (size_t)slot * H,
                             slot + 128 < 2 * M ? wsel(P.conv_w16, P.conv_w) + (size_t)(slot + 128) * H : nullptr};
        wcv.issue(r2, H, lane);
    };
    auto issue_d0 = [&]() { const wt_t* r1[1] = {wsel(P.d0_w16, P.d0_w) + (size_t)u * H}; wd0.issue(r1, H, lane); };
    auto issue_d1 = [&]() { const wt_t* r1[1] = {wsel(P.d1_w16, P.d1_w) + (size_t)u * H}; wd1.issue(r1, H, lane); };
    auto issue_att_ih = [&]() { gate_rows(wsel(P.att_w_ih16, P.att_w_ih), M); wa_ih.issue(rows4, M, lane); };
    gate_rows(wsel(P.att_w_hh16, P.att_w_hh), H); wa_hh.issue(rows4, H, lane);
    if constexpr (F32) { gate_rows(P.l0_w_ih, H + A); w0_ih.issue(rows4, H, lane); }
    else { gate_rows(wsel(P.l0_w_ih16, P.l0_w_ih), H + A); w0_ih.issue(rows4, H + A, lane); }
    gate_rows(wsel(P.l0_w_hh16, P.l0_w_hh), H); w0_hh.issue(rows4, H, lane);
    gate_rows(wsel(P.l1_w_hh16, P.l1_w_hh), H); w1_hh.issue(rows4, H, lane);
    if constexpr (!F32) {
        gate_rows(P.l1_w_ih16, H); w1_ih.issue(rows4, H, lane);
        issue_att_ih();
        if constexpr (!FORCED) issue_q();
        issue_cv();
        issue_d0();
        issue_d1();
    }
    float b_att[4], b_0[4], b_1[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const size_t r = (size_t)g * H + u;
        b_att[g] = sfloat(P.att_b_ih[r] + P.att_b_hh[r]); b_0[g] = sfloat(P.l0_b_ih[r] + P.l0_b_hh[r]); b_1[g] = sfloat(P.l1_b_ih[r] + P.l1_b_hh[r]);
    }
    const float b_d0 = sfloat(P.d0_b[u]), b_d1 = sfloat(P.d1_b[u]);
    const float b_cv[2] = {sfloat(P.conv_b[slot]), sfloat(slot + 128 < 2 * M ? P.conv_b[slot + 128] : 0.f)};
    for (int k = tid; k < A; k += 256) s_v[k] = P.v[k];
    for (int k = tid; k < H + A; k += 256) s_gw[k] = (c == 0 && P.gate_w) ? P.gate_w[k] : 0.f;
    const float gate_b = (c == 0 && P.gate_w) ? P.gate_b[0] : 0.f;
    constexpr int KRES = F32 ? 1 : 2, VRES = F32 ? 2 : 4;         // dec_persist_k's register-held key rows / value columns
    constexpr bool LIBM = F32 && FT_DECODE_LIBM;
    auto act_tanh = [](float x) { if constexpr (LIBM) return tanhf(x); else return fast_tanh(x); };
    const bool prof = p.prof != nullptr && c == 0 && tid == 0;
    auto stamp = [&](int k) { if (prof && i < 512) p.prof[(size_t)i * 12 + k] = wall_clock64(); };
    // granule offsets of the stage vectors (utterance b's segment: + b * its length)
    const int gO = G_O * nb, gHATT = G_HATT * nb, gQ = G_Q * nb, gSC = G_SC * nb, gCTX = G_CTX * nb, gH0 = G_H0 * nb, gH1 = G_H1 * nb,
              gU1 = G_U1 * nb, gU2 = G_U2 * nb;
    for (; nlive > 0; ++i) {
        const unsigned e0 = (unsigned)i * 16u;
        stamp(0);
        // ================= S1: inverse coupling of frame i-1, the end of every utterance that stopped there, attention LSTM of frame i
        if constexpr (F32) issue_att_ih();
        if (i > 0) {
            float z[NB];
#pragma unroll
            for (int k = 0; k < NB; ++k) z[k] = (k < nlive && tid < M) ? P.residual[((size_t)lv(k) * N + i - 1) * M + tid] : 0.f;
            if (!gather_b(R, gO, G_HATT - G_O, 2 * M + 1, 2 * M, live, nlive, e0 - 16u + 9u, &s_o[0][0], 2 * M + 16, p, t_start)) return;
            stamp(1);
            unsigned still = 0;
            int n_still = 0;
#pragma unroll
            for (int k = 0; k < NB; ++k)
                if (k < nlive) {
                    const int b = lv(k);
                    if (tid < M) {
                        const float x = (z[k] - s_o[b][M + tid]) / expf(s_o[b][tid]);
                        s_prev[b][tid] = x;
                        if (c == 0) P.mel_out[((size_t)b * N + i - 1) * M + tid] = x;
                    }
                    if (c == 0 && tid == 0) P.n_done_dev[b] = i;
                    if (s_o[b][2 * M] == 0.f && i < min(pb.n_lim[b], N)) { still |= (unsigned)b << (8 * n_still); ++n_still; }
                }
            live = __builtin_amdgcn_readfirstlane(still);
            nlive = __builtin_amdgcn_readfirstlane(n_still);
        } else {
            for (int k = tid; k < NB * M; k += 256) s_prev[k / M][k % M] = 0.f;
        }
        __syncthreads();
        if (nlive == 0) break;
        for (int k = 0; k < nlive; ++k) {
            const int b = lv(k);
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            wa_ih.dot(s_prev[b], M, lane, acc);
            wa_hh.dot(s_cat[b], H, lane, acc);
            float pre[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) pre[g] = wsum(acc[g]) + b_att[g];
            float cs = s_cell[0][b][wave], h;
            cell_update<LIBM>(pre, cs, h);
            if (lane == 0) { s_cell[0][b][wave] = cs; publish(p.gran + gHATT + b * H + u, e0 + 1u, h); }
        }
        // ================= S2: query rows slot + 128 k
        stamp(2);
        if constexpr (F32 && !FORCED) issue_q();
        // forced form: the rows of frame i, column tid + 256 j of utterance lv(k), requested in front of the wait for h_att
        float f_row[NB][LMAX / 256];
        if constexpr (FORCED) {
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                const int b = k < nlive ? lv(k) : 0, Lb = k < nlive ? keys_of(pb.n_keys, b, L) : 0;
#pragma unroll
                for (int j = 0; j < LMAX / 256; ++j)
                    f_row[k][j] = tid + 256 * j < Lb ? P.forced[((size_t)b * N + i) * L + tid + 256 * j] : 0.f;
            }
        }
        __syncthreads();                                          // (S1 has read the previous h_att that this gather overwrites)
        if (!gather_b(R, gHATT, H, H, 0, live, nlive, e0 + 1u, &s_cat[0][0], H + A, p, t_start)) return;
        stamp(3);
        if constexpr (FORCED) {
            stamp(4);
#pragma unroll
            for (int k = 0; k < NB; ++k)
                if (k < nlive) {
                    const int b = lv(k), Lb = keys_of(pb.n_keys, b, L);
#pragma unroll
                    for (int j = 0; j < LMAX / 256; ++j)
                        if (tid + 256 * j < Lb) {
                            s_pr[b][tid + 256 * j] = f_row[k][j];
                            if (c == 0) P.attn_out[((size_t)b * N + i) * L + tid + 256 * j] = f_row[k][j];   // the given row, verbatim
                        }
                }
            __syncthreads();
            stamp(5);
        }
        const int nfree = FORCED ? 0 : nlive;                     // (the query and score loops: none along a given row)
        for (int k = 0; k < nfree; ++k) {
            const int b = lv(k);
            float acc[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            wq.dot(s_cat[b], H, lane, acc);
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                const float v = wsum(acc[r]);
                if (lane == 0) publish_local(R.loc + gQ + b * A + slot + 128 * r, e0 + 2u, v);
            }
        }
        // ================= S3a: scores of text positions slot + 128 k < L_b (key rows from the L2)
        if (!FORCED && !gather_b(R, gQ, A, A, A, live, nlive, e0 + 2u, &s_q[0][0], A, p, t_start)) return;
        if constexpr (!FORCED) stamp(4);
        for (int k = 0; k < nfree; ++k) {
            const int b = lv(k), Lb = keys_of(pb.n_keys, b, L);  // (utterance b's own text: dec_persist_k's code at L = Lb)
            const float* const Kb = P.K + (size_t)b * L * A;
            // dec_persist_k's shape of this stage: the first KRES positions from registers, unrolled, the rest in the loop (the same
            // expressions; the compiler fuses the two shapes differently, so the shape is kept); here the registers are filled from
            // the L2 for each utterance
            float k_row[KRES][A / 64];
#pragma unroll
            for (int j = 0; j < A / 64; ++j)
#pragma unroll
                for (int kk = 0; kk < KRES; ++kk) k_row[kk][j] = slot + 128 * kk < Lb ? Kb[(size_t)(slot + 128 * kk) * A + lane + 64 * j] : 0.f;
#pragma unroll
            for (int kk = 0; kk < KRES; ++kk)
                if (slot + 128 * kk < Lb) {
                    float sc = 0.f;
#pragma unroll
                    for (int j = 0; j < A / 64; ++j) sc += s_v[lane + 64 * j] * act_tanh(s_q[b][lane + 64 * j] + k_row[kk][j]);
                    sc = wsum(sc);
                    if (lane == 0) publish_local(R.loc + gSC + b * LMAX + slot + 128 * kk, e0 + 3u, sc * P.inv_temp);
                }
            for (int l = slot + 128 * KRES; l < Lb; l += 128) {
                float sc = 0.f;
#pragma unroll
                for (int j = 0; j < A / 64; ++j) sc += s_v[lane + 64 * j] * act_tanh(s_q[b][lane + 64 * j] + Kb[(size_t)l * A + lane + 64 * j]);
                sc = wsum(sc);
                if (lane == 0) publish_local(R.loc + gSC + b * LMAX + l, e0 + 3u, sc * P.inv_temp);
            }
        }
        // ================= S3b: softmax over L_b, context channels slot + 128 k (value columns from the L2; attn_out rows of stride L)
        if (!FORCED && !gather_b(R, gSC, LMAX, L, L, live, nlive, e0 + 3u, &s_pr[0][0], LMAX, p, t_start, pb.n_keys)) return;
        if constexpr (!FORCED) stamp(5);
        for (int k = 0; k < nlive; ++k) {
            const int b = lv(k), Lb = keys_of(pb.n_keys, b, L);
            float* const pr = s_pr[b];
            const float* const Vb = P.V + (size_t)b * L * A;
            float v_col[5][VRES];                                 // (requested before the softmax; dec_persist_k's shape, as the scores)
#pragma unroll
            for (int r = 0; r < 5; ++r)
#pragma unroll
                for (int j = 0; j < VRES; ++j) v_col[r][j] = lane + 64 * j < Lb ? Vb[(size_t)(lane + 64 * j) * A + slot + 128 * r] : 0.f;
            if constexpr (!FORCED) {                              // (a given row is taken as it is)
                float m = -INFINITY;
                for (int l = tid; l < Lb; l += 256) m = fmaxf(m, pr[l]);
                m = wave_max(m);
                if (lane == 0) s_red[wave] = m;
                __syncthreads();
                m = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
                float sum = 0.f;
                for (int l = tid; l < Lb; l += 256) { const float e = expf(pr[l] - m); pr[l] = e; sum += e; }
                sum = wsum(sum);
                if (lane == 0) s_red[4 + wave] = sum;
                __syncthreads();
                sum = s_red[4] + s_red[5] + s_red[6] + s_red[7];
                for (int l = tid; l < Lb; l += 256) {
                    const float pl = pr[l] / sum;
                    pr[l] = pl;
                    if (c == 0) P.attn_out[((size_t)b * N + i) * L + l] = pl;
                }
                __syncthreads();
            }
            float pl[VRES];
#pragma unroll
            for (int j = 0; j < VRES; ++j) pl[j] = lane + 64 * j < Lb ? pr[lane + 64 * j] : 0.f;
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                float cx = 0.f;
#pragma unroll
                for (int j = 0; j < VRES; ++j) cx += pl[j] * v_col[r][j];
                for (int l = lane + 64 * VRES; l < Lb; l += 64) cx += pr[l] * Vb[(size_t)l * A + slot + 128 * r];
                cx = wsum(cx);
                if (lane == 0) publish_local(R.loc + gCTX + b * A + slot + 128 * r, e0 + 4u, cx);
            }
        }
        // ================= S4: LSTM layer 0 (input [h_att ; ctx], recurrent h0); workgroup 0 also evaluates the gates
        if (!gather_b(R, gCTX, A, A, A, live, nlive, e0 + 4u, &s_cat[0][H], H + A, p, t_start)) return;
        stamp(6);
        if (c == 0) {                                             // (uniform branch: all of workgroup 0)
            for (int k = 0; k < nlive; ++k) {
                const int b = lv(k);
                float gate_done = 0.f;
                if (P.gate_w) {
                    float g = 0.f;
                    for (int kk = tid; kk < H + A; kk += 256) g += s_gw[kk] * s_cat[b][kk];
                    g = wsum(g);
                    if (lane == 0) s_red[wave] = g;
                    __syncthreads();
                    const float gs = gate_b + s_red[0] + s_red[1] + s_red[2] + s_red[3];
                    gate_done = (1.f / (1.f + expf(-gs)) > P.gate_threshold) ? 1.f : 0.f;
                    __syncthreads();                              // (s_red is the next utterance's)
                }
                if (tid == 0) s_gdone[b] = gate_done;
            }
        }
        for (int k = 0; k < nlive; ++k) {
            const int b = lv(k);
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (F32) { w0_ih.dot(s_cat[b], H, lane, acc); dot_l2(P.l0_w_ih + (size_t)u * (H + A) + H, (size_t)H * (H + A), s_cat[b] + H, A, acc); }
            else w0_ih.dot(s_cat[b], H + A, lane, acc);
            w0_hh.dot(s_h0[b], H, lane, acc);
            float pre[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) pre[g] = wsum(acc[g]) + b_0[g];
            float cs = s_cell[1][b][wave], h;
            cell_update<LIBM>(pre, cs, h);
            if (lane == 0) { s_cell[1][b][wave] = cs; publish(p.gran + gH0 + b * H + u, e0 + 5u, h); }
        }
        // ================= S5: LSTM layer 1
        __syncthreads();                                          // (S4 has read the previous h0)
        if (!gather_b(R, gH0, H, H, 0, live, nlive, e0 + 5u, &s_h0[0][0], H, p, t_start)) return;
        stamp(7);
        for (int k = 0; k < nlive; ++k) {
            const int b = lv(k);
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            if constexpr (F32) dot_l2(P.l1_w_ih + (size_t)u * H, (size_t)H * H, s_h0[b], H, acc);
            else w1_ih.dot(s_h0[b], H, lane, acc);
            w1_hh.dot(s_h1[b], H, lane, acc);
            float pre[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) pre[g] = wsum(acc[g]) + b_1[g];
            float cs = s_cell[2][b][wave], h;
            cell_update<LIBM>(pre, cs, h);
            if (lane == 0) { s_cell[2][b][wave] = cs; publish(p.gran + gH1 + b * H + u, e0 + 6u, h); }
        }
        // ================= S6 / S7: dense + tanh, row u
        if constexpr (F32) issue_d0();
        __syncthreads();                                          // (S5 has read the previous h1)
        if (!gather_b(R, gH1, H, H, 0, live, nlive, e0 + 6u, &s_h1[0][0], H, p, t_start)) return;
        stamp(8);
        for (int k = 0; k < nlive; ++k) {
            const int b = lv(k);
            float acc[1] = {0.f};
            wd0.dot(s_h1[b], H, lane, acc);
            const float v = act_tanh(wsum(acc[0]) + b_d0);
            if (lane == 0) publish(p.gran + gU1 + b * H + u, e0 + 7u, v);
        }
        if constexpr (F32) issue_d1();
        if (!gather_b(R, gU1, H, H, 0, live, nlive, e0 + 7u, &s_u1[0][0], H, p, t_start)) return;
        stamp(9);
        for (int k = 0; k < nlive; ++k) {
            const int b = lv(k);
            float acc[1] = {0.f};
            wd1.dot(s_u1[b], H, lane, acc);
            const float v = act_tanh(wsum(acc[0]) + b_d1);
            if (lane == 0) publish(p.gran + gU2 + b * H + u, e0 + 8u, v);
        }
        // ================= S8: 1x1 conv rows slot, slot + 128; workgroup 0 appends the stop flags
        if constexpr (F32) issue_cv();
        if (!gather_b(R, gU2, H, H, 0, live, nlive, e0 + 8u, &s_u2[0][0], H, p, t_start)) return;
        stamp(10);
        for (int k = 0; k < nlive; ++k) {
            const int b = lv(k);
            float acc[2] = {0.f, 0.f};
            wcv.dot(s_u2[b], H, lane, acc);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const float v = wsum(acc[r]) + b_cv[r];
                if (lane == 0 && slot + 128 * r < 2 * M) publish_local(R.loc + gO + b * (G_HATT - G_O) + slot + 128 * r, e0 + 9u, v);
            }
            if (c == 0 && tid == 0) publish(p.gran + gO + b * (G_HATT - G_O) + 2 * M, e0 + 9u, s_gdone[b]);
        }
    }
}
