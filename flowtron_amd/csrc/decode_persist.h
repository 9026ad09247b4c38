// Hand-off protocol and weight-row helpers of the persistent decode kernels: dec_persist_k (csrc/decode.hip) and
// dec_persist_batch_k (csrc/decode_batch_k.h; decode_batch.hip, decode_forced.hip) share them, so a batched utterance runs the same floating-point operations.
// Included inside the anonymous namespace of decode.hip, decode_batch.hip and decode_forced.hip.
#pragma once

struct DecP {
    DecodeDev d;
    unsigned long long* gran;     // granule buffers, one per stage vector (offsets below, in granules)
    unsigned* census;             // 8 counters behind the nine granule copies (zeroed with them)
    int* status;
    long timeout_ticks;
    long* prof;                   // debug: [frame][12] wall-clock stamps of workgroup 0 (ft_decode_debug_prof), or null
};
enum { G_O = 0, G_HATT = 256, G_Q = 256 + 1024, G_SC = G_Q + 640, G_CTX = G_SC + 1024, G_H0 = G_CTX + 640, G_H1 = G_H0 + 1024,
       G_U1 = G_H1 + 1024, G_U2 = G_U1 + 1024, G_TOTAL = G_U2 + 1024 };

typedef __attribute__((address_space(1))) unsigned long long dgu64;
typedef __attribute__((ext_vector_type(4))) unsigned int du32x4;
constexpr int DEC_LAUX = 2;         // aux bits of the XCD-local gather loads: 2 = nt (as lstm_persist.hip's default), 16 = sc1

__device__ __forceinline__ void publish(unsigned long long* g, unsigned epoch, float v) {
    __hip_atomic_store((dgu64*)g, ((unsigned long long)epoch << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// into this XCD's copy: stays in its L2
__device__ __forceinline__ void publish_local(unsigned long long* g, unsigned epoch, float v) {
    __hip_atomic_store((dgu64*)g, ((unsigned long long)epoch << 32) | __float_as_uint(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Hand-off topology.  256 workgroups each polling a whole vector across the fabric is 2 MB of sc1 reads per pass -- measured,
// that contention (not the weight stream) is what a stage costs: ~3.5 us per hop against 0.63 us for a lone poller
// (scripts/exp/handoff_probe.hip).  So every vector crosses the fabric ONCE PER XCD: the 32 workgroups of an XCD (run-time census,
// as lstm_persist.hip) each relay a 1/32 slice from the global copy (sc1 polls, 16 lanes) into their XCD's own copy with
// workgroup-scope stores that stay in that XCD's L2, and all of them gather the whole vector from the local copy (~0.25 us).
// Tags travel with the data, so a granule is only ever forwarded / consumed when it shows the epoch: no fences anywhere.
struct Relay {
    unsigned long long* glob;     // p.gran: the producers' copy (write-through stores)
    unsigned long long* loc;      // this XCD's copy
    int q;                        // rank of this workgroup inside its XCD, 0..31
};

// all 256 threads: granules [0, n) of stage vector `off` (epoch-tagged, n <= 1024) -> dst[0, n) in LDS.  false = timed out.
// Granules [0, relay_lo) were produced INSIDE this XCD (stages every XCD computes for itself, below); [relay_lo, n) come from
// the chip-wide producers through the relay (relay_lo even).
__device__ __forceinline__ bool gather(const Relay& R, int off, int n, int relay_lo, unsigned epoch, float* dst, const DecP& p, long t_start) {
    const int npad = (n + 1) & ~1;
    bool ok_all = true;
    if (relay_lo < n) {   // ---- relay: slice q of [relay_lo, n) of the global copy -> local copy; lane pairs of wave 0
        const int S = 2 * ((n - relay_lo + 63) >> 6);
        const int j = relay_lo + R.q * S + 2 * (int)threadIdx.x;
        if ((int)threadIdx.x * 2 < S && j < n) {
            __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(R.glob + off, 0, npad * 8, 0x00020000);
            for (unsigned spins = 0;; ++spins) {
                const du32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rg, j * 8, 0, 16);        // sc1: two granules
                if (v[1] == epoch && (j + 1 >= n || v[3] == epoch)) {
                    __hip_atomic_store((dgu64*)(R.loc + off + j), ((unsigned long long)v[1] << 32) | v[0], __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                    if (j + 1 < n)
                        __hip_atomic_store((dgu64*)(R.loc + off + j + 1), ((unsigned long long)v[3] << 32) | v[2], __ATOMIC_RELAXED,
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
    // ---- gather from the XCD-local copy: a thread owns granule pairs 2 tid and 2 tid + 512, re-reads both while stale
    __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(R.loc + off, 0, npad * 8, 0x00020000);
    const int j0 = threadIdx.x * 2, j1 = j0 + 512;
    bool need0 = j0 < n, need1 = j1 < n;
    for (unsigned spins = 0; ok_all && (need0 | need1); ++spins) {
        du32x4 v0, v1;
        if (need0) v0 = __builtin_amdgcn_raw_buffer_load_b128(rs, j0 * 8, 0, DEC_LAUX);
        if (need1) v1 = __builtin_amdgcn_raw_buffer_load_b128(rs, j1 * 8, 0, DEC_LAUX);
        if (need0 && v0[1] == epoch && (j0 + 1 >= n || v0[3] == epoch)) {
            dst[j0] = __uint_as_float(v0[0]);
            if (j0 + 1 < n) dst[j0 + 1] = __uint_as_float(v0[2]);
            need0 = false;
        }
        if (need1 && v1[1] == epoch && (j1 + 1 >= n || v1[3] == epoch)) {
            dst[j1] = __uint_as_float(v1[0]);
            if (j1 + 1 < n) dst[j1 + 1] = __uint_as_float(v1[2]);
            need1 = false;
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

// R weight rows (bf16, K % 8 == 0) of one wave: `issue` requests every 16-byte piece (NL per lane and row) -- called BEFORE the
// wait for the stage's input --, `dot` multiplies them with the fp32 activation vector in LDS.
template <int R, int NL>
struct WRows {
    uint4 w[R][NL];
    __device__ __forceinline__ void issue(const bf16_t* const (&row)[R], int K, int lane) {
        const int K8 = K >> 3;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int kk = lane + 64 * j;
#pragma unroll
            for (int r = 0; r < R; ++r)
                w[r][j] = (kk < K8 && row[r]) ? reinterpret_cast<const uint4*>(row[r])[kk] : make_uint4(0u, 0u, 0u, 0u);
        }
    }
    __device__ __forceinline__ void dot(const float* x, int K, int lane, float (&acc)[R]) const {
        const int K8 = K >> 3;
        const float4* x4 = reinterpret_cast<const float4*>(x);
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int kk = lane + 64 * j;
            if (kk < K8) {
                const float4 xa = x4[2 * kk], xb = x4[2 * kk + 1];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // resident weights (dec_persist_k): an opaque copy keeps the bf16 -> fp32 unpacking INSIDE the frame loop;
                    // hoisted, the unpacked forms double the live set (480 registers) and spill to scratch
                    uint4 t = w[r][j];
                    asm volatile("" : "+v"(t.x), "+v"(t.y), "+v"(t.z), "+v"(t.w));
                    acc[r] += dot8(t, xa, xb);
                }
            }
        }
    }
};

// The same for fp32 weight rows (dec_persist_k<true>: the reference's own inference precision, inference.py:68-71).  A chunk of 8
// weights is two float4; `issue` requests them, `dot` multiplies.  RESIDENT rows are issued once before the frame loop and live in
// registers (AGPRs take what the 256 architectural registers cannot hold: the compiler parks them there and reads them back per
// use); STREAMED rows are re-issued every frame right before the wait for the stage's input and come from the L2 / Infinity Cache.
template <int R, int NL>
struct WRowsF {
    float4 w[R][NL][2];
    __device__ __forceinline__ void issue(const float* const (&row)[R], int K, int lane) {
        const int K8 = K >> 3;
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int kk = lane + 64 * j;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const bool ok = kk < K8 && row[r];
                const float4* src = reinterpret_cast<const float4*>(row[r]) + 2 * kk;
                w[r][j][0] = ok ? src[0] : make_float4(0.f, 0.f, 0.f, 0.f);
                w[r][j][1] = ok ? src[1] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    __device__ __forceinline__ void dot(const float* x, int K, int lane, float (&acc)[R]) const {
        const int K8 = K >> 3;
        const float4* x4 = reinterpret_cast<const float4*>(x);
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            const int kk = lane + 64 * j;
            if (kk < K8) {
                const float4 xa = x4[2 * kk], xb = x4[2 * kk + 1];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float4 a = w[r][j][0], b = w[r][j][1];
                    acc[r] += (a.x * xa.x + a.y * xa.y + a.z * xa.z + a.w * xa.w) + (b.x * xb.x + b.y * xb.y + b.z * xb.z + b.w * xb.w);
                }
            }
        }
    }
};

template <bool PRECISE = false>
__device__ __forceinline__ void cell_update(const float (&pre)[4], float& c, float& h) {
    float ig, fg, gg, og, cn;
    lstm_cell<!PRECISE>(pre, c, ig, fg, gg, og, cn, h);       // fast: v_exp / v_rcp forms (common.h, 16-bit operand modes); precise: libm
    c = cn;
}
// wave sum by DPP butterflies inside the 16-lane rows + four v_readlane (the ds_bpermute ladder of common.h's wave_sum costs
// ~0.2 us per sum, several sums sit on every stage's critical path); the result is wave-uniform
__device__ __forceinline__ float wsum(float v) {
    auto step = [](float x, auto ctrl) {
        return x + __uint_as_float(__builtin_amdgcn_update_dpp(0u, __float_as_uint(x), decltype(ctrl)::value, 0xf, 0xf, false));
    };
    v = step(v, std::integral_constant<int, 0xB1>{});     // quad_perm [1,0,3,2]
    v = step(v, std::integral_constant<int, 0x4E>{});     // quad_perm [2,3,0,1]
    v = step(v, std::integral_constant<int, 0x141>{});    // row_half_mirror
    v = step(v, std::integral_constant<int, 0x140>{});    // row_mirror
    const unsigned b = __float_as_uint(v);
    return (__uint_as_float(__builtin_amdgcn_readlane(b, 0)) + __uint_as_float(__builtin_amdgcn_readlane(b, 16))) +
           (__uint_as_float(__builtin_amdgcn_readlane(b, 32)) + __uint_as_float(__builtin_amdgcn_readlane(b, 48)));
}
__device__ __forceinline__ float sfloat(float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); }
__device__ __forceinline__ float fast_tanh(float x) {
    return 1.f - 2.f * __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(2.f * 1.4426950408889634f * x) + 1.f);
}

#ifndef FT_DECODE_LIBM
#define FT_DECODE_LIBM 0
#endif
template <int R, int NL, bool F32> using template_rows = typename std::conditional<F32, WRowsF<R, NL>, WRows<R, NL>>::type;
