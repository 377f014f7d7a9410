// The three big GEMMs of an attention layer on the split-16-bit main loop of gemm_split_glds.h (round 4): qkv_kv, mlp.0 (merge and
// the linear-attention apply folded in) and mlp.3, for the fp16 arithmetics (FP16X3 / FP16X4); the score contraction of BF16X6 and
// FP16X4 runs on the same loop.  Same maths, same buffers and the same epilogues (gatsspg_epilogue.h) as the fp32 kernels of gatsspg_gemm_kernels.hip
// (GATs_SuperGlue.py:69-128); what differs is how the operands reach the matrix pipe.
#include "gemm_split_glds.h"
#include "gatsspg_epilogue.h"
#include "gatsspg_launch.h"

#include <type_traits>

namespace gatsspg {

#ifndef GATSSPG_PROFILING_BUILD
static constexpr unsigned long long* g_trace = nullptr;   // (profiling builds: the buffer of gatsspg_debug_set_trace, tools/trace_sp.py)
#define SP_TRACE_ON(ptr) false
#else
#define SP_TRACE_ON(ptr) ((ptr) != nullptr)
#endif

// plain hooks: no side work; the first product of the K loop starts from zero (FRESH0) or from the caller's accumulators
template <bool FRESH0>
struct SpPlainHooks {
    static constexpr bool ENABLED = false;
    template <int I, int TM>
    __device__ __forceinline__ f32x16 (&target(f32x16 (&acc)[TM]))[TM] { return acc; }
    template <int I, int P>
    static constexpr bool fresh() { return FRESH0 && I == 0 && P == 0; }
    template <int I, int P>
    __device__ __forceinline__ void bvals(const float (&)[8]) {}
    template <int I, int TM>
    __device__ __forceinline__ void in_step(f32x16 (&)[TM]) {}
};

// =====================================================================================================
// K1  QKV projection + KV / ksum partials (qkv_kv_kernel of gatsspg_gemm_kernels.hip on the split loop).
//     128 x 64 tile on 4 waves (64 x 32 per wave), two stages (48 KiB): three workgroups per CU, so the 756 tiles of the headline
//     shape are resident at once and every SIMD holds three waves of three different workgroups (no common barrier).
// =====================================================================================================
template <int MODE>
using QkvSpTile = SpTile<128, 2, 2, 2, MODE>;

// fp16 modes on the slot schedule (SCHED 4); the bias through an LDS table, the Q tiles stored straight from the accumulators
template <class T, class LT = ColLayout>
__global__ __launch_bounds__(T::THREADS, 3) void qkv_kv_sp_kernel(const float* __restrict__ sc, const float* __restrict__ bqkv,
                                                                const unsigned short* __restrict__ P0, const unsigned short* __restrict__ P1,
                                                                const unsigned short* __restrict__ P2, const float* __restrict__ Z,
                                                                float* __restrict__ Qbuf, float* __restrict__ kvpart, LT L) {
    if (launch_is_off(L)) return;
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    float* smem = reinterpret_cast<float*>(smem_c);
    if constexpr (T::F16) fp16_saturate_mode();
    int rt, ct;
    if (!xcd_tile_map_g(6, active_tiles(L), L.xgs, rt, ct)) return;
    ct = global_tile(L, ct);
    const int c0 = ct * T::BN, ld = L.ld;
    if (tile_dead(L, c0)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / T::WN, wn = wave % T::WN, half = lane >> 5, l31 = lane & 31;
    static_assert(T::BM == 128, "one half piece of bias values");
    float* btab = reinterpret_cast<float*>(smem_c + T::RING_BYTES);   // bias table behind the ring (T::BM floats)
    float bias[T::TM][16];
    const float inv = T::F16 ? 1.f / (sc[0] * T::ACT_SCALE) : 1.f;
    f32x16 acc[T::TM][T::TN];
    const size_t ro = (size_t)rt * 128 * BK;
    // slab-major planes
    auto apl = [&](int kt, int pl) -> const void* { return (pl == 0 ? P0 : pl == 1 ? P1 : P2) + ro + (size_t)kt * 768 * BK; };
    auto bsl = [&](int kt) { return Z + (size_t)kt * BK * ld + c0; };
    SpPlainHooks<true> hooks;
    SpNoBx nobx;
    auto pre = [&]() {
        if (wave == 0 && lane < 32) glds16(bqkv + rt * 128 + 4 * lane, btab);   // 128 floats: half a piece
    };
    gemm_mainloop_sp<T, D / BK, decltype(apl), decltype(bsl), SpPlainHooks<true>, SpNoBx, 4, decltype(pre)>(
        reinterpret_cast<f32x16(&)[T::TM]>(acc), smem_c, apl, bsl, ld, hooks, nobx, nullptr, pre, false, 64);
    read_bias16<T>(btab, wm, half, bias);

    if (rt < 2) {
#pragma unroll
        for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][0][r] = elu1_select(fmaf(acc[tm][0][r], inv, bias[tm][r])) + 1.f;
        store_tile_regs<T>(acc, Qbuf + (size_t)rt * 128 * ld + c0, ld, [](int, float v) { return v; });
        return;
    }
    // ---- K_h / V_h tile -> LDS -> KV partial (second MFMA pass, fp32: exact like the fp32 kernel's; twin of the block in qkv_kv_kernel: keep
    // the two in step, gatsspg_epilogue.h says why it is not one helper)
    const int h = rt - 2;
    const TileSeg ts = tile_seg(L, c0, T::BN);
    constexpr int TS = T::BN + 4;
    static_assert(T::BN == QKV_BN && T::WAVES >= 4 && 128 * TS * 4 <= T::RING_BYTES, "one KV partial per 64-column tile");
    float* Tl = smem;
    float opmx = 0.f;   // largest K (> 0) or |V| entry this wave holds: its 64 rows are all K_h or all V_h
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (wm * T::TM + tm) * 32 + mfma_row(r, half);  // 0..63 = K_h channel d, 64..127 = V_h channel q
            const int col = wn * 32 + l31;
            float v = fmaf(acc[tm][0][r], inv, bias[tm][r]);
            const float kf = elu1_select(v) + 1.f;
            v = row < 64 ? kf : v;
            v = col >= ts.valid ? 0.f : v;  // pad columns must not enter the sums
            opmx = fmaxf(opmx, fabsf(v));
            Tl[row * TS + col] = v;
        }
    {
        // bound data for kv_final's scale of the message operator (|KV_h[q][d]| <= max |V| * ksum[d]): slots [4..7] max |V| per wave here,
        // slots [0..3] the per-wave largest key sum of the tile (ksum pass below).  Written in every arithmetic (a partial / database cache
        // must never carry uninitialised slots: round-5 advisor)
        static_assert((T::WAVES == 4 && T::TM == 2) || (T::WAVES == 8 && T::TM == 1), "4 waves: 0, 1 hold K_h, 2, 3 V_h; 8 waves: 0..3 K_h, 4..7 V_h");
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) opmx = fmaxf(opmx, __shfl_xor(opmx, o));
        if (lane == 0) {   // slots 4..7: max |V| per V-holding wave (0 for the K-holding ones); slots 0..3: the ksum pass below
            float* mx = kvpart + ((size_t)ct * H + h) * KVP + DH * DH + DH;
            if constexpr (T::WAVES == 8) {
                if (wave >= 4) mx[wave] = opmx;
            } else {
                mx[4 + wave] = wm == 0 ? 0.f : opmx;
            }
        }
    }
    __syncthreads();
    if (wave < 4) {   // (an 8-wave workgroup leaves this short pass to its first four waves)
        const int qi = wave >> 1, di = wave & 1;
        f32x16 kv;
#pragma unroll
        for (int r = 0; r < 16; ++r) kv[r] = 0.f;
        const float4* ap = reinterpret_cast<const float4*>(Tl + (di * 32 + l31) * TS + half * 32);
        const float4* bp = reinterpret_cast<const float4*>(Tl + (64 + qi * 32 + l31) * TS + half * 32);
#pragma unroll
        for (int v4 = 0; v4 < 8; ++v4) {
            const float4 a = ap[v4], b = bp[v4];
            kv = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, kv, 0, 0, 0);
            kv = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, kv, 0, 0, 0);
            kv = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, kv, 0, 0, 0);
            kv = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, kv, 0, 0, 0);
        }
        float* out = kvpart + ((size_t)ct * H + h) * KVP;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int d = di * 32 + mfma_row(r, half);
            out[d * DH + qi * 32 + l31] = kv[r];
        }
        {   // ksum[d] = sum_m K[d][m]: 4 lanes per row (16 columns each, fixed order), combined by 2 shuffles
            const int d = tid >> 2, qtr = tid & 3;
            const float* kr = Tl + d * TS + qtr * 16;
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < 16; ++m) s += kr[m];
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            if (qtr == 0) out[DH * DH + d] = s;
            // slot `wave` of the bound data (kv_final_kernel): the largest of this wave's 16 key sums
            float m = s;
#pragma unroll
            for (int o = 4; o <= 32; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
            if (lane == 0) out[DH * DH + DH + wave] = m;
        }
    }
}

// =====================================================================================================
// K4  mlp.0 with merge and the linear-attention apply folded in (mlp0_kernel / AttnFoldHooks of the fp32 path):
//         u = W0a x + sum_h z_h (.) (M_h Qf_h) + b,   z_h[n] = 1 / (Qf_h[:, n] . ksum_h + 1e-6)
//     K loop over [x ; Qf]: slabs 0..7 accumulate the x part, slabs 8 + 2h, 9 + 2h head h into one of TWO alternating head
//     accumulators that start from zero (the first product takes C = 0); head h - 1 is folded into the kept sum with its per-column
//     z while head h multiplies, so the fold's VALU work never waits for the matrix pipe.  The denominators come from the RAW B
//     values a lane holds anyway (8 consecutive k of its column per k16 half): 8 FMAs against the source's ksum (an LDS table),
//     added over the head's four halves in a fixed order, the two lane halves combined by one exchange -- per-lane in exactly the
//     32x32 C layout the fold needs, no LDS round trip.
// =====================================================================================================
template <int TM>
struct AttnFoldSp {
    static constexpr bool ENABLED = true;
    static constexpr int SPLIT = 8;
    f32x16 hacc[2][TM];
    float dpart[2];
    const float* ks;   // LDS: ksum of the source segment [4][64]
    float zfac[4];     // per head: (scale of the W0 planes) / (scale of the head's operator planes), an exact power of two (1 in the bf16 modes)
    int half;
    template <int I, int TM_>
    __device__ __forceinline__ f32x16 (&target(f32x16 (&acc)[TM_]))[TM_] {
        if constexpr (I < SPLIT) return acc;
        else return hacc[((I - SPLIT) >> 1) & 1];
    }
    template <int I, int P>
    static constexpr bool fresh() { return P == 0 && (I == 0 || (I >= SPLIT && ((I - SPLIT) & 1) == 0)); }
    template <int I, int P>
    __device__ __forceinline__ void bvals(const float (&v)[8]) {
        if constexpr (I >= SPLIT) {
            constexpr int h = (I - SPLIT) >> 1;
            const float* k = ks + h * 64 + ((I - SPLIT) & 1) * 32 + P * 16 + 8 * half;
            const float4 k0 = *reinterpret_cast<const float4*>(k), k1 = *reinterpret_cast<const float4*>(k + 4);
            float p = v[0] * k0.x;
            p = fmaf(v[1], k0.y, p); p = fmaf(v[2], k0.z, p); p = fmaf(v[3], k0.w, p);
            p = fmaf(v[4], k1.x, p); p = fmaf(v[5], k1.y, p); p = fmaf(v[6], k1.z, p); p = fmaf(v[7], k1.w, p);
            if constexpr (((I - SPLIT) & 1) == 0 && P == 0) dpart[h & 1] = p;
            else dpart[h & 1] += p;
        }
    }
    template <int HD>
    __device__ __forceinline__ void fold(f32x16 (&kept)[TM]) {
        float d = dpart[HD & 1];
        const float o = __shfl_xor(d, 32);
        d = half ? o + d : d + o;   // lane half 0's partial first on both halves
        const float z = zfac[HD] / (d + 1e-6f);
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) kept[tm][r] = fmaf(z, hacc[HD & 1][tm][r], kept[tm][r]);
    }
    // head h - 1 is folded beside the first products of head h (its own products were issued a whole slab earlier)
    template <int I, int TM_>
    __device__ __forceinline__ void in_step(f32x16 (&acc)[TM_]) {
        if constexpr (I >= SPLIT + 2 && ((I - SPLIT) & 1) == 0) fold<((I - SPLIT) >> 1) - 1>(acc);
    }
};

template <int MODE>
using Mlp0SpTileW = SpTile<128, 2, 4, 3, MODE>;   // 128 x 128 on 8 waves: 252 workgroups at the headline shape, one per CU, 96 KiB ring
template <int MODE>
using Mlp0SpTileN = SpTile<128, 2, 2, 3, MODE>;   // 128 x 64 on 4 waves: twice the workgroups (small shapes), two per CU

// fp16 modes on the slot schedule (SCHED 4); the bias through an LDS table
template <class T, class LT = ColLayout>
__global__ __launch_bounds__(T::THREADS, (T::TM == 4 ? 1 : (T::WAVES == 4 && T::NST == 2) ? 3 : 2)) void mlp0_sp_kernel(const float* __restrict__ sc, const float* __restrict__ b0,
                                                              const unsigned short* __restrict__ P0, const unsigned short* __restrict__ P1,
                                                              const unsigned short* __restrict__ P2, const float* __restrict__ Z,
                                                              const float* __restrict__ Qbuf, const unsigned short* __restrict__ Mpl,
                                                              const float* __restrict__ ksumT, const float* __restrict__ zsc,
                                                              float* __restrict__ U, float* __restrict__ statpart, float* __restrict__ stats,
                                                              int* __restrict__ statcnt, LT L, unsigned long long* trace) {
    if (launch_is_off(L)) return;
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    float* smem = reinterpret_cast<float*>(smem_c);
    if constexpr (T::F16) fp16_saturate_mode();
    SpTrace tr;
    const unsigned long long t_entry = SP_TRACE_ON(trace) ? __builtin_readcyclecounter() : 0;
    const unsigned long long w_entry = SP_TRACE_ON(trace) ? wall_clock64() : 0;   // 100 MHz constant clock: calibrates the s_memtime ticks
    int rt, ct;
    constexpr int TPW = T::BN / MLP0_BN;   // 64-column tiles (= InstanceNorm partials) per workgroup
    constexpr int MT = 512 / T::BM;
    if (!xcd_tile_map(MT, active_tiles(L) / TPW, rt, ct)) return;
    ct = global_tile(L, ct * TPW) / TPW;   // windows and segments are multiples of 128 columns
    const int c0 = ct * T::BN, ld = L.ld;
    if (tile_dead(L, c0)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / T::WN, wn = wave % T::WN, half = lane >> 5, l31 = lane & 31;
    const TileSeg ts = tile_seg(L, c0, T::BN);
    // ksum of the source segment -> LDS table behind the ring (published by the first barrier of the main loop)
    float* tab = reinterpret_cast<float*>(smem_c + T::RING_BYTES);
    // (filled by ONE LDS-DMA piece in front of the first slab requests: no register hop, no wait of its own)
    // requested before the main loop (behind it the two dependent round trips would sit on the critical path: measured 3.9 k cycles of
    // a 39 k-cycle kernel); hipcc parks some of the 32 values in scratch across the loop, which costs two scratch instructions each
    static_assert(T::BM == 128, "one half piece of bias values");
    float* btab = tab + 256;   // bias: a second LDS table (T::BM floats behind the ksum table)
    float bias[T::TM][16];
    const float inv = T::F16 ? 1.f / (sc[1] * T::ACT_SCALE) : 1.f;
    f32x16 acc[T::TM][T::TN];
    const size_t ro = (size_t)rt * T::BM * BK;   // slab-major planes: (m, k) at ((k / 32) * 512 + m) * 32 + k % 32
    const unsigned short* Mh = Mpl + (size_t)ts.seg * 3 * MPL_PLANE + ro;
    // slab-major planes of W0 (x half) and of the segment's message operator
    auto apl = [&](int kt, int pl) -> const void* {
        return kt < 8 ? (pl == 0 ? P0 : pl == 1 ? P1 : P2) + ro + (size_t)kt * 512 * BK : Mh + (size_t)pl * MPL_PLANE + (size_t)(kt - 8) * 512 * BK;
    };
    auto bsl = [&](int kt) { return (kt < 8 ? Z + (size_t)kt * BK * ld : Qbuf + (size_t)(kt - 8) * BK * ld) + c0; };
    AttnFoldSp<T::TM> hooks;
    hooks.ks = tab; hooks.half = half;
    {
        const float4 zf = *reinterpret_cast<const float4*>(zsc + ts.seg * H);
        hooks.zfac[0] = zf.x; hooks.zfac[1] = zf.y; hooks.zfac[2] = zf.z; hooks.zfac[3] = zf.w;
    }
    SpNoBx nobx;
    auto pre = [&]() {
        if (wave == 0) glds16(ksumT + (size_t)ts.seg * H * DH + 4 * lane, tab);   // [4][64] floats = 1 KiB
        if (wave == 1 && lane < 32) glds16(b0 + rt * T::BM + 4 * lane, btab);   // 128 floats: half a piece
    };
    gemm_mainloop_sp<T, 512 / BK, decltype(apl), decltype(bsl), AttnFoldSp<T::TM>, SpNoBx, 4, decltype(pre)>(
        reinterpret_cast<f32x16(&)[T::TM]>(acc), smem_c, apl, bsl, ld, hooks, nobx, &tr, pre, SP_TRACE_ON(trace), 64);
    if (SP_TRACE_ON(trace)) tr.t[9] = __builtin_readcyclecounter();    // behind the loop's last barrier
    hooks.template fold<3>(reinterpret_cast<f32x16(&)[T::TM]>(acc));
    read_bias16<T>(btab, wm, half, bias);

    // staging tile [BM][BN + 4]: the row stride (4 banks) keeps the scalar writes from the MFMA layout, the 16-byte row reads of the
    // store pass AND (with the walk skew below) the statistics reads free of bank conflicts (the [BN + 1] form of the fp32 kernel costs
    // a 4-way conflict on every read of the store pass: 12 % of this kernel's LDS cycles in profiles/r04_pmc_fp16x4_sq_lds.txt)
    constexpr int TS = T::BN + 4;
    static_assert(T::BM * TS * 4 <= T::RING_BYTES, "the output tile is staged in the ring");
    float* Tl = smem;
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (wm * T::TM + tm) * 32 + mfma_row(r, half);
            Tl[row * TS + wn * 32 + l31] = fmaf(acc[tm][0][r], inv, bias[tm][r]);
        }
    if (SP_TRACE_ON(trace)) tr.t[10] = __builtin_readcyclecounter();   // last fold + bias + tile written to LDS
    __syncthreads();
    if (SP_TRACE_ON(trace)) tr.t[11] = __builtin_readcyclecounter();
    // the tile leaves through LDS as 16-byte stores: 16 lanes cover one 256-byte row segment.  (A lambda, as the statistics were before they
    // moved to gatsspg_epilogue.h: written as a plain loop the 128-column kernel takes 76 instead of 77 SGPRs.)
    auto tile_stores = [&]() {
#pragma unroll
        for (int idx = tid; idx < T::BM * (T::BN / 4); idx += T::THREADS) {
            const int row = idx / (T::BN / 4), c4 = (idx % (T::BN / 4)) * 4;
            const vf4 v = *reinterpret_cast<const vf4*>(Tl + row * TS + c4);
            *reinterpret_cast<vf4*>(U + (size_t)(rt * T::BM + row) * ld + c0 + c4) = v;
        }
    };
    // per-tile InstanceNorm partials with the walk skew (mlp0_tile_statistics); the partial stores go first, the tile's own stores follow them
    mlp0_tile_statistics<T, TS, true>(Tl, statpart, ts.valid, rt, ct);
    asm volatile("" ::: "memory");
    tile_stores();
    if (SP_TRACE_ON(trace)) tr.t[12] = __builtin_readcyclecounter();   // tile stores issued
    constexpr int TILE_STORES = T::BM * (T::BN / 4) / T::THREADS;   // per thread, behind its partial stores
    static_assert(T::BM * (T::BN / 4) % T::THREADS == 0, "whole stores per thread");
    if (statcnt) stat_last_block<T, TILE_STORES>(statpart, stats, statcnt, L, ts, rt, smem);   // (never taken, statcnt = nullptr: kept so that the kernel's code is unchanged)
    if (SP_TRACE_ON(trace) && lane == 0) {   // 24 x u64 per wave: [hw_id, xcc_id, t_entry, t[0..8], t_end, rt, ct, wave, t[9..12], wall clock at entry / exit]
        unsigned long long* r = trace + ((size_t)blockIdx.x * T::WAVES + wave) * 24;
        r[0] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
        r[1] = __builtin_amdgcn_s_getreg((31 << 11) | 20);
        r[2] = t_entry;
#pragma unroll
        for (int k = 0; k < 9; ++k) r[3 + k] = tr.t[k];
        r[12] = __builtin_readcyclecounter();
        r[13] = rt; r[14] = ct; r[15] = wave;
#pragma unroll
        for (int k = 0; k < 4; ++k) r[16 + k] = tr.t[9 + k];
        r[20] = w_entry; r[21] = wall_clock64();
    }
}

// =====================================================================================================
// K6  mlp.3:  Z = (Z + b3) + W3 relu((u - mean) * rstd)   (mlp3_kernel of the fp32 path).  The InstanceNorm statistics of the
//     tile's segment sit in an LDS table (mean, rstd x activation pre-scale) and are applied to the raw B values in registers.
// =====================================================================================================
template <int MODE>
using Mlp3SpTile = SpTile<128, 2, 2, 3, MODE>;   // 128 x 64 on 4 waves (252 workgroups at the headline shape)
template <int MODE>
using Mlp3SpTile2 = SpTile<128, 2, 2, 2, MODE>;  // two-stage ring (52 KiB with the statistics table): three workgroups per CU

struct InstNormBx {
    static constexpr bool ON = true;
    const float* tab;   // LDS: mean[512] | rstd[512]
    __device__ __forceinline__ void fetch(int k, float2 (&x)[8]) const {
        const vf4* pm = reinterpret_cast<const vf4*>(tab + k);         // k is a multiple of 8: 32-byte aligned
        const vf4* pr = reinterpret_cast<const vf4*>(tab + 512 + k);
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const vf4 m = pm[q], r = pr[q];
#pragma unroll
            for (int e = 0; e < 4; ++e) x[4 * q + e] = make_float2(m[e], r[e]);
        }
    }
    __device__ __forceinline__ float apply(float v, float2 ms) const { return fmaxf((v - ms.x) * ms.y, 0.f); }
};

// fp16 modes on the slot schedule (SCHED 4); the tile stored straight from the accumulators
template <class T, class LT = ColLayout>
__global__ __launch_bounds__(T::THREADS, (T::NST == 2 ? 3 : 2)) void mlp3_sp_kernel(const float* __restrict__ sc, const float* __restrict__ b3,
                                                              const unsigned short* __restrict__ P0, const unsigned short* __restrict__ P1,
                                                              const unsigned short* __restrict__ P2, const float* __restrict__ U,
                                                              const float* __restrict__ stats, float* __restrict__ Z, LT L) {
    if (launch_is_off(L)) return;
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    float* smem = reinterpret_cast<float*>(smem_c);
    if constexpr (T::F16) fp16_saturate_mode();
    int rt, ct;
    constexpr int MT = 256 / T::BM;
    constexpr int TPW = T::BN / 64;
    if (!xcd_tile_map_g(MT, active_tiles(L) / TPW, L.xgs, rt, ct)) return;
    ct = global_tile(L, ct * TPW) / TPW;
    const int c0 = ct * T::BN, ld = L.ld;
    if (tile_dead(L, c0)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / T::WN, wn = wave % T::WN, half = lane >> 5, l31 = lane & 31;
    const TileSeg ts = tile_seg(L, c0, T::BN);
    const float sA = T::F16 ? sc[2] : 1.f;
    const float scale = sA * T::ACT_SCALE, inv = 1.f / scale;
    // statistics table behind the ring
    float* tab = reinterpret_cast<float*>(smem_c + T::RING_BYTES);   // mean[512] | rstd[512]: four LDS-DMA pieces in front of the first slabs
    static_assert(T::WAVES >= 4, "statistics table fill: one piece per wave");
    // start from (residual + bias) x the accumulator scale (exact: a power of two)
    f32x16 acc[T::TM][T::TN];
    {
        float bias[T::TM][16];   // (four 16-byte loads per 32-row tile instead of sixteen broadcast dword loads)
        load_bias16<T>(b3 + rt * T::BM, wm, half, bias);
#pragma unroll
        for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rt * T::BM + (wm * T::TM + tm) * 32 + mfma_row(r, half);
                acc[tm][0][r] = (Z[(size_t)row * ld + c0 + wn * 32 + l31] + bias[tm][r]) * scale;
            }
    }
    const size_t ro = (size_t)rt * T::BM * BK;
    auto apl = [&](int kt, int pl) -> const void* { return (pl == 0 ? P0 : pl == 1 ? P1 : P2) + ro + (size_t)kt * 256 * BK; };
    auto bsl = [&](int kt) { return U + (size_t)kt * BK * ld + c0; };
    SpPlainHooks<false> hooks;
    InstNormBx bx;
    bx.tab = tab;
    auto pre = [&]() {
        if (wave < 4) glds16(stats + (size_t)ts.seg * 2 * 512 + wave * 256 + 4 * lane, tab + wave * 256);
    };
    gemm_mainloop_sp<T, 512 / BK, decltype(apl), decltype(bsl), SpPlainHooks<false>, InstNormBx, 4, decltype(pre)>(
        reinterpret_cast<f32x16(&)[T::TM]>(acc), smem_c, apl, bsl, ld, hooks, bx, nullptr, pre, false, 64);
    store_tile_regs<T>(acc, Z + (size_t)rt * T::BM * ld + c0, ld, [inv](int, float v) { return v * inv; });
}

// =====================================================================================================
// K8  score contraction + exp (score_exp_kernel of the fp32 path, GATs_SuperGlue.py:217-218) on the split loop, for the fp32-class
//     arithmetics only (bf16x6, fp16x4):  E[n][m] = exp( (sum_d A[n][d] B[d][m]) / scale_factor ),  A = the 16-bit planes of the
//     normalised query descriptors (written by final_proj_norm_kernel: unit-norm rows, fp16 planes of 2^10 x), B = the fp32
//     normalised 3D descriptors, split in registers with the same 2^10.  Same tile (128 x 64), same partial-sum layout and the same
//     epilogue as the fp32 kernel: conf_finalize_kernel cannot tell them apart.
// =====================================================================================================
template <int MODE>
using ScoreSpTile = SpTile<SC_BM, 2, 2, 2, MODE, SCORE_SPLIT_SCALE_LOG2>;

template <class T, class LT = ColLayout>
__global__ __launch_bounds__(T::THREADS, 3) void score_exp_sp_kernel(const unsigned short* __restrict__ MDTp, const float* __restrict__ MD,
                                                                   float* __restrict__ conf, float* __restrict__ rowpart,
                                                                   float* __restrict__ colpart, LT L, float scale) {
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    float* smem = reinterpret_cast<float*>(smem_c);
    static_assert(T::BN == SC_BN && T::BM == SC_BM, "partial sums are per 128 x 64 tile");
    if constexpr (T::F16) fp16_saturate_mode();
    const int nrt = L.n1p / T::BM, nct = L.n2p / T::BN;   // segments are padded to multiples of 128
    int rt, ct;
    const int frame = blockIdx.y;
    if (!xcd_tile_map(nrt, nct, rt, ct)) return;
    if constexpr (is_frames<LT>) {
        if (rt * T::BM >= q_np(L, frame)) return;   // a row tile past the frame's own
    }
    const int ld = L.ld;
    const size_t R = (size_t)L.b * L.n1p;
    const size_t m0 = (size_t)frame * L.n1p + (size_t)rt * T::BM;
    const float* Bp = MD + (size_t)frame * L.np + L.n1p + ct * T::BN;
    f32x16 acc[T::TM][T::TN];
    auto apl = [&](int kt, int pl) { return MDTp + (size_t)pl * R * D + ((size_t)kt * R + m0) * BK; };
    auto bsl = [&](int kt) { return Bp + (size_t)kt * BK * ld; };
    SpPlainHooks<true> hooks;
    SpNoBx nobx;
    constexpr int SS = T::F16 ? 4 : 0;   // fp16x4: the slot schedule (gemm_split_glds.h); bf16x6: the plain one
    gemm_mainloop_sp<T, D / BK, decltype(apl), decltype(bsl), SpPlainHooks<true>, SpNoBx, SS>(reinterpret_cast<f32x16(&)[T::TM]>(acc), smem_c, apl, bsl, ld,
                                                                                                hooks, nobx);
    const float inv = T::F16 ? 1.f / (T::ACT_SCALE * T::ACT_SCALE) : 1.f;   // both operands carry the scale
    constexpr int TS = T::BN + 4;   // staged tile [128][68]: conflict-free 16-byte row reads (see mlp0_sp_kernel)
    static_assert(T::BM * TS * 4 <= T::RING_BYTES, "the output tile is staged in the ring");
    score_epilogue<T, TS, true, false, true>(acc, smem, conf, rowpart, colpart, L, frame, rt, ct, nrt, nct, inv, scale);
}

// ------------------------------------------------------------------------------------------------------
// host-side launchers
// ------------------------------------------------------------------------------------------------------
template <int MODE>
static void launch_score_sp_t(const Workspace& w, float* conf, float scale, hipStream_t s, ProfileHook* hk) {
    using T = ScoreSpTile<MODE>;
    with_layout(w, [&](const auto& L) {
        using LT = std::decay_t<decltype(L)>;
        allow_big_lds<score_exp_sp_kernel<T, LT>>();
        GATSSPG_LAUNCH(hk, KID_SCORE_EXP, s, (score_exp_sp_kernel<T, LT>), dim3(xcd_grid(w.L.n1p / T::BM, w.L.n2p / T::BN), w.L.b), dim3(T::THREADS),
                       (size_t)T::RING_BYTES, s, w.MDTp, w.MD, conf, w.rowpart, w.colpart, L, scale);
    });
}
void launch_score_exp_sp(const Workspace& w, float* conf, float scale, hipStream_t s, ProfileHook* hk) {
    if (w.prec == BF16X6) launch_score_sp_t<BF16X6>(w, conf, scale, s, hk);
    else launch_score_sp_t<FP16X4>(w, conf, scale, s, hk);
}

// The product runs the fp16 modes on the slot schedule (SCHED 4, gemm_split_glds.h) with the bias through an LDS table and the Q / mlp3 tiles
// stored straight from the accumulators, and the bf16x6 score contraction on the plain schedule (SCHED 0).  Removed alternatives, each
// measured and lost: schedules 0 / 2 / 3 for the three GEMMs (profiles/r04_ab_live_schedules.txt, r04_ab_live_slot_schedule.txt: 2 is 1.0-1.4 %
// faster per frame than 0, 3 another 1.0-1.6 %, 4 another 0.4 %), the ping-pong schedule, staged tile stores (r04_ab_live_direct_store.txt:
// -0.5 % per frame), per-lane bias loads (r04_ab_live_bias_table.txt), the four-stage ring and the two-stage / one-wave-per-SIMD mlp0 tiles
// (r04_ab_live_footprints.txt, r04_trace_sp_trace_*.txt), the main-loop ablations (r04_split_loop_ablations.txt), the bf16 modes and the
// fp32 arithmetic on this loop (r04_split_loop_ab.txt, r04_ab_live_fp32_dma.txt).

// mlp0's tile choice: the 128-column tile (8 waves, one workgroup per CU) moves two thirds of the operand bytes per product through L2: taken
// when its 4 x tiles workgroups make ONE round of the 256 CUs and fill at least three quarters of it (the headline shape: 252); with fewer the
// 64-column tile (4 waves, two workgroups per CU, twice as many) fills the chip better, with more than one round its co-resident pairs overlap
// one workgroup's store tail with the other's loop (fp16x4, 8 frames per step: 173 vs 185 us per launch)
constexpr int SP_MLP0_WIDE_MIN = 48, SP_MLP0_WIDE_MAX = 64;
static bool mlp0_sp_wide(int tiles) {   // tiles: 64-column tiles of the launch (of the frame alone, on a frames layout)
    const int wide_min = tuning_knob("SP_MLP0_WIDE_MIN", SP_MLP0_WIDE_MIN), wide_max = tuning_knob("SP_MLP0_WIDE_MAX", SP_MLP0_WIDE_MAX);
    return tiles / 2 >= wide_min && tiles / 2 <= wide_max;
}
// (mlp.0 leaving U point-major from transposed accumulators, read by mlp.3 as a transposed B operand: 1908 vs 1925 frames/s in flight, 237-243
//  registers instead of 192; and XCD-paired column tiles beside the 128-column mlp0 tile: no effect, 1912 vs 1908.  profiles/r05c_ab_live_ut_xcd_direct.txt;
//  both removed.  ColLayout::xgs stays 0: the kernels still read it, so that their code is unchanged.)

template <int MODE>
static void launch_qkv_sp_t(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk) {
    using T = QkvSpTile<MODE>;
    const WPlanes p = a.qkv_planes();
    with_layout(w, [&](const auto& L) {
        using LT = std::decay_t<decltype(L)>;
        allow_big_lds<qkv_kv_sp_kernel<T, LT>>();
        GATSSPG_LAUNCH(hk, KID_QKV_KV, s, (qkv_kv_sp_kernel<T, LT>), dim3(xcd_grid(6, active_tiles(w.L))), dim3(T::THREADS), (size_t)T::RING_BYTES + 1024, s,
                       a.SC(), a.BQKV(), p.h16, p.l16, p.l16, w.Z, w.Q, w.kvpart, L);
    });
}
void launch_qkv_kv_sp(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk) {
    if (w.prec == FP16X3) launch_qkv_sp_t<FP16X3>(a, w, s, hk);
    else launch_qkv_sp_t<FP16X4>(a, w, s, hk);
}

template <class T>
static void launch_mlp0_sp_t(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk) {
    const WPlanes p = a.w0_planes();
    const int NT = active_tiles(w.L) / (T::BN / MLP0_BN);
    with_layout(w, [&](const auto& L) {
        using LT = std::decay_t<decltype(L)>;
        allow_big_lds<mlp0_sp_kernel<T, LT>>();
        GATSSPG_LAUNCH(hk, KID_MLP0, s, (mlp0_sp_kernel<T, LT>), dim3(xcd_grid(512 / T::BM, NT)), dim3(T::THREADS), (size_t)T::RING_BYTES + 2048, s, a.SC(), a.B0(),
                       p.h16, p.l16, p.l16, w.Z, w.Q, w.Mpl, w.ksumT, w.zsc, w.U, w.statpart, w.stats, nullptr, L, g_trace);
    });
}
template <int MODE>
static void launch_mlp0_sp_m(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk) {
    // (the two tiles walk the columns of a statistics partial from different starts: every frame of a frames layout takes the tile it takes alone)
    launch_by_form(
        w, [](int tiles) { return mlp0_sp_wide(tiles); }, [&](const Workspace& v) { launch_mlp0_sp_t<Mlp0SpTileW<MODE>>(a, v, s, hk); },
        [&](const Workspace& v) { launch_mlp0_sp_t<Mlp0SpTileN<MODE>>(a, v, s, hk); });
}
void launch_mlp0_sp(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk) {
    if (w.prec == FP16X3) launch_mlp0_sp_m<FP16X3>(a, w, s, hk);
    else launch_mlp0_sp_m<FP16X4>(a, w, s, hk);
}

template <class T>
static void launch_mlp3_sp_v(const AttnLayer& a, int NT, const Workspace& w, hipStream_t s, ProfileHook* hk) {
    const WPlanes p = a.w3_planes();
    with_layout(w, [&](const auto& L) {
        using LT = std::decay_t<decltype(L)>;
        allow_big_lds<mlp3_sp_kernel<T, LT>>();
        GATSSPG_LAUNCH(hk, KID_MLP3, s, (mlp3_sp_kernel<T, LT>), dim3(xcd_grid(256 / T::BM, NT)), dim3(T::THREADS), (size_t)T::RING_BYTES + 4096, s, a.SC(), a.B3(),
                       p.h16, p.l16, p.l16, w.U, w.stats, w.Z, L);
    });
}
template <int MODE>
static void launch_mlp3_sp_t(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk) {
    using T = Mlp3SpTile<MODE>;
    using T2 = Mlp3SpTile2<MODE>;
    const int NT = active_tiles(w.L) / (T::BN / 64);
    // more than one round of the three-stage ring's two workgroups per CU (batched frames, N_3D = 20000): the two-stage ring's three
    // per CU turn 1.46 rounds into one at 8 frames per step (fp16x4-b8: 0.565 vs 0.571 ms per frame, profiles/r04_ab_live_b8_tiles.txt).
    // Tuning builds: GATSSPG_SP_NST2 >= 0 forces the choice (bit 1 = two-stage ring).
    const int nst2 = tuning_knob("SP_NST2", -1);
    const bool two_stage = nst2 >= 0 ? (nst2 & 2) != 0 : (256 / T2::BM) * NT > 512;
    if (two_stage) launch_mlp3_sp_v<T2>(a, NT, w, s, hk);
    else launch_mlp3_sp_v<T>(a, NT, w, s, hk);
}
void launch_mlp3_sp(const AttnLayer& a, const Workspace& w, hipStream_t s, ProfileHook* hk) {
    if (w.prec == FP16X3) launch_mlp3_sp_t<FP16X3>(a, w, s, hk);
    else launch_mlp3_sp_t<FP16X4>(a, w, s, hk);
}

}  // namespace gatsspg
