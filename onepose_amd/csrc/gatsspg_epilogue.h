// Matcher-only device pieces shared by the two GEMM kernel families of the GATsSPG forward -- the register-staged loops
// (gatsspg_gemm_kernels.hip on gemm_f32_mfma.h) and the LDS-DMA split loop (gatsspg_split_kernels.hip on gemm_split_glds.h): the attention
// fold hooks, the bias fetch, mlp.0's tile statistics, the score epilogue and the fused InstanceNorm reducer.  One copy of each, so that a
// fix to pad masking or a fixed summation order reaches every arithmetic.
// Not here, on purpose: the K/V tile -> KV partial pass of qkv_kv_kernel / qkv_kv_sp_kernel and mlp.0's 16-byte tile stores.  Every helper
// form of the KV pass that was tried (whole, fill and MFMA pass apart, indices or the output pointer as arguments, with and without a value
// functor) moved hipcc's register allocation of the fp32-path kernel -- bf16x3 88 -> 106..108 VGPRs (5 -> 4 waves per SIMD), bf16x6
// 100 -> 104, fp32 80 -> 71..73 -- and the shared tile stores that of the 128-column mlp0_sp_kernel (186 -> 188); both stay in their kernels.
#pragma once
#include "gemm_f32_mfma.h"

namespace gatsspg {

__device__ __forceinline__ float elu1(float x) { return x > 0.f ? x : expm1f(x); }
// same values, branch-free: both sides are evaluated and selected (epilogues that apply elu to 16-32 accumulator values per
// lane: a divergent branch per value serialises whatever sits next to it)
__device__ __forceinline__ float elu1_select(float x) {
    const float e = expm1f(fminf(x, 0.f));
    return x > 0.f ? x : e;
}

// ---------------------------------------------------------------------------------------------------------------------
// Main-loop hooks of the mlp.0 kernel with the linear-attention apply folded in (GATs_SuperGlue.py:78-79,101,113,122):
//   u = W0a x + sum_h z_h (.) (M_h Qf_h) + b,   M_h = (W0b Wm)[:, head h] KV_h  (kv_final_kernel),   Qf = elu(q) + 1,
//   z_h[n] = 1 / (sum_d Qf_h[d][n] ksum_h[d] + 1e-6).
// The K loop runs over [x ; Qf] (16 slabs of 32): slabs 0..7 accumulate the x part, slabs 8 + 2h, 9 + 2h the product of
// head h into a zeroed accumulator, which is folded into the kept sum with the per-column z_h (a per-lane scalar in the
// 32x32 MFMA C layout) when the pair ends.  The denominators come from the staged Qf values themselves: every thread
// multiplies the 4 consecutive k rows of ONE column it sees (fp32 loop: from the LDS slab being computed; split-bf16
// loops: the registers it is about to split) with the source's ksum, the two slabs of a head are added in the thread, the
// eight per-wave partials go to LDS and are summed in wave order at the fold: fixed order, no atomics.
// Requires a 64-column tile on 8 waves (thread = (k group = wave, column = lane)) and one 32x32 MFMA tile per wave.
// ---------------------------------------------------------------------------------------------------------------------
struct AttnFoldHooks {
    static constexpr bool ENABLED = true;
    static constexpr int SPLIT = 8;          // first slab of the head phase
    static constexpr int ZP_FLOATS = 2 * 8 * 64;
    const float* ks;                         // ksum of the source segment, [4][64] (global, wave-uniform reads)
    float* zp;                               // LDS [2 (head parity)][8 waves][64 columns]
    f32x16 kept;                             // x part + folded heads
    float carry;                             // this thread's partial of the first slab of the current head
    int wave, lane, col;                     // col = this lane's column in the MFMA C layout (wn * 32 + l31)
    __device__ __forceinline__ void init(const float* ksum_src, float* zp_lds, int wn) {
        ks = ksum_src; zp = zp_lds; carry = 0.f;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        lane = threadIdx.x & 63;
        col = wn * 32 + (lane & 31);
    }
    // j = slab index within the head phase (0..7); v0..v3 = rows 4 * wave .. + 3 of that slab, column `lane` of the tile
    __device__ __forceinline__ void partial(int j, float v0, float v1, float v2, float v3) {
        const int h = j >> 1;
        const float* k = ks + h * 64 + (j & 1) * 32 + wave * 4;
        float p = v0 * k[0];
        p = fmaf(v1, k[1], p);
        p = fmaf(v2, k[2], p);
        p = fmaf(v3, k[3], p);
        if (j & 1) zp[((h & 1) * 8 + wave) * 64 + lane] = carry + p;
        else carry = p;
    }
    // called after the barrier that ends the slab pair (i, i + 1)
    __device__ __forceinline__ void pair_end(int i, f32x16& acc) {
        if (i < SPLIT - 2) return;
        if (i == SPLIT - 2) {
            kept = acc;
        } else {
            const int h = (i - SPLIT) >> 1;
            const float* zr = zp + (h & 1) * 8 * 64 + col;
            float d = zr[0];
#pragma unroll
            for (int w = 1; w < 8; ++w) d += zr[w * 64];
            const float z = 1.f / (d + 1e-6f);
#pragma unroll
            for (int r = 0; r < 16; ++r) kept[r] = fmaf(z, acc[r], kept[r]);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    }
};

// A lane's 16 bias values per 32-row MFMA tile (rows 8 k + 4 half + 0..3 of the tile: four 16-byte reads), in two forms:
//   load_bias16: from global memory (b = the bias of the workgroup's first row).  Requested BEFORE the main loop where the registers
//     allow it: read in the epilogue next to elu's branch they became 16 dependent load -> wait -> write rounds per lane.
//   read_bias16: from an LDS table of the workgroup's BM bias values.  The table is filled by HALF an LDS-DMA piece (32 lanes x 16 bytes)
//     requested at kernel entry -- older than every operand load of the main loop, so the loop's own waits and barriers cover and publish
//     it -- and read behind the loop: no bias registers across the loop, no per-lane global loads in front of the first operand requests
//     (frames in flight: +3..4 % on the split loop, profiles/r04_ab_live_bias_table.txt).
template <class T>
__device__ __forceinline__ void unpack_bias16(const float* b, int wm, int half, float (&bias)[T::TM][16]) {
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const vf4 b4 = ldg4(b + (wm * T::TM + tm) * 32 + 8 * k + 4 * half);
            bias[tm][4 * k + 0] = b4[0]; bias[tm][4 * k + 1] = b4[1]; bias[tm][4 * k + 2] = b4[2]; bias[tm][4 * k + 3] = b4[3];
        }
}
template <class T>
__device__ __forceinline__ void load_bias16(const float* b, int wm, int half, float (&bias)[T::TM][16]) { unpack_bias16<T>(b, wm, half, bias); }
template <class T>
__device__ __forceinline__ void read_bias16(const float* tab, int wm, int half, float (&bias)[T::TM][16]) { unpack_bias16<T>(tab, wm, half, bias); }

// ---------------------------------------------------------------------------------------------------------------------
// InstanceNorm statistics fused into the mlp.0 launch (replaces the stat_final_kernel launch between mlp.0 and mlp.3): the LAST
// workgroup of a (segment, row tile) to finish turns the per-tile partials of its rows into mean / rstd.
//   * every workgroup leaves its partials with write-through (agent-scope) stores, waits for them (vmcnt(0) + barrier) and draws a
//     ticket from the (segment, row tile) counter with one relaxed agent-scope atomic -- no L2 write-back fence (guide G16, sc1 form);
//   * the workgroup that draws the last ticket reads ALL partials of its rows with agent-scope loads and merges them exactly like
//     stat_final_kernel did (Chan's formula in double precision, tile ranges summed in tile order, ranges combined in range order):
//     the result does not depend on WHICH workgroup is last nor on the order of arrival -- run-to-run bit-identical;
//   * the counters are zeroed by kv_final_kernel (always enqueued before mlp.0 on the same segments) and reset by the reducer.
// smem: 2 * THREADS doubles + one int, free at the call.  stats: [seg][2][512] (mean, 1 / sqrt(var + 1e-5)), GATs_SuperGlue.py:126.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int STATCNT_PER_SEG = 8;   // row tiles of mlp.0 per segment (512 / 64 at most)
__device__ __forceinline__ void stat_partial_store(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// PENDING: vector-memory instructions this thread issued AFTER its partial stores (the tile's own stores), which may stay in flight
// NOT VALID ON A FRAMES LAYOUT (FramesLayout, gatsspg_common.h): the arrival count nwg, the tile count nt and n below are the CAPACITY's there,
// while the workgroups past a frame's own tiles never arrive and the frame's sums run over its own tiles (stat_final_kernel takes q_n / q_np).
// Every launcher passes statcnt = nullptr, so the call is compiled in and never taken; whoever switches the fused form back on must first
// make this function take the layout type and use q_n / q_np, as stat_final_kernel does.
template <class T, int PENDING>
__device__ __forceinline__ void stat_last_block(const float* statpart, float* stats, int* cnt, const ColLayout& L, const TileSeg& ts, int rt,
                                                void* smem_v) {
    constexpr int BM = T::BM, PARTS = T::THREADS / BM;
    static_assert(T::THREADS % BM == 0 && 512 / BM <= STATCNT_PER_SEG, "row tile / counter layout");
    double* red = reinterpret_cast<double*>(smem_v);   // [2][PARTS][BM]
    int* flag = reinterpret_cast<int*>(red + 2 * PARTS * BM);
    const int tid = threadIdx.x;
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PENDING) : "memory");   // this wave's partial stores (and everything before them) have been acknowledged
    __syncthreads();                                                  // ... every wave's; nobody still uses the staged tile in LDS
    if (tid == 0) {
        const int nwg = (ts.side ? L.n2p : L.n1p) / T::BN;
        const int old = __hip_atomic_fetch_add(cnt + ts.seg * STATCNT_PER_SEG + rt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = old == nwg - 1;
    }
    __syncthreads();
    if (!*flag) return;   // block-uniform
    const int row = tid % BM, part = tid / BM;
    const int t0 = (ts.frame * L.np + (ts.side ? L.n1p : 0)) / MLP0_BN;
    const int nt = (ts.side ? L.n2p : L.n1p) / MLP0_BN;
    const int n = ts.side ? L.n2 : L.n1;
    const int per = (nt + PARTS - 1) / PARTS;
    const int tb = part * per, te = min(nt, tb + per);
    const int ch = rt * BM + row;
    double S = 0.0, QP = 0.0;
    constexpr int CH = 32;   // tiles per round trip: this workgroup is the last one running in its group, so latency is all that counts
    for (int tt = tb; tt < te; tt += CH) {   // 2 x 32 loads in flight at a time on clamped addresses
        float xs[CH], xm[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const size_t tile = (size_t)(t0 + min(tt + u, nt - 1));
            xs[u] = __hip_atomic_load(statpart + (tile * 2 + 0) * 512 + ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            xm[u] = __hip_atomic_load(statpart + (tile * 2 + 1) * 512 + ch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int t = tt + u;
            const int nv = min(MLP0_BN, n - t * MLP0_BN);   // real columns of tile t of this segment (<= 0: pad-only tile)
            if (t < te && nv > 0) {
                const double st = (double)xs[u], mt = (double)xm[u];
                const double inv = nv == MLP0_BN ? 1.0 / MLP0_BN : 1.0 / nv;
                S += st;
                QP += mt + st * st * inv;
            }
        }
    }
    red[(0 * PARTS + part) * BM + row] = S;
    red[(1 * PARTS + part) * BM + row] = QP;
    __syncthreads();
    if (part == 0) {
        S = red[row];
        QP = red[PARTS * BM + row];
#pragma unroll
        for (int p = 1; p < PARTS; ++p) {
            S += red[p * BM + row];
            QP += red[(PARTS + p) * BM + row];
        }
        const double mean = S / n;
        double var = (QP - S * mean) / n;
        if (var < 0.0) var = 0.0;
        stats[((size_t)ts.seg * 2 + 0) * 512 + ch] = (float)mean;
        stats[((size_t)ts.seg * 2 + 1) * 512 + ch] = (float)(1.0 / sqrt(var + 1e-5));
    }
    if (tid == 0) __hip_atomic_store(cnt + ts.seg * STATCNT_PER_SEG + rt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------------------
// mlp.0's per-tile InstanceNorm partials from the staged output tile Tl [BM][TS] (mlp0_kernel: TS = BN + 1; mlp0_sp_kernel: TS = BN + 4
// with SKEW).
// ---------------------------------------------------------------------------------------------------------------------
// Per-row (sum, centred sum of squares) of the real columns of each 64-column tile: THREADS / BM lanes per row, each a fixed contiguous
// column range, combined by shuffles (fixed order).  One pass, shifted by the first column of the row (a pivot within a few std of the
// mean), so M2 = sum d^2 - (sum d)^2 / n does not cancel even when |mean| >> std; stat_final merges the tiles with Chan's formula.
// SKEW (TS = BN + 4): the LPR lanes of a row start a multiple of 32 banks apart and rows are 4 banks apart: lane (row, q) starts its walk
// q + LPR * ((row >> 3) mod (4 / LPR)) columns into its range, so that the 32 lanes of a read (32 / LPR rows) cover the 32 banks once.
template <class T, int TS, bool SKEW>
__device__ __forceinline__ void mlp0_tile_statistics(const float* Tl, float* statpart, int valid_cols, int rt, int ct) {
    constexpr int TPW = T::BN / MLP0_BN;       // 64-column tiles (= InstanceNorm partials) per workgroup
    constexpr int LPR = T::THREADS / T::BM;    // lanes per row
    constexpr int LPS = LPR / TPW;             // lanes per (row, 64-column tile)
    constexpr int CPL = MLP0_BN / LPS;         // columns per lane
    static_assert(LPS >= 1, "at least one lane per row and 64-column tile");
    static_assert(!SKEW || (TS % 32 == 4 && CPL == 32 && (LPR == 4 || LPR == 2)), "walk skew of the statistics reads");
    const int tid = threadIdx.x;
    const int row = tid / LPR, q = tid % LPR, sub = q / LPS, part = q % LPS;
    const int valid = min(max(valid_cols - sub * MLP0_BN, 0), MLP0_BN);
    const float pivot = Tl[row * TS + sub * MLP0_BN];
    const float* tr = Tl + row * TS + sub * MLP0_BN + part * CPL;
    const int skew = SKEW ? q + (LPR == 2 ? 2 * ((row >> 3) & 1) : 0) : 0;
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int m0 = 0; m0 < CPL; ++m0) {
        const int m = SKEW ? (m0 + skew) % CPL : m0;
        const float t = tr[m];                                           // unconditional LDS read (a guarded one becomes a
        const float d = (part * CPL + m < valid) ? t - pivot : 0.f;      // branch + s_waitcnt per element), masked afterwards
        s1 += d;
        s2 += d * d;
    }
#pragma unroll
    for (int o = 1; o < LPS; o <<= 1) {
        s1 += __shfl_xor(s1, o);
        s2 += __shfl_xor(s2, o);
    }
    if (part == 0) {
        const float nv = (float)valid;
        const size_t t64 = (size_t)ct * TPW + sub;
        stat_partial_store(statpart + (t64 * 2 + 0) * 512 + rt * T::BM + row, nv * pivot + s1);                      // sum
        stat_partial_store(statpart + (t64 * 2 + 1) * 512 + rt * T::BM + row, nv > 0.f ? s2 - s1 * s1 / nv : 0.f);   // M2
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Epilogue of the score contraction (score_exp_kernel, score_exp_sp_kernel; GATs_SuperGlue.py:217-218):  E = exp(score(acc)) of the real
// entries of the 128 x 64 tile (0 elsewhere) -> LDS (Tl [BM][TS], free at the call) -> conf, plus the tile's row sums (over its 64 columns)
// and column sums (over its 128 rows) into the partial buffers that conf_finalize_kernel reduces in a fixed order.
//   score = acc / scale, or with PRESCALED (acc * inv) / scale: the split kernel's operands carry a power-of-two scale, inv undoes it
//   (exact).  A value functor in place of PRESCALED / inv was tried: score_exp_kernel<RAW> then takes 34 instead of 30 SGPRs.
//   RAW: the scaled scores themselves are written, no sums (max-subtracting path).
//   TS / SKEW: row stride of the staged tile and the bank skew of the row-sum walk (fp32 kernel: BN + 1, none; split kernel: BN + 4 --
//   conflict-free 16-byte row reads, see mlp0_sp_kernel -- and rows 4 banks apart, the two lanes of a row 32 banks apart).
// ---------------------------------------------------------------------------------------------------------------------
// LT: ColLayout, or FramesLayout -- conf rows and the row masks then go by the frame's own count n1 = q_n(L, frame), addresses by the capacity L.n1.
template <class T, int TS, bool SKEW, bool RAW, bool PRESCALED, class LT>
__device__ __forceinline__ void score_epilogue(const f32x16 (&acc)[T::TM][T::TN], float* Tl, float* conf, float* rowpart, float* colpart,
                                               const LT& L, int frame, int rt, int ct, int nrt, int nct, float inv, float scale) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / T::WN, wn = wave % T::WN, half = lane >> 5, l31 = lane & 31;
    float* cf = conf + (size_t)frame * L.n1 * L.n2;
    const int n1 = q_n(L, frame);
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (wm * T::TM + tm) * 32 + mfma_row(r, half);
            const int col = wn * 32 + l31;
            const int gi = rt * T::BM + row, gj = ct * T::BN + col;
            const float sc = PRESCALED ? (acc[tm][0][r] * inv) / scale : acc[tm][0][r] / scale;
            Tl[row * TS + col] = (gi < n1 && gj < L.n2) ? (RAW ? sc : expf(sc)) : 0.f;
        }
    __syncthreads();
    // the tile leaves through LDS: 16 lanes cover one 256-byte row segment (16-byte stores when the rows of conf are
    // 16-byte aligned, i.e. n2 % 4 == 0 and an aligned base; otherwise 4-byte stores, 64 lanes per row segment)
    if ((L.n2 & 3) == 0 && (reinterpret_cast<uintptr_t>(cf) & 15) == 0) {
        for (int idx = tid; idx < T::BM * (T::BN / 4); idx += T::THREADS) {
            const int row = idx / (T::BN / 4), c4 = (idx % (T::BN / 4)) * 4;
            const int gi = rt * T::BM + row, gj = ct * T::BN + c4;
            if (gi < n1 && gj < L.n2) {
                const float* t = Tl + row * TS + c4;
                vf4 v;
                if constexpr (TS % 4 == 0) v = *reinterpret_cast<const vf4*>(t);
                else v = (vf4){t[0], t[1], t[2], t[3]};
                *reinterpret_cast<vf4*>(cf + (size_t)gi * L.n2 + gj) = v;
            }
        }
    } else {
        for (int idx = tid; idx < T::BM * T::BN; idx += T::THREADS) {
            const int row = idx / T::BN, col = idx % T::BN;
            const int gi = rt * T::BM + row, gj = ct * T::BN + col;
            if (gi < n1 && gj < L.n2) cf[(size_t)gi * L.n2 + gj] = Tl[row * TS + col];
        }
    }
    if constexpr (!RAW) {
        // row sums: THREADS / BM lanes per row; column sums: THREADS / BN row groups of the rows, one thread per (group, column)
        // (conflict-free column walks); fixed order throughout
        constexpr int LPR = T::THREADS / T::BM, CPL = T::BN / LPR;
        static_assert(!SKEW || (LPR == 2 && CPL == 32 && TS % 32 == 4), "walk skew of the row sums");
        const int row = tid / LPR, hp = tid % LPR;
        const float* tr = Tl + row * TS + hp * CPL;
        const int skew = SKEW ? hp + 2 * ((row >> 3) & 1) : 0;
        float s = 0.f;
#pragma unroll 8
        for (int m = 0; m < CPL; ++m) s += tr[SKEW ? (m + skew) % CPL : m];
#pragma unroll
        for (int o = 1; o < LPR; o <<= 1) s += __shfl_xor(s, o);
        if (hp == 0 && rt * T::BM + row < L.n1p) rowpart[((size_t)frame * nct + ct) * L.n1p + rt * T::BM + row] = s;
        constexpr int NQ = T::THREADS / T::BN, RPQ = T::BM / NQ;   // NQ row groups of RPQ rows, one thread per (group, column)
        const int c = tid % T::BN, qp = tid / T::BN;
        float t = 0.f;
#pragma unroll 8
        for (int m = 0; m < RPQ; ++m) t += Tl[(qp * RPQ + m) * TS + c];
        __syncthreads();
        Tl[qp * T::BN + c] = t;   // re-use the tile head for the NQ x BN part sums
        __syncthreads();
        if (tid < T::BN) {
            float tot = 0.f;
#pragma unroll
            for (int q = 0; q < NQ; ++q) tot += Tl[q * T::BN + tid];
            colpart[((size_t)frame * nrt + rt) * L.n2p + ct * T::BN + tid] = tot;
        }
    }
}

}  // namespace gatsspg
