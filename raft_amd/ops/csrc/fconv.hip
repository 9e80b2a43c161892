// fconv: fused NHWC bf16 conv for the RAFT update loop (K4 and friends).
//
// Replaces the reference's per-iteration tensorpack Conv2D chains
// (model_utils.py:110-185) — which PyTorch/MIOpen executed as
// im2col + GEMM + transpose + bias + activation + concat kernels (~45% of
// the step, see profiles/r01_eager_bench_kernel_stats.md) — with one
// MFMA kernel per conv:
//
//   out[b,y,x,n] = act( sum_{ty,tx,c} In[b, y+ty-cy, x+tx-cx, c]
//                                     * Wp[ty*kw+tx][n][c] + bias[n] )
//
//   * In is the logical channel-concat of up to TWO NHWC tensors (h|x for
//     the GRU, cor|flo for the motion encoder) — no concat materialization;
//   * Wp is host-packed [taps][Cout][Cin] (c contiguous = the MFMA B
//     fragment order);
//   * SAME zero padding, arbitrary odd kh x kw (templated per shape);
//   * epilogue modes: plain activation / GRU z+r (sigmoid, r*h product) /
//     GRU candidate (tanh + h' = (1-z)h + z*q) — model_utils.py:138-169 /
//     plain fp32 store;
//   * the second input can be a channel slice of a wider buffer, and the
//     accumulators can start from an fp32 tensor instead of zero: the GRU
//     convs read [h | motion | flow] and start from the context channels'
//     share of the pre-activation, which is the same in every iteration
//     and computed once per pair with the fp32 store;
//   * output can be written into a channel-slice of a wider NHWC buffer
//     (n_off / out_cstride), which is how the per-iteration GRU input
//     buffer x = [ctx | motion | flow] is assembled without copies.
//
// Geometry: 256 threads = 4 waves (2m x 2n). Tile selection (all
// A/B-measured, see profiles/r01_final_optimization_pass.md): 64x128
// (big) only when the grid is large AND N >= 128 fills the tile's
// columns; otherwise 2D tiles of 4 output rows x 8 cols (TH=4 — at
// batch-1 grids per-CU concurrency beats per-wave MFMA efficiency, and
// vertical taps share the staged row slabs). K-loop: per (kernel row,
// BK=32 channel step) stage the halo'd input slab(s) and weight tiles
// (AT variant: all taps per step), one barrier pair, then
// shifted-LDS-read MFMA groups; stride-2 stages even/odd input columns as
// parity slabs. Interior tiles take unguarded staging fast paths (per-
// element guarded loads serialize — guide §5 trap 4c). Small-Cin shapes
// bypass this kernel entirely: 7x7-S2 stems and the 7x7/C=2 convf1 run
// as im2col-in-LDS MFMA GEMMs with K = taps*C (one barrier per block).
// Every structural choice here is A/B-measured: see tools/bench_fconv.py
// and profiles/; losers stay selectable via the RAFT_AMD_* switches
// documented in ARCHITECTURE.md. Which kernel a shape gets is decided by
// fconv_pick() in fconv_dispatch.h (plain host C++, characterised by
// tests/test_fconv_dispatch.py); the launcher below maps that pick onto
// the instantiations and refuses a shape that has none.

#include "common.h"
#include "fconv_dispatch.h"
#include <hip/hip_bf16.h>
#include <cstdio>

typedef short short8 __attribute__((ext_vector_type(8)));
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));

#define FC_BM 64
#define FC_BN 128
#define FC_BK 32
#define FC_ROWB (FC_BK * 2)   // 64 B rows, swizzled (no pad)

// Grouping-independent XOR swizzle: for any 16 rows at a fixed 16-B column
// the swizzled addresses hit 16 DISTINCT bank slots (bits 4-7 of the
// address enumerate (row&3, (row&3)^((row>>2)&3)) — a bijection), so
// ds_read_b128 is conflict-free regardless of how the HW partitions the 64
// lanes into service groups. PMC showed ~1100 conflict-cycles/wave with a
// +16B-pad scheme whose residue argument assumed contiguous lane groups.
// Bijective per 1-KiB window: bits 4-5 ^= row&3, bits 6-7 ^= (row>>2)&3.
RAFT_DEV unsigned fswz(int row, unsigned colbyte) {
    return (unsigned)(row * FC_ROWB + colbyte) ^
           (((unsigned)row & 3u) << 4) ^ ((((unsigned)row >> 2) & 3u) << 6);
}

// epilogue modes
#define EP_PLAIN 0
#define EP_GRU_ZR 1   // N = 2*hd: [z | r] -> z_buf = sig(z), rh = sig(r)*h
#define EP_GRU_Q 2    // N = hd: h' = (1-z)*h + z*tanh(q)
#define EP_RES_RELU 3 // out = relu(res + relu(v)) — residual blocks
                      // (res tensor passed via the h_state slot)
#define EP_PLAIN_F32 4 // out is float*: v stored unrounded, no activation
                       // (the GRU convs' hoisted context term, see `pre`)

// MI/NJ: per-wave 16x16 fragment repeats; tile = (32*MI) x (32*NJ*2)
// with the fixed 2x2 wave layout. (2,4) = 64x128 (compute-efficient);
// (1,2) = 32x64 (4x the workgroups — batch-1 grids on 256 CUs).
// AT (all-taps staging): stage every kernel-row slab and every tap's
// weight tile per K-step, so each barrier pair covers KH*KW MFMA groups
// instead of KW — trades LDS (occupancy) for barrier amortization; only
// meaningful for KH > 1 (the 5x1 GRU conv had 2 MFMA per barrier).
// MT: m-tiles per block — each block computes MT consecutive 32*MI-wide
// position tiles, re-using every staged weight tile MT times (the weight
// slice is re-staged once per BLOCK per K-step; at batch-1 grids the
// m-tile count is what multiplies that traffic).
// S: convolution stride (1 or 2). Stride-2 stages each kernel-row slab as
// TWO parity sub-slabs (even/odd input columns), so tap reads stay
// consecutive-row (conflict-free swizzle) — input cols 2m+tx map to
// parity (tx-PB)&1, row offset (tx-PB)>>1. Requires even input dims
// (TF-SAME pad (K-2)/2 begin — Conv2dTF semantics for even inputs).
// TH: output rows per tile (2 = 2 rows x 16 cols instead of 1 x 32, AT
// and MI=1 only): vertical taps then SHARE staged row slabs — a 5x1 conv
// stages KH+1=6 slabs of 16 positions per 32 outputs instead of 5 slabs
// of 32 (1.7x less A staging), a 3x3 stages 4x18 instead of 3x34.
// PIPE: software-pipelined k-loop (round 2, r1 verdict lever #2). The
// single-buffered loop exposes the full global-load latency every k-step:
// stage -> barrier -> tiny MFMA burst -> barrier, ~500 ns/step serialized
// at 4-7 blocks/CU (loop convs measured 20-26 us vs a 2-4 us MFMA floor).
// PIPE prefetches k-step s+1 into REGISTERS right after the store barrier,
// so the loads' latency overlaps the step-s MFMA burst plus the next
// leading barrier, without the LDS double-buffer that halved occupancy
// (measured worse in r1). Register cost is tiny at the TH4 tiles
// (RA+RB <= 6 dwordx4 = 24 VGPRs).
template <int KH, int KW, int MI, int NJ, bool AT, int MT, int S, int TH = 1,
          bool PIPE = false>
__global__ __launch_bounds__(256) void fconv_nhwc_bf16_k(
    const __hip_bfloat16* __restrict__ in1, int C1,
    int in1_stride, int in1_off,                      // strided slice of in1
    const __hip_bfloat16* __restrict__ in2, int C2,   // may be null/0
    int in2_stride,       // in2 = first channel of a slice of such rows
    const __hip_bfloat16* __restrict__ wp,            // [KH*KW][N][C1+C2]
    const float* __restrict__ bias,                   // [N] or null
    __hip_bfloat16* __restrict__ out,                 // NHWC slice target
    int H, int W, int N, int n_off, int out_cstride, int act, int mode,
    int pre_stride,                                   // see pre
    const __hip_bfloat16* __restrict__ h_state,       // [B,H,W,hd] (GRU)
    // [B,H,W,hd] z gate: written by EP_GRU_ZR, read by EP_GRU_Q. One
    // slot for both keeps the explicit arguments within 128 bytes.
    __hip_bfloat16* __restrict__ z_buf,
    __hip_bfloat16* __restrict__ rh_out,              // [B,H,W,hd] (EP_GRU_ZR)
    // fp32 per-position term the accumulators start from,
    // pre[p * pre_stride + n] (a channel slice of rows of pre_stride
    // floats, pre at its first channel): for the GRU convs the part of
    // the conv over input channels that stay the same in every iteration,
    // computed once (EP_PLAIN_F32, bias folded in). Null: none.
    const float* __restrict__ pre) {
    constexpr int TAPS = KH * KW;
    constexpr int BM = 32 * MI;          // block output positions
    constexpr int BN = 32 * NJ;          // block output channels
    constexpr int PAR = (S == 2) ? 2 : 1;          // parity slabs
    constexpr int PBW = (S == 2) ? (KW - 2) / 2 : KW / 2;  // left pad
    constexpr int PBH = (S == 2) ? (KH - 2) / 2 : KH / 2;
    constexpr int RLO = (S == 2) ? (PBW + 1) / 2 : 0;
    constexpr int BMX = BM / TH;         // x extent of the position tile
    constexpr int AW = (S == 2) ? (BM + RLO + (KW + 1) / 2 + 1)
                                : (BMX + KW - 1);  // slab rows (+halo)
    constexpr int APAD = ((AW + 15) / 16) * 16;  // swizzle window rounding
    constexpr int NSLAB = ((AT ? KH : 1) + TH - 1) * MT * PAR;
    constexpr int NBT = AT ? TAPS : KW;
    constexpr int ABYTES = APAD * FC_ROWB;
    constexpr int BBYTES = BN * FC_ROWB;
    // single-buffered LDS: a 2-phase double buffer was measured SLOWER here
    // (it halves blocks/CU at these batch-1 grids; occupancy is the
    // latency-hiding lever, not intra-block pipelining)
    __shared__ char smem[NSLAB * ABYTES + NBT * BBYTES];

    const int Cin = C1 + C2;
    const int b = blockIdx.z;
    const int tiles_per_row = (W + MT * BMX - 1) / (MT * BMX);
    const int y = TH * (blockIdx.y / tiles_per_row);
    const int x0 = (blockIdx.y % tiles_per_row) * (MT * BMX);
    const int n0 = blockIdx.x * BN;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = (wave >> 1) * (16 * MI);
    const int wn = (wave & 1) * (16 * NJ);
    const long long HW = (long long)H * W;
    const int ksteps = (Cin + FC_BK - 1) / FC_BK;
    const int nsteps = AT ? ksteps : KH * ksteps;

    floatx4 acc[MT][MI][NJ];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[mt][i][j] = {0.f, 0.f, 0.f, 0.f};
    // a hoisted term: the accumulators start from it, so the loads'
    // latency hides under the k-loop (same indexing as the epilogue;
    // adding it there instead measured 0.16 ms/step slower on the headline
    // config — profiles/gru_hoist.md). Block-uniform branch.
    if (pre) {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = wm + i * 16 + (lane >> 4) * 4 + r;
                        const int n = n0 + wn + j * 16 + (lane & 15);
                        const int yy2 = y + m / BMX;
                        const int x = x0 + mt * BMX + m % BMX;
                        if (x < W && n < N && yy2 < H)
                            acc[mt][i][j][r] = pre[
                                (((long long)b * H + yy2) * W + x) *
                                pre_stride + n];
                    }
    }

    char* const sAbase = smem;
    char* const sBbase = smem + NSLAB * ABYTES;

    // stage step s into LDS. !AT: s = ty * ksteps + kstep (one row slab +
    // KW weight tiles). AT: s = kstep (KH row slabs + TAPS weight tiles).
    auto stage = [&](int s) {
        const int ty0 = AT ? 0 : s / ksteps;
        const int k0 = (AT ? s : (s - ty0 * ksteps)) * FC_BK;
        // ---- A slabs: NSLAB (= rows x m-tiles x parity) x AW x FC_BK ch
        const int Hi = (S == 2) ? 2 * H : H;     // input dims (even for S2)
        const int Wi = (S == 2) ? 2 * W : W;
        // interior fast path (guide trap 4c: per-element guarded loads
        // serialize — hipcc branches around each load and waits vmcnt(0)):
        // all rows/cols in bounds AND this k-chunk entirely in one tensor.
        const bool a_one = (k0 + FC_BK <= C1) || (k0 >= C1);
        const bool a_rows =
            (S == 1) && (y - KH / 2 + (AT ? 0 : ty0) >= 0) &&
            (y + (AT ? KH - 1 : ty0) + TH - 1 - KH / 2 < H);
        const bool a_cols = (x0 - KW / 2 + (MT - 1) * 0 >= 0) &&
                            (x0 + MT * BMX - 1 + (KW - 1) / 2 < W);
        if (a_one && a_rows && a_cols && S == 1) {
            const bool use1 = k0 + FC_BK <= C1;
            const __hip_bfloat16* src = use1 ? in1 : in2;
            const int cs = use1 ? in1_stride : in2_stride;
            const int co = use1 ? (in1_off + k0) : (k0 - C1);
            for (int e = tid; e < NSLAB * AW * (FC_BK / 8); e += 256) {
                const int sl = e / (AW * (FC_BK / 8));
                const int rem0 = e % (AW * (FC_BK / 8));
                const int ar = rem0 / (FC_BK / 8);
                const int c8 = (rem0 % (FC_BK / 8)) * 8;
                const int mt = (sl / PAR) % MT;
                const int rsl = sl / (PAR * MT);
                const int row = y + (ty0 + rsl) - PBH;
                const int x = x0 + mt * BMX + ar - PBW;
                const uint4v v = *(const uint4v*)(
                    src + (((long long)b * H + row) * W + x) * cs + co + c8);
                *(uint4v*)(sAbase + sl * ABYTES + fswz(ar, c8 * 2)) = v;
            }
        } else
        for (int e = tid; e < NSLAB * AW * (FC_BK / 8); e += 256) {
            const int sl = e / (AW * (FC_BK / 8));
            const int rem0 = e % (AW * (FC_BK / 8));
            const int ar = rem0 / (FC_BK / 8);
            const int c8 = (rem0 % (FC_BK / 8)) * 8;
            char* sA = sAbase + sl * ABYTES;
            const int par = sl % PAR;
            const int mt = (sl / PAR) % MT;      // m-tile index
            const int rsl = sl / (PAR * MT);     // kernel-row slab index
            const int row = (S == 2) ? (2 * y + (ty0 + rsl) - PBH)
                                     : (y + (ty0 + rsl) - PBH);
            const bool row_ok = (row >= 0 && row < Hi);
            const int x = (S == 2)
                ? (2 * (x0 + mt * BMX + ar - RLO) + par)
                : (x0 + mt * BMX + ar - PBW);
            uint4v v = {0, 0, 0, 0};
            if (row_ok && x >= 0 && x < Wi) {
                const int k = k0 + c8;
                const long long p = ((long long)b * Hi + row) * Wi + x;
                if (k < C1) {
                    if (k + 8 <= C1)
                        v = *(const uint4v*)(in1 + p * in1_stride + in1_off
                                             + k);
                    else {  // straddles the in1|in2 seam: scalar gather
                        __hip_bfloat16 tmp[8];
                        for (int u = 0; u < 8; ++u) {
                            const int kk = k + u;
                            tmp[u] = (kk < C1)
                                   ? in1[p * in1_stride + in1_off + kk]
                                   : (kk - C1 < C2
                                          ? in2[p * in2_stride + kk - C1]
                                          : (__hip_bfloat16)0.f);
                        }
                        v = *(const uint4v*)tmp;
                    }
                } else if (k - C1 < C2) {
                    if (k - C1 + 8 <= C2)
                        v = *(const uint4v*)(in2 + p * in2_stride
                                             + (k - C1));
                    else {
                        __hip_bfloat16 tmp[8];
                        for (int u = 0; u < 8; ++u) {
                            const int kk = k - C1 + u;
                            tmp[u] = kk < C2 ? in2[p * in2_stride + kk]
                                             : (__hip_bfloat16)0.f;
                        }
                        v = *(const uint4v*)tmp;
                    }
                }
            }
            *(uint4v*)(sA + fswz(ar, c8 * 2)) = v;
        }
        // ---- weight tiles [NBT][BN][FC_BK]. Fast path for fully
        // interior tiles (block-uniform: no per-chunk guards — they were
        // ~9 guarded chunks/thread/step in the AT 3x3 kernel)
        if (n0 + BN <= N && k0 + FC_BK <= Cin) {
            for (int e = tid; e < NBT * BN * (FC_BK / 8); e += 256) {
                const int t = e / (BN * (FC_BK / 8));
                const int rem = e % (BN * (FC_BK / 8));
                const int n = rem / (FC_BK / 8);
                const int c8 = (rem % (FC_BK / 8)) * 8;
                const int tap = AT ? t : (ty0 * KW + t);
                const uint4v v = *(const uint4v*)(
                    wp + ((size_t)tap * N + n0 + n) * Cin + k0 + c8);
                *(uint4v*)(sBbase + t * BBYTES + fswz(n, c8 * 2)) = v;
            }
        } else {
            for (int e = tid; e < NBT * BN * (FC_BK / 8); e += 256) {
                const int t = e / (BN * (FC_BK / 8));
                const int rem = e % (BN * (FC_BK / 8));
                const int n = rem / (FC_BK / 8);
                const int c8 = (rem % (FC_BK / 8)) * 8;
                uint4v v = {0, 0, 0, 0};
                const int gn = n0 + n;
                const int k = k0 + c8;
                const int tap = AT ? t : (ty0 * KW + t);
                if (gn < N && k + 8 <= Cin)
                    v = *(const uint4v*)(
                        wp + ((size_t)tap * N + gn) * Cin + k);
                else if (gn < N) {
                    __hip_bfloat16 tmp[8];
                    for (int u = 0; u < 8; ++u)
                        tmp[u] = (k + u < Cin)
                            ? wp[((size_t)tap * N + gn) * Cin + k + u]
                            : (__hip_bfloat16)0.f;
                    v = *(const uint4v*)tmp;
                }
                *(uint4v*)(sBbase + t * BBYTES + fswz(n, c8 * 2)) = v;
            }
        }
    };

    auto do_mfma = [&]() {
        const unsigned cb = (lane >> 4) * 16;
#pragma unroll
        for (int rsl = 0; rsl < (AT ? KH : 1); ++rsl) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
                for (int tx = 0; tx < KW; ++tx) {
                    const int d = tx - PBW;
                    const int par = (S == 2) ? (d & 1) : 0;
                    const int roff = (S == 2) ? ((d >> 1) + RLO) : (d + PBW);
                    short8 af[MI], bf[NJ];
#pragma unroll
                    for (int i = 0; i < MI; ++i) {
                        // per-lane slab row: the fragment's 16 m-positions
                        // may span TH output rows (TH=4: 2 rows per wave)
                        const int m_af = wm + i * 16 + (lane & 15);
                        const int rslot = rsl + m_af / BMX;
                        const char* sA = sAbase +
                            ((rslot * MT + mt) * PAR + par) * ABYTES;
                        af[i] = *(const short8*)(
                            sA + fswz(m_af % BMX + roff, cb));
                    }
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        bf[j] = *(const short8*)(
                            sBbase + (rsl * KW + tx) * BBYTES +
                            fswz(wn + j * 16 + (lane & 15), cb));
#pragma unroll
                    for (int i = 0; i < MI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ; ++j)
                            acc[mt][i][j] =
                                __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                                    af[i], bf[j], acc[mt][i][j], 0, 0, 0);
                }
            }
        }
    };

    if constexpr (!PIPE) {
        for (int s = 0; s < nsteps; ++s) {
            stage(s);
            __syncthreads();
            do_mfma();
            __syncthreads();
        }
    } else {
        // register-prefetch pipeline: loads for step s+1 issue before the
        // MFMA burst of step s, so their latency hides behind compute +
        // the next leading barrier instead of being serially exposed.
        constexpr int TOTA = NSLAB * AW * (FC_BK / 8);
        constexpr int TOTB = NBT * BN * (FC_BK / 8);
        constexpr int RA = (TOTA + 255) / 256;
        constexpr int RB = (TOTB + 255) / 256;
        uint4v ra[RA], rb[RB];

        auto loadA = [&](int s, uint4v* rg) {
            const int ty0 = AT ? 0 : s / ksteps;
            const int k0 = (AT ? s : (s - ty0 * ksteps)) * FC_BK;
            const int Hi = (S == 2) ? 2 * H : H;
            const int Wi = (S == 2) ? 2 * W : W;
            const bool a_one = (k0 + FC_BK <= C1) || (k0 >= C1);
            const bool a_rows =
                (S == 1) && (y - KH / 2 + (AT ? 0 : ty0) >= 0) &&
                (y + (AT ? KH - 1 : ty0) + TH - 1 - KH / 2 < H);
            const bool a_cols = (x0 - KW / 2 >= 0) &&
                                (x0 + MT * BMX - 1 + (KW - 1) / 2 < W);
            if (S == 1 && a_one && a_rows && a_cols) {
                const bool use1 = k0 + FC_BK <= C1;
                const __hip_bfloat16* src = use1 ? in1 : in2;
                const int cs = use1 ? in1_stride : in2_stride;
                const int co = use1 ? (in1_off + k0) : (k0 - C1);
#pragma unroll
                for (int r = 0; r < RA; ++r) {
                    const int e = tid + r * 256;
                    if (e < TOTA) {
                        const int sl = e / (AW * (FC_BK / 8));
                        const int rem0 = e % (AW * (FC_BK / 8));
                        const int ar = rem0 / (FC_BK / 8);
                        const int c8 = (rem0 % (FC_BK / 8)) * 8;
                        const int mt = (sl / PAR) % MT;
                        const int rsl = sl / (PAR * MT);
                        const int row = y + (ty0 + rsl) - PBH;
                        const int x = x0 + mt * BMX + ar - PBW;
                        rg[r] = *(const uint4v*)(
                            src + (((long long)b * H + row) * W + x) * cs +
                            co + c8);
                    }
                }
                return;
            }
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const int e = tid + r * 256;
                uint4v v = {0, 0, 0, 0};
                if (e < TOTA) {
                    const int sl = e / (AW * (FC_BK / 8));
                    const int rem0 = e % (AW * (FC_BK / 8));
                    const int ar = rem0 / (FC_BK / 8);
                    const int c8 = (rem0 % (FC_BK / 8)) * 8;
                    const int par = sl % PAR;
                    const int mt = (sl / PAR) % MT;
                    const int rsl = sl / (PAR * MT);
                    const int row = (S == 2) ? (2 * y + (ty0 + rsl) - PBH)
                                             : (y + (ty0 + rsl) - PBH);
                    const bool row_ok = (row >= 0 && row < Hi);
                    const int x = (S == 2)
                        ? (2 * (x0 + mt * BMX + ar - RLO) + par)
                        : (x0 + mt * BMX + ar - PBW);
                    if (row_ok && x >= 0 && x < Wi) {
                        const int k = k0 + c8;
                        const long long p = ((long long)b * Hi + row) * Wi + x;
                        if (k < C1) {
                            if (k + 8 <= C1)
                                v = *(const uint4v*)(
                                    in1 + p * in1_stride + in1_off + k);
                            else {
                                __hip_bfloat16 tmp[8];
                                for (int u = 0; u < 8; ++u) {
                                    const int kk = k + u;
                                    tmp[u] = (kk < C1)
                                        ? in1[p * in1_stride + in1_off + kk]
                                        : (kk - C1 < C2
                                               ? in2[p * in2_stride + kk - C1]
                                               : (__hip_bfloat16)0.f);
                                }
                                v = *(const uint4v*)tmp;
                            }
                        } else if (k - C1 < C2) {
                            if (k - C1 + 8 <= C2)
                                v = *(const uint4v*)(
                                    in2 + p * in2_stride + (k - C1));
                            else {
                                __hip_bfloat16 tmp[8];
                                for (int u = 0; u < 8; ++u) {
                                    const int kk = k - C1 + u;
                                    tmp[u] = kk < C2
                                        ? in2[p * in2_stride + kk]
                                        : (__hip_bfloat16)0.f;
                                }
                                v = *(const uint4v*)tmp;
                            }
                        }
                    }
                }
                rg[r] = v;
            }
        };

        auto loadB = [&](int s, uint4v* rg) {
            const int ty0 = AT ? 0 : s / ksteps;
            const int k0 = (AT ? s : (s - ty0 * ksteps)) * FC_BK;
            if (n0 + BN <= N && k0 + FC_BK <= Cin) {
#pragma unroll
                for (int r = 0; r < RB; ++r) {
                    const int e = tid + r * 256;
                    if (e < TOTB) {
                        const int t = e / (BN * (FC_BK / 8));
                        const int rem = e % (BN * (FC_BK / 8));
                        const int n = rem / (FC_BK / 8);
                        const int c8 = (rem % (FC_BK / 8)) * 8;
                        const int tap = AT ? t : (ty0 * KW + t);
                        rg[r] = *(const uint4v*)(
                            wp + ((size_t)tap * N + n0 + n) * Cin + k0 + c8);
                    }
                }
                return;
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int e = tid + r * 256;
                uint4v v = {0, 0, 0, 0};
                if (e < TOTB) {
                    const int t = e / (BN * (FC_BK / 8));
                    const int rem = e % (BN * (FC_BK / 8));
                    const int n = rem / (FC_BK / 8);
                    const int c8 = (rem % (FC_BK / 8)) * 8;
                    const int gn = n0 + n;
                    const int k = k0 + c8;
                    const int tap = AT ? t : (ty0 * KW + t);
                    if (gn < N && k + 8 <= Cin)
                        v = *(const uint4v*)(
                            wp + ((size_t)tap * N + gn) * Cin + k);
                    else if (gn < N) {
                        __hip_bfloat16 tmp[8];
                        for (int u = 0; u < 8; ++u)
                            tmp[u] = (k + u < Cin)
                                ? wp[((size_t)tap * N + gn) * Cin + k + u]
                                : (__hip_bfloat16)0.f;
                        v = *(const uint4v*)tmp;
                    }
                }
                rg[r] = v;
            }
        };

        auto store_regs = [&]() {
#pragma unroll
            for (int r = 0; r < RA; ++r) {
                const int e = tid + r * 256;
                if (e < TOTA) {
                    const int sl = e / (AW * (FC_BK / 8));
                    const int rem0 = e % (AW * (FC_BK / 8));
                    const int ar = rem0 / (FC_BK / 8);
                    const int c8 = (rem0 % (FC_BK / 8)) * 8;
                    *(uint4v*)(sAbase + sl * ABYTES + fswz(ar, c8 * 2)) =
                        ra[r];
                }
            }
#pragma unroll
            for (int r = 0; r < RB; ++r) {
                const int e = tid + r * 256;
                if (e < TOTB) {
                    const int t = e / (BN * (FC_BK / 8));
                    const int rem = e % (BN * (FC_BK / 8));
                    const int n = rem / (FC_BK / 8);
                    const int c8 = (rem % (FC_BK / 8)) * 8;
                    *(uint4v*)(sBbase + t * BBYTES + fswz(n, c8 * 2)) = rb[r];
                }
            }
        };

        loadA(0, ra);
        loadB(0, rb);
        for (int s = 0; s < nsteps; ++s) {
            if (s) __syncthreads();
            store_regs();
            __syncthreads();
            if (s + 1 < nsteps) {
                loadA(s + 1, ra);
                loadB(s + 1, rb);
            }
            do_mfma();
        }
    }

    // ------------------------------------------------------------- epilogue
    const int hd = (mode == EP_GRU_ZR) ? N / 2 : N;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = wm + i * 16 + (lane >> 4) * 4 + r;
                const int n = n0 + wn + j * 16 + (lane & 15);
                const int yy2 = y + m / BMX;
                const int x = x0 + mt * BMX + m % BMX;
                if (x >= W || n >= N || yy2 >= H) continue;
                const long long p = ((long long)b * H + yy2) * W + x;
                float v = acc[mt][i][j][r];
                if (bias) v += bias[n];
                if (mode == EP_PLAIN) {
                    out[p * out_cstride + n_off + n] =
                        (__hip_bfloat16)factivate(v, act);
                } else if (mode == EP_RES_RELU) {
                    const float res = (float)h_state[p * hd + n];
                    out[p * out_cstride + n_off + n] = (__hip_bfloat16)
                        fmaxf(res + fmaxf(v, 0.0f), 0.0f);
                } else if (mode == EP_PLAIN_F32) {
                    ((float*)out)[p * out_cstride + n_off + n] = v;
                } else if (mode == EP_GRU_ZR) {
                    const float s = 1.0f / (1.0f + __expf(-v));
                    if (n < hd) {
                        z_buf[p * hd + n] = (__hip_bfloat16)s;
                    } else {
                        const int c = n - hd;
                        rh_out[p * hd + c] = (__hip_bfloat16)(
                            s * (float)h_state[p * hd + c]);
                    }
                } else {  // EP_GRU_Q
                    const float q = tanhf(v);
                    const float z = (float)z_buf[p * hd + n];
                    const float h = (float)h_state[p * hd + n];
                    out[p * out_cstride + n_off + n] =
                        (__hip_bfloat16)((1.0f - z) * h + z * q);
                }
            }
}


// ------------------------------------------------------ stem conv (S2, C=8)
// The encoder stems are 7x7 stride-2 over the 8-channel zero-padded image
// (x8 buffer): the generic S2 path stages FC_BK=32-channel K-steps of
// which only 8 carry data (measured 223 us/call after the small-tile
// switch, 369 before). This kernel im2cols in LDS with K = taps*8: an
// MFMA k-group's 8 contiguous k ARE one tap's 8 channels, so the whole
// 7-row input tile (all taps) plus the full [52][32][8] weight tile fit
// LDS -> ONE barrier, then 13 straight mfma_16x16x32 per wave.
extern "C" __global__ __launch_bounds__(256) void fconv_stem_s2_k(
    const __hip_bfloat16* __restrict__ in,   // [B, 2H, 2W, 8]
    const __hip_bfloat16* __restrict__ wp,   // [49][N][8]
    const float* __restrict__ bias,          // [N] or null
    __hip_bfloat16* __restrict__ out,        // [B, H, W, N]
    int H, int W, int N, int act) {
    constexpr int KT = 49, KTP = 52;         // taps; padded to 13 k-chunks
    constexpr int AROW = 72;                 // 69 staged input cols, padded
    __shared__ __hip_bfloat16 sa[7 * AROW * 8];
    __shared__ __hip_bfloat16 sb[KTP * 32 * 8];
    const int b = blockIdx.z;
    const int tiles = (W + 31) >> 5;
    const int y = blockIdx.y / tiles;
    const int x0 = (blockIdx.y % tiles) << 5;
    const int n0 = blockIdx.x * 32;
    const int tid = threadIdx.x;
    const int Hi = 2 * H, Wi = 2 * W;
    // A: rows 2y-2..2y+4, cols 2x0-2..2x0+66 (Conv2dTF even-input SAME:
    // pad_beg = (7-2)/2 = 2), 8 ch = one 16-byte load per pixel
    for (int e = tid; e < 7 * 69; e += 256) {
        const int r = e / 69, c = e % 69;
        const int yy = 2 * y + r - 2;
        const int xx = 2 * x0 + c - 2;
        uint4v v = {0, 0, 0, 0};
        if (yy >= 0 && yy < Hi && xx >= 0 && xx < Wi)
            v = *(const uint4v*)(
                in + (((long long)b * Hi + yy) * Wi + xx) * 8);
        *(uint4v*)(sa + ((size_t)r * AROW + c) * 8) = v;
    }
    // B: [52][32][8]; taps >= 49 and n >= N are zero (pad chunks vanish)
    for (int e = tid; e < KTP * 32; e += 256) {
        const int t = e / 32, n = e % 32;
        uint4v v = {0, 0, 0, 0};
        if (t < KT && n0 + n < N)
            v = *(const uint4v*)(wp + ((size_t)t * N + n0 + n) * 8);
        *(uint4v*)(sb + (size_t)e * 8) = v;
    }
    __syncthreads();
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = (wave >> 1) * 16;
    const int wn = (wave & 1) * 16;
    const int kg = lane >> 4;
    const int m_af = wm + (lane & 15);
    const int n_bf = wn + (lane & 15);
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < 13; ++kc) {
        const int t = kc * 4 + kg;
        const int tc = t < KT ? t : KT - 1;   // pad taps: B is zero there,
        const int dy = tc / 7, dx = tc % 7;   // clamp A address in-bounds
        const short8 af = *(const short8*)(
            sa + ((size_t)dy * AROW + 2 * m_af + dx) * 8);
        const short8 bf = *(const short8*)(sb + ((size_t)t * 32 + n_bf) * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int mm = wm + (lane >> 4) * 4 + r;
        const int nn = n0 + wn + (lane & 15);
        const int x = x0 + mm;
        if (x >= W || nn >= N) continue;
        float v = acc[r];
        if (bias) v += bias[nn];
        out[(((long long)b * H + y) * W + x) * N + nn] =
            (__hip_bfloat16)factivate(v, act);
    }
}

// ----------------------------------------------------------- tiny-N conv
// N <= 4 (the flow head's final 3x3 -> 2): an MFMA tile wastes 97% of its
// columns. One wave per position: lanes stride over K = taps*Cin with N
// accumulators each, then a cross-lane tree reduce per n.
template <int NN>
__global__ __launch_bounds__(256) void fconv_tinyn_k(
    const __hip_bfloat16* __restrict__ in,    // [B,H,W,Cin] (full rows)
    int Cin, int in_stride, int in_off,
    const __hip_bfloat16* __restrict__ wp,    // [taps][N][Cin]
    const float* __restrict__ bias,
    __hip_bfloat16* __restrict__ out,         // [B,H,W,N] (null if coords)
    const float* __restrict__ coords_in,      // fused coords1 += dflow
    float* __restrict__ coords_out,           // (NN == 2 only)
    // with coords_out: also flow = coords_out - pixel grid as bf16 into a
    // channel slice of rows of flow_stride elements (the GRU input
    // buffer's flow channels, as the lookup kernel writes them). Null: off.
    __hip_bfloat16* __restrict__ flow_out, int flow_stride, int flow_off,
    int H, int W, int kh, int kw, int act, long long ncells) {
    const int lane = threadIdx.x & 63;
    const long long cell = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cell >= ncells) return;
    const int x = (int)(cell % W);
    const int y = (int)((cell / W) % H);
    const int b = (int)(cell / ((long long)W * H));
    const int taps = kh * kw;

    float acc[NN];
#pragma unroll
    for (int n = 0; n < NN; ++n) acc[n] = 0.0f;

    // tap-outer, channel-inner: one bounds check per tap, lane-contiguous
    // (coalesced) channel loads
    for (int t = 0; t < taps; ++t) {
        const int yy = y + t / kw - kh / 2;
        const int xx = x + t % kw - kw / 2;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        const __hip_bfloat16* src =
            in + (((long long)b * H + yy) * W + xx) * in_stride + in_off;
        const __hip_bfloat16* wr = wp + (size_t)t * NN * Cin;
        for (int c = lane; c < Cin; c += 64) {
            const float v = (float)src[c];
#pragma unroll
            for (int n = 0; n < NN; ++n)
                acc[n] = fmaf(v, (float)wr[n * Cin + c], acc[n]);
        }
    }
#pragma unroll
    for (int n = 0; n < NN; ++n)
        for (int off = 32; off > 0; off >>= 1)
            acc[n] += __shfl_down(acc[n], off, 64);
    if (lane == 0) {    // tree reduce leaves each total in lane 0
#pragma unroll
        for (int n = 0; n < NN; ++n) {
            float v = acc[n] + (bias ? bias[n] : 0.0f);
            v = factivate(v, act);
            if (coords_out) {  // fused coords1 = coords1 + delta_flow
                const float c = coords_in[cell * NN + n] + v;
                coords_out[cell * NN + n] = c;
                if (flow_out) {
                    const float base = (n == 0) ? (float)x : (float)y;
                    flow_out[cell * flow_stride + flow_off + n] =
                        (__hip_bfloat16)(c - base);
                }
            } else
                out[cell * NN + n] = (__hip_bfloat16)v;
        }
    }
}



// tinyn v2: row-tile staged variant — 8 positions per block share the
// staged kh x (8+kw-1) x Cin input window and the full weight set in LDS
// (the cell-per-wave version re-read each cell's 9x256-ch window from
// global: 14.4 us/call). Each wave reduces 2 positions; lanes stride the
// channel axis (conflict-free: row stride is Cin elements).
template <int NN>
__global__ __launch_bounds__(256) void fconv_tinyn2_k(
    const __hip_bfloat16* __restrict__ in, int Cin, int in_stride,
    int in_off, const __hip_bfloat16* __restrict__ wp,
    const float* __restrict__ bias, __hip_bfloat16* __restrict__ out,
    const float* __restrict__ coords_in, float* __restrict__ coords_out,
    __hip_bfloat16* __restrict__ flow_out, int flow_stride, int flow_off,
    int H, int W, int kh, int kw, int act) {
    extern __shared__ __hip_bfloat16 sm2[];
    constexpr int TP = 8;
    const int aw = TP + kw - 1;
    __hip_bfloat16* sin = sm2;                    // [kh][aw][Cin]
    __hip_bfloat16* sw = sm2 + kh * aw * Cin;     // [taps][NN][Cin]
    const int taps = kh * kw;
    const int tid = threadIdx.x;
    const int tiles = (W + TP - 1) / TP;
    const int y = blockIdx.x / tiles;
    const int x0 = (blockIdx.x % tiles) * TP;
    const int b = blockIdx.z;
    for (int e8 = tid; e8 < taps * NN * Cin / 8; e8 += 256)
        *(uint4v*)(sw + (size_t)e8 * 8) = *(const uint4v*)(wp + (size_t)e8 * 8);
    const int c8n = Cin / 8;
    for (int e = tid; e < kh * aw * c8n; e += 256) {
        const int pix = e / c8n;
        const int c8 = (e % c8n) * 8;
        const int r = pix / aw, cx = pix % aw;
        const int yy = y + r - kh / 2;
        const int xx = x0 + cx - kw / 2;
        uint4v v = {0, 0, 0, 0};
        if (yy >= 0 && yy < H && xx >= 0 && xx < W)
            v = *(const uint4v*)(
                in + (((long long)b * H + yy) * W + xx) * in_stride
                + in_off + c8);
        *(uint4v*)(sin + (size_t)pix * Cin + c8) = v;
    }
    __syncthreads();
    const int lane = tid & 63;
    const int wave = tid >> 6;
#pragma unroll
    for (int pi = 0; pi < 2; ++pi) {
        const int p = wave * 2 + pi;
        const int x = x0 + p;
        float acc[NN];
#pragma unroll
        for (int n = 0; n < NN; ++n) acc[n] = 0.f;
        for (int t = 0; t < taps; ++t) {
            const __hip_bfloat16* win =
                sin + ((size_t)(t / kw) * aw + p + t % kw) * Cin;
            const __hip_bfloat16* wr = sw + (size_t)t * NN * Cin;
            for (int c = lane; c < Cin; c += 64) {
                const float v = (float)win[c];
#pragma unroll
                for (int n = 0; n < NN; ++n)
                    acc[n] = fmaf(v, (float)wr[n * Cin + c], acc[n]);
            }
        }
#pragma unroll
        for (int n = 0; n < NN; ++n)
            for (int off = 32; off > 0; off >>= 1)
                acc[n] += __shfl_down(acc[n], off, 64);
        if (lane == 0 && x < W) {
            const long long cell = ((long long)b * H + y) * W + x;
#pragma unroll
            for (int n = 0; n < NN; ++n) {
                float v = acc[n] + (bias ? bias[n] : 0.0f);
                v = factivate(v, act);
                if (coords_out) {
                    const float c = coords_in[cell * NN + n] + v;
                    coords_out[cell * NN + n] = c;
                    if (flow_out) {
                        const float base = (n == 0) ? (float)x : (float)y;
                        flow_out[cell * flow_stride + flow_off + n] =
                            (__hip_bfloat16)(c - base);
                    }
                } else
                    out[cell * NN + n] = (__hip_bfloat16)v;
            }
        }
    }
}

// ------------------------------------------------------------- dispatch
// fconv_pick() (fconv_dispatch.h) decides which kernel a shape gets; the
// fc_try* tables below are the one place that names the instantiations
// of fconv_nhwc_bf16_k (78 of them) and launch the one a pick selects.
static const FconvKnobs& fconv_knobs() {
    static const FconvKnobs k = fconv_knobs_from_env();  // once per process
    return k;
}

struct FconvArgs {
    const __hip_bfloat16 *in1, *in2, *wp;
    const float* bias;
    __hip_bfloat16* out;
    const __hip_bfloat16 *h_state, *z_buf_in;
    __hip_bfloat16 *z_buf_out, *rh_out;
    int act;
    hipStream_t s;
    // not part of FconvShape: none of these steers the pick. in2 and pre
    // already point at the first channel of their slice.
    int in2_stride;
    const float* pre;
    int pre_stride;
};

template <int KH, int KW, int MI, int NJ, bool AT, int MT, int S, int TH,
          bool PIPE>
static bool fc_try(const FconvPick& p, const FconvShape& sh,
                   const FconvArgs& a) {
    if (p.KH != KH || p.KW != KW || p.MI != MI || p.NJ != NJ ||
        (p.AT != 0) != AT || p.MT != MT || p.S != S || p.TH != TH ||
        (p.PIPE != 0) != PIPE)
        return false;
    unsigned g[3];
    fconv_generic_grid(p, sh, g);
    hipLaunchKernelGGL(
        (fconv_nhwc_bf16_k<KH, KW, MI, NJ, AT, MT, S, TH, PIPE>),
        dim3(g[0], g[1], g[2]), dim3(256), 0, a.s, a.in1, sh.C1,
        sh.in1_stride, sh.in1_off, a.in2, sh.C2, a.in2_stride, a.wp, a.bias,
        a.out, sh.H, sh.W, sh.N, sh.n_off, sh.out_cstride, a.act, sh.mode,
        a.pre_stride, a.h_state,
        sh.mode == EP_GRU_ZR ? a.z_buf_out
                             : const_cast<__hip_bfloat16*>(a.z_buf_in),
        a.rh_out, a.pre);
    return true;
}

// both k-loops (single-buffered / register-prefetch) of one tile shape
template <int KH, int KW, int MI, int NJ, bool AT, int MT, int S, int TH>
static bool fc_try_pp(const FconvPick& p, const FconvShape& sh,
                      const FconvArgs& a) {
    return fc_try<KH, KW, MI, NJ, AT, MT, S, TH, false>(p, sh, a) ||
           fc_try<KH, KW, MI, NJ, AT, MT, S, TH, true>(p, sh, a);
}

// stride-1 instantiations of one kernel shape
template <int KH, int KW>
static bool fc_try_s1(const FconvPick& p, const FconvShape& sh,
                      const FconvArgs& a) {
    if (p.S != 1 || p.KH != KH || p.KW != KW) return false;
    // 1-row tiles: 64x128 (big); 32x32 and 32x64 (x MT m-tiles), both
    // with and without all-taps staging, unpipelined
    if (fc_try_pp<KH, KW, 2, 4, false, 1, 1, 1>(p, sh, a) ||
        fc_try<KH, KW, 1, 1, false, 1, 1, 1, false>(p, sh, a) ||
        fc_try<KH, KW, 1, 1, true, 1, 1, 1, false>(p, sh, a) ||
        fc_try<KH, KW, 1, 2, false, 1, 1, 1, false>(p, sh, a) ||
        fc_try<KH, KW, 1, 2, false, 2, 1, 1, false>(p, sh, a) ||
        fc_try<KH, KW, 1, 2, false, 4, 1, 1, false>(p, sh, a) ||
        fc_try<KH, KW, 1, 2, true, 1, 1, 1, false>(p, sh, a) ||
        fc_try<KH, KW, 1, 2, true, 2, 1, 1, false>(p, sh, a) ||
        fc_try<KH, KW, 1, 2, true, 4, 1, 1, false>(p, sh, a))
        return true;
    // 2D tiles (all-taps, TH rows): <.., NJ, AT, MT, S, TH>
    if (fc_try_pp<KH, KW, 1, 1, true, 1, 1, 4>(p, sh, a)) return true;
    if constexpr (KW > 1 || KH > 1) {
        if (fc_try_pp<KH, KW, 1, 2, true, 1, 1, 4>(p, sh, a) ||
            fc_try_pp<KH, KW, 1, 1, true, 2, 1, 4>(p, sh, a))
            return true;
    }
    if constexpr (KH > 1) {
        if (fc_try_pp<KH, KW, 1, 1, true, 1, 1, 2>(p, sh, a) ||
            fc_try_pp<KH, KW, 1, 2, true, 1, 1, 2>(p, sh, a) ||
            fc_try_pp<KH, KW, 1, 1, true, 1, 1, 8>(p, sh, a))
            return true;
    }
    return false;
}

// stride-2 instantiations (encoder): 64x128 and 32x64, one row slab pair
template <int K>
static bool fc_try_s2(const FconvPick& p, const FconvShape& sh,
                      const FconvArgs& a) {
    return fc_try<K, K, 2, 4, false, 1, 2, 1, false>(p, sh, a) ||
           fc_try<K, K, 1, 2, false, 1, 2, 1, false>(p, sh, a);
}

extern "C" void launch_fconv_nhwc_bf16(
    const void* in1, int C1, int in1_stride, int in1_off, const void* in2,
    int C2, int in2_stride, int in2_off, const void* wp, const float* bias,
    void* out, int B, int H, int W, int N, int n_off, int out_cstride,
    int kh, int kw, int act, int mode, const void* h_state,
    const void* z_buf_in, void* z_buf_out, void* rh_out, const float* pre,
    int pre_stride, int pre_off, int alltaps, int mtiles, int stride,
    hipStream_t s) {
    // H, W are OUTPUT dims (stride 2: input = 2H x 2W). mode EP_PLAIN_F32:
    // out is a float buffer (n_off / out_cstride in floats).
    const FconvShape sh{B, H, W, N, C1, in1_stride, in1_off, C2,
                        in2 != nullptr, kh, kw, stride, mode, n_off,
                        out_cstride};
    const FconvPick p = fconv_pick(sh, alltaps, mtiles, fconv_knobs());
    // the slice offsets of in2 and pre are folded into the pointers (the
    // kernel is short of scalar registers, not of address arithmetic)
    const FconvArgs a{(const __hip_bfloat16*)in1,
                      in2 ? (const __hip_bfloat16*)in2 + in2_off : nullptr,
                      (const __hip_bfloat16*)wp, bias, (__hip_bfloat16*)out,
                      (const __hip_bfloat16*)h_state,
                      (const __hip_bfloat16*)z_buf_in,
                      (__hip_bfloat16*)z_buf_out, (__hip_bfloat16*)rh_out,
                      act, s, in2_stride, pre ? pre + pre_off : nullptr,
                      pre_stride};
    const dim3 blk(256);
    switch (p.kind) {
    case FCONV_TINYN: {
        const long long ncells = (long long)B * H * W;
        hipLaunchKernelGGL(fconv_tinyn_k<2>, dim3((unsigned)((ncells + 3) / 4)),
                           blk, 0, s, a.in1, C1, in1_stride, in1_off, a.wp,
                           bias, a.out, nullptr, nullptr, nullptr, 0, 0, H, W,
                           kh, kw, act, ncells);
        return;
    }
    case FCONV_TINYN2: {
        const int smem = (kh * (8 + kw - 1) * C1 + kh * kw * 2 * C1) * 2;
        hipLaunchKernelGGL(fconv_tinyn2_k<2>,
                           dim3((unsigned)(H * ((W + 7) / 8)), 1, (unsigned)B),
                           blk, smem, s, a.in1, C1, in1_stride, in1_off, a.wp,
                           bias, a.out, nullptr, nullptr, nullptr, 0, 0, H, W,
                           kh, kw, act);
        return;
    }
    case FCONV_STEM:
        hipLaunchKernelGGL(fconv_stem_s2_k,
                           dim3(cdiv(N, 32), H * cdiv(W, 32), B), blk, 0, s,
                           a.in1, a.wp, bias, a.out, H, W, N, act);
        return;
    case FCONV_GENERIC:
        if (fc_try_s1<1, 1>(p, sh, a) || fc_try_s1<3, 3>(p, sh, a) ||
            fc_try_s1<1, 5>(p, sh, a) || fc_try_s1<5, 1>(p, sh, a) ||
            fc_try_s2<7>(p, sh, a) || fc_try_s2<3>(p, sh, a) ||
            fc_try_s2<1>(p, sh, a))
            return;
        break;
    case FCONV_NONE:
        break;
    }
    // an unsupported shape, or a pick without an instantiation: never a
    // silent no-op (the output buffer would stay uninitialized)
    fprintf(stderr,
            "fconv: no kernel for %dx%d stride %d, N=%d (pick kind %d "
            "<%d,%d,%d,%d,%d,%d,%d,%d,%d>)\n", kh, kw, stride, N,
            (int)p.kind, p.KH, p.KW, p.MI, p.NJ, p.AT, p.MT, p.S, p.TH,
            p.PIPE);
    abort();
}

// --------------------------------------------------------- small-K direct
// Direct conv for tiny input-channel counts (the motion encoder's flow
// branch: convf1 is 7x7 over Cin=2 — model_utils.py:114). K = Cin*kh*kw is
// far below MFMA efficiency. LDS-staged form: weights staged once per
// block, PPB = 256/N positions per block share them; all-lane-uniform
// input reads broadcast from LDS.
#define SK_MAXW (49 * 128 * 4)       // taps x N x C cap (bf16)
#define SK_MAXIN (8 * 49 * 4)        // PPB x taps x C cap

extern "C" __global__ __launch_bounds__(256) void fconv_smallk_lds_k(
    const __hip_bfloat16* __restrict__ in,    // [B, Hi, Wi, *] slice
    int in_stride, int in_off,
    const __hip_bfloat16* __restrict__ wp,    // [kh*kw][N][C]
    const float* __restrict__ bias,
    __hip_bfloat16* __restrict__ out,         // [B, H, W, N] (output dims)
    int H, int W, int C, int N, int kh, int kw, int act, int cstride,
    long long ncells) {
    __shared__ __hip_bfloat16 smem[SK_MAXW + SK_MAXIN];
    __hip_bfloat16* sw = smem;
    __hip_bfloat16* sin = smem + SK_MAXW;
    const int taps = kh * kw;
    const int PPB = 256 / N;
    const int tid = threadIdx.x;
    for (int e = tid; e < taps * N * C; e += 256) sw[e] = wp[e];

    const long long groups = (ncells + PPB - 1) / PPB;
    for (long long g = blockIdx.x; g < groups; g += gridDim.x) {
        const long long cell0 = g * (long long)PPB;
        // stage PPB windows (zero-padded SAME). Interior fast path: all
        // cells of the group in-bounds with full windows and no row wrap
        // (guide trap 4c — per-element guarded loads serialize).
        const int Hi = cstride * H;
        const int Wi = cstride * W;
        const int pb = (cstride == 2) ? (kh - 2) / 2 : kh / 2;
        const int pbw = (cstride == 2) ? (kw - 2) / 2 : kw / 2;
        const int x_f = (int)(cell0 % W);
        const int y_f = (int)((cell0 / W) % H);
        const bool interior =
            (cell0 + PPB <= ncells) && (x_f + PPB <= W) &&
            (cstride * y_f - pb >= 0) &&
            (cstride * y_f + kh - 1 - pb < Hi) &&
            (cstride * x_f - pbw >= 0) &&
            (cstride * (x_f + PPB - 1) + kw - 1 - pbw < Wi);
        if (interior) {
            const int b0 = (int)(cell0 / ((long long)W * H));
            for (int e = tid; e < PPB * taps * C; e += 256) {
                const int p = e / (taps * C);
                const int rem = e % (taps * C);
                const int t = rem / C;
                const int c = rem % C;
                const int yy = cstride * y_f + t / kw - pb;
                const int xx = cstride * (x_f + p) + t % kw - pbw;
                sin[e] = in[(((long long)b0 * Hi + yy) * Wi + xx)
                            * in_stride + in_off + c];
            }
        } else
        for (int e = tid; e < PPB * taps * C; e += 256) {
            const int p = e / (taps * C);
            const int rem = e % (taps * C);
            const int t = rem / C;
            const int c = rem % C;
            const long long cell = cell0 + p;
            __hip_bfloat16 v = (__hip_bfloat16)0.f;
            if (cell < ncells) {
                const int x = (int)(cell % W);
                const int y = (int)((cell / W) % H);
                const int b = (int)(cell / ((long long)W * H));
                const int yy = cstride * y + t / kw - pb;
                const int xx = cstride * x + t % kw - pbw;
                if (yy >= 0 && yy < Hi && xx >= 0 && xx < Wi)
                    v = in[(((long long)b * Hi + yy) * Wi + xx) * in_stride
                           + in_off + c];
            }
            sin[e] = v;
        }
        __syncthreads();
        const int p = tid / N;
        const int n = tid - p * N;
        const long long cell = cell0 + p;
        if (cell < ncells) {
            float acc = bias ? bias[n] : 0.0f;
            const __hip_bfloat16* win = sin + p * taps * C;
            for (int t = 0; t < taps; ++t)
                for (int c = 0; c < C; ++c)
                    acc = fmaf((float)win[t * C + c],
                               (float)sw[(t * N + n) * C + c], acc);
            out[cell * N + n] = (__hip_bfloat16)factivate(acc, act);
        }
        __syncthreads();
    }
}


// small-C MFMA conv (stride 1): same im2col-in-LDS trick as the stem
// kernel but for the motion encoder's convf1 (7x7 over the 2-channel
// flow slice, K = taps*C = 98 -> 4 MFMA chunks). Three phases: stage the
// raw kh x (32+kw-1) x C tile + the [n][K] weight image, barrier,
// im2col-expand the 32 positions' windows into [pos][K] rows (LDS->LDS),
// barrier, then kchunks straight mfma_16x16x32 per wave. Rows padded to
// K+8 elements so the 16 m/n lanes of a fragment read stride 272 B
// (4-bank rotation) instead of 256 B (single-bank pileup).
#define SCM_KP 136                    // 128-padded K + 8-element row pad
extern "C" __global__ __launch_bounds__(256) void fconv_smallc_mfma_k(
    const __hip_bfloat16* __restrict__ in,    // [B,H,W,*] slice
    int in_stride, int in_off,
    const __hip_bfloat16* __restrict__ wp,    // [taps][N][C]
    const float* __restrict__ bias,
    __hip_bfloat16* __restrict__ out,         // [B,H,W,N]
    int H, int W, int C, int N, int kh, int kw, int act, int kchunks) {
    __shared__ __hip_bfloat16 sraw[9 * 40 * 4];
    __shared__ __hip_bfloat16 sa[32 * SCM_KP];
    __shared__ __hip_bfloat16 sb[32 * SCM_KP];
    const int b = blockIdx.z;
    const int tiles = (W + 31) >> 5;
    const int y = blockIdx.y / tiles;
    const int x0 = (blockIdx.y % tiles) << 5;
    const int n0 = blockIdx.x * 32;
    const int tid = threadIdx.x;
    const int aw = 32 + kw - 1;
    const int pb = kh / 2, pbw = kw / 2;
    const int taps = kh * kw;
    const int K = taps * C;
    const int Kp = kchunks * 32;
    for (int e = tid; e < kh * aw; e += 256) {
        const int r = e / aw, cx = e % aw;
        const int yy = y + r - pb, xx = x0 + cx - pbw;
        const bool ok = (yy >= 0 && yy < H && xx >= 0 && xx < W);
        const __hip_bfloat16* src =
            in + (((long long)b * H + yy) * W + xx) * in_stride + in_off;
        for (int c = 0; c < C; ++c)
            sraw[e * C + c] = ok ? src[c] : (__hip_bfloat16)0.f;
    }
    // weights -> [n][K] rows; wp is contiguous in (n, c) per tap, so load
    // 8 elements (= 8/C n-adjacent channel groups) per 16-byte chunk and
    // scatter into the per-n rows
    for (int e8 = tid; e8 < taps * 32 * C / 8; e8 += 256) {
        const int per_tap = 32 * C / 8;
        const int t = e8 / per_tap;
        const int j = (e8 % per_tap) * 8;      // element offset within tap
        __hip_bfloat16 tmp[8];
        if (n0 * C + j + 8 <= N * C) {
            *(uint4v*)tmp = *(const uint4v*)(
                wp + ((size_t)t * N + n0) * C + j);
        } else {
            for (int u = 0; u < 8; ++u) {
                const int n = n0 + (j + u) / C;
                tmp[u] = n < N ? wp[((size_t)t * N + n) * C + (j + u) % C]
                               : (__hip_bfloat16)0.f;
            }
        }
        for (int u = 0; u < 8; ++u) {
            const int n = (j + u) / C;
            const int c = (j + u) % C;
            sb[n * SCM_KP + t * C + c] = tmp[u];
        }
    }
    // zero the K padding of the weight rows
    for (int e = tid; e < 32 * (Kp - K); e += 256)
        sb[(e / (Kp - K)) * SCM_KP + K + e % (Kp - K)] = (__hip_bfloat16)0.f;
    __syncthreads();
    for (int e = tid; e < 32 * Kp; e += 256) {
        const int pos = e / Kp, k = e % Kp;
        __hip_bfloat16 v = (__hip_bfloat16)0.f;
        if (k < K) {
            const int t = k / C, c = k % C;
            v = sraw[((t / kw) * aw + pos + t % kw) * C + c];
        }
        sa[pos * SCM_KP + k] = v;
    }
    __syncthreads();
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = (wave >> 1) * 16;
    const int wn = (wave & 1) * 16;
    const int kg = lane >> 4;
    const int m_af = wm + (lane & 15);
    const int n_bf = wn + (lane & 15);
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < kchunks; ++kc) {
        const short8 af = *(const short8*)(
            sa + (size_t)m_af * SCM_KP + kc * 32 + kg * 8);
        const short8 bf = *(const short8*)(
            sb + (size_t)n_bf * SCM_KP + kc * 32 + kg * 8);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int mm = wm + (lane >> 4) * 4 + r;
        const int nn = n0 + wn + (lane & 15);
        const int x = x0 + mm;
        if (x >= W || nn >= N) continue;
        float v = acc[r];
        if (bias) v += bias[nn];
        out[(((long long)b * H + y) * W + x) * N + nn] =
            (__hip_bfloat16)factivate(v, act);
    }
}

// fconv_smallc_mfma_k with one block per 32-position tile computing ALL N
// output channels, and the weights pre-packed on the host into the [N][128]
// image its B fragments read (k = tap*C + c, zero tail — packed once: the
// weights never change). The kernel above runs N/32 blocks per position
// tile, each re-laying its weight slice into LDS with scalar stores and
// redoing the same raw staging and im2col; here the window is staged and
// expanded once, the four waves split the N/16 channel tiles and B comes
// straight from the (L2-resident, 32 KB) image, so one barrier pair and no
// weight pass. Same k order, same 32-wide chunks ascending from a zero
// accumulator: the output is the kernel above's bit for bit.
extern "C" __global__ __launch_bounds__(256) void fconv_smallc_packed_k(
    const __hip_bfloat16* __restrict__ in,    // [B,H,W,*] slice
    int in_stride, int in_off,
    const __hip_bfloat16* __restrict__ wpk,   // [N][128]
    const float* __restrict__ bias,
    __hip_bfloat16* __restrict__ out,         // [B,H,W,N]
    int H, int W, int C, int N, int kh, int kw, int act, int kchunks) {
    __shared__ __hip_bfloat16 sraw[9 * 40 * 4];
    __shared__ __hip_bfloat16 sa[32 * SCM_KP];
    const int b = blockIdx.y;
    const int tiles = (W + 31) >> 5;
    const int y = blockIdx.x / tiles;
    const int x0 = (blockIdx.x % tiles) << 5;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int kg = lane >> 4;
    const int l15 = lane & 15;
    const int aw = 32 + kw - 1;
    const int pb = kh / 2, pbw = kw / 2;
    const int K = kh * kw * C;
    const int Kp = kchunks * 32;
    const int ntiles = N >> 4;
    // this wave's B fragments (n-tiles wave, wave+4): issued first, in
    // flight under the staging
    short8 bf[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int nt = wave + j * 4;
            short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (nt < ntiles && kc < kchunks)
                v = *(const short8*)(wpk + (size_t)(nt * 16 + l15) * 128 +
                                     kc * 32 + kg * 8);
            bf[j][kc] = v;
        }
    for (int e = tid; e < kh * aw; e += 256) {
        const int r = e / aw, cx = e % aw;
        const int yy = y + r - pb, xx = x0 + cx - pbw;
        const bool ok = (yy >= 0 && yy < H && xx >= 0 && xx < W);
        const __hip_bfloat16* src =
            in + (((long long)b * H + yy) * W + xx) * in_stride + in_off;
        for (int c = 0; c < C; ++c)
            sraw[e * C + c] = ok ? src[c] : (__hip_bfloat16)0.f;
    }
    __syncthreads();
    for (int e = tid; e < 32 * Kp; e += 256) {
        const int pos = e / Kp, k = e % Kp;
        __hip_bfloat16 v = (__hip_bfloat16)0.f;
        if (k < K) {
            const int t = k / C, c = k % C;
            v = sraw[((t / kw) * aw + pos + t % kw) * C + c];
        }
        sa[pos * SCM_KP + k] = v;
    }
    __syncthreads();
    floatx4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < 4; ++kc) {
        if (kc >= kchunks) break;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const short8 af = *(const short8*)(
                sa + (size_t)(i * 16 + l15) * SCM_KP + kc * 32 + kg * 8);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    af, bf[j][kc], acc[i][j], 0, 0, 0);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int nt = wave + j * 4;
        if (nt >= ntiles) continue;
        const int nn = nt * 16 + l15;
        const float bz = bias ? bias[nn] : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int x = x0 + i * 16 + kg * 4 + r;
                if (x >= W) continue;
                float v = acc[i][j][r];
                if (bias) v += bz;
                out[(((long long)b * H + y) * W + x) * N + nn] =
                    (__hip_bfloat16)factivate(v, act);
            }
    }
}

// Serves stride-1 C <= 4, K = taps*C <= 128, N a multiple of 16 up to 128
// (wpk: the [N][128] image). Returns 0 for anything else.
extern "C" int launch_fconv_smallc_packed(
    const void* in, int in_stride, int in_off, const void* wpk,
    const float* bias, void* out, int B, int H, int W, int C, int N, int kh,
    int kw, int act, hipStream_t s) {
    const int taps = kh * kw;
    if (C < 1 || C > 4 || taps * C > 128 || kh > 9 || kw > 9 || N < 16 ||
        N > 128 || N % 16 != 0)
        return 0;
    const int kchunks = (taps * C + 31) / 32;
    dim3 grid((unsigned)(H * ((W + 31) / 32)), (unsigned)B);
    hipLaunchKernelGGL(fconv_smallc_packed_k, grid, dim3(256), 0, s,
                       (const __hip_bfloat16*)in, in_stride, in_off,
                       (const __hip_bfloat16*)wpk, bias,
                       (__hip_bfloat16*)out, H, W, C, N, kh, kw, act,
                       kchunks);
    return 1;
}

// 2D-tile small-C direct conv (stride 1): the per-position window staging
// above re-reads every overlapped tap (convf1 7x7/C=2: 49 scattered 2-byte
// loads per output pixel — 43.7 us/call measured). This version stages a
// 16-position row tile WITH halo once per block (window overlap reused
// ~kw-fold) plus a 64-channel weight slice as floats, then does the tiny
// K=C*taps dot products from LDS: w reads are lane-consecutive, a reads
// wave-uniform (broadcast) — both conflict-free.
extern "C" __global__ __launch_bounds__(256) void fconv_smallc_tile_k(
    const __hip_bfloat16* __restrict__ in,    // [B, H, W, *] slice
    int in_stride, int in_off,
    const __hip_bfloat16* __restrict__ wp,    // [kh*kw][N][C]
    const float* __restrict__ bias,
    __hip_bfloat16* __restrict__ out,         // [B, H, W, N]
    int H, int W, int C, int N, int kh, int kw, int act) {
    extern __shared__ float smem_f[];
    const int AWIDTH = 16 + kw - 1;
    float* sa = smem_f;                       // [kh][AWIDTH][C]
    float* sw = smem_f + kh * AWIDTH * C;     // [taps][64][C]
    const int taps = kh * kw;
    const int tid = threadIdx.x;
    const int xt = (W + 15) >> 4;
    const int y = blockIdx.x / xt;
    const int x0 = (blockIdx.x % xt) * 16;
    const int n0 = blockIdx.y * 64;
    const int b = blockIdx.z;
    if ((N & 63) == 0) {
        // vectorized: the 64xC weight slice of each tap is contiguous in
        // wp and 16-byte aligned (N, n0 multiples of 64) — 8 bf16 per
        // load. (The scalar loop below was ~24 serial 2-byte rounds: the
        // dominant cost of the whole kernel at C=2.)
        const int per_tap = 64 * C / 8;
        for (int e8 = tid; e8 < taps * per_tap; e8 += 256) {
            const int t = e8 / per_tap;
            const int j = (e8 % per_tap) * 8;
            const uint4v v = *(const uint4v*)(
                wp + ((size_t)t * N + n0) * C + j);
            const unsigned int w4[4] = {v.x, v.y, v.z, v.w};
            float* dst = sw + t * 64 * C + j;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                union { unsigned int i; float f; } lo, hi;
                lo.i = (w4[q] & 0xffffu) << 16;
                hi.i = (w4[q] >> 16) << 16;
                dst[2 * q] = lo.f;
                dst[2 * q + 1] = hi.f;
            }
        }
    } else
    for (int e = tid; e < taps * 64 * C; e += 256) {
        const int t = e / (64 * C);
        const int rem = e % (64 * C);
        const int n = rem / C, c = rem % C;
        sw[e] = (n0 + n < N)
            ? (float)wp[((size_t)t * N + n0 + n) * C + c] : 0.f;
    }
    const int pb = kh / 2, pbw = kw / 2;
    for (int e = tid; e < kh * AWIDTH * C; e += 256) {
        const int r = e / (AWIDTH * C);
        const int rem = e % (AWIDTH * C);
        const int a = rem / C, c = rem % C;
        const int yy = y + r - pb;
        const int xx = x0 + a - pbw;
        float v = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W)
            v = (float)in[(((long long)b * H + yy) * W + xx) * in_stride
                          + in_off + c];
        sa[e] = v;
    }
    __syncthreads();
    const int lane = tid & 63;
    const int wavep = (tid >> 6) * 4;         // wave's first of 4 positions
    float acc[4];
    const float bz = (bias && n0 + lane < N) ? bias[n0 + lane] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = bz;
    for (int t = 0; t < taps; ++t) {
        const int dy = t / kw, dx = t % kw;
        for (int c = 0; c < C; ++c) {
            const float w = sw[(t * 64 + lane) * C + c];
            const float* arow = sa + (dy * AWIDTH) * C + c;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i] = fmaf(arow[(wavep + i + dx) * C], w, acc[i]);
        }
    }
    if (n0 + lane < N) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int x = x0 + wavep + i;
            if (x < W)
                out[(((long long)b * H + y) * W + x) * N + n0 + lane] =
                    (__hip_bfloat16)factivate(acc[i], act);
        }
    }
}

// grid-stride naive fallback for shapes outside the LDS caps
extern "C" __global__ void fconv_smallk_nhwc_bf16_k(
    const __hip_bfloat16* __restrict__ in, int in_stride, int in_off,
    const __hip_bfloat16* __restrict__ wp,
    const float* __restrict__ bias,
    __hip_bfloat16* __restrict__ out,
    int H, int W, int C, int N, int kh, int kw, int act, long long total) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const int n = (int)(idx % N);
        const long long q = idx / N;
        const int x = (int)(q % W);
        const int y = (int)((q / W) % H);
        const int b = (int)(q / ((long long)W * H));
        float acc = bias ? bias[n] : 0.0f;
        for (int ty = 0; ty < kh; ++ty) {
            const int yy = y + ty - kh / 2;
            if (yy < 0 || yy >= H) continue;
            for (int tx = 0; tx < kw; ++tx) {
                const int xx = x + tx - kw / 2;
                if (xx < 0 || xx >= W) continue;
                const __hip_bfloat16* src =
                    in + (((long long)b * H + yy) * W + xx) * in_stride
                    + in_off;
                const __hip_bfloat16* wr =
                    wp + ((size_t)(ty * kw + tx) * N + n) * C;
                for (int c = 0; c < C; ++c)
                    acc = fmaf((float)src[c], (float)wr[c], acc);
            }
        }
        out[idx] = (__hip_bfloat16)factivate(acc, act);
    }
}

extern "C" void launch_fconv_smallk_nhwc_bf16(
    const void* in, int in_stride, int in_off, const void* wp,
    const float* bias, void* out, int B, int H, int W, int C, int N, int kh,
    int kw, int act, int conv_stride, hipStream_t s) {
    // H, W are OUTPUT dims (input = conv_stride*H x conv_stride*W)
    const long long ncells = (long long)B * H * W;
    const int taps = kh * kw;
    static const int scm = [] {
        const char* e = getenv("RAFT_AMD_SMALLC_MFMA");
        return e ? atoi(e) : 1;
    }();
    if (scm && conv_stride == 1 && C <= 4 && taps * C <= 128 && kh <= 9 &&
        kw <= 9 && (N * C) % 8 == 0) {
        const int kchunks = (taps * C + 31) / 32;
        dim3 grid((unsigned)((N + 31) / 32),
                  (unsigned)(H * ((W + 31) / 32)), (unsigned)B);
        hipLaunchKernelGGL(fconv_smallc_mfma_k, grid, dim3(256), 0, s,
                           (const __hip_bfloat16*)in, in_stride, in_off,
                           (const __hip_bfloat16*)wp, bias,
                           (__hip_bfloat16*)out, H, W, C, N, kh, kw, act,
                           kchunks);
        return;
    }
    const int smem_tile =
        (kh * (16 + kw - 1) * C + taps * 64 * C) * (int)sizeof(float);
    if (conv_stride == 1 && C <= 4 && taps <= 81 && smem_tile <= 49152) {
        dim3 grid((unsigned)(H * ((W + 15) >> 4)),
                  (unsigned)((N + 63) >> 6), (unsigned)B);
        hipLaunchKernelGGL(fconv_smallc_tile_k, grid, dim3(256), smem_tile,
                           s, (const __hip_bfloat16*)in, in_stride, in_off,
                           (const __hip_bfloat16*)wp, bias,
                           (__hip_bfloat16*)out, H, W, C, N, kh, kw, act);
        return;
    }
    if (N <= 128 && 256 % N == 0 && taps * N * C <= SK_MAXW &&
        (256 / N) * taps * C <= SK_MAXIN) {
        const int PPB = 256 / N;
        const long long groups = (ncells + PPB - 1) / PPB;
        // cap the grid well below the group count: every block stages the
        // full weight set once (25 KB for convf1) — 3520 one-group blocks
        // cost 88 MB of weight reads (measured 43.5 us); ~640 blocks
        // amortize it ~6x while still filling 256 CUs.
        int blocks = (int)min(groups, (long long)640);
        hipLaunchKernelGGL(fconv_smallk_lds_k, dim3(blocks), dim3(256), 0,
                           s, (const __hip_bfloat16*)in, in_stride, in_off,
                           (const __hip_bfloat16*)wp, bias,
                           (__hip_bfloat16*)out, H, W, C, N, kh, kw, act,
                           conv_stride, ncells);
        return;
    }
    // naive fallback is stride-1 only
    if (conv_stride != 1) return;
    const long long total = ncells * N;
    int blocks = (int)min((total + 255) / 256, (long long)4096);
    hipLaunchKernelGGL(fconv_smallk_nhwc_bf16_k, dim3(blocks), dim3(256), 0,
                       s, (const __hip_bfloat16*)in, in_stride, in_off,
                       (const __hip_bfloat16*)wp, bias,
                       (__hip_bfloat16*)out, H, W, C, N, kh, kw, act, total);
}


// delta-flow head with the coords update fused: coords_out = coords_in +
// conv(in) — removes the per-iteration cast+add (aten::copy_/add_ glue,
// ~30 us/iter measured in the chrome trace).
extern "C" void launch_fconv_dflow_coords(
    const void* in, int Cin, int in_stride, int in_off, const void* wp,
    const float* bias, const float* coords_in, float* coords_out,
    void* flow_out, int flow_stride, int flow_off, int B, int H, int W,
    int kh, int kw, hipStream_t s) {
    const long long ncells = (long long)B * H * W;
    if (fconv_tinyn2_ok(fconv_knobs(), Cin, kh, kw)) {
        const int smem = (kh * (8 + kw - 1) * Cin + kh * kw * 2 * Cin) * 2;
        dim3 g2((unsigned)(H * ((W + 7) / 8)), 1, (unsigned)B);
        hipLaunchKernelGGL(fconv_tinyn2_k<2>, g2, dim3(256), smem, s,
                           (const __hip_bfloat16*)in, Cin, in_stride,
                           in_off, (const __hip_bfloat16*)wp, bias, nullptr,
                           coords_in, coords_out, (__hip_bfloat16*)flow_out,
                           flow_stride, flow_off, H, W, kh, kw, 0);
        return;
    }
    dim3 tg((unsigned)((ncells + 3) / 4));
    hipLaunchKernelGGL(fconv_tinyn_k<2>, tg, dim3(256), 0, s,
                       (const __hip_bfloat16*)in, Cin, in_stride, in_off,
                       (const __hip_bfloat16*)wp, bias, nullptr, coords_in,
                       coords_out, (__hip_bfloat16*)flow_out, flow_stride,
                       flow_off, H, W, kh, kw, 0, ncells);
}
