// NHWC (channels-last) correlation kernels — the MI355X-native layout.
//
// corr_volume_nhwc: C[b,m,n] = sum_k F1[b,m,k] * F2[b,n,k] / sqrt(K), bf16
// inputs, fp32 accumulate (MFMA v_mfma_f32_16x16x32_bf16), fp32 or bf16
// volume out.  Channels-last fmaps make BOTH operands k-contiguous, so LDS
// staging is a straight contiguous copy and fragments are ds_read_b128 with
// an XOR swizzle (guide §5.5 T2) — no transposes anywhere.
//
// corr_lookup_nhwc: same tap math as corr_lookup.hip (edge-clamp trunc
// bilinear, [::-1] window order) but the output is physical NHWC
// [B,H,W,L*KK] with the tap channel fastest: consecutive lanes write
// consecutive channels of one query (fully coalesced) and read overlapping
// window cells (L1-friendly).  Template on the volume dtype (fp32 / bf16).

#include "common.h"
#include "lookup_conv_geom.h"
#include <type_traits>
#include <hip/hip_bf16.h>

typedef short short8 __attribute__((ext_vector_type(8)));
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));
typedef unsigned int uint2v __attribute__((ext_vector_type(2)));

#define CV_BM 128
#define CV_BN 128
#define CV_BK 64
// +16 B row pad: consecutive rows land on distinct 16-B bank slots mod the
// 256-B bank row (stride 144: 16 distinct residues), so the 16-lane
// ds_read_b128 groups (16 different rows, same column) are conflict-free
// (guide §2/§6 Guideline 4).
#define CV_ROWB (CV_BK * 2 + 16)

RAFT_DEV unsigned swz(int row, unsigned colbyte) {
    return row * CV_ROWB + colbyte;
}

// L2 band remap (r2, verdict #6): with row-major tile order every m-tile
// row re-streams BOTH 16.6-MB fmaps from HBM (config 4: ~8.4 GB reads
// measured as a 1.8 ms kernel). Walking tiles column-major within an
// m-band of `super` tiles keeps the band's A rows (1 MB at super=16)
// L2-hot and cuts reads to A + B*(tiles_m/super) ≈ 0.3 GB.
RAFT_DEV void band_remap(int super, int& mt, int& nt) {
    if (super <= 0) return;
    const int tiles_n = gridDim.x, tiles_m = gridDim.y;
    const long long lin = (long long)mt * tiles_n + nt;
    const long long band = (long long)super * tiles_n;
    const int b0 = (int)(lin / band);
    const int rem = (int)(lin % band);
    const int gh = min(super, tiles_m - b0 * super);
    nt = rem / gh;
    mt = b0 * super + rem % gh;
}

// Shared tile body. BIDIR additionally writes every finished tile a second
// time, transposed, into out_t [B, N, M] (requires M == N): the backward
// volume C21[n, m] = C12[m, n] comes from the same fp32 accumulators with
// the same scale and bf16 rounding, so it is the bit-exact transpose.
template <typename OUT_T, bool BIDIR>
RAFT_DEV void corr_volume_nhwc_tile(
    const __hip_bfloat16* __restrict__ f1,   // [B, M, K]
    const __hip_bfloat16* __restrict__ f2,   // [B, N, K]
    OUT_T* __restrict__ out,                 // [B, M, N]
    __hip_bfloat16* __restrict__ out_t,      // [B, N, M] (BIDIR only)
    int M, int N, int K, float scale, int super) {
    __shared__ char smem[2 * CV_BM * CV_ROWB];
    char* sA = smem;
    char* sB = smem + CV_BM * CV_ROWB;

    const int b = blockIdx.z;
    int mt_ = blockIdx.y, nt_ = blockIdx.x;
    band_remap(super, mt_, nt_);
    const int m0 = mt_ * CV_BM;
    const int n0 = nt_ * CV_BN;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = (wave >> 1) * 64;
    const int wn = (wave & 1) * 64;

    const __hip_bfloat16* A = f1 + (size_t)b * M * K;
    const __hip_bfloat16* Bp = f2 + (size_t)b * N * K;

    floatx4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

    const int srow = tid >> 1;                 // 0..127
    const unsigned scol = (tid & 1) * 64;      // byte offset within row half

    // register-prefetch pipeline (r2): loads for k-step s+1 issue before
    // step s's MFMA burst — the single-buffered loop exposed the full
    // global latency on each of the K/CV_BK steps
    uint4v pa[4], pb[4];
    const bool oka = m0 + srow < M, okb = n0 + srow < N;
    const __hip_bfloat16* ga =
        A + (size_t)min(m0 + srow, M - 1) * K + (tid & 1) * 32;
    const __hip_bfloat16* gb =
        Bp + (size_t)min(n0 + srow, N - 1) * K + (tid & 1) * 32;
    auto load_step = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pa[j] = oka ? *(const uint4v*)(ga + k0 + j * 8)
                        : uint4v{0, 0, 0, 0};
            pb[j] = okb ? *(const uint4v*)(gb + k0 + j * 8)
                        : uint4v{0, 0, 0, 0};
        }
    };
    load_step(0);
    for (int k0 = 0; k0 < K; k0 += CV_BK) {
        if (k0) __syncthreads();
        {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                *(uint4v*)(sA + swz(srow, scol + j * 16)) = pa[j];
                *(uint4v*)(sB + swz(srow, scol + j * 16)) = pb[j];
            }
        }
        __syncthreads();
        if (k0 + CV_BK < K) load_step(k0 + CV_BK);

#pragma unroll
        for (int kk = 0; kk < CV_BK / 32; ++kk) {
            short8 af[4], bf[4];
            const unsigned cb = kk * 64 + (lane >> 4) * 16;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                af[i] = *(const short8*)(sA + swz(wm + i * 16 + (lane & 15), cb));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                bf[j] = *(const short8*)(sB + swz(wn + j * 16 + (lane & 15), cb));
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                        af[i], bf[j], acc[i][j], 0, 0, 0);
        }
    }

    // Vectorized interior store (r2, verdict #6): the C-fragment layout
    // scatters 2-B elements across 4 rows per store instruction, which
    // quarters HBM write efficiency — and config 4's 2.1 GB volume write
    // is the kernel's bound. Round-trip the tile through LDS (free after
    // the k-loop) and emit 16-B/lane row-contiguous stores.
    bool fwd_done = false;
    if constexpr (std::is_same<OUT_T, __hip_bfloat16>::value) {
        if (m0 + CV_BM <= M && n0 + CV_BN <= N) {
            constexpr int STP = CV_BN + 8;    // +8 elem pad: bank rotation
            __syncthreads();
            __hip_bfloat16* st = (__hip_bfloat16*)smem;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        st[(wm + i * 16 + (lane >> 4) * 4 + r) * STP +
                           wn + j * 16 + (lane & 15)] =
                            (__hip_bfloat16)(acc[i][j][r] * scale);
            __syncthreads();
            const int row = tid >> 1;
            const int c0 = (tid & 1) * 64;
            const __hip_bfloat16* src = st + (size_t)row * STP + c0;
            OUT_T* dst = out + ((size_t)b * M + m0 + row) * N + n0 + c0;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                *(uint4v*)(dst + q * 8) = *(const uint4v*)(src + q * 8);
            if constexpr (BIDIR) {
                // Reverse store: a second LDS round trip with the tile
                // transposed. The C fragment holds 4 consecutive m for one
                // n, so st_t[n][m] takes one packed 8-B LDS write per
                // fragment (16 per lane, which the compiler pairs into 8
                // two-address writes, instead of the forward image's 64
                // 2-B writes). Pitch: an 8-B write is banked (a/4)%32
                // over 16-lane groups = 16 n-rows of one m-quad, so only
                // a pitch of 2*odd dwords is conflict-free — and such rows
                // are just 8-B aligned, which turns the read-back into
                // half-rate two-address reads with their own 2-way
                // conflict. The forward pitch (68 dwords, 16-B aligned
                // rows) is 2-way on the write (rows r, r+8: 8 LDS cycles
                // against the instruction's 6) and keeps the read-back the
                // conflict-free ds_read_b128 of the forward path: ~160
                // LDS cycles per wave and tile against ~230, so it stays.
                // 16-B global stores need 16-B aligned row starts.
                if ((M & 7) == 0) {
                    constexpr int TP = CV_BM + 8;
                    static_assert(CV_BN * TP * 2 <= (int)sizeof(smem),
                                  "transposed tile must fit the k-loop LDS");
                    __syncthreads();
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            unsigned short h[4];
#pragma unroll
                            for (int r = 0; r < 4; ++r)
                                h[r] = __bfloat16_as_ushort(
                                    (__hip_bfloat16)(acc[i][j][r] * scale));
                            uint2v pk;
                            pk.x = (unsigned)h[0] | ((unsigned)h[1] << 16);
                            pk.y = (unsigned)h[2] | ((unsigned)h[3] << 16);
                            *(uint2v*)(st + (wn + j * 16 + (lane & 15)) * TP +
                                       wm + i * 16 + (lane >> 4) * 4) = pk;
                        }
                    __syncthreads();
                    const __hip_bfloat16* srct = st + (size_t)row * TP + c0;
                    __hip_bfloat16* dstt =
                        out_t + ((size_t)b * N + n0 + row) * M + m0 + c0;
#pragma unroll
                    for (int q = 0; q < 8; ++q)
                        *(uint4v*)(dstt + q * 8) =
                            *(const uint4v*)(srct + q * 8);
                    return;
                }
                // unaligned rows: the scalar reverse store below
                fwd_done = true;
            } else {
                return;
            }
        }
    }
    if (!fwd_done) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
                    const int n = n0 + wn + j * 16 + (lane & 15);
                    if (m < M && n < N)
                        out[((size_t)b * M + m) * N + n] =
                            (OUT_T)(acc[i][j][r] * scale);
                }
    }
    if constexpr (BIDIR) {
        // edge tiles and unaligned rows: scalar guarded reverse store
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + wm + i * 16 + (lane >> 4) * 4 + r;
                    const int n = n0 + wn + j * 16 + (lane & 15);
                    if (m < M && n < N)
                        out_t[((size_t)b * N + n) * M + m] =
                            (__hip_bfloat16)(acc[i][j][r] * scale);
                }
    }
}

template <typename OUT_T>
__global__ __launch_bounds__(256) void corr_volume_nhwc_bf16_k(
    const __hip_bfloat16* __restrict__ f1,   // [B, M, K]
    const __hip_bfloat16* __restrict__ f2,   // [B, N, K]
    OUT_T* __restrict__ out,                 // [B, M, N]
    int M, int N, int K, float scale, int super) {
    corr_volume_nhwc_tile<OUT_T, false>(f1, f2, out, nullptr, M, N, K, scale,
                                        super);
}

// forward volume into out, its transpose into out_t — one GEMM, two stores
__global__ __launch_bounds__(256) void corr_volume_nhwc_bidir_k(
    const __hip_bfloat16* __restrict__ f1,   // [B, M, K]
    const __hip_bfloat16* __restrict__ f2,   // [B, M, K]
    __hip_bfloat16* __restrict__ out,        // [B, M, M]
    __hip_bfloat16* __restrict__ out_t,      // [B, M, M]
    int M, int K, float scale, int super) {
    corr_volume_nhwc_tile<__hip_bfloat16, true>(f1, f2, out, out_t, M, M, K,
                                                scale, super);
}

extern "C" int corr_super_band() {
    // band height in tiles; 0 disables the remap (RAFT_AMD_CORR_SUPER)
    static const int v = [] {
        const char* e = getenv("RAFT_AMD_CORR_SUPER");
        return e ? atoi(e) : 16;
    }();
    return v;
}

extern "C" void launch_corr_volume_nhwc_bf16(
    const void* f1, const void* f2, void* out, bool out_bf16, int Bsz,
    int M, int N, int K, float scale, hipStream_t s) {
    dim3 grid(cdiv(N, CV_BN), cdiv(M, CV_BM), Bsz);
    const int super = corr_super_band();
    if (out_bf16)
        hipLaunchKernelGGL(corr_volume_nhwc_bf16_k<__hip_bfloat16>, grid,
                           dim3(256), 0, s, (const __hip_bfloat16*)f1,
                           (const __hip_bfloat16*)f2, (__hip_bfloat16*)out,
                           M, N, K, scale, super);
    else
        hipLaunchKernelGGL(corr_volume_nhwc_bf16_k<float>, grid, dim3(256),
                           0, s, (const __hip_bfloat16*)f1,
                           (const __hip_bfloat16*)f2, (float*)out,
                           M, N, K, scale, super);
}

extern "C" void launch_corr_volume_nhwc_bidir(
    const void* f1, const void* f2, void* out, int Bsz, int M, int K,
    float scale, hipStream_t s) {
    // out: [2*Bsz, M, M] bf16 — forward half, then the transposed half
    dim3 grid(cdiv(M, CV_BN), cdiv(M, CV_BM), Bsz);
    __hip_bfloat16* o = (__hip_bfloat16*)out;
    hipLaunchKernelGGL(corr_volume_nhwc_bidir_k, grid, dim3(256), 0, s,
                       (const __hip_bfloat16*)f1, (const __hip_bfloat16*)f2,
                       o, o + (size_t)Bsz * M * M, M, K, scale,
                       corr_super_band());
}

// --------------------------------------------------------------- NHWC lookup
struct LevelsT {
    const void* ptr[4];
    int H[4];
    int W[4];
};

// volume-element load: fp32/bf16 direct, e4m3 via the hw convert; fp8
// volumes carry a stored scale undone by vol_scale (see corr_fp8.hip)
template <typename T>
RAFT_DEV float lvload(const T& v) { return (float)v; }
template <>
RAFT_DEV float lvload<unsigned char>(const unsigned char& v) {
    return __builtin_amdgcn_cvt_f32_fp8((int)v, 0);
}

// One lookup tap: channel c = lvl*KK + k of query q, as fp32 before the
// output rounding. The single definition of the tap arithmetic — the
// lookup kernel and the fused lookup -> conv kernel both evaluate
// corr_tap_at(corr_tap_col(c), q), so the two produce the same bits. The
// split lets a caller that keeps c over many queries compute the
// channel's part (level, window offset, level geometry) once.
template <typename T>
struct TapCol {
    const T* base;     // the level's volume
    int H2, W2;
    float inv;         // 1 / 2^lvl
    float dx, dy;      // window offset of the tap
};

template <typename T>
RAFT_DEV TapCol<T> corr_tap_col(const LevelsT& lv, int c, int K, int KK,
                                int radius) {
    const int lvl = c / KK;
    const int k = c - lvl * KK;
    TapCol<T> t;
    t.inv = 1.0f / (float)(1 << lvl);
    t.dx = (float)(k / K - radius);
    t.dy = (float)(k % K - radius);
    t.H2 = lv.H[lvl];
    t.W2 = lv.W[lvl];
    t.base = (const T*)lv.ptr[lvl];
    return t;
}

template <typename T>
RAFT_DEV float corr_tap_at(const TapCol<T>& tc,
                           const float* __restrict__ coords, long long q,
                           float vs) {
    const float cx = coords[q * 2] * tc.inv + tc.dx;
    const float cy = coords[q * 2 + 1] * tc.inv + tc.dy;

    const int H2 = tc.H2, W2 = tc.W2;
    const T* slice = tc.base + q * (size_t)H2 * W2;
    BilinearTap t = make_tap(cx, cy, W2, H2);
    const float Ia = lvload(slice[t.y0 * W2 + t.x0]);
    const float Ib = lvload(slice[t.y1 * W2 + t.x0]);
    const float Ic = lvload(slice[t.y0 * W2 + t.x1]);
    const float Id = lvload(slice[t.y1 * W2 + t.x1]);
    return vs * (t.wa * Ia + t.wb * Ib + t.wc * Ic + t.wd * Id);
}

template <typename T>
RAFT_DEV float corr_tap(const LevelsT& lv, const float* __restrict__ coords,
                        long long q, int c, int K, int KK, int radius,
                        float vs) {
    return corr_tap_at(corr_tap_col<T>(lv, c, K, KK, radius), coords, q, vs);
}

template <typename T, typename OT>
__global__ void corr_lookup_nhwc_k(
    LevelsT lv, const float* __restrict__ coords,  // [B, H, W, 2]
    OT* __restrict__ out,                          // [B, H, W, Cs]
    __hip_bfloat16* __restrict__ flow_out,         // strided slice or null
    int flow_stride, int flow_off,
    const float* __restrict__ vol_scale,           // null -> 1.0
    int H, int W, int num_levels, int radius, int Cs, long long total) {
    const float vs = vol_scale ? *vol_scale : 1.0f;
    const int K = 2 * radius + 1;
    const int KK = K * K;
    const int C = num_levels * KK;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const int c = (int)(idx % C);
        const long long q = idx / C;               // b*H*W + y*W + x

        if (flow_out && c < 2) {
            // fused flow = coords - identity grid (coords0 is the pixel
            // grid by construction, RAFT.py:111-117); written into a
            // channel slice of the GRU input buffer directly
            const float base = (c == 0) ? (float)(q % W)
                                        : (float)((q / W) % H);
            flow_out[q * flow_stride + flow_off + c] =
                (__hip_bfloat16)(coords[q * 2 + c] - base);
        }
        out[q * Cs + c] =
            (OT)corr_tap<T>(lv, coords, q, c, K, KK, radius, vs);
    }
}

// flow = coords - pixel grid as bf16 into a channel slice of rows of
// flow_stride elements: what corr_lookup_nhwc_k's flow_out writes, on its
// own. The fused loop calls it once per loop entry; from then on the
// delta-flow kernel writes the slice for the next iteration.
__global__ void flow_slice_k(const float* __restrict__ coords,
                             __hip_bfloat16* __restrict__ flow_out,
                             int flow_stride, int flow_off, int H, int W,
                             long long total) {   // total = B*H*W*2
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const int c = (int)(idx & 1);
        const long long q = idx >> 1;
        const float base = (c == 0) ? (float)(q % W)
                                    : (float)((q / W) % H);
        flow_out[q * flow_stride + flow_off + c] =
            (__hip_bfloat16)(coords[idx] - base);
    }
}

extern "C" void launch_flow_slice(const float* coords, void* flow_out,
                                  int flow_stride, int flow_off, int B,
                                  int H, int W, hipStream_t s) {
    const long long total = (long long)B * H * W * 2;
    int blocks = (int)min((total + 255) / 256, (long long)2048);
    hipLaunchKernelGGL(flow_slice_k, dim3(blocks), dim3(256), 0, s, coords,
                       (__hip_bfloat16*)flow_out, flow_stride, flow_off, H,
                       W, total);
}

// vol_type: 0 = fp32, 1 = bf16, 2 = e4m3 (vol_scale dequantizes)
extern "C" void launch_corr_lookup_nhwc(
    const void* const* level_ptrs, const int* level_h, const int* level_w,
    int vol_type, const float* vol_scale, const float* coords, void* out,
    bool out_bf16, void* flow_out, int flow_stride, int flow_off, int B,
    int H, int W, int num_levels, int radius, int Cs, hipStream_t s) {
    LevelsT lv{};
    for (int i = 0; i < num_levels; ++i) {
        lv.ptr[i] = level_ptrs[i];
        lv.H[i] = level_h[i];
        lv.W[i] = level_w[i];
    }
    const int K = 2 * radius + 1;
    const long long total = (long long)B * H * W * num_levels * K * K;
    int blocks = (int)min((total + 255) / 256, (long long)8192);
#define LKCASE(T, VT, OT, OTC)                                              \
    if (vol_type == VT && out_bf16 == OTC) {                                \
        hipLaunchKernelGGL((corr_lookup_nhwc_k<T, OT>), dim3(blocks),       \
                           dim3(256), 0, s, lv, coords, (OT*)out,           \
                           (__hip_bfloat16*)flow_out, flow_stride,          \
                           flow_off, vol_scale, H, W, num_levels, radius,   \
                           Cs, total);                                      \
        return;                                                             \
    }
    LKCASE(float, 0, float, false)
    LKCASE(float, 0, __hip_bfloat16, true)
    LKCASE(__hip_bfloat16, 1, float, false)
    LKCASE(__hip_bfloat16, 1, __hip_bfloat16, true)
    LKCASE(unsigned char, 2, float, false)
    LKCASE(unsigned char, 2, __hip_bfloat16, true)
#undef LKCASE
}

// ------------------------------------------- fused lookup -> 1x1 conv
// out[q, n] = act(sum_c bf16(tap(q, c)) * Wp[n][c] + bias[n]): the lookup
// and the pointwise conv that consumes it (the motion encoder's convc1)
// as one kernel, without the [positions, Cs] round trip between them. A
// pointwise consumer needs no halo, so a block computes the taps of its
// BM positions straight into LDS as the A operand (rows of Kp = kchunks*32
// bf16, zero past C — the pad columns of the unfused buffer), and after
// ONE barrier its waves split the N/16 output-channel tiles: 16x16x32
// MFMA over the k-chunks in ascending order from a zero accumulator, bias
// then activation in the epilogue — the order fconv_nhwc_bf16_k uses for
// a 1x1, so the result is the unfused pair's bit for bit. B fragments come
// straight from global memory in fragment layout (a lane's 16 bytes at
// wp[n][k0 + (lane>>4)*8]): the packed weights are L2-resident and shared
// by every block, and the k-loop needs no barrier. Geometry (tile, grid,
// LDS) is decided by lookup_conv_geom() in lookup_conv_geom.h.
template <typename T, int BM, int NW>
__global__ __launch_bounds__(NW * 64) void corr_lookup_conv1x1_k(
    LevelsT lv, const float* __restrict__ coords,  // [P, 2]
    const __hip_bfloat16* __restrict__ wp,         // [N][Cs]
    const float* __restrict__ bias,                // [N] or null
    __hip_bfloat16* __restrict__ out,              // [P, N]
    const float* __restrict__ vol_scale,           // null -> 1.0
    int num_levels, int radius, int Cs, int N, int act, int kchunks,
    long long P) {
    extern __shared__ __hip_bfloat16 lc_sa[];      // [BM][Kp + pad]
    constexpr int NT = NW * 64;
    constexpr int MI = BM / 16;
    constexpr int NJ = 16 / NW;                    // n-tiles per wave (max)
    const float vs = vol_scale ? *vol_scale : 1.0f;
    const int K = 2 * radius + 1;
    const int KK = K * K;
    const int C = num_levels * KK;
    const int Kp = kchunks * 32;
    const int KR = Kp + LCONV_ROW_PAD;
    const long long q0 = (long long)blockIdx.x * BM;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int kg = lane >> 4;
    const int l15 = lane & 15;
    const int ntiles = N >> 4;

    // B fragments of one k-chunk: rows past N (wave-uniform) and columns
    // past Cs are zero, as the staged weight tiles of the unfused conv
    auto loadB = [&](int kc, short8* bf) {
        const int k = kc * 32 + kg * 8;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int nt = wave + j * NW;
            short8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            if (nt < ntiles && k < Cs)
                v = *(const short8*)(wp + (size_t)(nt * 16 + l15) * Cs + k);
            bf[j] = v;
        }
    };
    short8 bcur[NJ], bnxt[NJ];
    loadB(0, bcur);          // in flight under the tap phase

    // tap phase: consecutive lanes take consecutive channels of one
    // query (overlapping window cells), as the lookup kernel does. A
    // thread keeps its channel over the tile's rows — NT/C rows per pass —
    // so the channel's part of the tap (integer divisions, level
    // geometry) is computed once per thread, not once per tap; with fewer
    // threads than channels it walks the channels instead.
    const int rpp = NT >= C ? NT / C : 1;          // rows per pass
    const int r0 = NT >= C ? tid / C : 0;
    if (r0 < rpp) {
        for (int c = tid - r0 * C; c < C; c += NT) {
            const TapCol<T> tc = corr_tap_col<T>(lv, c, K, KK, radius);
            for (int pos = r0; pos < BM; pos += rpp) {
                const long long q = q0 + pos;
                __hip_bfloat16 v = (__hip_bfloat16)0.f;
                if (q < P)
                    v = (__hip_bfloat16)corr_tap_at(tc, coords, q, vs);
                lc_sa[pos * KR + c] = v;
            }
        }
    }
    // zero columns [C, Kp): the pad channels of the unfused buffer
    const int padw = Kp - C;
    for (int e = tid; e < BM * padw; e += NT) {
        const int pos = e / padw;
        lc_sa[pos * KR + C + (e - pos * padw)] = (__hip_bfloat16)0.f;
    }
    __syncthreads();

    floatx4 acc[MI][NJ];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < kchunks; ++kc) {
        if (kc + 1 < kchunks) loadB(kc + 1, bnxt);
        short8 af[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i)
            af[i] = *(const short8*)(lc_sa + (i * 16 + l15) * KR + kc * 32 +
                                     kg * 8);
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                    af[i], bcur[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < NJ; ++j) bcur[j] = bnxt[j];
    }

#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int nt = wave + j * NW;
        if (nt >= ntiles) continue;
        const int n = nt * 16 + l15;
        const float bz = bias ? bias[n] : 0.0f;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long q = q0 + i * 16 + kg * 4 + r;
                if (q >= P) continue;
                float v = acc[i][j][r];
                if (bias) v += bz;
                out[q * N + n] = (__hip_bfloat16)factivate(v, act);
            }
    }
}

// vol_type: 1 = bf16, 2 = e4m3 (vol_scale dequantizes). Returns 0 when
// the shape or the volume type is not served: the caller runs the pair.
extern "C" int launch_corr_lookup_conv1x1(
    const void* const* level_ptrs, const int* level_h, const int* level_w,
    int vol_type, const float* vol_scale, const float* coords,
    const void* wp, const float* bias, void* out, int B, int H, int W,
    int num_levels, int radius, int Cs, int N, int act, hipStream_t s) {
    static const int tile = lookup_conv_tile_from_env();
    const int K = 2 * radius + 1;
    const long long P = (long long)B * H * W;
    const LookupConvGeom g =
        lookup_conv_geom(P, num_levels * K * K, Cs, N, tile);
    if (!g.ok || (vol_type != 1 && vol_type != 2)) return 0;
    LevelsT lv{};
    for (int i = 0; i < num_levels; ++i) {
        lv.ptr[i] = level_ptrs[i];
        lv.H[i] = level_h[i];
        lv.W[i] = level_w[i];
    }
#define LCCASE(T, VT, BM_, NW_)                                             \
    if (vol_type == VT && g.BM == BM_ && g.waves == NW_) {                  \
        hipLaunchKernelGGL((corr_lookup_conv1x1_k<T, BM_, NW_>),            \
                           dim3(g.grid), dim3(g.block), g.lds_bytes, s, lv, \
                           coords, (const __hip_bfloat16*)wp, bias,         \
                           (__hip_bfloat16*)out, vol_scale, num_levels,     \
                           radius, Cs, N, act, g.kchunks, P);               \
        return 1;                                                           \
    }
#define LCTILES(T, VT)                                                      \
    LCCASE(T, VT, 16, 4) LCCASE(T, VT, 16, 8) LCCASE(T, VT, 16, 16)         \
    LCCASE(T, VT, 32, 4) LCCASE(T, VT, 32, 8) LCCASE(T, VT, 32, 16)
    LCTILES(__hip_bfloat16, 1)
    LCTILES(unsigned char, 2)
#undef LCTILES
#undef LCCASE
    return 0;
}

// backward: scatter into fp32 grad volumes from an NHWC grad_out
struct GradLevels {
    float* ptr[4];
    int H[4];
    int W[4];
};

extern "C" __global__ void corr_lookup_nhwc_bwd_k(
    GradLevels lv, const float* __restrict__ coords,
    const float* __restrict__ grad_out,            // [B, H, W, L*KK]
    int H, int W, int num_levels, int radius, long long total) {
    const int K = 2 * radius + 1;
    const int KK = K * K;
    const int C = num_levels * KK;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const float g = grad_out[idx];
        const int c = (int)(idx % C);
        const long long q = idx / C;
        const int lvl = c / KK;
        const int k = c - lvl * KK;
        const float inv = 1.0f / (float)(1 << lvl);
        const float cx = coords[q * 2] * inv + (float)(k / K - radius);
        const float cy = coords[q * 2 + 1] * inv + (float)(k % K - radius);
        const int H2 = lv.H[lvl], W2 = lv.W[lvl];
        float* slice = lv.ptr[lvl] + q * (size_t)H2 * W2;
        BilinearTap t = make_tap(cx, cy, W2, H2);
        atomicAdd(&slice[t.y0 * W2 + t.x0], t.wa * g);
        atomicAdd(&slice[t.y1 * W2 + t.x0], t.wb * g);
        atomicAdd(&slice[t.y0 * W2 + t.x1], t.wc * g);
        atomicAdd(&slice[t.y1 * W2 + t.x1], t.wd * g);
    }
}

extern "C" void launch_corr_lookup_nhwc_bwd(
    float* const* grad_ptrs, const int* level_h, const int* level_w,
    const float* coords, const float* grad_out, int B, int H, int W,
    int num_levels, int radius, hipStream_t s) {
    GradLevels lv{};
    for (int i = 0; i < num_levels; ++i) {
        lv.ptr[i] = grad_ptrs[i];
        lv.H[i] = level_h[i];
        lv.W[i] = level_w[i];
    }
    const int K = 2 * radius + 1;
    const long long total = (long long)B * H * W * num_levels * K * K;
    int blocks = (int)min((total + 255) / 256, (long long)8192);
    hipLaunchKernelGGL(corr_lookup_nhwc_bwd_k, dim3(blocks), dim3(256), 0, s,
                       lv, coords, grad_out, H, W, num_levels, radius, total);
}

// bf16 2x2/2 avg pool (for the bf16 volume pyramid)
extern "C" __global__ void corr_pool2x_bf16_k(
    const __hip_bfloat16* __restrict__ in, __hip_bfloat16* __restrict__ out,
    int H, int W, int Ho, int Wo, long long total) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const int xo = (int)(idx % Wo);
        const int yo = (int)((idx / Wo) % Ho);
        const long long q = idx / ((long long)Wo * Ho);
        const __hip_bfloat16* src = in + (q * H + 2 * yo) * W + 2 * xo;
        out[idx] = (__hip_bfloat16)(0.25f * ((float)src[0] + (float)src[1] +
                                             (float)src[W] + (float)src[W + 1]));
    }
}

extern "C" void launch_corr_pool2x_bf16(const void* in, void* out, int H,
                                        int W, int Ho, int Wo,
                                        long long total, hipStream_t s) {
    int blocks = (int)min((total + 255) / 256, (long long)2048);
    hipLaunchKernelGGL(corr_pool2x_bf16_k, dim3(blocks), dim3(256), 0, s,
                       (const __hip_bfloat16*)in, (__hip_bfloat16*)out, H, W,
                       Ho, Wo, total);
}
