// Residual of one refinement iteration (the convergence gate's measure):
// per sample, the largest squared coords update max_sq = max(dx*dx + dy*dy)
// over the 1/8-grid cells and the number of cells with !(d2 <= thr_sq).
//
// One thread per cell, grid (blocks per sample, B): a block never straddles
// two samples. The element strides of (sample, cell, component) are
// arguments, so the fused loop's interleaved [B,H8,W8,2] coords and the
// eager model's planar [B,2,H8,W8] coords both run without a copy.
//
// Reduction: d2 >= +0 or NaN, so its bit pattern with the sign cleared
// orders like the value under an unsigned max, with every NaN above +inf.
// Wave: shuffle max of the masked bits + population count of a 64-bit
// ballot. Block: the four wave partials through LDS. Grid: one 32-bit
// atomicMax and one 32-bit unsigned atomicAdd per block into the [B,2]
// int32 result. Integer atomics only: the result is independent of arrival
// order, so inference stays bit-reproducible.
//
// Two stream-ordered nodes, no host sync, graph-capturable: an async
// memset of the result, then the kernel.
//
// Mirrors raft_amd.ops.torch_ref.flow_residual BIT FOR BIT: the two
// products and the sum of d2 are rounded on their own (fp contraction off).

#include "common.h"

#define FR_THREADS 256
#define FR_WAVES (FR_THREADS / 64)

__global__ __launch_bounds__(FR_THREADS) void flow_residual_k(
    const float* __restrict__ prev, const float* __restrict__ nxt,
    unsigned int* __restrict__ result,   // [B, 2]: max_sq bits, above count
    int cells, long long s_b, long long s_cell, long long s_comp,
    float thr_sq) {
#pragma clang fp contract(off)
    __shared__ unsigned int w_max[FR_WAVES];
    __shared__ unsigned int w_cnt[FR_WAVES];
    const int b = blockIdx.y;
    const int cell = blockIdx.x * FR_THREADS + threadIdx.x;
    unsigned int bits = 0u;
    bool above = false;
    if (cell < cells) {
        const long long o = (long long)b * s_b + (long long)cell * s_cell;
        const float dx = nxt[o] - prev[o];
        const float dy = nxt[o + s_comp] - prev[o + s_comp];
        const float d2 = dx * dx + dy * dy;
        bits = __float_as_uint(d2) & 0x7fffffffu;
        above = !(d2 <= thr_sq);          // NaN is above
    }
    // the ballot spans the whole 64-wide wave; lanes past the grid vote 0
    const unsigned int cnt = (unsigned int)__popcll(__ballot(above));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
        bits = max(bits, (unsigned int)__shfl_xor((int)bits, off, 64));
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        w_max[wave] = bits;
        w_cnt[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int m = w_max[0], c = w_cnt[0];
#pragma unroll
        for (int w = 1; w < FR_WAVES; ++w) {
            m = max(m, w_max[w]);
            c += w_cnt[w];
        }
        atomicMax(result + 2 * b, m);
        atomicAdd(result + 2 * b + 1, c);
    }
}

// Returns the first HIP error of the two nodes (hipSuccess = 0): without
// the memset the atomics would fold into the previous call's result.
extern "C" int launch_flow_residual(
    const float* prev, const float* nxt, int* result, int B, int cells,
    long long s_b, long long s_cell, long long s_comp, float thr_sq,
    hipStream_t s) {
    if (B == 0) return (int)hipSuccess;
    hipError_t err = hipMemsetAsync(result, 0, (size_t)B * 2 * sizeof(int), s);
    if (err != hipSuccess || cells == 0) return (int)err;
    const int blocks = (cells + FR_THREADS - 1) / FR_THREADS;
    hipLaunchKernelGGL(flow_residual_k, dim3(blocks, B), dim3(FR_THREADS), 0,
                       s, prev, nxt, (unsigned int*)result, cells, s_b,
                       s_cell, s_comp, thr_sq);
    return (int)hipGetLastError();
}
