// Deterministic forward projection of a flow field (RAFT's warm start,
// forward_interpolate, as a nearest-source splat): every source cell p with
// flow f targets t = p + direction * f and is a candidate for the up-to-four
// integer cells around t; each cell keeps the value f of its nearest
// candidate (exact ties: lowest source index), cells with no candidate are
// holes filled from the nearest covered cells left/right/up/down.
//
// Three stream-ordered nodes, no host sync, graph-capturable:
//   1. async memset of the [B,H,W] 64-bit key buffer to all-ones,
//   2. scatter: global 64-bit atomicMin of (float_bits(d2) << 32) | source
//      (d2 >= +0, so its bit pattern orders like the value; the minimum is
//      independent of arrival order -> bit-reproducible),
//   3. resolve: one thread per cell, a gather for covered cells and four
//      scans for holes.
// The phases are ordered by kernel boundaries (no grid-wide barrier): the
// grids are 1/8-resolution flow fields, a few 10k cells, off the hot loop.
//
// Mirrors raft_amd.ops.torch_ref.forward_project BIT FOR BIT: every product
// and sum below is rounded on its own (fp contraction is off in both
// kernels) and the hole mean is a correctly rounded division.

#include "common.h"

#define FP_EMPTY 0xFFFFFFFFFFFFFFFFull

__global__ void flow_project_scatter_k(
    const float* __restrict__ flow,          // [B, 2, H, W]
    unsigned long long* __restrict__ keys,   // [B, H, W], preset to FP_EMPTY
    int H, int W, bool fwd, long long total) {
#pragma clang fp contract(off)
    const long long HW = (long long)H * W;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const long long b = idx / HW;
        const unsigned int src = (unsigned int)(idx - b * HW);   // y*W + x
        const int x = (int)(src % (unsigned int)W);
        const int y = (int)(src / (unsigned int)W);
        const float* f = flow + b * 2 * HW;
        const float fx = f[src], fy = f[src + HW];
        // one fp32 add (direction +1) or subtract (-1) per coordinate
        const float tx = fwd ? (float)x + fx : (float)x - fx;
        const float ty = fwd ? (float)y + fy : (float)y - fy;
        // NaN / Inf fail the comparisons and are dropped
        if (!(tx >= 0.0f && tx <= xmax && ty >= 0.0f && ty <= ymax)) continue;
        const float x0f = floorf(tx), y0f = floorf(ty);
        const int x0 = (int)x0f, y0 = (int)y0f;       // in [0,W-1] x [0,H-1]
        unsigned long long* kb = keys + b * HW;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const int qy = y0 + dy;
            if (qy > H - 1) continue;
            const float ddy = ty - (y0f + (float)dy);
            const float ddy2 = ddy * ddy;
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int qx = x0 + dx;
                if (qx > W - 1) continue;
                const float ddx = tx - (x0f + (float)dx);
                const float d2 = ddx * ddx + ddy2;
                const unsigned long long key =
                    ((unsigned long long)__float_as_uint(d2) << 32) | src;
                atomicMin(kb + (long long)qy * W + qx, key);
            }
        }
    }
}

__global__ void flow_project_resolve_k(
    const float* __restrict__ flow,                // [B, 2, H, W]
    const unsigned long long* __restrict__ keys,   // [B, H, W]
    float* __restrict__ out,                       // [B, 2, H, W]
    unsigned char* __restrict__ holes,             // [B, 1, H, W]
    int H, int W, long long total) {
#pragma clang fp contract(off)
    const long long HW = (long long)H * W;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const long long b = idx / HW;
        const long long cell = idx - b * HW;
        const int x = (int)(cell % W);
        const int y = (int)(cell / W);
        const float* f = flow + b * 2 * HW;
        const unsigned long long* kb = keys + b * HW;
        float* o = out + b * 2 * HW;
        const unsigned long long k = kb[cell];
        if (k != FP_EMPTY) {
            const long long src = (long long)(k & 0xFFFFFFFFull);
            o[cell] = f[src];
            o[cell + HW] = f[src + HW];
            holes[idx] = 0;
            continue;
        }
        // hole: nearest covered cell left, right, up, down (in that order)
        float sx = 0.0f, sy = 0.0f;
        int cnt = 0;
        long long hit;
        hit = -1;
        for (int xx = x - 1; xx >= 0; --xx)
            if (kb[(long long)y * W + xx] != FP_EMPTY) {
                hit = (long long)y * W + xx;
                break;
            }
        if (hit >= 0) {
            const long long s = (long long)(kb[hit] & 0xFFFFFFFFull);
            sx = sx + f[s]; sy = sy + f[s + HW]; ++cnt;
        }
        hit = -1;
        for (int xx = x + 1; xx < W; ++xx)
            if (kb[(long long)y * W + xx] != FP_EMPTY) {
                hit = (long long)y * W + xx;
                break;
            }
        if (hit >= 0) {
            const long long s = (long long)(kb[hit] & 0xFFFFFFFFull);
            sx = sx + f[s]; sy = sy + f[s + HW]; ++cnt;
        }
        hit = -1;
        for (int yy = y - 1; yy >= 0; --yy)
            if (kb[(long long)yy * W + x] != FP_EMPTY) {
                hit = (long long)yy * W + x;
                break;
            }
        if (hit >= 0) {
            const long long s = (long long)(kb[hit] & 0xFFFFFFFFull);
            sx = sx + f[s]; sy = sy + f[s + HW]; ++cnt;
        }
        hit = -1;
        for (int yy = y + 1; yy < H; ++yy)
            if (kb[(long long)yy * W + x] != FP_EMPTY) {
                hit = (long long)yy * W + x;
                break;
            }
        if (hit >= 0) {
            const long long s = (long long)(kb[hit] & 0xFFFFFFFFull);
            sx = sx + f[s]; sy = sy + f[s + HW]; ++cnt;
        }
        if (cnt > 0) {
            const float c = (float)cnt;
            sx = __fdiv_rn(sx, c);
            sy = __fdiv_rn(sy, c);
        }
        o[cell] = sx;
        o[cell + HW] = sy;
        holes[idx] = 1;
    }
}

// Returns the first HIP error of the three nodes (hipSuccess = 0): with
// garbage keys the resolve kernel would gather from arbitrary sources, so
// the binding must not hand the result out after a failed memset.
extern "C" int launch_flow_project(
    const float* flow, unsigned long long* keys, float* out,
    unsigned char* holes, int B, int H, int W, int direction,
    hipStream_t s) {
    const long long total = (long long)B * H * W;
    if (total == 0) return (int)hipSuccess;
    hipError_t err = hipMemsetAsync(
        keys, 0xFF, (size_t)total * sizeof(unsigned long long), s);
    if (err != hipSuccess) return (int)err;
    const int blocks = (int)min((total + 255) / 256, (long long)2048);
    hipLaunchKernelGGL(flow_project_scatter_k, dim3(blocks), dim3(256), 0, s,
                       flow, keys, H, W, direction > 0, total);
    err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(flow_project_resolve_k, dim3(blocks), dim3(256), 0, s,
                       flow, (const unsigned long long*)keys, out, holes, H,
                       W, total);
    return (int)hipGetLastError();
}
