// Frame interpolation at time t from a bidirectional flow pair: the frame
// between im0 and im1, with the occlusion masks deciding which of the two
// frames a cell may draw from.
//
//   1. two nearest-source splats to time t (the rules of flow_project.hip,
//      targets p + t*fw[p] from frame 0 and p + (1-t)*bw[p] from frame 1),
//   2. per cell q the intermediate flows Ft0 (to frame 0) and Ft1 (to
//      frame 1): from the own splat's winner, else from the other splat's,
//      else the linear approximation from fw[q] and bw[q],
//   3. visibility from the masks at the cells nearest to q+Ft0 / q+Ft1,
//   4. a visibility-weighted blend of the two bilinear samples.
//
// Three stream-ordered nodes, no host sync, graph-capturable:
//   1. async memset of the [2,B,H,W] 64-bit key buffer to all-ones,
//   2. scatter: ONE launch over 2*B*H*W sources (first half splat A, second
//      half splat B), global 64-bit atomicMin of (float_bits(d2) << 32) |
//      source — the minimum does not depend on arrival order,
//   3. synthesis: one thread per output cell; keys, flows, visibility and
//      the eight corner indices / weights are computed once, the channel
//      loop is innermost over contiguous NCHW planes (x fastest across
//      lanes, so neighbouring lanes gather neighbouring addresses).
// Full resolution (~450k cells per image at 436x1024), bandwidth- and
// atomic-bound, no matrix work: grids are sized by the work, 64-bit indices.
//
// Mirrors raft_amd.ops.torch_ref.interpolate_frame BIT FOR BIT: every
// product and sum is rounded on its own (fp contraction is off in both
// kernels) and the final division is correctly rounded.

#include "common.h"

#define FI_EMPTY 0xFFFFFFFFFFFFFFFFull

__global__ void frame_interp_scatter_k(
    const float* __restrict__ fw,            // [B, 2, H, W]
    const float* __restrict__ bw,            // [B, 2, H, W]
    unsigned long long* __restrict__ keys,   // [2, B, H, W], preset to EMPTY
    int H, int W, float tf, long long half) {   // half = B*H*W
#pragma clang fp contract(off)
    const long long HW = (long long)H * W;
    const float u = 1.0f - tf;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const long long total = 2 * half;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const bool second = idx >= half;               // splat B
        const long long loc = second ? idx - half : idx;
        const long long b = loc / HW;
        const unsigned int src = (unsigned int)(loc - b * HW);   // y*W + x
        const int x = (int)(src % (unsigned int)W);
        const int y = (int)(src / (unsigned int)W);
        const float* f = (second ? bw : fw) + b * 2 * HW;
        const float s = second ? u : tf;
        const float fx = f[src], fy = f[src + HW];
        // one product and one add per coordinate
        const float tx = (float)x + s * fx;
        const float ty = (float)y + s * fy;
        // NaN / Inf fail the comparisons and are dropped
        if (!(tx >= 0.0f && tx <= xmax && ty >= 0.0f && ty <= ymax)) continue;
        const float x0f = floorf(tx), y0f = floorf(ty);
        const int x0 = (int)x0f, y0 = (int)y0f;       // in [0,W-1] x [0,H-1]
        unsigned long long* kb = keys + (second ? half : 0) + b * HW;
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

// Bilinear taps of torch_ref.fb_consistency: corners floor / floor+1, both
// clamped to the frame, weights clamped to [0,1]; NaN -> corner 0, weight 0
// (fmaxf / fminf drop NaN and keep huge values in range).
struct FiTap {
    long long i00, i01, i10, i11;
    float w00, w01, w10, w11;
};

RAFT_DEV FiTap fi_tap(float px, float py, int H, int W) {
#pragma clang fp contract(off)
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const float x0f = fminf(fmaxf(floorf(px), 0.0f), xmax);
    const float y0f = fminf(fmaxf(floorf(py), 0.0f), ymax);
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    const float ax = fminf(fmaxf(px - x0f, 0.0f), 1.0f);
    const float ay = fminf(fmaxf(py - y0f, 0.0f), 1.0f);
    FiTap t;
    t.w00 = (1.0f - ax) * (1.0f - ay);
    t.w01 = ax * (1.0f - ay);
    t.w10 = (1.0f - ax) * ay;
    t.w11 = ax * ay;
    t.i00 = (long long)y0 * W + x0;
    t.i01 = (long long)y0 * W + x1;
    t.i10 = (long long)y1 * W + x0;
    t.i11 = (long long)y1 * W + x1;
    return t;
}

// Cell nearest to (px, py): round half to even, clamped; NaN -> 0.
RAFT_DEV long long fi_nearest(float px, float py, int H, int W) {
    const float xr = fminf(fmaxf(rintf(px), 0.0f), (float)(W - 1));
    const float yr = fminf(fmaxf(rintf(py), 0.0f), (float)(H - 1));
    return (long long)(int)yr * W + (int)xr;
}

__global__ void frame_interp_synth_k(
    const float* __restrict__ im0,                 // [B, C, H, W]
    const float* __restrict__ im1,                 // [B, C, H, W]
    const float* __restrict__ fw,                  // [B, 2, H, W]
    const float* __restrict__ bw,                  // [B, 2, H, W]
    const unsigned char* __restrict__ occ_fw,      // [B, 1, H, W]
    const unsigned char* __restrict__ occ_bw,      // [B, 1, H, W]
    const unsigned long long* __restrict__ keys,   // [2, B, H, W]
    float* __restrict__ frame,                     // [B, C, H, W]
    float* __restrict__ flow_t0,                   // [B, 2, H, W]
    float* __restrict__ flow_t1,                   // [B, 2, H, W]
    unsigned char* __restrict__ cover,             // [B, 1, H, W]
    int C, int H, int W, float tf, long long half) {
#pragma clang fp contract(off)
    const long long HW = (long long)H * W;
    const float u = 1.0f - tf;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < half; idx += stride) {
        const long long b = idx / HW;
        const long long cell = idx - b * HW;
        const int x = (int)(cell % W);
        const int y = (int)(cell / W);
        const float* f = fw + b * 2 * HW;
        const float* g = bw + b * 2 * HW;

        const unsigned long long kA = keys[idx];
        const unsigned long long kB = keys[half + idx];
        const bool covA = kA != FI_EMPTY, covB = kB != FI_EMPTY;
        float gAx = 0.0f, gAy = 0.0f, gBx = 0.0f, gBy = 0.0f;
        if (covA) {
            const long long s = (long long)(kA & 0xFFFFFFFFull);
            gAx = f[s]; gAy = f[s + HW];
        }
        if (covB) {
            const long long s = (long long)(kB & 0xFFFFFFFFull);
            gBx = g[s]; gBy = g[s + HW];
        }

        float t0x, t0y, t1x, t1y;
        if (covA || covB) {
            if (covA) { t0x = (-tf) * gAx; t0y = (-tf) * gAy; }
            else      { t0x = tf * gBx;    t0y = tf * gBy; }
            if (covB) { t1x = (-u) * gBx;  t1y = (-u) * gBy; }
            else      { t1x = u * gAx;     t1y = u * gAy; }
        } else {
            // neither splat reached q: linear approximation at q itself
            const float fx = f[cell], fy = f[cell + HW];
            const float bx = g[cell], by = g[cell + HW];
            const float ut = u * tf, tt = tf * tf, uu = u * u;
            t0x = (-ut) * fx + tt * bx;
            t0y = (-ut) * fy + tt * by;
            t1x = uu * fx + (-ut) * bx;
            t1y = uu * fy + (-ut) * by;
        }
        flow_t0[b * 2 * HW + cell] = t0x;
        flow_t0[b * 2 * HW + cell + HW] = t0y;
        flow_t1[b * 2 * HW + cell] = t1x;
        flow_t1[b * 2 * HW + cell + HW] = t1y;
        cover[idx] = (unsigned char)((covA ? 1 : 0) | (covB ? 2 : 0));

        const float p0x = (float)x + t0x, p0y = (float)y + t0y;
        const float p1x = (float)x + t1x, p1y = (float)y + t1y;
        // NaN compares false -> outside
        const bool in0 = p0x >= 0.0f && p0x <= xmax && p0y >= 0.0f &&
                         p0y <= ymax;
        const bool in1 = p1x >= 0.0f && p1x <= xmax && p1y >= 0.0f &&
                         p1y <= ymax;
        const bool o0 = occ_fw[b * HW + fi_nearest(p0x, p0y, H, W)] != 0;
        const bool o1 = occ_bw[b * HW + fi_nearest(p1x, p1y, H, W)] != 0;
        float w0 = (in0 && !o1) ? u : 0.0f;
        float w1 = (in1 && !o0) ? tf : 0.0f;
        if (w0 + w1 == 0.0f) { w0 = u; w1 = tf; }
        const float wsum = w0 + w1;

        const FiTap a = fi_tap(p0x, p0y, H, W);
        const FiTap c = fi_tap(p1x, p1y, H, W);
        const float* s0 = im0 + b * C * HW;
        const float* s1 = im1 + b * C * HW;
        float* o = frame + b * C * HW + cell;
        for (int ch = 0; ch < C; ++ch) {
            const float v0 = ((a.w00 * s0[a.i00] + a.w01 * s0[a.i01]) +
                              a.w10 * s0[a.i10]) + a.w11 * s0[a.i11];
            const float v1 = ((c.w00 * s1[c.i00] + c.w01 * s1[c.i01]) +
                              c.w10 * s1[c.i10]) + c.w11 * s1[c.i11];
            *o = __fdiv_rn(w0 * v0 + w1 * v1, wsum);
            s0 += HW; s1 += HW; o += HW;
        }
    }
}

// Returns the first HIP error of the three nodes (hipSuccess = 0): with
// garbage keys the synthesis would gather from arbitrary sources, so the
// binding must not hand the result out after a failed memset.
extern "C" int launch_frame_interp(
    const float* im0, const float* im1, const float* fw, const float* bw,
    const unsigned char* occ_fw, const unsigned char* occ_bw,
    unsigned long long* keys, float* frame, float* flow_t0, float* flow_t1,
    unsigned char* cover, int B, int C, int H, int W, float tf,
    hipStream_t s) {
    const long long half = (long long)B * H * W;
    if (half == 0) return (int)hipSuccess;
    hipError_t err = hipMemsetAsync(
        keys, 0xFF, (size_t)(2 * half) * sizeof(unsigned long long), s);
    if (err != hipSuccess) return (int)err;
    // one source / one cell per thread up to the cap, grid-stride beyond
    const long long cap = 8192;
    const int sblocks = (int)min((2 * half + 255) / 256, cap);
    hipLaunchKernelGGL(frame_interp_scatter_k, dim3(sblocks), dim3(256), 0, s,
                       fw, bw, keys, H, W, tf, half);
    err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
    const int cblocks = (int)min((half + 255) / 256, cap);
    hipLaunchKernelGGL(frame_interp_synth_k, dim3(cblocks), dim3(256), 0, s,
                       im0, im1, fw, bw, occ_fw, occ_bw,
                       (const unsigned long long*)keys, frame, flow_t0,
                       flow_t1, cover, C, H, W, tf, half);
    return (int)hipGetLastError();
}
