// Forward-backward consistency (UnFlow / Meister et al. occlusion test):
// for each pixel of a flow f, sample the partner flow w at p + f (standard
// bilinear, edge-clamped) and flag the pixel occluded when it leaves the
// frame or |f + w|^2 > alpha1 * (|f|^2 + |w|^2) + alpha2.
//
// One launch covers both directions: the index space is [2B, H, W]; images
// b < B test the forward flow against the backward one, b >= B the reverse
// (partner = (b + B) % 2B). One thread per pixel, W fastest, grid-stride.
// Bandwidth-trivial (tens of MB at 1080p): no LDS tiling on purpose — its
// point is that masks leave the device in the same call as the flows.
// Mirrors raft_amd.ops.torch_ref.fb_consistency term by term.

#include "common.h"
#include <hip/hip_bf16.h>

template <typename T>
__global__ void fb_consistency_k(
    const T* __restrict__ fw,           // [B, 2, H, W]
    const T* __restrict__ bw,           // [B, 2, H, W]
    unsigned char* __restrict__ occ,    // [2B, 1, H, W]
    float* __restrict__ res_out,        // [2B, 1, H, W] or null
    float* __restrict__ bound_out,      // [2B, 1, H, W] or null
    int B, int H, int W, float alpha1, float alpha2, long long total) {
    const long long HW = (long long)H * W;
    const float xmax = (float)(W - 1), ymax = (float)(H - 1);
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
         idx < total; idx += stride) {
        const int x = (int)(idx % W);
        const int y = (int)((idx / W) % H);
        const int b2 = (int)(idx / HW);                 // 0 .. 2B-1
        const int b = b2 < B ? b2 : b2 - B;
        const T* self = (b2 < B ? fw : bw) + (long long)b * 2 * HW;
        const T* other = (b2 < B ? bw : fw) + (long long)b * 2 * HW;

        const long long pix = (long long)y * W + x;
        const float fx = (float)self[pix];
        const float fy = (float)self[pix + HW];
        const float px = (float)x + fx;
        const float py = (float)y + fy;
        // NaN compares false -> out of frame -> occluded
        const bool inb = px >= 0.0f && px <= xmax && py >= 0.0f && py <= ymax;

        // clamp in float before the int cast: fmaxf/fminf drop NaN and
        // keep huge values in range, so the corner indices are always valid
        const float x0f = fminf(fmaxf(floorf(px), 0.0f), xmax);
        const float y0f = fminf(fmaxf(floorf(py), 0.0f), ymax);
        const int x0 = (int)x0f, y0 = (int)y0f;
        const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
        const float ax = fminf(fmaxf(px - x0f, 0.0f), 1.0f);
        const float ay = fminf(fmaxf(py - y0f, 0.0f), 1.0f);
        const float w00 = (1.0f - ax) * (1.0f - ay), w01 = ax * (1.0f - ay);
        const float w10 = (1.0f - ax) * ay, w11 = ax * ay;

        const long long i00 = (long long)y0 * W + x0, i01 = (long long)y0 * W + x1;
        const long long i10 = (long long)y1 * W + x0, i11 = (long long)y1 * W + x1;
        const float wx = w00 * (float)other[i00] + w01 * (float)other[i01] +
                         w10 * (float)other[i10] + w11 * (float)other[i11];
        const float wy = w00 * (float)other[i00 + HW] +
                         w01 * (float)other[i01 + HW] +
                         w10 * (float)other[i10 + HW] +
                         w11 * (float)other[i11 + HW];

        const float sx = fx + wx, sy = fy + wy;
        const float res = sx * sx + sy * sy;
        const float bound =
            alpha1 * ((fx * fx + fy * fy) + (wx * wx + wy * wy)) + alpha2;
        occ[idx] = (!inb || res > bound) ? 1 : 0;
        if (res_out) res_out[idx] = res;
        if (bound_out) bound_out[idx] = bound;
    }
}

extern "C" void launch_fb_consistency(
    const void* fw, const void* bw, unsigned char* occ, float* res,
    float* bound, int bf16, int B, int H, int W, float alpha1, float alpha2,
    hipStream_t s) {
    const long long total = 2LL * B * H * W;
    if (total == 0) return;
    int blocks = (int)min((total + 255) / 256, (long long)2048);
    if (bf16)
        hipLaunchKernelGGL(fb_consistency_k<__hip_bfloat16>, dim3(blocks),
                           dim3(256), 0, s, (const __hip_bfloat16*)fw,
                           (const __hip_bfloat16*)bw, occ, res, bound, B, H,
                           W, alpha1, alpha2, total);
    else
        hipLaunchKernelGGL(fb_consistency_k<float>, dim3(blocks), dim3(256),
                           0, s, (const float*)fw, (const float*)bw, occ,
                           res, bound, B, H, W, alpha1, alpha2, total);
}
