// Torch bindings for the raft_amd gfx950 kernels (native HIP, no CUDA path).
// Host-side plumbing only: tensor checks, allocation, launch on the current
// HIP stream. Device code lives in the .hip files; each exposes an
// extern "C" launcher so this TU needs no cross-TU kernel symbols.
#include <torch/extension.h>
#include "lookup_conv_geom.h"

#include <ATen/hip/HIPContext.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <vector>

extern "C" {
void launch_corr_volume_f32(const float*, const float*, float*, int, int,
                            int, int, float, hipStream_t);
void launch_corr_pool2x_f32(const float*, float*, int, int, int, int,
                            long long, hipStream_t);
void launch_corr_lookup_fwd_f32(const float* const*, const int*, const int*,
                                const float*, float*, int, int, int, int,
                                int, hipStream_t);
void launch_corr_lookup_bwd_f32(float* const*, const int*, const int*,
                                const float*, const float*, int, int, int,
                                int, int, hipStream_t);
void launch_corr_lookup_bwd_wave_f32(float* const*, const int*, const int*,
                                     const float*, const void*, int, int,
                                     int, int, int, int, int, hipStream_t);
void launch_gru_gates_fwd_f32(const float*, const float*, const float*,
                              float*, long long, hipStream_t);
void launch_gru_gates_bwd_f32(const float*, const float*, const float*,
                              const float*, float*, float*, float*,
                              long long, hipStream_t);
void launch_gru_gates_fwd_bf16(const void*, const void*, const void*, void*,
                               long long, hipStream_t);
void launch_gru_gates_bwd_bf16(const void*, const void*, const void*,
                               const void*, void*, void*, void*, long long,
                               hipStream_t);
void launch_convex_upsample_fwd_bf16(const void*, const void*, float*, int,
                                     int, int, hipStream_t);
void launch_convex_upsample_bwd_bf16(const float*, const void*, const void*,
                                     float*, void*, int, int, int,
                                     hipStream_t);
void launch_convex_upsample_fwd_cl(const void*, const void*, float*, int,
                                   int, int, int, hipStream_t);
void launch_convex_upsample_bwd_cl(const float*, const void*, const void*,
                                   float*, void*, int, int, int, int,
                                   hipStream_t);
void launch_convex_upsample_fwd_f32(const float*, const float*, float*, int,
                                    int, int, hipStream_t);
void launch_convex_upsample_bwd_f32(const float*, const float*, const float*,
                                    float*, float*, int, int, int,
                                    hipStream_t);
void launch_quant_fp8(const void*, void*, const float*, long long,
                      hipStream_t);
void launch_corr_volume_nhwc_fp8(const void*, const void*, void*, int,
                                 const float*, const float*, int, int, int,
                                 int, float, hipStream_t);
void launch_corr_pool2x_fp8(const void*, void*, int, int, int, int,
                            long long, hipStream_t);
void launch_fconv_fp8_gru(const void*, int, const void*, int, const void*,
                          const float*, const float*, float, int, int, int,
                          int, int, int, int, const void*, const void*,
                          void*, void*, hipStream_t);
void launch_corr_volume_nhwc_bf16(const void*, const void*, void*, bool,
                                  int, int, int, int, float, hipStream_t);
void launch_corr_volume_nhwc_bidir(const void*, const void*, void*, int, int,
                                   int, float, hipStream_t);
void launch_fb_consistency(const void*, const void*, unsigned char*, float*,
                           float*, int, int, int, int, float, float,
                           hipStream_t);
int launch_flow_project(const float*, unsigned long long*, float*,
                        unsigned char*, int, int, int, int, hipStream_t);
int launch_flow_residual(const float*, const float*, int*, int, int,
                         long long, long long, long long, float, hipStream_t);
int launch_frame_interp(const float*, const float*, const float*,
                        const float*, const unsigned char*,
                        const unsigned char*, unsigned long long*, float*,
                        float*, float*, unsigned char*, int, int, int, int,
                        float, hipStream_t);
void launch_corr_lookup_nhwc(const void* const*, const int*, const int*,
                             int, const float*, const float*, void*, bool,
                             void*, int, int, int, int, int, int, int, int,
                             hipStream_t);
void launch_corr_lookup_nhwc_bwd(float* const*, const int*, const int*,
                                 const float*, const float*, int, int, int,
                                 int, int, hipStream_t);
void launch_corr_pool2x_bf16(const void*, void*, int, int, int, int,
                             long long, hipStream_t);
void launch_fconv_nhwc_bf16(const void*, int, int, int, const void*, int,
                            int, int, const void*, const float*, void*, int,
                            int, int, int, int, int, int, int, int, int,
                            const void*, const void*, void*, void*,
                            const float*, int, int, int, int, int,
                            hipStream_t);
void launch_inorm_stats(const void*, float*, float*, float*, int, int,
                        int, float, hipStream_t);
int inorm_stats_partitions(int);
void launch_inorm_apply(const void*, const float*, const float*,
                        const void*, void*, int, int, int, int,
                        hipStream_t);
void launch_fconv_smallk_nhwc_bf16(const void*, int, int, const void*,
                                   const float*, void*, int, int, int, int,
                                   int, int, int, int, int, hipStream_t);
void launch_fconv_dflow_coords(const void*, int, int, int, const void*,
                               const float*, const float*, float*, void*,
                               int, int, int, int, int, int, int,
                               hipStream_t);
void launch_flow_slice(const float*, void*, int, int, int, int, int,
                       hipStream_t);
int launch_corr_lookup_conv1x1(const void* const*, const int*, const int*,
                               int, const float*, const float*, const void*,
                               const float*, void*, int, int, int, int, int,
                               int, int, int, hipStream_t);
int launch_fconv_smallc_packed(const void*, int, int, const void*,
                               const float*, void*, int, int, int, int, int,
                               int, int, int, hipStream_t);
}

namespace {

hipStream_t current_stream() {
    return c10::hip::getCurrentHIPStream().stream();
}

#define CHECK_DEV(x) TORCH_CHECK((x).is_cuda(), #x " must be on GPU")
#define CHECK_CONT(x) TORCH_CHECK((x).is_contiguous(), #x " must be contiguous")

at::Tensor to_f32(const at::Tensor& t) {
    return t.scalar_type() == at::kFloat ? t : t.to(at::kFloat);
}

at::Tensor corr_volume(at::Tensor fmap1, at::Tensor fmap2) {
    CHECK_DEV(fmap1); CHECK_DEV(fmap2);
    CHECK_CONT(fmap1); CHECK_CONT(fmap2);
    TORCH_CHECK(fmap1.sizes() == fmap2.sizes(), "fmap shape mismatch");
    auto f1 = to_f32(fmap1);
    auto f2 = to_f32(fmap2);
    const int B = f1.size(0), C = f1.size(1), H = f1.size(2), W = f1.size(3);
    const int M = H * W;
    auto out = at::empty({B, M, H, W}, f1.options());
    launch_corr_volume_f32(f1.data_ptr<float>(), f2.data_ptr<float>(),
                           out.data_ptr<float>(), B, M, M, C,
                           1.0f / std::sqrt((float)C), current_stream());
    return out;
}

at::Tensor corr_pool2x(at::Tensor corr) {
    CHECK_DEV(corr); CHECK_CONT(corr);
    TORCH_CHECK(corr.scalar_type() == at::kFloat, "corr must be fp32");
    const int B = corr.size(0), Q = corr.size(1);
    const int H = corr.size(2), W = corr.size(3);
    const int Ho = H / 2, Wo = W / 2;
    auto out = at::empty({B, Q, Ho, Wo}, corr.options());
    const long long total = (long long)B * Q * Ho * Wo;
    launch_corr_pool2x_f32(corr.data_ptr<float>(), out.data_ptr<float>(), H,
                           W, Ho, Wo, total, current_stream());
    return out;
}

at::Tensor corr_lookup(std::vector<at::Tensor> levels, at::Tensor coords,
                       int64_t radius) {
    TORCH_CHECK(!levels.empty() && levels.size() <= 4, "1..4 pyramid levels");
    CHECK_DEV(coords); CHECK_CONT(coords);
    TORCH_CHECK(coords.scalar_type() == at::kFloat, "coords must be fp32");
    const int B = coords.size(0), H = coords.size(1), W = coords.size(2);
    const int L = (int)levels.size();
    const int K = 2 * (int)radius + 1;
    const float* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
    int hs[4] = {0}, ws[4] = {0};
    for (int i = 0; i < L; ++i) {
        CHECK_DEV(levels[i]); CHECK_CONT(levels[i]);
        TORCH_CHECK(levels[i].scalar_type() == at::kFloat,
                    "pyramid must be fp32");
        TORCH_CHECK(levels[i].size(1) == (int64_t)H * W,
                    "level query dim mismatch");
        ptrs[i] = levels[i].data_ptr<float>();
        hs[i] = levels[i].size(2);
        ws[i] = levels[i].size(3);
    }
    auto out = at::empty({B, (int64_t)L * K * K, H, W}, coords.options());
    launch_corr_lookup_fwd_f32(ptrs, hs, ws, coords.data_ptr<float>(),
                               out.data_ptr<float>(), B, H, W, L,
                               (int)radius, current_stream());
    return out;
}

std::vector<at::Tensor> corr_lookup_backward(
    at::Tensor grad_out, at::Tensor coords, int64_t radius,
    std::vector<std::vector<int64_t>> level_shapes, bool grads_bf16) {
    // grad_out may arrive as a permuted NHWC view (the r2 training path) —
    // each branch below lays it out as it needs
    CHECK_DEV(grad_out);
    CHECK_DEV(coords); CHECK_CONT(coords);
    const int B = coords.size(0), H = coords.size(1), W = coords.size(2);
    const int L = (int)level_shapes.size();
    std::vector<at::Tensor> grads;
    float* ptrs[4] = {nullptr, nullptr, nullptr, nullptr};
    int hs[4] = {0}, ws[4] = {0};
    const auto gdt = grads_bf16 ? at::kBFloat16 : at::kFloat;
    for (int i = 0; i < L; ++i) {
        grads.push_back(at::zeros(level_shapes[i],
                                  grad_out.options().dtype(gdt)));
        ptrs[i] = (float*)grads[i].data_ptr();
        hs[i] = (int)level_shapes[i][2];
        ws[i] = (int)level_shapes[i][3];
    }
    static const int flat = [] {
        const char* e = getenv("RAFT_AMD_LOOKUP_BWD_FLAT");
        return e ? atoi(e) : 0;
    }();
    if (!flat && radius <= 4) {
        // r2 wave-LDS backward (no global atomics); grad re-laid
        // tap-contiguous once (a free view when it came from the NHWC
        // training path), fp32 or bf16
        auto go = grad_out.reshape({B, -1, H, W})
                      .permute({0, 2, 3, 1}).contiguous();
        const bool gb = go.scalar_type() == at::kBFloat16;
        if (!gb) go = to_f32(go);
        launch_corr_lookup_bwd_wave_f32(ptrs, hs, ws,
                                        coords.data_ptr<float>(),
                                        go.data_ptr(), gb ? 1 : 0,
                                        grads_bf16 ? 1 : 0, B, H, W,
                                        L, (int)radius, current_stream());
        return grads;
    }
    TORCH_CHECK(!grads_bf16,
                "flat-atomic lookup backward supports fp32 grads only");
    auto go = to_f32(grad_out).contiguous();
    launch_corr_lookup_bwd_f32(ptrs, hs, ws, coords.data_ptr<float>(),
                               go.data_ptr<float>(), B, H, W, L, (int)radius,
                               current_stream());
    return grads;
}

static bool same_dense_layout(const at::Tensor& a, const at::Tensor& b,
                              const at::Tensor& c) {
    // elementwise kernels only need identical dense layouts — accepting
    // channels-last strides directly avoids a re-layout copy per call in
    // the training loop (r2)
    return a.is_non_overlapping_and_dense() &&
           b.is_non_overlapping_and_dense() &&
           c.is_non_overlapping_and_dense() &&
           a.strides() == b.strides() && a.strides() == c.strides() &&
           a.sizes() == b.sizes() && a.sizes() == c.sizes();
}

at::Tensor gru_gates_fwd(at::Tensor h, at::Tensor z, at::Tensor q) {
    CHECK_DEV(h);
    if (h.scalar_type() == at::kBFloat16 &&
        z.scalar_type() == at::kBFloat16 &&
        q.scalar_type() == at::kBFloat16 &&
        same_dense_layout(h, z, q)) {
        // r2: bf16-native path — the fp32-only binding cast every operand
        // around every autocast training call
        auto out = at::empty_like(h);
        launch_gru_gates_fwd_bf16(h.data_ptr(), z.data_ptr(), q.data_ptr(),
                                  out.data_ptr(), h.numel(),
                                  current_stream());
        return out;
    }
    auto hf = to_f32(h).contiguous();
    auto zf = to_f32(z).contiguous();
    auto qf = to_f32(q).contiguous();
    auto out = at::empty_like(hf);
    launch_gru_gates_fwd_f32(hf.data_ptr<float>(), zf.data_ptr<float>(),
                             qf.data_ptr<float>(), out.data_ptr<float>(),
                             hf.numel(), current_stream());
    return out.scalar_type() == h.scalar_type() ? out : out.to(h.scalar_type());
}

std::vector<at::Tensor> gru_gates_bwd(at::Tensor go, at::Tensor h,
                                      at::Tensor z, at::Tensor q) {
    if (go.scalar_type() == at::kBFloat16 &&
        h.scalar_type() == at::kBFloat16 &&
        z.scalar_type() == at::kBFloat16 &&
        q.scalar_type() == at::kBFloat16 &&
        same_dense_layout(go, h, z) && same_dense_layout(h, z, q)) {
        auto gh = at::empty_like(h);
        auto gz = at::empty_like(h);
        auto gq = at::empty_like(h);
        launch_gru_gates_bwd_bf16(go.data_ptr(), h.data_ptr(), z.data_ptr(),
                                  q.data_ptr(), gh.data_ptr(), gz.data_ptr(),
                                  gq.data_ptr(), h.numel(),
                                  current_stream());
        return {gh, gz, gq};
    }
    auto gof = to_f32(go).contiguous(); auto hf = to_f32(h).contiguous();
    auto zf = to_f32(z).contiguous(); auto qf = to_f32(q).contiguous();
    auto gh = at::empty_like(hf);
    auto gz = at::empty_like(hf);
    auto gq = at::empty_like(hf);
    launch_gru_gates_bwd_f32(gof.data_ptr<float>(), hf.data_ptr<float>(),
                             zf.data_ptr<float>(), qf.data_ptr<float>(),
                             gh.data_ptr<float>(), gz.data_ptr<float>(),
                             gq.data_ptr<float>(), hf.numel(),
                             current_stream());
    return {gh.to(h.scalar_type()), gz.to(z.scalar_type()),
            gq.to(q.scalar_type())};
}

at::Tensor convex_upsample(at::Tensor flow, at::Tensor mask) {
    CHECK_DEV(flow); CHECK_DEV(mask);
    const int B = flow.size(0), H = flow.size(2), W = flow.size(3);
    TORCH_CHECK(mask.size(1) == 576, "mask must have 64*9 channels");
    // output is ALWAYS fp32 (bf16 at 8x resolution quantizes large flows)
    auto out = at::empty({B, 2, 8 * H, 8 * W},
                         flow.options().dtype(at::kFloat));
    // channels-last fast path (training loop tensors): no re-layout, and
    // lane-contiguous mask reads
    if (mask.is_contiguous(at::MemoryFormat::ChannelsLast) &&
        mask.scalar_type() == flow.scalar_type()) {
        auto fcl = flow.contiguous(at::MemoryFormat::ChannelsLast);
        const bool bf = mask.scalar_type() == at::kBFloat16;
        if (bf || mask.scalar_type() == at::kFloat) {
            launch_convex_upsample_fwd_cl(fcl.data_ptr(), mask.data_ptr(),
                                          out.data_ptr<float>(), bf ? 1 : 0,
                                          B, H, W, current_stream());
            return out;
        }
    }
    flow = flow.contiguous();
    mask = mask.contiguous();
    if (mask.scalar_type() == at::kBFloat16) {
        // r2 bf16-native path: avoids casting the [B,576,H,W] mask (the
        // 2-channel flow cast is negligible)
        auto fb = flow.scalar_type() == at::kBFloat16
                      ? flow : flow.to(at::kBFloat16);
        launch_convex_upsample_fwd_bf16(fb.data_ptr(), mask.data_ptr(),
                                        out.data_ptr<float>(), B, H, W,
                                        current_stream());
        return out;
    }
    auto ff = to_f32(flow); auto mf = to_f32(mask);
    launch_convex_upsample_fwd_f32(ff.data_ptr<float>(), mf.data_ptr<float>(),
                                   out.data_ptr<float>(), B, H, W,
                                   current_stream());
    return out;
}

std::vector<at::Tensor> convex_upsample_backward(at::Tensor grad_up,
                                                 at::Tensor flow,
                                                 at::Tensor mask) {
    const int B = flow.size(0), H = flow.size(2), W = flow.size(3);
    auto gf = to_f32(grad_up).contiguous();
    if (mask.is_contiguous(at::MemoryFormat::ChannelsLast) &&
        mask.scalar_type() == flow.scalar_type() &&
        (mask.scalar_type() == at::kBFloat16 ||
         mask.scalar_type() == at::kFloat)) {
        auto fcl = flow.contiguous(at::MemoryFormat::ChannelsLast);
        const bool bf = mask.scalar_type() == at::kBFloat16;
        auto grad_flow = at::zeros({B, 2, H, W},
                                   flow.options().dtype(at::kFloat));
        auto grad_mask = at::empty_like(mask);   // keeps channels-last
        launch_convex_upsample_bwd_cl(gf.data_ptr<float>(), fcl.data_ptr(),
                                      mask.data_ptr(),
                                      grad_flow.data_ptr<float>(),
                                      grad_mask.data_ptr(), bf ? 1 : 0, B,
                                      H, W, current_stream());
        return {grad_flow.to(flow.scalar_type()), grad_mask};
    }
    if (mask.scalar_type() == at::kBFloat16 && mask.is_contiguous()) {
        auto fb = (flow.scalar_type() == at::kBFloat16
                       ? flow : flow.to(at::kBFloat16)).contiguous();
        auto grad_flow = at::zeros({B, 2, H, W},
                                   flow.options().dtype(at::kFloat));
        auto grad_mask = at::empty_like(mask);
        launch_convex_upsample_bwd_bf16(gf.data_ptr<float>(), fb.data_ptr(),
                                        mask.data_ptr(),
                                        grad_flow.data_ptr<float>(),
                                        grad_mask.data_ptr(), B, H, W,
                                        current_stream());
        return {grad_flow.to(flow.scalar_type()), grad_mask};
    }
    auto ff = to_f32(flow).contiguous();
    auto mf = to_f32(mask).contiguous();
    auto grad_flow = at::zeros_like(ff);
    auto grad_mask = at::empty_like(mf);
    launch_convex_upsample_bwd_f32(gf.data_ptr<float>(), ff.data_ptr<float>(),
                                   mf.data_ptr<float>(),
                                   grad_flow.data_ptr<float>(),
                                   grad_mask.data_ptr<float>(), B, H, W,
                                   current_stream());
    return {grad_flow.to(flow.scalar_type()), grad_mask.to(mask.scalar_type())};
}

// --------------------------------------------------------------- NHWC path
// Physical-NHWC tensors ([B,H,W,C] row-major) for the fused inference loop.

at::Tensor corr_volume_nhwc(at::Tensor f1, at::Tensor f2, bool out_bf16) {
    // f1/f2: physical NHWC [B, H, W, C] bf16, row-major contiguous
    CHECK_DEV(f1); CHECK_CONT(f1); CHECK_DEV(f2); CHECK_CONT(f2);
    TORCH_CHECK(f1.scalar_type() == at::kBFloat16, "nhwc volume needs bf16");
    TORCH_CHECK(f1.sizes() == f2.sizes());
    const int B = f1.size(0), H = f1.size(1), W = f1.size(2), C = f1.size(3);
    TORCH_CHECK(C % 64 == 0, "C must be a multiple of 64");
    const int M = H * W;
    auto out = at::empty({B, M, H, W},
                         f1.options().dtype(out_bf16 ? at::kBFloat16
                                                     : at::kFloat));
    launch_corr_volume_nhwc_bf16(f1.data_ptr(), f2.data_ptr(),
                                 out.data_ptr(), out_bf16, B, M, M, C,
                                 1.0f / std::sqrt((float)C),
                                 current_stream());
    return out;
}

at::Tensor corr_volume_nhwc_bidir(at::Tensor f1, at::Tensor f2) {
    // both directions from one GEMM: out[:B] is corr_volume_nhwc(f1, f2)
    // (bf16), out[B:] its exact transpose == the volume of (f2, f1)
    CHECK_DEV(f1); CHECK_CONT(f1); CHECK_DEV(f2); CHECK_CONT(f2);
    TORCH_CHECK(f1.scalar_type() == at::kBFloat16 &&
                f2.scalar_type() == at::kBFloat16, "nhwc volume needs bf16");
    TORCH_CHECK(f1.dim() == 4 && f1.sizes() == f2.sizes());
    const int B = f1.size(0), H = f1.size(1), W = f1.size(2), C = f1.size(3);
    TORCH_CHECK(C % 64 == 0, "C must be a multiple of 64");
    const int M = H * W;
    auto out = at::empty({2 * (int64_t)B, M, H, W}, f1.options());
    if (out.numel() == 0) return out;
    launch_corr_volume_nhwc_bidir(f1.data_ptr(), f2.data_ptr(),
                                  out.data_ptr(), B, M, C,
                                  1.0f / std::sqrt((float)C),
                                  current_stream());
    return out;
}

std::vector<at::Tensor> fb_consistency(at::Tensor flow_fw, at::Tensor flow_bw,
                                       double alpha1, double alpha2,
                                       bool return_terms) {
    // flows: [B,2,H,W] fp32 or bf16, NCHW-contiguous. Returns the uint8
    // masks [2B,1,H,W] (forward half, then backward half) and, on request,
    // the fp32 residual and bound of the same shape.
    CHECK_DEV(flow_fw); CHECK_DEV(flow_bw);
    CHECK_CONT(flow_fw); CHECK_CONT(flow_bw);
    TORCH_CHECK(flow_fw.dim() == 4 && flow_fw.size(1) == 2 &&
                flow_fw.sizes() == flow_bw.sizes(),
                "flows must both be [B,2,H,W]");
    TORCH_CHECK(flow_fw.scalar_type() == flow_bw.scalar_type() &&
                (flow_fw.scalar_type() == at::kFloat ||
                 flow_fw.scalar_type() == at::kBFloat16),
                "flows must both be fp32 or both bf16");
    const int B = flow_fw.size(0), H = flow_fw.size(2), W = flow_fw.size(3);
    auto occ = at::empty({2 * (int64_t)B, 1, H, W},
                         flow_fw.options().dtype(at::kByte));
    std::vector<at::Tensor> ret{occ};
    float* rp = nullptr;
    float* bp = nullptr;
    if (return_terms) {
        ret.push_back(at::empty({2 * (int64_t)B, 1, H, W},
                                flow_fw.options().dtype(at::kFloat)));
        ret.push_back(at::empty_like(ret[1]));
        rp = ret[1].data_ptr<float>();
        bp = ret[2].data_ptr<float>();
    }
    launch_fb_consistency(flow_fw.data_ptr(), flow_bw.data_ptr(),
                          occ.data_ptr<unsigned char>(), rp, bp,
                          flow_fw.scalar_type() == at::kBFloat16 ? 1 : 0, B,
                          H, W, (float)alpha1, (float)alpha2,
                          current_stream());
    return ret;
}

std::vector<at::Tensor> forward_project(at::Tensor flow, int64_t direction) {
    // flow: [B,2,H,W] fp32 NCHW-contiguous. Returns (projected [B,2,H,W]
    // fp32, holes [B,1,H,W] bool). Memset + two kernels on the current
    // stream; the key scratch buffer comes from the caching allocator, so
    // the call is capturable.
    CHECK_DEV(flow); CHECK_CONT(flow);
    TORCH_CHECK(flow.dim() == 4 && flow.size(1) == 2,
                "flow must be [B,2,H,W]");
    TORCH_CHECK(flow.scalar_type() == at::kFloat, "flow must be fp32");
    TORCH_CHECK(direction == 1 || direction == -1,
                "direction must be +1 or -1");
    const int64_t B = flow.size(0), H = flow.size(2), W = flow.size(3);
    // the source index shares a 64-bit key with the distance bits
    TORCH_CHECK(H * W < (int64_t(1) << 31), "H*W must be below 2^31");
    auto out = at::empty_like(flow);
    auto holes = at::empty({B, 1, H, W}, flow.options().dtype(at::kBool));
    if (flow.numel() == 0) return {out, holes};
    auto keys = at::empty({B, H, W}, flow.options().dtype(at::kLong));
    const int err = launch_flow_project(
        flow.data_ptr<float>(), (unsigned long long*)keys.data_ptr<int64_t>(),
        out.data_ptr<float>(), (unsigned char*)holes.data_ptr<bool>(), (int)B,
        (int)H, (int)W, (int)direction, current_stream());
    TORCH_CHECK(err == 0, "forward_project: ",
                hipGetErrorString((hipError_t)err));
    return {out, holes};
}

// flow_residual reads a logical [B,2,H,W] pair in place when both tensors
// share their strides and the H*W cells of a sample sit at one stride.
// The stride of a size-1 dim carries no meaning (contiguous() may leave
// any value there), so it is neither tested nor used.
bool residual_one_cell_stride(const at::Tensor& t) {
    const int64_t H = t.size(2), W = t.size(3);
    return H == 1 || W == 1 || t.stride(2) == W * t.stride(3);
}

int64_t residual_cell_stride(const at::Tensor& t) {
    return t.size(3) == 1 ? t.stride(2) : t.stride(3);
}

bool residual_same_layout(const at::Tensor& a, const at::Tensor& b) {
    // strides compared where they are used: sample, component, cell
    return (a.size(0) == 1 || a.stride(0) == b.stride(0)) &&
           a.stride(1) == b.stride(1) &&
           (a.size(2) * a.size(3) == 1 ||
            residual_cell_stride(a) == residual_cell_stride(b));
}

bool flow_residual_in_place(at::Tensor prev, at::Tensor nxt) {
    // True when flow_residual would read this pair without a copy.
    TORCH_CHECK(prev.dim() == 4 && prev.size(1) == 2,
                "prev must be [B,2,H,W]");
    TORCH_CHECK(prev.sizes() == nxt.sizes(), "prev and nxt differ in shape");
    return residual_same_layout(prev, nxt) &&
           residual_one_cell_stride(prev) && residual_one_cell_stride(nxt);
}

at::Tensor flow_residual(at::Tensor prev, at::Tensor nxt, double thr_sq,
                         c10::optional<at::Tensor> out) {
    // prev/nxt: logical [B,2,H,W] fp32 with equal strides whose cells sit
    // at one stride (planar NCHW, or the permuted view of an interleaved
    // [B,H,W,2] tensor): read in place. Returns the [B,2] int32 result —
    // column 0 the bits of max_sq, column 1 the count of cells above
    // thr_sq — written into `out` when given. Memset + one kernel on the
    // current stream: capturable, no host sync.
    CHECK_DEV(prev); CHECK_DEV(nxt);
    TORCH_CHECK(prev.dim() == 4 && prev.size(1) == 2,
                "prev must be [B,2,H,W]");
    TORCH_CHECK(prev.sizes() == nxt.sizes(), "prev and nxt differ in shape");
    TORCH_CHECK(prev.scalar_type() == at::kFloat &&
                nxt.scalar_type() == at::kFloat, "prev and nxt must be fp32");
    const int64_t B = prev.size(0), H = prev.size(2), W = prev.size(3);
    TORCH_CHECK(B <= 65535, "batch must fit the grid's y dimension");
    TORCH_CHECK(H * W < (int64_t(1) << 31), "H*W must be below 2^31");
    if (!flow_residual_in_place(prev, nxt)) {
        prev = prev.contiguous();
        nxt = nxt.contiguous();
    }
    at::Tensor res;
    if (out.has_value()) {
        res = *out;
        CHECK_DEV(res); CHECK_CONT(res);
        TORCH_CHECK(res.scalar_type() == at::kInt && res.dim() == 2 &&
                    res.size(0) == B && res.size(1) == 2,
                    "out must be [B,2] int32");
    } else {
        res = at::empty({B, 2}, prev.options().dtype(at::kInt));
    }
    const int err = launch_flow_residual(
        prev.data_ptr<float>(), nxt.data_ptr<float>(), res.data_ptr<int>(),
        (int)B, (int)(H * W), prev.stride(0), residual_cell_stride(prev),
        prev.stride(1),
        (float)thr_sq, current_stream());
    TORCH_CHECK(err == 0, "flow_residual: ",
                hipGetErrorString((hipError_t)err));
    return res;
}

std::vector<at::Tensor> interpolate_frame(at::Tensor im0, at::Tensor im1,
                                          at::Tensor fw, at::Tensor bw,
                                          at::Tensor occ_fw,
                                          at::Tensor occ_bw, double t) {
    // im0/im1: [B,C,H,W] fp32; fw/bw: [B,2,H,W] fp32; occ_*: [B,1,H,W]
    // uint8 (non-zero = occluded); all NCHW-contiguous on one device.
    // Returns (frame [B,C,H,W] fp32, flow_t0, flow_t1 [B,2,H,W] fp32,
    // cover [B,1,H,W] uint8: bit 0 splat A, bit 1 splat B). Memset + two
    // kernels on the current stream; the key scratch buffer comes from the
    // caching allocator, so the call is capturable.
    CHECK_DEV(im0); CHECK_DEV(im1); CHECK_DEV(fw); CHECK_DEV(bw);
    CHECK_DEV(occ_fw); CHECK_DEV(occ_bw);
    CHECK_CONT(im0); CHECK_CONT(im1); CHECK_CONT(fw); CHECK_CONT(bw);
    CHECK_CONT(occ_fw); CHECK_CONT(occ_bw);
    TORCH_CHECK(im0.dim() == 4 && im0.size(1) >= 1 &&
                im0.sizes() == im1.sizes(),
                "images must both be [B,C,H,W] with C >= 1");
    const int64_t B = im0.size(0), C = im0.size(1), H = im0.size(2),
                  W = im0.size(3);
    TORCH_CHECK(fw.dim() == 4 && fw.size(0) == B && fw.size(1) == 2 &&
                fw.size(2) == H && fw.size(3) == W &&
                fw.sizes() == bw.sizes(),
                "flows must both be [B,2,H,W] of the images' B, H, W");
    TORCH_CHECK(occ_fw.dim() == 4 && occ_fw.size(0) == B &&
                occ_fw.size(1) == 1 && occ_fw.size(2) == H &&
                occ_fw.size(3) == W && occ_fw.sizes() == occ_bw.sizes(),
                "masks must both be [B,1,H,W] of the images' B, H, W");
    TORCH_CHECK(im0.scalar_type() == at::kFloat &&
                im1.scalar_type() == at::kFloat &&
                fw.scalar_type() == at::kFloat &&
                bw.scalar_type() == at::kFloat,
                "images and flows must be fp32");
    TORCH_CHECK(occ_fw.scalar_type() == at::kByte &&
                occ_bw.scalar_type() == at::kByte, "masks must be uint8");
    const auto dev = im0.device();
    TORCH_CHECK(im1.device() == dev && fw.device() == dev &&
                bw.device() == dev && occ_fw.device() == dev &&
                occ_bw.device() == dev, "inputs must share one device");
    TORCH_CHECK(t >= 0.0 && t <= 1.0, "t must lie in [0, 1]");
    // the source index shares a 64-bit key with the distance bits
    TORCH_CHECK(H * W < (int64_t(1) << 31), "H*W must be below 2^31");
    auto frame = at::empty_like(im0);
    auto flow_t0 = at::empty_like(fw);
    auto flow_t1 = at::empty_like(fw);
    auto cover = at::empty({B, 1, H, W}, im0.options().dtype(at::kByte));
    if (B * H * W == 0) return {frame, flow_t0, flow_t1, cover};
    auto keys = at::empty({2, B, H, W}, im0.options().dtype(at::kLong));
    const int err = launch_frame_interp(
        im0.data_ptr<float>(), im1.data_ptr<float>(), fw.data_ptr<float>(),
        bw.data_ptr<float>(), occ_fw.data_ptr<unsigned char>(),
        occ_bw.data_ptr<unsigned char>(),
        (unsigned long long*)keys.data_ptr<int64_t>(),
        frame.data_ptr<float>(), flow_t0.data_ptr<float>(),
        flow_t1.data_ptr<float>(), cover.data_ptr<unsigned char>(), (int)B,
        (int)C, (int)H, (int)W, (float)t, current_stream());
    TORCH_CHECK(err == 0, "interpolate_frame: ",
                hipGetErrorString((hipError_t)err));
    return {frame, flow_t0, flow_t1, cover};
}

at::Tensor corr_volume_nhwc_fp8(at::Tensor f1, at::Tensor f2, bool out_bf16) {
    // fp8 e4m3 variant (r2): per-tensor software quantization + the MX
    // block-scaled MFMA with unit scales (~2.2x the bf16 MFMA rate).
    // amax stays on-device so the path is async/graph-capturable.
    CHECK_DEV(f1); CHECK_CONT(f1); CHECK_DEV(f2); CHECK_CONT(f2);
    TORCH_CHECK(f1.scalar_type() == at::kBFloat16, "fp8 volume needs bf16 in");
    TORCH_CHECK(f1.sizes() == f2.sizes());
    const int B = f1.size(0), H = f1.size(1), W = f1.size(2), C = f1.size(3);
    TORCH_CHECK(C % 128 == 0, "fp8 corr needs C % 128 == 0");
    const int M = H * W;
    auto amax1 = f1.abs().amax().to(at::kFloat).contiguous();
    auto amax2 = f2.abs().amax().to(at::kFloat).contiguous();
    auto q1 = at::empty({B, M, C}, f1.options().dtype(at::kByte));
    auto q2 = at::empty({B, M, C}, f1.options().dtype(at::kByte));
    launch_quant_fp8(f1.data_ptr(), q1.data_ptr(),
                     amax1.data_ptr<float>(), (long long)B * M * C,
                     current_stream());
    launch_quant_fp8(f2.data_ptr(), q2.data_ptr(),
                     amax2.data_ptr<float>(), (long long)B * M * C,
                     current_stream());
    auto out = at::empty({B, M, H, W},
                         f1.options().dtype(out_bf16 ? at::kBFloat16
                                                     : at::kFloat));
    launch_corr_volume_nhwc_fp8(q1.data_ptr(), q2.data_ptr(), out.data_ptr(),
                                out_bf16 ? 1 : 0, amax1.data_ptr<float>(),
                                amax2.data_ptr<float>(), B, M, M, C,
                                1.0f / std::sqrt((float)C),
                                current_stream());
    return out;
}

std::vector<at::Tensor> corr_volume_nhwc_fp8s(at::Tensor f1, at::Tensor f2) {
    // fp8 GEMM with fp8 e4m3 VOLUME STORAGE (r2 roadmap #4): returns
    // (uint8 volume [B,M,H,W], vol_scale scalar) where true corr =
    // decode(byte) * vol_scale, vol_scale = sqrt(c)*amax1*amax2/448.
    CHECK_DEV(f1); CHECK_CONT(f1); CHECK_DEV(f2); CHECK_CONT(f2);
    TORCH_CHECK(f1.scalar_type() == at::kBFloat16, "fp8 volume needs bf16 in");
    TORCH_CHECK(f1.sizes() == f2.sizes());
    const int B = f1.size(0), H = f1.size(1), W = f1.size(2), C = f1.size(3);
    TORCH_CHECK(C % 128 == 0, "fp8 corr needs C % 128 == 0");
    const int M = H * W;
    auto amax1 = f1.abs().amax().to(at::kFloat).contiguous();
    auto amax2 = f2.abs().amax().to(at::kFloat).contiguous();
    auto q1 = at::empty({B, M, C}, f1.options().dtype(at::kByte));
    auto q2 = at::empty({B, M, C}, f1.options().dtype(at::kByte));
    launch_quant_fp8(f1.data_ptr(), q1.data_ptr(),
                     amax1.data_ptr<float>(), (long long)B * M * C,
                     current_stream());
    launch_quant_fp8(f2.data_ptr(), q2.data_ptr(),
                     amax2.data_ptr<float>(), (long long)B * M * C,
                     current_stream());
    auto out = at::empty({B, M, H, W}, f1.options().dtype(at::kByte));
    launch_corr_volume_nhwc_fp8(q1.data_ptr(), q2.data_ptr(), out.data_ptr(),
                                2, amax1.data_ptr<float>(),
                                amax2.data_ptr<float>(), B, M, M, C,
                                1.0f / std::sqrt((float)C),
                                current_stream());
    auto vol_scale = (amax1 * amax2 *
                      (std::sqrt((float)C) / 448.0f)).contiguous();
    return {out, vol_scale};
}

at::Tensor quant_fp8(at::Tensor t, at::Tensor amax) {
    // bf16 -> e4m3 with scale 448/amax (device scalar); same shape, uint8
    CHECK_DEV(t); CHECK_CONT(t);
    TORCH_CHECK(t.scalar_type() == at::kBFloat16, "quant_fp8 needs bf16");
    auto out = at::empty_like(t, t.options().dtype(at::kByte));
    launch_quant_fp8(t.data_ptr(), out.data_ptr(), amax.data_ptr<float>(),
                     (long long)t.numel(), current_stream());
    return out;
}

std::vector<at::Tensor> fconv_fp8_gru_zr(at::Tensor h8, at::Tensor x8,
                                         at::Tensor h_bf, at::Tensor w8,
                                         at::Tensor bias, at::Tensor ax,
                                         double aw, int64_t kh, int64_t kw) {
    // h8/x8: [B,H,W,C] uint8 e4m3; h_bf: [B,H,W,hd] bf16 (for rh=sig(r)*h)
    // w8: [taps][2hd][C1+C2] uint8; returns (z bf16 [B,H,W,hd], rh8 uint8)
    CHECK_DEV(h8); CHECK_CONT(h8); CHECK_CONT(x8); CHECK_CONT(h_bf);
    const int B = h8.size(0), H = h8.size(1), W = h8.size(2);
    const int C1 = h8.size(3), C2 = x8.size(3);
    const int N = w8.size(1), hd = N / 2;
    TORCH_CHECK(C1 % 128 == 0 && C2 % 128 == 0, "fp8 GRU needs C%128==0");
    auto z = at::empty({B, H, W, hd}, h_bf.options());
    auto rh8 = at::empty({B, H, W, hd}, h8.options());
    launch_fconv_fp8_gru(h8.data_ptr(), C1, x8.data_ptr(), C2, w8.data_ptr(),
                         bias.data_ptr<float>(), ax.data_ptr<float>(),
                         (float)aw, B, H, W, N, (int)kh, (int)kw, 1,
                         h_bf.data_ptr(), nullptr, z.data_ptr(),
                         rh8.data_ptr(), current_stream());
    return {z, rh8};
}

at::Tensor fconv_fp8_gru_q(at::Tensor rh8, at::Tensor x8, at::Tensor w8,
                           at::Tensor bias, at::Tensor ax, double aw,
                           int64_t kh, int64_t kw, at::Tensor z,
                           at::Tensor h_bf) {
    CHECK_DEV(rh8); CHECK_CONT(rh8); CHECK_CONT(x8); CHECK_CONT(z);
    const int B = rh8.size(0), H = rh8.size(1), W = rh8.size(2);
    const int C1 = rh8.size(3), C2 = x8.size(3);
    const int N = w8.size(1);
    TORCH_CHECK(C1 % 128 == 0 && C2 % 128 == 0, "fp8 GRU needs C%128==0");
    auto out = at::empty({B, H, W, N}, h_bf.options());
    launch_fconv_fp8_gru(rh8.data_ptr(), C1, x8.data_ptr(), C2,
                         w8.data_ptr(), bias.data_ptr<float>(),
                         ax.data_ptr<float>(), (float)aw, B, H, W, N,
                         (int)kh, (int)kw, 2, h_bf.data_ptr(), z.data_ptr(),
                         out.data_ptr(), nullptr, current_stream());
    return out;
}

at::Tensor corr_pool2x_fp8(at::Tensor corr) {
    CHECK_DEV(corr); CHECK_CONT(corr);
    TORCH_CHECK(corr.scalar_type() == at::kByte);
    const int B = corr.size(0), Q = corr.size(1);
    const int H = corr.size(2), W = corr.size(3);
    const int Ho = H / 2, Wo = W / 2;
    auto out = at::empty({B, Q, Ho, Wo}, corr.options());
    launch_corr_pool2x_fp8(corr.data_ptr(), out.data_ptr(), H, W, Ho, Wo,
                           (long long)B * Q * Ho * Wo, current_stream());
    return out;
}

at::Tensor corr_pool2x_bf16(at::Tensor corr) {
    CHECK_DEV(corr); CHECK_CONT(corr);
    TORCH_CHECK(corr.scalar_type() == at::kBFloat16);
    const int B = corr.size(0), Q = corr.size(1);
    const int H = corr.size(2), W = corr.size(3);
    const int Ho = H / 2, Wo = W / 2;
    auto out = at::empty({B, Q, Ho, Wo}, corr.options());
    launch_corr_pool2x_bf16(corr.data_ptr(), out.data_ptr(), H, W, Ho, Wo,
                            (long long)B * Q * Ho * Wo, current_stream());
    return out;
}

at::Tensor corr_lookup_nhwc(std::vector<at::Tensor> levels,
                            at::Tensor coords, int64_t radius,
                            int64_t c_stride, bool out_bf16,
                            c10::optional<at::Tensor> out_buf,
                            c10::optional<at::Tensor> flow_buf,
                            int64_t flow_off,
                            c10::optional<at::Tensor> vol_scale) {
    // coords: [B, H, W, 2] fp32; returns physical NHWC [B, H, W, c_stride]
    // with channels [L*KK..c_stride) zero-filled (pad for fconv Cin%8).
    CHECK_DEV(coords); CHECK_CONT(coords);
    TORCH_CHECK(!levels.empty() && levels.size() <= 4, "1..4 pyramid levels");
    const int B = coords.size(0), H = coords.size(1), W = coords.size(2);
    const int L = (int)levels.size();
    const int K = 2 * (int)radius + 1;
    const int C = L * K * K;
    TORCH_CHECK(c_stride >= C);
    const void* ptrs[4];
    int hs[4] = {0}, ws[4] = {0};
    int vol_type = 0;
    if (levels[0].scalar_type() == at::kBFloat16) vol_type = 1;
    else if (levels[0].scalar_type() == at::kByte) vol_type = 2;
    const float* vsp = nullptr;
    if (vol_type == 2) {
        TORCH_CHECK(vol_scale.has_value(),
                    "fp8 volume lookup needs vol_scale");
        vsp = vol_scale->data_ptr<float>();
    }
    for (int i = 0; i < L; ++i) {
        CHECK_DEV(levels[i]); CHECK_CONT(levels[i]);
        ptrs[i] = levels[i].data_ptr();
        hs[i] = levels[i].size(2);
        ws[i] = levels[i].size(3);
    }
    // pad channels [C..c_stride) must be zero for the consumer's padded
    // weights; zero-fill once per call only when padded (kernel writes the
    // first C channels of every row with the Cs stride).
    auto opts = coords.options().dtype(out_bf16 ? at::kBFloat16
                                                 : at::kFloat);
    at::Tensor out;
    if (out_buf.has_value()) {
        out = out_buf.value();   // caller owns pad-channel zeroing
        TORCH_CHECK(out.is_contiguous() && out.size(3) == c_stride);
    } else {
        out = (c_stride == C)
            ? at::empty({B, H, W, (int64_t)c_stride}, opts)
            : at::zeros({B, H, W, (int64_t)c_stride}, opts);
    }
    void* fptr = nullptr;
    int fstride = 2;
    if (flow_buf.has_value()) {
        TORCH_CHECK(flow_buf->is_contiguous() &&
                    flow_buf->scalar_type() == at::kBFloat16);
        fptr = flow_buf->data_ptr();
        fstride = (int)flow_buf->size(3);
    }
    launch_corr_lookup_nhwc(ptrs, hs, ws, vol_type, vsp,
                            coords.data_ptr<float>(), out.data_ptr(),
                            out_bf16, fptr, fstride, (int)flow_off, B, H, W,
                            L, (int)radius, (int)c_stride,
                            current_stream());
    return out;
}

at::Tensor fconv_plain(at::Tensor in1, c10::optional<at::Tensor> in2,
                       at::Tensor wp, c10::optional<at::Tensor> bias,
                       int64_t kh, int64_t kw, int64_t act,
                       c10::optional<at::Tensor> out_buf, int64_t n_off,
                       int64_t in1_off, int64_t in1_len,
                       int64_t alltaps, int64_t mtiles, int64_t stride,
                       c10::optional<at::Tensor> res) {
    CHECK_DEV(in1); CHECK_CONT(in1); CHECK_DEV(wp); CHECK_CONT(wp);
    TORCH_CHECK(in1.scalar_type() == at::kBFloat16, "fconv needs bf16");
    const int B = in1.size(0), H = in1.size(1), W = in1.size(2);
    const int in1_stride = in1.size(3);
    const int C1 = in1_len > 0 ? (int)in1_len : in1_stride;
    TORCH_CHECK(in1_off + C1 <= in1_stride);
    const void* p2 = nullptr;
    int C2 = 0;
    if (in2.has_value()) {
        CHECK_CONT(in2.value());
        p2 = in2->data_ptr();
        C2 = in2->size(3);
    }
    const int N = wp.size(1);
    TORCH_CHECK(wp.size(0) == kh * kw && wp.size(2) == C1 + C2,
                "packed weight shape mismatch");
    const float* bptr = nullptr;
    if (bias.has_value()) {
        TORCH_CHECK(bias->scalar_type() == at::kFloat);
        bptr = bias->data_ptr<float>();
    }
    if (stride == 1) {
        TORCH_CHECK((kh == 1 && kw == 1) || (kh == 3 && kw == 3) ||
                    (kh == 1 && kw == 5) || (kh == 5 && kw == 1),
                    "fconv: unsupported kernel shape ", kh, "x", kw,
                    " (use fconv_smallk for tiny-Cin large kernels)");
    } else {
        TORCH_CHECK(stride == 2 && kh == kw &&
                    (kh == 1 || kh == 3 || kh == 7),
                    "fconv stride-2 supports 1x1/3x3/7x7");
        TORCH_CHECK(H % 2 == 0 && W % 2 == 0,
                    "stride-2 fconv needs even input dims");
    }
    const int Ho = (stride == 2) ? H / 2 : H;
    const int Wo = (stride == 2) ? W / 2 : W;
    const void* res_ptr = nullptr;
    int mode = 0;
    if (res.has_value()) {
        CHECK_CONT(res.value());
        TORCH_CHECK(res->size(3) == N, "residual channel mismatch");
        res_ptr = res->data_ptr();
        mode = 3;   // EP_RES_RELU: out = relu(res + relu(v))
    }
    at::Tensor out;
    int cstride;
    if (out_buf.has_value()) {
        out = out_buf.value();
        CHECK_CONT(out);
        cstride = out.size(3);
    } else {
        out = at::empty({B, Ho, Wo, N}, in1.options());
        cstride = N;
        n_off = 0;
    }
    launch_fconv_nhwc_bf16(in1.data_ptr(), C1, in1_stride, (int)in1_off,
                           p2, C2, C2, 0, wp.data_ptr(), bptr,
                           out.data_ptr(), B, Ho, Wo, N, (int)n_off, cstride,
                           (int)kh, (int)kw, (int)act, mode, res_ptr,
                           nullptr, nullptr, nullptr, nullptr, 0, 0,
                           (int)alltaps, (int)mtiles, (int)stride,
                           current_stream());
    return out;
}

std::vector<at::Tensor> fconv_gru_zr(at::Tensor h, at::Tensor x,
                                     at::Tensor wp, at::Tensor bias,
                                     int64_t kh, int64_t kw) {
    CHECK_DEV(h); CHECK_CONT(h); CHECK_CONT(x); CHECK_CONT(wp);
    const int B = h.size(0), H = h.size(1), W = h.size(2), hd = h.size(3);
    const int N = wp.size(1);
    TORCH_CHECK(N == 2 * hd, "zr weights must stack [Wz; Wr]");
    auto z = at::empty_like(h);
    auto rh = at::empty_like(h);
    launch_fconv_nhwc_bf16(h.data_ptr(), hd, hd, 0, x.data_ptr(),
                           x.size(3), x.size(3), 0, wp.data_ptr(),
                           bias.data_ptr<float>(), nullptr, B, H, W, N, 0, 0,
                           (int)kh, (int)kw, 0, 1, h.data_ptr(), nullptr,
                           z.data_ptr(), rh.data_ptr(), nullptr, 0, 0, -1,
                           -1, 1, current_stream());
    return {z, rh};
}

at::Tensor fconv_gru_q(at::Tensor rh, at::Tensor x, at::Tensor wp,
                       at::Tensor bias, int64_t kh, int64_t kw, at::Tensor z,
                       at::Tensor h) {
    CHECK_DEV(rh); CHECK_CONT(rh); CHECK_CONT(x); CHECK_CONT(wp);
    CHECK_CONT(z); CHECK_CONT(h);
    const int B = rh.size(0), H = rh.size(1), W = rh.size(2);
    const int hd = rh.size(3);
    TORCH_CHECK(wp.size(1) == hd);
    auto out = at::empty_like(h);
    launch_fconv_nhwc_bf16(rh.data_ptr(), hd, hd, 0, x.data_ptr(),
                           x.size(3), x.size(3), 0, wp.data_ptr(),
                           bias.data_ptr<float>(), out.data_ptr(), B, H, W,
                           hd, 0, hd, (int)kh, (int)kw, 0, 2, h.data_ptr(),
                           z.data_ptr(), nullptr, nullptr, nullptr, 0, 0,
                           -1, -1, 1, current_stream());
    return out;
}

// ---- GRU convs with the constant part of the input hoisted out.
// x = [inp | rest]: conv([h | x]) = conv([h | rest]) + conv(inp), and inp
// (the context features) is the same in every refinement iteration. The
// second term is computed once (fconv_plain_f32, bias included) and handed
// in as `pre`; the per-iteration conv reads the rest slice of x in place.

// fp32 conv output, no activation: [B,H,W,N] float
at::Tensor fconv_plain_f32(at::Tensor in1, at::Tensor wp,
                           c10::optional<at::Tensor> bias, int64_t kh,
                           int64_t kw, int64_t in1_off, int64_t in1_len) {
    CHECK_DEV(in1); CHECK_CONT(in1); CHECK_DEV(wp); CHECK_CONT(wp);
    TORCH_CHECK(in1.scalar_type() == at::kBFloat16 &&
                wp.scalar_type() == at::kBFloat16, "fconv needs bf16");
    TORCH_CHECK((kh == 1 && kw == 1) || (kh == 3 && kw == 3) ||
                (kh == 1 && kw == 5) || (kh == 5 && kw == 1),
                "fconv: unsupported kernel shape ", kh, "x", kw);
    const int B = in1.size(0), H = in1.size(1), W = in1.size(2);
    const int in1_stride = in1.size(3);
    const int C1 = in1_len > 0 ? (int)in1_len : in1_stride;
    TORCH_CHECK(in1_off >= 0 && in1_off % 8 == 0 &&
                in1_off + C1 <= in1_stride, "in1 slice out of bounds or "
                "not 16-byte aligned");
    const int N = wp.size(1);
    TORCH_CHECK(wp.size(0) == kh * kw && wp.size(2) == C1,
                "packed weight shape mismatch");
    const float* bptr = nullptr;
    if (bias.has_value()) {
        CHECK_DEV(bias.value()); CHECK_CONT(bias.value());
        TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == N);
        bptr = bias->data_ptr<float>();
    }
    auto out = at::empty({B, H, W, N}, in1.options().dtype(at::kFloat));
    launch_fconv_nhwc_bf16(in1.data_ptr(), C1, in1_stride, (int)in1_off,
                           nullptr, 0, 0, 0, wp.data_ptr(), bptr,
                           out.data_ptr(), B, H, W, N, 0, N, (int)kh, (int)kw,
                           0, 4 /* EP_PLAIN_F32 */, nullptr, nullptr, nullptr,
                           nullptr, nullptr, 0, 0, -1, -1, 1,
                           current_stream());
    return out;
}

// shared argument checks of the two hoisted GRU convs; N = output channels
static void check_gru_pre(const at::Tensor& h, const at::Tensor& x,
                          const at::Tensor& wp, const at::Tensor& pre,
                          int64_t pre_off, int64_t x_off, int64_t x_len,
                          int64_t N) {
    TORCH_CHECK(h.scalar_type() == at::kBFloat16 &&
                x.scalar_type() == at::kBFloat16 &&
                wp.scalar_type() == at::kBFloat16, "fconv needs bf16");
    TORCH_CHECK(x.dim() == 4 && x.size(0) == h.size(0) &&
                x.size(1) == h.size(1) && x.size(2) == h.size(2),
                "x and h disagree in B/H/W");
    TORCH_CHECK(x_off % 8 == 0, "x_off must be a multiple of 8 (16-byte "
                "vector loads), got ", x_off);
    TORCH_CHECK(x_off >= 0 && x_len > 0 && x_off + x_len <= x.size(3),
                "x slice [", x_off, ", ", x_off + x_len, ") exceeds ",
                x.size(3), " channels");
    TORCH_CHECK(wp.size(2) == h.size(3) + x_len,
                "packed weight must have hd + x_len input channels");
    CHECK_DEV(pre);
    TORCH_CHECK(pre.scalar_type() == at::kFloat, "pre must be fp32");
    TORCH_CHECK(pre.is_contiguous(), "pre must be contiguous");
    TORCH_CHECK(pre.dim() == 4 && pre.size(0) == h.size(0) &&
                pre.size(1) == h.size(1) && pre.size(2) == h.size(2),
                "pre and h disagree in B/H/W");
    TORCH_CHECK(pre_off >= 0 && pre_off + N <= pre.size(3),
                "pre_off + N = ", pre_off + N, " exceeds pre's ",
                pre.size(3), " channels");
}

std::vector<at::Tensor> fconv_gru_zr_pre(at::Tensor h, at::Tensor x,
                                         at::Tensor wp, int64_t kh,
                                         int64_t kw, at::Tensor pre,
                                         int64_t pre_off, int64_t x_off,
                                         int64_t x_len) {
    CHECK_DEV(h); CHECK_CONT(h); CHECK_CONT(x); CHECK_CONT(wp);
    const int B = h.size(0), H = h.size(1), W = h.size(2), hd = h.size(3);
    const int N = wp.size(1);
    TORCH_CHECK(N == 2 * hd, "zr weights must stack [Wz; Wr]");
    check_gru_pre(h, x, wp, pre, pre_off, x_off, x_len, N);
    auto z = at::empty_like(h);
    auto rh = at::empty_like(h);
    launch_fconv_nhwc_bf16(h.data_ptr(), hd, hd, 0, x.data_ptr(), (int)x_len,
                           (int)x.size(3), (int)x_off, wp.data_ptr(),
                           nullptr, nullptr, B, H, W, N, 0, 0, (int)kh,
                           (int)kw, 0, 1, h.data_ptr(), nullptr,
                           z.data_ptr(), rh.data_ptr(),
                           pre.data_ptr<float>(), (int)pre.size(3),
                           (int)pre_off, -1, -1, 1, current_stream());
    return {z, rh};
}

at::Tensor fconv_gru_q_pre(at::Tensor rh, at::Tensor x, at::Tensor wp,
                           int64_t kh, int64_t kw, at::Tensor z, at::Tensor h,
                           at::Tensor pre, int64_t pre_off, int64_t x_off,
                           int64_t x_len) {
    CHECK_DEV(rh); CHECK_CONT(rh); CHECK_CONT(x); CHECK_CONT(wp);
    CHECK_CONT(z); CHECK_CONT(h);
    const int B = rh.size(0), H = rh.size(1), W = rh.size(2);
    const int hd = rh.size(3);
    TORCH_CHECK(wp.size(1) == hd);
    check_gru_pre(rh, x, wp, pre, pre_off, x_off, x_len, hd);
    auto out = at::empty_like(h);
    launch_fconv_nhwc_bf16(rh.data_ptr(), hd, hd, 0, x.data_ptr(),
                           (int)x_len, (int)x.size(3), (int)x_off,
                           wp.data_ptr(), nullptr, out.data_ptr(), B, H, W,
                           hd, 0, hd, (int)kh, (int)kw, 0, 2, h.data_ptr(),
                           z.data_ptr(), nullptr, nullptr,
                           pre.data_ptr<float>(), (int)pre.size(3),
                           (int)pre_off, -1, -1, 1, current_stream());
    return out;
}

at::Tensor fconv_smallk(at::Tensor in1, at::Tensor wp,
                        c10::optional<at::Tensor> bias, int64_t kh,
                        int64_t kw, int64_t act, int64_t in1_off,
                        int64_t in1_len, int64_t conv_stride) {
    CHECK_DEV(in1); CHECK_CONT(in1); CHECK_CONT(wp);
    const int B = in1.size(0), H = in1.size(1), W = in1.size(2);
    const int stride = in1.size(3);
    const int C = in1_len > 0 ? (int)in1_len : stride;
    const int N = wp.size(1);
    const float* bptr = bias.has_value() ? bias->data_ptr<float>() : nullptr;
    const int Ho = (int)(H / conv_stride), Wo = (int)(W / conv_stride);
    TORCH_CHECK(conv_stride == 1 ||
                (conv_stride == 2 && H % 2 == 0 && W % 2 == 0));
    auto out = at::empty({B, Ho, Wo, N}, in1.options());
    launch_fconv_smallk_nhwc_bf16(in1.data_ptr(), stride, (int)in1_off,
                                  wp.data_ptr(), bptr, out.data_ptr(), B,
                                  Ho, Wo, C, N, (int)kh, (int)kw, (int)act,
                                  (int)conv_stride, current_stream());
    return out;
}

at::Tensor fconv_dflow_coords(at::Tensor in1, at::Tensor wp, at::Tensor bias,
                              at::Tensor coords, int64_t kh, int64_t kw,
                              c10::optional<at::Tensor> flow_buf,
                              int64_t flow_off) {
    // delta-flow 3x3 -> 2 head with the coords update fused:
    // returns coords_new = coords + conv(in1). flow_buf: also write
    // bf16(coords_new - pixel grid) into channels [flow_off, flow_off+2)
    // of that NHWC buffer (the next iteration's flow input).
    CHECK_DEV(in1); CHECK_CONT(in1); CHECK_CONT(wp); CHECK_CONT(coords);
    const int B = in1.size(0), H = in1.size(1), W = in1.size(2);
    const int Cin = wp.size(2);
    TORCH_CHECK(wp.size(1) == 2 && coords.scalar_type() == at::kFloat);
    auto out = at::empty_like(coords);
    void* fptr = nullptr;
    int fstride = 0;
    if (flow_buf.has_value()) {
        CHECK_DEV(flow_buf.value());
        TORCH_CHECK(flow_buf->is_contiguous() && flow_buf->dim() == 4 &&
                    flow_buf->scalar_type() == at::kBFloat16);
        TORCH_CHECK(flow_buf->size(0) == B && flow_buf->size(1) == H &&
                    flow_buf->size(2) == W && flow_off >= 0 &&
                    flow_off + 2 <= flow_buf->size(3),
                    "flow_buf does not hold a 2-channel slice at flow_off");
        fptr = flow_buf->data_ptr();
        fstride = (int)flow_buf->size(3);
    }
    launch_fconv_dflow_coords(in1.data_ptr(), Cin, in1.size(3), 0,
                              wp.data_ptr(), bias.data_ptr<float>(),
                              coords.data_ptr<float>(),
                              out.data_ptr<float>(), fptr, fstride,
                              (int)flow_off, B, H, W, (int)kh, (int)kw,
                              current_stream());
    return out;
}

void flow_slice(at::Tensor coords, at::Tensor flow_buf, int64_t flow_off) {
    // flow_buf[..., flow_off:flow_off+2] = bf16(coords - pixel grid)
    CHECK_DEV(coords); CHECK_CONT(coords); CHECK_DEV(flow_buf);
    TORCH_CHECK(coords.scalar_type() == at::kFloat && coords.dim() == 4 &&
                coords.size(3) == 2);
    const int B = coords.size(0), H = coords.size(1), W = coords.size(2);
    TORCH_CHECK(flow_buf.is_contiguous() && flow_buf.dim() == 4 &&
                flow_buf.scalar_type() == at::kBFloat16);
    TORCH_CHECK(flow_buf.size(0) == B && flow_buf.size(1) == H &&
                flow_buf.size(2) == W && flow_off >= 0 &&
                flow_off + 2 <= flow_buf.size(3),
                "flow_buf does not hold a 2-channel slice at flow_off");
    launch_flow_slice(coords.data_ptr<float>(), flow_buf.data_ptr(),
                      (int)flow_buf.size(3), (int)flow_off, B, H, W,
                      current_stream());
}

bool lookup_conv_serves(int64_t positions, int64_t C, int64_t Cs, int64_t N) {
    return lookup_conv_geom(positions, (int)C, (int)Cs, (int)N, 0).ok != 0;
}

at::Tensor corr_lookup_conv1x1(std::vector<at::Tensor> levels,
                               at::Tensor coords, int64_t radius,
                               at::Tensor wp, c10::optional<at::Tensor> bias,
                               int64_t act,
                               c10::optional<at::Tensor> vol_scale) {
    // act(conv1x1(bf16 lookup(levels, coords))) -> [B, H, W, N] bf16 without
    // the lookup buffer; wp: packed [1, N, Cs] bf16, zero columns past
    // L*(2r+1)^2. bf16 or e4m3 (+ vol_scale) volumes.
    CHECK_DEV(coords); CHECK_CONT(coords); CHECK_DEV(wp); CHECK_CONT(wp);
    TORCH_CHECK(!levels.empty() && levels.size() <= 4, "1..4 pyramid levels");
    TORCH_CHECK(coords.scalar_type() == at::kFloat && coords.dim() == 4 &&
                coords.size(3) == 2);
    TORCH_CHECK(wp.scalar_type() == at::kBFloat16 && wp.dim() == 3 &&
                wp.size(0) == 1, "wp must be a packed 1x1 conv [1, N, Cs]");
    const int B = coords.size(0), H = coords.size(1), W = coords.size(2);
    const int L = (int)levels.size();
    const int N = wp.size(1), Cs = wp.size(2);
    const void* ptrs[4];
    int hs[4] = {0}, ws[4] = {0};
    int vol_type = 0;
    if (levels[0].scalar_type() == at::kBFloat16) vol_type = 1;
    else if (levels[0].scalar_type() == at::kByte) vol_type = 2;
    const float* vsp = nullptr;
    if (vol_type == 2) {
        TORCH_CHECK(vol_scale.has_value(),
                    "fp8 volume lookup needs vol_scale");
        vsp = vol_scale->data_ptr<float>();
    }
    for (int i = 0; i < L; ++i) {
        CHECK_DEV(levels[i]); CHECK_CONT(levels[i]);
        TORCH_CHECK(levels[i].scalar_type() == levels[0].scalar_type() &&
                    levels[i].dim() == 4 &&
                    levels[i].size(0) * levels[i].size(1) ==
                        (int64_t)B * H * W,
                    "pyramid level does not match coords");
        ptrs[i] = levels[i].data_ptr();
        hs[i] = levels[i].size(2);
        ws[i] = levels[i].size(3);
    }
    const float* bptr = nullptr;
    if (bias.has_value()) {
        TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == N);
        bptr = bias->data_ptr<float>();
    }
    auto out = at::empty({B, H, W, (int64_t)N},
                         coords.options().dtype(at::kBFloat16));
    const int ok = launch_corr_lookup_conv1x1(
        ptrs, hs, ws, vol_type, vsp, coords.data_ptr<float>(),
        wp.data_ptr(), bptr, out.data_ptr(), B, H, W, L, (int)radius, Cs, N,
        (int)act, current_stream());
    TORCH_CHECK(ok, "corr_lookup_conv1x1: no kernel for this shape or volume "
                    "type (Cs=", Cs, ", N=", N, ", vol_type=", vol_type,
                    "); run corr_lookup_nhwc + fconv_plain");
    return out;
}

at::Tensor fconv_smallc_packed(at::Tensor in1, at::Tensor wpk,
                               c10::optional<at::Tensor> bias, int64_t kh,
                               int64_t kw, int64_t act, int64_t in1_off,
                               int64_t in1_len) {
    // fconv_smallk's stride-1 small-C MFMA conv with the weights
    // pre-packed as [N, 128] (k = tap*C + c, zero tail)
    CHECK_DEV(in1); CHECK_CONT(in1); CHECK_DEV(wpk); CHECK_CONT(wpk);
    TORCH_CHECK(in1.scalar_type() == at::kBFloat16 &&
                wpk.scalar_type() == at::kBFloat16 && wpk.dim() == 2 &&
                wpk.size(1) == 128, "wpk must be [N, 128] bf16");
    const int B = in1.size(0), H = in1.size(1), W = in1.size(2);
    const int stride = in1.size(3);
    const int C = in1_len > 0 ? (int)in1_len : stride;
    TORCH_CHECK(in1_off >= 0 && in1_off + C <= stride);
    const int N = wpk.size(0);
    const float* bptr = bias.has_value() ? bias->data_ptr<float>() : nullptr;
    auto out = at::empty({B, H, W, (int64_t)N}, in1.options());
    const int ok = launch_fconv_smallc_packed(
        in1.data_ptr(), stride, (int)in1_off, wpk.data_ptr(), bptr,
        out.data_ptr(), B, H, W, C, N, (int)kh, (int)kw, (int)act,
        current_stream());
    TORCH_CHECK(ok, "fconv_smallc_packed: no kernel for C=", C, " N=", N,
                " ", kh, "x", kw, "; use fconv_smallk");
    return out;
}

std::vector<at::Tensor> inorm_stats(at::Tensor in) {
    CHECK_DEV(in); CHECK_CONT(in);
    const int B = in.size(0), H = in.size(1), W = in.size(2);
    const int C = in.size(3);
    const int S = inorm_stats_partitions(H * W);
    auto acc = at::empty({B, C, S, 2}, in.options().dtype(at::kFloat));
    auto mean = at::empty({B, C}, in.options().dtype(at::kFloat));
    auto rstd = at::empty({B, C}, in.options().dtype(at::kFloat));
    launch_inorm_stats(in.data_ptr(), acc.data_ptr<float>(),
                       mean.data_ptr<float>(), rstd.data_ptr<float>(), B,
                       H * W, C, 1e-5f, current_stream());
    return {mean, rstd};
}

at::Tensor inorm_apply(at::Tensor in, at::Tensor mean, at::Tensor rstd,
                       c10::optional<at::Tensor> res, int64_t mode) {
    CHECK_DEV(in); CHECK_CONT(in);
    const int B = in.size(0), H = in.size(1), W = in.size(2);
    const int C = in.size(3);
    const void* rptr = nullptr;
    if (res.has_value()) {
        CHECK_CONT(res.value());
        rptr = res->data_ptr();
    }
    auto out = at::empty_like(in);
    launch_inorm_apply(in.data_ptr(), mean.data_ptr<float>(),
                       rstd.data_ptr<float>(), rptr, out.data_ptr(), B,
                       H * W, C, (int)mode, current_stream());
    return out;
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.def("corr_volume", &corr_volume, "all-pairs correlation volume (MFMA)");
    m.def("corr_pool2x", &corr_pool2x, "2x2/2 avg-pool one pyramid level");
    m.def("corr_lookup", &corr_lookup, "multi-scale window lookup");
    m.def("corr_lookup_backward", &corr_lookup_backward,
          py::arg("grad_out"), py::arg("coords"), py::arg("radius"),
          py::arg("level_shapes"), py::arg("grads_bf16") = false);
    m.def("gru_gates_fwd", &gru_gates_fwd, "fused GRU gate pointwise");
    m.def("gru_gates_bwd", &gru_gates_bwd);
    m.def("convex_upsample", &convex_upsample, "8x convex upsample");
    m.def("convex_upsample_backward", &convex_upsample_backward);
    // NHWC / fused inference path
    m.def("corr_volume_nhwc", &corr_volume_nhwc,
          "bf16 NT-GEMM correlation volume (physical NHWC fmaps)");
    m.def("corr_volume_nhwc_bidir", &corr_volume_nhwc_bidir,
          "forward + transposed bf16 corr volumes from one GEMM [2B,M,H,W]");
    m.def("fb_consistency", &fb_consistency,
          "forward-backward occlusion masks for both directions",
          py::arg("flow_fw"), py::arg("flow_bw"), py::arg("alpha1") = 0.01,
          py::arg("alpha2") = 0.5, py::arg("return_terms") = false);
    m.def("forward_project", &forward_project,
          "deterministic forward projection of a flow field -> "
          "(projected, holes)",
          py::arg("flow"), py::arg("direction") = 1);
    m.def("flow_residual", &flow_residual,
          "per-sample (max squared coords update bits, cells above thr_sq) "
          "-> [B,2] int32",
          py::arg("prev"), py::arg("nxt"), py::arg("thr_sq"),
          py::arg("out") = py::none());
    m.def("flow_residual_in_place", &flow_residual_in_place,
          "whether flow_residual reads this pair without a copy",
          py::arg("prev"), py::arg("nxt"));
    m.def("interpolate_frame", &interpolate_frame,
          "frame at time t from a bidirectional flow pair -> "
          "(frame, flow_t0, flow_t1, cover)",
          py::arg("im0"), py::arg("im1"), py::arg("fw"), py::arg("bw"),
          py::arg("occ_fw_u8"), py::arg("occ_bw_u8"), py::arg("t"));
    m.def("corr_volume_nhwc_fp8", &corr_volume_nhwc_fp8,
          "fp8 e4m3 corr volume (MX-scaled MFMA, per-tensor quant)");
    m.def("corr_volume_nhwc_fp8s", &corr_volume_nhwc_fp8s,
          "fp8 GEMM with fp8 volume STORAGE -> (uint8 volume, vol_scale)");
    m.def("corr_pool2x_fp8", &corr_pool2x_fp8);
    m.def("quant_fp8", &quant_fp8, "bf16 -> e4m3 with 448/amax scale");
    m.def("fconv_fp8_gru_zr", &fconv_fp8_gru_zr,
          "fp8 MX-MFMA GRU z/r conv pair -> (z bf16, rh e4m3)");
    m.def("fconv_fp8_gru_q", &fconv_fp8_gru_q,
          "fp8 MX-MFMA GRU candidate conv + state update");
    m.def("corr_pool2x_bf16", &corr_pool2x_bf16);
    m.def("corr_lookup_nhwc", &corr_lookup_nhwc,
          "pyramid lookup writing physical NHWC (channel-padded)",
          py::arg("levels"), py::arg("coords"), py::arg("radius"),
          py::arg("c_stride"), py::arg("out_bf16"),
          py::arg("out_buf") = c10::nullopt,
          py::arg("flow_buf") = c10::nullopt, py::arg("flow_off") = 0,
          py::arg("vol_scale") = c10::nullopt);
    m.def("fconv_plain", &fconv_plain,
          "fused NHWC bf16 conv (+bias +activation, slice output)");
    m.def("fconv_gru_zr", &fconv_gru_zr, "GRU z/r gate conv pair");
    m.def("fconv_smallk", &fconv_smallk, "direct NHWC conv for tiny Cin");
    m.def("inorm_stats", &inorm_stats, "per-(b,c) instance-norm stats");
    m.def("inorm_apply", &inorm_apply,
          "instance-norm apply (+relu / +residual-relu)");
    m.def("fconv_dflow_coords", &fconv_dflow_coords,
          "flow-head final conv fused with the coords update (+ the next "
          "iteration's bf16 flow slice into flow_buf)",
          py::arg("in1"), py::arg("wp"), py::arg("bias"), py::arg("coords"),
          py::arg("kh"), py::arg("kw"), py::arg("flow_buf") = c10::nullopt,
          py::arg("flow_off") = 0);
    m.def("flow_slice", &flow_slice,
          "flow_buf[..., off:off+2] = bf16(coords - pixel grid)",
          py::arg("coords"), py::arg("flow_buf"), py::arg("flow_off"));
    m.def("lookup_conv_serves", &lookup_conv_serves,
          "whether corr_lookup_conv1x1 has a kernel for this shape",
          py::arg("positions"), py::arg("C"), py::arg("Cs"), py::arg("N"));
    m.def("corr_lookup_conv1x1", &corr_lookup_conv1x1,
          "pyramid lookup fused with the pointwise conv that consumes it",
          py::arg("levels"), py::arg("coords"), py::arg("radius"),
          py::arg("wp"), py::arg("bias"), py::arg("act"),
          py::arg("vol_scale") = c10::nullopt);
    m.def("fconv_smallc_packed", &fconv_smallc_packed,
          "small-C MFMA conv, all N per block, host-packed [N,128] weights",
          py::arg("in1"), py::arg("wpk"), py::arg("bias"), py::arg("kh"),
          py::arg("kw"), py::arg("act"), py::arg("in1_off") = 0,
          py::arg("in1_len") = 0);
    m.def("fconv_gru_q", &fconv_gru_q, "GRU candidate conv + state update");
    m.def("fconv_plain_f32", &fconv_plain_f32,
          "NHWC bf16 conv (+bias) with unrounded fp32 output, no activation",
          py::arg("in1"), py::arg("wp"), py::arg("bias"), py::arg("kh"),
          py::arg("kw"), py::arg("in1_off") = 0, py::arg("in1_len") = 0);
    m.def("fconv_gru_zr_pre", &fconv_gru_zr_pre,
          "GRU z/r conv pair over [h | x[..., x_off:x_off+x_len]] plus the "
          "fp32 term pre[..., pre_off:pre_off+2*hd] (bias folded in)",
          py::arg("h"), py::arg("x"), py::arg("wp"), py::arg("kh"),
          py::arg("kw"), py::arg("pre"), py::arg("pre_off"),
          py::arg("x_off"), py::arg("x_len"));
    m.def("fconv_gru_q_pre", &fconv_gru_q_pre,
          "GRU candidate conv + state update over [rh | x slice] plus the "
          "fp32 term pre[..., pre_off:pre_off+hd] (bias folded in)",
          py::arg("rh"), py::arg("x"), py::arg("wp"), py::arg("kh"),
          py::arg("kw"), py::arg("z"), py::arg("h"), py::arg("pre"),
          py::arg("pre_off"), py::arg("x_off"), py::arg("x_len"));
}
