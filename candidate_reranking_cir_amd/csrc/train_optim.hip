// Training pass: AdamW (torch.optim.AdamW semantics), with the bias corrections from the host (cir_adamw_step) or with the whole step decided
// on the device (GradScaler.step's found_inf skip, stage2_train.py:215-218).  None of it is on the inference path.

#include <algorithm>
#include "common.hpp"

namespace cir {

// AdamW (decoupled weight decay, torch.optim.AdamW semantics): in place on fp32 param / moments
__global__ __launch_bounds__(256) void adamw_kernel(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                                                    float wd, float bc1, float bc2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float gi = g[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi, vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi; v[i] = vi;
    float w = p[i] * (1.f - lr * wd);
    w -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
    p[i] = w;
}

// ---- the optimizer step without a host read (round 6) -------------------------------------------------------------------------------
// state (device, 8 x 32 bit): [0] found_inf of the step in flight, [1] applied steps t, [2] skipped steps, [3] / [4] the fp32 bias
// corrections 1 - beta^t of the step in flight.  cir_grads_check ORs into [0]; cir_adamw_begin turns the flag into t / skipped and the
// corrections; cir_adamw_step_dev returns at once when the flag is set - GradScaler.step's found_inf skip (stage2_train.py:215-218) with
// the decision taken where the gradients are.
__global__ __launch_bounds__(256) void grads_check_kernel(float* g, int64_t n4, int64_t n, float scale, int* state) {
    int bad = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    auto nf = [](float f) { return (int)((__float_as_uint(f) & 0x7f800000u) == 0x7f800000u); };      // (finite <=> exponent field not all ones)
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += 4 * stride) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * stride < n4) x[u] = reinterpret_cast<float4*>(g)[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * stride < n4) {
                if (scale != 1.f) {
                    x[u].x *= scale; x[u].y *= scale; x[u].z *= scale; x[u].w *= scale;
                    reinterpret_cast<float4*>(g)[i + u * stride] = x[u];
                }
                bad |= nf(x[u].x) | nf(x[u].y) | nf(x[u].z) | nf(x[u].w);
            }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {           // tail of a length that is not a multiple of 4
        float x = g[4 * n4 + threadIdx.x];
        if (scale != 1.f) { x *= scale; g[4 * n4 + threadIdx.x] = x; }
        bad |= nf(x);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(state, 1);
}

__global__ void adamw_begin_kernel(int* state, float b1, float b2) {
    if (threadIdx.x || blockIdx.x) return;
    if (state[0]) { state[2] += 1; return; }
    const int t = state[1] + 1;
    state[1] = t;
    reinterpret_cast<float*>(state)[3] = (float)(1.0 - pow((double)b1, (double)t));
    reinterpret_cast<float*>(state)[4] = (float)(1.0 - pow((double)b2, (double)t));
}

template <typename T16>
__global__ __launch_bounds__(256) void adamw_dev_kernel(float* p, const float* g, float* m, float* v, int64_t n4, int64_t n, float lr, float b1, float b2,
                                                        float eps, float wd, const int* state, T16* p16) {
    if (state[0]) return;                                               // non-finite gradients somewhere in this step: nothing is applied
    const float bc1 = reinterpret_cast<const float*>(state)[3], bc2 = reinterpret_cast<const float*>(state)[4];
    auto upd = [&](float& pi, float gi, float& mi, float& vi) {
        mi = b1 * mi + (1.f - b1) * gi;
        vi = b2 * vi + (1.f - b2) * gi * gi;
        float w = pi * (1.f - lr * wd);
        w -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
        pi = w;
    };
    // two float4 per thread, 256 apart: all eight 16-byte loads of a thread are in flight before the first update
    const int64_t i0 = (int64_t)blockIdx.x * 512 + threadIdx.x;
    float4 pp[2], mm[2], vv[2], gg[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t i = i0 + 256 * u;
        if (i < n4) {
            pp[u] = reinterpret_cast<float4*>(p)[i]; mm[u] = reinterpret_cast<float4*>(m)[i]; vv[u] = reinterpret_cast<float4*>(v)[i];
            gg[u] = reinterpret_cast<const float4*>(g)[i];
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t i = i0 + 256 * u;
        if (i < n4) {
            upd(pp[u].x, gg[u].x, mm[u].x, vv[u].x); upd(pp[u].y, gg[u].y, mm[u].y, vv[u].y);
            upd(pp[u].z, gg[u].z, mm[u].z, vv[u].z); upd(pp[u].w, gg[u].w, mm[u].w, vv[u].w);
            reinterpret_cast<float4*>(p)[i] = pp[u]; reinterpret_cast<float4*>(m)[i] = mm[u]; reinterpret_cast<float4*>(v)[i] = vv[u];
            if (p16) {
                u32x2 h;
                h.x = pack2<T16>(pp[u].x, pp[u].y); h.y = pack2<T16>(pp[u].z, pp[u].w);
                reinterpret_cast<u32x2*>(p16)[i] = h;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {
        const int64_t j = 4 * n4 + threadIdx.x;
        float pi = p[j], mi = m[j], vi = v[j];
        upd(pi, g[j], mi, vi);
        p[j] = pi; m[j] = mi; v[j] = vi;
        if (p16) p16[j] = static_cast<T16>(pi);
    }
}

}  // namespace cir

using namespace cir;

extern "C" int cir_grads_check(float* g, int64_t n, float scale, int32_t* state, void* stream) {
    CIR_CHECK_PTR(g); CIR_CHECK_PTR(state);
    if (n <= 0) return CIR_EINVAL;
    if (!cir_aligned16(g)) return CIR_EALIGN;
    const int64_t n4 = n / 4;
    const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((n4 + 1023) / 1024, 1), 256 * 32);
    hipLaunchKernelGGL(grads_check_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, n4, n, scale, state);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_adamw_begin(int32_t* state, float beta1, float beta2, void* stream) {
    CIR_CHECK_PTR(state);
    hipLaunchKernelGGL(adamw_begin_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), state, beta1, beta2);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_adamw_step_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                                  float weight_decay, const int32_t* state, void* p16, int dtype16, void* stream) {
    CIR_CHECK_PTR(p); CIR_CHECK_PTR(g); CIR_CHECK_PTR(m); CIR_CHECK_PTR(v); CIR_CHECK_PTR(state);
    if (n <= 0) return CIR_EINVAL;
    if (p16 && dtype16 != CIR_BF16 && dtype16 != CIR_F16) return CIR_EDTYPE;
    if (!cir_aligned16(p) || !cir_aligned16(g) || !cir_aligned16(m) || !cir_aligned16(v) || (p16 && (reinterpret_cast<uintptr_t>(p16) & 7))) return CIR_EALIGN;
    const int64_t n4 = n / 4;
    const dim3 grid((unsigned)std::max<int64_t>((n4 + 511) / 512, 1)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype16(p16 ? dtype16 : CIR_F16, [&](auto t) {      // (without a 16-bit copy dtype16 is not looked at: the fp16 instantiation, p16 = NULL)
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((adamw_dev_kernel<T>), grid, block, 0, s, p, g, m, v, n4, n, lr, beta1, beta2, eps, weight_decay, state, reinterpret_cast<T*>(p16));
    });
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                              int step, void* stream) {
    CIR_CHECK_PTR(p); CIR_CHECK_PTR(g); CIR_CHECK_PTR(m); CIR_CHECK_PTR(v);
    if (n <= 0 || step <= 0) return CIR_EINVAL;
    const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, g, m, v, n, lr, beta1,
                       beta2, eps, weight_decay, bc1, bc2);
    CIR_LAUNCH_RESULT();
}
