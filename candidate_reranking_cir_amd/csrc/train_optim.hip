// Training pass: AdamW (torch.optim.AdamW semantics), with the bias corrections from the host (cir_adamw_step) or with the whole step decided
// on the device (GradScaler.step's found_inf skip, stage2_train.py:215-218); with parameter groups and clip_grad_norm_'s global-norm clip
// decided there as well (cir_grads_sumsq, cir_adamw_begin_clip, cir_adamw_step_groups, below).  None of it is on the inference path.

#include <algorithm>
#include <cmath>
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

// ---- parameter groups and the global-norm clip, decided on the device ---------------------------------------------------------------
// torch.nn.utils.clip_grad_norm_ + an AdamW with several param_groups (stage2_train.py:138 builds the one-group optimizer, :215-218 steps
// it under the scaler; utils.py:216-241 are the schedules that write every group's lr) without a host read:
//   grads_sumsq_kernel     one read-only pass over a flat gradient buffer: state[0] |= any non-finite element (grads_check_kernel's exponent
//                          test) and ONE float64 sum of squares per workgroup.  Each thread adds its squares in double in the order of its
//                          loop (trip, quarter u, x y z w, then its tail element), the workgroup folds its 256 sums in a fixed LDS tree:
//                          no float atomics, the partials repeat bit for bit.  A finite fp32 buffer cannot overflow a double.
//   adamw_begin_clip_kernel adamw_begin_kernel's job + the clip: one workgroup adds the partials of every work item of the step (thread j
//                          takes j, j + 256, ... in index order, then the same tree), total_norm = fp32(sqrt(sum)),
//                          coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 - clip_grad_norm_'s rule; state[5] = coef, state[6] = norm.
//   adamw_groups_kernel    adamw_dev_kernel with (lr, weight_decay, eps) per float4 from a segment table and g * state[5] in registers.
constexpr int SUMSQ_CAP = 1024;                                         // the largest grid of the norm pass: 4 workgroups per CU

__global__ __launch_bounds__(256) void grads_sumsq_kernel(const float* g, int64_t n4, int64_t n, int* state, double* partials) {
    __shared__ double red[256];
    int bad = 0;
    double acc = 0.0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    auto nf = [](float f) { return (int)((__float_as_uint(f) & 0x7f800000u) == 0x7f800000u); };
    auto sq = [](float f) { return (double)f * (double)f; };
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += 4 * stride) {
        float4 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * stride < n4) x[u] = reinterpret_cast<const float4*>(g)[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i + u * stride < n4) {
                bad |= nf(x[u].x) | nf(x[u].y) | nf(x[u].z) | nf(x[u].w);
                acc += sq(x[u].x); acc += sq(x[u].y); acc += sq(x[u].z); acc += sq(x[u].w);
            }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {           // tail of a length that is not a multiple of 4
        const float x = g[4 * n4 + threadIdx.x];
        bad |= nf(x);
        acc += sq(x);
    }
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = red[0];
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(state, 1);
}

__global__ __launch_bounds__(256) void adamw_begin_clip_kernel(int* state, float b1, float b2, const double* partials, int64_t n_partials, float max_norm) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int64_t j = threadIdx.x; j < n_partials; j += 256) acc += partials[j];
    red[threadIdx.x] = acc;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x) return;
    // sqrt and the quotient in double, rounded once to fp32: both are the correctly rounded fp32 results (53 >= 2 * 24 + 2 bits)
    const float norm = (float)sqrt(red[0]);
    reinterpret_cast<float*>(state)[6] = norm;
    if (state[0]) { state[2] += 1; reinterpret_cast<float*>(state)[5] = 0.f; return; }
    const float den = norm + 1e-6f;
    reinterpret_cast<float*>(state)[5] = fminf(1.f, (float)((double)max_norm / (double)den));
    const int t = state[1] + 1;
    state[1] = t;
    reinterpret_cast<float*>(state)[3] = (float)(1.0 - pow((double)b1, (double)t));
    reinterpret_cast<float*>(state)[4] = (float)(1.0 - pow((double)b2, (double)t));
}

// Where a float4 finds its segment: the workgroup's first element is looked up by a binary search whose every load has a workgroup-uniform
// address (the table is read-only and a few KB: it stays in cache, and the search runs while the thread's eight 16-byte loads are in
// flight); from that segment each float4 walks forward, one table read per segment boundary between the block's start and itself - none in
// the common case of a block inside one segment, which is tested once per workgroup and then runs with the group's scalars in scalar
// registers (the per-lane selects cost 4 - 9 % of the kernel on full-size slabs when every workgroup paid them).  Chosen over a per-block start hint because it needs no second table tied to the block
// size, and over a table in LDS because a slab's table (one segment per run of parameters of one group) can exceed what a block would stage.
// A malformed table cannot send a read outside it: the walk stops at the last segment, and group ids are taken modulo 8.
template <typename T16>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* p, const float* g, float* m, float* v, int64_t n4, int64_t n, float b1, float b2,
                                                           const int* state, T16* p16, const int64_t* seg_end, const int32_t* seg_group, int nseg,
                                                           int group0, cir_adamw_groups groups, int clip) {
    if (state[0]) return;                                               // non-finite gradients somewhere in this step: nothing is applied
    const float bc1 = reinterpret_cast<const float*>(state)[3], bc2 = reinterpret_cast<const float*>(state)[4];
    const float coef = clip ? reinterpret_cast<const float*>(state)[5] : 1.f;
    auto upd = [&](float& pi, float gi, float& mi, float& vi, float lr, float wd, float eps) {
        mi = b1 * mi + (1.f - b1) * gi;
        vi = b2 * vi + (1.f - b2) * gi * gi;
        float w = pi * (1.f - lr * wd);
        w -= lr * (mi / bc1) / (sqrtf(vi / bc2) + eps);
        pi = w;
    };
    auto pick = [&](const float* a, int id) {                           // (selects, not an indexed read of the argument block)
        float x = a[0];
#pragma unroll
        for (int k = 1; k < CIR_ADAMW_MAX_GROUPS; ++k) x = id == k ? a[k] : x;
        return x;
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
    int s = 0, uid = group0;
    bool one = true;                                                    // the whole workgroup lies in ONE segment (always, without a table)
    if (seg_end) {                                                      // first segment that ends behind the block's first element
        const int64_t e0 = (int64_t)blockIdx.x * 2048;
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (seg_end[mid] > e0) hi = mid; else lo = mid + 1;
        }
        s = lo;
        one = s == nseg - 1 || seg_end[s] >= e0 + 2048;
        uid = seg_group[s] & (CIR_ADAMW_MAX_GROUPS - 1);
    }
    auto run = [&](auto scalars) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t i = i0 + 256 * u;
            if (i < n4) {
                float lr, wd, eps;
                scalars(i, lr, wd, eps);
                if (clip) { gg[u].x *= coef; gg[u].y *= coef; gg[u].z *= coef; gg[u].w *= coef; }
                upd(pp[u].x, gg[u].x, mm[u].x, vv[u].x, lr, wd, eps); upd(pp[u].y, gg[u].y, mm[u].y, vv[u].y, lr, wd, eps);
                upd(pp[u].z, gg[u].z, mm[u].z, vv[u].z, lr, wd, eps); upd(pp[u].w, gg[u].w, mm[u].w, vv[u].w, lr, wd, eps);
                reinterpret_cast<float4*>(p)[i] = pp[u]; reinterpret_cast<float4*>(m)[i] = mm[u]; reinterpret_cast<float4*>(v)[i] = vv[u];
                if (p16) {
                    u32x2 h;
                    h.x = pack2<T16>(pp[u].x, pp[u].y); h.y = pack2<T16>(pp[u].z, pp[u].w);
                    reinterpret_cast<u32x2*>(p16)[i] = h;
                }
            }
        }
    };
    if (one) {
        // all but the few workgroups that straddle a boundary: the group's scalars are wave-uniform (scalar registers, 1 - lr wd once),
        // as cir_adamw_step_dev holds its arguments
        const int id = __builtin_amdgcn_readfirstlane(uid);
        const float lr1 = pick(groups.lr, id), wd1 = pick(groups.weight_decay, id), eps1 = pick(groups.eps, id);
        run([&](int64_t, float& lr, float& wd, float& eps) { lr = lr1; wd = wd1; eps = eps1; });
    } else {
        run([&](int64_t i, float& lr, float& wd, float& eps) {
            while (s < nseg - 1 && seg_end[s] <= 4 * i) ++s;
            const int id = seg_group[s] & (CIR_ADAMW_MAX_GROUPS - 1);
            lr = pick(groups.lr, id); wd = pick(groups.weight_decay, id); eps = pick(groups.eps, id);
        });
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(n - 4 * n4)) {           // (the form without a table only: a table's n is a multiple of 4)
        const int64_t j = 4 * n4 + threadIdx.x;
        const float lr = pick(groups.lr, group0), wd = pick(groups.weight_decay, group0), eps = pick(groups.eps, group0);
        float pi = p[j], mi = m[j], vi = v[j], gi = g[j];
        if (clip) gi *= coef;
        upd(pi, gi, mi, vi, lr, wd, eps);
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

static int64_t sumsq_blocks(int64_t n) { return std::min<int64_t>(std::max<int64_t>((n / 4 + 1023) / 1024, 1), SUMSQ_CAP); }

extern "C" int64_t cir_grads_sumsq_workspace(int64_t n) { return n <= 0 ? (int64_t)CIR_EINVAL : sumsq_blocks(n); }

extern "C" int cir_grads_sumsq(const float* g, int64_t n, int32_t* state, double* partials, void* stream) {
    CIR_CHECK_PTR(g); CIR_CHECK_PTR(state); CIR_CHECK_PTR(partials);
    if (n <= 0) return CIR_EINVAL;
    if (!cir_aligned16(g) || (reinterpret_cast<uintptr_t>(partials) & 7)) return CIR_EALIGN;
    hipLaunchKernelGGL(grads_sumsq_kernel, dim3((unsigned)sumsq_blocks(n)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), g, n / 4, n, state, partials);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_adamw_begin_clip(int32_t* state, float beta1, float beta2, const double* partials, int64_t n_partials, float max_norm, void* stream) {
    CIR_CHECK_PTR(state); CIR_CHECK_PTR(partials);
    if (n_partials <= 0 || !(max_norm > 0.f) || !std::isfinite(max_norm)) return CIR_EINVAL;
    if (reinterpret_cast<uintptr_t>(partials) & 7) return CIR_EALIGN;
    hipLaunchKernelGGL(adamw_begin_clip_kernel, dim3(1), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), state, beta1, beta2, partials, n_partials, max_norm);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_adamw_step_groups(float* p, const float* g, float* m, float* v, int64_t n, float beta1, float beta2, const int32_t* state,
                                     const int64_t* seg_end, const int32_t* seg_group, int nseg, int group, const cir_adamw_groups* groups, int ngroups,
                                     int clip, void* p16, int dtype16, void* stream) {
    CIR_CHECK_PTR(p); CIR_CHECK_PTR(g); CIR_CHECK_PTR(m); CIR_CHECK_PTR(v); CIR_CHECK_PTR(state); CIR_CHECK_PTR(groups);
    if (n <= 0 || nseg < 1 || ngroups < 1 || ngroups > CIR_ADAMW_MAX_GROUPS) return CIR_EINVAL;
    if ((seg_end == nullptr) != (seg_group == nullptr)) return CIR_EINVAL;
    if (seg_end ? (n % 4 != 0) : (nseg != 1 || group < 0 || group >= ngroups)) return CIR_EINVAL;
    if (p16 && dtype16 != CIR_BF16 && dtype16 != CIR_F16) return CIR_EDTYPE;
    if (!cir_aligned16(p) || !cir_aligned16(g) || !cir_aligned16(m) || !cir_aligned16(v) || (p16 && (reinterpret_cast<uintptr_t>(p16) & 7))) return CIR_EALIGN;
    if (seg_end && ((reinterpret_cast<uintptr_t>(seg_end) & 7) || (reinterpret_cast<uintptr_t>(seg_group) & 3))) return CIR_EALIGN;
    const int64_t n4 = n / 4;
    const dim3 grid((unsigned)std::max<int64_t>((n4 + 511) / 512, 1)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const cir_adamw_groups gr = *groups;
    by_dtype16(p16 ? dtype16 : CIR_F16, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((adamw_groups_kernel<T>), grid, block, 0, s, p, g, m, v, n4, n, beta1, beta2, state, reinterpret_cast<T*>(p16), seg_end, seg_group,
                           nseg, seg_end ? 0 : group, gr, clip != 0);
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
