// The two heads of the stage-I training step, built from one set of pieces; none of it is on the inference path.
// ---- contrastive head of the stage-I training step (blip_stage1.py:83-91): p_hat = F.normalize(p), logits = p_hat target^T / temp, and its
// adjoint.  ~0.5 GFLOP at B = 1024: plain fp32 FMA chains, every reduction in a fixed order (wave butterflies, block trees, serial loops over
// rows) and no atomics - the head's outputs repeat bit for bit.  temp is read on the device.
// ---- image side of the stage-I step when the image encoder is trained (stage1_train.py --blip-img-tune): the gradient of the logits
// w.r.t. the target features, and the pooled head F.normalize(vision_proj(tokens[:, 0])) (blip_stage1.py:57) with its adjoint.  Same
// conventions: fp32 FMA chains, fixed-order reductions, no atomics.

#include "common.hpp"

namespace cir {

constexpr int kHeadMaxE = 1024;
constexpr int kPoolMaxD = 2048;
constexpr int kHeadChunks = kHeadMaxE / 256;      // a 256-thread block holds a row of E values as element t + 256 c of thread t

// fixed-order sum over a 256-thread block (wave butterflies, then the four wave sums in order); every thread gets the result
__device__ __forceinline__ float block256_sum(float v, float* red4) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// acc[c] = sum_k coef[k * stride] M[k][t + 256 c]: the rows k of M (E wide, contiguous) in order, one FMA chain from 0 per element
__device__ __forceinline__ void weighted_rows_sum(float (&acc)[kHeadChunks], const float* __restrict__ coef, int64_t stride,
                                                  const float* __restrict__ M, int rows, int E) {
    const int t = threadIdx.x;
#pragma unroll
    for (int c = 0; c < kHeadChunks; ++c) acc[c] = 0.f;
    for (int64_t k = 0; k < rows; ++k) {
        const float g = coef[k * stride];
        const float* mr = M + k * E;
#pragma unroll
        for (int c = 0; c < kHeadChunks; ++c) {
            const int e = t + 256 * c;
            if (e < E) acc[c] = fmaf(g, mr[e], acc[c]);
        }
    }
}

// The adjoint of F.normalize for one row h = x / max(||x||, eps), inv = 1 / max(||x||, eps): out = (g - h (h . g)) inv; returns h . g (each
// thread's FMA chain over its elements, then block256_sum).  CLAMP: a row clamped by the epsilon (inv = 1e12) gets out = g inv, F.normalize's
// own gradient there (the clamp is a constant divisor).  The pooled head does that, the contrastive head keeps the h (h . g) term on such a
// row too: the two differ today and this is where it shows (LABNOTES.md section 24).
template <bool CLAMP>
__device__ __forceinline__ float normalize_adjoint_row(const float (&g)[kHeadChunks], const float* __restrict__ h, float inv,
                                                       float* __restrict__ out, int E, float* red4) {
    const int t = threadIdx.x;
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < kHeadChunks; ++c) {
        const int e = t + 256 * c;
        if (e < E) s = fmaf(h[e], g[c], s);
    }
    const float dot = block256_sum(s, red4);
    const float sd = (CLAMP && inv >= 1.0f / 1e-12f) ? 0.f : dot;           // (the forward's value of inv for ||x|| < eps)
#pragma unroll
    for (int c = 0; c < kHeadChunks; ++c) {
        const int e = t + 256 * c;
        if (e < E) out[e] = (g[c] - h[e] * sd) * inv;
    }
    return dot;
}

// one block per query row i: its norm, p_hat row and inverse norm, then one wave per target column j
__global__ __launch_bounds__(256) void contrastive_fwd_kernel(const float* __restrict__ p, const float* __restrict__ target,
                                                              const float* __restrict__ temp, float* __restrict__ p_hat,
                                                              float* __restrict__ inv_norm, float* __restrict__ logits, int Bt, int E) {
    __shared__ float ph[kHeadMaxE];
    __shared__ float red4[4];
    const int64_t i = blockIdx.x;
    const int t = threadIdx.x;
    const float* pr = p + i * E;
    float s = 0.f;
    for (int e = t; e < E; e += 256) s = fmaf(pr[e], pr[e], s);
    const float nrm = fmaxf(sqrtf(block256_sum(s, red4)), 1e-12f);      // F.normalize: x / max(||x||, eps)
    for (int e = t; e < E; e += 256) {
        const float v = pr[e] / nrm;
        ph[e] = v;
        p_hat[i * E + e] = v;
    }
    if (t == 0) inv_norm[i] = 1.f / nrm;
    __syncthreads();
    const float tp = temp[0];
    const int wave = t >> 6, lane = t & 63;
    for (int j = wave; j < Bt; j += 4) {
        const float* tr = target + (int64_t)j * E;
        float acc = 0.f;
        for (int e = lane; e < E; e += 64) acc = fmaf(ph[e], tr[e], acc);
        acc = wave_sum(acc);
        if (lane == 0) logits[i * Bt + j] = acc / tp;
    }
}

// adjoint, one block per query row i: dp_hat = dlogits[i] . target / temp, dp = (dp_hat - p_hat (p_hat . dp_hat)) / ||p||; the row's
// p_hat . dp_hat = sum_j dlogits_ij logits_ij is kept for dtemp
__global__ __launch_bounds__(256) void contrastive_bwd_rows_kernel(const float* __restrict__ dlogits, const float* __restrict__ target,
                                                                   const float* __restrict__ temp, const float* __restrict__ p_hat,
                                                                   const float* __restrict__ inv_norm, float* __restrict__ dp,
                                                                   float* __restrict__ row_dot, int Bt, int E) {
    __shared__ float red4[4];
    const int64_t i = blockIdx.x;
    float acc[kHeadChunks];
    weighted_rows_sum(acc, dlogits + i * Bt, 1, target, Bt, E);
    const float tp = temp[0];
#pragma unroll
    for (int c = 0; c < kHeadChunks; ++c) acc[c] /= tp;
    const float sd = normalize_adjoint_row<false>(acc, p_hat + i * E, inv_norm[i], dp + i * E, E, red4);
    if (threadIdx.x == 0) row_dot[i] = sd;
}

// dtarget[j][:] = (1 / temp) sum_i dlogits[i][j] p_hat[i][:] (the adjoint of blip_stage1.py:91 w.r.t. target_features): one block per
// target row j, the query rows i in order
__global__ __launch_bounds__(256) void contrastive_bwd_target_kernel(const float* __restrict__ dlogits, const float* __restrict__ p_hat,
                                                                     const float* __restrict__ temp, float* __restrict__ dtarget,
                                                                     int B, int Bt, int E) {
    const int64_t j = blockIdx.x;
    float acc[kHeadChunks];
    weighted_rows_sum(acc, dlogits + j, Bt, p_hat, B, E);
    const float tp = temp[0];
#pragma unroll
    for (int c = 0; c < kHeadChunks; ++c) {
        const int e = threadIdx.x + 256 * c;
        if (e < E) dtarget[j * E + e] = acc[c] / tp;
    }
}

// one block per image i: t = x_i W^T + b with the k-ordered FMA chain of linear_f32_kernel (misc.hip: acc from 0 over k = 0 .. D - 1, then
// + bias), the norm with l2_normalize_kernel's one-wave order (lane-strided FMA sums, the wave butterfly), t_hat = t * inv - so t_hat has the
// bits of cir_l2_normalize(cir_linear_f32(...)).  x_i = the CLS row of image i, read in place at row stride ldx
__global__ __launch_bounds__(256) void pooled_head_fwd_kernel(const float* __restrict__ x, int64_t ldx, const float* __restrict__ W,
                                                              const float* __restrict__ bias, float* __restrict__ t_hat,
                                                              float* __restrict__ inv_norm, int E, int D) {
    __shared__ __attribute__((aligned(16))) float xs[kPoolMaxD];
    __shared__ float ts[kHeadMaxE];
    __shared__ float inv_s;
    const int64_t i = blockIdx.x;
    const int t = threadIdx.x;
    for (int d = t; d < D; d += 256) xs[d] = x[i * ldx + d];
    __syncthreads();
    for (int e = t; e < E; e += 256) {
        const float4* wr = reinterpret_cast<const float4*>(W + (int64_t)e * D);
        float acc = 0.f;
        for (int d4 = 0; d4 < D / 4; ++d4) {
            const float4 w = wr[d4];
            const float4 a = *reinterpret_cast<const float4*>(xs + 4 * d4);
            acc = fmaf(a.x, w.x, acc);
            acc = fmaf(a.y, w.y, acc);
            acc = fmaf(a.z, w.z, acc);
            acc = fmaf(a.w, w.w, acc);
        }
        ts[e] = acc + bias[e];
    }
    __syncthreads();
    if (t < 64) {
        float s = 0.f;
        for (int c = t; c < E; c += 64) { const float v = ts[c]; s = fmaf(v, v, s); }
        const float inv = 1.0f / fmaxf(sqrtf(wave_sum(s)), 1e-12f);          // F.normalize: x / max(||x||, eps)
        if (t == 0) { inv_s = inv; inv_norm[i] = inv; }
    }
    __syncthreads();
    const float inv = inv_s;
    for (int e = t; e < E; e += 256) t_hat[i * E + e] = ts[e] * inv;
}

// normalise adjoint, one block per image i: dt = inv (dt_hat - t_hat (t_hat . dt_hat)), an epsilon-clamped row dt = inv dt_hat
__global__ __launch_bounds__(256) void pooled_head_bwd_rows_kernel(const float* __restrict__ dt_hat, const float* __restrict__ t_hat,
                                                                   const float* __restrict__ inv_norm, float* __restrict__ dt, int E) {
    __shared__ float red4[4];
    const int64_t i = blockIdx.x;
    float g[kHeadChunks];
#pragma unroll
    for (int c = 0; c < kHeadChunks; ++c) {
        const int e = threadIdx.x + 256 * c;
        g[c] = e < E ? dt_hat[i * E + e] : 0.f;
    }
    normalize_adjoint_row<true>(g, t_hat + i * E, inv_norm[i], dt + i * E, E, red4);
}

// projection dgrad: dx[i][d] = sum_e g[i][e] W[e][d]  (written into rows of stride lddx: the CLS rows of the stream gradient)
__global__ __launch_bounds__(256) void head_dgrad_kernel(const float* __restrict__ dp, const float* __restrict__ W, float* __restrict__ dx,
                                                         int64_t lddx, int E, int D) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    const int64_t i = blockIdx.y;
    if (d >= D) return;
    const float* g = dp + i * E;
    float acc = 0.f;
    for (int e = 0; e < E; ++e) acc = fmaf(g[e], W[(int64_t)e * D + d], acc);
    dx[i * lddx + d] = acc;
}

// projection weight and bias gradients: dW[e][d] = sum_i g[i][e] x[i][d] (x rows of stride ldx: the CLS rows of the stream), db[e] = sum_i
// g[i][e]; rows in order, one adder per element.  Written for text_proj (ADD = false); ADDED to dW / db for vision_proj (ADD = true: the
// blip_bs mini-batches of a step each contribute).  blockIdx.y = e; the first x-block column carries db
template <bool ADD>
__global__ __launch_bounds__(256) void head_wgrad_kernel(const float* __restrict__ g, const float* __restrict__ x, int64_t ldx,
                                                         float* __restrict__ dW, float* __restrict__ db, int B, int E, int D) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    const int64_t e = blockIdx.y;
    if (d < D) {
        float acc = 0.f;
        for (int64_t i = 0; i < B; ++i) acc = fmaf(g[i * E + e], x[i * ldx + d], acc);
        if (ADD) dW[e * D + d] += acc; else dW[e * D + d] = acc;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        float acc = 0.f;
        for (int64_t i = 0; i < B; ++i) acc += g[i * E + e];
        if (ADD) db[e] += acc; else db[e] = acc;
    }
}

// dtemp = -sum_i row_dot[i] / temp (written, rows in order)
__global__ void head_dtemp_kernel(const float* __restrict__ row_dot, const float* __restrict__ temp, float* __restrict__ dtemp, int B) {
    if (blockIdx.x || threadIdx.x) return;
    float acc = 0.f;
    for (int i = 0; i < B; ++i) acc += row_dot[i];
    dtemp[0] = -acc / temp[0];
}

}  // namespace cir

using namespace cir;

// ---- host-side checks shared by the five entry points (each keeps its own ORDER of pointer, extent, dtype, shape and alignment tests: the
// code a call with several faults gets is part of the contract) ------------------------------------------------------------------------
// E in 256-column chunks of registers / LDS, one block per row, the logits indexed in 31 bits
static bool head_shape_ok(int E, int rows, int64_t logits) { return E <= kHeadMaxE && E % 4 == 0 && rows <= 65535 && logits < (int64_t(1) << 31); }
// `rows` rows of D floats at stride ld (the CLS rows of a token stream, in place): extent, then alignment
static bool head_rows_fit(int64_t ld, int rows, int D) { return ld >= D && (int64_t)(rows - 1) * ld + D < (int64_t(1) << 40); }
static bool cir_rows_ok(const void* p, int64_t ld) { return cir_aligned16(p) && (ld % 4) == 0; }
static bool cir_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

extern "C" int cir_contrastive_fwd(const float* p, const float* target, const float* temp, float* p_hat, float* inv_norm, float* logits,
                                   int B, int Bt, int E, int dtype, void* stream) {
    CIR_CHECK_PTR(p); CIR_CHECK_PTR(target); CIR_CHECK_PTR(temp); CIR_CHECK_PTR(p_hat); CIR_CHECK_PTR(inv_norm); CIR_CHECK_PTR(logits);
    if (B <= 0 || Bt <= 0 || E <= 0) return CIR_EINVAL;
    if (dtype != CIR_F32) return CIR_EDTYPE;
    if (!head_shape_ok(E, B, (int64_t)B * Bt)) return CIR_ESHAPE;
    if (!cir_aligned16(p) || !cir_aligned16(target) || !cir_aligned16(p_hat) || !cir_aligned16(logits) || !cir_aligned4(temp) || !cir_aligned4(inv_norm))
        return CIR_EALIGN;
    hipLaunchKernelGGL(contrastive_fwd_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p, target, temp, p_hat, inv_norm, logits, Bt, E);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_contrastive_bwd(const float* dlogits, const float* target, const float* temp, const float* p_hat, const float* inv_norm,
                                   float* dp, float* row_scratch, float* dtemp, const float* x, int64_t ldx, const float* W, float* dx, int64_t lddx,
                                   float* dW, float* db, int D, int B, int Bt, int E, int dtype, void* stream) {
    CIR_CHECK_PTR(dlogits); CIR_CHECK_PTR(target); CIR_CHECK_PTR(temp); CIR_CHECK_PTR(p_hat); CIR_CHECK_PTR(inv_norm);
    CIR_CHECK_PTR(dp); CIR_CHECK_PTR(row_scratch); CIR_CHECK_PTR(dtemp);
    const bool proj = x != nullptr || W != nullptr || dx != nullptr || dW != nullptr || db != nullptr;
    if (proj && (x == nullptr || W == nullptr || dx == nullptr || dW == nullptr || db == nullptr || D <= 0)) return CIR_EINVAL;
    if (B <= 0 || Bt <= 0 || E <= 0) return CIR_EINVAL;
    if (dtype != CIR_F32) return CIR_EDTYPE;
    if (!head_shape_ok(E, B, (int64_t)B * Bt)) return CIR_ESHAPE;
    if (proj && (D % 4 != 0 || !head_rows_fit(ldx, B, D) || !head_rows_fit(lddx, B, D))) return CIR_ESHAPE;
    if (!cir_aligned16(dlogits) || !cir_aligned16(target) || !cir_aligned16(p_hat) || !cir_aligned16(dp) || !cir_aligned4(temp) ||
        !cir_aligned4(inv_norm) || !cir_aligned4(row_scratch) || !cir_aligned4(dtemp))
        return CIR_EALIGN;
    if (proj && (!cir_rows_ok(x, ldx) || !cir_rows_ok(dx, lddx) || !cir_aligned16(W) || !cir_aligned16(dW) || !cir_aligned16(db))) return CIR_EALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(contrastive_bwd_rows_kernel, dim3(B), dim3(256), 0, s, dlogits, target, temp, p_hat, inv_norm, dp, row_scratch, Bt, E);
    if (proj) {
        hipLaunchKernelGGL(head_dgrad_kernel, dim3((D + 255) / 256, B), dim3(256), 0, s, dp, W, dx, lddx, E, D);
        hipLaunchKernelGGL(head_wgrad_kernel<false>, dim3((D + 255) / 256, E), dim3(256), 0, s, dp, x, ldx, dW, db, B, E, D);
    }
    hipLaunchKernelGGL(head_dtemp_kernel, dim3(1), dim3(64), 0, s, row_scratch, temp, dtemp, B);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_contrastive_bwd_target(const float* dlogits, const float* p_hat, const float* temp, float* dtarget, int B, int Bt, int E,
                                          int dtype, void* stream) {
    CIR_CHECK_PTR(dlogits); CIR_CHECK_PTR(p_hat); CIR_CHECK_PTR(temp); CIR_CHECK_PTR(dtarget);
    if (B <= 0 || Bt <= 0 || E <= 0) return CIR_EINVAL;
    if (dtype != CIR_F32) return CIR_EDTYPE;
    if (!head_shape_ok(E, B, (int64_t)B * Bt) || Bt > 65535) return CIR_ESHAPE;
    if (!cir_aligned16(dlogits) || !cir_aligned16(p_hat) || !cir_aligned16(dtarget) || !cir_aligned4(temp)) return CIR_EALIGN;
    hipLaunchKernelGGL(contrastive_bwd_target_kernel, dim3(Bt), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), dlogits, p_hat, temp, dtarget,
                       B, Bt, E);
    CIR_LAUNCH_RESULT();
}

static int pooled_head_shape(const float* x, int64_t ldx, int Bt, int E, int D) {
    if (Bt <= 0 || E <= 0 || D <= 0) return CIR_EINVAL;
    if (!head_shape_ok(E, Bt, 0) || D > kPoolMaxD || D % 4 != 0 || !head_rows_fit(ldx, Bt, D)) return CIR_ESHAPE;
    return cir_rows_ok(x, ldx) ? CIR_OK : CIR_EALIGN;
}

extern "C" int cir_pooled_head_fwd(const float* x, int64_t ldx, const float* W, const float* bias, float* t_hat, float* inv_norm, int Bt, int E,
                                   int D, int dtype, void* stream) {
    CIR_CHECK_PTR(x); CIR_CHECK_PTR(W); CIR_CHECK_PTR(bias); CIR_CHECK_PTR(t_hat); CIR_CHECK_PTR(inv_norm);
    if (dtype != CIR_F32) return CIR_EDTYPE;
    const int rc = pooled_head_shape(x, ldx, Bt, E, D);
    if (rc != CIR_OK) return rc;
    if (!cir_aligned16(W) || !cir_aligned16(t_hat) || !cir_aligned4(bias) || !cir_aligned4(inv_norm)) return CIR_EALIGN;
    hipLaunchKernelGGL(pooled_head_fwd_kernel, dim3(Bt), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), x, ldx, W, bias, t_hat, inv_norm, E, D);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_pooled_head_bwd(const float* dt_hat, const float* t_hat, const float* inv_norm, const float* x, int64_t ldx, const float* W,
                                   float* dt, float* dx, int64_t lddx, float* dW, float* db, int Bt, int E, int D, int dtype, void* stream) {
    CIR_CHECK_PTR(dt_hat); CIR_CHECK_PTR(t_hat); CIR_CHECK_PTR(inv_norm); CIR_CHECK_PTR(x); CIR_CHECK_PTR(W); CIR_CHECK_PTR(dt);
    CIR_CHECK_PTR(dW); CIR_CHECK_PTR(db);
    if (dtype != CIR_F32) return CIR_EDTYPE;
    const int rc = pooled_head_shape(x, ldx, Bt, E, D);
    if (rc != CIR_OK) return rc;
    if (dx != nullptr && !head_rows_fit(lddx, Bt, D)) return CIR_ESHAPE;
    if (!cir_aligned16(dt_hat) || !cir_aligned16(t_hat) || !cir_aligned16(dt) || !cir_aligned16(W) || !cir_aligned16(dW) || !cir_aligned4(db) ||
        !cir_aligned4(inv_norm) || (dx != nullptr && !cir_rows_ok(dx, lddx)))
        return CIR_EALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pooled_head_bwd_rows_kernel, dim3(Bt), dim3(256), 0, s, dt_hat, t_hat, inv_norm, dt, E);
    if (dx != nullptr) hipLaunchKernelGGL(head_dgrad_kernel, dim3((D + 255) / 256, Bt), dim3(256), 0, s, dt, W, dx, lddx, E, D);
    hipLaunchKernelGGL(head_wgrad_kernel<true>, dim3((D + 255) / 256, E), dim3(256), 0, s, dt, x, ldx, dW, db, Bt, E, D);
    CIR_LAUNCH_RESULT();
}
