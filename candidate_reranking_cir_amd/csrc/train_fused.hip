// Fused row kernels of the TRAINING pass (round 4).  Round 3 ran every step of BertSelfOutput / BertOutput
// (nlvr_encoder.py:248-264, 399-409: dense -> dropout -> + residual -> LayerNorm) and of its adjoint as its own launch over fp32
// tensors - 41 elementwise and 25 column-sum launches per layer, 17 ms of a 65 ms step.  Here each block of that chain is ONE pass:
//   forward   cir_residual_layernorm_train : pre = dropout(alpha * (t0 + t1)) + residual ; y = LayerNorm(pre)   -> pre, y (fp32), y (16-bit)
//   backward  cir_layernorm_bwd_fused      : d pre from dy ; dgamma, dbeta ; and the gradient that flows back through the dropout to
//                                            the dense layer, alpha * dropout'(d pre + t_add), as the 16-bit operand of that layer's
//                                            dgrad / wgrad products together with its column sums (the dense layer's bias gradient)
//             cir_rows16_colsum            : column sums of a 16-bit gradient (bias gradients behind the attention adjoints), or
//                                            dz = df * gelu'(z) on 16-bit tensors with the column sums of dz in the same pass
// Gradients between the dense layers travel as 16-bit tensors (what autocast's backward gives the reference, stage2_train.py:208-216);
// the residual-stream gradient stays fp32.
#include "common.hpp"

namespace cir {

constexpr int kRowVec = 4;       // float4 groups per lane: cols <= 1024, cols % 4 == 0

template <typename T>
__device__ __forceinline__ void store4(T* p, const float (&v)[4]) {
    typedef __attribute__((ext_vector_type(4))) T t4;
    t4 o = {static_cast<T>(v[0]), static_cast<T>(v[1]), static_cast<T>(v[2]), static_cast<T>(v[3])};
    *reinterpret_cast<t4*>(p) = o;
}

// ---- forward: dropout + residual + LayerNorm, one wave per row ------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void res_ln_train_kernel(const float* t0, const float* t1, const float* res, const float* gamma, const float* beta,
                                                           float* pre, float* y32, T* y16, int64_t rows, int cols, float eps, float alpha,
                                                           float p_drop, uint64_t seed) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= rows) return;
    const float keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    const int64_t base = row * cols;
    const uint32_t rkey = drop_row_key(seed, (uint64_t)row), thr = drop_threshold(p_drop);
    float v[kRowVec][4];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kRowVec; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < cols) {
            float4 a = *reinterpret_cast<const float4*>(t0 + base + c);
            if (t1 != nullptr) {
                const float4 b = *reinterpret_cast<const float4*>(t1 + base + c);
                a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
            }
            const float4 r = *reinterpret_cast<const float4*>(res + base + c);
            const float tv[4] = {a.x, a.y, a.z, a.w}, rv[4] = {r.x, r.y, r.z, r.w};
            const uint32_t b01 = thr ? drop_bits(rkey, c) : 0u, b23 = thr ? drop_bits(rkey, c + 2) : 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool kept = drop_kept(e < 2 ? b01 : b23, (uint32_t)e, thr);
                v[i][e] = (kept ? tv[e] * alpha * keep : 0.f) + rv[e];
                s += v[i][e];
            }
            *reinterpret_cast<float4*>(pre + base + c) = make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[i][e] = 0.f;
        }
    }
    const float mean = wave_sum(s) / cols;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kRowVec; ++i)
        if ((lane + 64 * i) * 4 < cols) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; q += d * d; }
        }
    const float rstd = rsqrtf(wave_sum(q) / cols + eps);
#pragma unroll
    for (int i = 0; i < kRowVec; ++i) {
        const int c = (lane + 64 * i) * 4;
        if (c < cols) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c), b = *reinterpret_cast<const float4*>(beta + c);
            const float gv[4] = {g.x, g.y, g.z, g.w}, bv[4] = {b.x, b.y, b.z, b.w};
            float y[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * rstd * gv[e] + bv[e];
            if (y32 != nullptr) *reinterpret_cast<float4*>(y32 + base + c) = make_float4(y[0], y[1], y[2], y[3]);
            if (y16 != nullptr) store4<T>(y16 + base + c, y);
        }
    }
}

// ---- backward: LayerNorm adjoint + the dropout adjoint of the dense branch + that branch's bias gradient -------------------------
// One wave per row; the per-column sums (dgamma, dbeta, bias gradient) of a block's rows stay in registers and are added once per block.
// Rows per block trade those atomics against occupancy: at 8192 rows, 32 rows per block are 256 blocks = ONE wave per SIMD, each walking
// its rows serially through two wave reductions; fewer rows per block were measured and lose (see the launch).
// ORD (deterministic mode, cir_layernorm_bwd_fused_ordered): the block stores its sums to row blockIdx.x of `part` (dgamma | dbeta | bias
// gradient, `cols` each; the third only when a bias gradient is wanted) instead of adding them.
template <typename T, int ITERS, bool ORD>      // 4 * ITERS rows per block (one wave per row at a time)
__global__ __launch_bounds__(256) void ln_bwd_fused_kernel(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta,
                                                           const float* t_add, T* dt16, float* db1, float* db2, int64_t rows, int cols, float eps,
                                                           float alpha, float p_drop, uint64_t seed, float* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    const uint32_t thr = drop_threshold(p_drop);
    float pg[kRowVec][4], pb[kRowVec][4], pd[kRowVec][4];
#pragma unroll
    for (int i = 0; i < kRowVec; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) { pg[i][e] = 0.f; pb[i][e] = 0.f; pd[i][e] = 0.f; }
    float gv[kRowVec][4];
#pragma unroll
    for (int i = 0; i < kRowVec; ++i) {
        const int c = (lane + 64 * i) * 4;
        const float4 g = c < cols ? *reinterpret_cast<const float4*>(gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        gv[i][0] = g.x; gv[i][1] = g.y; gv[i][2] = g.z; gv[i][3] = g.w;
    }
    for (int it = 0; it < ITERS; ++it) {
        const int64_t row = (int64_t)blockIdx.x * (4 * ITERS) + it * 4 + wave;
        if (row >= rows) break;
        const int64_t base = row * cols;
        const uint32_t rkey = drop_row_key(seed, (uint64_t)row);
        float xv[kRowVec][4], dv[kRowVec][4];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kRowVec; ++i) {
            const int c = (lane + 64 * i) * 4;
            const bool in = c < cols;
            const float4 a = in ? *reinterpret_cast<const float4*>(x + base + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 d = in ? *reinterpret_cast<const float4*>(dy + base + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            xv[i][0] = a.x; xv[i][1] = a.y; xv[i][2] = a.z; xv[i][3] = a.w;
            dv[i][0] = d.x; dv[i][1] = d.y; dv[i][2] = d.z; dv[i][3] = d.w;
            s += (a.x + a.y) + (a.z + a.w);
        }
        const float mean = wave_sum(s) / cols;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < kRowVec; ++i)
            if ((lane + 64 * i) * 4 < cols) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = xv[i][e] - mean; q += d * d; }
            }
        const float rstd = rsqrtf(wave_sum(q) / cols + eps);
        float a = 0.f, b = 0.f;           // mean(dy*gamma), mean(dy*gamma*xhat)
#pragma unroll
        for (int i = 0; i < kRowVec; ++i)
            if ((lane + 64 * i) * 4 < cols) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    xv[i][e] = (xv[i][e] - mean) * rstd;                           // xhat from here on
                    const float gq = dv[i][e] * gv[i][e];
                    a += gq; b += gq * xv[i][e];
                }
            }
        a = wave_sum(a) / cols; b = wave_sum(b) / cols;
#pragma unroll
        for (int i = 0; i < kRowVec; ++i) {
            const int c = (lane + 64 * i) * 4;
            if (c < cols) {
                float r[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    r[e] = rstd * (dv[i][e] * gv[i][e] - a - xv[i][e] * b);
                    pg[i][e] += dv[i][e] * xv[i][e];
                    pb[i][e] += dv[i][e];
                }
                if (dx != nullptr) *reinterpret_cast<float4*>(dx + base + c) = make_float4(r[0], r[1], r[2], r[3]);
                if (dt16 != nullptr) {
                    if (t_add != nullptr) {
                        const float4 t = *reinterpret_cast<const float4*>(t_add + base + c);
                        r[0] += t.x; r[1] += t.y; r[2] += t.z; r[3] += t.w;
                    }
                    const uint32_t b01 = thr ? drop_bits(rkey, c) : 0u, b23 = thr ? drop_bits(rkey, c + 2) : 0u;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool kept = drop_kept(e < 2 ? b01 : b23, (uint32_t)e, thr);
                        r[e] = kept ? r[e] * alpha * keep : 0.f;
                        pd[i][e] += r[e];
                    }
                    store4<T>(dt16 + base + c, r);
                }
            }
        }
    }
    __shared__ float red[4][64 * kRowVec * 4];
    const bool bias = dt16 != nullptr && db1 != nullptr;
    for (int pass = 0; pass < (bias ? 3 : 2); ++pass) {
        if (pass) __syncthreads();
#pragma unroll
        for (int i = 0; i < kRowVec; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) red[wave][(lane + 64 * i) * 4 + e] = pass == 0 ? pg[i][e] : pass == 1 ? pb[i][e] : pd[i][e];
        __syncthreads();
        for (int c = threadIdx.x; c < cols; c += 256) {
            const float v = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
            if constexpr (ORD) { part[((int64_t)blockIdx.x * (bias ? 3 : 2) + pass) * cols + c] = v; continue; }
            if (pass == 0) atomicAdd(dgamma + c, v);
            else if (pass == 1) atomicAdd(dbeta + c, v);
            else { atomicAdd(db1 + c, v); if (db2 != nullptr) atomicAdd(db2 + c, v); }
        }
    }
}

// ---- 16-bit rows: column sums, optionally behind dz = a * gelu'(z) -----------------------------------------------------------------
// block = 32 column groups (8 columns each: one 16-byte load) x 8 row lanes, 64 rows per block; column sums over the block's rows in
// registers, then across the row lanes through LDS, one atomic per column and block.
// ORD (deterministic mode, cir_rows16_colsum_ordered): `sums` is the partial workspace, the block stores to its row blockIdx.y.
template <typename T, int MODE, bool ORD>      // MODE 0: sums of a;  1: out = a * gelu'(z), sums of out
__global__ __launch_bounds__(256) void rows16_colsum_kernel(const T* a, int64_t lda, const T* z, int64_t ldz, T* out, int64_t ldo, float* sums,
                                                            int64_t rows, int cols) {
    typedef typename Elem<T>::x8 X8;
    const int cg = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = (blockIdx.x * 32 + cg) * 8;
    const int64_t r0 = (int64_t)blockIdx.y * 64;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (c < cols) {
#pragma unroll 2
        for (int it = 0; it < 8; ++it) {
            const int64_t r = r0 + it * 8 + rl;
            if (r >= rows) break;
            const X8 av = *reinterpret_cast<const X8*>(a + r * lda + c);
            if (MODE == 1) {
                const X8 zv = *reinterpret_cast<const X8*>(z + r * ldz + c);
                X8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float v = static_cast<float>(av[e]) * gelu_grad(static_cast<float>(zv[e]));
                    o[e] = static_cast<T>(v);
                    acc[e] += v;
                }
                *reinterpret_cast<X8*>(out + r * ldo + c) = o;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] += static_cast<float>(av[e]);
            }
        }
    }
    if (sums == nullptr) return;
    __shared__ float red[8][256 + 8];
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rl][cg * 8 + e] = acc[e];
    __syncthreads();
    const int cc = blockIdx.x * 256 + threadIdx.x;
    if (cc < cols) {
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) v += red[j][threadIdx.x];
        if constexpr (ORD) sums[(int64_t)blockIdx.y * cols + cc] = v;
        else atomicAdd(sums + cc, v);
    }
}

// ---- 16-bit rows: dz = a * gelu'(z) AND f = gelu(z) from one read of z, with the column sums of dz --------------------------------------
// The backward of a CHECKPOINTED ViT block (vit.py:36-37, 103-105): gelu(z) was released with the forward, and fc2's weight gradient wants
// it back as its left operand.  z (3072 / 4096 columns) is the widest tensor of the block; this pass reads it anyway for dz.  Same block
// shape and the same reduction as rows16_colsum_kernel MODE 1 (whose dz and sums it reproduces bit for bit), gelu_exact as cir_eltwise
// mode 0 evaluates it.  ORD: `sums` is the partial workspace, the block stores to its row blockIdx.y.
template <typename T, bool ORD>
__global__ __launch_bounds__(256) void rows16_gelu_pair_kernel(const T* a, int64_t lda, const T* z, int64_t ldz, T* out, int64_t ldo, T* outf, int64_t ldf,
                                                               float* sums, int64_t rows, int cols) {
    typedef typename Elem<T>::x8 X8;
    const int cg = threadIdx.x & 31, rl = threadIdx.x >> 5;
    const int c = (blockIdx.x * 32 + cg) * 8;
    const int64_t r0 = (int64_t)blockIdx.y * 64;
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    if (c < cols) {
#pragma unroll 2
        for (int it = 0; it < 8; ++it) {
            const int64_t r = r0 + it * 8 + rl;
            if (r >= rows) break;
            const X8 av = *reinterpret_cast<const X8*>(a + r * lda + c);
            const X8 zv = *reinterpret_cast<const X8*>(z + r * ldz + c);
            X8 o, f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float zf = static_cast<float>(zv[e]);
                const float v = static_cast<float>(av[e]) * gelu_grad(zf);
                o[e] = static_cast<T>(v);
                acc[e] += v;
                f[e] = static_cast<T>(gelu_exact(zf));
            }
            *reinterpret_cast<X8*>(out + r * ldo + c) = o;
            *reinterpret_cast<X8*>(outf + r * ldf + c) = f;
        }
    }
    if (sums == nullptr) return;
    __shared__ float red[8][256 + 8];
#pragma unroll
    for (int e = 0; e < 8; ++e) red[rl][cg * 8 + e] = acc[e];
    __syncthreads();
    const int cc = blockIdx.x * 256 + threadIdx.x;
    if (cc < cols) {
        float v = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) v += red[j][threadIdx.x];
        if constexpr (ORD) sums[(int64_t)blockIdx.y * cols + cc] = v;
        else atomicAdd(sums + cc, v);
    }
}

// ---- out = a + s[row / rows_per_group] * b : a per-GROUP scale of a branch added to the stream (DropPath: timm's per-sample stochastic
// depth, vit.py:98-109), or with a = NULL the scaled branch gradient written as the 16-bit operand of the adjoint products
template <typename TO>
__global__ __launch_bounds__(256) void rows_scale_add_kernel(const float* a, const float* b, const float* scale, TO* out, int64_t rows, int cols,
                                                             int64_t rows_per_group) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= rows * cols) return;
    const float sc = scale[(i / cols) / rows_per_group];
    const float4 bv = *reinterpret_cast<const float4*>(b + i);
    float r[4] = {bv.x * sc, bv.y * sc, bv.z * sc, bv.w * sc};
    if (a != nullptr) {
        const float4 av = *reinterpret_cast<const float4*>(a + i);
        r[0] += av.x; r[1] += av.y; r[2] += av.z; r[3] += av.w;
    }
    if constexpr (sizeof(TO) == 4) *reinterpret_cast<float4*>(out + i) = make_float4(r[0], r[1], r[2], r[3]);
    else store4<TO>(out + i, r);
}

}  // namespace cir

using namespace cir;

extern "C" int cir_rows_scale_add(const float* a, const float* b, const float* scale, void* out, int64_t rows, int cols, int64_t rows_per_group,
                                  int out_dtype, void* stream) {
    CIR_CHECK_PTR(b); CIR_CHECK_PTR(scale); CIR_CHECK_PTR(out);
    if (rows <= 0 || cols <= 0 || rows_per_group <= 0) return CIR_EINVAL;
    if (cols % 4 != 0) return CIR_ESHAPE;
    if (!cir_aligned16(a) || !cir_aligned16(b) || (reinterpret_cast<uintptr_t>(out) & (out_dtype == CIR_F32 ? 15u : 7u))) return CIR_EALIGN;
    const int64_t n4 = rows * cols / 4;
    dim3 grid((unsigned)((n4 + 255) / 256)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (out_dtype != CIR_F32 && out_dtype != CIR_BF16 && out_dtype != CIR_F16) return CIR_EDTYPE;
    by_dtype3(out_dtype, [&](auto t) {
        using TO = typename decltype(t)::type;
        hipLaunchKernelGGL((rows_scale_add_kernel<TO>), grid, block, 0, s, a, b, scale, reinterpret_cast<TO*>(out), rows, cols, rows_per_group);
    });
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_residual_layernorm_train(const float* t0, const float* t1, const float* residual, const float* gamma, const float* beta, float* pre,
                                            float* y32, void* y16, int64_t rows, int cols, float eps, float alpha, float p_drop, uint64_t seed,
                                            int dtype16, void* stream) {
    CIR_CHECK_PTR(t0); CIR_CHECK_PTR(residual); CIR_CHECK_PTR(gamma); CIR_CHECK_PTR(beta); CIR_CHECK_PTR(pre);
    if (rows <= 0 || cols <= 0 || p_drop < 0.f || p_drop >= 1.f) return CIR_EINVAL;
    if (cols % 4 != 0 || cols > 256 * kRowVec) return CIR_ESHAPE;
    if (dtype16 != CIR_BF16 && dtype16 != CIR_F16) return CIR_EDTYPE;
    if (!cir_aligned16(t0) || !cir_aligned16(t1) || !cir_aligned16(residual) || !cir_aligned16(pre) || !cir_aligned16(y32) || !cir_aligned16(gamma) ||
        !cir_aligned16(beta) || (reinterpret_cast<uintptr_t>(y16) & 7u)) return CIR_EALIGN;
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype16(dtype16, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((res_ln_train_kernel<T>), grid, block, 0, s, t0, t1, residual, gamma, beta, pre, y32, reinterpret_cast<T*>(y16), rows, cols,
                           eps, alpha, p_drop, seed);
    });
    CIR_LAUNCH_RESULT();
}

// validation shared by cir_layernorm_bwd_fused and its ordered form
static int ln_bwd_fused_check(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, const float* t_add,
                              void* dt16, int64_t rows, int cols, float p_drop, int dtype16) {
    CIR_CHECK_PTR(x); CIR_CHECK_PTR(gamma); CIR_CHECK_PTR(dy); CIR_CHECK_PTR(dgamma); CIR_CHECK_PTR(dbeta);
    if (dx == nullptr && dt16 == nullptr) return CIR_EINVAL;
    if (rows <= 0 || cols <= 0 || p_drop < 0.f || p_drop >= 1.f) return CIR_EINVAL;
    if (cols % 4 != 0 || cols > 256 * kRowVec) return CIR_ESHAPE;
    if (dtype16 != CIR_BF16 && dtype16 != CIR_F16) return CIR_EDTYPE;
    if (!cir_aligned16(x) || !cir_aligned16(gamma) || !cir_aligned16(dy) || !cir_aligned16(dx) || !cir_aligned16(t_add) ||
        (reinterpret_cast<uintptr_t>(dt16) & 7u)) return CIR_EALIGN;
    return CIR_OK;
}

extern "C" int cir_layernorm_bwd_fused(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, const float* t_add,
                                       void* dt16, float* dbias, float* dbias2, int64_t rows, int cols, float eps, float alpha, float p_drop,
                                       uint64_t seed, int dtype16, void* stream) {
    const int bad = ln_bwd_fused_check(x, gamma, dy, dx, dgamma, dbeta, t_add, dt16, rows, cols, p_drop, dtype16);
    if (bad != CIR_OK) return bad;
    // 32 rows per block.  Measured (tools, round 4; 8192 x 768, dropout + bias sums on): 32 rows 30.6 us, 16 rows 29.6 us, 8 rows 43.3 us -
    // the column-sum atomics (3 x 768 per block) outweigh the occupancy gained
    dim3 block(256), grid((unsigned)((rows + 31) / 32));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype16(dtype16, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((ln_bwd_fused_kernel<T, 8, false>), grid, block, 0, s, x, gamma, dy, dx, dgamma, dbeta, t_add, reinterpret_cast<T*>(dt16),
                           dbias, dbias2, rows, cols, eps, alpha, p_drop, seed, (float*)nullptr);
    });
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_layernorm_bwd_fused_ordered(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta,
                                               const float* t_add, void* dt16, float* dbias, float* dbias2, int64_t rows, int cols, float eps,
                                               float alpha, float p_drop, uint64_t seed, int dtype16, float* partials, int64_t partial_elems,
                                               void* stream) {
    const int bad = ln_bwd_fused_check(x, gamma, dy, dx, dgamma, dbeta, t_add, dt16, rows, cols, p_drop, dtype16);
    if (bad != CIR_OK) return bad;
    CIR_CHECK_PTR(partials);
    const bool bias = dt16 != nullptr && dbias != nullptr;                      // (as the kernel: dbias2 counts only beside dbias)
    const int64_t blocks = (rows + 31) / 32;
    if (partial_elems < blocks * (bias ? 3 : 2) * cols) return CIR_ESHAPE;
    dim3 block(256), grid((unsigned)blocks);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype16(dtype16, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((ln_bwd_fused_kernel<T, 8, true>), grid, block, 0, s, x, gamma, dy, dx, dgamma, dbeta, t_add, reinterpret_cast<T*>(dt16),
                           dbias, dbias2, rows, cols, eps, alpha, p_drop, seed, partials);
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    OrderedDst d{};
    d.out[0] = dgamma; d.out[1] = dbeta; d.src[1] = 1; d.nout = 2;
    if (bias) {
        d.out[2] = dbias; d.src[2] = 2; d.nout = 3;
        if (dbias2 != nullptr) { d.out[3] = dbias2; d.src[3] = 2; d.nout = 4; }
    }
    return colsum_ordered_launch(partials, (int64_t)(bias ? 3 : 2) * cols, blocks, cols, d, s);
}

static int rows16_colsum(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, float* sums, int64_t rows, int cols,
                         int mode, int dtype, float* partials, int64_t partial_elems, void* stream) {
    const bool ord = partials != nullptr;
    CIR_CHECK_PTR(a);
    if (rows <= 0 || cols <= 0 || mode < 0 || mode > 1) return CIR_EINVAL;
    if (mode == 0 && sums == nullptr) return CIR_EINVAL;
    if (mode == 1 && (z == nullptr || out == nullptr)) return CIR_EINVAL;
    if (cols % 8 != 0 || lda % 8 != 0 || (mode == 1 && (ldz % 8 != 0 || ldo % 8 != 0))) return CIR_ESHAPE;
    if (dtype != CIR_BF16 && dtype != CIR_F16) return CIR_EDTYPE;
    if (!cir_aligned16(a) || !cir_aligned16(z) || !cir_aligned16(out)) return CIR_EALIGN;
    const int64_t row_blocks = (rows + 63) / 64;
    if (row_blocks > 65535) return CIR_ESHAPE;
    if (ord && partial_elems < row_blocks * cols) return CIR_ESHAPE;
    dim3 grid((cols + 255) / 256, (unsigned)row_blocks), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype16(dtype, [&](auto t) { by_bool(mode != 0, [&](auto md) { by_bool(ord, [&](auto od) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((rows16_colsum_kernel<T, decltype(md)::value ? 1 : 0, decltype(od)::value>), grid, block, 0, s, reinterpret_cast<const T*>(a), lda,
                           reinterpret_cast<const T*>(z), ldz, reinterpret_cast<T*>(out), ldo, ord ? partials : sums, rows, cols);
    }); }); });
    if (!ord) CIR_LAUNCH_RESULT();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    OrderedDst d{};
    d.out[0] = sums; d.nout = 1;
    return colsum_ordered_launch(partials, cols, row_blocks, cols, d, s);
}

extern "C" int cir_rows16_colsum(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, float* sums, int64_t rows, int cols,
                                 int mode, int dtype, void* stream) {
    return rows16_colsum(a, lda, z, ldz, out, ldo, sums, rows, cols, mode, dtype, nullptr, 0, stream);
}

extern "C" int cir_rows16_colsum_ordered(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, float* sums, int64_t rows,
                                         int cols, int mode, int dtype, float* partials, int64_t partial_elems, void* stream) {
    CIR_CHECK_PTR(sums); CIR_CHECK_PTR(partials);
    return rows16_colsum(a, lda, z, ldz, out, ldo, sums, rows, cols, mode, dtype, partials, partial_elems, stream);
}

// The pair pass of a checkpointed ViT block: argument checks of the rows16 family, then one launch (+ the finishing sum of the ordered form)
static int rows16_gelu_pair(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, void* out_f, int64_t ldf, float* sums,
                            int64_t rows, int cols, int dtype, bool ord, float* partials, int64_t partial_elems, void* stream) {
    CIR_CHECK_PTR(a); CIR_CHECK_PTR(z); CIR_CHECK_PTR(out); CIR_CHECK_PTR(out_f);
    if (ord) CIR_CHECK_PTR(partials);
    if (rows <= 0 || cols <= 0) return CIR_EINVAL;
    if (cols % 8 != 0) return CIR_ESHAPE;
    if (lda % 8 != 0 || ldz % 8 != 0 || ldo % 8 != 0 || ldf % 8 != 0) return CIR_EALIGN;
    if (lda < cols || ldz < cols || ldo < cols || ldf < cols) return CIR_ESHAPE;
    if (dtype != CIR_BF16 && dtype != CIR_F16) return CIR_EDTYPE;
    if (!cir_aligned16(a) || !cir_aligned16(z) || !cir_aligned16(out) || !cir_aligned16(out_f)) return CIR_EALIGN;
    const int64_t row_blocks = (rows + 63) / 64;
    if (row_blocks > 65535) return CIR_ESHAPE;
    ord = ord && sums != nullptr;                                              // no sums wanted: nothing to order
    if (ord && partial_elems < row_blocks * cols) return CIR_ESHAPE;
    dim3 grid((cols + 255) / 256, (unsigned)row_blocks), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype16(dtype, [&](auto t) { by_bool(ord, [&](auto od) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((rows16_gelu_pair_kernel<T, decltype(od)::value>), grid, block, 0, s, reinterpret_cast<const T*>(a), lda,
                           reinterpret_cast<const T*>(z), ldz, reinterpret_cast<T*>(out), ldo, reinterpret_cast<T*>(out_f), ldf, ord ? partials : sums,
                           rows, cols);
    }); });
    if (!ord) CIR_LAUNCH_RESULT();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    OrderedDst d{};
    d.out[0] = sums; d.nout = 1;
    return colsum_ordered_launch(partials, cols, row_blocks, cols, d, s);
}

extern "C" int cir_rows16_gelu_pair(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, void* out_f, int64_t ldf,
                                    float* sums, int64_t rows, int cols, int dtype, void* stream) {
    return rows16_gelu_pair(a, lda, z, ldz, out, ldo, out_f, ldf, sums, rows, cols, dtype, false, nullptr, 0, stream);
}

extern "C" int cir_rows16_gelu_pair_ordered(const void* a, int64_t lda, const void* z, int64_t ldz, void* out, int64_t ldo, void* out_f, int64_t ldf,
                                            float* sums, int64_t rows, int cols, int dtype, float* partials, int64_t partial_elems, void* stream) {
    return rows16_gelu_pair(a, lda, z, ldz, out, ldo, out_f, ldf, sums, rows, cols, dtype, true, partials, partial_elems, stream);
}
