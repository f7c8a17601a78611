// Training-mode operators of the two-branch encoder (BLIP_NLVR.img_txt_fusion in train() mode + backward,
// blip_stage2.py:65-99 driven by stage2_train.py:202-216).  The dense Linear layers keep running on the MFMA GEMM
// (cir_gemm_bias_act: forward and dgrad, the latter through a transposed weight copy; wgrad is cir_bmm reading dy and x as stored); this file holds
// the stand-alone row and elementwise operators the training pass needs besides: row softmax with additive mask and counter-based dropout
// (+ backward), LayerNorm backward, GELU / ReLU forward-backward, dropout, column sums, embedding scatter-add.  The transposes and the
// batched matmul are in train_bmm.hip, AdamW in train_optim.hip, the stage-I heads in train_head.hip.  None of it is on the inference path.

#include "common.hpp"

namespace cir {

// counter-based uniform in [0, 1): one 64-bit mix (splitmix64) of (seed, element index) - the same mask is regenerated in
// the backward pass from the same (seed, index), no mask tensor is stored
__device__ __forceinline__ float uniform01(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(z >> 40) * (1.0f / 16777216.0f);
}

// ---- row softmax with additive key mask and dropout: P = softmax(S * scale + mask), Pd = dropout(P) ----------------------
// one wave per row; S fp32 (rows, cols) with leading dimension lds_; mask fp32 (cols) per group of `rows_per_mask` rows or NULL.
// Rows up to 64 * kSmCols columns are held in registers (one pass over S / dPd); longer rows take the re-reading loops.
constexpr int kSmCols = 12;      // 768 columns: the 577 / 197 image tokens and any caption length
template <typename T>
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* S, int64_t ld_s, const float* mask, int64_t rows_per_mask, int64_t ld_mask,
                                                          T* P, T* Pd, int64_t ld_p, int64_t rows, int cols, float scale, float p_drop, uint64_t seed) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* sr = S + row * ld_s;
    const float* mr = mask ? mask + (row / rows_per_mask) * ld_mask : nullptr;
    const float keep = 1.0f / (1.0f - p_drop);
    if (cols <= 64 * kSmCols) {
        float v[kSmCols];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < kSmCols; ++i) {
            const int c = lane + i * 64;
            v[i] = c < cols ? fmaf(sr[c], scale, mr ? mr[c] : 0.f) : -INFINITY;
            mx = fmaxf(mx, v[i]);
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < kSmCols; ++i) { v[i] = (lane + i * 64 < cols) ? __expf(v[i] - mx) : 0.f; sum += v[i]; }
        const float inv = 1.0f / wave_sum(sum);
#pragma unroll
        for (int i = 0; i < kSmCols; ++i) {
            const int c = lane + i * 64;
            if (c < cols) {
                const float p = v[i] * inv;
                P[row * ld_p + c] = static_cast<T>(p);
                const bool kept = p_drop <= 0.f || uniform01(seed, (uint64_t)row * (uint64_t)cols + c) >= p_drop;
                Pd[row * ld_p + c] = static_cast<T>(kept ? p * (p_drop > 0.f ? keep : 1.0f) : 0.f);
            }
        }
        return;
    }
    float mx = -INFINITY;
    for (int c = lane; c < cols; c += 64) mx = fmaxf(mx, fmaf(sr[c], scale, mr ? mr[c] : 0.f));
    mx = wave_max(mx);
    float sum = 0.f;
    for (int c = lane; c < cols; c += 64) sum += __expf(fmaf(sr[c], scale, mr ? mr[c] : 0.f) - mx);
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
    for (int c = lane; c < cols; c += 64) {
        const float p = __expf(fmaf(sr[c], scale, mr ? mr[c] : 0.f) - mx) * inv;
        P[row * ld_p + c] = static_cast<T>(p);
        const bool kept = p_drop <= 0.f || uniform01(seed, (uint64_t)row * (uint64_t)cols + c) >= p_drop;
        Pd[row * ld_p + c] = static_cast<T>(kept ? p * (p_drop > 0.f ? keep : 1.0f) : 0.f);
    }
}

// dS = scale * P * (dP - sum_c dP * P) with dP = dropout-backward(dPd): rows as in the forward, dPd fp32, dS 16-bit
template <typename T>
__global__ __launch_bounds__(256) void softmax_bwd_kernel(const T* P, int64_t ld_p, const float* dPd, int64_t ld_d, T* dS, int64_t ld_ds,
                                                          int64_t rows, int cols, float scale, float p_drop, uint64_t seed) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    if (cols <= 64 * kSmCols) {
        float dp[kSmCols], pv[kSmCols];
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < kSmCols; ++i) {
            const int c = lane + i * 64;
            dp[i] = 0.f; pv[i] = 0.f;
            if (c < cols) {
                const bool kept = p_drop <= 0.f || uniform01(seed, (uint64_t)row * (uint64_t)cols + c) >= p_drop;
                dp[i] = kept ? dPd[row * ld_d + c] * keep : 0.f;
                pv[i] = static_cast<float>(P[row * ld_p + c]);
                dot += dp[i] * pv[i];
            }
        }
        dot = wave_sum(dot);
#pragma unroll
        for (int i = 0; i < kSmCols; ++i) {
            const int c = lane + i * 64;
            if (c < cols) dS[row * ld_ds + c] = static_cast<T>(scale * pv[i] * (dp[i] - dot));
        }
        return;
    }
    float dot = 0.f;
    for (int c = lane; c < cols; c += 64) {
        const bool kept = p_drop <= 0.f || uniform01(seed, (uint64_t)row * (uint64_t)cols + c) >= p_drop;
        const float dp = kept ? dPd[row * ld_d + c] * keep : 0.f;
        dot += dp * static_cast<float>(P[row * ld_p + c]);
    }
    dot = wave_sum(dot);
    for (int c = lane; c < cols; c += 64) {
        const bool kept = p_drop <= 0.f || uniform01(seed, (uint64_t)row * (uint64_t)cols + c) >= p_drop;
        const float dp = kept ? dPd[row * ld_d + c] * keep : 0.f;
        dS[row * ld_ds + c] = static_cast<T>(scale * static_cast<float>(P[row * ld_p + c]) * (dp - dot));
    }
}

// ---- LayerNorm backward: y = (x - mean) * rstd * gamma + beta over `cols`; x fp32 (the saved pre-LN sum) -----------------
// dx fp32 (written), dgamma / dbeta fp32 (atomically accumulated: zero them first).  One wave per row, 32 rows per block: the
// per-column sums of those rows are kept in registers (cols <= 64 * kLnCols) and added once per block, not once per row.
// ORD (deterministic mode, cir_layernorm_bwd_ordered): the block stores its sums to row blockIdx.x of `part` (2 * cols: dgamma | dbeta) instead.
constexpr int kLnCols = 16;      // columns per lane: cols <= 1024
template <bool ORD>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta,
                                                            int64_t rows, int cols, float eps, float* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float pg[kLnCols], pb[kLnCols];
#pragma unroll
    for (int i = 0; i < kLnCols; ++i) { pg[i] = 0.f; pb[i] = 0.f; }
    for (int it = 0; it < 8; ++it) {
        const int64_t row = (int64_t)blockIdx.x * 32 + it * 4 + wave;
        if (row >= rows) break;
        const float* xr = x + row * cols;
        const float* dr = dy + row * cols;
        float xv[kLnCols], dv[kLnCols];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kLnCols; ++i) {
            const int c = lane + i * 64;
            xv[i] = c < cols ? xr[c] : 0.f;
            dv[i] = c < cols ? dr[c] : 0.f;
            s += xv[i];
        }
        const float mean = wave_sum(s) / cols;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < kLnCols; ++i) { const float d = (lane + i * 64 < cols) ? xv[i] - mean : 0.f; q += d * d; }
        const float rstd = rsqrtf(wave_sum(q) / cols + eps);
        float a = 0.f, b = 0.f;           // mean(dy*gamma), mean(dy*gamma*xhat)
#pragma unroll
        for (int i = 0; i < kLnCols; ++i) {
            const int c = lane + i * 64;
            if (c < cols) {
                const float xh = (xv[i] - mean) * rstd, gq = dv[i] * gamma[c];
                a += gq; b += gq * xh;
            }
        }
        a = wave_sum(a) / cols; b = wave_sum(b) / cols;
#pragma unroll
        for (int i = 0; i < kLnCols; ++i) {
            const int c = lane + i * 64;
            if (c < cols) {
                const float xh = (xv[i] - mean) * rstd, gq = dv[i] * gamma[c];
                dx[row * cols + c] = rstd * (gq - a - xh * b);
                pg[i] += dv[i] * xh;
                pb[i] += dv[i];
            }
        }
    }
    __shared__ float red[2][4][64 * kLnCols];
#pragma unroll
    for (int i = 0; i < kLnCols; ++i) { red[0][wave][lane + i * 64] = pg[i]; red[1][wave][lane + i * 64] = pb[i]; }
    __syncthreads();
    for (int c = threadIdx.x; c < cols; c += 256) {
        if constexpr (ORD) {
            float* pr = part + (int64_t)blockIdx.x * 2 * cols;
            pr[c] = red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c];
            pr[cols + c] = red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c];
        } else {
            atomicAdd(dgamma + c, red[0][0][c] + red[0][1][c] + red[0][2][c] + red[0][3][c]);
            atomicAdd(dbeta + c, red[1][0][c] + red[1][1][c] + red[1][2][c] + red[1][3][c]);
        }
    }
}

// ---- elementwise ------------------------------------------------------------------------------------------------------------
// mode 0: y = gelu(z); 1: dz = dy * gelu'(z); 2: y = relu(z); 3: dz = dy * (z > 0); 4: y = dropout(z) [dy unused]; 5: y = z + dy (add);
// 6: y = p_drop * z (scale by the factor passed in p_drop)
// (Tried in round 4: the logistic-fit GELU of the inference epilogue for 16-bit outputs - the 2R x 3072 pass went 58 -> 54 us, it is bound
//  by its 200 MB of traffic, not by erff - at the price of moving train197's worst same-piece gradient 1.5e-2 -> 1.75e-2: dropped.)
__device__ __forceinline__ float eltwise_op(float v, float d, int mode, float p_drop, float keep, uint64_t seed, int64_t i) {
    switch (mode) {
        case 0: return gelu_exact(v);
        case 1: return d * gelu_grad(v);
        case 2: return fmaxf(v, 0.f);
        case 3: return v > 0.f ? d : 0.f;
        case 4: return (p_drop <= 0.f || uniform01(seed, (uint64_t)i) >= p_drop) ? v * keep : 0.f;
        case 5: return v + d;
        default: return v * p_drop;
    }
}

template <typename TZ, typename TO>
__global__ __launch_bounds__(256) void eltwise_kernel(const TZ* z, const float* dy, TO* out, int64_t n, int mode, float p_drop, uint64_t seed, int vec) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;         // four consecutive elements per thread
    if (i0 >= n) return;
    const float keep = p_drop > 0.f ? 1.0f / (1.0f - p_drop) : 1.0f;
    const bool use_dy = mode == 1 || mode == 3 || mode == 5;
    if (vec && i0 + 4 <= n) {                                                   // 16-byte fp32 accesses (host checked the alignment)
        float v[4], d[4] = {0.f, 0.f, 0.f, 0.f}, r[4];
        if constexpr (sizeof(TZ) == 4) {
            const float4 z4 = *reinterpret_cast<const float4*>(z + i0);
            v[0] = z4.x; v[1] = z4.y; v[2] = z4.z; v[3] = z4.w;
        } else {
            typedef __attribute__((ext_vector_type(4))) TZ tz4;                // one 8-byte load (i0 is a multiple of 4, the base 16-byte aligned)
            const tz4 z4 = *reinterpret_cast<const tz4*>(z + i0);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = static_cast<float>(z4[e]);
        }
        if (use_dy) {
            const float4 d4 = *reinterpret_cast<const float4*>(dy + i0);
            d[0] = d4.x; d[1] = d4.y; d[2] = d4.z; d[3] = d4.w;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = eltwise_op(v[e], d[e], mode, p_drop, keep, seed, i0 + e);
        if constexpr (sizeof(TO) == 4) {
            *reinterpret_cast<float4*>(out + i0) = make_float4(r[0], r[1], r[2], r[3]);
        } else {
            typedef __attribute__((ext_vector_type(4))) TO to4;
            to4 o = {static_cast<TO>(r[0]), static_cast<TO>(r[1]), static_cast<TO>(r[2]), static_cast<TO>(r[3])};
            *reinterpret_cast<to4*>(out + i0) = o;
        }
        return;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int64_t i = i0 + e;
        if (i >= n) break;
        out[i] = static_cast<TO>(eltwise_op(static_cast<float>(z[i]), use_dy ? dy[i] : 0.f, mode, p_drop, keep, seed, i));
    }
}

// column sums: out[c] += sum_r x[r][c] (fp32 x, atomics: zero `out` first)
__global__ __launch_bounds__(256) void colsum_kernel(const float* x, int64_t ld, float* out, int64_t rows, int cols, int64_t rows_per_block) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;          // four independent loads in flight per thread
    int64_t r = r0;
    for (; r + 3 < r1; r += 4) {
        s0 += x[r * ld + c]; s1 += x[(r + 1) * ld + c]; s2 += x[(r + 2) * ld + c]; s3 += x[(r + 3) * ld + c];
    }
    for (; r < r1; ++r) s0 += x[r * ld + c];
    atomicAdd(out + c, (s0 + s1) + (s2 + s3));
}

// embedding backward: dword[ids[r]][c] += dy[r][c], dpos[r % L][c] += dy[r][c]  (fp32, atomics: zero first)
__global__ __launch_bounds__(256) void embed_bwd_kernel(const int64_t* ids, const float* dy, float* dword, float* dpos, int64_t rows, int L, int cols) {
    const int64_t r = blockIdx.x;
    if (r >= rows) return;
    const int64_t id = ids[r];
    for (int c = threadIdx.x; c < cols; c += 256) {
        const float g = dy[r * cols + c];
        atomicAdd(dword + id * cols + c, g);
        atomicAdd(dpos + (r % L) * cols + c, g);
    }
}

}  // namespace cir

using namespace cir;

extern "C" int cir_softmax_dropout(const float* S, int64_t ld_s, const float* mask, int64_t rows_per_mask, int64_t ld_mask, void* P, void* Pd,
                                   int64_t ld_p, int64_t rows, int cols, float scale, float p_drop, uint64_t seed, int dtype, void* stream) {
    CIR_CHECK_PTR(S); CIR_CHECK_PTR(P); CIR_CHECK_PTR(Pd);
    if (rows <= 0 || cols <= 0 || p_drop < 0.f || p_drop >= 1.f || (mask && rows_per_mask <= 0)) return CIR_EINVAL;
    if (dtype != CIR_BF16 && dtype != CIR_F16) return CIR_EDTYPE;
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype16(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((softmax_fwd_kernel<T>), grid, block, 0, s, S, ld_s, mask, rows_per_mask, ld_mask, reinterpret_cast<T*>(P),
                           reinterpret_cast<T*>(Pd), ld_p, rows, cols, scale, p_drop, seed);
    });
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_softmax_dropout_bwd(const void* P, int64_t ld_p, const float* dPd, int64_t ld_d, void* dS, int64_t ld_ds, int64_t rows, int cols,
                                       float scale, float p_drop, uint64_t seed, int dtype, void* stream) {
    CIR_CHECK_PTR(P); CIR_CHECK_PTR(dPd); CIR_CHECK_PTR(dS);
    if (rows <= 0 || cols <= 0 || p_drop < 0.f || p_drop >= 1.f) return CIR_EINVAL;
    if (dtype != CIR_BF16 && dtype != CIR_F16) return CIR_EDTYPE;
    dim3 grid((unsigned)((rows + 3) / 4)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype16(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((softmax_bwd_kernel<T>), grid, block, 0, s, reinterpret_cast<const T*>(P), ld_p, dPd, ld_d, reinterpret_cast<T*>(dS),
                           ld_ds, rows, cols, scale, p_drop, seed);
    });
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_layernorm_bwd(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, int64_t rows, int cols,
                                 float eps, void* stream) {
    CIR_CHECK_PTR(x); CIR_CHECK_PTR(gamma); CIR_CHECK_PTR(dy); CIR_CHECK_PTR(dx); CIR_CHECK_PTR(dgamma); CIR_CHECK_PTR(dbeta);
    if (rows <= 0 || cols <= 0) return CIR_EINVAL;
    if (cols > 64 * kLnCols) return CIR_ESHAPE;
    dim3 grid((unsigned)((rows + 31) / 32)), block(256);
    hipLaunchKernelGGL(layernorm_bwd_kernel<false>, grid, block, 0, reinterpret_cast<hipStream_t>(stream), x, gamma, dy, dx, dgamma, dbeta, rows, cols, eps,
                       (float*)nullptr);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_layernorm_bwd_ordered(const float* x, const float* gamma, const float* dy, float* dx, float* dgamma, float* dbeta, int64_t rows,
                                         int cols, float eps, float* partials, int64_t partial_elems, void* stream) {
    CIR_CHECK_PTR(x); CIR_CHECK_PTR(gamma); CIR_CHECK_PTR(dy); CIR_CHECK_PTR(dx); CIR_CHECK_PTR(dgamma); CIR_CHECK_PTR(dbeta); CIR_CHECK_PTR(partials);
    if (rows <= 0 || cols <= 0) return CIR_EINVAL;
    const int64_t blocks = (rows + 31) / 32;
    if (cols > 64 * kLnCols || partial_elems < blocks * 2 * cols) return CIR_ESHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(layernorm_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, x, gamma, dy, dx, dgamma, dbeta, rows, cols, eps, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    OrderedDst d{};
    d.out[0] = dgamma; d.out[1] = dbeta; d.src[1] = 1; d.nout = 2;
    return colsum_ordered_launch(partials, 2 * (int64_t)cols, blocks, cols, d, s);
}

extern "C" int cir_eltwise(const void* z, int z_dtype, const float* dy, void* out, int out_dtype, int64_t n, int mode, float p_drop, uint64_t seed,
                           void* stream) {
    CIR_CHECK_PTR(z); CIR_CHECK_PTR(out);
    if (n <= 0 || mode < 0 || mode > 6 || (mode != 6 && (p_drop < 0.f || p_drop >= 1.f))) return CIR_EINVAL;
    if ((mode == 1 || mode == 3 || mode == 5) && dy == nullptr) return CIR_EINVAL;
    if ((n + 1023) / 1024 > 0x7fffffffLL) return CIR_ESHAPE;
    dim3 grid((unsigned)((n + 1023) / 1024)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int vec = (reinterpret_cast<uintptr_t>(z) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0 && reinterpret_cast<uintptr_t>(dy) % 16 == 0) ? 1 : 0;
    auto known = [](int dt) { return dt == CIR_F32 || dt == CIR_BF16 || dt == CIR_F16; };
    if (!known(z_dtype) || !known(out_dtype)) return CIR_EDTYPE;
    by_dtype3(z_dtype, [&](auto tz) { by_dtype3(out_dtype, [&](auto to) {
        using TZ = typename decltype(tz)::type;
        using TO = typename decltype(to)::type;
        hipLaunchKernelGGL((eltwise_kernel<TZ, TO>), grid, block, 0, s, reinterpret_cast<const TZ*>(z), dy, reinterpret_cast<TO*>(out), n, mode, p_drop, seed, vec);
    }); });
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_colsum(const float* x, int64_t ld, float* out, int64_t rows, int cols, void* stream) {
    CIR_CHECK_PTR(x); CIR_CHECK_PTR(out);
    if (rows <= 0 || cols <= 0) return CIR_EINVAL;
    const int64_t rpb = 32;
    if ((rows + rpb - 1) / rpb > 65535) return CIR_ESHAPE;   // grid.y: 65535 * 32 rows per call
    dim3 grid((cols + 255) / 256, (unsigned)((rows + rpb - 1) / rpb)), block(256);
    hipLaunchKernelGGL(colsum_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), x, ld, out, rows, cols, rpb);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_embed_bwd(const int64_t* ids, const float* dy, float* dword, float* dpos, int64_t rows, int L, int cols, void* stream) {
    CIR_CHECK_PTR(ids); CIR_CHECK_PTR(dy); CIR_CHECK_PTR(dword); CIR_CHECK_PTR(dpos);
    if (rows <= 0 || L <= 0 || cols <= 0) return CIR_EINVAL;
    if (rows > 0x7fffffffLL) return CIR_ESHAPE;   // one workgroup per row
    hipLaunchKernelGGL(embed_bwd_kernel, dim3((unsigned)rows), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), ids, dy, dword, dpos, rows, L, cols);
    CIR_LAUNCH_RESULT();
}
