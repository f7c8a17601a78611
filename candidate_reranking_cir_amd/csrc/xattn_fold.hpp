// Shared pieces of the folded cross-attention kernels (xattn_fold.hip: N <= 224 keys, 48 query rows per wave; xattn_fold_units.hip: N <= 608
// keys or L <= 64 tokens, 16-row blocks).
#pragma once
#include "common.hpp"
#include "gemm_args.hpp"

namespace cir {

struct FoldArgs {
    const void* q; int64_t q_sb, q_rs;          // element (branch b, row t L + tok, col) at q + b q_sb + row q_rs + col
    const void* x; int64_t x_s1;                // tokens (T, N, 768), rows contiguous
    const void* wkt; const void* wvp; int64_t w_sb;   // W_k^T (2, 768 f, 768 (h, d)); W_v (2, 768 (h, d), 768 f permuted)
    const float* bv;                            // (2, 768)
    void* out; int64_t o_st, o_sr, o_sb;        // element (t, tok, b, col) at out + t o_st + tok o_sr + b o_sb + col
    int T, L, N;
    float scale;
    const float* mask = nullptr; int64_t m_st = 0;   // optional additive key mask (T, N) fp32, rows m_st apart (round 6): logits = S scale + mask
};

typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr_f;
constexpr int kFoldD = 768, kFoldChunks = 12, kFoldKB = 14;      // width, 64-feature chunks, 16-key blocks (224 keys)
constexpr int kFoldBuf = 2560 * 16;                              // one X-chunk buffer: 2560 16-byte slots (phase 2: 224 rows x 10 slots + slack)
constexpr int kStride2 = 160;                                    // phase 2's LDS row stride: conflict-free transposing reads
constexpr int kStrideQ = 1568;                                   // q rows in LDS (1536 B + 32: the 16-lane groups of ds_read_b128 hit 64 distinct banks)

// LDS-DMA piece through a buffer descriptor (buffer_load_dwordx4 ... lds): wave-uniform resource + uniform byte offset + the lane's 32-bit
// byte offset.  A load hipcc COUNTS - its vmcnt waits for the weight fragments then leave younger DMA pieces in flight (behind an asm
// piece every compiler wait degenerates to "everything", i.e. to the HBM latency of the chunk just requested)
#define FOLD_DMA(RS, VOFF, SOFF, LDS_DST) __builtin_amdgcn_raw_ptr_buffer_load_lds(RS, (lptr_t)(LDS_DST), 16, VOFF, SOFF, 0, 0)

// 16-byte weight fragment through a buffer descriptor: wave-uniform base (SGPR resource) + uniform byte offset + the lane's 32-bit byte offset
template <typename X8>
__device__ __forceinline__ X8 wload(__amdgpu_buffer_rsrc_t rs, int voff, int soff) {
    return __builtin_bit_cast(X8, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 0));
}

template <typename T>
__device__ __forceinline__ typename Elem<T>::x8 pack_acc2(const f32x4& lo, const f32x4& hi) {
    typename Elem<T>::x8 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) { r[j] = static_cast<T>(lo[j]); r[4 + j] = static_cast<T>(hi[j]); }
    return r;
}


// The checks common to the folded entry points, in the order that decides which code a bad call gets, then the FoldArgs fill.  The caller
// names its limits (max_l tokens, max_n keys; lower ones where another entry point owns the range below) and the workgroup count its grid
// must hold in 31 bits.
inline int fold_args(FoldArgs& a, const void* q, int64_t q_sb, int64_t q_rs, const void* x, int64_t x_s1, const void* wkt, const void* wvp, int64_t w_sb,
                     const float* bv, const float* key_mask, int64_t mask_stride, void* out, int64_t o_st, int64_t o_sr, int64_t o_sb, int T, int L, int N,
                     int D, int H, float scale, int dtype, int max_l, int max_n, int64_t grid_bound, int min_l = 1, int min_n = 1) {
    CIR_CHECK_PTR(q); CIR_CHECK_PTR(x); CIR_CHECK_PTR(wkt); CIR_CHECK_PTR(wvp); CIR_CHECK_PTR(bv); CIR_CHECK_PTR(out);
    if (T <= 0 || L <= 0 || N <= 0) return CIR_EINVAL;
    if (D != kFoldD || H != 12 || L > max_l || N > max_n || L < min_l || N < min_n) return CIR_ESHAPE;
    if (dtype != CIR_BF16 && dtype != CIR_F16) return CIR_EDTYPE;
    if (!cir_aligned16(q) || !cir_aligned16(x) || !cir_aligned16(wkt) || !cir_aligned16(wvp) || !cir_aligned16(bv) || (reinterpret_cast<uintptr_t>(out) & 7) ||
        q_sb % 8 || q_rs % 8 || x_s1 % 8 || w_sb % 8 || o_st % 4 || o_sr % 4 || o_sb % 4)
        return CIR_EALIGN;
    if (grid_bound > 0x7fffffff) return CIR_ESHAPE;
    if (key_mask && mask_stride < N) return CIR_ESHAPE;
    a.q = q; a.q_sb = q_sb; a.q_rs = q_rs; a.x = x; a.x_s1 = x_s1; a.wkt = wkt; a.wvp = wvp; a.w_sb = w_sb; a.bv = bv;
    a.out = out; a.o_st = o_st; a.o_sr = o_sr; a.o_sb = o_sb; a.T = T; a.L = L; a.N = N; a.scale = scale;
    a.mask = key_mask; a.m_st = mask_stride;
    return CIR_OK;
}

// Every folded kernel takes its FoldArgs by value and its X buffers and q stage as dynamic LDS above the 64-KiB default: raise the limit, launch
using FoldKernel = void (*)(const FoldArgs);
inline int fold_launch(FoldKernel kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, const FoldArgs& a) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, grid, block, lds, s, a);
    CIR_LAUNCH_RESULT();
}

// N <= 608 keys (the reference's 384-px geometry: 577 tokens): one 16-row block per wave, three workgroups per (candidate, branch)
// (xattn_fold_units.hip)
int launch_fold16(const FoldArgs& a, int dtype, hipStream_t s);

}  // namespace cir
