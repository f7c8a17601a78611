// Training pass (blip_stage2.py:65-99 driven by stage2_train.py:202-216): 16-bit transposes, and a batched matmul on
// the matrix cores for products of any extents and storage orders (weight gradients dy^T x read as stored; the un-fused attention and its
// four adjoints per (candidate or triplet, head)).  None of it is on the inference path.

#include "common.hpp"

namespace cir {

template <typename T> __device__ __forceinline__ float ldf(const T* p) { return static_cast<float>(*p); }

// ---- transpose: dst[b][c][r] = src[b][r][c] (16-bit elements; 32 x 32 tiles through LDS) --------------------------------
template <typename T>
__global__ __launch_bounds__(256) void transpose_kernel(const T* src, T* dst, int rows, int cols, int64_t ld_src, int64_t ld_dst,
                                                        int64_t s_src, int64_t s_dst) {
    __shared__ T tile[32][33];
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 8 rows per pass
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? src[b * s_src + (int64_t)r * ld_src + c] : static_cast<T>(0.f);
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) dst[b * s_dst + (int64_t)c * ld_dst + r] = tile[tx][i];
    }
}

// ---- many transposes in one launch: matrix i (rows_i x cols_i, contiguous) at element offset off_i of src -> its transpose at the SAME
// offset of dst.  table = 4 int64 per matrix: {offset, rows, cols, first 32 x 32 tile}; a block finds its matrix by binary search.
// (The trainer's dgrad operands: every trained weight of the flat 16-bit parameter buffer, once per step.)
template <typename T>
__global__ __launch_bounds__(256) void transpose_multi_kernel(const T* src, T* dst, const int64_t* table, int count) {
    __shared__ T tile[32][33];
    int lo = 0, hi = count - 1;
    const int64_t bid = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[4 * mid + 3] <= bid) lo = mid; else hi = mid - 1;
    }
    const int64_t off = table[4 * lo], t = bid - table[4 * lo + 3];
    const int rows = (int)table[4 * lo + 1], cols = (int)table[4 * lo + 2];
    const int tiles_c = (cols + 31) / 32;
    const int r0 = (int)(t / tiles_c) * 32, c0 = (int)(t % tiles_c) * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < rows && c < cols) ? src[off + (int64_t)r * cols + c] : static_cast<T>(0.f);
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < cols && r < rows) dst[off + (int64_t)c * rows + r] = tile[tx][i];
    }
}

// ---- small batched matmul: C[b] = alpha * op(A[b]) * op(B[b]) (+ C[b]) ----------------------------------------------------
// op(A) is (M, K): A stored (M, K) [ta = 0] or (K, M) [ta = 1]; op(B) is (K, N): B stored (K, N) [tb = 0] or (N, K) [tb = 1].
// 16 x 16 output tile per 256-thread block, fp32 accumulate; inputs TI (16-bit or float), output TO.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void bmm_kernel(const TI* A, const TI* B, TO* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc,
                                                  int ta, int tb, int nb2, int64_t sA1, int64_t sA2, int64_t sB1, int64_t sB2, int64_t sC1, int64_t sC2,
                                                  float alpha, int accumulate) {
    __shared__ float As[16][17], Bs[16][17];
    const int z1 = blockIdx.z / nb2, z2 = blockIdx.z % nb2;
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int m = blockIdx.y * 16 + ty, n = blockIdx.x * 16 + tx;
    const TI* Ab = A + z1 * sA1 + z2 * sA2;
    const TI* Bb = B + z1 * sB1 + z2 * sB2;
    float acc = 0.f;
    for (int k0 = 0; k0 < K; k0 += 16) {
        {   // A tile: element (ty = m-local, tx = k-local)
            const int kk = k0 + tx;
            As[ty][tx] = (m < M && kk < K) ? ldf(ta ? Ab + (int64_t)kk * lda + m : Ab + (int64_t)m * lda + kk) : 0.f;
        }
        {   // B tile: element (ty = k-local, tx = n-local)
            const int kk = k0 + ty;
            Bs[ty][tx] = (kk < K && n < N) ? ldf(tb ? Bb + (int64_t)n * ldb + kk : Bb + (int64_t)kk * ldb + n) : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) acc = fmaf(As[ty][k], Bs[k][tx], acc);
        __syncthreads();
    }
    if (m < M && n < N) {
        TO* cp = C + z1 * sC1 + z2 * sC2 + (int64_t)m * ldc + n;
        const float v = alpha * acc + (accumulate ? static_cast<float>(*cp) : 0.f);
        *cp = static_cast<TO>(v);
    }
}

// ---- the same product on the matrix cores (16-bit operands) ------------------------------------------------------------------
// 64 x 64 output tile per 256-thread block (4 waves, 32 x 32 each = 2 x 2 MFMA 16x16x32 tiles), K in steps of 32 through LDS.
// Every extent is arbitrary (edges are zero-filled / predicated) and each operand may be stored either way, so the adjoints
// need no transposed copies: wgrad reads dy (rows, N) and x (rows, K) as they are (ta = 1), attention reads head slices of the
// (rows, D) projections in place.  Two batch levels (z = z1 * nb2 + z2, a stride per level and operand): (candidate, head) or
// (triplet, head) in one launch; split-K of a weight gradient is a batch over row chunks into partial sums.
// 16-byte global loads when the host says the operand allows them (leading dimension and strides multiples of 8 elements,
// base 16-byte aligned; a row then also has room for the 8-element read past a ragged edge), 2-byte loads otherwise.
struct BmmArgs {
    const void* A; const void* B; void* C;
    int M, N, K;
    int64_t lda, ldb, ldc;
    int ta, tb, nb2;
    int64_t sA1, sA2, sB1, sB2, sC1, sC2;
    float alpha;
    int accumulate, vecA, vecB;
};

constexpr int kBmmLd = 40;      // LDS row: 32 k-elements + 8 pad (80 bytes: 16-byte aligned fragments, rows spread over the banks)

// 64 rows of an operand tile (rows r0 .. r0+63 of the M or N extent x 32 of K) from global memory into 8 registers per thread
// kmajor = 0: stored (R, K), K contiguous: thread -> (row = tid / 4, 8 consecutive k)
// kmajor = 1: stored (K, R), R contiguous: thread -> (k = tid / 8, 8 consecutive rows)
template <typename T>
__device__ __forceinline__ typename Elem<T>::x8 bmm_fetch(const T* base, int64_t ld, int kmajor, int R, int K, int r0, int k0, int vec, int tid) {
    typedef typename Elem<T>::x8 X8;
    X8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = static_cast<T>(0.f);
    if (!kmajor) {
        const int r = r0 + (tid >> 2), k = k0 + (tid & 3) * 8;
        if (r < R && k < K) {
            const T* p = base + (int64_t)r * ld + k;
            if (vec) {
                v = *reinterpret_cast<const X8*>(p);
#pragma unroll
                for (int i = 0; i < 8; ++i) if (k + i >= K) v[i] = static_cast<T>(0.f);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) if (k + i < K) v[i] = p[i];
            }
        }
    } else {
        const int k = k0 + (tid >> 3), r = r0 + (tid & 7) * 8;
        if (k < K && r < R) {
            const T* p = base + (int64_t)k * ld + r;
            if (vec) {
                v = *reinterpret_cast<const X8*>(p);
#pragma unroll
                for (int i = 0; i < 8; ++i) if (r + i >= R) v[i] = static_cast<T>(0.f);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) if (r + i < R) v[i] = p[i];
            }
        }
    }
    return v;
}

// LDS images of one operand tile (BT rows of the M / N extent x 32 of K):
//   stored (R, K) [kmajor 0]: [BT][40] - a row's 32 k-elements + 8 pad; the MFMA fragment (row r15, k = 8g .. 8g+7) is one ds_read_b128
//   stored (K, R) [kmajor 1]: [32][BT + 16] - as it comes from memory (16-byte writes, no scatter); the fragment is two
//     ds_read_b64_tr_b16 (hardware transpose: a 16-lane group reads 4 k-rows x 16 r-columns and lane i receives column i)
typedef __attribute__((address_space(3))) s16x4* bmm_lds_s16x4_ptr;

template <typename T, int BT>
__device__ __forceinline__ void bmm_stash(char* tile, typename Elem<T>::x8 v, int kmajor, int tid, int h) {
    typedef typename Elem<T>::x8 X8;
    if (!kmajor) *reinterpret_cast<X8*>(tile + (((tid >> 2) + h * 64) * kBmmLd + (tid & 3) * 8) * 2) = v;
    else *reinterpret_cast<X8*>(tile + ((tid >> 3) * (BT + 16) + (tid & 7) * 8 + h * 64) * 2) = v;
}

template <typename T, int BT>
__device__ __forceinline__ typename Elem<T>::x8 bmm_frag(const char* tile, int kmajor, int row0, int lane) {
    typedef typename Elem<T>::x8 X8;
    const int r15 = lane & 15, g = lane >> 4;
    if (!kmajor) return *reinterpret_cast<const X8*>(tile + ((row0 + r15) * kBmmLd + g * 8) * 2);
    const int q = r15 >> 2, p = r15 & 3;
    const char* base = tile + ((8 * g + q) * (BT + 16) + row0 + 4 * p) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bmm_lds_s16x4_ptr)(base));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bmm_lds_s16x4_ptr)(base + 4 * (BT + 16) * 2));
    s16x8 both;
    both.s0 = lo.x; both.s1 = lo.y; both.s2 = lo.z; both.s3 = lo.w;
    both.s4 = hi.x; both.s5 = hi.y; both.s6 = hi.z; both.s7 = hi.w;
    return __builtin_bit_cast(X8, both);
}

// F = MFMA tiles per wave and dimension: F = 2 -> 64 x 64 block tile (small products: one head of self-attention is 32 x 32),
// F = 4 -> 128 x 128 (16 MFMAs per wave between two barriers: the weight gradients and the stacked cross-attention products)
// KS = 32-wide K slabs per step (each its own LDS image).  KS = 2 (twice the bytes in flight per block, half the barriers) costs a
// third of the occupancy (141 VGPRs, 80 KB LDS) and measured 1.8x SLOWER on the weight gradients: both instantiations use KS = 1.
template <typename T, typename TO, int F, int KS>
__global__ __launch_bounds__(256, 3) void bmm_mfma_kernel(BmmArgs a) {      // three blocks per CU: 168 registers per lane
    typedef typename Elem<T>::x8 X8;
    constexpr int BT = 32 * F, H = F / 2;                   // block tile extent; 64-row fetch slabs per operand
    constexpr int kImg = (BT * kBmmLd > 32 * (BT + 16) ? BT * kBmmLd : 32 * (BT + 16)) * 2;
    constexpr int BK = 32 * KS;
    __shared__ __attribute__((aligned(16))) char As[2][KS][kImg]; // two image sets per operand: tile k+1 is written while tile k is read,
    __shared__ __attribute__((aligned(16))) char Bs[2][KS][kImg]; // one barrier per K step
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r15 = lane & 15, g = lane >> 4, wm = wave >> 1, wn = wave & 1;
    // XCD-aware block order: workgroups are dealt to the 8 XCDs round-robin by linear id, each XCD has its own 4 MB L2.  When the
    // batch count is a multiple of 8, all tiles of one batch item (one row chunk of a weight gradient: 1.5 MB of dy and x; one
    // (candidate, head) of the attention products) run on ONE XCD, so its operands are fetched into that L2 once instead of
    // streaming from the Infinity Cache into all eight (measured: weight gradients +8 %, the attention products +10 .. 30 %).
    // (Tried and dropped: a second register set for a two-tile-deep prefetch - hipcc then duplicates the accumulators,
    //  240 VGPRs + 128 AGPRs, one wave per SIMD, 2.5x slower.)
    int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
    if (gridDim.z % 8 == 0) {
        const int tiles = gridDim.x * gridDim.y;
        const int lin = bx + gridDim.x * (by + gridDim.y * bz);
        const int j = lin >> 3, t = j % tiles;
        bz = (lin & 7) + 8 * (j / tiles);
        bx = t % gridDim.x;
        by = t / gridDim.x;
    }
    const int z1 = bz / a.nb2, z2 = bz % a.nb2;
    const T* A = reinterpret_cast<const T*>(a.A) + z1 * a.sA1 + z2 * a.sA2;
    const T* B = reinterpret_cast<const T*>(a.B) + z1 * a.sB1 + z2 * a.sB2;
    TO* C = reinterpret_cast<TO*>(a.C) + z1 * a.sC1 + z2 * a.sC2;
    const int m0 = by * BT, n0 = bx * BT;
    const int ka = a.ta, kb = !a.tb;                        // A stored (K, M) when ta = 1; B stored (K, N) when tb = 0
    f32x4 acc[F][F];
#pragma unroll
    for (int i = 0; i < F; ++i)
#pragma unroll
        for (int j = 0; j < F; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    // interior tiles: one 16-byte load per slab from a pointer computed once (the generic fetch re-derives a 64-bit address and
    // masks eight elements per load - more VALU issue per K step than the step's MFMAs take)
    const T* pa[H]; const T* pb[H];
    bool fa[H], fb[H];
#pragma unroll
    for (int h = 0; h < H; ++h) {
        pa[h] = ka ? A + (int64_t)(tid >> 3) * a.lda + m0 + h * 64 + (tid & 7) * 8 : A + (int64_t)(m0 + h * 64 + (tid >> 2)) * a.lda + (tid & 3) * 8;
        pb[h] = kb ? B + (int64_t)(tid >> 3) * a.ldb + n0 + h * 64 + (tid & 7) * 8 : B + (int64_t)(n0 + h * 64 + (tid >> 2)) * a.ldb + (tid & 3) * 8;
        fa[h] = a.vecA && (ka ? m0 + h * 64 + (tid & 7) * 8 + 8 <= a.M : m0 + h * 64 + (tid >> 2) < a.M);
        fb[h] = a.vecB && (kb ? n0 + h * 64 + (tid & 7) * 8 + 8 <= a.N : n0 + h * 64 + (tid >> 2) < a.N);
    }
    const int64_t stepA = ka ? a.lda : 1, stepB = kb ? a.ldb : 1;       // elements per unit of k
    auto fetch_a = [&](int h, int k) -> X8 {
        if (fa[h] && k + 32 <= a.K) return *reinterpret_cast<const X8*>(pa[h] + k * stepA);
        return bmm_fetch<T>(A, a.lda, ka, a.M, a.K, m0 + h * 64, k, a.vecA, tid);
    };
    auto fetch_b = [&](int h, int k) -> X8 {
        if (fb[h] && k + 32 <= a.K) return *reinterpret_cast<const X8*>(pb[h] + k * stepB);
        return bmm_fetch<T>(B, a.ldb, kb, a.N, a.K, n0 + h * 64, k, a.vecB, tid);
    };
    X8 ra[KS][H], rb[KS][H];
#pragma unroll
    for (int sl = 0; sl < KS; ++sl)
#pragma unroll
        for (int h = 0; h < H; ++h) {
            ra[sl][h] = fetch_a(h, sl * 32);
            rb[sl][h] = fetch_b(h, sl * 32);
        }
#pragma unroll
    for (int sl = 0; sl < KS; ++sl)
#pragma unroll
        for (int h = 0; h < H; ++h) {
            bmm_stash<T, BT>(As[0][sl], ra[sl][h], ka, tid, h);
            bmm_stash<T, BT>(Bs[0][sl], rb[sl][h], kb, tid, h);
        }
    if (BK < a.K) {
#pragma unroll
        for (int sl = 0; sl < KS; ++sl)
#pragma unroll
            for (int h = 0; h < H; ++h) {
                ra[sl][h] = fetch_a(h, BK + sl * 32);
                rb[sl][h] = fetch_b(h, BK + sl * 32);
            }
    }
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < a.K; k0 += BK, buf ^= 1) {
#pragma unroll
        for (int sl = 0; sl < KS; ++sl) {
            X8 af[F], bf[F];
#pragma unroll
            for (int i = 0; i < F; ++i) {
                af[i] = bmm_frag<T, BT>(As[buf][sl], ka, wm * 16 * F + i * 16, lane);
                bf[i] = bmm_frag<T, BT>(Bs[buf][sl], kb, wn * 16 * F + i * 16, lane);
            }
            if (sl == 0 && k0 + BK < a.K) {                  // tile k+1 (in registers since the last step) into the other image set,
#pragma unroll
                for (int s2 = 0; s2 < KS; ++s2)
#pragma unroll
                    for (int h = 0; h < H; ++h) {
                        bmm_stash<T, BT>(As[buf ^ 1][s2], ra[s2][h], ka, tid, h);
                        bmm_stash<T, BT>(Bs[buf ^ 1][s2], rb[s2][h], kb, tid, h);
                    }
                if (k0 + 2 * BK < a.K) {                     // tile k+2's loads fly under this tile's MFMAs
#pragma unroll
                    for (int s2 = 0; s2 < KS; ++s2)
#pragma unroll
                        for (int h = 0; h < H; ++h) {
                            ra[s2][h] = fetch_a(h, k0 + 2 * BK + s2 * 32);
                            rb[s2][h] = fetch_b(h, k0 + 2 * BK + s2 * 32);
                        }
                }
            }
#pragma unroll
            for (int mi = 0; mi < F; ++mi)
#pragma unroll
                for (int ni = 0; ni < F; ++ni) acc[mi][ni] = Elem<T>::mfma16(af[mi], bf[ni], acc[mi][ni]);
        }
        __syncthreads();                                     // image set buf^1 complete; set buf free for the step after next
    }
    // lane (r15, g) holds C[m = 4 g + jj][n = r15] of each 16 x 16 tile
#pragma unroll
    for (int mi = 0; mi < F; ++mi)
#pragma unroll
        for (int ni = 0; ni < F; ++ni) {
            const int n = n0 + wn * 16 * F + ni * 16 + r15;
            if (n >= a.N) continue;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int m = m0 + wm * 16 * F + mi * 16 + g * 4 + jj;
                if (m >= a.M) continue;
                TO* cp = C + (int64_t)m * a.ldc + n;
                if constexpr (sizeof(TO) == 4) {
                    if (a.accumulate == 2) { atomicAdd(cp, a.alpha * acc[mi][ni][jj]); continue; }     // split-K batches summing into ONE C
                }
                const float v = a.alpha * acc[mi][ni][jj] + (a.accumulate ? static_cast<float>(*cp) : 0.f);
                *cp = static_cast<TO>(v);
            }
        }
}

}  // namespace cir

using namespace cir;

extern "C" int cir_transpose16(const void* src, void* dst, int rows, int cols, int64_t ld_src, int64_t ld_dst, int batch, int64_t s_src,
                               int64_t s_dst, int dtype, void* stream) {
    CIR_CHECK_PTR(src); CIR_CHECK_PTR(dst);
    if (rows <= 0 || cols <= 0 || batch <= 0) return CIR_EINVAL;
    if (dtype != CIR_BF16 && dtype != CIR_F16) return CIR_EDTYPE;
    dim3 grid((cols + 31) / 32, (rows + 31) / 32, batch), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    // (bf16 and fp16 are both 16-bit payloads: one instantiation moves either)
    hipLaunchKernelGGL((transpose_kernel<unsigned short>), grid, block, 0, s, reinterpret_cast<const unsigned short*>(src),
                       reinterpret_cast<unsigned short*>(dst), rows, cols, ld_src, ld_dst, s_src, s_dst);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_transpose16_multi(const void* src, void* dst, const int64_t* table, int count, int64_t total_tiles, int dtype, void* stream) {
    CIR_CHECK_PTR(src); CIR_CHECK_PTR(dst); CIR_CHECK_PTR(table);
    if (count <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffffLL) return CIR_EINVAL;
    if (dtype != CIR_BF16 && dtype != CIR_F16) return CIR_EDTYPE;
    hipLaunchKernelGGL((transpose_multi_kernel<unsigned short>), dim3((unsigned)total_tiles), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const unsigned short*>(src), reinterpret_cast<unsigned short*>(dst), table, count);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_bmm(const void* A, const void* B, void* C, int M, int N, int K, int64_t lda, int64_t ldb, int64_t ldc, int trans_a, int trans_b,
                       int nb1, int nb2, int64_t sA1, int64_t sA2, int64_t sB1, int64_t sB2, int64_t sC1, int64_t sC2, float alpha, int accumulate,
                       int in_dtype, int out_dtype, void* stream) {
    CIR_CHECK_PTR(A); CIR_CHECK_PTR(B); CIR_CHECK_PTR(C);
    if (M <= 0 || N <= 0 || K <= 0 || nb1 <= 0 || nb2 <= 0) return CIR_EINVAL;
    if ((int64_t)nb1 * nb2 > 65535) return CIR_ESHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (accumulate < 0 || accumulate > 2) return CIR_EINVAL;
    if (in_dtype == CIR_F32) {                               // fp32 operands: the plain kernel
        if (out_dtype != CIR_F32) return CIR_EDTYPE;
        if (accumulate == 2) return CIR_EDTYPE;
        dim3 grid((N + 15) / 16, (M + 15) / 16, nb1 * nb2), block(256);
        hipLaunchKernelGGL((bmm_kernel<float, float>), grid, block, 0, s, reinterpret_cast<const float*>(A), reinterpret_cast<const float*>(B),
                           reinterpret_cast<float*>(C), M, N, K, lda, ldb, ldc, trans_a, trans_b, nb2, sA1, sA2, sB1, sB2, sC1, sC2, alpha, accumulate);
        CIR_LAUNCH_RESULT();
    }
    if (in_dtype != CIR_BF16 && in_dtype != CIR_F16) return CIR_EDTYPE;
    if (out_dtype != CIR_F32 && out_dtype != in_dtype) return CIR_EDTYPE;
    if (accumulate == 2 && out_dtype != CIR_F32) return CIR_EDTYPE;
    auto vec_ok = [](const void* p, int64_t ld, int64_t s1, int64_t s2) {
        return (reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % 8 == 0 && s1 % 8 == 0 && s2 % 8 == 0) ? 1 : 0;
    };
    BmmArgs a{A, B, C, M, N, K, lda, ldb, ldc, trans_a ? 1 : 0, trans_b ? 1 : 0, nb2, sA1, sA2, sB1, sB2, sC1, sC2, alpha, accumulate,
              vec_ok(A, lda, sA1, sA2), vec_ok(B, ldb, sB1, sB2)};
    dim3 block(256);
    const bool big = M > 64 && N > 64;                       // 128 x 128 tiles unless one extent fits a 64 tile anyway
    const int bt = big ? 128 : 64;
    dim3 grid((N + bt - 1) / bt, (M + bt - 1) / bt, nb1 * nb2);
    by_dtype16(in_dtype, [&](auto t) { by_bool(out_dtype == CIR_F32, [&](auto f32_out) { by_bool(big, [&](auto b) {
        using T = typename decltype(t)::type;
        using TO = std::conditional_t<decltype(f32_out)::value, float, T>;
        hipLaunchKernelGGL((bmm_mfma_kernel<T, TO, decltype(b)::value ? 4 : 2, 1>), grid, block, 0, s, a);
    }); }); });
    CIR_LAUNCH_RESULT();
}
