// The shared pieces of the "keys on rows" 32 x 32 tile update (attention.hip has the formulation): every attention kernel of
// attention.hip, attention_f32.hip, train_attn.hip and attn_maps.hip is built from these, so the V-tile swizzle, the transposed read and the
// accumulator's element map each exist once.  Device-only; nothing here launches or owns LDS.
//
// NOT here, on purpose: the softmax steps.  Four exist and they are four different computations:
//   softmax_tile (attention.hip)       lazy rescale, scale inside the exponent's FMA when there is no mask
//   softmax_plain (below)              exp2f, rescale on every tile: attn_f32_kernel and attn_split32_kernel
//   tattn_fwd_kernel (train_attn.hip)  dropout, __builtin_amdgcn_exp2f
//   cls_xattn_kernel (attention.hip)   scores summed over four waves, scale inside the FMA
// Only the second is used twice.
#pragma once
#include "attention_args.hpp"

namespace cir {

constexpr float kLog2e = 1.4426950408889634f;
// the training kernels' mask clamp and the lse of a group whose every key sits at it (train_attn.hip has the account; attn_maps.hip shares them)
constexpr float kMaskClamp = -2.0e38f;
constexpr float kSatLse = kMaskClamp * kLog2e;                  // = fmaf(kMaskClamp, kLog2e, s) for every |s| < 1e30
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_ptr;

// accumulator index i of a 32 x 32 tile -> row inside the tile (keys, for a score tile); this lane's column is lane & 31
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// Online-softmax state of one 32-query tile: lane = (query r, key/dh half hh).
struct Softmax {
    float m_run, l_run;
    f32x16 o[2];
    __device__ __forceinline__ void init() {
        m_run = -INFINITY;
        l_run = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) { o[0][i] = 0.f; o[1][i] = 0.f; }
    }
};

// ---- transposed LDS reads --------------------------------------------------------------------------------------------------
// this lane's address inside a 4-row x 16-column transposed-read block of a row-major 16-bit tile with `row_bytes` per row:
// row (4*hh + q), byte column (16*(G&1) + 4p)*2
__device__ __forceinline__ int tr_block_offset(int lane, int row_bytes) {
    const int i16 = lane & 15, hh = lane >> 5;
    return (4 * hh + (i16 >> 2)) * row_bytes + (16 * ((lane >> 4) & 1) + 4 * (i16 & 3)) * 2;
}
// the same for the swizzled 128-byte-row tile (v_tile_offset): the 64-byte halves are swapped when the row's bit 1 is set, and
// voff[dt] is the offset for dh-tile dt (tile-invariant: computed once per wave)
__device__ __forceinline__ void tr_offsets(int lane, int (&voff)[2]) {
    const int off = tr_block_offset(lane, 128) ^ ((((lane & 15) >> 2) >> 1) << 6);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) voff[dt] = ((off & 0x7f) ^ (dt * 64)) + (off & ~0x7f);
}
// rows [0, 16) x 16 columns at `base`, transposed: one 32x32x16 A-operand fragment (two reads, 8 rows apart)
template <typename T>
__device__ __forceinline__ typename Elem<T>::x8 tr_read8(const char* base, int row_bytes) {
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(base + 8 * row_bytes));
    s16x8 both;
    both.s0 = lo.x; both.s1 = lo.y; both.s2 = lo.z; both.s3 = lo.w;
    both.s4 = hi.x; both.s5 = hi.y; both.s6 = hi.z; both.s7 = hi.w;
    return __builtin_bit_cast(typename Elem<T>::x8, both);
}
// acc^T[64 dh][32 cols] += tile^T[dh][32 rows] * frag[rows][cols]: `tile` = 32 rows x 64 dh row-major in LDS (v_tile_offset), frag = the
// packed accumulator-layout values of the 32 x 32 score-like tile.  The two row halves and the two 8-row blocks of a read pair are
// immediate offsets.
template <typename T>
__device__ __forceinline__ void tr_accumulate(f32x16 (&acc)[2], const char* tile, const int (&voff)[2], const typename Elem<T>::x8 (&frag)[2]) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) acc[dt] = Elem<T>::mfma32(tr_read8<T>(tile + voff[dt] + (16 * s2) * 128, 128), frag[s2], acc[dt]);
}

// ---- the 32-row x 64-dh LDS tile ---------------------------------------------------------------------------------------------
// byte offset of 16-byte chunk `ch` of row `row`: 128-byte rows, 64-byte halves swapped on rows with bit 1 set so that the 4-row
// transposed reads of a 32-lane half hit 64 distinct banks
__device__ __forceinline__ int v_tile_offset(int row, int ch) { return row * 128 + ((ch * 16) ^ (((row >> 1) & 1) << 6)); }

// row-major 32 x 64 tile of 16-bit rows (row r of the source at src + min(row0 + r, rows - 1) * stride) -> registers -> the wave's LDS tile:
// lane covers chunk lane & 7 of rows (lane >> 3) + 8 i
template <typename T>
__device__ __forceinline__ void tile_load(const T* src, int64_t stride, int row0, int rows, int lane, typename Elem<T>::x8 (&reg)[4]) {
    using X8 = typename Elem<T>::x8;
    const int rl = lane >> 3, ch = lane & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) reg[i] = *reinterpret_cast<const X8*>(src + (int64_t)min(row0 + rl + 8 * i, rows - 1) * stride + ch * 8);
}
template <typename T>
__device__ __forceinline__ void tile_store(char* tile, int lane, const typename Elem<T>::x8 (&reg)[4]) {
    using X8 = typename Elem<T>::x8;
    const int rl = lane >> 3, ch = lane & 7;
#pragma unroll
    for (int i = 0; i < 4; ++i) *reinterpret_cast<X8*>(tile + v_tile_offset(rl + 8 * i, ch)) = reg[i];
}
// fragments of rows (lane & 31) of a row-major matrix: d-chunks 8 hh + 16 s (A operand rows / B operand columns of mfma_f32_32x32x16)
template <typename T>
__device__ __forceinline__ void frag_load(const T* row_ptr, typename Elem<T>::x8 (&f)[4]) {
    using X8 = typename Elem<T>::x8;
#pragma unroll
    for (int s = 0; s < 4; ++s) f[s] = *reinterpret_cast<const X8*>(row_ptr + 16 * s);
}

// ---- which tile a wave owns ----------------------------------------------------------------------------------------------------
// four waves per workgroup, one unit each: unit = rest * ntiles + tile.  false: past the last unit - the WHOLE wave leaves, so EXEC
// stays all-ones for the transposed LDS reads of the waves that stay.
__device__ __forceinline__ bool wave_unit(int wave, int64_t total, int ntiles, int& tile, int64_t& rest) {
    const int64_t unit = (int64_t)blockIdx.x * 4 + wave;
    if (unit >= total) return false;
    tile = (int)(unit % ntiles);
    rest = unit / ntiles;
    return true;
}
// cir_attention's unit: (query tile, head, inner item, outer item) and the tensors' bases for it (E = element type of q / k / v)
struct AttnUnit {
    int qt, h, b0;
    int64_t b1;
    __device__ __forceinline__ bool decode(const AttnArgs& a, int wave) {
        int64_t t;
        if (!wave_unit(wave, a.total, a.nqt, qt, t)) return false;
        h = (int)(t % a.H);
        t /= a.H;
        b0 = (int)(t % a.B0);
        b1 = t / a.B0;
        return true;
    }
    template <typename E>
    __device__ __forceinline__ const E* q_row(const AttnArgs& a, int qrow) const {
        return reinterpret_cast<const E*>(a.q) + b1 * a.q_s1 + b0 * a.q_s0 + (int64_t)qrow * a.q_rs + h * 64;
    }
    // K / V of item `kb1`: b1 itself, or the bank row kv_item() names
    __device__ __forceinline__ int64_t kv_item(const AttnArgs& a) const { return a.kv_index ? a.kv_index[b1] : b1; }
    template <typename E>
    __device__ __forceinline__ const E* k_base(const AttnArgs& a, int64_t kb1) const { return reinterpret_cast<const E*>(a.k) + kb1 * a.k_s1 + b0 * a.k_s0 + h * 64; }
    template <typename E>
    __device__ __forceinline__ const E* v_base(const AttnArgs& a, int64_t kb1) const { return reinterpret_cast<const E*>(a.v) + kb1 * a.v_s1 + b0 * a.v_s0 + h * 64; }
    __device__ __forceinline__ const float* mask_base(const AttnArgs& a) const { return a.mask + b1 * a.m_s1 + b0 * a.m_s0; }
    // the output's item base in elements of E (split8 rows: E = char, strides in bytes)
    template <typename E>
    __device__ __forceinline__ E* out_base(const AttnArgs& a) const { return reinterpret_cast<E*>(a.out) + b1 * a.o_s1 + b0 * a.o_s0; }
};

// ---- the plain online-softmax step (log2 domain; lane = query r, 16 of the tile's 32 keys) --------------------------------------
// raw scores s -> probabilities sv (fp32), running max / sum, rescale of O on EVERY tile.  exp2f, not the bare instruction: this is
// the step of the fp32-statistics kernels.
template <bool MASKED>
__device__ __forceinline__ void softmax_plain(Softmax& st, const f32x16& s, float sl, const float* mp, int key0, int hh, int Lk, float (&sv)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int key = key0 + acc_row(i, hh);
        float x = s[i] * sl;
        if constexpr (MASKED) x = fmaf(fmaxf(mp[min(key, Lk - 1)], -2.0e38f), kLog2e, x);    // finfo.min-style masks stay finite
        sv[i] = key < Lk ? x : -INFINITY;
    }
    float mx = sv[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, sv[i]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(st.m_run, mx);             // finite: every tile holds at least one valid key
    const float alpha = exp2f(st.m_run - m_new);
    st.m_run = m_new;
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        sv[i] = exp2f(sv[i] - m_new);
        psum += sv[i];
    }
    psum += __shfl_xor(psum, 32, 64);
    st.l_run = st.l_run * alpha + psum;
#pragma unroll
    for (int i = 0; i < 16; ++i) { st.o[0][i] *= alpha; st.o[1][i] *= alpha; }
}

// ---- output stores of a transposed accumulator: element (row = lane & 31, dh = 32 dt + 8 qd + 4 hh + j) -----------------------------
// four consecutive features of group qd, scaled and packed to 16 bits
template <typename T>
__device__ __forceinline__ u32x2 pack4(const f32x16& acc, int qd, float mul) {
    u32x2 p;
    p.x = pack2<T>(acc[qd * 4 + 0] * mul, acc[qd * 4 + 1] * mul);
    p.y = pack2<T>(acc[qd * 4 + 2] * mul, acc[qd * 4 + 3] * mul);
    return p;
}
template <typename T, int NDT>
__device__ __forceinline__ void store_out(const f32x16 (&acc)[NDT], T* rowp /* + 4 hh */, float mul) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) *reinterpret_cast<u32x2*>(rowp + dt * 32 + 8 * qd) = pack4<T>(acc[dt], qd, mul);
}
__device__ __forceinline__ void store_f32(const f32x16 (&acc)[2], float* rowp /* + 4 hh */, float mul) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int qd = 0; qd < 4; ++qd)
            *reinterpret_cast<float4*>(rowp + dt * 32 + 8 * qd) =
                make_float4(acc[dt][qd * 4 + 0] * mul, acc[dt][qd * 4 + 1] * mul, acc[dt][qd * 4 + 2] * mul, acc[dt][qd * 4 + 3] * mul);
}
// the context as "split8" operand rows [D x fp16 | D x e4m3 lo | D x e4m3 hi] (common.hpp) at `row` (d_model = D features, this head's
// at f_head): the two half-waves exchange 4-element groups so that a lane holds 8 consecutive features and stores 16 + 8 + 8 bytes per
// group.  Every lane takes part in the exchange; `valid` guards the stores only.
__device__ __forceinline__ void store_split8_rows(const f32x16 (&acc)[2], float mul, char* row, int d_model, int f_head, int hh, bool valid) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float lo4[4], hi4[4];          // own groups qd = 2p (features 8 qd + 4 hh + j) and qd = 2p + 1
#pragma unroll
            for (int j = 0; j < 4; ++j) { lo4[j] = acc[dt][(2 * p) * 4 + j] * mul; hi4[j] = acc[dt][(2 * p + 1) * 4 + j] * mul; }
            // swap: lanes 0-31 end with (own group 2p | partner's group 2p) = 8 consecutive features at 8 (2p); lanes 32-63 with
            // (partner's group 2p+1 | own group 2p+1) = 8 consecutive features at 8 (2p+1).  As asm with both results named: hipcc folds
            // max(r.x, r.y)-style uses of the builtin's two results into one of them when both inputs are the same register.
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(lo4[j]), "+v"(hi4[j]));
            const int f0 = f_head + dt * 32 + 8 * (2 * p + hh);
            const Split4 s0 = split8_x4(lo4), s1 = split8_x4(hi4);
            if (valid) {
                *reinterpret_cast<u32x4*>(row + 2 * f0) = u32x4{s0.h01, s0.h23, s1.h01, s1.h23};
                *reinterpret_cast<u32x2*>(row + 2 * d_model + f0) = u32x2{s0.lo8, s1.lo8};
                *reinterpret_cast<u32x2*>(row + 3 * d_model + f0) = u32x2{s0.hi8, s1.hi8};
            }
        }
}

}  // namespace cir
