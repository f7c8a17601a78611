// cir_attention with fp32 tensors - the "exact" precision mode (round 5): softmax(q k^T * scale + mask) v with fp32 operands in
// BOTH products, fp32 statistics, fp32 out; head dimension 64.  Bound: fp32 MFMA (v_mfma_f32_32x32x2_f32: 64 flop / clk / SIMD,
// 157.3 TFLOP/s peak - f32 in, f32 accumulate, a chain of IEEE fmaf's); 4 * Lq * Lk * 64 flop per (item, head).
//
// One wave per (item, head, 32 queries), nothing shared between waves, no LDS: at 1/16 of the 16-bit MFMA rate a 32-key tile
// is 64 MFMAs = 4096 matrix-pipe cycles, against 8 + 32 load instructions - the operand stream is not the problem here.
// Same formulation as the 16-bit kernels (attention.hip), with the fp32 MFMA's one-value-per-lane operands:
//   S^T[key][query] = K_tile Q^T : lane (r, hh) holds K[key0 + r][8c + 4hh + s] and Q[q0 + r][8c + 4hh + s] (16-byte loads, c < 8, s < 4);
//                                  MFMA (c, s) contracts d in {8c + s, 8c + 4 + s} - 32 MFMAs cover d < 64;
//   the score tile's register i is key  key0 + (i & 3) + 8 (i >> 2) + 4 hh  of query r: online softmax in registers + one lane^32 exchange;
//   O^T[d][query] += V_tile^T P^T : MFMA i takes P^T's register i as the B operand (accumulator-as-operand: no LDS trip for P) and
//                                  V[key(i, hh)][32 dt + r] as A - one 4-byte load per lane, 32 consecutive d per half-wave = a whole 128-byte line.
// The next tile's K fragments are requested behind the score product, its V behind the second product.
// Replaces BertSelfAttention.forward (nlvr_encoder.py:140-222, med.py:158-240) and Attention.forward's core (vit.py:73-83) when every
// tensor of the model is fp32, like the reference's (validate_stage2.py:140-141).

#include "attn_tile.hpp"

namespace cir {

// SPLIT (round 6): the context rows leave as "split8" operand rows [D x fp16 | D x e4m3 lo | D x e4m3 hi] (common.hpp) - what the
// self-attention output projection of the text32 mode reads - instead of fp32: the two half-waves exchange 4-element groups
// (v_permlane32_swap) so that a lane holds 8 consecutive features and stores 16 + 8 + 8 bytes per group.
template <bool MASKED, bool SPLIT = false>
__global__ __launch_bounds__(256, 2) void attn_f32_kernel(const AttnArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    AttnUnit u;
    if (!u.decode(a, wave)) return;

    const int r = lane & 31, hh = lane >> 5;
    const int q0 = u.qt * 32;
    const float* qp = u.q_row<float>(a, min(q0 + r, a.Lq - 1)) + 4 * hh;
    const int64_t kb1 = u.kv_item(a);
    const float* kb = u.k_base<float>(a, kb1) + 4 * hh;
    const float* vb = u.v_base<float>(a, kb1) + r;
    const float* mp = MASKED ? u.mask_base(a) : nullptr;

    f32x4 qf[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) qf[c] = *reinterpret_cast<const f32x4*>(qp + 8 * c);

    const int nkt = (a.Lk + 31) >> 5;
    auto load_k = [&](int kt, f32x4 (&kf)[8]) {
        const float* kp = kb + (int64_t)min(kt * 32 + r, a.Lk - 1) * a.k_rs;
#pragma unroll
        for (int c = 0; c < 8; ++c) kf[c] = *reinterpret_cast<const f32x4*>(kp + 8 * c);
    };
    auto load_v = [&](int kt, float (&vf)[2][16]) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = min(kt * 32 + acc_row(i, hh), a.Lk - 1);     // rows past Lk: probability 0, any finite value
            const float* vp = vb + (int64_t)key * a.v_rs;
            vf[0][i] = vp[0];
            vf[1][i] = vp[32];
        }
    };

    Softmax st;
    st.init();
    const float sl = a.scale * kLog2e;

    f32x4 kf[8];
    float vf[2][16];
    load_k(0, kf);
    load_v(0, vf);
    for (int kt = 0; kt < nkt; ++kt) {
        const int key0 = kt * 32;
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int c = 0; c < 8; ++c)
#pragma unroll
            for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[c][e], qf[c][e], s, 0, 0, 0);
        if (kt + 1 < nkt) load_k(kt + 1, kf);
        float sv[16];
        softmax_plain<MASKED>(st, s, sl, mp, key0, hh, a.Lk, sv);
        // ---- O^T += V_tile^T P^T ----
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            st.o[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[0][i], sv[i], st.o[0], 0, 0, 0);
            st.o[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[1][i], sv[i], st.o[1], 0, 0, 0);
        }
        if (kt + 1 < nkt) load_v(kt + 1, vf);
    }
    if constexpr (SPLIT)
        store_split8_rows(st.o, 1.0f / st.l_run, u.out_base<char>(a) + (int64_t)min(q0 + r, a.Lq - 1) * a.o_rs, a.H * 64, u.h * 64, hh, q0 + r < a.Lq);
    else if (q0 + r < a.Lq)
        store_f32(st.o, u.out_base<float>(a) + (int64_t)(q0 + r) * a.o_rs + u.h * 64 + 4 * hh, 1.0f / st.l_run);
}

int launch_attention_f32(const AttnArgs& a, hipStream_t s) {
    const int64_t nblk = (a.total + 3) / 4;
    if (nblk > 0x7fffffff) return CIR_ESHAPE;
    dim3 grid((unsigned)nblk), block(256);
    if (a.out_split) {
        if (a.mask) hipLaunchKernelGGL((attn_f32_kernel<true, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((attn_f32_kernel<false, true>), grid, block, 0, s, a);
    } else if (a.mask) hipLaunchKernelGGL((attn_f32_kernel<true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((attn_f32_kernel<false>), grid, block, 0, s, a);
    CIR_LAUNCH_RESULT();
}

}  // namespace cir
