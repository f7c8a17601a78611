// Attention maps of the TRAINING pass's fused attention (nlvr_encoder.py:199-203: `attention_probs` after the softmax and BEFORE the
// dropout, saved by save_attention_map, and the gradient its register_hook receives): what train_attn.hip keeps in registers, written out.
//   probs  P  = exp2(S * scale*log2e + mask*log2e - LSE2)      the forward's log2-domain lse; no online softmax, no dropout
//   dprobs dP = dmul * dO V^T                                  the adjoint of the context product w.r.t. the probabilities
//   cam       = mean_h P * max(dmul * dO V^T, 0)               Grad-CAM over the heads, no (.., H, Lq, Lk) tensor in memory
// Built from attn_tile.hpp as tattn_bwd_dq_kernel is: one wave = 32 query rows, the keys streamed in 32-row tiles, both products
// TRANSPOSED (S^T = K Q^T, G^T = V dO^T: the dQ kernel's first two), so a lane owns ONE query row and, per tile, the 4 x 4 consecutive
// keys acc_row names: four 16-byte fp32 stores per output and tile.  No third product: no LDS, no barrier.  A group whose every key lies
// under a saturated mask is recognised by its lse (kSatLse) and gets P = exp2(-log2 Lk), as in the dQ kernel.
// Outputs are fp32 with row pitch ldk (ldk % 4 == 0, ldk >= Lk): columns [Lk, ldk) of every row are written with 0, rows past Lq are
// never stored, nothing else is touched.  All stores are plain vector stores; cam mode uses no atomics (the heads are a loop of the
// wave that owns the tile: the sum has ONE order, the result repeats bit for bit).
#include <type_traits>

#include "attn_tile.hpp"

namespace cir {

struct MapArgs {
    const void* q; int64_t q_sg, q_sh, q_sr;
    const void* k; int64_t k_sg, k_sh, k_sr;
    const void* v; int64_t v_sg, v_sh, v_sr;
    const void* d_o; int64_t o_sg, o_sh, o_sr;
    const float* mask;                                            // additive key mask (G, Lk) contiguous, or null
    const float* lse;                                             // (G, H, Lq) log2-domain log-sum-exp of the forward
    float* probs; float* dprobs;                                  // maps mode: (G, H, Lq, ldk); dprobs null = probabilities only
    float* cam;                                                   // cam mode: (G, Lq, ldk)
    int64_t ldk;
    int G, H, Lq, Lk, nqt, nkt;
    float scale, dmul;
};

enum { kMapProbs = 0, kMapGrads = 1, kMapCam = 2 };

// -lse of a row as the exponent's addend, the score scale and the mask weight (the dQ kernel's prologue): a saturated group gets
// scale 0, mask weight 0 and -log2 Lk; a query row past Lq gets -inf (p = 0; it is not stored either)
struct RowStat { float nlse, sl, l2e; };
template <bool MASKED>
__device__ __forceinline__ RowStat row_stat(float lse_r, bool qvalid, float scale, int Lk) {
    const bool gsat = MASKED && lse_r == kSatLse;
    RowStat s;
    s.nlse = qvalid ? (gsat ? -log2f((float)Lk) : -lse_r) : -INFINITY;
    s.sl = gsat ? 0.f : scale * kLog2e;
    s.l2e = gsat ? 0.f : kLog2e;
    return s;
}
// probability of accumulator element i of the tile at key0 (0 for a key past Lk)
template <bool MASKED>
__device__ __forceinline__ float map_prob(float s, const RowStat& st, const float* mp, int key, int Lk) {
    float c = st.nlse;
    if constexpr (MASKED) c = fmaf(fmaxf(mp[min(key, Lk - 1)], kMaskClamp), st.l2e, st.nlse);
    c = key < Lk ? c : -INFINITY;
    return __builtin_amdgcn_exp2f(fmaf(s, st.sl, c));
}
// the four key groups of a lane's row in the tile at key0: columns key0 + 8 j + 4 hh + (0..3), stored where they lie below ldk
__device__ __forceinline__ void store_tile_row(float* rowp, const float (&x)[16], int key0, int hh, int64_t ldk) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int col = key0 + 8 * j + 4 * hh;
        if (col < ldk) *reinterpret_cast<float4*>(rowp + col) = make_float4(x[4 * j + 0], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]);
    }
}
// columns [32 nkt, ldk) of the row: the pad beyond the last key tile
__device__ __forceinline__ void zero_row_tail(float* rowp, int col0, int hh, int64_t ldk) {
    for (int64_t col = col0 + 4 * hh; col < ldk; col += 8) *reinterpret_cast<float4*>(rowp + col) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// ------------------------------------------------------------------------------------------------------------------ maps: (group, head, query tile)
template <typename T, bool MASKED, int MODE>
__global__ __launch_bounds__(256) void attn_maps_kernel(const MapArgs a) {
    using X8 = typename Elem<T>::x8;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, hh = lane >> 5;
    if constexpr (MODE != kMapCam) {
        int qt;
        int64_t gh;
        if (!wave_unit(wave, (int64_t)a.G * a.H * a.nqt, a.nqt, qt, gh)) return;
        const int h = (int)(gh % a.H);
        const int64_t g = gh / a.H;
        const int q0 = qt * 32;
        const int qrow = min(q0 + r, a.Lq - 1);
        const bool qvalid = q0 + r < a.Lq;
        const T* kb = reinterpret_cast<const T*>(a.k) + g * a.k_sg + h * a.k_sh;
        const float* mp = MASKED ? a.mask + g * a.Lk : nullptr;
        X8 qf[4], dof[4], kf[4], vf[4];
        frag_load<T>(reinterpret_cast<const T*>(a.q) + g * a.q_sg + h * a.q_sh + (int64_t)qrow * a.q_sr + 8 * hh, qf);
        const T* vb = nullptr;
        if constexpr (MODE == kMapGrads) {
            vb = reinterpret_cast<const T*>(a.v) + g * a.v_sg + h * a.v_sh;
            frag_load<T>(reinterpret_cast<const T*>(a.d_o) + g * a.o_sg + h * a.o_sh + (int64_t)qrow * a.o_sr + 8 * hh, dof);
        }
        const RowStat st = row_stat<MASKED>(a.lse[gh * a.Lq + qrow], qvalid, a.scale, a.Lk);
        const int64_t row_off = (gh * a.Lq + qrow) * a.ldk;       // (a clamped row is never stored)
        float* prow = a.probs + row_off;
        float* grow = MODE == kMapGrads ? a.dprobs + row_off : nullptr;
        for (int kt = 0; kt < a.nkt; ++kt) {
            const int key0 = kt * 32;
            const int krow = min(key0 + r, a.Lk - 1);
            frag_load<T>(kb + (int64_t)krow * a.k_sr + 8 * hh, kf);
            if constexpr (MODE == kMapGrads) frag_load<T>(vb + (int64_t)krow * a.v_sr + 8 * hh, vf);
            f32x16 s, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
            for (int sx = 0; sx < 4; ++sx) {
                s = Elem<T>::mfma32(kf[sx], qf[sx], s);
                if constexpr (MODE == kMapGrads) dp = Elem<T>::mfma32(vf[sx], dof[sx], dp);
            }
            float p[16], gq[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = key0 + acc_row(i, hh);
                p[i] = map_prob<MASKED>(s[i], st, mp, key, a.Lk);
                gq[i] = key < a.Lk ? dp[i] * a.dmul : 0.f;
            }
            if (qvalid) {
                store_tile_row(prow, p, key0, hh, a.ldk);
                if constexpr (MODE == kMapGrads) store_tile_row(grow, gq, key0, hh, a.ldk);
            }
        }
        if (qvalid) {
            zero_row_tail(prow, a.nkt * 32, hh, a.ldk);
            if constexpr (MODE == kMapGrads) zero_row_tail(grow, a.nkt * 32, hh, a.ldk);
        }
    } else {
        // ---------------------------------------------------------------------------------------------------------- cam: (group, query tile, key tile)
        int kt;
        int64_t gq_;
        if (!wave_unit(wave, (int64_t)a.G * a.nqt * a.nkt, a.nkt, kt, gq_)) return;
        const int qt = (int)(gq_ % a.nqt);
        const int64_t g = gq_ / a.nqt;
        const int q0 = qt * 32, key0 = kt * 32;
        const int qrow = min(q0 + r, a.Lq - 1), krow = min(key0 + r, a.Lk - 1);
        const bool qvalid = q0 + r < a.Lq;
        const float* mp = MASKED ? a.mask + g * a.Lk : nullptr;
        float acc[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        for (int h = 0; h < a.H; ++h) {                              // heads in the order 0 .. H-1: one summation order
            X8 qf[4], dof[4], kf[4], vf[4];
            frag_load<T>(reinterpret_cast<const T*>(a.q) + g * a.q_sg + h * a.q_sh + (int64_t)qrow * a.q_sr + 8 * hh, qf);
            frag_load<T>(reinterpret_cast<const T*>(a.d_o) + g * a.o_sg + h * a.o_sh + (int64_t)qrow * a.o_sr + 8 * hh, dof);
            frag_load<T>(reinterpret_cast<const T*>(a.k) + g * a.k_sg + h * a.k_sh + (int64_t)krow * a.k_sr + 8 * hh, kf);
            frag_load<T>(reinterpret_cast<const T*>(a.v) + g * a.v_sg + h * a.v_sh + (int64_t)krow * a.v_sr + 8 * hh, vf);
            const RowStat st = row_stat<MASKED>(a.lse[(g * a.H + h) * a.Lq + qrow], qvalid, a.scale, a.Lk);
            f32x16 s, dp;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = 0.f; dp[i] = 0.f; }
#pragma unroll
            for (int sx = 0; sx < 4; ++sx) { s = Elem<T>::mfma32(kf[sx], qf[sx], s); dp = Elem<T>::mfma32(vf[sx], dof[sx], dp); }
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = map_prob<MASKED>(s[i], st, mp, key0 + acc_row(i, hh), a.Lk);      // 0 for a key past Lk
                acc[i] = fmaf(p, fmaxf(dp[i] * a.dmul, 0.f), acc[i]);
            }
        }
        if (qvalid) {
            const float inv_h = 1.0f / (float)a.H;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] *= inv_h;
            float* crow = a.cam + (g * a.Lq + qrow) * a.ldk;
            store_tile_row(crow, acc, key0, hh, a.ldk);
            if (kt == a.nkt - 1) zero_row_tail(crow, a.nkt * 32, hh, a.ldk);
        }
    }
}

static int maps_check(const MapArgs& a, int head_dim, int dtype) {
    if (a.G <= 0 || a.H <= 0 || a.Lq <= 0 || a.Lk <= 0) return CIR_EINVAL;
    if (head_dim != 64) return CIR_ESHAPE;
    if (a.ldk % 4 || a.ldk < a.Lk) return CIR_ESHAPE;
    if (dtype != CIR_BF16 && dtype != CIR_F16) return CIR_EDTYPE;
    const int64_t s16[] = {a.q_sg, a.q_sh, a.q_sr, a.k_sg, a.k_sh, a.k_sr, a.v_sg, a.v_sh, a.v_sr, a.o_sg, a.o_sh, a.o_sr};
    for (int64_t s : s16)
        if (s % 8) return CIR_EALIGN;
    if (!cir_aligned16(a.q) || !cir_aligned16(a.k) || !cir_aligned16(a.v) || !cir_aligned16(a.d_o) || !cir_aligned16(a.probs) ||
        !cir_aligned16(a.dprobs) || !cir_aligned16(a.cam))
        return CIR_EALIGN;
    if ((int64_t)a.G * a.H * a.nqt > 0x7fffffffLL || (int64_t)a.G * a.nqt * a.nkt > 0x7fffffffLL) return CIR_ESHAPE;
    return CIR_OK;
}

static void maps_fill(MapArgs& a, const void* q, int64_t q_sg, int64_t q_sh, int64_t q_sr, const void* k, int64_t k_sg, int64_t k_sh, int64_t k_sr,
                      const void* v, int64_t v_sg, int64_t v_sh, int64_t v_sr, const float* mask, const void* d_o, int64_t o_sg, int64_t o_sh,
                      int64_t o_sr, const float* lse, int64_t ldk, int G, int H, int Lq, int Lk, float scale, float dmul) {
    a.q = q; a.q_sg = q_sg; a.q_sh = q_sh; a.q_sr = q_sr;
    a.k = k; a.k_sg = k_sg; a.k_sh = k_sh; a.k_sr = k_sr;
    a.v = v; a.v_sg = v_sg; a.v_sh = v_sh; a.v_sr = v_sr;
    a.d_o = d_o; a.o_sg = o_sg; a.o_sh = o_sh; a.o_sr = o_sr;
    a.mask = mask; a.lse = lse; a.ldk = ldk;
    a.G = G; a.H = H; a.Lq = Lq; a.Lk = Lk; a.nqt = (Lq + 31) / 32; a.nkt = (Lk + 31) / 32;
    a.scale = scale; a.dmul = dmul;
}

}  // namespace cir

extern "C" int cir_attention_maps(const void* q, int64_t q_sg, int64_t q_sh, int64_t q_sr, const void* k, int64_t k_sg, int64_t k_sh, int64_t k_sr,
                                  const void* v, int64_t v_sg, int64_t v_sh, int64_t v_sr, const float* mask, const void* d_o, int64_t o_sg,
                                  int64_t o_sh, int64_t o_sr, const float* lse, float* probs, float* dprobs, int64_t ldk, int G, int H, int Lq,
                                  int Lk, int head_dim, float scale, float dmul, int dtype, void* stream) {
    using namespace cir;
    CIR_CHECK_PTR(q); CIR_CHECK_PTR(k); CIR_CHECK_PTR(lse); CIR_CHECK_PTR(probs);
    const bool grads = dprobs != nullptr;
    if ((v != nullptr) != grads || (d_o != nullptr) != grads) return CIR_ESHAPE;       // v, d_o, dprobs: all or none
    MapArgs a = {};
    maps_fill(a, q, q_sg, q_sh, q_sr, k, k_sg, k_sh, k_sr, v, v_sg, v_sh, v_sr, mask, d_o, o_sg, o_sh, o_sr, lse, ldk, G, H, Lq, Lk, scale, dmul);
    a.probs = probs; a.dprobs = dprobs;
    if (const int e = maps_check(a, head_dim, dtype)) return e;
    dim3 grid((unsigned)(((int64_t)G * H * a.nqt + 3) / 4)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype_mask(dtype, mask != nullptr, [&](auto t, auto mk) { by_bool(grads, [&](auto gr) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((attn_maps_kernel<T, decltype(mk)::value, decltype(gr)::value ? kMapGrads : kMapProbs>), grid, block, 0, s, a);
    }); });
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_attention_gradcam(const void* q, int64_t q_sg, int64_t q_sh, int64_t q_sr, const void* k, int64_t k_sg, int64_t k_sh,
                                     int64_t k_sr, const void* v, int64_t v_sg, int64_t v_sh, int64_t v_sr, const float* mask, const void* d_o,
                                     int64_t o_sg, int64_t o_sh, int64_t o_sr, const float* lse, float* cam, int64_t ldk, int G, int H, int Lq,
                                     int Lk, int head_dim, float scale, float dmul, int dtype, void* stream) {
    using namespace cir;
    CIR_CHECK_PTR(q); CIR_CHECK_PTR(k); CIR_CHECK_PTR(v); CIR_CHECK_PTR(d_o); CIR_CHECK_PTR(lse); CIR_CHECK_PTR(cam);
    MapArgs a = {};
    maps_fill(a, q, q_sg, q_sh, q_sr, k, k_sg, k_sh, k_sr, v, v_sg, v_sh, v_sr, mask, d_o, o_sg, o_sh, o_sr, lse, ldk, G, H, Lq, Lk, scale, dmul);
    a.cam = cam;
    if (const int e = maps_check(a, head_dim, dtype)) return e;
    dim3 grid((unsigned)(((int64_t)G * a.nqt * a.nkt + 3) / 4)), block(256);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    by_dtype_mask(dtype, mask != nullptr, [&](auto t, auto mk) {
        hipLaunchKernelGGL((attn_maps_kernel<typename decltype(t)::type, decltype(mk)::value, kMapCam>), grid, block, 0, s, a);
    });
    CIR_LAUNCH_RESULT();
}
