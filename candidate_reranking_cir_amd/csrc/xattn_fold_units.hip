// The query-side fold of xattn_fold.hip in 16-row steps: one kernel body, X staged per 32-feature UNIT, behind four entry points -
//   cir_cross_attention_folded for 225 .. 608 image tokens (the reference's 384-px geometry: 577 tokens; validate_stage2.py:327), L <= 32;
//   cir_cross_attention_folded_long for captions of up to 64 tokens against up to 224 image tokens (nlvr_encoder.py:150-168, 183-217 with
//   encoder_hidden_states = the candidate's image tokens; the reference tokenises with padding='longest' and no 32-token cut,
//   blip_stage2.py:113, and FashionIQ joins two captions per query);
//   cir_cross_attention_folded_short for captions of at most 16 tokens against up to 608 image tokens: one 16-row block per head and no more;
//   cir_cross_attention_folded_long_wide for captions of 33 .. 64 tokens against 225 .. 608 image tokens (the same reference lines at the
//   384-px geometry, validate_stage2.py:327): the KEYS of a head split over two waves (below).
// The work is 12 ceil(L / 16) 16-row blocks per (candidate, branch) and nothing more: a wave owns ONE head and NB consecutive 16-token blocks of
// it, which share every X fragment read from LDS and every W_k^T / W_v fragment of their head.  The transposed score tile S^T of a block
// against KB 16-key blocks is KB accumulator tiles = 4 KB registers, and that decides the instantiations:
//     608 keys (KB = 38), L <= 32: NB = 1, two waves per head (S^T = 152 registers; three blocks, as in the 224-key kernel, would need 456)
//                         L <= 16: NB = 1, one wave per head (cir_cross_attention_folded_short only)
//     224 keys (KB = 14), L <= 16: NB = 1, one wave per head      L <= 32: NB = 2, one wave per head
//                         L <= 48: NB = 3, one wave per head (S^T = 168 registers)      L <= 64: NB = 2, two waves per head (S^T = 112 registers)
//     640 keys (KB = 40, capacity; N <= 608), 33 <= L <= 64: NB = 2, two token halves x TWO KEY HALVES (KH = 2) = four waves per head,
//                         each with key blocks 0-19 or 20-39 (S^T = 2 x 20 x 4 = 160 registers); a workgroup covers 2 heads, six per
//                         (candidate, branch).  Every X fragment read feeds two MFMAs (fold16: one).  33-48 tokens run it with block 4 on zero queries.
// Without the key split a workgroup covers 4 heads (4 or 8 waves); three workgroups per (candidate, branch), none waits for another: 4 heads x 32 tokens = 128 stacked
// query rows are what 8 waves of one block each hold.  Same four products and the same accumulator-as-operand chaining as xattn_fold.hip
// (G1 Q'^T = W_k^T q^T, G2 S^T += X Q'^T, softmax in registers, G3 C'^T = X^T P^T, G4 ctx^T += W_v C'^T, epilogue ctx / rowsum + b_v) and the same
// packed weights (ops.fold_pack_key / fold_pack_value).  X is staged per UNIT (KB x 16 keys x 32 features, two buffers) in two LDS layouts:
// 64-byte rows with the chunk position XOR-swizzled by f(row) = {0, 2, 3, 1}[(row >> 2) & 3] for phase 1's ds_read_b128 (the four 16-lane
// groups of a b128 read then hit 64 distinct banks), 96-byte rows for phase 2's transposing reads (8 rows x 8 dwords at a 24-dword stride:
// distinct multiples of 8).  At 577 keys, per (candidate, branch): 1.50 GFLOP instead of 2.83 (K|V GEMM 2.72 + attention 0.11).
// A query row is one COLUMN of every product, so its result depends on nothing but its own q row, X and the weights: every instantiation
// runs the same accumulation order per row (units in order, key blocks in order), hence a row's bits do not depend on T, on the candidate's
// place in the batch, on L or on the block assignment.  Rows >= L are computed on zero queries and never stored; keys >= N are read
// clamped to row N - 1 and get probability 0.
// The key-split instantiation (KH = 2) keeps all of that but sums a row's keys in TWO parts: its two key-half waves exchange their row maxima
// through LDS and both form P against the COMMON maximum (P rounds to 16 bits against the same reference point as everywhere else; a half
// without a valid key - N <= 320, or a mask - has maximum -inf, probabilities 0 and sum 0: half 0 always holds key 0, so the common maximum
// is finite and no -inf meets -inf); each accumulates C'^T and ctx^T over its own keys (G4 is linear), and at the end half 1 hands its row
// sums and its 64 x 32 fp32 ctx^T tile through LDS to half 0, which adds in the fixed order half 0 + half 1, applies / rowsum + b_v and
// stores.  Summation order of a row: units in order; key blocks in order within a half; half 0 + half 1.  Its rows are therefore NOT
// bit-identical to fold16's (one sum over all key blocks) - they are to each other, whatever T, L (33 .. 64), the place in the batch or the wave.
// Every cross-wave step is an LDS write, a workgroup barrier that all eight waves reach, and a read; no workgroup waits for another, no atomics.

#include "xattn_fold.hpp"

namespace cir {

constexpr int kStrideP2U = 96;               // phase 2's row stride

// What follows from the key-block count: KB 16-key blocks over 4 WPH waves, 1-KiB DMA pieces (64 slots of 16 B) per wave and unit.  KH key
// halves per head: the workgroup's 4 WPH waves then cover 4 / KH heads
template <int NB, int WPH, int KB, int KH = 1>
struct FoldUnitGeom {
    static constexpr int kHeads = 4 / KH;                                    // heads per workgroup
    static constexpr int kWaves = kHeads * WPH * KH;
    static constexpr int kStrideQ = kHeads * 128 + 32;                       // q rows in LDS: heads x 64 x 2 B + 32 (136 / 72 dwords = 8 mod 64: conflict-free b128 fragment reads)
    static constexpr int kRows = 16 * NB * WPH;                              // token rows the workgroup covers
    static constexpr int kP1 = (KB + kWaves - 1) / kWaves;                   // phase 1: 16 KB rows x 4 slots = KB pieces
    static constexpr int kP2 = (3 * KB + 2 * kWaves - 1) / (2 * kWaves);     // phase 2: 16 KB rows x 6 slots = 1.5 KB pieces
    static constexpr int kBuf = kWaves * kP2 * 1024;                         // one X-unit buffer (608 keys: 64 KiB, 224 keys: 24 KiB)
    static constexpr int kEx = KH == 2 ? kWaves * NB * 16 * 4 : 0;           // the key halves' row maxima: one float per (wave, block, row)
    static constexpr int kLds = 2 * kBuf + kRows * kStrideQ + kEx;
};

// NB 16-row blocks per wave, WPH token-split waves and KH key-split waves per head, KB 16-key blocks of which a wave holds KB / KH:
// wave = (head within the group, token part tw, key half kh), rows 16 (NB tw + nb) + l16 of head (4 / KH) hg + hw
template <typename T, bool MASKED, int NB, int WPH, int KB, int KH = 1>
__device__ __forceinline__ void fold_unit_body(const FoldArgs& a) {
    using X8 = typename Elem<T>::x8;
    using G = FoldUnitGeom<NB, WPH, KB, KH>;
    constexpr int KBW = KB / KH;                                  // key blocks per wave
    static_assert(KH == 1 || KH == 2, "one wave per head and token part, or two key halves");
    static_assert(KBW * KH == KB && KBW <= 38 && KBW % 2 == 0, "phase 2's steps are written out for at most 38 key blocks, and P packs them in pairs");
    static_assert(4 + G::kP2 <= KBW && 4 + G::kP1 <= KBW, "a unit's memory requests ride on its key-block steps");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int kThreads = 64 * G::kWaves;
    constexpr int kRows = G::kRows, kP1 = G::kP1, kP2 = G::kP2, kBuf = G::kBuf, kStrideQU = G::kStrideQ, kHeads = G::kHeads;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, g = lane >> 4;
    // XCDs 0-3 run branch 0, XCDs 4-7 branch 1 (see xattn_fold.hip); within a branch: (candidate, head group of 4 / KH)
    const int b = (blockIdx.x >> 2) & 1;
    const int idx = (blockIdx.x >> 3) * 4 + (blockIdx.x & 3);
    const int t = idx / (3 * KH), hg = idx - 3 * KH * t;
    if (t >= a.T) return;                                        // (whole workgroup; the grid is rounded up to a multiple of 8)

    const T* X = reinterpret_cast<const T*>(a.x) + (int64_t)t * a.x_s1;
    const int hw = wave / (WPH * KH);                            // head within the group
    const int tw = (wave / KH) % WPH;                            // token part
    const int kh = wave % KH;                                    // key half: key blocks [KBW kh, KBW kh + KBW)
    const int head = kHeads * hg + hw;
    const int tok0 = 16 * NB * tw + l16;                         // this lane's token row in block nb: tok0 + 16 nb

    // q of this workgroup's 4 / KH heads in LDS: kRows token rows x 64 kHeads values, rows beyond L zero
    char* const qs = smem + 2 * kBuf;
    {
        constexpr int kPc = 8 * kHeads;                           // 16-byte pieces per row
        const T* qb_ = reinterpret_cast<const T*>(a.q) + (int64_t)b * a.q_sb + (int64_t)t * a.L * a.q_rs + hg * (64 * kHeads);
#pragma unroll
        for (int i = 0; i < kRows * kPc / kThreads; ++i) {
            const int c = tid + i * kThreads;                     // 16-byte pieces: kRows rows x kPc
            const int row = c / kPc, ch = c % kPc;
            X8 v;
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = static_cast<T>(0.f);
            if (row < a.L) v = *reinterpret_cast<const X8*>(qb_ + (int64_t)row * a.q_rs + ch * 8);
            *reinterpret_cast<X8*>(qs + row * kStrideQU + ch * 16) = v;
        }
    }
    const int qoff = tok0 * kStrideQU + (hw * 64 + 8 * g) * 2;   // block nb: + 16 nb rows

    const __amdgpu_buffer_rsrc_t rs_x = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(X), 0, a.N * kFoldD * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(reinterpret_cast<const T*>(a.wkt) + (int64_t)b * a.w_sb), 0, kFoldD * kFoldD * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(reinterpret_cast<const T*>(a.wvp) + (int64_t)b * a.w_sb), 0, kFoldD * kFoldD * 2, 0x00020000);
    const int wlane = lane * 16;

    // phase-1 staging: slot s = row s >> 2, position s & 3 holds chunk (s & 3) ^ f(row); rows >= N repeat row N - 1
    int xoff1[kP1];
#pragma unroll
    for (int j = 0; j < kP1; ++j) {
        const int s = (wave * kP1 + j) * 64 + lane;
        const int row = s >> 2;
        const int f = (0x1E >> (2 * ((row >> 2) & 3))) & 3;      // {0, 2, 3, 1}[(row >> 2) & 3] packed two bits each: 0b00_01_11_10 -> 0x1E
        xoff1[j] = (min(row, a.N - 1) * kFoldD + (((s & 3) ^ f) * 8)) * 2;
    }

    // ---------------------------------------------------------------- phase 1: S^T (16 KB keys x 16 NB rows per wave) --------------------
    f32x4 S[KBW][NB];
#pragma unroll
    for (int kb = 0; kb < KBW; ++kb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) S[kb][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    X8 w[2][2];                                                   // [interleaved 16-feature tile][k-step]
    {
        char* base = smem + wave * kP1 * 1024;
#pragma unroll
        for (int j = 0; j < kP1; ++j) FOLD_DMA(rs_x, xoff1[j], 0, base + j * 1024);
    }
#pragma unroll
    for (int fbh = 0; fbh < 2; ++fbh)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) w[fbh][ks] = wload<X8>(rs_k, wlane, ((fbh * 12 + head) * 2 + ks) * 1024);
    const int fr = (0x1E >> (2 * ((l16 >> 2) & 3))) & 3;         // this lane's read swizzle: row = 16 kb + l16 -> f depends on (l16 >> 2) only
    for (int u = 0; u < 24; ++u) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const char* xs = smem + (u & 1) * kBuf;
        // G1: Q'^T tiles of features [32 u, 32 u + 32), interleaved (tile fbh row 4 g' + r = feature 8 g' + 4 fbh + r), for the NB row blocks
        f32x4 a1[2][NB];
#pragma unroll
        for (int fbh = 0; fbh < 2; ++fbh)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) a1[fbh][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            X8 qf[NB];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) qf[nb] = *reinterpret_cast<const X8*>(qs + qoff + nb * 16 * kStrideQU + 64 * ks);
#pragma unroll
            for (int fbh = 0; fbh < 2; ++fbh)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) a1[fbh][nb] = Elem<T>::mfma16(w[fbh][ks], qf[nb], a1[fbh][nb]);
        }
        X8 bq[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bq[nb] = pack_acc2<T>(a1[0][nb], a1[1][nb]);
        __builtin_amdgcn_sched_barrier(0);
        const bool more = u + 1 < 24;
        auto mem_op = [&](int j) {                                // next unit's 4 weight fragments, then its DMA pieces: one request per key block
            if (!more) return;
            if (j < 4) w[j >> 1][j & 1] = wload<X8>(rs_k, wlane, ((((u + 1) * 2 + (j >> 1)) * 12 + head) * 2 + (j & 1)) * 1024);
            else if (j < 4 + kP1) FOLD_DMA(rs_x, xoff1[j - 4], (u + 1) * 64, smem + ((u + 1) & 1) * kBuf + (wave * kP1 + j - 4) * 1024);
        };
        // G2: k-slot (g, j) = feature 32 u + 8 g + j: piece g of the key's 64-byte row, at position g ^ f(row)
        const char* xr = xs + KBW * kh * 1024 + l16 * 64 + ((g ^ fr) << 4);
        auto rd = [&](int kb) { return *reinterpret_cast<const X8*>(xr + kb * 16 * 64); };
        constexpr int kAhead = NB >= 3 ? 1 : 2;                   // fragments in flight: three MFMAs per key block cover one read's latency
        X8 xa[kAhead + 1];
#pragma unroll
        for (int kb = 0; kb < kAhead; ++kb) xa[kb] = rd(kb);
#pragma unroll
        for (int kb = 0; kb < KBW; ++kb) {
            if (kb + kAhead < KBW) xa[(kb + kAhead) % (kAhead + 1)] = rd(kb + kAhead);
            mem_op(kb);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) S[kb][nb] = Elem<T>::mfma16(xa[kb % (kAhead + 1)], bq[nb], S[kb][nb]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // The lane's coordinates for everything behind phase 1, taken anew (from mbcnt, not from threadIdx): held across phase 1 they are the
    // registers that no longer fit beside the 168 of S^T at NB = 3
    const int lane2 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const int l16b = lane2 & 15, gb = lane2 >> 4;
    // ---------------------------------------------------------------- softmax over the keys of each row (log2 domain) -------------------
    const float sl = a.scale * 1.4426950408889634f;
    float rinv[NB];
    X8 P[KBW / 2][NB];
    // logits and row maxima: the key's validity (a compare = an SGPR pair) and its mask value serve the NB blocks at once and die
    float mx[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) mx[nb] = -INFINITY;
#pragma unroll
    for (int kb = 0; kb < KBW; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int key = 16 * (KBW * kh + kb) + 4 * gb + r;
            const bool live = key < a.N;
            float mk = 0.f;
            if constexpr (MASKED)     // (as xattn_fold_kernel: log2-domain logits incl. the additive key mask)
                mk = fmaxf(a.mask[(int64_t)t * a.m_st + min(key, a.N - 1)], -2.0e38f);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                float v = live ? S[kb][nb][r] : -INFINITY;
                if constexpr (MASKED) v = live ? fmaf(mk, 1.4426950408889634f, S[kb][nb][r] * sl) : -INFINITY;
                S[kb][nb][r] = v;
                mx[nb] = fmaxf(mx[nb], v);
            }
            if (r == 3) __builtin_amdgcn_sched_barrier(0);       // (keeps the compares next to their selects: 4 KB hoisted compare masks do not fit the SGPR file)
        }
    if constexpr (KH == 2) {
        // the two key halves of a (head, token part) are waves 2 p and 2 p + 1: each leaves its row maxima in LDS, and both go on with the
        // common one.  A half without a valid key leaves -inf; the common maximum is finite (key 0 is in half 0), so its exp2 below are 0
        float* const ex = reinterpret_cast<float*>(smem + 2 * kBuf + kRows * kStrideQU);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            float m = mx[nb];
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            mx[nb] = m;
            ex[(wave * NB + nb) * 16 + l16b] = m;                 // (all four 16-lane groups hold and write the same value: no branch, which
                                                                  // would let the compiler sink block 1's selects past it, their compare masks spilled)
        }
        __syncthreads();
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) mx[nb] = fmaxf(mx[nb], ex[((wave ^ 1) * NB + nb) * 16 + l16b]);
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        float m = mx[nb];
        if constexpr (KH == 1) {
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));
        }
        const float ms = MASKED ? m : m * sl;
        float sum = 0.f;
#pragma unroll
        for (int kb = 0; kb < KBW; ++kb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = MASKED ? __builtin_amdgcn_exp2f(S[kb][nb][r] - ms) : __builtin_amdgcn_exp2f(fmaf(S[kb][nb][r], sl, -ms));
                S[kb][nb][r] = p;
                sum += p;
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        rinv[nb] = KH == 1 ? 1.0f / sum : sum;                    // (KH = 2: this half's sum; the epilogue adds the halves)
#pragma unroll
        for (int p = 0; p < KBW / 2; ++p) P[p][nb] = pack_acc2<T>(S[2 * p][nb], S[2 * p + 1][nb]);
    }

    // ---------------------------------------------------------------- phase 2: ctx^T (64 d x 16 NB rows per wave) ------------------------
    f32x4 c4[4][NB];
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) c4[db][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    X8 wv[4];
    const int wlane2 = lane2 * 16;
    // staging: slot s = row s / 6, position s % 6 (positions 4, 5 are padding)
    int xoff2[kP2];
#pragma unroll
    for (int j = 0; j < kP2; ++j) {
        const int s = (wave * kP2 + j) * 64 + lane2;
        const int row = s / 6, c = s - 6 * row;
        xoff2[j] = (min(row, a.N - 1) * kFoldD + min(c, 3) * 8) * 2;
    }
    __syncthreads();                                              // every wave is done with phase 1's buffers
    {
        char* base = smem + wave * kP2 * 1024;
#pragma unroll
        for (int j = 0; j < kP2; ++j) FOLD_DMA(rs_x, xoff2[j], 0, base + j * 1024);
    }
    const int troff = (4 * gb + (l16b >> 2)) * kStrideP2U + (4 * (l16b & 3)) * 2;
    for (int u = 0; u < 24; ++u) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        const bool more = u + 1 < 24;
        auto mem_op = [&](int j) {                                // this unit's 4 W_v fragments (needed by G4 at its end), then the next unit's DMA pieces
            if (j < 4) wv[j] = wload<X8>(rs_v, wlane2, ((u * 4 + j) * 12 + head) * 1024);
            else if (j < 4 + kP2 && more) FOLD_DMA(rs_x, xoff2[j - 4], (u + 1) * 64, smem + ((u + 1) & 1) * kBuf + (wave * kP2 + j - 4) * 1024);
        };
        const unsigned xaddr = (unsigned)(size_t)(lptr_t)(smem + (u & 1) * kBuf + KBW * kh * 16 * kStrideP2U + troff);
        f32x4 a3[2][NB];
#pragma unroll
        for (int fbh = 0; fbh < 2; ++fbh)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) a3[fbh][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
        u32x2 lo[3], hi[3];
        // The transposing reads are inline asm with counted waits of their own (see xattn_fold.hip); step I = key pair I >> 1 (32 keys),
        // 16-feature block I & 1.  Expanded by macro, not by `#pragma unroll`: the asm immediates need the step index as a literal, and with a
        // 38-case switch inside the loop hipcc gave up unrolling - P and the fragment registers then lived in scratch.  38 steps are written
        // out; `if constexpr` discards those at and beyond KB.
#define FOLDU_TR(SLOT, I)                                                                                                       \
        asm volatile("ds_read_b64_tr_b16 %0, %2 offset:%3\n\tds_read_b64_tr_b16 %1, %2 offset:%4"                                 \
                     : "=&v"(lo[SLOT]), "=&v"(hi[SLOT]) : "v"(xaddr), "n"((32 * ((I) >> 1)) * kStrideP2U + (16 * ((I) & 1)) * 2),    \
                       "n"((32 * ((I) >> 1) + 16) * kStrideP2U + (16 * ((I) & 1)) * 2) : "memory")
        FOLDU_TR(0, 0);
        FOLDU_TR(1, 1);
#define FOLDU_STEP(I)                                                                                                             \
        if constexpr ((I) < KBW) {                                                                                                 \
            if constexpr ((I) + 2 < KBW) FOLDU_TR(((I) + 2) % 3, (I) + 2);                                                           \
            mem_op(I);                                                                                                             \
            if constexpr ((I) + 2 < KBW) asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(lo[(I) % 3]), "+v"(hi[(I) % 3]));                \
            else if constexpr ((I) + 1 < KBW) asm volatile("s_waitcnt lgkmcnt(2)" : "+v"(lo[(I) % 3]), "+v"(hi[(I) % 3]));           \
            else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(lo[(I) % 3]), "+v"(hi[(I) % 3]));                                       \
            __builtin_amdgcn_sched_barrier(0);                                                                                     \
            const u32x4 both = {lo[(I) % 3].x, lo[(I) % 3].y, hi[(I) % 3].x, hi[(I) % 3].y};                                        \
            const X8 xa = __builtin_bit_cast(X8, both);                                                                            \
            _Pragma("unroll") for (int nb = 0; nb < NB; ++nb) a3[(I) & 1][nb] = Elem<T>::mfma16(xa, P[(I) >> 1][nb], a3[(I) & 1][nb]); \
            __builtin_amdgcn_sched_barrier(0);                                                                                     \
        }
#define FOLDU_STEP4(I) FOLDU_STEP(I) FOLDU_STEP((I) + 1) FOLDU_STEP((I) + 2) FOLDU_STEP((I) + 3)
        FOLDU_STEP4(0) FOLDU_STEP4(4) FOLDU_STEP4(8) FOLDU_STEP4(12) FOLDU_STEP4(16) FOLDU_STEP4(20) FOLDU_STEP4(24) FOLDU_STEP4(28) FOLDU_STEP4(32)
        FOLDU_STEP(36) FOLDU_STEP(37)
#undef FOLDU_STEP4
#undef FOLDU_STEP
#undef FOLDU_TR
        // G4: ctx^T += W_v[:, these 32 features (k-slot order)] C'^T
        X8 bq[NB];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) bq[nb] = pack_acc2<T>(a3[0][nb], a3[1][nb]);
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) c4[db][nb] = Elem<T>::mfma16(wv[db], bq[nb], c4[db][nb]);
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---------------------------------------------------------------- epilogue ---------------------------------------------------------
    if constexpr (KH == 2) {
        // Half 1 hands its row sums and its ctx^T tile (4 NB accumulator tiles, lane-major: 16-byte pieces of consecutive lanes) to half 0
        // through X buffer 0: the last unit read buffer 1, every wave finished its reads of buffer 0 before the barrier of that unit, and
        // no DMA is under way.  Half 0 adds in the order half 0 + half 1.
        f32x4* const cx = reinterpret_cast<f32x4*>(smem) + (wave >> 1) * (4 * NB * 64) + lane2;
        float* const sx = reinterpret_cast<float*>(smem + (kThreads / 128) * 4 * NB * 64 * 16) + (wave >> 1) * (NB * 64) + lane2;
        static_assert((kThreads / 128) * (4 * NB * 64 * 16 + NB * 64 * 4) <= kBuf, "the hand-over fits one X buffer");
        if (kh == 1) {
#pragma unroll
            for (int db = 0; db < 4; ++db)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) cx[(db * NB + nb) * 64] = c4[db][nb];
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) sx[nb * 64] = rinv[nb];
        }
        __syncthreads();
        if (kh == 1) return;
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) c4[db][nb] = c4[db][nb] + cx[(db * NB + nb) * 64];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) rinv[nb] = 1.0f / (rinv[nb] + sx[nb * 64]);
    }
    T* ob = reinterpret_cast<T*>(a.out) + (int64_t)t * a.o_st + (int64_t)b * a.o_sb + head * 64 + 4 * gb;
    const float* brow = a.bv + b * kFoldD + head * 64 + 4 * gb;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int tok = 16 * NB * tw + l16b + 16 * nb;
        if (tok >= a.L) continue;
        T* orow = ob + (int64_t)tok * a.o_sr;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
            const float4 b4 = *reinterpret_cast<const float4*>(brow + 16 * db);
            u32x2 o;
            o.x = pack2<T>(fmaf(c4[db][nb][0], rinv[nb], b4.x), fmaf(c4[db][nb][1], rinv[nb], b4.y));
            o.y = pack2<T>(fmaf(c4[db][nb][2], rinv[nb], b4.z), fmaf(c4[db][nb][3], rinv[nb], b4.w));
            *reinterpret_cast<u32x2*>(orow + 16 * db) = o;
        }
    }
}

// Five kernels around the one body (the fifth, with the key split, below), two waves per SIMD each (256 registers): 608 keys, two waves of one block per head (8 waves); 224 keys,
// one wave of NB blocks per head (4 waves); 224 keys, two waves of two blocks per head (8 waves); 608 keys, one wave of one block per head (4 waves).
// (separate kernels with literal bounds: a launch bound that depends on a template parameter, 256 * WPH, fails to substitute in hipcc's host pass)
template <typename T, bool MASKED>
__global__ __launch_bounds__(512, 2) void xattn_fold16_kernel(const FoldArgs a) { fold_unit_body<T, MASKED, 1, 2, 38>(a); }
template <typename T, bool MASKED, int NB>
__global__ __launch_bounds__(256, 2) void xattn_fold_long_kernel(const FoldArgs a) { fold_unit_body<T, MASKED, NB, 1, kFoldKB>(a); }
template <typename T, bool MASKED>
__global__ __launch_bounds__(512, 2) void xattn_fold_long64_kernel(const FoldArgs a) { fold_unit_body<T, MASKED, 2, 2, kFoldKB>(a); }
// 608 keys, captions of at most 16 tokens: one wave of one block per head (4 waves) - fold16 without its second, all-zero wave.  10 phase-1 and
// 15 phase-2 DMA pieces per wave (40 for 38 key blocks, 60 for 57 KiB): the surplus pieces lie inside the unit buffer and read rows clamped to
// N - 1, and the 14 (19) memory requests of a unit spread over its 38 key-block steps.  128.5 KiB of LDS: one workgroup per CU whatever the
// bound; (256, 2) keeps S^T in 234 VGPRs, (256, 1) moves it to AGPRs and pays ~400 v_accvgpr copies (LABNOTES.md section 18).
template <typename T, bool MASKED>
__global__ __launch_bounds__(256, 2) void xattn_fold16_short_kernel(const FoldArgs a) { fold_unit_body<T, MASKED, 1, 1, 38>(a); }
// 640 keys of capacity (N <= 608), captions of 33 .. 64 tokens: per head two token halves of two blocks x two key halves of 20 key blocks
// (8 waves = 2 heads).  5 phase-1 and 8 phase-2 DMA pieces per wave: the same 64-KiB unit buffers as fold16's; 147 KiB of LDS with the q rows of
// 2 heads and the row maxima: one workgroup per CU.
template <typename T, bool MASKED>
__global__ __launch_bounds__(512, 2) void xattn_fold_wide_kernel(const FoldArgs a) { fold_unit_body<T, MASKED, 2, 2, 40, 2>(a); }

template <int NB, int WPH, int KB, int KH = 1>
static int launch_fold_units(FoldKernel kernel, const FoldArgs& a, hipStream_t s) {
    using G = FoldUnitGeom<NB, WPH, KB, KH>;
    const int64_t per_branch = 3 * KH * (int64_t)a.T;
    return fold_launch(kernel, dim3((unsigned)(8 * ((per_branch + 3) / 4))), dim3(64 * G::kWaves), G::kLds, s, a);
}

int launch_fold16(const FoldArgs& a, int dtype, hipStream_t s) {
    return by_dtype_mask(dtype, a.mask != nullptr, [&](auto t, auto mk) {
        const FoldKernel k = &xattn_fold16_kernel<typename decltype(t)::type, decltype(mk)::value>;
        return launch_fold_units<1, 2, 38>(k, a, s);
    });
}

// cost in 16-row steps: 1, 2 or 3 blocks per wave and head up to 48 tokens, two waves of 2 blocks per head above
template <typename T, bool MASKED>
static int launch_fold_long(const FoldArgs& a, hipStream_t s) {
    if (a.L <= 16) return launch_fold_units<1, 1, kFoldKB>(xattn_fold_long_kernel<T, MASKED, 1>, a, s);
    if (a.L <= 32) return launch_fold_units<2, 1, kFoldKB>(xattn_fold_long_kernel<T, MASKED, 2>, a, s);
    if (a.L <= 48) return launch_fold_units<3, 1, kFoldKB>(xattn_fold_long_kernel<T, MASKED, 3>, a, s);
    return launch_fold_units<2, 2, kFoldKB>(xattn_fold_long64_kernel<T, MASKED>, a, s);
}

// captions of at most 16 tokens: 12 blocks per (candidate, branch) at either key count
template <typename T, bool MASKED>
static int launch_fold_short(const FoldArgs& a, hipStream_t s) {
    if (a.N <= 16 * kFoldKB) return launch_fold_units<1, 1, kFoldKB>(xattn_fold_long_kernel<T, MASKED, 1>, a, s);
    return launch_fold_units<1, 1, 38>(xattn_fold16_short_kernel<T, MASKED>, a, s);
}

// captions of 33 .. 64 tokens against 225 .. 608 keys: ONE instantiation for every L, so a row's bits do not depend on the caption's length
template <typename T, bool MASKED>
static int launch_fold_wide(const FoldArgs& a, hipStream_t s) {
    return launch_fold_units<2, 2, 40, 2>(xattn_fold_wide_kernel<T, MASKED>, a, s);
}

}  // namespace cir

// The query-side fold for captions of up to 64 tokens (nlvr_encoder.py:150-168, 183-217; blip_stage2.py:113: padding='longest', no
// 32-token cut) against up to 224 keys; parameters as cir_cross_attention_folded.
extern "C" int cir_cross_attention_folded_long(const void* q, int64_t q_sb, int64_t q_rs, const void* x, int64_t x_s1, const void* wkt, const void* wvp,
                                               int64_t w_sb, const float* bv, const float* key_mask, int64_t mask_stride, void* out, int64_t o_st,
                                               int64_t o_sr, int64_t o_sb, int T, int L, int N, int D, int H, float scale, int dtype, void* stream) {
    using namespace cir;
    FoldArgs a;
    const int rc = fold_args(a, q, q_sb, q_rs, x, x_s1, wkt, wvp, w_sb, bv, key_mask, mask_stride, out, o_st, o_sr, o_sb, T, L, N, D, H, scale, dtype,
                             64, 16 * kFoldKB, (int64_t)T * 6 + 8);
    if (rc != CIR_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return by_dtype_mask(dtype, key_mask != nullptr, [&](auto t, auto mk) { return launch_fold_long<typename decltype(t)::type, decltype(mk)::value>(a, s); });
}

// The query-side fold for captions of at most 16 tokens (nlvr_encoder.py:150-168, 183-217; blip_stage2.py:113: batch 1, padding='longest' -
// a short modification sentence is never padded to 32) against up to 608 keys; parameters as cir_cross_attention_folded.
extern "C" int cir_cross_attention_folded_short(const void* q, int64_t q_sb, int64_t q_rs, const void* x, int64_t x_s1, const void* wkt, const void* wvp,
                                                int64_t w_sb, const float* bv, const float* key_mask, int64_t mask_stride, void* out, int64_t o_st,
                                                int64_t o_sr, int64_t o_sb, int T, int L, int N, int D, int H, float scale, int dtype, void* stream) {
    using namespace cir;
    FoldArgs a;
    const int rc = fold_args(a, q, q_sb, q_rs, x, x_s1, wkt, wvp, w_sb, bv, key_mask, mask_stride, out, o_st, o_sr, o_sb, T, L, N, D, H, scale, dtype,
                             16, 608, (int64_t)T * 6 + 8);
    if (rc != CIR_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return by_dtype_mask(dtype, key_mask != nullptr, [&](auto t, auto mk) { return launch_fold_short<typename decltype(t)::type, decltype(mk)::value>(a, s); });
}

// The query-side fold for captions of 33 .. 64 tokens (nlvr_encoder.py:150-168, 183-217; blip_stage2.py:113: padding='longest', no 32-token
// cut) against 225 .. 608 keys (validate_stage2.py:327: 384 px = 577 image tokens); parameters as cir_cross_attention_folded_long.  The keys
// of a head are summed in two halves (blocks 0-19, 20-39): units in order; key blocks in order within a half; half 0 + half 1.
extern "C" int cir_cross_attention_folded_long_wide(const void* q, int64_t q_sb, int64_t q_rs, const void* x, int64_t x_s1, const void* wkt, const void* wvp,
                                                    int64_t w_sb, const float* bv, const float* key_mask, int64_t mask_stride, void* out, int64_t o_st,
                                                    int64_t o_sr, int64_t o_sb, int T, int L, int N, int D, int H, float scale, int dtype, void* stream) {
    using namespace cir;
    FoldArgs a;
    const int rc = fold_args(a, q, q_sb, q_rs, x, x_s1, wkt, wvp, w_sb, bv, key_mask, mask_stride, out, o_st, o_sr, o_sb, T, L, N, D, H, scale, dtype,
                             64, 608, (int64_t)T * 12 + 8, 33, 225);
    if (rc != CIR_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    return by_dtype_mask(dtype, key_mask != nullptr, [&](auto t, auto mk) { return launch_fold_wide<typename decltype(t)::type, decltype(mk)::value>(a, s); });
}
