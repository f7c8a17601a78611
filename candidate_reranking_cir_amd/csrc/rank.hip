// The per-row sorts of the library: one bitonic network on (value, column) pairs in LDS (rank_sort_first), one order - a before b <=>
// a.val > b.val, or equal values and a.idx < b.idx; a NaN reads as -inf; an excluded column does not exist.  That order is strict and
// total, so every result below is unique.
//
// cir_topk_desc: the whole order of rows of at most 8192 columns - level 1 below on one segment with k = n, which keeps every place.
//
// Stage-I retrieval over an index of any size: the first k columns of every row's descending order (cir_topk_select) and the place of
// a few given columns in that order (cir_rank_of) - what stage II reads of a full ranking (validate.py:57-64, 202-226), without the
// 8192-column ceiling of one workgroup's sort.  Because the order is total,
//   first_k(row) = first_k(union over segments of first_k(segment))
// holds exactly - ties across segment seams, NaNs, +-inf and exclusions included.  Level 1 sorts each segment of at most 8192 columns in
// LDS and keeps its first k (value, column) pairs; level 2 sorts groups of floor(8192 / k) such lists the same way until one is left.
// Lists are always k pairs long: missing places hold the padding pair (-inf, INT_MAX), which comes after every real column (columns are
// below 2^31 - 1) and never reaches the result: cir_topk_select has k <= n - 1 real columns in every row, and cir_topk_desc's one segment
// holds exactly k = n real pairs before its padding.
//
// Rank refinement (cir_rank_undecided, cir_rank_refine_apply; validate_stage2.py:53, 174, 188): the same sort and order, on rows of at most
// 8192 logits of a fast precision mode - which entries lie within 2 * margin of a neighbour of the sorted row, so that only they are scored
// again by the exact mode, and the write-back of those scores with a check of the margin on the values they replace.  cir_rank_undecided_cuts
// keeps of them only the runs of linked places that reach into the first places or straddle a recall cut-off: what top-k lists and Recall@c
// read.  The two entry points share the host path and the scan and emit launches; each has its own flag kernel.
#include "common.hpp"

namespace cir {

constexpr int RANK_SEG = 8192;                  // pairs per workgroup sort: 64 KiB of LDS
constexpr int RANK_PAD = 0x7fffffff;

struct __attribute__((aligned(8))) RankPair { float v; int i; };

__device__ __forceinline__ bool rank_before(float va, int ia, float vb, int ib) { return (va > vb) || (va == vb && ia < ib); }
__device__ __forceinline__ float rank_key(float v) { return v != v ? -INFINITY : v; }   // NaN sorts last

// the pairs one workgroup sorts for n of them.  The host sizes LDS and the block by it and hands it to the two levels of cir_topk_select, which
// ask again only for a row's last segment or group of lists: it may be shorter than the others
__host__ __device__ inline int rank_pow2(int n) { int p = 2; while (p < n) p <<= 1; return p; }
static dim3 rank_block(int pow2) { return dim3(pow2 >= 2048 ? 1024 : 256); }

// The first `first` places of the sorted order, in place (first: a power of two, 2 <= first <= n_pow2; every thread of the workgroup calls it).
// Phase 1 is the bitonic network on interleaved pairs (one 8-byte LDS access per pair), stopped at runs of `first`: they
// come out alternately descending and ascending.  Phase 2 halves the number of runs until one is left: a descending run and its ascending
// neighbour form a bitonic sequence, so the pairwise winners (place i against place i, `span` apart) are the `first` leading pairs of the two
// runs and bitonic again; one merge pass (strides first / 2 .. 1) sorts them, descending or ascending by the run's new number.  Only winners
// are kept, so a segment of 8192 costs 28 + 6 * 8 steps at first = 128, all but the first 28 on a shrinking part, against 91 full ones.
__device__ __forceinline__ void rank_sort_first(RankPair* p, int n_pow2, int first) {
    for (int size = 2; size <= first; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < n_pow2 / 2; t += blockDim.x) {
                const int lo = 2 * t - (t & (stride - 1));
                const int hi = lo + stride;
                const bool asc_block = ((lo & size) != 0);
                const RankPair a = p[lo], b = p[hi];
                const bool a_first = rank_before(a.v, a.i, b.v, b.i);
                if (asc_block ? a_first : !a_first) { p[lo] = b; p[hi] = a; }
            }
            __syncthreads();
        }
    }
    const int lg = __ffs(first) - 1;
    for (int span = first; span < n_pow2;) {
        for (int t = threadIdx.x; t < (n_pow2 / (2 * span)) * first; t += blockDim.x) {
            const int lo = (t >> lg) * 2 * span + (t & (first - 1));
            const RankPair a = p[lo], b = p[lo + span];
            if (!rank_before(a.v, a.i, b.v, b.i)) p[lo] = b;          // the loser's run is not read again
        }
        __syncthreads();
        span <<= 1;
        for (int stride = first >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (n_pow2 / span) * (first >> 1); t += blockDim.x) {
                const int run = t >> (lg - 1), u = t & ((first >> 1) - 1);
                const int lo = run * span + 2 * u - (u & (stride - 1));
                const int hi = lo + stride;
                const RankPair a = p[lo], b = p[hi];
                const bool a_first = rank_before(a.v, a.i, b.v, b.i);
                if ((run & 1) ? a_first : !a_first) { p[lo] = b; p[hi] = a; }
            }
            __syncthreads();
        }
    }
}

// the first k sorted pairs: to a k-pair list of the workspace, or - the last level - to the result rows
__device__ __forceinline__ void rank_emit(const RankPair* p, int n_pow2, int k, RankPair* list, int64_t* idx, float* val) {
    for (int j = threadIdx.x; j < k; j += blockDim.x) {
        RankPair e;
        if (j < n_pow2) e = p[j]; else { e.v = -INFINITY; e.i = RANK_PAD; }
        if (list != nullptr) list[j] = e;
        else { idx[j] = e.i; if (val != nullptr) val[j] = e.v; }
    }
}

// ---- level 1: one workgroup per (row, segment); blockIdx.x = row * segs + segment ----
__global__ __launch_bounds__(1024) void topk_segment_kernel(const float* __restrict__ values, int64_t ld, const int64_t* __restrict__ exclude, int n, int k,
                                                            int seg_pow2, int keep, int segs, RankPair* __restrict__ lists,
                                                            int64_t* __restrict__ idx, float* __restrict__ val) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    RankPair* p = reinterpret_cast<RankPair*>(dyn);
    const int64_t row = blockIdx.x / (unsigned)segs;
    const int seg = (int)(blockIdx.x - row * segs);
    const int c0 = seg * RANK_SEG;                      // < n
    const int len = min(n - c0, RANK_SEG);
    const int n_pow2 = seg + 1 < segs || segs == 1 ? seg_pow2 : rank_pow2(len);     // only the last of several segments is shorter than the host's
    const int64_t ex = exclude != nullptr ? exclude[row] : -1;
    const float* src = values + row * ld + c0;
    for (int i = threadIdx.x; i < n_pow2; i += blockDim.x) {
        RankPair e;
        if (i < len && (int64_t)(c0 + i) != ex) { e.v = rank_key(src[i]); e.i = c0 + i; }
        else { e.v = -INFINITY; e.i = RANK_PAD; }
        p[i] = e;
    }
    __syncthreads();
    rank_sort_first(p, n_pow2, min(keep, n_pow2));
    if (lists != nullptr) rank_emit(p, n_pow2, k, lists + (int64_t)blockIdx.x * k, nullptr, nullptr);
    else rank_emit(p, n_pow2, k, nullptr, idx + row * k, val != nullptr ? val + row * k : nullptr);
}

// ---- level 2: one workgroup per (row, group of at most `group` lists); blockIdx.x = row * lists_out + g; group * k <= 8192 ----
__global__ __launch_bounds__(1024) void topk_merge_kernel(const RankPair* __restrict__ in, int lists_in, int group, int lists_out, int k, int grp_pow2, int keep,
                                                          RankPair* __restrict__ out, int64_t* __restrict__ idx, float* __restrict__ val) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    RankPair* p = reinterpret_cast<RankPair*>(dyn);
    const int64_t row = blockIdx.x / (unsigned)lists_out;
    const int g = (int)(blockIdx.x - row * lists_out);
    const int first = g * group;
    const int cnt = min(group, lists_in - first) * k;
    const int n_pow2 = g + 1 < lists_out || lists_out == 1 ? grp_pow2 : rank_pow2(cnt);     // as for level 1's last segment
    const RankPair* src = in + (row * lists_in + first) * k;
    for (int i = threadIdx.x; i < n_pow2; i += blockDim.x) {
        RankPair e;
        if (i < cnt) e = src[i]; else { e.v = -INFINITY; e.i = RANK_PAD; }
        p[i] = e;
    }
    __syncthreads();
    rank_sort_first(p, n_pow2, min(keep, n_pow2));
    if (out != nullptr) rank_emit(p, n_pow2, k, out + (int64_t)blockIdx.x * k, nullptr, nullptr);
    else rank_emit(p, n_pow2, k, nullptr, idx + row * k, val != nullptr ? val + row * k : nullptr);
}

// (value, column) -> one unsigned 64-bit word whose integer order is the order above: a before b <=> rank_word(a) > rank_word(b).  High half: the
// key's bits made monotone (-0 joins +0, as the float compare has them equal); low half: INT_MAX - column, so the lower column is the larger word.
__device__ __forceinline__ unsigned long long rank_word(float v, int col) {
    v = rank_key(v);
    if (v == 0.f) v = 0.f;
    const unsigned u = __float_as_uint(v);
    const unsigned hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)hi << 32) | (unsigned)(RANK_PAD - col);
}

// ---- rank[q][t] = number of columns of row q that come before column cols[q][t]; one workgroup per row, one pass, integer counts ----
__global__ __launch_bounds__(256) void rank_of_kernel(const float* __restrict__ values, int64_t ld, const int64_t* __restrict__ cols,
                                                      const int64_t* __restrict__ exclude, int64_t* __restrict__ rank, int n, int m) {
    __shared__ int part[4][8];
    const int64_t row = blockIdx.x;
    const float* r = values + row * ld;
    int64_t ex = exclude != nullptr ? exclude[row] : -1;
    if (ex < 0 || ex >= n) ex = -1;
    unsigned long long kw[8];
    int cnt[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int64_t c = t < m ? cols[row * m + t] : -1;
        const bool valid = c >= 0 && c < n && c != ex;
        kw[t] = valid ? rank_word(r[c], (int)c) : ~0ull;   // no word is above ~0: an invalid column counts nothing
        cnt[t] = 0;
    }
    auto count = [&](float v, int j) {
        const unsigned long long w = rank_word(v, j);
#pragma unroll
        for (int t = 0; t < 8; ++t) cnt[t] += w > kw[t] ? 1 : 0;
    };
    // scalar head up to the row's first 16-byte boundary, float4 body, scalar tail (rows of a strided view start anywhere)
    const int head = min(n, (int)((4 - ((reinterpret_cast<uintptr_t>(r) >> 2) & 3)) & 3));
    const int nvec = (n - head) >> 2;
    if ((int)threadIdx.x < head) count(r[threadIdx.x], threadIdx.x);
    const float4* r4 = reinterpret_cast<const float4*>(r + head);
    for (int i = threadIdx.x; i < nvec; i += 256) {
        const float4 v = r4[i];
        const int j = head + 4 * i;
        count(v.x, j); count(v.y, j + 1); count(v.z, j + 2); count(v.w, j + 3);
    }
    const int tail0 = head + 4 * nvec;
    if ((int)threadIdx.x < n - tail0) count(r[tail0 + threadIdx.x], tail0 + threadIdx.x);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt[t] += __shfl_xor(cnt[t], o, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][t] = cnt[t];
    }
    __syncthreads();
    if ((int)threadIdx.x < m) {
        const int t = threadIdx.x;
        const int64_t c = cols[row * m + t];
        const bool valid = c >= 0 && c < n && c != ex;
        int total = part[0][t] + part[1][t] + part[2][t] + part[3][t];   // fixed order (and integers)
        if (valid && ex >= 0 && rank_word(r[ex], (int)ex) > rank_word(r[c], (int)c)) total -= 1;   // the excluded column was counted
        rank[row * m + t] = valid ? (int64_t)total : -1;
    }
}

// ---- rank refinement: which entries of a row of fast logits can the fast mode not order? (validate_stage2.py:53, 174, 188) ----
// One workgroup per row sorts the whole row (rank_sort_first with first = n_pow2) and links neighbours of the sorted row whose fp32 difference
// is at most `width` = 2 * margin; an entry linked to either neighbour is undecided.  flags[row * K + column] receives 1 / 0 for every column
// (an inactive row: all 0), row_count[row] the number of ones.  The padding pairs sort behind all K real ones, so places 0 .. K - 1 are real
// and every column written is below K.  A difference that is not a number (-inf against -inf: NaN keys, the padding) fails `<=` and links nothing.
__global__ __launch_bounds__(1024) void undecided_flag_kernel(const float* __restrict__ values, int64_t ld, const unsigned char* __restrict__ active,
                                                              float width, int K, unsigned char* __restrict__ flags, int* __restrict__ row_count) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    RankPair* p = reinterpret_cast<RankPair*>(dyn);
    const int64_t row = blockIdx.x;
    unsigned char* f = flags + row * K;
    if (active != nullptr && active[row] == 0) {                       // uniform over the workgroup: nobody reaches a barrier
        for (int i = threadIdx.x; i < K; i += blockDim.x) f[i] = 0;
        if (threadIdx.x == 0) row_count[row] = 0;
        return;
    }
    int n_pow2 = 2;
    while (n_pow2 < K) n_pow2 <<= 1;
    const float* src = values + row * ld;
    for (int i = threadIdx.x; i < n_pow2; i += blockDim.x) {
        RankPair e;
        if (i < K) { e.v = rank_key(src[i]); e.i = i; }
        else { e.v = -INFINITY; e.i = RANK_PAD; }
        p[i] = e;
    }
    __syncthreads();
    rank_sort_first(p, n_pow2, n_pow2);
    int mine = 0;
    for (int j = threadIdx.x; j < K; j += blockDim.x) {
        const RankPair e = p[j];
        bool und = false;
        if (j > 0) und = (p[j - 1].v - e.v) <= width;
        if (j + 1 < K) und = und || ((e.v - p[j + 1].v) <= width);
        f[e.i] = und ? 1 : 0;
        mine += und ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    __syncthreads();                                                    // the sorted pairs are read: their memory takes the waves' partial counts
    int* part = reinterpret_cast<int*>(dyn);                            // (at least 16 ints: the launch asks for 128 bytes or more)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) total += part[w];
        row_count[row] = total;
    }
}

// ---- the same, for the first places and the recall cut-offs only (cir_rank_undecided_cuts) ----
// bound[0 .. n): the boundaries B of {first} and the cuts with 1 <= B <= K - 1 (the host drops the others: they straddle nothing).
struct UndecidedBounds { int first, n, bound[9]; };

constexpr int CUTS_PER_THREAD = 8;                                      // places per thread: 8192 / 1024, or at most 1024 / 256
constexpr int CUTS_LDS_INTS = 16 * 18 + 18 + 16;                        // the waves' partial L / R, the reduced L / R, the waves' partial counts

// Same sort, same links.  A linked place j is flagged iff j < first, or L_B <= j <= R_B for a boundary B whose link (B - 1, B) holds, where
// [L_B, R_B] is the cluster that straddles B: L_B the largest place <= B - 1 that is place 0 or has no link to its predecessor, R_B the
// smallest place >= B that is place K - 1 or has no link to its successor.  A boundary whose link does not hold gets R_B = -1: nothing lies
// in [L_B, -1].  Every thread keeps its places' columns and links in registers, so the memory of the sorted pairs (all 64 KiB at K = 8192)
// can take the integer max / min reductions: waves by shuffles, the 16 waves in a fixed order.
__global__ __launch_bounds__(1024) void undecided_cuts_flag_kernel(const float* __restrict__ values, int64_t ld, const unsigned char* __restrict__ active,
                                                                   float width, int K, UndecidedBounds bounds, unsigned char* __restrict__ flags,
                                                                   int* __restrict__ row_count) {
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    RankPair* p = reinterpret_cast<RankPair*>(dyn);
    const int64_t row = blockIdx.x;
    unsigned char* f = flags + row * K;
    if (active != nullptr && active[row] == 0) {                       // uniform over the workgroup: nobody reaches a barrier
        for (int i = threadIdx.x; i < K; i += blockDim.x) f[i] = 0;
        if (threadIdx.x == 0) row_count[row] = 0;
        return;
    }
    int n_pow2 = 2;
    while (n_pow2 < K) n_pow2 <<= 1;
    const float* src = values + row * ld;
    for (int i = threadIdx.x; i < n_pow2; i += blockDim.x) {
        RankPair e;
        if (i < K) { e.v = rank_key(src[i]); e.i = i; }
        else { e.v = -INFINITY; e.i = RANK_PAD; }
        p[i] = e;
    }
    __syncthreads();
    rank_sort_first(p, n_pow2, n_pow2);
    int col[CUTS_PER_THREAD];
    unsigned prev_link = 0, next_link = 0;                              // bit i: place threadIdx.x + i * blockDim.x is linked to its predecessor / successor
    int lo[9], hi[9];
#pragma unroll
    for (int b = 0; b < 9; ++b) { lo[b] = -1; hi[b] = K; }
#pragma unroll
    for (int i = 0; i < CUTS_PER_THREAD; ++i) {
        const int j = threadIdx.x + i * blockDim.x;
        col[i] = 0;
        if (j < K) {
            const RankPair e = p[j];
            col[i] = e.i;
            const bool lp = j > 0 && (p[j - 1].v - e.v) <= width;
            const bool ln = j + 1 < K && (e.v - p[j + 1].v) <= width;
            prev_link |= lp ? 1u << i : 0u;
            next_link |= ln ? 1u << i : 0u;
#pragma unroll
            for (int b = 0; b < 9; ++b) {
                if (b < bounds.n) {
                    const int B = bounds.bound[b];
                    if (j <= B - 1 && !lp) lo[b] = max(lo[b], j);
                    if (j >= B && !ln) hi[b] = min(hi[b], j);
                    if (j == B && !lp) hi[b] = -1;
                }
            }
        }
    }
#pragma unroll
    for (int b = 0; b < 9; ++b) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo[b] = max(lo[b], __shfl_xor(lo[b], o, 64));
            hi[b] = min(hi[b], __shfl_xor(hi[b], o, 64));
        }
    }
    __syncthreads();                                                    // the sorted pairs are read: their memory takes the reductions
    int* part = reinterpret_cast<int*>(dyn);                            // (the launch asks for CUTS_LDS_INTS ints or more)
    int* red = part + 16 * 18;
    int* cnt = red + 18;
    const int waves = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int b = 0; b < 9; ++b) { part[(threadIdx.x >> 6) * 18 + b] = lo[b]; part[(threadIdx.x >> 6) * 18 + 9 + b] = hi[b]; }
    }
    __syncthreads();
    if (threadIdx.x < 18) {
        const bool is_lo = threadIdx.x < 9;
        int r = part[threadIdx.x];
        for (int w = 1; w < waves; ++w) r = is_lo ? max(r, part[w * 18 + threadIdx.x]) : min(r, part[w * 18 + threadIdx.x]);
        red[threadIdx.x] = r;
    }
    __syncthreads();
#pragma unroll
    for (int b = 0; b < 9; ++b) {
        if (b < bounds.n) { lo[b] = red[b]; hi[b] = red[9 + b]; }
        else { lo[b] = 0; hi[b] = -1; }
    }
    int mine = 0;
#pragma unroll
    for (int i = 0; i < CUTS_PER_THREAD; ++i) {
        const int j = threadIdx.x + i * blockDim.x;
        if (j < K) {
            bool sel = j < bounds.first;
#pragma unroll
            for (int b = 0; b < 9; ++b) sel = sel || (lo[b] <= j && j <= hi[b]);
            const bool und = sel && (((prev_link | next_link) >> i) & 1u) != 0;
            f[col[i]] = und ? 1 : 0;
            mine += und ? 1 : 0;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
    if ((threadIdx.x & 63) == 0) cnt[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < waves; ++w) total += cnt[w];
        row_count[row] = total;
    }
}

// row_start[q] = sum of row_count[0 .. q - 1], row_start[Q] = count[0] = the total: ONE workgroup, thread t owns the rows
// [t * per, (t + 1) * per); integers, so the result does not depend on how the sum is bracketed
__global__ __launch_bounds__(1024) void undecided_scan_kernel(const int* __restrict__ row_count, int64_t Q, int64_t* __restrict__ row_start,
                                                              int64_t* __restrict__ count) {
    __shared__ int64_t part[1024];
    const int64_t per = (Q + 1023) / 1024;
    const int64_t r0 = min((int64_t)threadIdx.x * per, Q), r1 = min(r0 + per, Q);
    int64_t sum = 0;
    for (int64_t r = r0; r < r1; ++r) sum += row_count[r];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                                // inclusive scan of the 1024 partial sums
        const int64_t add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int64_t run = part[threadIdx.x] - sum;
    for (int64_t r = r0; r < r1; ++r) { row_start[r] = run; run += row_count[r]; }
    if (threadIdx.x == 1023) { row_start[Q] = part[1023]; count[0] = part[1023]; }
}

// pos[row_start[row] + (number of flagged columns below k)] = row * K + k for every flagged column k: ascending within the row, rows in
// order.  One workgroup of 256 per row; thread t owns the columns [t * per, (t + 1) * per), per <= 32.
__global__ __launch_bounds__(256) void undecided_emit_kernel(const unsigned char* __restrict__ flags, const int* __restrict__ row_count,
                                                             const int64_t* __restrict__ row_start, int K, int64_t* __restrict__ pos) {
    __shared__ int part[256];
    const int64_t row = blockIdx.x;
    if (row_count[row] == 0) return;                                   // uniform over the workgroup
    const unsigned char* f = flags + row * K;
    const int per = (K + 255) / 256;
    const int c0 = min((int)threadIdx.x * per, K), c1 = min(c0 + per, K);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += f[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
        const int add = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int64_t at = row_start[row] + (part[threadIdx.x] - sum);            // < row_start[row] + row_count[row] <= Q * K: inside pos
    for (int c = c0; c < c1; ++c)
        if (f[c]) pos[at++] = row * K + c;
}

// values[pos[i]] <- referee[i], i < n, and what the overwritten values say about the bound: stats_max[0] = max |old - referee| (a difference
// that is not a number does not enter the maximum), stats_bad[0] = how many i fail |old - referee| <= margin (a NaN difference fails).
// ONE workgroup: a maximum and an integer count, reduced in a fixed order.  A position outside [0, Q * K) is skipped and counted as failing.
__global__ __launch_bounds__(1024) void refine_apply_kernel(float* __restrict__ values, int64_t ld, int K, int64_t total,
                                                            const int64_t* __restrict__ pos, const float* __restrict__ referee, int64_t n,
                                                            float margin, float* __restrict__ stats_max, int64_t* __restrict__ stats_bad) {
    __shared__ float wmax[16];
    __shared__ int64_t wbad[16];
    float m = 0.f;
    int64_t bad = 0;
    for (int64_t i = threadIdx.x; i < n; i += 1024) {
        const int64_t at = pos[i];
        if (at < 0 || at >= total) { bad += 1; continue; }
        float* dst = values + (at / K) * ld + (at % K);
        const float d = fabsf(*dst - referee[i]);
        *dst = referee[i];
        if (d > m) m = d;
        if (!(d <= margin)) bad += 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = fmaxf(m, __shfl_xor(m, o, 64));
        bad += __shfl_xor(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { wmax[threadIdx.x >> 6] = m; wbad[threadIdx.x >> 6] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float tm = 0.f;
        int64_t tb = 0;
        for (int w = 0; w < 16; ++w) { tm = fmaxf(tm, wmax[w]); tb += wbad[w]; }
        stats_max[0] = tm;
        stats_bad[0] = tb;
    }
}

// workspace of cir_rank_undecided: flags (Q * K bytes), row_count (Q int32), row_start (Q + 1 int64), each part on an 8-byte boundary
struct UndecidedPlan { int64_t off_count, off_start, bytes; };

static int undecided_plan(int64_t Q, int64_t K, UndecidedPlan* plan) {
    if (Q <= 0 || K <= 0) return CIR_EINVAL;
    if (K > RANK_SEG || Q > 0x7fffffffLL) return CIR_ESHAPE;
    plan->off_count = (Q * K + 7) & ~(int64_t)7;
    plan->off_start = plan->off_count + ((Q * 4 + 7) & ~(int64_t)7);
    plan->bytes = plan->off_start + (Q + 1) * 8;
    return CIR_OK;
}

struct RankPlan { int segs, group; int64_t bytes_a, bytes_b; };

// the extents' checks and the workspace layout shared by the three entry points: list buffer A (Q * segs lists of k pairs, level 1's
// output) and, above one segment, buffer B (Q * ceil(segs / group) lists); the merge rounds alternate between the two
static int rank_plan(int64_t Q, int64_t n, int64_t k, RankPlan* plan) {
    if (Q <= 0 || n <= 0 || k <= 0) return CIR_EINVAL;
    if (k > 2048 || k > n - 1 || n > 0x7fffffffLL) return CIR_ESHAPE;
    const int64_t segs = (n + RANK_SEG - 1) / RANK_SEG;
    if (Q * segs > 0x7fffffffLL) return CIR_ESHAPE;      // one grid dimension over (row, segment)
    plan->segs = (int)segs;
    plan->group = (int)(RANK_SEG / k);
    plan->bytes_a = Q * segs * k * (int64_t)sizeof(RankPair);
    plan->bytes_b = segs > 1 ? Q * ((segs + plan->group - 1) / plan->group) * k * (int64_t)sizeof(RankPair) : 0;
    return CIR_OK;
}

}  // namespace cir

// the whole order of a row: level 1 on one segment with k = n, so rank_sort_first keeps every place; the K real pairs come before the padding,
// so places 0 .. K - 1 are real.  Not through rank_plan: its k <= n - 1 belongs to cir_topk_select's lists.
extern "C" int cir_topk_desc(const float* logits, int64_t* idx, int Q, int K, void* stream) {
    using namespace cir;
    CIR_CHECK_PTR(logits); CIR_CHECK_PTR(idx);
    if (Q <= 0 || K <= 0) return CIR_EINVAL;
    if (K > RANK_SEG) return CIR_ESHAPE;   // every index of the reference's datasets fits
    const int pow2 = rank_pow2(K);
    hipLaunchKernelGGL(topk_segment_kernel, dim3((unsigned)Q), rank_block(pow2), (size_t)pow2 * sizeof(RankPair), reinterpret_cast<hipStream_t>(stream),
                       logits, (int64_t)K, nullptr, K, K, pow2, pow2, 1, nullptr, idx, nullptr);
    CIR_LAUNCH_RESULT();
}

extern "C" int64_t cir_topk_select_workspace(int Q, int n, int k) {
    cir::RankPlan plan;
    const int code = cir::rank_plan(Q, n, k, &plan);
    return code != CIR_OK ? (int64_t)code : plan.bytes_a + plan.bytes_b;
}

extern "C" int cir_topk_select(const float* values, int64_t ld, const int64_t* exclude, int64_t* idx, float* val, int Q, int n, int k,
                               void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace cir;
    CIR_CHECK_PTR(values); CIR_CHECK_PTR(idx);
    if (ld < n) return CIR_EINVAL;
    RankPlan plan;
    const int code = rank_plan(Q, n, k, &plan);
    if (code != CIR_OK) return code;
    if (workspace == nullptr || workspace_bytes < plan.bytes_a + plan.bytes_b) return CIR_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int seg_pow2 = rank_pow2(n < RANK_SEG ? n : RANK_SEG);
    RankPair* buf_a = reinterpret_cast<RankPair*>(workspace);
    RankPair* buf_b = reinterpret_cast<RankPair*>(reinterpret_cast<char*>(workspace) + plan.bytes_a);
    {
        dim3 grid((unsigned)((int64_t)Q * plan.segs));
        hipLaunchKernelGGL(topk_segment_kernel, grid, rank_block(seg_pow2), (size_t)seg_pow2 * sizeof(RankPair), s, values, ld, exclude, n, k,
                           seg_pow2, rank_pow2(k), plan.segs,
                           plan.segs > 1 ? buf_a : nullptr, idx, val);
    }
    RankPair *in = buf_a, *out = buf_b;
    for (int lists = plan.segs; lists > 1;) {
        const int lists_out = (lists + plan.group - 1) / plan.group;
        const int pow2 = rank_pow2((lists < plan.group ? lists : plan.group) * k);
        dim3 grid((unsigned)((int64_t)Q * lists_out));
        hipLaunchKernelGGL(topk_merge_kernel, grid, rank_block(pow2), (size_t)pow2 * sizeof(RankPair), s, in, lists, plan.group, lists_out, k, pow2, rank_pow2(k),
                           lists_out > 1 ? out : nullptr, idx, val);
        RankPair* t = in; in = out; out = t;
        lists = lists_out;
    }
    CIR_LAUNCH_RESULT();
}

extern "C" int64_t cir_rank_undecided_workspace(int Q, int K) {
    cir::UndecidedPlan plan;
    const int code = cir::undecided_plan(Q, K, &plan);
    return code != CIR_OK ? (int64_t)code : plan.bytes;
}

// both rank_undecided entry points, after their argument checks: the extents' refusals, the workspace, the three launches.
// bounds == nullptr: the full rule's flag kernel
static int rank_undecided_launch(const float* values, int64_t ld, const unsigned char* active, float margin, const cir::UndecidedBounds* bounds,
                                 int64_t* pos, int64_t* count, int Q, int K, void* workspace, int64_t workspace_bytes, void* stream) {
    using namespace cir;
    UndecidedPlan plan;
    const int code = undecided_plan(Q, K, &plan);
    if (code != CIR_OK) return code;
    if (workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || workspace_bytes < plan.bytes) return CIR_EINVAL;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned char* flags = reinterpret_cast<unsigned char*>(workspace);
    int* row_count = reinterpret_cast<int*>(flags + plan.off_count);
    int64_t* row_start = reinterpret_cast<int64_t*>(flags + plan.off_start);
    const int pow2 = rank_pow2(K);
    const size_t floor_bytes = bounds == nullptr ? 128 : ((size_t)CUTS_LDS_INTS * sizeof(int) + 127) & ~(size_t)127;
    const size_t lds = (size_t)pow2 * sizeof(RankPair) < floor_bytes ? floor_bytes : (size_t)pow2 * sizeof(RankPair);
    if (bounds == nullptr)
        hipLaunchKernelGGL(undecided_flag_kernel, dim3((unsigned)Q), rank_block(pow2), lds, s, values, ld, active, 2.f * margin, K, flags, row_count);
    else
        hipLaunchKernelGGL(undecided_cuts_flag_kernel, dim3((unsigned)Q), rank_block(pow2), lds, s, values, ld, active, 2.f * margin, K, *bounds, flags,
                           row_count);
    hipLaunchKernelGGL(undecided_scan_kernel, dim3(1), dim3(1024), 0, s, row_count, (int64_t)Q, row_start, count);
    hipLaunchKernelGGL(undecided_emit_kernel, dim3((unsigned)Q), dim3(256), 0, s, flags, row_count, row_start, K, pos);
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_rank_undecided(const float* values, int64_t ld, const unsigned char* active, float margin, int64_t* pos, int64_t* count,
                                  int Q, int K, void* workspace, int64_t workspace_bytes, void* stream) {
    CIR_CHECK_PTR(values); CIR_CHECK_PTR(pos); CIR_CHECK_PTR(count);
    if (ld < K || !(margin >= 0.f) || !(margin <= 3.402823466e38f)) return CIR_EINVAL;      // (a NaN margin fails both comparisons)
    return rank_undecided_launch(values, ld, active, margin, nullptr, pos, count, Q, K, workspace, workspace_bytes, stream);
}

extern "C" int cir_rank_undecided_cuts(const float* values, int64_t ld, const unsigned char* active, float margin, int first, const int* cuts,
                                       int n_cuts, int64_t* pos, int64_t* count, int Q, int K, void* workspace, int64_t workspace_bytes,
                                       void* stream) {
    CIR_CHECK_PTR(values); CIR_CHECK_PTR(pos); CIR_CHECK_PTR(count);
    if (ld < K || !(margin >= 0.f) || !(margin <= 3.402823466e38f)) return CIR_EINVAL;      // (a NaN margin fails both comparisons)
    if (first < 0 || n_cuts < 0 || n_cuts > 8 || (n_cuts > 0 && cuts == nullptr)) return CIR_EINVAL;
    for (int i = 0; i < n_cuts; ++i)
        if (cuts[i] < 1 || (i > 0 && cuts[i] <= cuts[i - 1])) return CIR_EINVAL;
    cir::UndecidedBounds bounds;                                         // (for a K the plan refuses: never launched)
    bounds.first = first < K ? first : K;
    bounds.n = 0;
    for (int b = 0; b < 9; ++b) bounds.bound[b] = 0;
    if (first >= 1 && first <= K - 1) bounds.bound[bounds.n++] = first;
    for (int i = 0; i < n_cuts; ++i)
        if (cuts[i] <= K - 1) bounds.bound[bounds.n++] = cuts[i];
    return rank_undecided_launch(values, ld, active, margin, &bounds, pos, count, Q, K, workspace, workspace_bytes, stream);
}

extern "C" int cir_rank_refine_apply(float* values, int64_t ld, const int64_t* pos, const float* referee, int64_t n, float margin, void* stats,
                                     int Q, int K, void* stream) {
    CIR_CHECK_PTR(values); CIR_CHECK_PTR(stats);
    if (n < 0 || Q <= 0 || K <= 0 || ld < K || !(margin >= 0.f) || !(margin <= 3.402823466e38f)) return CIR_EINVAL;
    if (n > 0 && (pos == nullptr || referee == nullptr)) return CIR_EINVAL;
    if ((reinterpret_cast<uintptr_t>(stats) & 7u) != 0) return CIR_EALIGN;
    if (n > (int64_t)Q * K) return CIR_ESHAPE;
    hipLaunchKernelGGL(cir::refine_apply_kernel, dim3(1), dim3(1024), 0, reinterpret_cast<hipStream_t>(stream), values, ld, K, (int64_t)Q * K, pos,
                       referee, n, margin, reinterpret_cast<float*>(stats), reinterpret_cast<int64_t*>(reinterpret_cast<char*>(stats) + 8));
    CIR_LAUNCH_RESULT();
}

extern "C" int cir_rank_of(const float* values, int64_t ld, const int64_t* cols, const int64_t* exclude, int64_t* rank, int Q, int n, int m,
                           void* stream) {
    CIR_CHECK_PTR(values); CIR_CHECK_PTR(cols); CIR_CHECK_PTR(rank);
    if (Q <= 0 || n <= 0 || m <= 0 || ld < n) return CIR_EINVAL;
    if (m > 8) return CIR_ESHAPE;
    dim3 grid((unsigned)Q), block(256);
    hipLaunchKernelGGL(cir::rank_of_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), values, ld, cols, exclude, rank, n, m);
    CIR_LAUNCH_RESULT();
}
