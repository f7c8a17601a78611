// Fixed-order sums of the deterministic training mode (include/cirrank.h, "Fixed-order forms"): what the reverse pass adds across
// workgroups with fp32 atomics by default - per-column sums of row blocks, scattered embedding rows - formed here with plain stores and
// plain read-modify-writes by ONE workgroup per destination, in an order that depends on the shapes alone.  No workgroup waits for another.
//
// Bound: memory (every kernel here reads its rows once); none is on the default path.
#include "common.hpp"

namespace cir {

// ---- ordered column sums ------------------------------------------------------------------------------------------------------------
// block = 32 columns x 8 row lanes.  Row lane l adds rows r0 + l, r0 + l + 8, ... of its row block in ascending order into one accumulator
// that starts at 0; the eight lanes meet in LDS and are combined as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)).  The result is either stored
// to row blockIdx.y of `part` (first level of a long sum: kOrdRows rows per block) or added to its destination (grid.y = 1: all rows).
// Output column t of the launch reads source column d.src[t / seg] * seg + t % seg and belongs to d.out[t / seg] - one launch finishes the
// two or three vectors of a LayerNorm adjoint, and one source segment may feed two destinations (the bias gradient of a shared dense layer).
// `tail_cols`: the LAST row holds only its first tail_cols columns (the ragged last sequence of the embedding adjoint's dpos sum).
__global__ __launch_bounds__(256) void colsum_ordered_kernel(const float* __restrict__ x, int64_t ld, int64_t rows, int seg, const OrderedDst d,
                                                             float* __restrict__ part, int64_t tail_cols) {
    const int cl = threadIdx.x & 31, l = threadIdx.x >> 5;
    const int64_t t = (int64_t)blockIdx.x * 32 + cl;
    const int64_t total = (int64_t)d.nout * seg;
    const int j = t < total ? (int)(t / seg) : 0;
    const int c = (int)(t - (int64_t)j * seg);
    const int sj = j == 0 ? d.src[0] : j == 1 ? d.src[1] : j == 2 ? d.src[2] : d.src[3];
    const int64_t sc = (int64_t)sj * seg + c;
    const int64_t rows_c = sc < tail_cols ? rows : rows - 1;              // rows that hold this column
    const int64_t r0 = part != nullptr ? (int64_t)blockIdx.y * kOrdRows : 0;
    const int64_t r1 = part != nullptr && r0 + kOrdRows < rows_c ? r0 + kOrdRows : rows_c;
    float s = 0.f;
    if (t < total) {
        int64_t r = r0 + l;
        for (; r + 24 < r1; r += 32) {                       // four loads in flight, added in row order
            const float a0 = x[r * ld + sc], a1 = x[(r + 8) * ld + sc], a2 = x[(r + 16) * ld + sc], a3 = x[(r + 24) * ld + sc];
            s += a0; s += a1; s += a2; s += a3;
        }
        for (; r < r1; r += 8) s += x[r * ld + sc];
    }
    __shared__ float red[8][32];
    red[l][cl] = s;
    __syncthreads();
    if (l != 0 || t >= total) return;
    const float v = ((red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl])) + ((red[4][cl] + red[5][cl]) + (red[6][cl] + red[7][cl]));
    if (part != nullptr) { part[(int64_t)blockIdx.y * total + t] = v; return; }
    float* o = j == 0 ? d.out[0] : j == 1 ? d.out[1] : j == 2 ? d.out[2] : d.out[3];
    o[c] += v;                                               // the only writer of this element in the launch
}

int colsum_ordered_launch(const float* x, int64_t ld, int64_t rows, int seg, const OrderedDst& d, hipStream_t s) {
    const int64_t total = (int64_t)d.nout * seg;
    hipLaunchKernelGGL(colsum_ordered_kernel, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, s, x, ld, rows, seg, d, (float*)nullptr, total);
    CIR_LAUNCH_RESULT();
}

// x (rows, cols; the last row `tail_cols` wide) -> out (cols) +=, through `partials` when there is more than one row block
static int colsum_ordered(const float* x, int64_t ld, float* out, int64_t rows, int64_t cols, int64_t tail_cols, float* partials, hipStream_t s) {
    const int64_t nblk = (rows + kOrdRows - 1) / kOrdRows;
    OrderedDst d{};
    d.out[0] = out; d.nout = 1;
    hipLaunchKernelGGL(colsum_ordered_kernel, dim3((unsigned)((cols + 31) / 32), (unsigned)nblk), dim3(256), 0, s, x, ld, rows, (int)cols, d,
                       nblk == 1 ? nullptr : partials, tail_cols);
    if (nblk == 1) CIR_LAUNCH_RESULT();
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    return colsum_ordered_launch(partials, cols, nblk, (int)cols, d, s);
}

// ---- ordered embedding backward -------------------------------------------------------------------------------------------------------
// The rows are cut into chunks of kEmbChunk.  index[chunk][id] = the first row of the chunk that carries `id` (integer atomicMin: the result
// does not depend on arrival order).  That row's workgroup owns the chunk's sum for `id`: it adds the chunk's rows of that id in ascending
// row order, starting from its own.  With one chunk the sum goes straight into dword[id]; otherwise it is stored to row `owner` of `part`,
// and the owner of the FIRST chunk that holds the id adds the chunk sums in ascending chunk order and then adds the total to dword[id].
// A list of one id is thus never longer than kEmbChunk rows or (rows / kEmbChunk) chunk sums per workgroup: the padding id, which fills
// half of a stage-I batch, costs its owners 512 rows each instead of one workgroup 16 384.  Ids outside [0, table_rows) are skipped.
constexpr int kEmbNone = 0x7f7f7f7f;

__global__ __launch_bounds__(256) void embed_first_kernel(const int64_t* __restrict__ ids, int* __restrict__ index, int64_t rows, int64_t table_rows) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int64_t id = ids[r];
    if (id < 0 || id >= table_rows) return;
    atomicMin(index + (r / kEmbChunk) * table_rows + id, (int)r);
}

// Ordered list, in LDS, of the entries e in [0, n) for which pred(e) holds (wave 0 builds it; n <= 512); returns its length to every thread.
template <typename P>
__device__ __forceinline__ int ordered_list(int* list, int* count, int n, P pred) {
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < 64) {
        int cnt = 0;
        for (int b = 0; b < n; b += 64) {
            const int e = b + lane;
            const bool m = e < n && pred(e);
            const unsigned long long mask = __ballot(m);
            if (m) list[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = e;
            cnt += __popcll(mask);
        }
        if (lane == 0) *count = cnt;
    }
    __syncthreads();
    return *count;
}

__global__ __launch_bounds__(256) void embed_chunk_kernel(const int64_t* __restrict__ ids, const float* __restrict__ dy, const int* __restrict__ index,
                                                          float* __restrict__ part, float* __restrict__ dword, int64_t rows, int cols,
                                                          int64_t table_rows) {
    const int64_t r = blockIdx.x;
    const int64_t id = ids[r];
    if (id < 0 || id >= table_rows) return;
    const int64_t chunk = r / kEmbChunk;
    if (index[chunk * table_rows + id] != (int)r) return;                       // (uniform over the workgroup)
    const int64_t r_end = (chunk + 1) * kEmbChunk < rows ? (chunk + 1) * kEmbChunk : rows;
    __shared__ int list[kEmbChunk];
    __shared__ int count;
    const int64_t* later = ids + r + 1;
    const int n = ordered_list(list, &count, (int)(r_end - r - 1), [&](int e) { return later[e] == id; });
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= cols) return;
    const float* src = dy + (r + 1) * cols + c;
    float s = dy[r * cols + c];
    int j = 0;
    for (; j + 3 < n; j += 4) {
        const float a0 = src[(int64_t)list[j] * cols], a1 = src[(int64_t)list[j + 1] * cols], a2 = src[(int64_t)list[j + 2] * cols],
                    a3 = src[(int64_t)list[j + 3] * cols];
        s += a0; s += a1; s += a2; s += a3;
    }
    for (; j < n; ++j) s += src[(int64_t)list[j] * cols];
    if (dword != nullptr) dword[id * cols + c] += s;                            // one chunk: this workgroup is the id's only writer
    else part[r * cols + c] = s;
}

__global__ __launch_bounds__(256) void embed_finish_kernel(const int64_t* __restrict__ ids, const int* __restrict__ index, const float* __restrict__ part,
                                                           float* __restrict__ dword, int64_t rows, int cols, int64_t table_rows) {
    const int64_t r = blockIdx.x;
    const int64_t id = ids[r];
    if (id < 0 || id >= table_rows) return;
    const int64_t chunk = r / kEmbChunk, chunks = (rows + kEmbChunk - 1) / kEmbChunk;
    const int* col = index + id;                                                // index[chunk][id] over the chunks
    if (col[chunk * table_rows] != (int)r) return;
    int earlier = 0;
    for (int64_t q = threadIdx.x; q < chunk; q += 256) earlier |= col[q * table_rows] != kEmbNone;
    if (__syncthreads_or(earlier)) return;                                      // an earlier chunk holds the id: its owner finishes it
    __shared__ int list[kEmbChunk];
    __shared__ int count;
    const int c = blockIdx.y * 256 + threadIdx.x;
    float s = c < cols ? part[r * cols + c] : 0.f;
    for (int64_t base = chunk + 1; base < chunks; base += kEmbChunk) {          // later chunks, kEmbChunk of them per LDS list
        const int span = (int)(chunks - base < kEmbChunk ? chunks - base : kEmbChunk);
        const int n = ordered_list(list, &count, span, [&](int e) { return col[(base + e) * table_rows] != kEmbNone; });
        if (c < cols)
            for (int j = 0; j < n; ++j) s += part[(int64_t)col[(base + list[j]) * table_rows] * cols + c];
        __syncthreads();                                                        // the list is rebuilt by the next round
    }
    if (c < cols) dword[id * cols + c] += s;
}

}  // namespace cir

using namespace cir;

extern "C" int cir_colsum_ordered(const float* x, int64_t ld, float* out, int64_t rows, int cols, float* partials, int64_t partial_elems,
                                  void* stream) {
    CIR_CHECK_PTR(x); CIR_CHECK_PTR(out);
    if (rows <= 0 || cols <= 0) return CIR_EINVAL;
    const int64_t nblk = (rows + kOrdRows - 1) / kOrdRows;
    if (ld < cols || nblk > 65535) return CIR_ESHAPE;
    if (nblk > 1) {
        CIR_CHECK_PTR(partials);
        if (partial_elems < nblk * cols) return CIR_ESHAPE;
    }
    return colsum_ordered(x, ld, out, rows, cols, cols, partials, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int cir_embed_bwd_ordered(const int64_t* ids, const float* dy, float* dword, float* dpos, int64_t rows, int L, int cols, int64_t table_rows,
                                     float* partials, int64_t partial_elems, int32_t* index, int64_t index_elems, void* stream) {
    CIR_CHECK_PTR(ids); CIR_CHECK_PTR(dy); CIR_CHECK_PTR(dword); CIR_CHECK_PTR(dpos); CIR_CHECK_PTR(index);
    if (rows <= 0 || L <= 0 || cols <= 0 || table_rows <= 0) return CIR_EINVAL;
    if (rows >= kEmbNone) return CIR_ESHAPE;                                    // row numbers fit the index
    const int64_t chunks = (rows + kEmbChunk - 1) / kEmbChunk, seqs = (rows + L - 1) / L, pos_cols = (int64_t)L * cols;
    const int64_t pos_blocks = (seqs + kOrdRows - 1) / kOrdRows;
    if (pos_blocks > 65535 || pos_cols > 0x7fffffffLL) return CIR_ESHAPE;
    const int64_t need_word = chunks > 1 ? rows * cols : 0, need_pos = pos_blocks > 1 ? pos_blocks * pos_cols : 0;
    const int64_t need = need_word > need_pos ? need_word : need_pos;          // (the two sums use the workspace one after the other)
    if (need > 0) CIR_CHECK_PTR(partials);
    if (partial_elems < need || index_elems < chunks * table_rows) return CIR_ESHAPE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(index, 0x7f, (size_t)(chunks * table_rows) * sizeof(int32_t), s);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(embed_first_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, ids, index, rows, table_rows);
    const dim3 grid((unsigned)rows, (unsigned)((cols + 255) / 256));
    hipLaunchKernelGGL(embed_chunk_kernel, grid, dim3(256), 0, s, ids, dy, index, partials, chunks > 1 ? nullptr : dword, rows, cols, table_rows);
    if (chunks > 1) hipLaunchKernelGGL(embed_finish_kernel, grid, dim3(256), 0, s, ids, index, partials, dword, rows, cols, table_rows);
    e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    // dpos[l][c] = sum_b dy[b * L + l][c]: the column sums of dy read as (ceil(rows / L), L * cols), the last sequence possibly short
    return colsum_ordered(dy, pos_cols, dpos, seqs, pos_cols, (rows - (seqs - 1) * L) * cols, partials, s);
}
