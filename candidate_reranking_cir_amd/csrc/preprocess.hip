// The reference's image transform on the device (data_utils.py:23-101): TargetPad | SquarePad -> Resize(dim, BICUBIC) -> CenterCrop(dim)
// -> ToTensor -> Normalize, from decoded uint8 RGB images of any sizes to the normalised tensor, the ViT's patch operand rows or the raw
// resized uint8 image - one launch per batch, bit for bit PIL's 8-bit resize.
//
// The arithmetic (libImaging Resample.c, as PIL's Image.resize runs it for an 8-bit image):
//   horizontal pass first, into a UINT8 intermediate, then the vertical pass over that intermediate; one pass is
//       out = clip8(((1 << 21) + sum_j kk[j] * in[xmin + j]) >> 22)            int32 throughout, arithmetic shift
//   with kk the 22-bit fixed-point bicubic (a = -0.5) coefficients of precompute_coeffs.  The host forms them in float64 exactly as
//   libImaging does (candidate_reranking_cir_amd/preprocess.py: resample_taps) and hands them in as tables in coordinates of the PADDED
//   image; a pass PIL skips because the extent does not change is the table {x, 1, 1 << 22}: ((1 << 21) + (p << 22)) >> 22 = p.
//   The pad (data_utils.py:36-42 / 59-68: zeros, hp left and right, vp top and bottom) is never materialised: a padded coordinate outside
//   the source contributes 0, and a padded ROW contributes nothing at all (its horizontal pass gives clip8((1 << 21) >> 22) = 0): both are
//   skipped.  Tables hold only the dim rows / columns that survive CenterCrop(dim); ToTensor + Normalize (data_utils.py:82-83 / 99-100) are
//   a 768-entry table lookup (256 values per channel, formed by torch's own fp32 ops on the host).
//
// Shape: one workgroup of 192 threads per (image, band of 16 output rows, chunk of 64 output columns).  A thread owns one (column, channel)
// and 16 int32 accumulators - one per output row of the band.  The source rows the band's vertical windows cover are walked once, in order,
// through a double-buffered LDS stage of 3072 bytes: it holds as many rows' segments (the part of a source row the chunk's horizontal
// windows span, in aligned 16-byte pieces) as fit - 12 rows at 500 -> 481 columns - and each thread moves ONE piece per group of rows, the
// next group's loads issued before the current group's arithmetic (with one row per barrier a workgroup had ~250 bytes in flight and the
// kernel ran at the load latency: LABNOTES section 25).  Per staged row a thread forms its horizontal uint8 value from LDS bytes - its first
// 12 coefficients live in registers, the loop runs to the wave's longest window on scalar branches - and adds it into all 16 accumulators
// with the row's 16 vertical weights, which are staged with the rows (`vw`: 0 outside an output row's window, so the vertical pass is 16
// multiply-adds on four broadcast LDS reads, no branch; the branchy form it replaced cost as much as everything else together).  Both
// passes multiply with v_mad_i32_i24 (a 32-bit multiply runs at a quarter of the rate).
// Every tap count is a loop bound and every stage has a fixed size - nothing grows with the downscale factor: horizontal coefficients
// beyond the 12 are read from the table, at most 16 rows are staged at once, and a column whose window does not fit the 3072-byte stage (a
// downscale beyond ~15-fold on a full chunk) reads its pixels from global memory.  Results go through a 3 KiB LDS tile so that every layout
// is stored with consecutive lanes on consecutive elements.  Source rows that two neighbouring bands both need are read by both (19 % more
// rows at 375 -> 384 and at 224).
//
// Safety: the grid, and with it every output address, depends on B / dim / layout alone.  Descriptor and table CONTENT is never trusted:
// an image must lie inside the source buffer (else it is treated as having no rows: the image of an all-zero source), a tap-table row
// must lie inside the tap buffer (else its count is 0), every window is cut to the image's extent before the loop that reads it, a stage
// piece is loaded only where it lies inside the image's bytes, and a thread reads the stage only when its whole window lies in the part
// that was loaded.
#include "common.hpp"

namespace cir {

constexpr int kPreCols = 64;                  // output columns per workgroup
constexpr int kPreRows = 16;                  // output rows per workgroup (= one row of 16 x 16 patches)
constexpr int kPreThreads = kPreCols * 3;     // one thread per (column, channel)
constexpr int kPreSeg = kPreThreads * 16;     // bytes of a source row staged in LDS: one 16-byte piece per thread
constexpr int kPreHReg = 12;                  // horizontal coefficients a thread keeps in registers (windows up to a 2.5-fold downscale)
constexpr int kPreGroup = 16;                 // most source rows staged at once
constexpr int kPreSegPad = 48;                // a thread whose window is shorter than its wave's longest reads (with coefficient 0) past its own
constexpr int kPreDescInts = 16;
constexpr int kPreMaxTaps = 1 << 20;          // cap on a window length read from a table (keeps the index arithmetic inside int32 / int64)

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int clamp_i(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// a * b + c with a and b read as signed 24-bit values (v_mad_i32_i24, full rate; a 32-bit multiply runs at a quarter of it): PIL's
// coefficients stay below 1.3 * 2^22 in magnitude, pixels below 2^8.  The sum wraps in 32 bits like libImaging's int.
__device__ __forceinline__ int mad24(int a, int b, int c) { return (int)((unsigned)__mul24(a, b) + (unsigned)c); }

// one row of a tap table, checked against the buffer: {xmin, count}; count 0 when the row does not lie inside taps[0, taps_len)
struct TapRow { int xmin, cnt; };
__device__ __forceinline__ TapRow tap_row(const int* __restrict__ taps, int64_t taps_len, int tab, int stride, int idx, bool live) {
    TapRow t = {0, 0};
    const int64_t row = (int64_t)tab + (int64_t)idx * stride;
    if (live && tab >= 0 && stride >= 2 && row + 2 <= taps_len) {
        t.xmin = clamp_i(taps[row], -(1 << 29), 1 << 29);
        t.cnt = min(max(taps[row + 1], 0), min(stride - 2, kPreMaxTaps));
        if (row + 2 + t.cnt > taps_len) t.cnt = 0;
    }
    return t;
}

template <typename T>
__global__ __launch_bounds__(kPreThreads) void preprocess_kernel(const uint8_t* __restrict__ src, int64_t src_bytes, const int* __restrict__ desc,
                                                                 const int* __restrict__ taps, int64_t taps_len, const T* __restrict__ table,
                                                                 void* __restrict__ out, int dim, int chunks, int bands, int layout) {
    __shared__ __attribute__((aligned(16))) uint8_t seg[2][kPreSeg + kPreSegPad];
    __shared__ __attribute__((aligned(16))) int vw[2][kPreGroup][kPreRows];       // vertical weight of (staged source row, output row); 0 outside the window
    __shared__ int s_vlo[kPreRows], s_vcnt[kPreRows];                             // the band's vertical windows: first SOURCE row, length
    __shared__ uint8_t tile[kPreRows][kPreThreads];
    __shared__ T tab[768];
    const int tid = threadIdx.x;
    const int chunk = blockIdx.x % chunks, band = (blockIdx.x / chunks) % bands;
    const int64_t b = blockIdx.x / (chunks * bands);
    if (layout != CIR_PRE_RAW)
        for (int i = tid; i < 768; i += kPreThreads) tab[i] = table[i];

    // ---- the image (uniform over the workgroup)
    const int* d = desc + b * kPreDescInts;
    const int64_t base = (int64_t)d[0] * 16;
    const int w = d[2], htab = d[9], hstr = d[10], vtab = d[11], vstr = d[12];
    const int hp = clamp_i(d[3], -(1 << 29), 1 << 29), vp = clamp_i(d[4], -(1 << 29), 1 << 29);
    int h = d[1];
    if (d[0] < 0 || h <= 0 || w <= 0 || base + (int64_t)h * w * 3 > src_bytes) h = 0;        // does not fit its buffer: no rows are read
    const uint8_t* img = src + base;
    const int64_t avail = src_bytes - base;                                                  // bytes of the buffer from the image's first on

    // ---- this thread's horizontal window, cut to the image: taps [j0, j0 + n) of its table row read source columns [sxa, sxa + n)
    const int c = tid % 3, col = chunk * kPreCols + tid / 3;
    const TapRow hr = tap_row(taps, taps_len, htab, hstr, col, col < dim);
    const int j0 = clamp_i(hp - hr.xmin, 0, hr.cnt), j1 = clamp_i((int)min((int64_t)w + hp - hr.xmin, (int64_t)hr.cnt), j0, hr.cnt);
    const int n = h > 0 ? j1 - j0 : 0, sxa = hr.xmin + j0 - hp;
    const int* hk = taps + (n > 0 ? (int64_t)htab + (int64_t)col * hstr + 2 + j0 : 0);
    int hreg[kPreHReg];
#pragma unroll
    for (int i = 0; i < kPreHReg; ++i) hreg[i] = i < n ? hk[i] : 0;

    // ---- the source columns the chunk spans (uniform): from the first column's window to the last one's.  A thread reads the stage only
    // if its own window lies inside that span and the span's staged part (tables are not trusted to be monotone)
    const int last = min(chunk * kPreCols + kPreCols, dim) - 1;
    const TapRow f = tap_row(taps, taps_len, htab, hstr, chunk * kPreCols, true), l = tap_row(taps, taps_len, htab, hstr, last, true);
    const int xlo = clamp_i((int)max((int64_t)f.xmin - hp, (int64_t)0), 0, w);
    const int xhi = clamp_i((int)min((int64_t)l.xmin + l.cnt - hp, (int64_t)w), xlo, w);
    // the stage holds `rps` source rows of `ppr` 16-byte pieces each (a row's segment starts up to 15 bytes into its first piece): one
    // piece per thread and group of rows, so that a workgroup has a whole stage of loads in flight, not one row's
    const int ppr = min((int)(((int64_t)(xhi - xlo) * 3 + 30) >> 4), kPreThreads), rps = min(kPreThreads / ppr, kPreGroup);
    const int prow = tid / ppr, ppiece = tid - prow * ppr;
    const bool staged = n > 0 && sxa >= xlo && sxa + n <= xhi && (int64_t)(sxa + n - xlo) * 3 + 14 < (int64_t)ppr * 16;

    // ---- the band's vertical windows (LDS): thread r < 16 checks the table row of output row r
    const int64_t vbase = (int64_t)vtab + (int64_t)band * kPreRows * vstr + 2;           // coefficient j of output row r: taps[vbase + r * vstr + j]
    if (tid < kPreRows) {
        const TapRow t = tap_row(taps, taps_len, vtab, vstr, band * kPreRows + tid, band * kPreRows + tid < dim);
        s_vlo[tid] = t.xmin - vp;
        s_vcnt[tid] = t.cnt;
    }
    __syncthreads();
    // source rows [sy0, sy1): the union of the windows, cut to the image (rows of the pad contribute 0)
    int64_t y0 = 0, y1 = 0;
    bool any = false;
    for (int r = 0; r < kPreRows; ++r) {
        const int64_t lo = s_vlo[r], hi = lo + s_vcnt[r];
        if (hi > lo) {
            y0 = any ? min(y0, lo) : lo;
            y1 = any ? max(y1, hi) : hi;
            any = true;
        }
    }
    int sy0 = 0, sy1 = 0;
    if (any) {
        sy0 = __builtin_amdgcn_readfirstlane((int)min(max(y0, (int64_t)0), (int64_t)h));
        sy1 = __builtin_amdgcn_readfirstlane((int)min(max(y1, (int64_t)0), (int64_t)h));
    }
    // the weight of staged row (e / 16) of the group that starts at g in output row (e % 16), e = tid and tid + 192
    auto weight = [&](int g, int e) -> int {
        const int rr = e / kPreRows, r = e % kPreRows;
        const int64_t sy = (int64_t)g + rr;
        const unsigned j = (unsigned)sy - (unsigned)s_vlo[r];                             // (wraps far above any count when the row lies before the window)
        return (e < rps * kPreRows && sy < sy1 && j < (unsigned)s_vcnt[r]) ? taps[vbase + (int64_t)r * vstr + j] : 0;
    };

    // this thread's aligned 16-byte piece of the group of source rows that starts at g: piece `ppiece` of the segment [xlo, xhi) of row
    // g + prow; bytes outside the image's own are never loaded
    const int64_t img_bytes = (int64_t)h * w * 3;
    auto fetch = [&](int g) -> u32x4 {
        const int64_t sy = (int64_t)g + prow;
        const int64_t first = (sy * w + xlo) * 3, end = (sy * w + xhi) * 3;
        const int64_t off = (first & ~(int64_t)15) + ppiece * 16;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (prow < rps && sy < sy1 && off < end) {
            if (off + 16 <= img_bytes && off + 16 <= avail) {
                v = *reinterpret_cast<const u32x4*>(img + off);
            } else {                                          // the image's last piece: byte by byte up to its end
                unsigned q[4] = {0u, 0u, 0u, 0u};
                for (int k = 0; k < 16 && off + k < img_bytes; ++k) q[k >> 2] |= (unsigned)img[off + k] << (8 * (k & 3));
                v = u32x4{q[0], q[1], q[2], q[3]};
            }
        }
        return v;
    };

    int acc[kPreRows];
#pragma unroll
    for (int r = 0; r < kPreRows; ++r) acc[r] = 1 << 21;

    // horizontal pass of one source row at (col, c) - PIL's uint8 intermediate - from a byte pointer at this thread's first source pixel
    auto hpass = [&](const uint8_t* p) -> int {
        int ha = 1 << 21;
#pragma unroll
        for (int i = 0; i < kPreHReg; ++i)
            if (i < n) ha = mad24(hreg[i], (int)p[i * 3], ha);
        for (int i = kPreHReg; i < n; ++i) ha = mad24(hk[i], (int)p[i * 3], ha);
        return clip8(ha >> 22);
    };
    // the same from the LDS stage, without a test per lane: every lane of the wave runs the wave's longest window (scalar branches); a lane
    // beyond its own window multiplies by the 0 its registers hold there, and reads at most 33 bytes past it (kPreSegPad)
    const int nwave = __builtin_amdgcn_readfirstlane((int)wave_max((float)(staged ? n : 0)));
    auto hpass_lds = [&](const uint8_t* p) -> int {
        int ha = 1 << 21;
#pragma unroll
        for (int i = 0; i < kPreHReg; ++i)
            if (i < nwave) ha = mad24(hreg[i], (int)p[i * 3], ha);
        for (int i = kPreHReg; i < n; ++i) ha = mad24(hk[i], (int)p[i * 3], ha);
        return clip8(ha >> 22);
    };

    int buf = 0;
    u32x4 piece = {0u, 0u, 0u, 0u};
    int w0 = 0, w1 = 0;
    if (sy0 < sy1) { piece = fetch(sy0); w0 = weight(sy0, tid); w1 = weight(sy0, tid + kPreThreads); }
    for (int g = sy0; g < sy1; g += rps, buf ^= 1) {
        *reinterpret_cast<u32x4*>(&seg[buf][tid * 16]) = piece;  // (row prow, piece ppiece) sits at (prow * ppr + ppiece) * 16 = tid * 16
        (&vw[buf][0][0])[tid] = w0;
        if (tid + kPreThreads < kPreGroup * kPreRows) (&vw[buf][0][0])[tid + kPreThreads] = w1;
        __syncthreads();                                       // (two buffers: the next write of seg[buf] / vw[buf] follows the next barrier)
        if (g + rps < sy1) {                                    // in flight under this group's arithmetic
            piece = fetch(g + rps);
            w0 = weight(g + rps, tid);
            w1 = weight(g + rps, tid + kPreThreads);
        }
        const int rows = min(rps, sy1 - g);
        for (int rr = 0; rr < rows; ++rr) {
            const int sy = g + rr;
            const int shift = (int)((((int64_t)sy * w + xlo) * 3) & 15);
            const int h8 = staged ? hpass_lds(&seg[buf][rr * ppr * 16 + shift + (sxa - xlo) * 3 + c])
                                       : (n > 0 ? hpass(img + ((int64_t)sy * w + sxa) * 3 + c) : 0);
            // vertical pass: add it into every output row of the band whose window holds padded row sy + vp
            int wr[kPreRows];
#pragma unroll
            for (int q = 0; q < kPreRows / 4; ++q) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(&vw[buf][rr][4 * q]);   // one address for the whole workgroup: a broadcast
                wr[4 * q] = (int)v.x; wr[4 * q + 1] = (int)v.y; wr[4 * q + 2] = (int)v.z; wr[4 * q + 3] = (int)v.w;
            }
#pragma unroll
            for (int r = 0; r < kPreRows; ++r) acc[r] = mad24(wr[r], h8, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < kPreRows; ++r) tile[r][tid] = (uint8_t)clip8(acc[r] >> 22);
    __syncthreads();

    // ---- store: consecutive lanes on consecutive elements of the layout
    const int ncols = min(kPreCols, dim - chunk * kPreCols), nrows = min(kPreRows, dim - band * kPreRows);
    if (layout == CIR_PRE_RAW) {                                   // (B, dim, dim, 3) uint8
        uint8_t* o = static_cast<uint8_t*>(out);
        if (tid < ncols * 3)
            for (int r = 0; r < nrows; ++r)
                o[((b * dim + band * kPreRows + r) * dim + chunk * kPreCols) * 3 + tid] = tile[r][tid];
    } else if (layout == CIR_PRE_CHW) {                            // (B, 3, dim, dim)
        T* o = static_cast<T*>(out);
        for (int i = tid; i < 3 * kPreRows * kPreCols; i += kPreThreads) {
            const int x = i % kPreCols, r = (i / kPreCols) % kPreRows, ch = i / (kPreCols * kPreRows);
            if (x < ncols && r < nrows)
                o[((b * 3 + ch) * dim + band * kPreRows + r) * dim + chunk * kPreCols + x] = tab[ch * 256 + tile[r][x * 3 + ch]];
        }
    } else {                                                       // cir_patchify's rows: (B g g, 3 * 256), column (c, ky, kx); dim % 16 == 0
        T* o = static_cast<T*>(out);
        const int g = dim / 16;
        for (int i = tid; i < 3 * kPreRows * kPreCols; i += kPreThreads) {
            const int kx = i % 16, ky = (i / 16) % 16, ch = (i / 256) % 3, px = i / 768;
            const int x = px * 16 + kx;
            if (x < ncols)
                o[((b * g + band) * g + chunk * (kPreCols / 16) + px) * 768 + ch * 256 + ky * 16 + kx] = tab[ch * 256 + tile[ky][x * 3 + ch]];
        }
    }
}

}  // namespace cir

extern "C" int cir_preprocess_images(const uint8_t* src, int64_t src_bytes, const int32_t* desc, const int32_t* taps, int64_t taps_len,
                                     const void* table, void* out, int B, int dim, int layout, int dtype, void* stream) {
    using namespace cir;
    CIR_CHECK_PTR(src); CIR_CHECK_PTR(desc); CIR_CHECK_PTR(taps); CIR_CHECK_PTR(out);
    if (layout != CIR_PRE_CHW && layout != CIR_PRE_PATCHES && layout != CIR_PRE_RAW) return CIR_EINVAL;
    if (layout != CIR_PRE_RAW) CIR_CHECK_PTR(table);
    if (B <= 0 || dim <= 0 || src_bytes <= 0 || taps_len <= 0) return CIR_EINVAL;
    if (layout != CIR_PRE_RAW && dtype != CIR_BF16 && dtype != CIR_F16 && dtype != CIR_F32) return CIR_EDTYPE;
    if (dim > 4096 || (layout == CIR_PRE_PATCHES && dim % 16)) return CIR_ESHAPE;
    const int chunks = (dim + kPreCols - 1) / kPreCols, bands = (dim + kPreRows - 1) / kPreRows;
    if ((int64_t)B * chunks * bands > 0x7fffffffLL) return CIR_ESHAPE;
    if (!cir_aligned16(src) || !cir_aligned16(desc) || !cir_aligned16(taps) || !cir_aligned16(out) || (table && !cir_aligned16(table))) return CIR_EALIGN;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    dim3 grid((unsigned)((int64_t)B * chunks * bands)), block(kPreThreads);
    if (layout == CIR_PRE_RAW) {
        hipLaunchKernelGGL((preprocess_kernel<float>), grid, block, 0, s, src, src_bytes, desc, taps, taps_len, (const float*)nullptr, out, dim, chunks, bands, layout);
        CIR_LAUNCH_RESULT();
    }
    by_dtype3(dtype, [&](auto t) {
        using T = typename decltype(t)::type;
        hipLaunchKernelGGL((preprocess_kernel<T>), grid, block, 0, s, src, src_bytes, desc, taps, taps_len, (const T*)table, out, dim, chunks, bands, layout);
    });
    CIR_LAUNCH_RESULT();
}
