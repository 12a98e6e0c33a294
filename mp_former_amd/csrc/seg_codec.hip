// COCO ground truth to packed mask bits on MI355X: polygons (pycocotools' rleFrPoly) and run lengths (rleDecode) become the packed
// words every scoring kernel of seg_ap.hip / seg_boundary.hip / seg_box.hip / seg_pq.hip reads, without a dense mask on the host.
// Layout as there: position p = x * H + y (column-major, COCO's own order), 64 positions per uint64 word, bit b of word j =
// position 64 j + b, bits at or past H * W zero.
//
// rleFrPoly ends with "sort the boundary positions, take differences, merge zero-length runs": the mask at position p is the parity
// of the number of boundary positions <= p.  So both sources are written as TOGGLES, one XOR of one bit per boundary position into a
// zeroed plane, and one fill pass takes the running XOR in linear bit order.  No sort, no float on the mask side, and two toggles
// of one position cancel by themselves (a zero-length run, a boundary visited twice).
//
//   seg_poly_toggles_kernel   one workgroup per ring.  Edges are staged kStage at a time: scaled integer vertices, edge lengths
//                             max(|dx|, |dy|) + 1, a workgroup prefix sum.  Every thread walks dense point indices of the stage, finds
//                             the edge by binary search in the prefix, recomputes the point and its predecessor (the last point of the
//                             edge before, read from global memory where that edge belongs to the stage before) and applies the
//                             crossing rule: u changed, x on a pixel centre inside the image, y = the smaller v, clamped and rounded up.
//                             A surviving crossing is one 64-bit atomicXor.  Any vertex count: the stage is a loop.
//   seg_rle_toggles_kernel    one workgroup per mask: chunked prefix sum of its counts with a carry, a toggle at every cumulative
//                             position < H * W.
//   seg_toggles_fill_kernel   one workgroup per object: for each of its planes, the prefix XOR in the word (shifted XORs) and across
//                             words (a scan of the words' parities: wave ballot, then the waves through LDS, a carry between chunks),
//                             OR-ed over the object's planes (a COCO multi-polygon annotation is the union of its rings, rleMerge with
//                             intersect = 0).  A thread owns the words j = tid (mod kFillT) of the row, so the OR needs no atomics.
//   seg_unpack_masks_kernel   bits -> dense row-major [M, H, W] bytes (0 / 1): the inverse of seg_pack_masks_kernel, for training targets.
//
// Exactness: the polygon arithmetic is rleFrPoly's, IEEE double in its order, every product and sum rounded on its own (contraction
// into an FMA is switched off for this file).  XOR commutes, so the planes do not depend on the order the atomics arrive in: bitwise
// reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpf_common.h"

// rleFrPoly's doubles are rounded operation by operation.  HIP compiles device code with -ffp-contract=fast, and the __dmul_rn /
// __dadd_rn of its headers are plain operators that carry the headers' contraction flag into the caller, so the arithmetic below is
// written with plain operators under this pragma: no product here may join a sum in an FMA.
#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int kCodT = 256;                 // threads of the toggle and unpack kernels
constexpr int kStageEdges = 4;             // edges per thread and stage
constexpr int kStage = kCodT * kStageEdges;    // edges staged in LDS at a time (mpf_seg_poly_stage_edges reports it)
constexpr int kFillT = 1024;               // a row is filled by one workgroup: the widest one
constexpr int kFillWaves = kFillT / 64;

struct Edge {
    int xs, ys, xe, ye;                    // scaled integer ends, in the ring's direction
};

// rleFrPoly: x[j] = (int)(scale * xy[2j] + .5), scale = 5
__device__ __forceinline__ int scale5(double c) { return (int)(5.0 * c + 0.5); }

// edge j of a ring of K vertices whose first vertex is v0: from vertex j to vertex j + 1, the last one back to vertex 0
__device__ __forceinline__ Edge load_edge(const double* __restrict__ xy, int64_t v0, int64_t K, int64_t j)
{
    const int64_t a = v0 + j, b = v0 + (j + 1 == K ? 0 : j + 1);
    return Edge{scale5(xy[2 * a]), scale5(xy[2 * a + 1]), scale5(xy[2 * b]), scale5(xy[2 * b + 1])};
}

__device__ __forceinline__ int64_t abs64(int64_t v) { return v < 0 ? -v : v; }

// points of an edge: max(|dx|, |dy|) + 1 (a zero-length edge has one)
__device__ __forceinline__ int64_t edge_points(const Edge& e)
{
    const int64_t dx = abs64((int64_t)e.xe - e.xs), dy = abs64((int64_t)e.ys - e.ye);
    return (dx >= dy ? dx : dy) + 1;
}

// an edge as rleFrPoly walks it: ends swapped where it flips, the slope of the minor axis
struct Walk {
    int64_t xs, ys, dmax;
    double s;
    bool flip, xmajor;
};
__device__ __forceinline__ Walk walk_of(const Edge& e)
{
    int64_t xs = e.xs, ys = e.ys, xe = e.xe, ye = e.ye;
    const int64_t dx = abs64(xe - xs), dy = abs64(ys - ye);
    Walk w;
    w.xmajor = dx >= dy;
    w.flip = (w.xmajor && xs > xe) || (!w.xmajor && ys > ye);
    if (w.flip) {
        int64_t t = xs; xs = xe; xe = t;
        t = ys; ys = ye; ye = t;
    }
    w.xs = xs;
    w.ys = ys;
    w.dmax = w.xmajor ? dx : dy;
    // (0 / 0 on a zero-length edge is never used: its one point has u = xs, and point_v answers ys without the slope)
    w.s = w.dmax == 0 ? 0.0 : (w.xmajor ? (double)(ye - ys) / (double)dx : (double)(xe - xs) / (double)dy);
    return w;
}
// point d of the edge, counted from its original start: t = flip ? dmax - d : d
__device__ __forceinline__ int point_u(const Walk& w, int64_t d)
{
    const int64_t t = w.flip ? w.dmax - d : d;
    if (w.xmajor) return (int)(t + w.xs);
    return (int)((double)w.xs + w.s * (double)t + 0.5);
}
__device__ __forceinline__ int point_v(const Walk& w, int64_t d)
{
    const int64_t t = w.flip ? w.dmax - d : d;
    if (!w.xmajor) return (int)(t + w.ys);
    if (w.dmax == 0) return (int)w.ys;
    return (int)((double)w.ys + w.s * (double)t + 0.5);
}

// exclusive scan of one value per thread over the kCodT threads, in thread order -> (prefix of this thread, workgroup total)
__device__ __forceinline__ int64_t block_excl_scan64(int64_t v, int64_t& total)
{
    __shared__ int64_t wsum[kCodT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();                                         // (wsum may still be read from an earlier call)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int64_t base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kCodT / 64; ++i) {
        if (i < wave) base += wsum[i];
        total += wsum[i];
    }
    return base + inc - v;
}

__device__ __forceinline__ void toggle(u64* __restrict__ plane, int64_t p) { atomicXor(plane + (p >> 6), 1ull << (p & 63)); }

// the rule of rleFrPoly for the dense points (wp, dp) -> (wc, dc), consecutive in the ring
__device__ __forceinline__ void crossing(const Walk& wp, int64_t dp, const Walk& wc, int64_t dc, int H, int W, int64_t HW,
                                         u64* __restrict__ plane)
{
    const int uc = point_u(wc, dc), up = point_u(wp, dp);
    if (uc == up) return;
    // xd = (raw + .5) / 5 - .5 is an integer iff raw = 2 (mod 5); then xd = (raw - 2) / 5 exactly, and 0 <= xd needs raw >= 2
    const int64_t raw = uc < up ? (int64_t)uc : (int64_t)uc - 1;
    if (raw < 2 || raw % 5 != 2) return;
    const int64_t xd = (raw - 2) / 5;
    if (xd > W - 1) return;
    const int vc = point_v(wc, dc), vp = point_v(wp, dp);
    double yd = (double)(vc < vp ? vc : vp);
    yd = (yd + 0.5) / 5.0 - 0.5;
    if (yd < 0.0) yd = 0.0;
    else if (yd > (double)H) yd = (double)H;
    yd = ceil(yd);
    const int64_t p = xd * H + (int64_t)yd;
    if (p < HW) toggle(plane, p);
}

__global__ __launch_bounds__(kCodT) void seg_poly_toggles_kernel(const double* __restrict__ xy, const int64_t* __restrict__ ring_off, int H,
                                                                 int W, int64_t HW, int64_t nwords, u64* __restrict__ planes)
{
    __shared__ Edge edges[kStage];
    __shared__ int64_t pre[kStage + 1];                      // first dense point of every staged edge, then the stage's total
    const int64_t v0 = ring_off[blockIdx.x], K = ring_off[blockIdx.x + 1] - v0;
    if (K <= 0) return;                                      // (the whole workgroup)
    u64* plane = planes + (int64_t)blockIdx.x * nwords;
    for (int64_t e0 = 0; e0 < K; e0 += kStage) {
        const int n = (int)min((int64_t)kStage, K - e0);
        __syncthreads();                                     // the stage before has been walked
        int64_t len[kStageEdges], sum = 0;
#pragma unroll
        for (int q = 0; q < kStageEdges; ++q) {
            const int j = kStageEdges * threadIdx.x + q;
            len[q] = 0;
            if (j < n) {
                const Edge e = load_edge(xy, v0, K, e0 + j);
                edges[j] = e;
                len[q] = edge_points(e);
            }
            sum += len[q];
        }
        int64_t total;
        int64_t run = block_excl_scan64(sum, total);
#pragma unroll
        for (int q = 0; q < kStageEdges; ++q) {
            const int j = kStageEdges * threadIdx.x + q;
            if (j < n) pre[j] = run;
            run += len[q];
        }
        if (threadIdx.x == 0) pre[n] = total;
        __syncthreads();
        for (int64_t l = threadIdx.x; l < total; l += kCodT) {
            if (e0 == 0 && l == 0) continue;                 // the ring's first point has no predecessor
            int lo = 0, hi = n - 1;                          // the edge of point l: the last one with pre[j] <= l (pre is increasing)
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= l) lo = mid;
                else hi = mid - 1;
            }
            const int64_t d = l - pre[lo];
            const Walk wc = walk_of(edges[lo]);
            if (d > 0) {
                crossing(wc, d - 1, wc, d, H, W, HW, plane);
            } else {                                         // the predecessor is the last point of the edge before
                const Walk wp = walk_of(lo > 0 ? edges[lo - 1] : load_edge(xy, v0, K, e0 - 1));
                crossing(wp, wp.dmax, wc, 0, H, W, HW, plane);
            }
        }
    }
}

__global__ __launch_bounds__(kCodT) void seg_rle_toggles_kernel(const unsigned* __restrict__ counts, const int64_t* __restrict__ off, int64_t HW,
                                                                int64_t nwords, u64* __restrict__ planes)
{
    const int64_t c0 = off[blockIdx.x], n = off[blockIdx.x + 1] - c0;
    u64* plane = planes + (int64_t)blockIdx.x * nwords;
    int64_t carry = 0;
    for (int64_t i0 = 0; i0 < n; i0 += kCodT) {              // (n is the workgroup's: every thread makes every pass)
        const int64_t i = i0 + threadIdx.x;
        const int64_t v = i < n ? (int64_t)counts[c0 + i] : 0;
        int64_t total;
        const int64_t end = carry + block_excl_scan64(v, total) + v;     // where run i ends: the next run's first position
        if (i < n && end < HW) toggle(plane, end);
        carry += total;
    }
}

// the range of planes of object m: plane_obj is non-decreasing
__device__ __forceinline__ int first_plane_of(const int* __restrict__ plane_obj, int R, int m)
{
    int lo = 0, hi = R;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (plane_obj[mid] < m) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kFillT) void seg_toggles_fill_kernel(const u64* __restrict__ planes, const int* __restrict__ plane_obj, int R,
                                                                  int64_t HW, int64_t nwords, u64* __restrict__ bits)
{
    __shared__ unsigned wpar[kFillWaves];
    const int m = blockIdx.x;
    const int r0 = first_plane_of(plane_obj, R, m), r1 = first_plane_of(plane_obj, R, m + 1);
    u64* row = bits + (int64_t)m * nwords;
    if (r0 == r1) {                                          // an object without a plane
        for (int64_t j = threadIdx.x; j < nwords; j += kFillT) row[j] = 0ull;
        return;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int r = r0; r < r1; ++r) {
        const u64* src = planes + (int64_t)r * nwords;
        unsigned carry = 0;                                  // parity of the toggles before this chunk
        for (int64_t j0 = 0; j0 < nwords; j0 += kFillT) {
            const int64_t j = j0 + threadIdx.x;
            u64 x = j < nwords ? src[j] : 0ull;
            x ^= x << 1; x ^= x << 2; x ^= x << 4; x ^= x << 8; x ^= x << 16; x ^= x << 32;     // bit b: parity of the toggles at <= b
            const u64 odd = __ballot((int)(x >> 63));        // the words of this wave with an odd number of toggles
            const unsigned before = __popcll(odd & ((1ull << lane) - 1ull)) & 1u;
            __syncthreads();                                 // (wpar may still be read from the chunk before)
            if (lane == 0) wpar[wave] = __popcll(odd) & 1u;
            __syncthreads();
            unsigned waves_before = 0, chunk = 0;
#pragma unroll
            for (int i = 0; i < kFillWaves; ++i) {
                if (i < wave) waves_before ^= wpar[i];
                chunk ^= wpar[i];
            }
            if (carry ^ waves_before ^ before) x = ~x;
            carry ^= chunk;
            if (j < nwords) {
                const int64_t left = HW - j * 64;            // bits at and past H * W stay zero
                if (left < 64) x &= (1ull << left) - 1ull;
                row[j] = r == r0 ? x : (row[j] | x);         // this thread wrote row[j] for the plane before
            }
        }
    }
}

__global__ __launch_bounds__(kCodT) void seg_unpack_masks_kernel(const u64* __restrict__ bits, int H, int W, int64_t nwords,
                                                                 unsigned char* __restrict__ masks)
{
    const int64_t HW = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * kCodT + threadIdx.x;       // row-major output pixel
    if (i >= HW) return;
    const int y = (int)(i / W), x = (int)(i % W);
    const int64_t p = (int64_t)x * H + y;
    masks[(int64_t)blockIdx.y * HW + i] = (unsigned char)((bits[(int64_t)blockIdx.y * nwords + (p >> 6)] >> (p & 63)) & 1ull);
}

constexpr int kMaxPlanes = (1 << 24) - 1;

// the checks every entry point of this file shares: n >= 0 rows of an H x W image (who: the entry point without its mpf_ prefix)
int check_rows(const char* who, int n, int n_max, int H, int W)
{
    if (n < 0 || H <= 0 || W <= 0) return mpf::failf(MPF_E_SHAPE, who, "need a count >= 0 and H, W > 0");
    if ((int64_t)H * W >= (1ll << 31) || n > n_max) return mpf::failf(MPF_E_TOO_LARGE, who, "too large (H * W < 2^31, M <= 65535, R < 2^24)");
    return 0;
}
int64_t words_of(int H, int W) { return ((int64_t)H * W + 63) / 64; }

}  // namespace

extern "C" int mpf_seg_poly_stage_edges(void) { return kStage; }

extern "C" int mpf_seg_poly_toggles(const double* xy, const int64_t* ring_off, int R, int H, int W, uint64_t* planes, void* stream)
{
    if (int e = check_rows("seg_poly_toggles", R, kMaxPlanes, H, W)) return e;
    if (R == 0) return 0;
    if (!xy || !ring_off || !planes) return mpf::fail(MPF_E_NULL, "seg_poly_toggles: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, nwords = words_of(H, W);
    if (int e = mpf::check(hipMemsetAsync(planes, 0, (size_t)R * nwords * 8, st), "mpf_seg_poly_toggles (zero)")) return e;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_poly_toggles_kernel");
    hipLaunchKernelGGL(seg_poly_toggles_kernel, dim3((unsigned)R), dim3(kCodT), 0, st, xy, ring_off, H, W, HW, nwords, (u64*)planes);
    mpf::prof_end("seg_poly_toggles_kernel", st, 8.0 * (R + 1));
    return mpf::check(hipGetLastError(), "mpf_seg_poly_toggles");
}

extern "C" int mpf_seg_rle_toggles(const uint32_t* counts, const int64_t* off, int M, int H, int W, uint64_t* planes, void* stream)
{
    if (int e = check_rows("seg_rle_toggles", M, kMaxPlanes, H, W)) return e;
    if (M == 0) return 0;
    if (!counts || !off || !planes) return mpf::fail(MPF_E_NULL, "seg_rle_toggles: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, nwords = words_of(H, W);
    if (int e = mpf::check(hipMemsetAsync(planes, 0, (size_t)M * nwords * 8, st), "mpf_seg_rle_toggles (zero)")) return e;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_rle_toggles_kernel");
    hipLaunchKernelGGL(seg_rle_toggles_kernel, dim3((unsigned)M), dim3(kCodT), 0, st, (const unsigned*)counts, off, HW, nwords, (u64*)planes);
    mpf::prof_end("seg_rle_toggles_kernel", st, 8.0 * (M + 1));
    return mpf::check(hipGetLastError(), "mpf_seg_rle_toggles");
}

extern "C" int mpf_seg_toggles_fill(const uint64_t* planes, const int* plane_obj, int R, int M, int H, int W, uint64_t* bits, void* stream)
{
    if (int e = check_rows("seg_toggles_fill", M, 65535, H, W)) return e;
    if (int e = check_rows("seg_toggles_fill", R, kMaxPlanes, H, W)) return e;
    if (M == 0) return 0;
    if (!bits || (R > 0 && (!planes || !plane_obj))) return mpf::fail(MPF_E_NULL, "seg_toggles_fill: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, nwords = words_of(H, W);
    mpf::prof_begin(st);
    mpf::set_kernel("seg_toggles_fill_kernel");
    hipLaunchKernelGGL(seg_toggles_fill_kernel, dim3((unsigned)M), dim3(kFillT), 0, st, (const u64*)planes, plane_obj, R, HW, nwords, (u64*)bits);
    mpf::prof_end("seg_toggles_fill_kernel", st, 8.0 * nwords * ((double)R + M));
    return mpf::check(hipGetLastError(), "mpf_seg_toggles_fill");
}

extern "C" int mpf_seg_unpack_masks(const uint64_t* bits, int M, int H, int W, uint8_t* masks, void* stream)
{
    if (int e = check_rows("seg_unpack_masks", M, 65535, H, W)) return e;
    if (M == 0) return 0;
    if (!bits || !masks) return mpf::fail(MPF_E_NULL, "seg_unpack_masks: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, nwords = words_of(H, W);
    mpf::prof_begin(st);
    mpf::set_kernel("seg_unpack_masks_kernel");
    hipLaunchKernelGGL(seg_unpack_masks_kernel, dim3((unsigned)((HW + kCodT - 1) / kCodT), (unsigned)M), dim3(kCodT), 0, st, (const u64*)bits, H, W,
                       nwords, masks);
    mpf::prof_end("seg_unpack_masks_kernel", st, (double)M * (HW + 8.0 * nwords));
    return mpf::check(hipGetLastError(), "mpf_seg_unpack_masks");
}
