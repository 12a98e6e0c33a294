// Mask boundaries on packed bits for MI355X: boundary-iou-api's mask_to_boundary (the erosion the reference's
// tools/evaluate_coco_boundary_ap.py asks for with iouType="boundary"), on the packed masks of csrc/seg_ap.hip, without a dense mask.
//
//   eroded(y, x) = every pixel of the (2d+1) x (2d+1) square around (y, x) is set, pixels outside the image counting as unset
//   boundary     = mask & ~eroded
//
// Layout (seg_ap.hip): position p = x * H + y, bit b of word j = position 64 j + b.  y is the contiguous axis, a column is H
// consecutive bits that start on a word only where x * H % 64 == 0, and columns abut.
//
//   seg_boundary_kernel         one workgroup = one mask x one band of BW columns.  BW * H % 64 == 0, so a band owns whole output
//                               words and every word has one writer.  The band and a halo of d columns each side are unpacked into
//                               LDS COLUMN-ALIGNED: column c is tw = ceil(H / 64) words of its own, rows past H - 1 and columns
//                               outside the image zero.  A shift along y inside that image reads zeros past a column's last word
//                               (the index is tested), so no neighbouring column leaks in; the x window is an AND of whole words
//                               tw apart.  Both windows of length L = 2d + 1 are built FORWARD by doubling, r[q] &= r[q + s] for
//                               s = 1, 2, 4, ... and one remainder step, between two LDS buffers: O(log d) passes.  The result is
//                               the window that STARTS at (y, x); the output pass reads it at (y - d, x - d), re-packs it to the
//                               stream's alignment and writes in & ~eroded.
//                               Banking: a thread's word index runs along the column first, so the lanes of a wave read and write
//                               consecutive 8-byte slots in every pass (a shifted read is the same run moved by a constant): a
//                               32-lane half covers the 64 banks once, whatever tw is, and the image needs no padding.
//                               256 threads; 1024 where the image has 4096 words or more.
//   seg_boundary_direct_kernel  images whose band does not fit the LDS (tw * (2d + quantum) words, twice, above 160 KiB: beyond
//                               about 3000 x 4500 at ratio 0.02): one wave per output word, one lane per pixel, every set pixel
//                               tests the 2d + 1 column runs of its window in the stream.  O(d * d / 64) per pixel: correct, slow.
//   seg_boundary_copy_kernel    2d + 1 > min(H, W): no pixel has its whole window inside the image, boundary == mask.
//
// Integer and bit operations only, no atomics, no workgroup depends on another: bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "mpf_common.h"

namespace {

typedef unsigned long long u64;

constexpr int kBndT = 256;
constexpr int kBndTBig = 1024;                             // threads for a band of kBndBigWords words or more (a pass is latency-bound)
constexpr int kBndBigWords = 4096;
constexpr size_t kBndLdsMax = 160 * 1024;                  // one workgroup may take the whole LDS of a CU
constexpr int kBndWords = (int)(kBndLdsMax / 16);          // words of ONE of the two buffers

__device__ __forceinline__ u64 low_bits(int n)             // n in [0, 64]
{
    return n >= 64 ? ~0ull : ((1ull << n) - 1);
}

// 64 bits of column c of an LDS image starting at bit q of that column; bits before 0 or at / past 64 tw read zero
__device__ __forceinline__ u64 col_get(const u64* __restrict__ img, int c, int tw, int q)
{
    if (q <= -64 || q >= 64 * tw) return 0ull;
    const int iw = q >> 6, s = q & 63;                     // arithmetic shift: floor
    const u64* col = img + (size_t)c * tw;
    const u64 lo = iw >= 0 ? col[iw] : 0ull;
    if (s == 0) return lo;
    const u64 hi = iw + 1 < tw ? col[iw + 1] : 0ull;       // iw + 1 >= 0 here
    return (lo >> s) | (hi << (64 - s));
}

__global__ __launch_bounds__(kBndTBig) void seg_boundary_kernel(const u64* __restrict__ bits, int H, int W, int d, int64_t nwords, int BW,
                                                             int tw, u64* __restrict__ out)
{
    extern __shared__ u64 lds[];
    const int nc = BW + 2 * d, n = nc * tw, nt = blockDim.x;
    u64* cur = lds;
    u64* nxt = lds + n;
    const int x0 = blockIdx.x * BW;
    const u64* in = bits + (int64_t)blockIdx.y * nwords;
    u64* o = out + (int64_t)blockIdx.y * nwords;
    // unpack: column c = image column x0 - d + c, word i = rows 64 i .. 64 i + 63
    for (int idx = threadIdx.x; idx < n; idx += nt) {
        const int c = idx / tw, i = idx - c * tw;
        const int x = x0 - d + c;
        u64 v = 0ull;
        if (x >= 0 && x < W) {                              // 64 i < H always: tw = ceil(H / 64)
            const int64_t P = (int64_t)x * H + 64 * i;
            const int64_t j = P >> 6;
            const int s = (int)(P & 63);
            v = in[j] >> s;
            if (s && j + 1 < nwords) v |= in[j + 1] << (64 - s);
            v &= low_bits(H - 64 * i);                      // the next column's rows are not this column's
        }
        cur[idx] = v;
    }
    __syncthreads();
    const int L = 2 * d + 1;
    // y: r[q] = rows q .. q + L - 1 of the column all set
    for (int win = 1; win < L;) {
        const int s = 2 * win <= L ? win : L - win;
        for (int idx = threadIdx.x; idx < n; idx += nt) {
            const int c = idx / tw, i = idx - c * tw;
            nxt[idx] = cur[idx] & col_get(cur, c, tw, 64 * i + s);
        }
        __syncthreads();
        u64* t = cur; cur = nxt; nxt = t;
        win += s;
    }
    // x: r[c] = columns c .. c + L - 1 all set
    for (int win = 1; win < L;) {
        const int s = 2 * win <= L ? win : L - win;
        for (int idx = threadIdx.x; idx < n; idx += nt) {
            const int c = idx / tw;
            nxt[idx] = c + s < nc ? cur[idx] & cur[idx + s * tw] : 0ull;
        }
        __syncthreads();
        u64* t = cur; cur = nxt; nxt = t;
        win += s;
    }
    // re-pack: eroded(y, x) = r[column x - x0][row y - d]; the band's words are its own (BW * H % 64 == 0, or one band)
    const int64_t HW = (int64_t)H * W;
    const int64_t j0 = ((int64_t)x0 * H) >> 6;
    const int64_t j1 = x0 + BW >= W ? nwords : ((int64_t)(x0 + BW) * H) >> 6;
    for (int64_t j = j0 + threadIdx.x; j < j1; j += nt) {
        const int64_t P = 64 * j;
        int x = (int)(P / H), y = (int)(P - (int64_t)x * H);
        u64 er = 0ull;
        for (int b = 0; b < 64 && x < W;) {
            const int len = min(H - y, 64 - b);
            er |= (col_get(cur, x - x0, tw, y - d) & low_bits(len)) << b;
            b += len;
            ++x;
            y = 0;
        }
        u64 v = in[j] & ~er;
        if (HW - P < 64) v &= low_bits((int)(HW - P));
        o[j] = v;
    }
}

// the run of n bits from stream position P all set
__device__ __forceinline__ bool run_set(const u64* __restrict__ w, int64_t P, int n)
{
    const int64_t end = P + n;
    for (int64_t j = P >> 6; 64 * j < end; ++j) {
        u64 m = ~0ull;
        if (64 * j < P) m &= ~0ull << (int)(P - 64 * j);
        if (64 * (j + 1) > end) m &= ~0ull >> (int)(64 * (j + 1) - end);
        if ((w[j] & m) != m) return false;
    }
    return true;
}

// pixel p of the boundary, from the stream alone
__device__ __forceinline__ bool boundary_bit(const u64* __restrict__ in, int H, int W, int d, int64_t p)
{
    if (p >= (int64_t)H * W || !((in[p >> 6] >> (int)(p & 63)) & 1ull)) return false;
    const int x = (int)(p / H), y = (int)(p - (int64_t)x * H);
    if (x < d || x + d >= W || y < d || y + d >= H) return true;
    for (int k = -d; k <= d; ++k)
        if (!run_set(in, p + (int64_t)k * H - d, 2 * d + 1)) return true;
    return false;
}

__global__ __launch_bounds__(kBndT) void seg_boundary_direct_kernel(const u64* __restrict__ bits, int H, int W, int d, int64_t nwords,
                                                                    u64* __restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * (kBndT / 64) + (threadIdx.x >> 6);       // wave-uniform
    if (j >= nwords) return;
    const u64 v = __ballot(boundary_bit(bits + (int64_t)blockIdx.y * nwords, H, W, d, 64 * j + (threadIdx.x & 63)));
    if ((threadIdx.x & 63) == 0) out[(int64_t)blockIdx.y * nwords + j] = v;
}

__global__ __launch_bounds__(kBndT) void seg_boundary_copy_kernel(const u64* __restrict__ bits, int64_t HW, int64_t nwords,
                                                                  u64* __restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * kBndT + threadIdx.x;
    if (j >= nwords) return;
    u64 v = bits[(int64_t)blockIdx.y * nwords + j];
    if (HW - 64 * j < 64) v &= low_bits((int)(HW - 64 * j));
    out[(int64_t)blockIdx.y * nwords + j] = v;
}

}  // namespace

extern "C" int mpf_seg_mask_boundary(const uint64_t* bits, int M, int H, int W, int d, uint64_t* out, void* stream)
{
    if (M < 0 || H <= 0 || W <= 0 || d < 1) return mpf::fail(MPF_E_SHAPE, "seg_mask_boundary: need M >= 0 masks of H, W > 0 and d >= 1");
    if ((int64_t)H * W >= (1ll << 31) || M > 65535)
        return mpf::fail(MPF_E_TOO_LARGE, "seg_mask_boundary: too large (H * W < 2^31, M <= 65535)");
    if (M == 0) return 0;
    if (!bits || !out) return mpf::fail(MPF_E_NULL, "seg_mask_boundary: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W, nwords = (HW + 63) / 64;
    const double bytes = 16.0 * M * nwords;
    mpf::prof_begin(st);
    if (2 * (int64_t)d + 1 > std::min(H, W)) {              // no window fits the image: nothing is eroded
        mpf::set_kernel("seg_boundary_copy_kernel");
        hipLaunchKernelGGL(seg_boundary_copy_kernel, dim3((unsigned)((nwords + kBndT - 1) / kBndT), (unsigned)M), dim3(kBndT), 0, st,
                           (const u64*)bits, HW, nwords, (u64*)out);
        mpf::prof_end("seg_boundary_copy_kernel", st, bytes);
        return mpf::check(hipGetLastError(), "mpf_seg_mask_boundary");
    }
    // band: a multiple of the columns after which the stream is on a word again, about twice the halo, inside the LDS
    const int tw = (H + 63) / 64;
    int g = 64;
    while (H % g) g >>= 1;                                  // gcd(H, 64)
    const int quantum = 64 / g;
    const int room = kBndWords / tw - 2 * d;                // columns a band may have
    int BW = std::min((std::max(64, 4 * d) + quantum - 1) / quantum * quantum, room > 0 ? room / quantum * quantum : 0);
    if (BW >= W || (BW == 0 && room >= W)) BW = W;          // one band: its end is the stream's
    if (BW > 0) {
        static mpf::LdsAttr attr;
        if (int e = mpf::ensure_dynamic_lds((const void*)seg_boundary_kernel, kBndLdsMax, attr)) return e;
        const size_t lds = 16 * (size_t)tw * (size_t)(BW + 2 * d);
        mpf::set_kernel("seg_boundary_kernel");
        const int threads = tw * (BW + 2 * d) >= kBndBigWords ? kBndTBig : kBndT;
        hipLaunchKernelGGL(seg_boundary_kernel, dim3((unsigned)((W + BW - 1) / BW), (unsigned)M), dim3(threads), lds, st, (const u64*)bits,
                           H, W, d, nwords, BW, tw, (u64*)out);
        mpf::prof_end("seg_boundary_kernel", st, bytes);
    } else {
        mpf::set_kernel("seg_boundary_direct_kernel");
        hipLaunchKernelGGL(seg_boundary_direct_kernel, dim3((unsigned)((nwords + kBndT / 64 - 1) / (kBndT / 64)), (unsigned)M), dim3(kBndT),
                           0, st, (const u64*)bits, H, W, d, nwords, (u64*)out);
        mpf::prof_end("seg_boundary_direct_kernel", st, bytes);
    }
    return mpf::check(hipGetLastError(), "mpf_seg_mask_boundary");
}
