// What the per-pixel inference kernels of seg_infer.hip (images) and seg_video.hip (clips) share: the composed resampling of one
// output pixel from the low-resolution mask logits, the run-length passes over packed mask bits, and the argument checks and
// launches of both.  Everything sits in an unnamed namespace: each of the two files compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <type_traits>

#include "mpf_common.h"

namespace {

constexpr int kT = 256;            // threads per workgroup, every kernel
constexpr int kInstPix = 1024;     // instance: output pixels per workgroup

__device__ __forceinline__ float ldm(const float* p, int64_t i) { return p[i]; }
__device__ __forceinline__ float ldm(const __hip_bfloat16* p, int64_t i) { return __bfloat162float(p[i]); }

// torch upsample_bilinear2d, align_corners=False, no explicit scale: scale = in / out in fp32,
// src = max(scale * (dst + 0.5) - 0.5, 0), i0 = (int)src, i1 = i0 + (i0 < in - 1), l1 = src - i0, l0 = 1 - l1.
// (__fmul_rn / __fadd_rn: no contraction into an FMA, the same roundings as the reference's separate operations)
struct Tap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Tap tap(int dst, int in, int out)
{
    const float scale = (float)in / (float)out;
    float src = __fsub_rn(__fmul_rn(scale, __fadd_rn((float)dst, 0.5f)), 0.5f);
    src = src < 0.f ? 0.f : src;
    Tap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    t.l1 = __fsub_rn(src, (float)t.i0);
    t.l0 = __fsub_rn(1.f, t.l1);
    return t;
}

// The composed geometry of one output pixel: stage 2 (crop [hi, wi] of the padded grid -> [H, W]) picks 2 x 2 intermediate
// pixels, stage 1 ([h, w] -> [Hp, Wp]) resamples each of them from a 2 x 2 low-resolution neighbourhood.
struct PixGeom {
    int64_t off[2][2][4];          // [intermediate row a][intermediate col b][low-res tap r*2+c]
    float w1[2][2][4];
    float w2y[2], w2x[2];
};
// One view: Q logit planes [h, w] (stride_q elements apart) of a padded [Hp, Wp] grid whose [hi, wi] crop is the image, resized to
// the [H, W] output.  check_geom fills it; every per-pixel kernel takes it by value.
struct SegGeom {
    int64_t stride_q;
    int Q, h, w, Hp, Wp, hi, wi, H, W;
};
__device__ __forceinline__ void pix_geom(PixGeom& g, int y, int x, const SegGeom& s)
{
    const int h = s.h, w = s.w, Hp = s.Hp, Wp = s.Wp;
    const Tap ty = tap(y, s.hi, s.H), tx = tap(x, s.wi, s.W);
    g.w2y[0] = ty.l0; g.w2y[1] = ty.l1;
    g.w2x[0] = tx.l0; g.w2x[1] = tx.l1;
    const int ya[2] = {ty.i0, ty.i1}, xa[2] = {tx.i0, tx.i1};
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const Tap sy = tap(ya[a], h, Hp);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const Tap sx = tap(xa[b], w, Wp);
            g.off[a][b][0] = (int64_t)sy.i0 * w + sx.i0;
            g.off[a][b][1] = (int64_t)sy.i0 * w + sx.i1;
            g.off[a][b][2] = (int64_t)sy.i1 * w + sx.i0;
            g.off[a][b][3] = (int64_t)sy.i1 * w + sx.i1;
            g.w1[a][b][0] = sy.l0; g.w1[a][b][1] = sy.l1;    // row weights (h0lambda, h1lambda)
            g.w1[a][b][2] = sx.l0; g.w1[a][b][3] = sx.l1;    // column weights (w0lambda, w1lambda)
        }
    }
}

// torch's weight order at each stage: h0l * (w0l * x00 + w1l * x01) + h1l * (w0l * x10 + w1l * x11)
__device__ __forceinline__ float lerp2(float h0, float h1, float w0, float w1, float x00, float x01, float x10, float x11)
{
    return __fadd_rn(__fmul_rn(h0, __fadd_rn(__fmul_rn(w0, x00), __fmul_rn(w1, x01))),
                     __fmul_rn(h1, __fadd_rn(__fmul_rn(w0, x10), __fmul_rn(w1, x11))));
}

template <typename T>
__device__ __forceinline__ float resample(const T* m, const PixGeom& g)
{
    float v[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float* wt = g.w1[a][b];
            v[a][b] = lerp2(wt[0], wt[1], wt[2], wt[3], ldm(m, g.off[a][b][0]), ldm(m, g.off[a][b][1]), ldm(m, g.off[a][b][2]),
                            ldm(m, g.off[a][b][3]));
        }
    return lerp2(g.w2y[0], g.w2y[1], g.w2x[0], g.w2x[1], v[0][0], v[0][1], v[1][0], v[1][1]);
}

// ----------------------------------------------------------------------------------------------------------------
// masks as uncompressed COCO run lengths, from packed bits.  Position p = x * H + y (the mask flattened column-major), 64 positions
// per word, bits at or past H * W zero.  A boundary is a position whose bit differs from its predecessor's, with bit[-1] = 0:
// the counts of a mask are the differences of {0, boundaries ..., H * W}, so they start with a (possibly empty) run of zeros.
//   seg_rle_count_kernel    boundaries per tile of kRleWords words (one word per thread), from the packed bits
//   seg_rle_scan_kernel     ONE workgroup: exclusive scan of the tile counts in (entry, tile) order, + 1 end mark per entry
//                           -> first packed slot of every tile (int64) and the per-entry offsets [T + 1]
//   seg_rle_scatter_kernel  the boundary positions (and H * W as the end mark) to their slots: rank = tile start + a fixed-order
//                           scan inside the workgroup, no atomics
//   seg_rle_diff_kernel     counts[i] = pos[i] - pos[i - 1] (0 before the first slot of an entry: the slot after an end mark)
// ----------------------------------------------------------------------------------------------------------------
constexpr int kRleWords = kT;      // words (64 positions each) per tile of the count / scatter kernels

// the boundary mask of word j of one entry (bits beyond H * W are 0 in the packed words and are masked out here)
__device__ __forceinline__ unsigned long long rle_boundaries(const unsigned long long* __restrict__ row, int64_t j, int64_t HW)
{
    const unsigned long long wd = row[j];
    const unsigned long long prev = j > 0 ? row[j - 1] >> 63 : 0ull;
    unsigned long long s = wd ^ ((wd << 1) | prev);
    const int64_t left = HW - j * 64;
    if (left < 64) s &= (1ull << left) - 1ull;
    return s;
}

// inclusive scan of one int per thread over the workgroup, in thread order -> (exclusive prefix of this thread, workgroup total)
__device__ __forceinline__ int block_excl_scan(int v, int& total)
{
    __shared__ int wsum[kT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(inc, o);
        if (lane >= o) inc += u;
    }
    __syncthreads();                                         // (wsum may still be read from an earlier call)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < kT / 64; ++i) {
        if (i < wave) base += wsum[i];
        total += wsum[i];
    }
    return base + inc - v;
}

__global__ __launch_bounds__(kT) void seg_rle_count_kernel(const unsigned long long* __restrict__ bits, int64_t nwords, int64_t HW,
                                                           int* __restrict__ tile_cnt)
{
    const int t = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * kRleWords + threadIdx.x;
    int c = 0;
    if (j < nwords) c = __popcll(rle_boundaries(bits + t * nwords, j, HW));
    int total;
    block_excl_scan(c, total);
    if (threadIdx.x == 0) tile_cnt[(int64_t)t * gridDim.x + blockIdx.x] = total;
}

__global__ __launch_bounds__(kT) void seg_rle_scan_kernel(const int* __restrict__ tile_cnt, int tiles, int T, int64_t* __restrict__ tile_off,
                                                          int64_t* __restrict__ offsets)
{
    __shared__ int64_t part[kT];
    const int64_t n = (int64_t)T * tiles;
    const int64_t per = (n + kT - 1) / kT;
    const int64_t lo = min(n, per * threadIdx.x), hi = min(n, lo + per);
    int64_t s = 0;
    for (int64_t i = lo; i < hi; ++i) s += tile_cnt[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {                                   // 256 partial sums: serial, fixed order
        int64_t run = 0;
        for (int i = 0; i < kT; ++i) {
            const int64_t v = part[i];
            part[i] = run;
            run += v;
        }
        offsets[T] = run + T;
    }
    __syncthreads();
    int64_t run = part[threadIdx.x];
    for (int64_t i = lo; i < hi; ++i) {
        const int64_t t = i / tiles;
        const int64_t off = run + t;                          // + one end mark for every earlier entry
        tile_off[i] = off;
        if (i % tiles == 0) offsets[t] = off;
        run += tile_cnt[i];
    }
}

__global__ __launch_bounds__(kT) void seg_rle_scatter_kernel(const unsigned long long* __restrict__ bits, int64_t nwords, int64_t HW,
                                                             const int64_t* __restrict__ tile_off, const int64_t* __restrict__ offsets,
                                                             int64_t cap, unsigned* __restrict__ pos)
{
    const int t = blockIdx.y;
    const int64_t j = (int64_t)blockIdx.x * kRleWords + threadIdx.x;
    unsigned long long s = 0ull;
    if (j < nwords) s = rle_boundaries(bits + t * nwords, j, HW);
    int total;
    int64_t slot = tile_off[(int64_t)t * gridDim.x + blockIdx.x] + block_excl_scan(__popcll(s), total);
    while (s) {
        const int k = __ffsll((long long)s) - 1;
        if (slot < cap) pos[slot] = (unsigned)(j * 64 + k);      // (cap: the caller's total; never short when it read offsets[T])
        ++slot;
        s &= s - 1ull;
    }
    if (j == nwords - 1 && offsets[t + 1] <= cap) pos[offsets[t + 1] - 1] = (unsigned)HW;
}

__global__ __launch_bounds__(kT) void seg_rle_diff_kernel(const unsigned* __restrict__ pos, const int64_t* __restrict__ total_p, int64_t cap,
                                                          unsigned HW, unsigned* __restrict__ counts)
{
    const int64_t total = min(*total_p, cap);
    for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < total; i += (int64_t)gridDim.x * kT) {
        const unsigned before = i > 0 ? pos[i - 1] : HW;
        counts[i] = pos[i] - (before == HW ? 0u : before);
    }
}

// ---- host side: argument checks and launches that several entry points share -------------------------------------------------------
// records "<who>: <what>" as the error (who = the entry point without its mpf_ prefix, as in every message of these files)
int fail_who(int code, const char* who, const char* what)
{
    char msg[200];
    snprintf(msg, sizeof msg, "%s: %s", who, what);
    return mpf::fail(code, msg);
}

// the twelve leading arguments of the per-pixel entry points, checked and gathered into g
int check_geom(const char* who, const void* masks, int64_t stride_q, int dtype, int Q, int h, int w, int Hp, int Wp, int hi, int wi,
               int H, int W, SegGeom& g)
{
    if (!masks) return fail_who(MPF_E_NULL, who, "NULL mask logits");
    if (dtype != MPF_F32 && dtype != MPF_BF16) return fail_who(MPF_E_DTYPE, who, "mask logits must be f32 or bf16 (dtype)");
    if (Q <= 0 || h <= 0 || w <= 0 || Hp <= 0 || Wp <= 0 || hi <= 0 || wi <= 0 || H <= 0 || W <= 0 || hi > Hp || wi > Wp ||
        stride_q < (int64_t)h * w) {
        char what[160];
        snprintf(what, sizeof what, "bad sizes (Q %d, low-res %dx%d, padded %dx%d, image %dx%d, output %dx%d, stride_q %lld)", Q, h, w, Hp,
                 Wp, hi, wi, H, W, (long long)stride_q);
        return fail_who(MPF_E_SHAPE, who, what);
    }
    if ((int64_t)H * W >= (1ll << 31) || (int64_t)Q * stride_q >= (1ll << 40)) return fail_who(MPF_E_TOO_LARGE, who, "output too large");
    g = SegGeom{stride_q, Q, h, w, Hp, Wp, hi, wi, H, W};
    return 0;
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// bytes of n [h, w] planes of mask logits: what a per-pixel kernel reads
double logit_bytes(double n, const SegGeom& g, int dtype) { return n * g.h * g.w * (dtype == MPF_F32 ? 4 : 2); }

// f(masks as const T*) with T = the type of the mask logits; elem_t<decltype(pointer)> names T inside f
template <typename F>
void with_mask_type(int dtype, const void* masks, F&& f)
{
    if (dtype == MPF_F32) f((const float*)masks);
    else f((const __hip_bfloat16*)masks);
}
template <typename P>
using elem_t = std::remove_cv_t<std::remove_pointer_t<P>>;

// the count and scan passes over bits [M, nwords] (M masks of HW positions, tiles = ceil(nwords / kRleWords)):
// tile_cnt int32 [M * tiles] and tile_off int64 [M * tiles] are workspace, offsets int64 [M + 1] the result
void launch_rle_count_scan(const unsigned long long* bits, int M, int64_t nwords, int64_t tiles, int64_t HW, int* tile_cnt, int64_t* tile_off,
                           int64_t* offsets, hipStream_t st)
{
    hipLaunchKernelGGL(seg_rle_count_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kT), 0, st, bits, nwords, HW, tile_cnt);
    hipLaunchKernelGGL(seg_rle_scan_kernel, dim3(1), dim3(kT), 0, st, (const int*)tile_cnt, (int)tiles, M, tile_off, offsets);
}

// the scatter and difference passes: counts uint32 [total] from the same bits and the tile_off / offsets of launch_rle_count_scan
void launch_rle_write(const unsigned long long* bits, int M, int64_t nwords, int64_t tiles, int64_t HW, const int64_t* tile_off,
                      const int64_t* offsets, int64_t total, unsigned* pos, unsigned* counts, hipStream_t st)
{
    hipLaunchKernelGGL(seg_rle_scatter_kernel, dim3((unsigned)tiles, (unsigned)M), dim3(kT), 0, st, bits, nwords, HW, tile_off, offsets, total,
                       pos);
    const unsigned gdiff = (unsigned)std::min<int64_t>((total + kT - 1) / kT, 8 * mpf::cu_count());
    hipLaunchKernelGGL(seg_rle_diff_kernel, dim3(gdiff), dim3(kT), 0, st, (const unsigned*)pos, offsets + M, total, (unsigned)HW, counts);
}

}  // namespace
