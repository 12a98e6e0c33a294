// Training input on MI355X: the image half of large-scale jitter (flip, resize, fixed crop, pad) as ONE launch for a batch of decoded
// uint8 HWC images, with the values of PIL's 8-bit bilinear resize (ImagingResample, triangle filter) — what detectron2's
// ResizeTransform.apply_image gives for uint8 — and optionally the model's normalisation and size-divisibility canvas on top.
//
// PIL's resample is integer arithmetic once its coefficients are known: per axis and output index a first source index, a tap count
// and int32 weights k = (int)(0.5 + w * 2^22); a pass is clip(((1 << 21) + sum pixel * k) >> 22, 0, 255); the horizontal pass runs
// first and is rounded to uint8, the vertical pass reads those bytes.  The host computes the tables in double as PIL does, for the
// columns and rows of the CROP WINDOW only, and the kernel never forms the resized image: at scale 2.0 three quarters of it would be
// thrown away.  A pass whose size does not change has the coefficients (2^22, 0) and is the identity by the same formula.
//
//   img_resample_kernel   one workgroup per (image, output tile of tile_h x kTileW of the canvas).  Horizontal pass: for the source
//                         rows the tile's output rows tap (at most kSpanRows: the host picks tile_h per image so that this holds)
//                         and the tile's valid columns, three channels per thread, from the HWC source (read mirrored with the flip
//                         flag: equal to PIL on the flipped image; with flip_out the valid columns take the tables of their mirror
//                         column instead: the crop of the resize, flipped, which reads another window of the source than the crop
//                         of the flipped resize unless the crop is centred) into LDS as uint8 [row][channel][kTileW].  Vertical pass out of
//                         LDS, lanes along the output row, into the three channel planes of [B, 3, Hc, Wc]: the value inside the
//                         valid extent, the pad value in the rest of the crop rectangle, zero in the rest of the canvas; as uint8,
//                         as (v - mean[c]) / std[c] in fp32 (IEEE subtraction and division: bit-equal to torch's), or that rounded to
//                         bf16 (nearest even).
//
// LDS: kSpanRows * 3 * kTileW = 48 KiB per workgroup (three workgroups per CU).  Reads of a wave are kTileW consecutive bytes (16
// dwords, four lanes per dword: broadcast, no bank conflict).  Every tap range is checked on the host copy of the tables before the
// launch, so no index read from device memory can leave the source image or the LDS buffer.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mpf_common.h"

// (v - mean) / std must round as torch's two fp32 operations do: nothing here may be contracted or replaced by a reciprocal
#pragma clang fp contract(off)

namespace {

constexpr int kResT = 256;                 // threads per workgroup
constexpr int kTileW = 64;                 // output columns per tile: one wave per output row segment
constexpr int kSpanRows = 256;             // source rows of one tile held in LDS
constexpr int kMaxTileH = 32;
constexpr int kMaxRatio = 64;              // source size / resized size, per axis

typedef MpfResampleRecord Rec;

struct Norm {
    float mean[3], std[3];
};

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ unsigned short bf16_rne(float f)
{
    const unsigned u = __float_as_uint(f);                   // (finite by construction: no NaN case)
    return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <int kDtype>
__global__ __launch_bounds__(kResT) void img_resample_kernel(const Rec* __restrict__ recs, const int* __restrict__ tab, void* __restrict__ out,
                                                             int Hc, int Wc, int pad_value, Norm nm)
{
    __shared__ unsigned char hbuf[kSpanRows * 3 * kTileW];
    const Rec r = recs[blockIdx.z];
    const int th = r.tile_h;
    const int oy0 = blockIdx.y * th, ox0 = blockIdx.x * kTileW;
    if (oy0 >= Hc) return;                                   // (the whole workgroup: the grid is sized for the smallest tile_h of the batch)
    const int rows = min(th, Hc - oy0), cols = min(kTileW, Wc - ox0);
    const int nvr = max(0, min(rows, r.valid_h - oy0)), nvc = max(0, min(cols, r.valid_w - ox0));
    const int* __restrict__ xk = tab + r.xk_off;
    const int* __restrict__ xb = tab + r.xb_off;
    const int* __restrict__ yk = tab + r.yk_off;
    const int* __restrict__ yb = tab + r.yb_off;
    int r_lo = 0;
    if (nvr > 0 && nvc > 0) {
        r_lo = yb[2 * oy0];
        const int span = yb[2 * (oy0 + nvr - 1)] + yb[2 * (oy0 + nvr - 1) + 1] - r_lo;     // <= kSpanRows: checked by the entry point
        const unsigned char* __restrict__ src = (const unsigned char*)r.src;
        for (int i = threadIdx.x; i < span * nvc; i += kResT) {
            const int s = i / nvc, j = i - s * nvc;
            const int tx = r.flip_out ? r.valid_w - 1 - (ox0 + j) : ox0 + j;       // the table column: mirrored inside the valid extent
            const int x0 = xb[2 * tx], n = xb[2 * tx + 1];
            const int* __restrict__ k = xk + (int64_t)tx * r.ksize_x;
            const unsigned char* __restrict__ row = src + (int64_t)(r_lo + s) * r.src_stride;
            int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
            for (int t = 0; t < n; ++t) {
                const int x = r.flip ? r.src_w - 1 - (x0 + t) : x0 + t;
                const int kk = k[t];
                a0 += (int)row[3 * x] * kk;
                a1 += (int)row[3 * x + 1] * kk;
                a2 += (int)row[3 * x + 2] * kk;
            }
            unsigned char* h = hbuf + s * (3 * kTileW) + j;
            h[0] = (unsigned char)clip8(a0 >> 22);
            h[kTileW] = (unsigned char)clip8(a1 >> 22);
            h[2 * kTileW] = (unsigned char)clip8(a2 >> 22);
        }
    }
    __syncthreads();
    const int64_t plane = (int64_t)Hc * Wc;
    const int j = threadIdx.x & (kTileW - 1);
    if (j >= cols) return;
    for (int q = threadIdx.x / kTileW; q < rows * 3; q += kResT / kTileW) {      // (row, channel) pairs: one per wave and pass
        const int yl = q / 3, c = q - 3 * yl;
        const int oy = oy0 + yl, ox = ox0 + j;
        const bool in_crop = oy < r.crop_h && ox < r.crop_w;
        int v = pad_value;
        if (yl < nvr && j < nvc) {
            const int y0 = yb[2 * oy] - r_lo, n = yb[2 * oy + 1];
            const int* __restrict__ k = yk + (int64_t)oy * r.ksize_y;
            const unsigned char* h = hbuf + (y0 * 3 + c) * kTileW + j;
            int a = 1 << 21;
            for (int t = 0; t < n; ++t) a += (int)h[t * (3 * kTileW)] * k[t];
            v = clip8(a >> 22);
        }
        const int64_t o = ((int64_t)blockIdx.z * 3 + c) * plane + (int64_t)oy * Wc + ox;
        if (kDtype == MPF_U8) {
            ((unsigned char*)out)[o] = in_crop ? (unsigned char)v : (unsigned char)0;
        } else {
            const float f = in_crop ? ((float)v - nm.mean[c]) / nm.std[c] : 0.0f;
            if (kDtype == MPF_F32) ((float*)out)[o] = f;
            else ((unsigned short*)out)[o] = bf16_rne(f);
        }
    }
}

int bad(const char* what) { return mpf::failf(MPF_E_SHAPE, "img_resample", what); }

// one axis of one record against the host copy of the tables: n outputs tapping a source of `in` entries
int check_axis(const int* tab, int64_t tab_len, int k_off, int b_off, int ksize, int n, int in)
{
    if (ksize < 1 || ksize > 2 * kMaxRatio + 1) return bad("taps per output outside 1 .. 129 (a ratio above 64)");
    if (k_off < 0 || b_off < 0 || (int64_t)k_off + (int64_t)n * ksize > tab_len || (int64_t)b_off + 2 * (int64_t)n > tab_len)
        return bad("a coefficient table lies outside the table buffer");
    int first_before = 0, end_before = 0;
    for (int i = 0; i < n; ++i) {
        const int first = tab[b_off + 2 * i], count = tab[b_off + 2 * i + 1];
        if (first < 0 || count < 0 || count > ksize || first + count > in) return bad("a tap range leaves the source image");
        if (first < first_before || first + count < end_before) return bad("tap ranges must not move backwards");
        first_before = first;
        end_before = first + count;
    }
    return 0;
}

int check_record(const Rec& r, const int* tab, int64_t tab_len, int Hc, int Wc)
{
    if (!r.src) return mpf::fail(MPF_E_NULL, "img_resample: NULL source image");
    if (r.src_h <= 0 || r.src_w <= 0 || r.out_h <= 0 || r.out_w <= 0 || r.crop_h <= 0 || r.crop_w <= 0) return bad("sizes must be positive");
    if (r.src_stride < 3 * (int64_t)r.src_w) return bad("row stride below 3 * W");
    if ((int64_t)r.src_stride * r.src_h >= (1ll << 31)) return mpf::failf(MPF_E_TOO_LARGE, "img_resample", "source image of 2^31 bytes or more");
    if ((int64_t)r.src_h > (int64_t)kMaxRatio * r.out_h || (int64_t)r.src_w > (int64_t)kMaxRatio * r.out_w)
        return bad("source / resized size above 64 on an axis");
    if (r.crop_h > Hc || r.crop_w > Wc) return bad("canvas smaller than the crop");
    if (r.off_y < 0 || r.off_x < 0 || r.valid_h < 1 || r.valid_w < 1 || r.valid_h > r.crop_h || r.valid_w > r.crop_w ||
        r.off_y + r.valid_h > r.out_h || r.off_x + r.valid_w > r.out_w)
        return bad("the valid extent must lie inside the crop and the resized image");
    if (r.tile_h < 1 || r.tile_h > kMaxTileH) return bad("tile_h outside 1 .. 32");
    if (r.flip_out < 0 || r.flip_out > 1) return bad("flip_out must be 0 or 1");
    if (int e = check_axis(tab, tab_len, r.xk_off, r.xb_off, r.ksize_x, r.valid_w, r.src_w)) return e;
    if (int e = check_axis(tab, tab_len, r.yk_off, r.yb_off, r.ksize_y, r.valid_h, r.src_h)) return e;
    for (int y0 = 0; y0 < r.valid_h; y0 += r.tile_h) {       // (tap ranges do not move backwards: the last row of a tile ends last)
        const int y1 = (y0 + r.tile_h < r.valid_h ? y0 + r.tile_h : r.valid_h) - 1;
        if (tab[r.yb_off + 2 * y1] + tab[r.yb_off + 2 * y1 + 1] - tab[r.yb_off + 2 * y0] > kSpanRows)
            return bad("a tile taps more than 256 source rows: tile_h too large for this ratio");
    }
    return 0;
}

}  // namespace

extern "C" int mpf_img_resample_ksize(int in_size, int out_size)
{
    if (in_size <= 0 || out_size <= 0) return 0;
    const double scale = (double)in_size / out_size;
    return (int)ceil(scale < 1.0 ? 1.0 : scale) * 2 + 1;
}

// PIL's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter, for the outputs first .. first + count of one axis: host
// code, IEEE double in PIL's order (this file compiles without contraction), written straight into the caller's staging buffer
extern "C" int mpf_img_resample_tables(int in_size, int out_size, int first, int count, int32_t* coef, int32_t* bounds)
{
    if (in_size <= 0 || out_size <= 0 || first < 0 || count < 0 || (int64_t)first + count > out_size)
        return bad("tables: need sizes > 0 and 0 <= first <= first + count <= out_size");
    if ((int64_t)in_size > (int64_t)kMaxRatio * out_size) return bad("source / resized size above 64 on an axis");
    if (count == 0) return 0;
    if (!coef || !bounds) return mpf::fail(MPF_E_NULL, "img_resample_tables: NULL buffer");
    const double scale = (double)in_size / out_size, fs = scale < 1.0 ? 1.0 : scale, support = fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    double w[2 * kMaxRatio + 1];
    for (int i = 0; i < count; ++i) {
        const double center = (first + i + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double v = (x + xmin - center + 0.5) / fs;
            if (v < 0.0) v = -v;
            w[x] = v < 1.0 ? 1.0 - v : 0.0;
            ww += w[x];
        }
        int32_t* k = coef + (int64_t)i * ksize;
        for (int x = 0; x < ksize; ++x) k[x] = x < xmax ? (int32_t)(0.5 + (ww != 0.0 ? w[x] / ww : w[x]) * (double)(1 << 22)) : 0;
        bounds[2 * i] = xmin;
        bounds[2 * i + 1] = xmax;
    }
    return 0;
}

extern "C" int mpf_img_resample_span_rows(void) { return kSpanRows; }
extern "C" int mpf_img_resample_max_ratio(void) { return kMaxRatio; }

extern "C" int mpf_img_resample(const MpfResampleRecord* recs_host, const MpfResampleRecord* recs_dev, const int32_t* tab_host,
                                const int32_t* tab_dev, int64_t tab_len, int B, void* out, int dtype, int Hc, int Wc, int pad_value,
                                const float* mean, const float* std, void* stream)
{
    if (B < 0 || Hc <= 0 || Wc <= 0 || tab_len < 0) return bad("need B >= 0, a canvas Hc, Wc > 0 and tab_len >= 0");
    if (B == 0) return 0;
    if (!recs_host || !recs_dev || !tab_host || !tab_dev || !out) return mpf::fail(MPF_E_NULL, "img_resample: NULL buffer");
    if (dtype != MPF_U8 && dtype != MPF_F32 && dtype != MPF_BF16) return mpf::fail(MPF_E_DTYPE, "img_resample: output must be uint8, float32 or bfloat16");
    if (dtype != MPF_U8 && (!mean || !std)) return mpf::fail(MPF_E_NULL, "img_resample: float output needs mean and std");
    if (pad_value < 0 || pad_value > 255) return bad("pad value outside 0 .. 255");
    if (B > 65535) return mpf::failf(MPF_E_TOO_LARGE, "img_resample", "B <= 65535 images");
    int min_tile = kMaxTileH;
    for (int b = 0; b < B; ++b) {
        if (int e = check_record(recs_host[b], tab_host, tab_len, Hc, Wc)) return e;
        if (recs_host[b].tile_h < min_tile) min_tile = recs_host[b].tile_h;
    }
    Norm nm = {};
    for (int c = 0; c < 3; ++c) {
        nm.mean[c] = mean ? mean[c] : 0.0f;
        nm.std[c] = std ? std[c] : 1.0f;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((Wc + kTileW - 1) / kTileW), (unsigned)((Hc + min_tile - 1) / min_tile), (unsigned)B);
    if (grid.y > 65535) return mpf::failf(MPF_E_TOO_LARGE, "img_resample", "more than 65535 row tiles");
    mpf::prof_begin(st);
    mpf::set_kernel("img_resample_kernel");
    mpf::with_int_of<MPF_U8, MPF_F32, MPF_BF16>(dtype, [&](auto dt) {
        hipLaunchKernelGGL(img_resample_kernel<decltype(dt)::value>, grid, dim3(kResT), 0, st, recs_dev, (const int*)tab_dev, out, Hc, Wc, pad_value, nm);
    });
    const double esz = dtype == MPF_U8 ? 1.0 : (dtype == MPF_F32 ? 4.0 : 2.0);
    mpf::prof_end("img_resample_kernel", st, (double)B * 3.0 * Hc * Wc * esz);
    return mpf::check(hipGetLastError(), "mpf_img_resample");
}
