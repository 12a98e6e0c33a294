// Video training input on MI355X: the TARGET half of the reference's YTVISDatasetMapper (mask2former_video/data_video/
// dataset_mapper.py:239-267) and of prepare_targets (video_maskformer_model.py:227-253).  Per sampled frame and instance the mapper
// decodes the RLE to a dense mask, resizes it with PIL's nearest rule, flips it, and the model copies it into a zeroed
// [G, F, H_pad, W_pad] tensor.  Here a plane is one (tube, frame) of any clip of the batch and stays PACKED (mpf_seg_pack_masks'
// layout: position p = x Hs + y, 64 per word, as inference.rle_bits / polygon_bits leave it) until this one launch writes it, resized,
// flipped and padded, into its place of the tube store.  Every result is an integer.
//
//   mask_bits_resample_kernel   a workgroup owns a kTile x kTile tile of one plane.  The source is column-major bits, the result
//                               row-major bytes: the tile is transposed through 64-bit words.  Pass 1: a wave takes every fourth
//                               column of the tile and a lane is an output row; the lane reads its source bit through the two
//                               host-made tables (the nearest rule: the rows of a wave read neighbouring bits of ONE source column,
//                               a few words), a ballot gives the column's 64 rows as one word, which goes to LDS, its popcount to
//                               the plane's area.  Pass 2: a thread takes one row and 16 columns of the tile, picks its bit out of
//                               the 16 words (4 distinct LDS addresses per wave and step: broadcasts) and stores 16 bytes at once
//                               where the canvas width keeps the address aligned, in 4-byte or 1-byte pieces otherwise.  The whole
//                               canvas is written: 0 outside the valid rectangle, so the output needs no memset.  One writer per
//                               byte; the areas are integer sums (LDS, then one atomic per workgroup): independent of order.
//
// LDS: kTile words + the area = 520 B.  Every record and table entry is checked on the host copy before the launch, so no index
// read on the device leaves a source mask.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "mpf_common.h"

namespace {

constexpr int kT = 256;                    // threads per workgroup: 4 waves
constexpr int kTile = 64;                  // output rows and columns of a tile: a ballot is a column of it
constexpr int kSeg = 16;                   // output bytes a thread assembles in pass 2

typedef MpfMaskBitsRecord Rec;

__global__ __launch_bounds__(kT) void mask_bits_resample_kernel(const Rec* __restrict__ recs, const int* __restrict__ tab,
                                                                unsigned char* __restrict__ out, int32_t* __restrict__ areas, int Hc, int Wc)
{
    __shared__ unsigned long long col[kTile];
    __shared__ int sarea;
    const Rec r = recs[blockIdx.z];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int y0 = blockIdx.y * kTile, x0 = blockIdx.x * kTile;
    const unsigned long long* __restrict__ src = (const unsigned long long*)r.src;
    const int vh = src ? r.valid_h : 0, vw = src ? r.valid_w : 0;
    const bool live = y0 < vh && x0 < vw;                    // (uniform) a tile wholly in the pad reads nothing
    if (threadIdx.x == 0) sarea = 0;
    if (live) {
        const int oy = y0 + lane;
        const bool row_in = oy < vh;
        int sy = 0;
        if (row_in) sy = r.yt_off < 0 ? oy : tab[r.yt_off + oy];
        int area = 0;
        for (int c = wave; c < kTile; c += kT / 64) {
            const int ox = x0 + c;
            bool bit = false;
            if (ox < vw) {                                   // (uniform over the wave)
                const int vx = r.flip_out ? vw - 1 - ox : ox;
                const int sx = r.xt_off < 0 ? vx : tab[r.xt_off + vx];
                if (row_in) {
                    const int64_t p = (int64_t)sx * r.src_h + sy;
                    bit = (src[p >> 6] >> (p & 63)) & 1ull;
                }
            }
            const unsigned long long w = __ballot(bit);
            if (lane == 0) col[c] = w;
            area += __popcll(w);
        }
        __syncthreads();
        if (lane == 0 && area) atomicAdd(&sarea, area);
    }
    // pass 2: row `row` of the tile, columns seg * kSeg .. + kSeg - 1, as four 32-bit words of four bytes each
    const int row = threadIdx.x >> 2, seg = threadIdx.x & 3;
    const int oy = y0 + row, c0 = x0 + seg * kSeg;
    if (oy < Hc && c0 < Wc) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (live) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    w[k] |= (uint32_t)((col[seg * kSeg + 4 * k + b] >> row) & 1ull) << (8 * b);
        }
        unsigned char* o = out + ((int64_t)r.dst * Hc + oy) * Wc + c0;
        const unsigned al = (unsigned)(uintptr_t)out | (unsigned)Wc;
        if ((al & 15) == 0) {                                // every row of every plane is 16-byte aligned, and c0 + 16 <= Wc
            *(uint4*)o = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if ((al & 3) == 0 && c0 + 4 * k + 4 <= Wc) {
                    *(uint32_t*)(o + 4 * k) = w[k];
                } else {
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        if (c0 + 4 * k + b < Wc) o[4 * k + b] = (unsigned char)(w[k] >> (8 * b));
                }
            }
        }
    }
    if (live) {
        __syncthreads();
        if (threadIdx.x == 0 && sarea) atomicAdd(&areas[r.dst], sarea);
    }
}

int bad(const char* who, const char* what) { return mpf::failf(MPF_E_SHAPE, who, what); }

// one table of n entries indexing an axis of `in` entries; off == -1: the identity, which needs n == in
int check_table(const int32_t* tab, int64_t tab_len, int off, int n, int in, const char* who)
{
    if (off == -1) return n == in ? 0 : bad(who, "an identity record needs src == valid on that axis");
    if (off < 0 || (int64_t)off + n > tab_len) return bad(who, "an index table lies outside the table buffer");
    for (int i = 0; i < n; ++i)
        if (tab[off + i] < 0 || tab[off + i] >= in) return bad(who, "a table entry leaves the source mask");
    return 0;
}

}  // namespace

extern "C" int mpf_mask_bits_resample(const MpfMaskBitsRecord* recs_host, const MpfMaskBitsRecord* recs_dev, const int32_t* tab_host,
                                      const int32_t* tab_dev, int64_t tab_len, int P, uint8_t* out, int32_t* areas, int Hc, int Wc,
                                      void* stream)
{
    const char* who = "mask_bits_resample";
    if (P < 0 || Hc <= 0 || Wc <= 0 || tab_len < 0) return bad(who, "need P >= 0, a canvas Hc, Wc > 0 and tab_len >= 0");
    if (P == 0) return 0;
    if (!recs_host || !recs_dev || !tab_host || !tab_dev || !out || !areas) return mpf::fail(MPF_E_NULL, "mask_bits_resample: NULL buffer");
    if (P > 65535) return mpf::failf(MPF_E_TOO_LARGE, who, "P <= 65535 planes");
    if ((int64_t)Hc * Wc >= (1ll << 31)) return mpf::failf(MPF_E_TOO_LARGE, who, "canvas of 2^31 elements or more");
    std::vector<bool> seen((size_t)P, false);
    double src_bytes = 0.0;                                  // (the profiler's byte count: the words of the source masks)
    for (int i = 0; i < P; ++i) {
        const Rec& r = recs_host[i];
        if (r.dst < 0 || r.dst >= P || seen[(size_t)r.dst]) return bad(who, "dst must name every plane 0 .. P-1 once");
        seen[(size_t)r.dst] = true;
        if (!r.src) continue;                                // an empty plane: nothing else is read
        if ((uintptr_t)r.src & 7) return bad(who, "a source mask must be 8-byte aligned (int64 words)");
        if (r.src_h <= 0 || r.src_w <= 0 || r.valid_h <= 0 || r.valid_w <= 0) return bad(who, "sizes must be positive");
        if ((int64_t)r.src_h * r.src_w >= (1ll << 31)) return mpf::failf(MPF_E_TOO_LARGE, who, "source mask of 2^31 positions or more");
        if (r.valid_h > Hc || r.valid_w > Wc) return bad(who, "canvas smaller than the valid size");
        if (r.flip_out < 0 || r.flip_out > 1) return bad(who, "flip_out must be 0 or 1");
        if (int e = check_table(tab_host, tab_len, r.xt_off, r.valid_w, r.src_w, who)) return e;
        if (int e = check_table(tab_host, tab_len, r.yt_off, r.valid_h, r.src_h, who)) return e;
        src_bytes += 8.0 * (double)(((int64_t)r.src_h * r.src_w + 63) / 64);
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((Wc + kTile - 1) / kTile), (unsigned)((Hc + kTile - 1) / kTile), (unsigned)P);
    if (grid.y > 65535) return mpf::failf(MPF_E_TOO_LARGE, who, "canvas taller than 65535 tiles");
    mpf::prof_begin(st);
    mpf::set_kernel("mask_bits_resample_kernel");
    if (int e = mpf::check(hipMemsetAsync(areas, 0, (size_t)P * sizeof(int32_t), st), "mpf_mask_bits_resample")) return e;
    hipLaunchKernelGGL(mask_bits_resample_kernel, grid, dim3(kT), 0, st, recs_dev, (const int*)tab_dev, out, areas, Hc, Wc);
    mpf::prof_end("mask_bits_resample_kernel", st, (double)P * Hc * Wc + src_bytes);
    return mpf::check(hipGetLastError(), "mpf_mask_bits_resample");
}
