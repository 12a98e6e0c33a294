// Bounding boxes of packed instance masks for MI355X: Detectron2's BitMasks.get_bounding_boxes, the call the reference's
// instance_inference leaves commented out because it is slow on dense masks (mask2former/maskformer_model.py:393-395), on the packed
// bits of seg_ap.hip: position p = x * H + y (column-major), 64 positions per uint64 word, bit b of word j = position 64 j + b, bits
// at or past H * W zero.  A mask costs one read of 1/8 byte per pixel.
//
//   seg_bits_boxes_kernel    one workgroup per mask.  Positions are x-major, so the x range is that of the first and the last set
//                            position of the mask: x0 = pmin / H, x1 = pmax / H + 1.  The y range needs p mod H over the set bits: a
//                            word covers 64 consecutive positions, which lie in one column, straddle one column boundary (H >= 64) or
//                            span several columns (H < 64).  A thread walks the non-empty column segments of its non-zero words: the
//                            first set bit of what is left names the column, the segment is the word masked to that column, its lowest
//                            and highest set bit (ctz / clz) are the segment's y range.  Each thread keeps (pmin, pmax, ymin, ymax);
//                            they are reduced over the wave by shuffles, over the workgroup's waves through LDS, and thread 0 writes
//                            the box.  Integer only, one writer per box, no atomics: bitwise reproducible.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpf_common.h"

namespace {

constexpr int kBoxT = 1024;                // a mask is read by one workgroup: the widest one, kBoxLoads words per thread in flight
constexpr int kBoxWaves = kBoxT / 64;
constexpr int kBoxLoads = 4;
constexpr int kBoxNone = 0x7fffffff;       // pmin / ymin of a thread that saw no set bit (the maxima start at -1)

__global__ __launch_bounds__(kBoxT) void seg_bits_boxes_kernel(const unsigned long long* __restrict__ bits, int H, int HW, int nwords,
                                                               int* __restrict__ boxes)
{
    __shared__ int part[4][kBoxWaves];
    const int m = blockIdx.x;
    const unsigned long long* row = bits + (int64_t)m * nwords;
    const int tail = HW & 63;                // set positions of the last word; bits past H * W are not looked at
    int pmin = kBoxNone, pmax = -1, ymin = kBoxNone, ymax = -1;
    for (int j0 = threadIdx.x; j0 < nwords; j0 += kBoxLoads * kBoxT) {
        unsigned long long ws[kBoxLoads];                   // the loads of a pass are issued together, then walked
#pragma unroll
        for (int u = 0; u < kBoxLoads; ++u) {
            const int j = j0 + u * kBoxT;
            ws[u] = j < nwords ? row[j] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < kBoxLoads; ++u) {
            const int j = j0 + u * kBoxT;
            unsigned long long w = ws[u];
            if (j == nwords - 1 && tail) w &= (1ull << tail) - 1ull;
            if (w == 0ull) continue;
            const int p0 = j << 6;           // < 2^31: H * W < 2^31
            pmin = min(pmin, p0 + __builtin_ctzll(w));
            pmax = max(pmax, p0 + (63 - __builtin_clzll(w)));
            if (ymin == 0 && ymax == H - 1) continue;      // the y range is full already
            do {
                const int b = __builtin_ctzll(w);
                const int c0 = ((p0 + b) / H) * H;          // first position of the column of the lowest bit left
                const int e = min(c0 + H - p0, 64);         // its positions in this word: bits [b, e)
                const unsigned long long seg = e < 64 ? w & ((1ull << e) - 1ull) : w;
                ymin = min(ymin, p0 + b - c0);
                ymax = max(ymax, p0 - c0 + (63 - __builtin_clzll(seg)));
                w ^= seg;
            } while (w != 0ull);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        pmin = min(pmin, __shfl_xor(pmin, o));
        pmax = max(pmax, __shfl_xor(pmax, o));
        ymin = min(ymin, __shfl_xor(ymin, o));
        ymax = max(ymax, __shfl_xor(ymax, o));
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = pmin;
        part[1][wave] = pmax;
        part[2][wave] = ymin;
        part[3][wave] = ymax;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < kBoxWaves; ++v) {               // fixed order
            pmin = min(pmin, part[0][v]);
            pmax = max(pmax, part[1][v]);
            ymin = min(ymin, part[2][v]);
            ymax = max(ymax, part[3][v]);
        }
        const bool any = pmax >= 0;                         // an empty mask: (0, 0, 0, 0)
        int* box = boxes + 4 * (int64_t)m;
        box[0] = any ? pmin / H : 0;
        box[1] = any ? ymin : 0;
        box[2] = any ? pmax / H + 1 : 0;
        box[3] = any ? ymax + 1 : 0;
    }
}

}  // namespace

extern "C" int mpf_seg_bits_boxes(const uint64_t* bits, int M, int H, int W, int* boxes, void* stream)
{
    if (M < 0 || H <= 0 || W <= 0) return mpf::fail(MPF_E_SHAPE, "seg_bits_boxes: need M >= 0 masks of H, W > 0");
    if (M == 0) return 0;
    if (!bits || !boxes) return mpf::fail(MPF_E_NULL, "seg_bits_boxes: NULL buffer");
    if ((int64_t)H * W >= (1ll << 31) || M > 65535) return mpf::fail(MPF_E_TOO_LARGE, "seg_bits_boxes: too large (H * W < 2^31, M <= 65535)");
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W, nwords = (int)(((int64_t)HW + 63) / 64);
    mpf::prof_begin(st);
    mpf::set_kernel("seg_bits_boxes_kernel");
    hipLaunchKernelGGL(seg_bits_boxes_kernel, dim3((unsigned)M), dim3(kBoxT), 0, st, (const unsigned long long*)bits, H, HW, nwords, boxes);
    mpf::prof_end("seg_bits_boxes_kernel", st, 8.0 * M * nwords + 16.0 * M);
    return mpf::check(hipGetLastError(), "mpf_seg_bits_boxes");
}
