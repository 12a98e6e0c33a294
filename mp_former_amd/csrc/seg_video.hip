// Video instance segmentation post-processing for MI355X: the eval branch of the reference's VideoMaskFormer
// (mask2former_video/video_maskformer_model.py:204-287, forward's else branch and inference_video) and the per-tube areas of its
// YouTube-VIS evaluation (mask2former_video/data_video/datasets/ytvis_api/ytvoseval.py:100-104).
//
// Reference: at test time a whole video is one clip, mask_pred_results[0] is [Q, F, h, w];
//     masks = F.interpolate(pred_masks, (Hp, Wp), bilinear)                    fp32 [Q, F, Hp, Wp]  (all Q queries, ~6 GB at F = 36)
//     masks = masks[topk // K][:, :, :hi, :wi];  F.interpolate(masks, (H, W), bilinear) > 0;  .cpu()
// Here the top entries are selected first (the class scores do not depend on the masks) and every output pixel of a selected
// (entry, frame) is computed from its 4 x 4 low-resolution neighbourhood, with the composition, tap order and no-contraction rule of
// seg_rle_bits_kernel (seg_shared.h: pix_geom / resample): an image is a one-frame clip, bit for bit.
//
//   seg_video_bits_kernel   one launch per clip, (entry t, frame f) = (blockIdx.y, blockIdx.z): 64 positions per wave ballot -> one
//                           packed word of bits [T, F, nwords] (p = x * H + y, zero at and past H * W); the popcounts of the words a
//                           workgroup wrote are summed in LDS and added to frame_area [T, F] with ONE integer atomic per workgroup
//                           (zeroed by the call; integer addition commutes: bitwise reproducible).  dense != NULL: the same
//                           decision also stored as bytes [T, F, H, W] (the reference's bool masks), from the same registers.
//   seg_tube_areas_kernel   avg_area[m] = (double)sum / (double)count over the frames of tube m with a non-zero area (0.0 without one):
//                           np.array(l).mean() of ytvoseval.py:100-104 for integer sums below 2^53
// The run lengths of masks that are packed already come from the passes of seg_shared.h (mpf_seg_bits_rle_count / _write): the
// dense mask is not needed for a results file either.
// No float atomics, no workgroup waits on another, plain vector stores.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>

#include "mpf_common.h"
#include "seg_shared.h"

namespace {

// (measured and not kept: a workgroup that computes a pixel's geometry once and walks four frames with it takes the same 1.19 ms at
// T = 10, F = 36, 360 x 640, so the geometry's arithmetic is not what bounds it.  What does was not measured; the likely cost is the
// sixteen loads of a pixel: a wave's lanes run down a column (the bit layout), so each load touches a cache line per low-resolution row.)
template <typename T>
__global__ __launch_bounds__(kT) void seg_video_bits_kernel(const T* __restrict__ masks, const SegGeom s, int64_t stride_f, int F,
                                                            const int64_t* __restrict__ sel_q, int64_t nwords,
                                                            unsigned long long* __restrict__ bits, int* __restrict__ frame_area,
                                                            unsigned char* __restrict__ dense)
{
    __shared__ int wcnt[kT / 64];
    const int t = blockIdx.y, f = blockIdx.z;
    const int H = s.H, W = s.W;
    const int64_t HW = (int64_t)H * W;
    const int64_t row = (int64_t)t * F + f;
    const T* m = masks + sel_q[t] * s.stride_q + (int64_t)f * stride_f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int cnt = 0;                                              // lane 0: the set bits of the words this wave wrote
#pragma unroll
    for (int i = 0; i < kInstPix / kT; ++i) {
        const int64_t p = (int64_t)blockIdx.x * kInstPix + threadIdx.x + kT * i;    // wave-aligned: a wave covers one word
        bool on = false;
        if (p < HW) {
            const int y = (int)(p % H), x = (int)(p / H);
            PixGeom g;
            pix_geom(g, y, x, s);
            on = resample(m, g) > 0.f;
            if (dense) dense[row * HW + (int64_t)y * W + x] = on ? 1 : 0;
        }
        const unsigned long long b = __ballot(on);            // lanes at or past H * W vote 0
        if (lane == 0 && (p >> 6) < nwords) {
            bits[row * nwords + (p >> 6)] = b;
            cnt += __popcll(b);
        }
    }
    if (lane == 0) wcnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
#pragma unroll
        for (int i = 0; i < kT / 64; ++i) total += wcnt[i];
        if (total) atomicAdd(&frame_area[row], total);
    }
}

__global__ __launch_bounds__(kT) void seg_tube_areas_kernel(const int* __restrict__ frame_area, int M, int F, double* __restrict__ avg_area)
{
    const int m = blockIdx.x * kT + threadIdx.x;
    if (m >= M) return;
    long long sum = 0;
    int n = 0;
    for (int f = 0; f < F; ++f) {
        const int a = frame_area[(int64_t)m * F + f];
        if (a) { sum += a; ++n; }
    }
    avg_area[m] = n ? (double)sum / (double)n : 0.0;
}

// the workspace of mpf_seg_bits_rle_count: tile_off int64 [M * tiles], then tile_cnt int32 [M * tiles] (the bits stay the caller's)
struct BitsRleLayout {
    int64_t nwords, tiles;
    size_t tile_off, tile_cnt, total;
};
BitsRleLayout bits_rle_layout(int M, int H, int W)
{
    BitsRleLayout l;
    l.nwords = ((int64_t)H * W + 63) / 64;
    l.tiles = (l.nwords + kRleWords - 1) / kRleWords;
    l.tile_off = 0;
    l.tile_cnt = (size_t)M * l.tiles * 8;
    l.total = l.tile_cnt + (((size_t)M * l.tiles * 4 + 7) & ~(size_t)7);
    return l;
}

int check_bits_rle(const char* who, const void* bits, const void* workspace, size_t workspace_bytes, int M, int H, int W, BitsRleLayout& l)
{
    if (M <= 0 || H <= 0 || W <= 0) return fail_who(MPF_E_SHAPE, who, "need M >= 1 masks of H, W > 0");
    if ((int64_t)H * W >= (1ll << 31) || M > 65535) return fail_who(MPF_E_TOO_LARGE, who, "too large (H * W < 2^31, M <= 65535)");
    if (!bits || !workspace) return fail_who(MPF_E_NULL, who, "NULL buffer");
    l = bits_rle_layout(M, H, W);
    if (workspace_bytes < l.total) return fail_who(MPF_E_SHAPE, who, "workspace too small");
    if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)bits & 7) != 0) return fail_who(MPF_E_SHAPE, who, "bits and workspace must be 8-byte aligned");
    return 0;
}

}  // namespace

extern "C" int mpf_seg_video_bits(const void* masks, int64_t stride_q, int64_t stride_f, int dtype, int Q, int F, int h, int w, int Hp,
                                  int Wp, int hi, int wi, int H, int W, const int64_t* sel_q, int T, uint64_t* bits, int* frame_area,
                                  uint8_t* dense, void* stream)
{
    if (T < 0 || F < 0) return mpf::fail(MPF_E_SHAPE, "seg_video_bits: need T, F >= 0");
    SegGeom g;
    if (int e = check_geom("seg_video_bits", masks, stride_q, dtype, Q, h, w, Hp, Wp, hi, wi, H, W, g)) return e;
    if (F > 1 && stride_f < (int64_t)h * w) return mpf::fail(MPF_E_SHAPE, "seg_video_bits: stride_f smaller than a [h, w] plane");
    const int64_t HW = (int64_t)H * W;
    // the pair counts of a tube (mpf_seg_mask_pairs over F * nwords words) are int32
    if ((int64_t)F * HW >= (1ll << 31) || (int64_t)F * stride_f >= (1ll << 40))
        return mpf::fail(MPF_E_TOO_LARGE, "seg_video_bits: clip too large (F * H * W < 2^31)");
    if (T > 65535 || F > 65535) return mpf::fail(MPF_E_TOO_LARGE, "seg_video_bits: at most 65535 entries and 65535 frames (grid y, z)");
    if (T == 0 || F == 0) return 0;
    if (!sel_q || !bits || !frame_area) return mpf::fail(MPF_E_NULL, "seg_video_bits: NULL buffer");
    if (((uintptr_t)bits & 7) != 0) return mpf::fail(MPF_E_SHAPE, "seg_video_bits: bits must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    if (int e = mpf::check(hipMemsetAsync(frame_area, 0, sizeof(int) * (size_t)T * F, st), "mpf_seg_video_bits")) return e;
    const int64_t nwords = ceil_div(HW, 64);
    const dim3 grid((unsigned)ceil_div(HW, kInstPix), (unsigned)T, (unsigned)F);
    mpf::prof_begin(st);
    mpf::set_kernel(dense ? "seg_video_bits_kernel<dense>" : "seg_video_bits_kernel");
    with_mask_type(dtype, masks, [&](auto* m) {
        hipLaunchKernelGGL(seg_video_bits_kernel<elem_t<decltype(m)>>, grid, dim3(kT), 0, st, m, g, stride_f, F, sel_q, nwords,
                           (unsigned long long*)bits, frame_area, (unsigned char*)dense);
    });
    mpf::prof_end("seg_video_bits_kernel", st, logit_bytes((double)T * F, g, dtype) + (double)T * F * HW / 8 + (dense ? (double)T * F * HW : 0.0));
    return mpf::check(hipGetLastError(), "mpf_seg_video_bits");
}

extern "C" int mpf_seg_tube_areas(const int* frame_area, int M, int F, double* avg_area, void* stream)
{
    if (M < 0 || F < 0) return mpf::fail(MPF_E_SHAPE, "seg_tube_areas: need M, F >= 0");
    if ((int64_t)M * F >= (1ll << 31)) return mpf::fail(MPF_E_TOO_LARGE, "seg_tube_areas: too large");
    if (M == 0) return 0;
    if (!avg_area || (F && !frame_area)) return mpf::fail(MPF_E_NULL, "seg_tube_areas: NULL buffer");
    hipStream_t st = (hipStream_t)stream;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_tube_areas_kernel");
    hipLaunchKernelGGL(seg_tube_areas_kernel, dim3((unsigned)ceil_div(M, kT)), dim3(kT), 0, st, frame_area, M, F, avg_area);
    mpf::prof_end("seg_tube_areas_kernel", st, 4.0 * M * F + 8.0 * M);
    return mpf::check(hipGetLastError(), "mpf_seg_tube_areas");
}

extern "C" size_t mpf_seg_bits_rle_workspace_bytes(int M, int H, int W)
{
    if (M <= 0 || H <= 0 || W <= 0) return 0;
    return bits_rle_layout(M, H, W).total;
}

extern "C" int mpf_seg_bits_rle_count(const uint64_t* bits, int M, int H, int W, int64_t* offsets, void* workspace, size_t workspace_bytes,
                                      void* stream)
{
    BitsRleLayout l;
    if (int e = check_bits_rle("seg_bits_rle_count", bits, workspace, workspace_bytes, M, H, W, l)) return e;
    if (!offsets) return mpf::fail(MPF_E_NULL, "seg_bits_rle_count: NULL offsets");
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_rle_count_kernel+seg_rle_scan_kernel");
    launch_rle_count_scan((const unsigned long long*)bits, M, l.nwords, l.tiles, (int64_t)H * W, (int*)(ws + l.tile_cnt), (int64_t*)(ws + l.tile_off),
                          offsets, st);
    mpf::prof_end("seg_rle_count_kernel", st, 8.0 * M * l.nwords);
    return mpf::check(hipGetLastError(), "mpf_seg_bits_rle_count");
}

extern "C" int mpf_seg_bits_rle_write(const uint64_t* bits, const void* workspace, size_t workspace_bytes, int M, int H, int W,
                                      const int64_t* offsets, int64_t total, uint32_t* pos, uint32_t* counts, void* stream)
{
    BitsRleLayout l;
    if (int e = check_bits_rle("seg_bits_rle_write", bits, workspace, workspace_bytes, M, H, W, l)) return e;
    if (!offsets || !pos || !counts) return mpf::fail(MPF_E_NULL, "seg_bits_rle_write: NULL buffer");
    // every mask has at least its end mark and at most one boundary per position
    if (total < M || total > (int64_t)M * ((int64_t)H * W + 1)) return mpf::fail(MPF_E_SHAPE, "seg_bits_rle_write: total is not offsets[M]");
    hipStream_t st = (hipStream_t)stream;
    const char* ws = (const char*)workspace;
    mpf::prof_begin(st);
    mpf::set_kernel("seg_rle_scatter_kernel+seg_rle_diff_kernel");
    launch_rle_write((const unsigned long long*)bits, M, l.nwords, l.tiles, (int64_t)H * W, (const int64_t*)(ws + l.tile_off), offsets, total, pos,
                     counts, st);
    mpf::prof_end("seg_rle_scatter_kernel", st, 8.0 * M * l.nwords + 12.0 * total);
    return mpf::check(hipGetLastError(), "mpf_seg_bits_rle_write");
}
