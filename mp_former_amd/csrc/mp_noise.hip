// Point noise of the mask-piloted (MP) attention rows (mask2former_transformer_decoder.py:985-998, :1599-1620):
//   mpf_mp_open_counts   open (0) bytes per ground-truth row, once per level and forward
//   mpf_mp_noise_rows    the whole [N, pad, HW] byte tensor of one attention mask in ONE launch: padding rows all 1, occupied rows
//                        base ^ (u < ratio) with u from Philox4x32-10 keyed by (seed, draw, row, position)
// The contract of u(r, j) is spelled out in include/mpformer_hip.h; tests/test_mp_noise_*.py restate it in numpy.
#include "mpf_common.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct Philox4 { uint32_t x, y, z, w; };

// Philox4x32-10 (Salmon et al., SC'11): ten rounds, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
        const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
    return {c0, c1, c2, c3};
}

__device__ __forceinline__ uint32_t flip_bit(uint32_t word, float ratio)
{
    return ((float)(word >> 8) * 0x1p-24f) < ratio ? 1u : 0u;      // u in [0, 1), exact in fp32
}

// the four flips of positions 4 * quad .. 4 * quad + 3 of base row r, one per byte of the result
__device__ __forceinline__ uint32_t flips4(uint32_t quad, uint32_t r, uint32_t d_lo, uint32_t d_hi, uint32_t k0, uint32_t k1, float ratio)
{
    const Philox4 p = philox4x32_10(quad, r, d_lo, d_hi, k0, k1);
    return flip_bit(p.x, ratio) | (flip_bit(p.y, ratio) << 8) | (flip_bit(p.z, ratio) << 16) | (flip_bit(p.w, ratio) << 24);
}

// One lane owns 16 consecutive bytes of one output row: (output row, 16-byte chunk) flattened over the grid, so that a single
// instance still spreads over HW / 16 lanes.  VEC: HW % 16 == 0 and both buffers 16-byte aligned -> one 16-byte load of `base`
// and one 16-byte store; otherwise the same chunk byte by byte (rows are then not 16-byte aligned; the last chunk is partial).
template <bool VEC>
__global__ __launch_bounds__(kThreads) void mp_noise_rows_kernel(const uint8_t* __restrict__ base, const int* __restrict__ counts,
                                                                 const int* __restrict__ src_of, int R, int HW, int chunks,
                                                                 int64_t total, float scale, uint32_t k0, uint32_t k1,
                                                                 uint32_t d_lo, uint32_t d_hi, uint8_t* __restrict__ out)
{
    const int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const int64_t orow = idx / chunks;
    const int chunk = (int)(idx - orow * chunks);
    const int r = src_of[orow];
    const bool occupied = r >= 0 && r < R;            // (a row index outside `base` is treated as an empty slot, never read)
    const float ratio = occupied ? __fmul_rn((float)counts[r], scale) : 0.f;
    const bool noisy = ratio > 0.f;                   // u >= 0: no position can flip at ratio 0, the draws are not needed
    uint8_t* dst = out + orow * (int64_t)HW + (int64_t)chunk * 16;
    const uint8_t* src = base + (int64_t)(occupied ? r : 0) * HW + (int64_t)chunk * 16;
    if (VEC) {
        uint4 v = make_uint4(0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u);
        if (occupied) {
            v = *reinterpret_cast<const uint4*>(src);
            if (noisy) {
                const uint32_t q = (uint32_t)chunk * 4;
                v.x ^= flips4(q, (uint32_t)r, d_lo, d_hi, k0, k1, ratio);
                v.y ^= flips4(q + 1, (uint32_t)r, d_lo, d_hi, k0, k1, ratio);
                v.z ^= flips4(q + 2, (uint32_t)r, d_lo, d_hi, k0, k1, ratio);
                v.w ^= flips4(q + 3, (uint32_t)r, d_lo, d_hi, k0, k1, ratio);
            }
        }
        *reinterpret_cast<uint4*>(dst) = v;
    } else {
        const int left = HW - chunk * 16;
        const int n = left < 16 ? left : 16;
        for (int q = 0; q < 4 && q * 4 < n; ++q) {
            const uint32_t f = noisy ? flips4((uint32_t)chunk * 4 + q, (uint32_t)r, d_lo, d_hi, k0, k1, ratio) : 0u;
            for (int b = 0; b < 4 && q * 4 + b < n; ++b)
                dst[q * 4 + b] = occupied ? (uint8_t)(src[q * 4 + b] ^ ((f >> (8 * b)) & 1u)) : (uint8_t)1;
        }
    }
}

__device__ __forceinline__ int zero_bytes(uint32_t w)
{
    return ((w & 0xffu) == 0) + ((w & 0xff00u) == 0) + ((w & 0xff0000u) == 0) + ((w & 0xff000000u) == 0);
}

// one 64-lane wave per row, 16 bytes per lane and step; the wave total leaves through lane 0
template <bool VEC>
__global__ __launch_bounds__(kThreads) void mp_open_counts_kernel(const uint8_t* __restrict__ base, int R, int HW, int* __restrict__ counts)
{
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (r >= R) return;
    const uint8_t* row = base + (int64_t)r * HW;
    int n = 0;
    if (VEC) {
        for (int c = lane; c < HW / 16; c += 64) {
            const uint4 v = *reinterpret_cast<const uint4*>(row + (int64_t)c * 16);
            n += zero_bytes(v.x) + zero_bytes(v.y) + zero_bytes(v.z) + zero_bytes(v.w);
        }
    } else {
        for (int j = lane; j < HW; j += 64) n += row[j] == 0;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if (lane == 0) counts[r] = n;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int mpf_mp_open_counts(const uint8_t* base, int R, int HW, int* counts, void* stream)
{
    if (!base || !counts) return mpf::fail(MPF_E_NULL, "mpf_mp_open_counts: NULL buffer");
    if (R <= 0 || HW <= 0) return mpf::fail(MPF_E_SHAPE, "mpf_mp_open_counts: R and HW must be positive");
    if ((int64_t)R * HW >= ((int64_t)1 << 31)) return mpf::fail(MPF_E_TOO_LARGE, "mpf_mp_open_counts: R * HW exceeds 2^31");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((R + kThreads / 64 - 1) / (kThreads / 64)));
    mpf::prof_begin(st);
    mpf::set_kernel("mp_open_counts_kernel");
    if (HW % 16 == 0 && aligned16(base))
        hipLaunchKernelGGL(mp_open_counts_kernel<true>, grid, dim3(kThreads), 0, st, base, R, HW, counts);
    else
        hipLaunchKernelGGL(mp_open_counts_kernel<false>, grid, dim3(kThreads), 0, st, base, R, HW, counts);
    mpf::prof_end("mp_open_counts_kernel", st, (double)R * HW + 4.0 * R);
    return mpf::check(hipGetLastError(), "mpf_mp_open_counts");
}

extern "C" int mpf_mp_noise_rows(const uint8_t* base, const int* counts, const int* src_of, int R, int HW, int N, int pad,
                                 double noise_scale, uint64_t seed, uint64_t draw, uint8_t* out, void* stream)
{
    if (!base || !counts || !src_of || !out) return mpf::fail(MPF_E_NULL, "mpf_mp_noise_rows: NULL buffer");
    if (R <= 0 || HW <= 0 || N <= 0 || pad <= 0) return mpf::fail(MPF_E_SHAPE, "mpf_mp_noise_rows: R, HW, N and pad must be positive");
    if (!(noise_scale >= 0.0)) return mpf::fail(MPF_E_SHAPE, "mpf_mp_noise_rows: noise_scale must be >= 0");
    if ((int64_t)R * HW >= ((int64_t)1 << 31) || (int64_t)N * pad * HW >= ((int64_t)1 << 31))
        return mpf::fail(MPF_E_TOO_LARGE, "mpf_mp_noise_rows: R * HW or N * pad * HW exceeds 2^31");
    hipStream_t st = (hipStream_t)stream;
    const int chunks = (HW + 15) / 16;
    const int64_t total = (int64_t)N * pad * chunks;
    const dim3 grid((unsigned)((total + kThreads - 1) / kThreads));
    const float scale = (float)(noise_scale / (double)HW);
    const uint64_t key = seed ^ (uint64_t)MPF_MP_NOISE_KEY;
    const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32), d_lo = (uint32_t)draw, d_hi = (uint32_t)(draw >> 32);
    mpf::prof_begin(st);
    mpf::set_kernel("mp_noise_rows_kernel");
    if (HW % 16 == 0 && aligned16(base) && aligned16(out))
        hipLaunchKernelGGL(mp_noise_rows_kernel<true>, grid, dim3(kThreads), 0, st, base, counts, src_of, R, HW, chunks, total, scale,
                           k0, k1, d_lo, d_hi, out);
    else
        hipLaunchKernelGGL(mp_noise_rows_kernel<false>, grid, dim3(kThreads), 0, st, base, counts, src_of, R, HW, chunks, total, scale,
                           k0, k1, d_lo, d_hi, out);
    mpf::prof_end("mp_noise_rows_kernel", st, 2.0 * N * pad * HW);
    return mpf::check(hipGetLastError(), "mpf_mp_noise_rows");
}
