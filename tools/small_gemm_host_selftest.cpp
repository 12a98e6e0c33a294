// Stand-alone run of csrc/small_gemm_host.h on the host, for a sanitizer build: the four records of the small-row GEMM family with
// their checks and geometry over every single and every pairwise variation of a good problem, each field over its edge values
// (zeros, negatives, the values on both sides of each rule, INT_MAX — the values on which `int` geometry overflowed).  It launches
// nothing and needs no device.  Build and run from the repository root:
//   hipcc -x hip -std=c++17 --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I mp_former_amd/csrc tools/small_gemm_host_selftest.cpp -o /tmp/small_gemm_host_selftest && /tmp/small_gemm_host_selftest
// For everything the checks let through it asserts that the block counts fit their launch dimension (n_waves, first[] and the
// transpose blocks at most 2^31 - 1), that first[] is non-decreasing with first[n] the grid and the unused slots empty, that
// 1 <= gy <= ntiles with gy <= 65 535 exactly where the route's own check passes, that the weight-stationary LDS is 64 KiB for K = 256
// and 96 KiB for K = 768 (at most the 160 KiB of a workgroup).  It also pins the tile-width rule, which shows neither in results
// nor in profiler records: this program is the only place that can.
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "small_gemm_host.h"

namespace mpf {
static char t_err[256];
int fail(int code, const char* msg) { snprintf(t_err, sizeof(t_err), "%s", msg); return code; }
int failf(int code, const char* who, const char* what) { snprintf(t_err, sizeof(t_err), "%s: %s", who, what); return code; }
}  // namespace mpf

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed (last text: %s)\n", __FILE__, __LINE__, #c, mpf::t_err); abort(); } } while (0)

namespace {
char* const kPtr = (char*)0x7f0000001000;
long g_ok = 0, g_rejected = 0, g_empty = 0, g_too_large = 0;

void count(int e, bool empty)
{
    if (e) { REQUIRE(e < 0 && mpf::t_err[0]); ++g_rejected; g_too_large += e == MPF_E_TOO_LARGE; }
    else if (empty) ++g_empty;
    else ++g_ok;
}

// ---- one small GEMM ---------------------------------------------------------------------------------------------------------------
using SP = SmallGemmProblem;
struct IntField { int SP::*m; std::vector<int> values; };
struct StrideField { int64_t SP::*m; std::vector<int64_t> values; };
const std::vector<IntField> kInts = {
    {&SP::I, {-1, 0, 1, 15, 16, 17, 228, 1008, 1024, 4096, 1 << 20, 1 << 24, INT_MAX - 15, INT_MAX}},
    {&SP::J, {-1, 0, 1, 4, 18, 64, 256, 1 << 17, 1 << 21, INT_MAX - 3, INT_MAX}},
    {&SP::Kc, {-1, 0, 8, 12, 32, 33, 40, 64, INT_MAX - 7, INT_MAX}},
    {&SP::a_blk, {-32, 0, 32, 48, 256, INT_MAX}},
    {&SP::c_blk, {-64, 0, 32, 64, INT_MAX}},
    {&SP::relu, {0, 1}},
};
const std::vector<StrideField> kStrides = {
    {&SP::a_rs, {1, 2, 64, 68}}, {&SP::a_ks, {1, 2, 64}}, {&SP::b_rs, {1, 2, 64, 68}}, {&SP::b_ks, {1, 2, 64}},
    {&SP::ldc, {0, 16, 18, (int64_t)INT_MAX * 4}}, {&SP::ldcin, {0, 16, 18}},
};

SP good_gemm()
{
    return {kPtr, nullptr, kPtr, kPtr, nullptr, kPtr, kPtr, 64, 1, 0, 64, 1, 16, 16, 0, 0, 0, 16, 16, 64, 0};
}

void exercise(const SP& p)
{
    const int e = small_gemm_check(p);
    count(e, p.empty());
    if (e || p.empty()) return;
    const int nj = p.nj();
    REQUIRE(nj == 1 || nj == 2 || nj == 4);
    REQUIRE(p.n_it() == ((int64_t)p.I + 15) / 16 && p.tiles_j() == ((int64_t)p.J + 16 * nj - 1) / (16 * nj));
    REQUIRE(p.n_waves() == p.n_it() * p.tiles_j() && p.n_waves() >= 1 && p.n_waves() <= kSgGridX);
    REQUIRE(nj == 1 || p.n_waves() >= kSgFillBlocks);                                         // a wide tile only where it fills the chip
    REQUIRE(nj == 4 || p.n_it() * sg_ceil_div(p.J, 32 * nj) < kSgFillBlocks);                 // and the widest that does
    REQUIRE(p.masked() == (p.Kc % 32 != 0) && p.bytes() > 0.0);
}

void sweep_gemm()
{
    const auto pointers = [](SP p) {
        exercise(p);
        for (const void* SP::*m : {&SP::a, &SP::gate, &SP::b, &SP::bias, &SP::c_in})
            for (const void* v : {(const void*)nullptr, (const void*)kPtr, (const void*)(kPtr + 4), (const void*)(kPtr + 8)}) { SP q = p; q.*m = v; exercise(q); }
        for (void* SP::*m : {&SP::c, &SP::rowsum_a})
            for (void* v : {(void*)nullptr, (void*)(kPtr + 4)}) { SP q = p; q.*m = v; exercise(q); }
    };
    const auto strides = [&](const SP& p) {
        pointers(p);
        for (const StrideField& s : kStrides)
            for (int64_t v : s.values) { SP q = p; q.*s.m = v; exercise(q); }
        SP rows = p;                                   // the weight-gradient form: both operands row-contiguous
        rows.a_rs = rows.b_rs = 1; rows.a_ks = rows.b_ks = 1 << 20;
        pointers(rows);
    };
    strides(good_gemm());
    for (size_t a = 0; a < kInts.size(); ++a)
        for (int va : kInts[a].values) {
            SP p = good_gemm();
            p.*kInts[a].m = va;
            strides(p);
            for (size_t b = a + 1; b < kInts.size(); ++b)
                for (int vb : kInts[b].values) { SP q = p; q.*kInts[b].m = vb; strides(q); }
        }
}

void tile_width_rule()
{
    const int table[][3] = {{228, 256, 1}, {1008, 256, 2}, {1024, 256, 4}, {2048, 64, 2}, {4096, 4, 4}, {16, 4, 1}};       // I, J -> nj
    for (const auto& t : table) {
        SP p = good_gemm();
        p.I = t[0]; p.J = t[1];
        REQUIRE(small_gemm_check(p) == 0 && p.nj() == t[2]);
    }
    SP p = good_gemm();
    p.I = 228; p.J = 256;
    REQUIRE(p.n_waves() == 240);
    p.I = 1008;
    REQUIRE(p.n_waves() == 63 * 8 && p.n_it() * sg_ceil_div(p.J, 64) == 252);
    p.I = 1024;
    REQUIRE(p.n_waves() == 256);
}

// ---- grouped launch ---------------------------------------------------------------------------------------------------------------
MpfSmallGemmItem good_item(bool contig)
{
    MpfSmallGemmItem m;
    m.a = kPtr; m.gate = nullptr; m.b = kPtr; m.c = kPtr; m.rowsum_a = kPtr;
    m.a_rs = contig ? 64 : 1; m.a_ks = contig ? 1 : 16; m.a_bs = 0; m.b_rs = contig ? 64 : 1; m.b_ks = contig ? 1 : 16; m.ldc = 16;
    m.a_blk = 0; m.I = 16; m.J = 16; m.Kc = 32;
    return m;
}

void exercise_group(const MpfSmallGemmItem* items, int n)
{
    SmallGemmGroupPlan g;
    const int e = small_gemm_group_plan(g, items, n);
    count(e, g.n == 0);
    if (e || g.n == 0) return;
    REQUIRE(g.n <= n && g.n <= kSgGroupMax && g.first[0] == 0 && g.first[g.n] >= g.n && g.first[g.n] <= kSgGridX && g.bytes > 0.0);
    for (int t = 0; t < kSgGroupMax; ++t) {
        REQUIRE(g.first[t + 1] >= g.first[t] && (g.nj[t] == 1 || g.nj[t] == 2 || g.nj[t] == 4));
        if (t < g.n) REQUIRE(g.first[t + 1] - g.first[t] == g.it[t].n_waves() && g.nj[t] == g.it[t].nj() && g.it[t].masked() == g.masked
                             && (g.it[t].ac() && g.it[t].bc()) == g.contig && !g.it[t].empty());
        else REQUIRE(g.first[t + 1] == g.first[g.n] && g.it[t].a == g.it[0].a);          // an unused slot: an empty range of problem 0
    }
}

void sweep_group()
{
    const std::vector<int> sizes = {-1, 0, 1, 16, 1 << 20, 1 << 24, INT_MAX - 15, INT_MAX};
    const std::vector<int> depths = {-1, 0, 8, 32, 33, 40, INT_MAX - 7};
    for (int n : {-1, 0, 1, 2, 8, 9}) {
        exercise_group(nullptr, n);
        for (bool contig : {false, true}) {
            std::vector<MpfSmallGemmItem> items(9, good_item(contig));
            exercise_group(items.data(), n);
            if (n < 1 || n > 8) continue;
            for (int at : {0, n / 2, n - 1}) {
                for (int I : sizes) for (int J : sizes) for (int Kc : depths) {
                    auto v = items;
                    v[at].I = I; v[at].J = J; v[at].Kc = Kc;
                    exercise_group(v.data(), n);
                    for (auto& m : v) { m.I = I; m.J = J; }                     // every item large: the sum of the tiles
                    exercise_group(v.data(), n);
                }
                auto v = items;
                v[at] = good_item(!contig); exercise_group(v.data(), n);
                v = items; v[at].gate = kPtr; exercise_group(v.data(), n);
                v = items; v[at].a_rs = 2; exercise_group(v.data(), n);
                v = items; v[at].a = nullptr; exercise_group(v.data(), n);
                v = items; v[at].a_blk = 48; exercise_group(v.data(), n);
                v = items; v[at].a_blk = 32; v[at].a_bs = 1 << 20; exercise_group(v.data(), n);
            }
        }
    }
}

// ---- transposes -------------------------------------------------------------------------------------------------------------------
void exercise_transpose(const MpfTransposeItem* items, int n, int Rp)
{
    TransposeGroupPlan g;
    const int e = transpose_group_plan(g, items, n, Rp);
    count(e, g.n == 0);
    if (e || g.n == 0) return;
    REQUIRE(g.n == n && g.tiles_r == ((int64_t)Rp + 63) / 64 && g.first[0] == 0 && g.blocks() == g.first[n] && g.blocks() >= n && g.blocks() <= kSgGridX);
    for (int t = 0; t < n; ++t) REQUIRE(g.first[t + 1] - g.first[t] == g.tiles_r * (((int64_t)items[t].C + 63) / 64));
}

void sweep_transpose()
{
    for (int n : {-1, 0, 1, 2, 16, 17}) for (int Rp : {-8, 0, 8, 12, 64, 72, INT_MAX - 7, INT_MAX}) {
        exercise_transpose(nullptr, n, Rp);
        MpfTransposeItem good;
        good.src = kPtr; good.gate = nullptr; good.dst = kPtr; good.ld = 16; good.R = 8; good.C = 16;
        std::vector<MpfTransposeItem> items(17, good);
        exercise_transpose(items.data(), n, Rp);
        if (n < 1 || n > 16) continue;
        for (int R : {-1, 0, 1, 8, 9, INT_MAX}) for (int C : {-8, 0, 8, 12, 64, 72, 4096, INT_MAX - 7, INT_MAX}) for (int64_t ld : {(int64_t)16, (int64_t)20, (int64_t)INT_MAX * 8}) {
            auto v = items;
            v[n - 1].R = R; v[n - 1].C = C; v[n - 1].ld = ld;
            exercise_transpose(v.data(), n, Rp);
            for (auto& m : v) m.C = C;
            exercise_transpose(v.data(), n, Rp);
        }
        auto v = items;
        v[n / 2].src = nullptr; exercise_transpose(v.data(), n, Rp);
        v = items; v[n / 2].dst = kPtr + 8; exercise_transpose(v.data(), n, Rp);
        v = items; v[n / 2].gate = kPtr + 8; exercise_transpose(v.data(), n, Rp);
    }
}

// ---- tall ---------------------------------------------------------------------------------------------------------------------------
void exercise_tall(const TallGemmProblem& p)
{
    if (p.empty()) { ++g_empty; return; }
    const int e = tall_gemm_check(p);
    count(e, false);
    if (e) return;
    for (bool tall_ws : {false, true}) for (int cus : {1, 64, 256, 304}) for (int wgs : {0, 1, 3, 65535, 65536, 1 << 20, INT_MAX, -1}) {
        const TallRoute r = p.route(tall_ws, cus, wgs);
        REQUIRE(r.ws == (tall_ws && p.M >= 1024 && (p.K == 256 || p.K == 768)));
        REQUIRE(r.gx >= 1 && r.gx <= kSgGridX && r.gy >= 1 && r.gy <= r.ntiles);
        if (!r.ws) {
            REQUIRE(r.lds == 0 && r.gx == ((int64_t)p.N + 127) / 128 && r.gy == ((int64_t)p.M + 127) / 128 && r.gy <= kSgGridY && r.check() == 0);
            continue;
        }
        REQUIRE(r.KS * 32 == p.K && r.NBUF == 2 && (p.K == 256 ? r.NB == 2 && r.MB == 4 : r.NB == 1 && r.MB == 2));
        REQUIRE(r.lds == (p.K == 256 ? 64u : 96u) * 1024 && r.lds <= 160 * 1024);
        REQUIRE(r.ntiles * r.MB * 16 >= p.M && (r.ntiles - 1) * r.MB * 16 < p.M && r.gx * 64 * r.NB >= p.N && (r.gx - 1) * 64 * r.NB < p.N);
        if (wgs == 0) REQUIRE(r.gy * r.gx <= (int64_t)cus * (r.lds > 80 * 1024 ? 1 : 2) || r.gy == 1);       // one residency
        const int ec = r.check();
        REQUIRE((ec == 0) == (r.gy <= kSgGridY) && (ec == 0 || ec == MPF_E_TOO_LARGE));
        g_too_large += ec != 0;
    }
    REQUIRE(p.bytes() > 0.0 && p.flops() > 0.0);
}

void sweep_tall()
{
    const std::vector<int> Ms = {-1, 0, 1, 127, 128, 1023, 1024, 1025, 65535 * 128, 65535 * 128 + 1, 1 << 21, INT_MAX - 127, INT_MAX};
    const std::vector<int> Ns = {-1, 0, 1, 64, 65, 128, 130, 768, INT_MAX};
    const std::vector<int> Ks = {-32, 0, 32, 40, 64, 256, 768, 1024, INT_MAX - 31, INT_MAX};
    for (int M : Ms) for (int N : Ns) for (int K : Ks) {
        const TallGemmProblem good{kPtr, kPtr, kPtr, kPtr, 64, 64, 16, M, N, K};
        exercise_tall(good);
        TallGemmProblem p = good;
        p.bias = nullptr; exercise_tall(p);
        for (const void* TallGemmProblem::*m : {&TallGemmProblem::a, &TallGemmProblem::b})
            for (const void* v : {(const void*)nullptr, (const void*)(kPtr + 8)}) { p = good; p.*m = v; exercise_tall(p); }
        p = good; p.c = nullptr; exercise_tall(p);
        p = good; p.c = kPtr + 4; exercise_tall(p);
        for (int64_t TallGemmProblem::*m : {&TallGemmProblem::lda, &TallGemmProblem::ldb, &TallGemmProblem::ldc})
            for (int64_t v : {(int64_t)18, (int64_t)68, (int64_t)INT_MAX * 8}) { p = good; p.*m = v; exercise_tall(p); }
    }
}
}  // namespace

int main()
{
    tile_width_rule();
    sweep_gemm();
    sweep_group();
    sweep_transpose();
    sweep_tall();
    REQUIRE(g_ok > 0 && g_rejected > 0 && g_empty > 0 && g_too_large > 0);
    printf("small_gemm_host.h: %ld problems accepted, %ld empty, %ld rejected (%ld of them as too large for a launch)\n", g_ok, g_empty, g_rejected,
           g_too_large);
    return 0;
}
