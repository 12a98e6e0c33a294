// Stand-alone run of csrc/mask_fused_host.h on the host, for a sanitizer build: the record's arithmetic, its two workspace layouts
// and mask_fused_check over every single and every pairwise variation of a good problem per entry, with the values of the fault
// table of tools/record_mask_fused_host.py (zeros, negatives, 129 targets, 65 536 groups / frames / images, the 2^31 products,
// unaligned strides, a frame stride that overlaps, pixel counts off the tile, dtype 99) plus INT_MAX, the values on which `int`
// geometry overflowed.  It launches nothing and needs no device.  Build and run from the repository root:
//   hipcc -x hip -std=c++17 --offload-arch=gfx950 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all \
//         -I mp_former_amd/csrc tools/mask_fused_host_selftest.cpp -o /tmp/mask_fused_host_selftest && /tmp/mask_fused_host_selftest
// It asserts what must hold for every problem the check lets through: the cost kernel's LDS is within the 160 KiB of a workgroup,
// the grids are non-empty and within 65 535 on y and z, the workspace parts are 256-byte aligned, disjoint and inside the total,
// the pixel chunks of d E are whole 64-pixel steps that cover the plane.  Two grid dimensions have no rule in the check, as before
// the record existed: qgroups = ceil(Q / 128) on grid.z of the cost (not reached by these values: Q steps from 129 to 2^29, which
// the 2^31 rule rejects in every pair of the sweep) and mgroups = ceil(max_count / 128) on grid.y of d E, which max_count = INT_MAX exceeds;
// such a call is refused by the runtime at launch and is counted here, not asserted on.  The size queries run over all combinations
// of their values.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "mask_fused_host.h"

namespace mpf {
static char t_err[256];
int fail(int code, const char* msg) { snprintf(t_err, sizeof(t_err), "%s", msg); return code; }
int failf(int code, const char* who, const char* what) { snprintf(t_err, sizeof(t_err), "%s: %s", who, what); return code; }
}  // namespace mpf

#define REQUIRE(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s failed (last text: %s)\n", __FILE__, __LINE__, #c, mpf::t_err); abort(); } } while (0)

namespace {
using P = MaskFusedProblem;
using E = MaskFusedEntry;
constexpr int kIntMax = 0x7fffffff;
constexpr size_t kWorkgroupLds = 160 * 1024;
const void* const kPtr = (const void*)0x7f0000001000;

struct Field { int P::*m; std::vector<int> values; };
const std::vector<Field> kFields = {
    {&P::channels, {255, 256, kIntMax}},
    {&P::G, {-1, 0, 1, 512, 513, 65535, 65536, kIntMax}},
    {&P::Q, {-1, 0, 1, 128, 129, 1 << 29, kIntMax}},
    {&P::Tmax, {-1, 0, 1, 8, 9, 128, 129, kIntMax}},
    {&P::P, {-1, 0, 1, 32, 33, 32769, kIntMax}},
    {&P::F, {-1, 0, 1, 65535, 65536, kIntMax}},
    {&P::h, {-1, 0, kIntMax}},
    {&P::w, {-1, 0, kIntMax}},
    {&P::tsamp_rows, {-1, 0, 1, kIntMax}},
    {&P::N, {-1, 0, 1, 9, 513, 65535, 65536, kIntMax}},
    {&P::HW, {-1, 0, 4, 192, 258, 8576, 65536, kIntMax}},
    {&P::total_slots, {-1, 0, 1, kIntMax}},
    {&P::max_count, {-1, 0, 64, 65, 128, 129, 257, kIntMax}},
    {&P::d_embed_dtype, {MPF_F32, MPF_BF16, 99}},
};
struct Stride { int64_t P::*m; };
const std::vector<Stride> kStrides = {{&P::embed_row_stride}, {&P::feat_stride}, {&P::feat_frame_stride}, {&P::dfeat_stride}};

long g_ok = 0, g_rejected = 0, g_unlaunchable = 0, g_queries = 0;

bool has(E e, int P::*m)
{
    const bool cost = e == E::cost || e == E::cost_clip;
    if (m == &P::channels) return true;
    if (m == &P::F) return e == E::cost_clip;
    if (m == &P::N || m == &P::HW) return !cost;
    if (m == &P::total_slots || m == &P::max_count || m == &P::d_embed_dtype) return e == E::planes_bwd;
    return cost;
}

P good(E e)
{
    P p{e};
    if (p.is_cost()) {
        p.G = 6; p.Q = 100; p.Tmax = 5; p.P = 100; p.h = 8; p.w = 12; p.tsamp_rows = 40; p.embed_row_stride = 768; p.feat_stride = 24576;
        if (p.clip()) { p.F = 3; p.feat_stride = 3 * 24576; p.feat_frame_stride = 24576; }
    } else {
        p.N = 2; p.HW = 256; p.feat_stride = 65536;
        if (e == E::planes_bwd) { p.total_slots = 10; p.max_count = 6; p.dfeat_stride = 65536; p.d_features = p.d_embed = true; }
    }
    return p;
}

void parts_ok(size_t a, size_t b, size_t total)
{
    REQUIRE(a > 0 && a < b && b < total && a % 256 == 0 && b % 256 == 0 && total % 256 == 0);
}

void exercise(const char* who, const P& p)
{
    REQUIRE(mask_fused_check(who, p, {kPtr, nullptr}, kPtr, (size_t)-1) == MPF_E_NULL);
    const size_t need = p.workspace_bytes();
    const int e = mask_fused_check(who, p, {kPtr, kPtr}, kPtr, need);
    if (e) { REQUIRE(e < 0 && mpf::t_err[0]); ++g_rejected; return; }
    ++g_ok;
    if (p.entry != E::planes_fwd) {
        REQUIRE(need > 0 && mask_fused_check(who, p, {kPtr}, kPtr, need - 1) == MPF_E_SHAPE && mask_fused_check(who, p, {kPtr}, nullptr, need) == MPF_E_NULL);
    }
    const auto grid_ok = [](dim3 g) { return g.x > 0 && g.y > 0 && g.z > 0 && g.y <= (unsigned)kGridYZ && g.z <= (unsigned)kGridYZ; };
    if (p.is_cost()) {
        const CostWs ws = p.cost_ws();
        REQUIRE(p.cost_lds() <= kWorkgroupLds && p.cost_lds() == (size_t)kOffTV + 256 * p.tch() && 2 * p.tch() >= p.Tmax);
        REQUIRE(p.nwg() >= 1 && p.nwg() <= kRound && p.nwg() * p.tiles_per_wg() >= p.ntiles() && (p.nwg() - 1) * p.tiles_per_wg() < p.ntiles());
        REQUIRE(grid_ok(p.rowsum_grid()) && grid_ok(p.cost_grid()) && grid_ok(p.fold_grid()) && (int64_t)p.fold_grid().x * kT >= p.cells());
        parts_ok(ws.part_q, ws.tsum, ws.total);
        REQUIRE(ws.part_q >= (size_t)p.nwg() * p.cells() * 8 && ws.tsum - ws.part_q >= (size_t)p.nwg() * p.G * p.Q * 8 && ws.total - ws.tsum >= (size_t)p.tsamp_rows * 4);
        REQUIRE(p.cost_bytes() > 0.0 && p.cost_flops() > 0.0);
    } else if (p.entry == E::planes_fwd) {
        REQUIRE(grid_ok(p.fwd_grid()) && (int64_t)p.fwd_grid().x * kPxTile >= p.HW && p.fwd_bytes() > 0.0);
    } else {
        const PairBwdWs ws = p.pair_bwd_ws();
        REQUIRE(p.px_per_chunk() * p.KS() == p.HW && p.px_per_chunk() % kPxStep == 0 && p.KS() >= 1 && p.KS() <= kMaxKS);
        REQUIRE(p.KP() % 64 == 0 && p.KP() >= p.max_count && p.mgroups() * kSlotGroup >= p.max_count);
        parts_ok(ws.part, ws.valid, ws.total);
        REQUIRE(ws.part >= (size_t)p.N * kC * p.KP() * 2 && ws.valid - ws.part >= (size_t)p.KS() * p.total_slots * kC * 4 && ws.total - ws.valid >= (size_t)p.total_slots * 4);
        REQUIRE(grid_ok(p.transpose_grid()) && grid_ok(p.dfeat_grid()) && grid_ok(p.valid_grid()) && grid_ok(p.reduce_grid()));
        REQUIRE((int64_t)p.dfeat_grid().x * kPxTile == p.HW && p.dfeat_bytes() > 0.0 && p.dembed_bytes() > 0.0 && p.bwd_flops() > 0.0);
        if (p.mgroups() > kGridYZ) ++g_unlaunchable;
        else REQUIRE(grid_ok(p.dembed_grid()));
    }
}

// every stride of the entry at its good value, 4 more (unaligned) and, for the frame stride, 8 and 1 short of a frame
void with_strides(const char* who, P p)
{
    exercise(who, p);
    const P base = p;
    for (const Stride& s : kStrides) {
        if (base.*s.m == 0) continue;
        for (int64_t d : {(int64_t)4, (int64_t)-8, (int64_t)-1, -(base.*s.m) - 8}) { p = base; p.*s.m += d; exercise(who, p); }
    }
}

void sweep(const char* who, E e)
{
    with_strides(who, good(e));
    for (size_t a = 0; a < kFields.size(); ++a) {
        if (!has(e, kFields[a].m)) continue;
        for (int va : kFields[a].values) {
            P p = good(e);
            p.*kFields[a].m = va;
            with_strides(who, p);
            for (size_t b = a + 1; b < kFields.size(); ++b) {
                if (!has(e, kFields[b].m)) continue;
                for (int vb : kFields[b].values) {
                    P q = p;
                    q.*kFields[b].m = vb;
                    with_strides(who, q);
                    if (e == E::planes_bwd) { q.d_features = false; exercise(who, q); q.d_embed = false; exercise(who, q); }
                }
            }
        }
    }
}

void queries()
{
    const std::vector<int> any = {-1, 0, 1, 3, 100, 129, 4128, 65535, 65536, 1 << 24, kIntMax - 127, kIntMax};
    for (int G : any) for (int Q : any) for (int T : {-1, 0, 1, 128, kIntMax}) for (int Pn : any) for (int F : {-1, 0, 1, 3, 65536, kIntMax})
        for (int rows : {-1, 0, 200, kIntMax}) {
            P p{E::cost_clip};
            p.G = G; p.Q = Q; p.Tmax = T; p.P = Pn; p.F = F; p.tsamp_rows = rows;
            const CostWs ws = p.cost_ws();
            const bool none = G <= 0 || Q <= 0 || T <= 0 || Pn <= 0 || F <= 0 || rows < 0 || (int64_t)F * Pn >= (1ll << 31);
            REQUIRE(none ? ws.total == 0 : ws.total % 256 == 0 && p.nwg() >= 1 && p.nwg() <= kRound);
            ++g_queries;
        }
    for (int N : any) for (int HW : any) for (int slots : {-1, 0, 1, 500, kIntMax}) for (int mc : any) {
        P p{E::planes_bwd};
        p.N = N; p.HW = HW; p.total_slots = slots; p.max_count = mc;
        const PairBwdWs ws = p.pair_bwd_ws();
        const bool none = N <= 0 || HW <= 0 || slots <= 0 || mc <= 0;
        REQUIRE(none ? ws.total == 0 : ws.total % 256 == 0 && p.KS() >= 1 && p.KS() <= kMaxKS && p.KP() >= mc);
        ++g_queries;
    }
}
}  // namespace

int main()
{
    sweep("mpf_match_cost_fused", E::cost);
    sweep("mpf_match_cost_fused_clip", E::cost_clip);
    sweep("mpf_pair_planes_forward", E::planes_fwd);
    sweep("mpf_pair_planes_backward", E::planes_bwd);
    queries();
    printf("mask_fused_host.h: %ld problems accepted (%ld of them with more than 65535 slot groups on grid.y of d E), %ld rejected, %ld size queries\n",
           g_ok, g_unlaunchable, g_rejected, g_queries);
    return 0;
}
