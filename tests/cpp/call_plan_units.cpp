// call_plan_units.cpp -- the call plan (csrc/call_plan.cpp, with sizing.cpp and walk_plan.cpp) run without a device.
//   call_plan_units golden <file>         every line of tests/golden/call_plan_cases.txt -- a search call traced on a device: its inputs and
//                                         the kernels that ran -- through call_plan(): the same first pass, grid, LDS, retry action, re-rank
//                                         (the file's byte_handle= / walk_bytes= keys: CallFacts::rows / walked of kind U8)
//   call_plan_units grid <dims> <beams>   the conditions the plan guarantees by construction, over dims x beams (comma lists) x both metrics x
//                                         nq in {96, 2 048, 16 384} x untagged / tagged / byte-walk / half-base / half-walk calls x no history / a calm history
//   call_plan_units walkgrid <dims> <beams>  plan_walk() over the cross product of every input it reads (walk_grid below): the plan count and one
//                                         digest of the formatted plans per (feature variant, pass), compared with tests/golden/walk_plan_grid.txt
// Built by tests/test_call_plan_units.py from the three units' sources; the kernel tables' names (walk_plan_name), the visited set's byte counts
// and the knob defaults come from the library.  No HIP call.
#include "../../gbnns_dim_red_amd/csrc/call_plan.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

using namespace gbnns;
using namespace gbnns_api;

namespace gbnns_api { Knobs knob_defaults(); }

static int g_failed = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++g_failed; std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static size_t first_lds(const CallPlan& p) {
    return p.first.lds_fixed + (p.bitmap_pass ? 0 : walk_hash_bytes(p.hash_cap, p.first.hash_form(p.vs_shr)));
}

static bool same_walk_plan(const WalkPlan& a, const WalkPlan& b) {
    return a.pass == b.pass && a.inst == b.inst && a.lds_fixed == b.lds_fixed && a.packed == b.packed && a.knows_quotient == b.knows_quotient && a.lds_list == b.lds_list &&
           a.coop_serves == b.coop_serves && a.general_only == b.general_only && a.rr_base == b.rr_base && a.rr_in_table == b.rr_in_table;
}
static bool same_plan(const CallPlan& a, const CallPlan& b) {
    return a.skey == b.skey && a.coop == b.coop && a.late_rows == b.late_rows && a.spec_rows == b.spec_rows && a.all_general == b.all_general && a.force_wide == b.force_wide &&
           a.generic_only == b.generic_only && a.spec_from == b.spec_from && a.vs_shr == b.vs_shr && a.hash_cap == b.hash_cap && a.hash_limit == b.hash_limit &&
           a.rr_reserve == b.rr_reserve && a.bytes_dim == b.bytes_dim && same_walk_plan(a.first, b.first) && a.bitmap_pass == b.bitmap_pass && a.bitmap_per_cu == b.bitmap_per_cu &&
           a.fuse == b.fuse && a.skip_retry == b.skip_retry && a.retry_action == b.retry_action && same_walk_plan(a.retry, b.retry) && a.retry_hash_cap == b.retry_hash_cap &&
           a.retry_hash_limit == b.retry_hash_limit && a.sizing.auto_cap == b.sizing.auto_cap && a.sizing.form == b.sizing.form && a.sizing.cap == b.sizing.cap;
}

// ---- golden: "key=value;key=value;..." per line --------------------------------------------------------------------------------------------
static int golden(const char* path) {
    std::ifstream in(path);
    if (!in) { std::printf("cannot read %s\n", path); return 2; }
    std::string line;
    int lines = 0;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::map<std::string, std::string> kv;
        std::stringstream ss(line);
        std::string item;
        while (std::getline(ss, item, ';')) {
            const size_t eq = item.find('=');
            if (eq != std::string::npos) kv[item.substr(0, eq)] = item.substr(eq + 1);
        }
        auto num = [&](const char* k) { return std::strtoll(kv.at(k).c_str(), nullptr, 10); };
        CallFacts f{};
        f.metric = (int)num("metric"); f.n = (uint64_t)num("n"); f.d = (uint32_t)num("d"); f.d_pad = (uint32_t)num("d_pad"); f.ell_stride = (uint32_t)num("ell_stride");
        f.aux_stride = 0; f.rows = num("byte_handle") != 0 ? RowKind::U8 : RowKind::F32; f.cus = (size_t)num("cus"); f.knob = knob_defaults(); f.knob.hot = (int)num("hot");
        f.dim = (uint32_t)num("dim"); f.dstride = (uint32_t)num("dstride"); f.half_rows = false; f.walked = num("walk_bytes") != 0 ? RowKind::U8 : RowKind::F32; f.byte_queries = false;
        f.mode = (int)num("mode"); f.ef = (int)num("ef"); f.n_entries = (uint32_t)num("n_entries"); f.flags = (uint32_t)num("flags"); f.hash_capacity = (int32_t)num("hash_capacity");
        f.nq = (uint32_t)num("nq"); f.tagged = num("tagged") != 0; f.bridged = false; f.in_flight = num("in_flight") != 0; f.sync_host = num("sync_host") != 0;
        const CallPlan p = call_plan(f, SizingHistory{});
        SizingHistory h;
        if (num("h_cap") >= 0) {  // the class's history before this call
            h.cap_for_ef[p.skey] = (uint32_t)num("h_cap"); h.maxdc_for_ef[p.skey] = (uint32_t)num("h_maxdc"); h.calm_streak[p.skey] = (int)num("h_calm");
        }
        const CallPlan q = call_plan(f, h);
        const std::string id = kv.at("case") + " call " + kv.at("call");
        const char* planned = q.all_general ? "walk_general_kernel" : walk_plan_name(q.first);
        CHECK(planned && kv.at("first") == planned, "%s: first pass %s, traced %s", id.c_str(), planned ? planned : "(none)", kv.at("first").c_str());
        const long long wg = q.first.inst.family == WalkFamily::Coop ? 128 : 64;
        const long long grid = q.all_general ? 0 : (q.bitmap_pass ? (long long)(q.bitmap_per_cu * f.cus) : (long long)f.nq) * wg;
        CHECK(grid == num("grid"), "%s: grid %lld, traced %lld", id.c_str(), grid, num("grid"));
        if (num("lds") >= 0) CHECK((long long)first_lds(q) == num("lds"), "%s: LDS %zu, recorded %lld", id.c_str(), first_lds(q), num("lds"));
        const char* rn = q.retry_action == RetryAction::Launch ? walk_plan_name(q.retry) : nullptr;
        const std::string retry = q.retry_action == RetryAction::Launch ? (rn ? rn : "(none)") : (q.retry_action == RetryAction::Copy ? "copy" : "none");
        CHECK(retry == kv.at("retry"), "%s: retry %s, traced %s", id.c_str(), retry.c_str(), kv.at("retry").c_str());
        const bool rerank = f.mode != GBNNS_MODE_PLAIN && !q.fuse;
        CHECK(rerank == (num("rerank") != 0), "%s: stand-alone re-rank %d, traced %lld", id.c_str(), (int)rerank, num("rerank"));
        ++lines;
    }
    std::printf("golden: %d lines, %d failed\n", lines, g_failed);
    return (g_failed || lines == 0) ? 1 : 0;
}

// ---- grid ------------------------------------------------------------------------------------------------------------------------------------
static std::vector<int> ints(const char* csv) {
    std::vector<int> v;
    std::stringstream ss(csv);
    std::string item;
    while (std::getline(ss, item, ',')) v.push_back(std::atoi(item.c_str()));
    return v;
}

static void check_one(const CallFacts& f, const SizingHistory& h, const char* what) {
    const SizingHistory before = h;
    const CallPlan p = call_plan(f, h);
    char id[160];
    std::snprintf(id, sizeof id, "%s metric %d dim %u ef %d nq %u", what, f.metric, f.dim, f.ef, f.nq);
    CHECK(h == before, "%s: the history changed", id);
    CHECK(same_plan(p, call_plan(f, h)), "%s: two plans from the same inputs", id);
    CHECK(p.all_general || first_lds(p) <= kMaxLds, "%s: first pass on %zu bytes of LDS", id, first_lds(p));
    if (p.fuse) {
        const size_t room = p.first.rr_room(walk_hash_bytes(p.hash_cap, p.first.hash_form(p.vs_shr)));
        CHECK(!p.first.lds_list && (size_t)f.d_pad * 4 <= room, "%s: fused with room for %zu bytes", id, room);
    }
    if (p.bitmap_pass) CHECK(!p.coop && !f.tagged && f.walked == RowKind::F32 && p.bitmap_per_cu > 0, "%s: bitmap pass", id);
    if (f.rows == RowKind::F16 && f.mode != GBNNS_MODE_PLAIN) CHECK(!p.fuse, "%s: a half-base handle's re-rank fused", id);  // (a stand-alone re-rank follows)
    if (p.skip_retry) CHECK(p.sizing.auto_cap && !p.all_general && p.retry_action == RetryAction::None, "%s: skip_retry", id);
    if (p.all_general) CHECK(p.retry_action == RetryAction::None && !p.bitmap_pass, "%s: all_general with a pass of its own", id);
    if (!p.all_general) CHECK(walk_plan_name(p.first) != nullptr, "%s: no instance for the first pass", id);
    if (p.retry_action == RetryAction::Launch) CHECK(walk_plan_name(p.retry) != nullptr && p.retry_hash_cap > p.sizing.cap, "%s: retry launch", id);
}

static int grid(const char* dims_csv, const char* beams_csv) {
    int plans = 0;
    static const char* const kinds[] = {"untagged", "tagged", "byte walk", "half base", "half walk"};
    for (int kind = 0; kind < 5; ++kind)  // untagged LOWQ, tagged LOWQ, PLAIN byte walk, a half-base handle's LOWQ, PLAIN half walk
        for (int metric = 0; metric < 2; ++metric)
            for (int dim : ints(dims_csv))
                for (int ef : ints(beams_csv))
                    for (uint32_t nq : {96u, 2048u, 16384u})
                        for (int calm = 0; calm < 2; ++calm) {
                            CallFacts f{};
                            f.metric = metric; f.n = 20000; f.ell_stride = 32; f.cus = 256; f.knob = knob_defaults();
                            f.ef = ef; f.n_entries = 1; f.nq = nq; f.sync_host = true;
                            if (kind == 2) {
                                f.rows = f.walked = RowKind::U8; f.mode = GBNNS_MODE_PLAIN;
                                f.d = f.dim = (uint32_t)dim; f.d_pad = f.dstride = row_pad((uint32_t)dim, f.rows);
                            } else if (kind == 4) {
                                f.rows = f.walked = RowKind::F16; f.mode = GBNNS_MODE_PLAIN;
                                f.d = f.dim = (uint32_t)dim; f.d_pad = f.dstride = row_pad((uint32_t)dim, f.rows);
                            } else {
                                f.d = f.d_pad = 128; f.dim = (uint32_t)dim; f.dstride = ((uint32_t)dim + 3u) / 4u * 4u;
                                f.mode = GBNNS_MODE_LOWQ; f.tagged = kind == 1; f.rows = kind == 3 ? RowKind::F16 : RowKind::F32;
                            }
                            SizingHistory h;
                            if (calm) {  // a settled class: three quiet batches whose longest walk computed 30 ef distances
                                const int skey = call_plan(f, h).skey;
                                const uint32_t maxdc = 30u * (uint32_t)ef;
                                h.maxdc_for_ef[skey] = maxdc; h.cap_for_ef[skey] = (maxdc + maxdc / 16 + 64) / 15 * 16 + 16; h.calm_streak[skey] = 3;
                            }
                            check_one(f, h, kinds[kind]);
                            ++plans;
                        }
    std::printf("grid: %d plans, %d failed\n", plans, g_failed);
    return (g_failed || plans == 0) ? 1 : 0;
}

// ---- walkgrid --------------------------------------------------------------------------------------------------------------------------------
// Eighteen feature variants over an otherwise zeroed WalkParams; `dim` is the grid's dimension (dstride = dim rounded up to 4; "walk_half unkept": to 8).
static const char* const kVariants[] = {"plain", "coop", "late_rows", "spec_rows", "half_rows", "tagged", "tagged+bridged", "generic_only", "bytes_dim=128", "bytes_dim=40",
                                        "walk_bytes d=128", "walk_bytes q_b classes=7", "walk_bytes q_b classes=2", "stamps_on", "rr_reserve=160",
                                        "walk_half d=96", "walk_half unkept", "walk_half general"};
constexpr int kNumVariants = (int)(sizeof kVariants / sizeof kVariants[0]);
static void set_variant(WalkParams& p, int v) {
    static const uint8_t byte_queries[16] = {0};
    switch (v) {
        case 1: p.coop = 1; break;
        case 2: p.late_rows = 1; break;
        case 3: p.spec_rows = 1; break;
        case 4: p.half_rows = 1; break;
        case 5: p.tagged = 1; break;
        case 6: p.tagged = 1; p.bridged = 1; break;
        case 7: p.generic_only = 1; break;
        case 8: p.bytes_dim = 128; break;
        case 9: p.bytes_dim = 40; break;
        case 10: p.walk_bytes = 1; p.dim = p.dstride = 128; break;
        case 11: p.walk_bytes = 1; p.q_b = byte_queries; p.bq_classes = 7; break;
        case 12: p.walk_bytes = 1; p.q_b = byte_queries; p.bq_classes = 2; break;
        case 13: p.stamps_on = 1; break;
        case 14: p.rr_reserve = 160; break;
        case 15: p.walk_half = 1; p.dim = p.dstride = 96; break;
        case 16: p.walk_half = 1; p.half_unkept = 1; p.dstride = (p.dim + 7u) / 8u * 8u; break;
        case 17: p.walk_half = 1; p.half_general = 1; break;
        default: break;
    }
}

static int walk_grid(const char* dims_csv, const char* beams_csv) {
    static const uint32_t aux_rows[16] = {0};
    static const char* const pass_names[] = {"First", "Bitmap", "Retry"};
    const WalkEnv envs[] = {{true, false}, {false, true}};  // {wide2, stamps_generic}
    const std::vector<int> dims = ints(dims_csv), beams = ints(beams_csv);
    long long plans = 0;
    std::string lines;
    for (int v = 0; v < kNumVariants; ++v)
        for (int pass = 0; pass < 3; ++pass) {
            uint64_t digest = 0xcbf29ce484222325ull;  // FNV-1a, 64 bits, over the lines of this (variant, pass)
            for (const WalkEnv& env : envs)
                for (int metric = 0; metric < 2; ++metric)
                    for (int dim : dims)
                        for (uint32_t n : {3000u, 0xFEFFFFu, 0xFF0000u, 0x1000000u})  // either side of the two-wavefront walk's limit and of the 24-bit ids
                            for (uint32_t ell : {32u, 64u, 96u})
                                for (int aux = 0; aux < 2; ++aux)
                                    for (int ef : beams)
                                        for (uint32_t entries = 1; entries <= 2; ++entries)
                                            for (int wide = 0; wide < 2; ++wide) {
                                                WalkParams p{};
                                                p.dim = (uint32_t)dim; p.dstride = ((uint32_t)dim + 3u) / 4u * 4u; p.n = n; p.ell_stride = ell; p.ef = ef;
                                                p.n_entries = entries; p.force_wide = wide;
                                                if (aux) { p.aux_ell = aux_rows; p.aux_stride = 16; }
                                                set_variant(p, v);
                                                const WalkPlan pl = plan_walk(p, metric, (WalkPass)pass, env);
                                                const char* name = walk_plan_name(pl);
                                                char line[512];
                                                const int len = std::snprintf(line, sizeof line, "%s %d %zu %d %d %d %d %d %zu %d\n", name ? name : "-", (int)pl.inst.family, pl.lds_fixed,
                                                                              (int)pl.packed, (int)pl.knows_quotient, (int)pl.lds_list, (int)pl.coop_serves, (int)pl.general_only,
                                                                              pl.rr_base, (int)pl.rr_in_table);
                                                for (int i = 0; i < len; ++i) digest = (digest ^ (unsigned char)line[i]) * 0x100000001b3ull;
                                                ++plans;
                                            }
            char out[128];
            std::snprintf(out, sizeof out, "%s | %s | %016llx\n", kVariants[v], pass_names[pass], (unsigned long long)digest);
            lines += out;
        }
    std::printf("walkgrid: %lld plans\n%s", plans, lines.c_str());
    return plans == 0 ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::string(argv[1]) == "golden") return golden(argv[2]);
    if (argc == 4 && std::string(argv[1]) == "grid") return grid(argv[2], argv[3]);
    if (argc == 4 && std::string(argv[1]) == "walkgrid") return walk_grid(argv[2], argv[3]);
    std::printf("usage: call_plan_units golden <file> | grid <dims> <beams> | walkgrid <dims> <beams>\n");
    return 2;
}
