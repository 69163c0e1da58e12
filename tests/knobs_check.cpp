// The knob table of csrc/knobs.h run on made-up environments (through its getter parameter: the process environment is never touched): the
// defaults, every parse rule at its edges, the accessors of the variables read at use at their range ends, and what the product and the
// development build (-DPSGSDF_DEV) do with the development-only variables.  Every expected value below was taken by reading the parse lines the
// table replaced, none by asking the table a second way.  Built twice with the host sanitizers and run by tests/test_host_tools.py.
#define PSGSDF_KNOB_TABLE
#include "knobs.h"
#include <map>
using namespace psge;

#define CHECK(x) do { if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

typedef std::map<std::string, std::string> Env;
static const Env* g_env = nullptr;
static const char* fake_env(const char* name) { auto it = g_env->find(name); return it == g_env->end() ? nullptr : it->second.c_str(); }

struct Parsed { bool ok; Knobs k; KnobList set, ignored; };
static Parsed parse(const Env& env) { Parsed p; g_env = &env; p.ok = knobs_parse(fake_env, p.k, p.set, p.ignored); return p; }
static bool has(const KnobList& l, const char* name, const char* value) { for (auto& kv : l) if (kv.first == name && kv.second == value) return true; return false; }

static int defaults(const Knobs& k) {
    CHECK(k.pcg_poll && k.speculate && k.speculate_mr && k.fold_in_next && k.fuse_albedo && k.fuse_pcg_init && k.pcg_persist && k.pcg_fuse_apply && k.pcg_window);
    CHECK(k.pcg_solve_rows == 0 && k.areg_device && k.fm_solve && k.fm_solve_led && k.frame_solve == 0);
    CHECK(k.xr_enable && k.xf_enable && k.xs_enable && k.xh_enable && k.xwait_spins == 16777216 && k.img_compact && k.xcd_map == 163);
    CHECK(k.ao_cut && k.compare_chunk == 16777216ll && k.query_chunk == 1073741824ll && k.cu_mask_lo == -1 && k.cu_mask_hi == -1);
    CHECK(k.pcg_ablate == 0 && k.mbox_check && k.fault_solve == 0 && k.fault_halo == 0);
    return 0;
}

int main() {
    {   // nothing set: every default, nothing reported
        const Parsed p = parse({});
        CHECK(p.ok && p.set.empty() && p.ignored.empty());
        if (defaults(p.k)) return 1;
        const std::string e = knobs_effective(p.k);
        for (const char* part : {"\"pcg_poll\": 1", "\"speculate\": 1", "\"speculate_mr\": 1", "\"fold_in_next\": 1", "\"fuse_albedo\": 1", "\"fuse_pcg_init\": 1", "\"pcg_persist\": 1",
                                 "\"pcg_fuse_apply\": 1", "\"fm_solve\": 1", "\"fm_solve_led\": 1", "\"frame_solve\": \"ldlt\"", "\"img_compact\": 1", "\"xcd_map\": 163", "\"areg_device\": 1",
                                 "\"xr\": 1", "\"xf\": 1", "\"xs\": 1", "\"xh\": 1", "\"xwait_log2\": 24", "\"cu_mask\": [-1, -1]", "\"mbox_check\": 1", "\"pcg_ablate\": 0", "\"fault_solve\": 0",
                                 "\"fault_halo\": 0", "\"ao_cut\": 1", "\"compare_chunk\": 16777216", "\"query_chunk\": 1073741824", "\"pcg_window\": 1", "\"pcg_solve_rows\": 0"})
            if (e.find(part) == std::string::npos) { printf("FAILED: effective lacks %s in %s\n", part, e.c_str()); return 1; }
    }
    {   // flags: atoi(e) != 0, so "" and "x" mean off
        struct { const char* name; bool Knobs::*m; } flags[] = {
            {"PSGSDF_PCG_POLL", &Knobs::pcg_poll}, {"PSGSDF_SPECULATE", &Knobs::speculate}, {"PSGSDF_SPECULATE_MR", &Knobs::speculate_mr}, {"PSGSDF_FOLD_IN_NEXT", &Knobs::fold_in_next},
            {"PSGSDF_FUSE_ALBEDO", &Knobs::fuse_albedo}, {"PSGSDF_FUSE_PCG_INIT", &Knobs::fuse_pcg_init}, {"PSGSDF_PCG_PERSIST", &Knobs::pcg_persist}, {"PSGSDF_PCG_FUSE_APPLY", &Knobs::pcg_fuse_apply},
            {"PSGSDF_PCG_WINDOW", &Knobs::pcg_window}, {"PSGSDF_AREG_DEVICE", &Knobs::areg_device}, {"PSGSDF_XR", &Knobs::xr_enable}, {"PSGSDF_XF", &Knobs::xf_enable}, {"PSGSDF_XS", &Knobs::xs_enable},
            {"PSGSDF_XH", &Knobs::xh_enable}, {"PSGSDF_IMG_COMPACT", &Knobs::img_compact}, {"PSGSDF_AO_CUT", &Knobs::ao_cut}};
        for (auto& f : flags) {
            struct { const char* text; bool on; } cases[] = {{"", false}, {"0", false}, {"1", true}, {"x", false}};
            for (auto& cs : cases) {
                const Parsed p = parse({{f.name, cs.text}});
                if (!p.ok || p.k.*f.m != cs.on || p.set.size() != 1 || !has(p.set, f.name, cs.text) || !p.ignored.empty()) { printf("FAILED: %s=\"%s\"\n", f.name, cs.text); return 1; }
                Knobs rest = p.k; rest.*f.m = true;      // (every flag defaults to on) nothing else moved
                if (defaults(rest)) return 1;
            }
        }
    }
    {   // PSGSDF_PCG_SOLVE_ROWS: taken only if > 0
        CHECK(parse({{"PSGSDF_PCG_SOLVE_ROWS", "0"}}).k.pcg_solve_rows == 0);
        CHECK(parse({{"PSGSDF_PCG_SOLVE_ROWS", "-3"}}).k.pcg_solve_rows == 0);
        CHECK(parse({{"PSGSDF_PCG_SOLVE_ROWS", "192"}}).k.pcg_solve_rows == 192);
        CHECK(has(parse({{"PSGSDF_PCG_SOLVE_ROWS", "-3"}}).set, "PSGSDF_PCG_SOLVE_ROWS", "-3"));      // ("env" is verbatim, taken or not)
    }
    {   // PSGSDF_FM_SOLVE: 0 off; 1 on with the LED vector; anything else on without it
        Parsed p = parse({{"PSGSDF_FM_SOLVE", "0"}}); CHECK(!p.k.fm_solve && !p.k.fm_solve_led);
        p = parse({{"PSGSDF_FM_SOLVE", "1"}}); CHECK(p.k.fm_solve && p.k.fm_solve_led);
        p = parse({{"PSGSDF_FM_SOLVE", "2"}}); CHECK(p.k.fm_solve && !p.k.fm_solve_led);
        const std::string e = knobs_effective(p.k);
        CHECK(e.find("\"fm_solve\": 1") != std::string::npos && e.find("\"fm_solve_led\": 0") != std::string::npos);
    }
    {   // PSGSDF_FRAME_SOLVE: "eigen" or "1" give 1, anything else 0
        CHECK(parse({{"PSGSDF_FRAME_SOLVE", "eigen"}}).k.frame_solve == 1 && parse({{"PSGSDF_FRAME_SOLVE", "1"}}).k.frame_solve == 1);
        CHECK(parse({{"PSGSDF_FRAME_SOLVE", "ldlt"}}).k.frame_solve == 0 && parse({{"PSGSDF_FRAME_SOLVE", "2"}}).k.frame_solve == 0 && parse({{"PSGSDF_FRAME_SOLVE", ""}}).k.frame_solve == 0);
        CHECK(knobs_effective(parse({{"PSGSDF_FRAME_SOLVE", "eigen"}}).k).find("\"frame_solve\": \"eigen\"") != std::string::npos);
    }
    {   // PSGSDF_XWAIT_LOG2: 8 .. 30 give 1 << l, anything else is ignored
        CHECK(parse({{"PSGSDF_XWAIT_LOG2", "7"}}).k.xwait_spins == 16777216);
        CHECK(parse({{"PSGSDF_XWAIT_LOG2", "8"}}).k.xwait_spins == 256);
        CHECK(parse({{"PSGSDF_XWAIT_LOG2", "30"}}).k.xwait_spins == 1073741824);
        CHECK(parse({{"PSGSDF_XWAIT_LOG2", "31"}}).k.xwait_spins == 16777216);
        CHECK(knobs_effective(parse({{"PSGSDF_XWAIT_LOG2", "30"}}).k).find("\"xwait_log2\": 30") != std::string::npos);
    }
    {   // PSGSDF_COMPARE_CHUNK: atoll clamped to 1 .. 2^24
        CHECK(parse({{"PSGSDF_COMPARE_CHUNK", "0"}}).k.compare_chunk == 1);
        CHECK(parse({{"PSGSDF_COMPARE_CHUNK", "1"}}).k.compare_chunk == 1);
        CHECK(parse({{"PSGSDF_COMPARE_CHUNK", "16777216"}}).k.compare_chunk == 16777216ll);
        CHECK(parse({{"PSGSDF_COMPARE_CHUNK", "16777217"}}).k.compare_chunk == 16777216ll);
        CHECK(parse({{"PSGSDF_COMPARE_CHUNK", "4096"}}).k.compare_chunk == 4096);
    }
    {   // PSGSDF_QUERY_CHUNK: a whole decimal number, a multiple of 64 in 64 .. 2^30; anything else refuses the context
        Parsed p = parse({{"PSGSDF_QUERY_CHUNK", "64"}}); CHECK(p.ok && p.k.query_chunk == 64);
        p = parse({{"PSGSDF_QUERY_CHUNK", "128"}}); CHECK(p.ok && p.k.query_chunk == 128);
        p = parse({{"PSGSDF_QUERY_CHUNK", "1073741824"}}); CHECK(p.ok && p.k.query_chunk == 1073741824ll);
        for (const char* bad : {"100", "63", "128x", "", "1073741888", "0", "-64"}) if (parse({{"PSGSDF_QUERY_CHUNK", bad}}).ok) { printf("FAILED: PSGSDF_QUERY_CHUNK=\"%s\" accepted\n", bad); return 1; }
    }
    {   // PSGSDF_CU_MASK: "%d:%d" with 0 <= lo < hi (hi against the device: psgsdf_create)
        Parsed p = parse({{"PSGSDF_CU_MASK", "0:8"}}); CHECK(p.ok && p.k.cu_mask_lo == 0 && p.k.cu_mask_hi == 8);
        CHECK(knobs_effective(p.k).find("\"cu_mask\": [0, 8]") != std::string::npos);
        p = parse({{"PSGSDF_CU_MASK", "128:256"}}); CHECK(p.ok && p.k.cu_mask_lo == 128 && p.k.cu_mask_hi == 256);
        for (const char* bad : {"8:8", "-1:4", "4", "", "9:8"}) if (parse({{"PSGSDF_CU_MASK", bad}}).ok) { printf("FAILED: PSGSDF_CU_MASK=\"%s\" accepted\n", bad); return 1; }
    }
    {   // PSGSDF_XCD_MAP is any atoi; PSGSDF_XCD_STRIPE goes on top of it, the map first: (xcd_map & 255) | (v << 8)
        CHECK(parse({{"PSGSDF_XCD_MAP", "3"}}).k.xcd_map == 3 && parse({{"PSGSDF_XCD_MAP", "0"}}).k.xcd_map == 0 && parse({{"PSGSDF_XCD_MAP", "-1"}}).k.xcd_map == -1);
        CHECK(parse({{"PSGSDF_XCD_STRIPE", "2"}}).k.xcd_map == 675);                                 // 163 | 2 << 8
        CHECK(parse({{"PSGSDF_XCD_MAP", "3"}, {"PSGSDF_XCD_STRIPE", "2"}}).k.xcd_map == 515);        // 3 | 2 << 8
        CHECK(parse({{"PSGSDF_XCD_MAP", "771"}, {"PSGSDF_XCD_STRIPE", "1"}}).k.xcd_map == 259);      // the map's own bits 8 and up give way: 3 | 1 << 8
        CHECK(knobs_effective(parse({{"PSGSDF_XCD_MAP", "3"}, {"PSGSDF_XCD_STRIPE", "2"}}).k).find("\"xcd_map\": 515") != std::string::npos);
    }
    {   // the variables read at use: their accessors at the range ends, and "env" still lists them (they move no member)
        auto with = [](const char* name, const char* text) { static Env e; e = Env{{name, text}}; g_env = &e; };
        static const Env none; g_env = &none;
        CHECK(knob_fm_rows(fake_env) == 0 && knob_pcg_rows(fake_env) == 1 && knob_pcg_blocks(768, fake_env) == 768 && knob_pcg_col16(fake_env) && knob_xr_mem(fake_env) == 0);
        CHECK(knob_wait_timeout_s(fake_env) == 120.0 && knob_destroy_timeout_s(fake_env) == 15.0 && knob_socket_timeout_s(fake_env) == 120.0 && knob_solve_dump(fake_env) == nullptr);
        with("PSGSDF_FM_ROWS", "3"); CHECK(knob_fm_rows(fake_env) == 0);
        with("PSGSDF_FM_ROWS", "4"); CHECK(knob_fm_rows(fake_env) == 4);
        with("PSGSDF_FM_ROWS", "64"); CHECK(knob_fm_rows(fake_env) == 64);
        with("PSGSDF_FM_ROWS", "65"); CHECK(knob_fm_rows(fake_env) == 0);
        with("PSGSDF_PCG_ROWS", "0"); CHECK(knob_pcg_rows(fake_env) == 1);
        with("PSGSDF_PCG_ROWS", "1"); CHECK(knob_pcg_rows(fake_env) == 1);
        with("PSGSDF_PCG_ROWS", "2"); CHECK(knob_pcg_rows(fake_env) == 2);
        with("PSGSDF_PCG_ROWS", "3"); CHECK(knob_pcg_rows(fake_env) == 1);
        with("PSGSDF_PCG_BLOCKS", "0"); CHECK(knob_pcg_blocks(768, fake_env) == 768);
        with("PSGSDF_PCG_BLOCKS", "1"); CHECK(knob_pcg_blocks(768, fake_env) == 1);
        with("PSGSDF_PCG_BLOCKS", "768"); CHECK(knob_pcg_blocks(768, fake_env) == 768);
        with("PSGSDF_PCG_BLOCKS", "769"); CHECK(knob_pcg_blocks(768, fake_env) == 768);
        with("PSGSDF_PCG_BLOCKS", "500"); CHECK(knob_pcg_blocks(768, fake_env) == 500);
        with("PSGSDF_PCG_COL16", "0"); CHECK(!knob_pcg_col16(fake_env));
        with("PSGSDF_PCG_COL16", "1"); CHECK(knob_pcg_col16(fake_env));
        with("PSGSDF_PCG_COL16", ""); CHECK(!knob_pcg_col16(fake_env));      // (atoi: numerically 0)
        with("PSGSDF_XR_MEM", "fine"); CHECK(knob_xr_mem(fake_env) == 1);
        with("PSGSDF_XR_MEM", "uncached"); CHECK(knob_xr_mem(fake_env) == 2);
        with("PSGSDF_XR_MEM", "coarse"); CHECK(knob_xr_mem(fake_env) == 3);
        with("PSGSDF_XR_MEM", "Fine"); CHECK(knob_xr_mem(fake_env) == 0);
        with("PSGSDF_WAIT_TIMEOUT_S", "0"); CHECK(knob_wait_timeout_s(fake_env) == 120.0);
        with("PSGSDF_WAIT_TIMEOUT_S", "-5"); CHECK(knob_wait_timeout_s(fake_env) == 120.0);
        with("PSGSDF_WAIT_TIMEOUT_S", "0.5"); CHECK(knob_wait_timeout_s(fake_env) == 0.5);
        with("PSGSDF_DESTROY_TIMEOUT_S", "0"); CHECK(knob_destroy_timeout_s(fake_env) == 0.0);
        with("PSGSDF_DESTROY_TIMEOUT_S", "2.5"); CHECK(knob_destroy_timeout_s(fake_env) == 2.5);
        with("PSGSDF_SOCKET_TIMEOUT_S", "3"); CHECK(knob_socket_timeout_s(fake_env) == 3.0);
        with("PSGSDF_SOLVE_DUMP", "/tmp/x"); CHECK(knob_solve_dump(fake_env) && !strcmp(knob_solve_dump(fake_env), "/tmp/x"));
        const Env all = {{"PSGSDF_FM_ROWS", "999"}, {"PSGSDF_PCG_ROWS", "2"}, {"PSGSDF_PCG_BLOCKS", "7"}, {"PSGSDF_PCG_COL16", "0"}, {"PSGSDF_XR_MEM", "bogus"},
                         {"PSGSDF_WAIT_TIMEOUT_S", "1"}, {"PSGSDF_DESTROY_TIMEOUT_S", "1"}, {"PSGSDF_SOCKET_TIMEOUT_S", "1"}, {"PSGSDF_SOLVE_DUMP", "d"}};
        const Parsed p = parse(all);
        CHECK(p.ok && p.set.size() == 9 && p.ignored.empty());
        for (auto& kv : all) CHECK(has(p.set, kv.first.c_str(), kv.second.c_str()));
        if (defaults(p.k)) return 1;
    }
    {   // a name the table does not know is nobody's business
        const Parsed p = parse({{"PSGSDF_NO_SUCH_KNOB", "1"}, {"PSGSDF_BENCH_STEPS", "3"}});
        CHECK(p.ok && p.set.empty() && p.ignored.empty());
    }
    {   // the development-only variables
        const Env dev = {{"PSGSDF_PCG_ABLATE", "7"}, {"PSGSDF_MBOX_CHECK", "0"}, {"PSGSDF_FAULT_SOLVE", "3"}, {"PSGSDF_FAULT_HALO", "5000000000"}, {"PSGSDF_PCG_PERSIST", "0"}};
        const Parsed p = parse(dev);
        CHECK(p.ok && has(p.set, "PSGSDF_PCG_PERSIST", "0") && !p.k.pcg_persist);
#ifdef PSGSDF_DEV      // honoured, and reported with the rest
        CHECK(p.k.pcg_ablate == 5 && !p.k.mbox_check && p.k.fault_solve == 3 && p.k.fault_halo == 5000000000ll);      // (PCG_ABLATE: & 5)
        CHECK(p.ignored.empty() && p.set.size() == 5);
        for (auto& kv : dev) CHECK(has(p.set, kv.first.c_str(), kv.second.c_str()));
        CHECK(knobs_effective(p.k).find("\"fault_halo\": 5000000000") != std::string::npos);
        CHECK(parse({{"PSGSDF_PCG_ABLATE", "2"}}).k.pcg_ablate == 0 && parse({{"PSGSDF_PCG_ABLATE", "4"}}).k.pcg_ablate == 4 && parse({{"PSGSDF_MBOX_CHECK", "1"}}).k.mbox_check);
        printf("dev ");
#else                  // left at their defaults, and said so
        CHECK(p.k.pcg_ablate == 0 && p.k.mbox_check && p.k.fault_solve == 0 && p.k.fault_halo == 0);
        CHECK(p.set.size() == 1 && p.ignored.size() == 4);
        for (auto& kv : dev) if (kv.first != "PSGSDF_PCG_PERSIST") CHECK(has(p.ignored, kv.first.c_str(), kv.second.c_str()));
        printf("product ");
#endif
    }
    printf("ok\n");
    return 0;
}
