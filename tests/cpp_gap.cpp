// The clearance through the C++ host mirror (include/sdfbox.hpp): Program::GapParts on tests/gap_cases.py's "apart" -- ONE loaded model
// at half size in two places 0.4 apart.  Built and run by tests/test_gap.py (the argument checks, which need no GPU) and
// tests/test_gpu_gap.py (the bytes).
//   cpp_gap <model.asdf> <out prefix>
// writes <prefix>.gap; prints "argument checks ok" to stderr once they are; exit 0 ok, 3 = no usable GPU, anything else = failure.
#include "sdfbox.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

using namespace SDFbox;

// the call must throw an Error with SDFHIP_ERR_ARG
template <class Call> static bool refused(Call call)
{
    try {
        call();
    } catch (const Error &e) {
        return e.code == SDFHIP_ERR_ARG;
    }
    return false;
}

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage\n"); return 2; }
    try {
        Logic logic;
        OctData model = logic.MakeData(argv[1]);
        Program program, empty;
        std::vector<Program::Part> parts(2);
        for (int k = 0; k < 2; k++) {
            Program::Part &p = parts[k];
            p.program = &program;
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) p.rotation[i][j] = i == j ? 1.0f : 0.0f;
            p.scale = 0.5f;
            p.translation[0] = k == 0 ? 0.05f : 0.45f; p.translation[1] = 0.25f; p.translation[2] = 0.25f;
            p.op = SDFHIP_COMBINE_UNION;
        }
        // what needs no GPU: no parts, a part without a model, a null Program -- exceptions, never a crash
        if (!refused([&] { Program::GapParts({}); })) return 10;
        if (!refused([&] { Program::GapParts(parts); })) return 11;                // nothing is loaded yet
        std::vector<Program::Part> bad = parts;
        bad[1].program = nullptr;
        if (!refused([&] { Program::GapParts(bad); })) return 12;
        sdfhip_gap_options opt;
        sdfhip_gap_options_default(&opt);
        if (opt.size != sizeof opt || opt.flags != 0 || !(opt.limit > 3.0e38f)) return 13;
        fprintf(stderr, "argument checks ok\n");

        try {
            program.Load(model);
        } catch (const Error &e) {
            if (e.code == SDFHIP_ERR_DEVICE) { fprintf(stderr, "%s\n", e.what()); return 3; }
            throw;
        }
        bad[1].program = &empty;
        if (!refused([&] { Program::GapParts(bad); })) return 14;
        opt.limit = -1.0f;
        if (!refused([&] { Program::GapParts(parts, &opt); })) return 15;
        opt.limit = NAN;
        if (!refused([&] { Program::GapParts(parts, &opt); })) return 15;
        if (!refused([&] { Program::GapParts(std::vector<Program::Part>(65, parts[0])); })) return 16;
        sdfhip_gap_options_default(&opt);
        sdfhip_gap_stats st;
        const std::vector<sdfhip_gap> rec = Program::GapParts(parts, &opt, &st);
        if (rec.size() != 1 || st.pairs != 1 || st.pairs_searched != 1 || st.searches == 0 || st.visited < st.searches) return 17;
        FILE *f = fopen((std::string(argv[2]) + ".gap").c_str(), "wb");
        if (!f || fwrite(rec.data(), sizeof(sdfhip_gap), rec.size(), f) != rec.size()) return 18;
        fclose(f);
        // no pruning changes no byte and runs every candidate; a limit below the gap leaves no record; one part alone has no pair
        opt.flags = SDFHIP_GAP_NO_PRUNE;
        sdfhip_gap_stats all_st;
        const std::vector<sdfhip_gap> all = Program::GapParts(parts, &opt, &all_st);
        if (all.size() != 1 || memcmp(all.data(), rec.data(), sizeof(sdfhip_gap)) != 0 || all_st.searches < st.searches) return 19;
        opt.flags = 0;
        opt.limit = rec[0].gap * 0.5f;
        if (!Program::GapParts(parts, &opt).empty()) return 20;
        opt.limit = rec[0].gap;
        if (Program::GapParts(parts, &opt).size() != 1) return 21;
        if (!Program::GapParts({ parts[0] }).empty()) return 22;
        return 0;
    } catch (const SDFbox::Error &e) {
        fprintf(stderr, "Error %d: %s\n", e.code, e.what());
        return e.code == SDFHIP_ERR_DEVICE ? 3 : 23;
    }
}
