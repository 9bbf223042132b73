// The penetration depth through the C++ host mirror (include/sdfbox.hpp): Program::PenetrationParts on tests/clash_cases.py's "lens" --
// ONE loaded model at half size in two places 0.2 apart.  Built and run by tests/test_penetration.py (the argument checks, which need
// no GPU) and tests/test_gpu_penetration.py (the bytes).
//   cpp_penetration <model.asdf> <depth> <out prefix>
// writes <prefix>.penetration; prints "argument checks ok" to stderr once they are; exit 0 ok, 3 = no usable GPU, anything else = failure.
#include "sdfbox.hpp"
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
    if (argc < 4) { fprintf(stderr, "usage\n"); return 2; }
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
            p.translation[0] = k == 0 ? 0.05f : 0.25f; p.translation[1] = 0.25f; p.translation[2] = 0.25f;
            p.op = SDFHIP_COMBINE_UNION;
        }
        // what needs no GPU: no parts, a part without a model, a null Program -- exceptions, never a crash
        if (!refused([&] { Program::PenetrationParts({}); })) return 10;
        if (!refused([&] { Program::PenetrationParts(parts); })) return 11;                // nothing is loaded yet
        std::vector<Program::Part> bad = parts;
        bad[1].program = nullptr;
        if (!refused([&] { Program::PenetrationParts(bad); })) return 12;
        sdfhip_penetration_options opt;
        sdfhip_penetration_options_default(&opt);
        if (opt.size != sizeof opt || opt.flags != 0 || opt.depth != 6 || opt.origin[0] != 0.0f || opt.side != 1.0f) return 13;
        fprintf(stderr, "argument checks ok\n");

        try {
            program.Load(model);
        } catch (const Error &e) {
            if (e.code == SDFHIP_ERR_DEVICE) { fprintf(stderr, "%s\n", e.what()); return 3; }
            throw;
        }
        bad[1].program = &empty;
        if (!refused([&] { Program::PenetrationParts(bad); })) return 14;
        opt.depth = 11;
        if (!refused([&] { Program::PenetrationParts(parts, &opt); })) return 15;
        if (!refused([&] { Program::PenetrationParts(std::vector<Program::Part>(65, parts[0])); })) return 16;
        opt.depth = (uint32_t)atoi(argv[2]);
        sdfhip_penetration_stats st;
        const std::vector<sdfhip_penetration> rec = Program::PenetrationParts(parts, &opt, &st);
        if (rec.size() != 1 || st.points != (uint64_t)1 << (3 * opt.depth) || st.lookups > 2 * st.points || st.searches != 2 * (uint64_t)rec[0].points) return 17;
        FILE *f = fopen((std::string(argv[3]) + ".penetration").c_str(), "wb");
        if (!f || fwrite(rec.data(), sizeof(sdfhip_penetration), rec.size(), f) != rec.size()) return 18;
        fclose(f);
        // the skip changes no byte, and one part alone has no pair
        opt.flags = SDFHIP_PENETRATION_NO_SKIP;
        const std::vector<sdfhip_penetration> all = Program::PenetrationParts(parts, &opt, &st);
        if (all.size() != 1 || memcmp(all.data(), rec.data(), sizeof(sdfhip_penetration)) != 0 || st.lookups != 2 * st.points) return 19;
        if (!Program::PenetrationParts({ parts[0] }).empty()) return 20;
        return 0;
    } catch (const SDFbox::Error &e) {
        fprintf(stderr, "Error %d: %s\n", e.code, e.what());
        return e.code == SDFHIP_ERR_DEVICE ? 3 : 21;
    }
}
