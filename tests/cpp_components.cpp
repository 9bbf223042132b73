// The components of a scene through the C++ host mirror (include/sdfbox.hpp): Program::Components on ONE loaded model.  Built and run
// by tests/test_components.py (the argument checks, which need no GPU) and tests/test_gpu_components.py (the bytes).
//   cpp_components <model.asdf> <depth> <out prefix>
// writes <prefix>.components and <prefix>.labels; prints "argument checks ok" to stderr once they are; exit 0 ok, 3 = no usable GPU,
// anything else = failure.
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

template <class T> static bool written(const std::string &path, const std::vector<T> &v)
{
    FILE *f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    if (f) fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage\n"); return 2; }
    try {
        Logic logic;
        OctData model = logic.MakeData(argv[1]);
        Program program;
        // what needs no GPU: nothing is loaded yet -- an exception, never a crash
        if (!refused([&] { program.Components(); })) return 10;
        sdfhip_components_options opt;
        sdfhip_components_options_default(&opt);
        if (opt.size != sizeof opt || opt.flags != 0 || opt.depth != 6 || opt.origin[0] != 0.0f || opt.side != 1.0f) return 11;
        uint32_t n = 77;
        if (sdfhip_scene_components(nullptr, &opt, nullptr, 0, &n, nullptr, nullptr) != SDFHIP_ERR_ARG || n != 77) return 12;
        fprintf(stderr, "argument checks ok\n");

        try {
            program.Load(model);
        } catch (const Error &e) {
            if (e.code == SDFHIP_ERR_DEVICE) { fprintf(stderr, "%s\n", e.what()); return 3; }
            throw;
        }
        opt.depth = 10;
        if (!refused([&] { program.Components(&opt); })) return 13;
        opt.depth = (uint32_t)atoi(argv[2]);
        opt.flags = 1;
        if (!refused([&] { program.Components(&opt); })) return 14;
        opt.flags = 0;
        sdfhip_components_stats st;
        std::vector<uint32_t> labels;
        const std::vector<sdfhip_component> rec = program.Components(&opt, &labels, &st);
        const uint64_t points = (uint64_t)1 << (3 * opt.depth);
        if (rec.empty() || st.points != points || st.components != rec.size() || labels.size() != points) return 15;
        uint64_t sum = 0, inside = 0;
        uint32_t solids = 0;
        for (const sdfhip_component &c : rec) {
            sum += c.points;
            if (c.flags & SDFHIP_COMPONENT_SOLID) { inside += c.points; solids++; }
            if (labels[c.label] != c.label) return 16;
        }
        if (sum != points || inside != st.inside || solids != st.solids) return 17;
        if (!written(std::string(argv[3]) + ".components", rec) || !written(std::string(argv[3]) + ".labels", labels)) return 18;
        // without labels, and a second time: the same bytes
        const std::vector<sdfhip_component> again = program.Components(&opt);
        if (again.size() != rec.size() || memcmp(again.data(), rec.data(), rec.size() * sizeof(sdfhip_component)) != 0) return 19;
        return 0;
    } catch (const SDFbox::Error &e) {
        fprintf(stderr, "Error %d: %s\n", e.code, e.what());
        return e.code == SDFHIP_ERR_DEVICE ? 3 : 21;
    }
}
