// Selection through the C++ host mirror (include/sdfbox.hpp): Program::Select on ONE loaded model.  Built and run by
// tests/test_gpu_select.py.
//   cpp_select <model.asdf> <lattice depth> <out prefix>
// flips the model's largest solid (SDFHIP_SELECT_FLIP_LISTED of the label Program::Components gives it) and writes the result's host
// arrays to <prefix>.structs and <prefix>.values; prints "argument checks ok" to stderr once they are; exit 0 ok, 3 = no usable GPU,
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

static bool written(const std::string &path, const void *data, size_t bytes)
{
    FILE *f = fopen(path.c_str(), "wb");
    const bool ok = f && fwrite(data, 1, bytes, f) == bytes;
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
        if (!refused([&] { program.Select(); })) return 10;
        sdfhip_select_options opt;
        sdfhip_select_options_default(&opt);
        if (opt.size != sizeof opt || opt.flags != 0 || opt.lattice_depth != 6 || opt.origin[0] != 0.0f || opt.side != 1.0f || opt.depth != -1 ||
            opt.min_points != 0)
            return 11;
        sdfhip_scene *out = reinterpret_cast<sdfhip_scene *>(&opt);
        if (sdfhip_scene_select(nullptr, &opt, nullptr, 0, &out, nullptr, nullptr) != SDFHIP_ERR_ARG || out != reinterpret_cast<sdfhip_scene *>(&opt)) return 12;
        fprintf(stderr, "argument checks ok\n");

        try {
            program.Load(model);
        } catch (const Error &e) {
            if (e.code == SDFHIP_ERR_DEVICE) { fprintf(stderr, "%s\n", e.what()); return 3; }
            throw;
        }
        opt.lattice_depth = 10;
        if (!refused([&] { program.Select(&opt); })) return 13;
        opt.lattice_depth = (uint32_t)atoi(argv[2]);
        opt.flags = 32;
        if (!refused([&] { program.Select(&opt); })) return 14;
        opt.flags = SDFHIP_SELECT_FLIP_LISTED;
        if (!refused([&] { program.Select(&opt); })) return 15;                 // a listed rule and no list
        sdfhip_components_options lattice;
        sdfhip_components_options_default(&lattice);
        lattice.depth = opt.lattice_depth;
        const std::vector<sdfhip_component> rec = program.Components(&lattice);
        const sdfhip_component *largest = nullptr;
        for (const sdfhip_component &c : rec)
            if ((c.flags & SDFHIP_COMPONENT_SOLID) && (!largest || c.points > largest->points)) largest = &c;
        if (!largest) return 16;
        sdfhip_select_stats st;
        sdfhip_octdata host = {};
        program.Select(&opt, {largest->label, largest->label}, &st, &host);
        const bool ok = st.components == rec.size() && st.flipped_solids == 1 && st.flipped_voids == 0 && st.points_flipped == largest->points &&
                        st.nodes_out == host.length &&
                        written(std::string(argv[3]) + ".structs", host.structs, (size_t)host.length * 8) &&
                        written(std::string(argv[3]) + ".values", host.values, (size_t)host.length * 8);
        sdfhip_octdata_free(&host);
        return ok ? 0 : 17;
    } catch (const SDFbox::Error &e) {
        fprintf(stderr, "Error %d: %s\n", e.code, e.what());
        return e.code == SDFHIP_ERR_DEVICE ? 3 : 21;
    }
}
