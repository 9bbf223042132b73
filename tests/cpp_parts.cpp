// An assembly drawn, picked and sampled without baking through the C++ host mirror (include/sdfbox.hpp): Program::DrawParts,
// PickParts and SampleParts on tests/instances_cases.py's "two_spheres" -- ONE loaded model at half size in two places.  Built and
// run by tests/test_gpu_instances.py.
//   cpp_parts <model.asdf> <W> <H> <pixels.bin: n x {x, y} uint32> <points.bin: n x 3 float> <out prefix>
// writes <prefix>.frame, <prefix>.hits and <prefix>.probes; exit 0 ok, 3 = no usable GPU, anything else = failure.
#include "sdfbox.hpp"
#include <cstdio>
#include <cstring>
#include <string>

template <class T> static std::vector<T> read_all(const char *path)
{
    std::vector<T> out;
    FILE *f = fopen(path, "rb");
    if (!f) return out;
    T item;
    while (fread(&item, sizeof item, 1, f) == 1) out.push_back(item);
    fclose(f);
    return out;
}
template <class T> static bool write_all(const std::string &path, const std::vector<T> &v)
{
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
    fclose(f);
    return ok;
}

int main(int argc, char **argv)
{
    if (argc < 7) { fprintf(stderr, "usage\n"); return 2; }
    using namespace SDFbox;
    try {
        Logic logic;
        OctData model = logic.MakeData(argv[1]);
        const int W = atoi(argv[2]), H = atoi(argv[3]);
        logic.Resize(W, H);
        logic.SetHeading(0.0f, 0.0f);
        logic.SetPosition(0.5f, 0.5f, 0.1f);
        Program program;
        try {
            program.Load(model);
        } catch (const Error &e) {
            if (e.code == SDFHIP_ERR_DEVICE) { fprintf(stderr, "%s\n", e.what()); return 3; }
            throw;
        }
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
        const std::string prefix = argv[6];
        const std::vector<float> frame = Program::DrawParts(parts, logic.State, (uint32_t)W, (uint32_t)H);
        if (frame.size() != (size_t)W * H * 4 || !write_all(prefix + ".frame", frame)) return 12;
        const std::vector<sdfhip_part_hit> hits = Program::PickParts(parts, logic.State, read_all<uint32_t>(argv[4]));
        if (hits.empty() || !write_all(prefix + ".hits", hits)) return 13;
        const std::vector<sdfhip_part_probe> probes = Program::SampleParts(parts, read_all<float>(argv[5]));
        if (probes.empty() || !write_all(prefix + ".probes", probes)) return 14;
        // the options travel: one step cannot converge from outside, and the skip changes no byte
        sdfhip_instances_options opt = { (uint32_t)sizeof(sdfhip_instances_options), SDFHIP_INSTANCES_NO_SKIP, 0, 0.0f };
        const std::vector<float> all = Program::DrawParts(parts, logic.State, (uint32_t)W, (uint32_t)H, &opt);
        if (all.size() != frame.size() || memcmp(all.data(), frame.data(), frame.size() * 4) != 0) return 15;
        opt.max_steps = 1;
        const std::vector<sdfhip_part_hit> one = Program::PickParts(parts, logic.State, { (uint32_t)W / 2, (uint32_t)H / 2 }, &opt);
        if (one.size() != 1 || one[0].steps != 1 || one[0].status != SDFHIP_QUERY_EXHAUSTED) return 16;
        // the loaded model is still the source: nothing was adopted
        std::vector<float> own;
        program.Draw(logic.State, W, H, own);
        if (own.size() != frame.size() || memcmp(own.data(), frame.data(), frame.size() * 4) == 0) return 17;
        try {                                      // a part without a model: an exception, never a crash
            Program empty;
            parts[1].program = &empty;
            Program::DrawParts(parts, logic.State, 8, 8);
            return 18;
        } catch (const Error &e) {
            if (e.code != SDFHIP_ERR_ARG) return 19;
        }
        return 0;
    } catch (const SDFbox::Error &e) {
        fprintf(stderr, "Error %d: %s\n", e.code, e.what());
        return e.code == SDFHIP_ERR_DEVICE ? 3 : 20;
    }
}
