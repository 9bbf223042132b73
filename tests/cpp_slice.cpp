// Program::Slice through the C++ host mirror (include/sdfbox.hpp).  Built and run by tests/test_cpp_slice.py.
//   cpp_slice <model.asdf> <out records.raw> <out counts.raw>
// slices the model with the stack (0.6, 0, 0.8), 0.3 + 0.05 k, k < 12, and writes the records (node-major) and the layers' counts.
// exit 0 ok, 3 = no usable GPU, anything else = failure.
#include "sdfbox.hpp"
#include <cstdio>

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage\n"); return 2; }
    using namespace SDFbox;
    try {
        Logic logic;
        OctData model = logic.MakeData(argv[1]);
        Program program;
        try {
            program.Load(model);
        } catch (const Error &e) {
            if (e.code == SDFHIP_ERR_DEVICE) { fprintf(stderr, "%s\n", e.what()); return 3; }
            throw;
        }
        const float normal[3] = { 0.6f, 0.0f, 0.8f };
        std::vector<uint32_t> counts;
        sdfhip_slice_stats stats;
        const std::vector<sdfhip_segment> segs = program.Slice(normal, 0.3f, 0.05f, 12, -1, &counts, &stats);
        if (stats.n_segments != segs.size() || counts.size() != 12) return 10;
        if (program.Slice(normal, 5.0f).size() != 0) return 11;                       // a plane outside the cube, the defaults for the rest
        try {
            program.Slice(normal, 0.3f, 0.0f, 2);                                     // two layers and no pitch
            return 12;
        } catch (const Error &e) {
            if (e.code != SDFHIP_ERR_ARG) return 13;
        }
        FILE *f = fopen(argv[2], "wb");
        if (!f || fwrite(segs.data(), sizeof(sdfhip_segment), segs.size(), f) != segs.size()) return 14;
        fclose(f);
        f = fopen(argv[3], "wb");
        if (!f || fwrite(counts.data(), 4, counts.size(), f) != counts.size()) return 15;
        fclose(f);
        printf("segments %zu\n", segs.size());
        return 0;
    } catch (const Error &e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
