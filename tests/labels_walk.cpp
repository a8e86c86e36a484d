// Stand-alone walk of csrc/draw_labels_math.h for tests/test_labels_host.py: compiled by a plain C++ compiler with
// -fsanitize=address,undefined and run as a child process.  Reads cases from the file named on the command line, one per line:
//     x1 y1 x2 y2 has_id id has_score score_bits scale thickness window_x window_y
// (score_bits: the float32's bits as an unsigned integer, so that NaN and the neighbours of 0.005 arrive exactly), classifies
// every pixel of a 64 x 96 window at (window_x, window_y) and prints per case
//     drawn ncells pixels_in_colour pixels_in_text_colour fnv1a64_of_the_classes
// The test compares the lines with tests/label_ref.py; the sanitizers watch every path on the way.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "draw_labels_math.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *in = std::fopen(argv[1], "r");
    if (!in) return 2;
    long long v[12];
    int lines = 0;
    while (std::fscanf(in, "%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5], &v[6],
                       &v[7], &v[8], &v[9], &v[10], &v[11]) == 12) {
        const int32_t box[4] = {(int32_t)v[0], (int32_t)v[1], (int32_t)v[2], (int32_t)v[3]};
        const uint32_t bits = (uint32_t)v[7];
        float score;
        std::memcpy(&score, &bits, sizeof(score));
        const hrn::LabelRecord r = hrn::label_layout(box, v[4] != 0, (int32_t)v[5], v[6] != 0, score, (int)v[8], (int)v[9]);
        int32_t reach[4];
        const bool any = hrn::label_reach(r, reach);
        unsigned long long hash = 1469598103934665603ull;
        long colour = 0, text = 0;
        for (int y = 0; y < 64; ++y)
            for (int x = 0; x < 96; ++x) {
                const int px = (int)v[10] + x, py = (int)v[11] + y;
                const int cls = hrn::label_covers(r, px, py);
                if (cls != hrn::LABEL_NONE && !(any && px >= reach[0] && px <= reach[2] && py >= reach[1] && py <= reach[3])) {
                    std::fprintf(stderr, "case %d: pixel (%d, %d) is covered outside the record's reach\n", lines, px, py);
                    return 3;
                }
                colour += cls == hrn::LABEL_COLOUR, text += cls == hrn::LABEL_TEXT;
                hash = (hash ^ (unsigned long long)cls) * 1099511628211ull;
            }
        std::printf("%d %d %ld %ld %llu\n", (int)r.drawn, (int)r.ncells, colour, text, hash);
        ++lines;
    }
    std::fclose(in);
    return lines > 0 ? 0 : 2;
}
