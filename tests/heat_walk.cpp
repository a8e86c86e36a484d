// Stand-alone walk of csrc/heat_math.h for tests/test_heatmaps_host.py: compiled by a plain C++ compiler with
// -fsanitize=address,undefined -ffp-contract=off and run as a child process.  Reads cases from the file named on the command
// line, whitespace-separated integers per case:
//     format(0 BGR | 2 I420) H W hq wq n J alpha mode cutoff lo_bits hi_bits
//     J mask entries, n boxes of 4, n*J*hq*wq map values, 768 colour-table bytes
// (lo_bits, hi_bits and the map values: the float32's bits as unsigned integers, so that NaN, infinities and the neighbours of a
// half-step arrive exactly).  The canvas is packed and synthetic: byte i of the buffer is (131 i + 17) & 255.  Per case it prints
//     fnv1a64(Q) fnv1a64(V) written_pixels fnv1a64(the drawn buffer)
// The test compares the lines with tests/heat_ref.py; the sanitizers watch every path on the way.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "heat_math.h"

static unsigned long long fnv(const uint8_t *p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

static bool next(FILE *in, long long *v) { return std::fscanf(in, "%lld", v) == 1; }

static float as_float(long long bits) {
    const uint32_t b = (uint32_t)bits;
    float f;
    std::memcpy(&f, &b, sizeof(f));
    return f;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *in = std::fopen(argv[1], "r");
    if (!in) return 2;
    int lines = 0;
    long long head[12];
    while (next(in, &head[0])) {
        for (int k = 1; k < 12; ++k)
            if (!next(in, &head[k])) return 3;
        const int fmt = (int)head[0], H = (int)head[1], W = (int)head[2], hq = (int)head[3], wq = (int)head[4], n = (int)head[5], J = (int)head[6];
        const int alpha = (int)head[7], mode = (int)head[8], cutoff = (int)head[9];
        const float lo = as_float(head[10]), hi = as_float(head[11]);
        const float k = 255.0f / (hi - lo);
        const int cells = hq * wq;
        long long v;
        std::vector<uint8_t> mask(J), lut(768);
        std::vector<int32_t> boxes((size_t)4 * n);
        std::vector<float> maps((size_t)n * J * cells);
        for (auto &m : mask) {
            if (!next(in, &v)) return 3;
            m = (uint8_t)v;
        }
        for (auto &b : boxes) {
            if (!next(in, &v)) return 3;
            b = (int32_t)v;
        }
        for (auto &m : maps) {
            if (!next(in, &v)) return 3;
            m = as_float(v);
        }
        for (auto &c : lut) {
            if (!next(in, &v)) return 3;
            c = (uint8_t)v;
        }
        // 1. reduce and quantise
        std::vector<uint8_t> Q((size_t)n * cells);
        for (int i = 0; i < n; ++i)
            for (int c = 0; c < cells; ++c) {
                float best = __builtin_nanf("");
                for (int j = 0; j < J; ++j)
                    if (mask[j]) best = hrn::heat_max(best, maps[((size_t)i * J + j) * cells + c]);
                Q[(size_t)i * cells + c] = (uint8_t)hrn::heat_quantise(best, lo, k);
            }
        // 2., 3. sample and combine
        std::vector<uint8_t> V((size_t)H * W, 0);
        for (int i = 0; i < n; ++i) {
            const int32_t *b = &boxes[(size_t)4 * i];
            if (!hrn::heat_box_drawn(b[0], b[1], b[2], b[3])) continue;
            for (int py = b[1] > 0 ? b[1] : 0; py < (b[3] < H ? b[3] : H); ++py)
                for (int px = b[0] > 0 ? b[0] : 0; px < (b[2] < W ? b[2] : W); ++px) {
                    const int S = hrn::heat_sample(&Q[(size_t)i * cells], hq, wq, hrn::heat_coord(px - b[0], wq, b[2] - b[0]),
                                                   hrn::heat_coord(py - b[1], hq, b[3] - b[1]));
                    if (S < 0 || S > 255) return 4;
                    if (S > V[(size_t)py * W + px]) V[(size_t)py * W + px] = (uint8_t)S;
                }
        }
        // 4. blend into the synthetic canvas
        const size_t bytes = fmt == 0 ? (size_t)H * W * 3 : (size_t)H * W * 3 / 2;
        std::vector<uint8_t> canvas(bytes);
        for (size_t i = 0; i < bytes; ++i) canvas[i] = (uint8_t)((131 * i + 17) & 255);
        long written = 0;
        if (fmt == 0) {
            for (size_t p = 0; p < (size_t)H * W; ++p) {
                int a;
                if (!hrn::heat_written(V[p], alpha, mode, cutoff, &a)) continue;
                ++written;
                for (int ch = 0; ch < 3; ++ch) canvas[3 * p + ch] = (uint8_t)hrn::heat_blend(canvas[3 * p + ch], lut[3 * V[p] + ch], a);
            }
        } else {
            uint8_t *Y = canvas.data(), *U = Y + (size_t)H * W, *Vp = U + (size_t)(H / 2) * (W / 2);
            for (int by = 0; by < H / 2; ++by)
                for (int bx = 0; bx < W / 2; ++bx) {
                    int v4[4];
                    bool any = false;
                    for (int p = 0; p < 4; ++p) {
                        const size_t at = (size_t)(2 * by + (p >> 1)) * W + 2 * bx + (p & 1);
                        v4[p] = V[at];
                        int a;
                        if (!hrn::heat_written(v4[p], alpha, mode, cutoff, &a)) continue;
                        ++written, any = true;
                        Y[at] = (uint8_t)hrn::heat_blend(Y[at], lut[3 * v4[p]], a);
                    }
                    if (!any) continue;
                    const int vc = hrn::heat_block_value(v4[0], v4[1], v4[2], v4[3]), ac = hrn::heat_alpha(vc, alpha, mode);
                    if (ac <= 0) continue;
                    const size_t at = (size_t)by * (W / 2) + bx;
                    U[at] = (uint8_t)hrn::heat_blend(U[at], lut[3 * vc + 1], ac);
                    Vp[at] = (uint8_t)hrn::heat_blend(Vp[at], lut[3 * vc + 2], ac);
                }
        }
        std::printf("%llu %llu %ld %llu\n", fnv(Q.data(), Q.size()), fnv(V.data(), V.size()), written, fnv(canvas.data(), canvas.size()));
        ++lines;
    }
    std::fclose(in);
    return lines > 0 ? 0 : 2;
}
