// Stand-alone walk of csrc/mosaic_math.h for tests/test_mosaic_host.py: compiled by a plain C++ compiler with
// -fsanitize=address,undefined and run as a child process.  Reads cases from the file named on the command line,
// whitespace-separated integers per case:
//     format(0 BGR | 1 NV12 | 2 I420) H W cell n J K threshold_bits scale_num scale_den min_half
//     J > 0: K joint indices, then n*J*3 values of pts (y, x, confidence);  J == 0: n boxes of 4
// (threshold_bits and the pts values: the float32's bits as unsigned integers, so that NaN, infinities and fractions arrive
// exactly).  The canvas is packed and synthetic: byte i of the buffer is (131 i + 17) & 255.  Per case it prints
//     fnv1a64(regions as int32) fnv1a64(status as int32) cell_size marked_cells checksum(the changed buffer)
// with checksum = sum of byte[i] * (i % 65521 + 1) modulo 2^64.  The test compares the lines with tests/mosaic_ref.py; the
// sanitizers watch every path on the way.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mosaic_math.h"

static unsigned long long fnv(const void *data, size_t n) {
    const uint8_t *p = (const uint8_t *)data;
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

// one channel of a marked cell: its first byte, the bytes between rows and between samples, its rows and columns
static void flatten(uint8_t *first, size_t pitch, size_t step, int rows, int cols, int count) {
    int sum = 0;
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) sum += first[y * pitch + x * step];
    const int m = hrn::mosaic_mean(sum, count);
    for (int y = 0; y < rows; ++y)
        for (int x = 0; x < cols; ++x) first[y * pitch + x * step] = (uint8_t)m;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *in = std::fopen(argv[1], "r");
    if (!in) return 2;
    int lines = 0;
    long long head[11];
    while (next(in, &head[0])) {
        for (int k = 1; k < 11; ++k)
            if (!next(in, &head[k])) return 3;
        const int fmt = (int)head[0], H = (int)head[1], W = (int)head[2], cell = (int)head[3], n = (int)head[4], J = (int)head[5], K = (int)head[6];
        const float threshold = as_float(head[7]);
        const int num = (int)head[8], den = (int)head[9], min_half = (int)head[10];
        if (!hrn::mosaic_cell_valid(cell)) return 4;
        long long v;
        uint32_t bits[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        std::vector<float> pts((size_t)n * J * 3);
        std::vector<int32_t> boxes(J ? 0 : (size_t)4 * n);
        for (int k = 0; k < (J ? K : 0); ++k) {
            if (!next(in, &v) || v < 0 || v >= J) return 3;
            bits[v >> 5] |= 1u << (v & 31);
        }
        for (auto &p : pts) {
            if (!next(in, &v)) return 3;
            p = as_float(v);
        }
        for (auto &b : boxes) {
            if (!next(in, &v)) return 3;
            b = (int32_t)v;
        }
        // regions and status
        std::vector<int32_t> region((size_t)4 * n), status(n);
        for (int i = 0; i < n; ++i) {
            int out[4];
            status[i] = J ? hrn::mosaic_region_of_person(&pts[(size_t)i * J * 3], J, bits, threshold, num, den, min_half, H, W, out)
                          : hrn::mosaic_region_of_box(&boxes[(size_t)4 * i], H, W, out);
            for (int k = 0; k < 4; ++k) region[(size_t)4 * i + k] = out[k];
            if ((status[i] == hrn::MOSAIC_OK) != (out[2] > out[0] && out[3] > out[1])) return 5;
            if (out[0] < 0 || out[1] < 0 || out[2] > W || out[3] > H) return 5;
        }
        // marks: every cell against every region
        const int s = hrn::mosaic_cell_size(cell, H, W), gw = (W + s - 1) / s, gh = (H + s - 1) / s;
        std::vector<uint8_t> marks((size_t)gw * gh, 0);
        long marked = 0;
        for (int cy = 0; cy < gh; ++cy)
            for (int cx = 0; cx < gw; ++cx) {
                for (int i = 0; i < n && !marks[(size_t)cy * gw + cx]; ++i) {
                    const int32_t *r = &region[(size_t)4 * i];
                    marks[(size_t)cy * gw + cx] = hrn::mosaic_meets(r[0], r[1], r[2], r[3], cx * s, cy * s, s);
                }
                marked += marks[(size_t)cy * gw + cx];
            }
        // means into the synthetic canvas
        const size_t bytes = fmt == 0 ? (size_t)H * W * 3 : (size_t)H * W * 3 / 2;
        std::vector<uint8_t> canvas(bytes);
        for (size_t i = 0; i < bytes; ++i) canvas[i] = (uint8_t)((131 * i + 17) & 255);
        uint8_t *Y = canvas.data(), *U = Y + (size_t)H * W, *V = U + (size_t)(H / 2) * (W / 2);
        for (int cy = 0; cy < gh; ++cy)
            for (int cx = 0; cx < gw; ++cx) {
                if (!marks[(size_t)cy * gw + cx]) continue;
                const int x0 = cx * s, y0 = cy * s, w = hrn::mosaic_min(s, W - x0), h = hrn::mosaic_min(s, H - y0);
                const int c = hrn::mosaic_cell_count(x0, y0, s, H, W);
                if (c != w * h || c < 1) return 6;
                if (fmt == 0) {
                    for (int ch = 0; ch < 3; ++ch) flatten(Y + ((size_t)y0 * W + x0) * 3 + ch, (size_t)W * 3, 3, h, w, c);
                    continue;
                }
                flatten(Y + (size_t)y0 * W + x0, W, 1, h, w, c);
                if (fmt == 1) {
                    flatten(U + (size_t)(y0 / 2) * W + x0, W, 2, h / 2, w / 2, c / 4);
                    flatten(U + (size_t)(y0 / 2) * W + x0 + 1, W, 2, h / 2, w / 2, c / 4);
                } else {
                    flatten(U + (size_t)(y0 / 2) * (W / 2) + x0 / 2, W / 2, 1, h / 2, w / 2, c / 4);
                    flatten(V + (size_t)(y0 / 2) * (W / 2) + x0 / 2, W / 2, 1, h / 2, w / 2, c / 4);
                }
            }
        unsigned long long sum = 0;
        for (size_t i = 0; i < bytes; ++i) sum += (unsigned long long)canvas[i] * (i % 65521 + 1);
        std::printf("%llu %llu %d %ld %llu\n", fnv(region.data(), region.size() * 4), fnv(status.data(), status.size() * 4), s, marked, sum);
        ++lines;
    }
    std::fclose(in);
    return lines > 0 ? 0 : 2;
}
