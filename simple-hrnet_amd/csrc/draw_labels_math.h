// The arithmetic of the person labels (include/hrnet_mi355.h: hrn_draw_labels_dev, hrn_label_layout, hrn_label_covers), written
// ONCE for the host and the device: the glyph table, the record of one person, the function that builds it from (box, id, score,
// scale, thickness) and the function that classifies a pixel against it are compiled into the kernels of draw.hip, into the two
// host entries, and into the stand-alone program of tests/test_labels_host.py (a plain C++ compiler: nothing of HIP is needed).
// Integer arithmetic throughout; the one floating-point step, the percent of a score, is two float32 operations with fp
// contraction off -- the same bits on both sides.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define HRN_LABEL_FN __host__ __device__ inline
#else
#define HRN_LABEL_FN inline
#endif

namespace hrn {

constexpr int kLabelLo = -8192, kLabelHi = 16383;   // a drawn box has all four coordinates in [kLabelLo, kLabelHi]
constexpr int kLabelMaxScale = 16, kLabelMaxThickness = 16;
constexpr int kLabelMaxCells = 14;                  // 10 id digits, one blank, 3 percent digits
constexpr unsigned kLabelBlank = 15u;               // a cell's four bits: 0 .. 9 the digit, 15 a blank

// 5 columns x 7 rows, rows top to bottom, bit 4 = the leftmost column: the HD44780 digit set
HRN_LABEL_FN unsigned label_glyph_row(int digit, int row) {
    static constexpr unsigned char rows[10][7] = {
        {0x0E, 0x11, 0x13, 0x15, 0x19, 0x11, 0x0E}, {0x04, 0x0C, 0x04, 0x04, 0x04, 0x04, 0x0E}, {0x0E, 0x11, 0x01, 0x02, 0x04, 0x08, 0x1F},
        {0x1F, 0x02, 0x04, 0x02, 0x01, 0x11, 0x0E}, {0x02, 0x06, 0x0A, 0x12, 0x1F, 0x02, 0x02}, {0x1F, 0x10, 0x1E, 0x01, 0x01, 0x11, 0x0E},
        {0x06, 0x08, 0x10, 0x1E, 0x11, 0x11, 0x0E}, {0x1F, 0x01, 0x02, 0x04, 0x08, 0x08, 0x08}, {0x0E, 0x11, 0x11, 0x0E, 0x11, 0x11, 0x0E},
        {0x0E, 0x11, 0x11, 0x0F, 0x01, 0x02, 0x0C}};
    return rows[digit][row];
}

// One person's label: 16 int32, the layout of hrn_label_record.  Everything a pixel test needs, nothing of the frame.
struct LabelRecord {
    int32_t drawn;                        // 0: nothing of this person is drawn (every other field is 0)
    int32_t x1, y1, x2, y2;               // the outline rectangle, both corners inclusive
    int32_t thickness;                    // T: the outline is the rectangle minus its interior shrunk by T (T = 0: none)
    int32_t left, top, width, height;     // the plate: left <= px < left + width, top <= py < top + height (no cells: all 0)
    int32_t scale;                        // s: a glyph dot is s x s pixels
    int32_t ncells;                       // D in [0, 14]
    uint32_t cells_lo, cells_hi;          // cell k: four bits at 4 k of (cells_hi : cells_lo)
    uint32_t colour, text_colour;         // three bytes each, byte 0 first; hrn_label_layout leaves them 0 (it knows no palette)
};
static_assert(sizeof(LabelRecord) == 64, "hrn_label_record");

enum { LABEL_NONE = 0, LABEL_COLOUR = 1, LABEL_TEXT = 2 };   // what label_covers answers

HRN_LABEL_FN unsigned label_cell(const LabelRecord &r, int k) { return ((k < 8 ? r.cells_lo >> (4 * k) : r.cells_hi >> (4 * (k - 8)))) & 15u; }

// the percent of a score: v < 0 -> 0, v > 1 -> 1, then (int)(v * 100.0f + 0.5f), each operation rounded once; NaN: -1 (no field)
HRN_LABEL_FN int label_percent(float score) {
#pragma clang fp contract(off)
    if (score != score) return -1;
    const float v = score < 0.0f ? 0.0f : (score > 1.0f ? 1.0f : score);
    const float scaled = v * 100.0f;
    const float lifted = scaled + 0.5f;
    return (int)lifted;
}

// Python's modulo of a colour index: never negative
HRN_LABEL_FN int label_colour_index(int c, int count) {
    const int m = c % count;
    return m < 0 ? m + count : m;
}

// The record of one person from (box, id, score, scale s in [1, 16], thickness T in [0, 16]); the colours stay 0.
HRN_LABEL_FN LabelRecord label_layout(const int32_t box[4], bool has_id, int32_t id, bool has_score, float score, int s, int T) {
    LabelRecord r = {};
    const int x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
    const bool in_range = x1 >= kLabelLo && x1 <= kLabelHi && y1 >= kLabelLo && y1 <= kLabelHi && x2 >= kLabelLo && x2 <= kLabelHi &&
                          y2 >= kLabelLo && y2 <= kLabelHi;
    if (!in_range || x2 <= x1 || y2 <= y1) return r;
    r.drawn = 1, r.x1 = x1, r.y1 = y1, r.x2 = x2, r.y2 = y2, r.thickness = T, r.scale = s;
    // the cells, most significant digit first
    unsigned cells[kLabelMaxCells];
    int D = 0;
    const auto digits = [&](uint32_t value) {
        unsigned rev[10];
        int count = 0;
        do rev[count++] = value % 10u, value /= 10u;
        while (value != 0u);
        while (count > 0) cells[D++] = rev[--count];
    };
    if (has_id && id >= 0) digits((uint32_t)id);
    const int p = has_score ? label_percent(score) : -1;
    if (p >= 0) {
        if (D > 0) cells[D++] = kLabelBlank;
        digits((uint32_t)p);
    }
    r.ncells = D;
    for (int k = 0; k < D; ++k) {
        if (k < 8) r.cells_lo |= cells[k] << (4 * k);
        else r.cells_hi |= cells[k] << (4 * (k - 8));
    }
    if (D > 0) {
        r.width = s * (6 * D + 1), r.height = 9 * s;
        r.left = x1, r.top = y1 - 9 * s >= 0 ? y1 - 9 * s : y1;   // above the box when it fits the frame's top, else inside
    }
    return r;
}

// the pixels a record can touch: outline and plate, both corners inclusive; false: none (reach = (1, 1, 0, 0))
HRN_LABEL_FN bool label_reach(const LabelRecord &r, int32_t reach[4]) {
    const bool outline = r.drawn && r.thickness > 0, plate = r.drawn && r.ncells > 0;
    reach[0] = reach[1] = 1, reach[2] = reach[3] = 0;
    if (outline) reach[0] = r.x1, reach[1] = r.y1, reach[2] = r.x2, reach[3] = r.y2;
    if (plate) {
        const int px2 = r.left + r.width - 1, py2 = r.top + r.height - 1;
        if (!outline) {
            reach[0] = r.left, reach[1] = r.top, reach[2] = px2, reach[3] = py2;
        } else {
            reach[0] = r.left < reach[0] ? r.left : reach[0], reach[1] = r.top < reach[1] ? r.top : reach[1];
            reach[2] = px2 > reach[2] ? px2 : reach[2], reach[3] = py2 > reach[3] ? py2 : reach[3];
        }
    }
    return outline || plate;
}

// The highest primitive of the record on pixel (px, py): ink (LABEL_TEXT), else plate or outline (LABEL_COLOUR), else LABEL_NONE.
HRN_LABEL_FN int label_covers(const LabelRecord &r, int px, int py) {
    if (!r.drawn) return LABEL_NONE;
    if (r.ncells > 0 && px >= r.left && px < r.left + r.width && py >= r.top && py < r.top + r.height) {
        const int s = r.scale;
        const int a = px - r.left - s, v = py - r.top - s;   // a: from the first cell's left edge
        if (a >= 0 && v >= 0 && v < 7 * s) {
            const int k = a / (6 * s), u = a - k * 6 * s;    // cell k starts at s (1 + 6 k); u < 6 s, the last s of it is the gap
            if (k < r.ncells && u < 5 * s) {
                const unsigned d = label_cell(r, k);
                if (d < 10u && ((label_glyph_row((int)d, v / s) >> (4 - u / s)) & 1u)) return LABEL_TEXT;
            }
        }
        return LABEL_COLOUR;
    }
    const int T = r.thickness;
    if (T > 0 && px >= r.x1 && px <= r.x2 && py >= r.y1 && py <= r.y2 &&
        !(px >= r.x1 + T && px <= r.x2 - T && py >= r.y1 + T && py <= r.y2 - T))
        return LABEL_COLOUR;
    return LABEL_NONE;
}

}  // namespace hrn
