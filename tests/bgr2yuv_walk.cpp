// csrc/yuv_fwd.h alone, compiled for the host by a plain C++ compiler with AddressSanitizer and UBSan (tests/test_bgr2yuv_host.py):
// the blocks at which the sums of the BGR -> YCbCr conversion are extreme -- all 0, all 255, and per row of the table the block that
// maximises and the block that minimises its sum -- for every table and depth.  Signed overflow ends the program (UBSan), so a clean
// exit says that every sum fits int32.  One line per block: matrix range depth, the twelve input bytes, Y00 Y01 Y10 Y11 U V.
#include <stdint.h>
#include <stdio.h>

#include "yuv_fwd.h"

int main() {
    for (int matrix = 0; matrix < 2; ++matrix)
        for (int range = 0; range < 2; ++range) {
            int32_t c[hrn::kYuvFwdCoefs];
            if (!hrn::yuv_forward_table(matrix, range, c)) return 1;
            for (int depth = 8; depth <= 10; depth += 2)
                for (int k = 0; k < 8; ++k) {   // 0: all 0; 1: all 255; 2 + 2 row + side: the row's maximiser / minimiser
                    uint8_t px[3];              // (B, G, R) of all four pixels
                    for (int ch = 0; ch < 3; ++ch) {
                        if (k < 2) {
                            px[ch] = k ? 255 : 0;
                        } else {
                            const int row = (k - 2) / 2, coef = c[1 + 3 * row + (2 - ch)];   // the table's rows are (R, G, B)
                            px[ch] = ((coef > 0) == ((k & 1) == 0)) ? 255 : 0;
                        }
                    }
                    uint8_t bgr[12];
                    for (int p = 0; p < 4; ++p)
                        for (int ch = 0; ch < 3; ++ch) bgr[3 * p + ch] = px[ch];
                    uint16_t out[6];
                    hrn::yuv_fwd_block(c, depth == 10, bgr, out);
                    printf("%d %d %d", matrix, range, depth);
                    for (int b = 0; b < 12; ++b) printf(" %d", bgr[b]);
                    for (int s = 0; s < 6; ++s) printf(" %d", out[s]);
                    printf("\n");
                }
        }
    return hrn::yuv_forward_table(2, 0, nullptr) || hrn::yuv_forward_table(0, -1, nullptr) ? 1 : 0;
}
