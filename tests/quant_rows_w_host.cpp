// Host build of the weighted rules of csrc/rca_quant_rows.h (TEST INFRASTRUCTURE ONLY): what rca_quantize_rows_w's kernel calls per
// block, with the lane's own indexing of the weights (block `blk` reads weights + (blk % blocks_per_row) * 256), run on the CPU so that
// the arithmetic can be compared with tests/quant_weighted_ref.py and the indexing checked under AddressSanitizer / UBSan.
//   quant_rows_w_host TYPE ROWS K IN.f32 WEIGHTS.f32 OUT.bin     TYPE: 4 q4_k, 6 q5_k, 5 q6_k (the RCA_* dtype numbers)
// prints "status <or of the blocks' status bits> first_bad_input_row <row or -1> first_bad_d_row <row or -1>"
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rca_quant_rows.h"

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int type = atoi(argv[1]);
    const long rows = atol(argv[2]), K = atol(argv[3]);
    if (type != 4 && type != 5 && type != 6) return 2;
    std::vector<float> x((size_t)(rows * K)), qw((size_t)K);      // exactly K weights: a lane indexing them by block reads past them
    FILE* f = fopen(argv[4], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 3;
    fclose(f);
    f = fopen(argv[5], "rb");
    if (!f || fread(qw.data(), 4, qw.size(), f) != qw.size()) return 3;
    fclose(f);
    const long bs = type == 4 ? 144 : (type == 6 ? 176 : 210);
    const long nb = rows * K / 256, bpr = K / 256;
    std::vector<unsigned> words((size_t)((nb * bs + 3) / 4));
    unsigned char* out = (unsigned char*)words.data();
    int status = 0;
    long bad_in = -1, bad_d = -1;
    for (long b = 0; b < nb; ++b) {
        const float* w = qw.data() + (b % bpr) * 256;
        int s;
        if (type == 4) s = rca_quant::quantize_block_qk<15>(x.data() + b * 256, 1, (unsigned*)(out + b * bs), w);
        else if (type == 6) s = rca_quant::quantize_block_qk<31>(x.data() + b * 256, 1, (unsigned*)(out + b * bs), w);
        else s = rca_quant::quantize_block_q6k(x.data() + b * 256, 1, (unsigned short*)(out + b * bs), w);
        status |= s;
        if ((s & rca_quant::QS_BAD_INPUT) && bad_in < 0) bad_in = b / bpr;
        if ((s & rca_quant::QS_BAD_D) && bad_d < 0) bad_d = b / bpr;
    }
    f = fopen(argv[6], "wb");
    if (!f || fwrite(out, 1, (size_t)(nb * bs), f) != (size_t)(nb * bs)) return 4;
    fclose(f);
    printf("status %d first_bad_input_row %ld first_bad_d_row %ld\n", status, bad_in, bad_d);
    return 0;
}
