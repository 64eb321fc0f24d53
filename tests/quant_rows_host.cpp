// Host build of csrc/rca_quant_rows.h (TEST INFRASTRUCTURE ONLY): the functions the device kernels call, run on the CPU so that their
// arithmetic can be compared with tests/quant_search_ref.py, and their indexing checked under AddressSanitizer / UBSan, without a card.
//   quant_rows_host TYPE RULE ROWS K IN.f32 OUT.bin     TYPE: 2 q8_0, 4 q4_k, 6 q5_k, 5 q6_k (the RCA_* dtype numbers)
// prints "status <or of the blocks' status bits> first_bad_input_row <row or -1> first_bad_d_row <row or -1>"
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rca_quant_rows.h"

int main(int argc, char** argv) {
    if (argc != 7) return 2;
    const int type = atoi(argv[1]), rule = atoi(argv[2]);
    const long rows = atol(argv[3]), K = atol(argv[4]);
    std::vector<float> x((size_t)(rows * K));
    FILE* f = fopen(argv[5], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 3;
    fclose(f);
    const long nv = type == 2 ? 32 : 256, bs = type == 2 ? 34 : (type == 4 ? 144 : (type == 6 ? 176 : 210));
    const long nb = rows * K / nv, bpr = K / nv;
    std::vector<unsigned> words((size_t)((nb * bs + 3) / 4));      // exactly the blocks: a write past them is an ASan report
    unsigned char* out = (unsigned char*)words.data();
    int status = 0;
    long bad_in = -1, bad_d = -1;
    for (long b = 0; b < nb; ++b) {
        int s;
        if (type == 4) s = rca_quant::quantize_block_qk<15>(x.data() + b * nv, rule, (unsigned*)(out + b * bs));
        else if (type == 6) s = rca_quant::quantize_block_qk<31>(x.data() + b * nv, rule, (unsigned*)(out + b * bs));
        else if (type == 5) s = rca_quant::quantize_block_q6k(x.data() + b * nv, rule, (unsigned short*)(out + b * bs));
        else s = rca_quant::quantize_block_q8_0(x.data() + b * nv, (unsigned short*)(out + b * bs));
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
