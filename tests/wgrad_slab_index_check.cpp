// Stand-alone check of csrc/wgrad_slab_index.h (the slab flush of k_conv_wgrad_kd and the read / write indices of k_wgrad_reduce_kd), built by
// tests/test_host_wgrad_kd_slab.py with -fsanitize=address,undefined and run on the host: every index is used on heap buffers of EXACTLY the
// sizes the launcher assumes, so an index one element out of range is a sanitizer report, and the images are checked for being permutations.
//   argv: Cout Cin dw_ld col0 round_wgs ws_bytes nunits     prints "slabs <n>" and returns 0, or a message and 1
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "wgrad_slab_index.h"

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const int Cout = atoi(argv[1]), Cin = atoi(argv[2]), dw_ld = atoi(argv[3]), col0 = atoi(argv[4]), round_wgs = atoi(argv[5]);
    const long long ws_bytes = atoll(argv[6]);
    const int nunits = atoi(argv[7]);
    const int ncib = Cin / 32, nblocks = (Cout / 32) * ncib;
    const int nsl = wks::slab_count(round_wgs, nblocks, ws_bytes, nunits);
    printf("slabs %d\n", nsl);
    if (nsl < 1) return 0;
    if ((long long)nsl * nblocks * wks::BLOCK_FLOATS * 4 > ws_bytes || nsl > nunits || nsl * nblocks > round_wgs) { puts("slab count out of its bounds"); return 1; }
    // ---- flush: every (slab, block, wave group G, tap j, register, lane) of the kernel writes one element; the image is a permutation
    const size_t nws = (size_t)nsl * nblocks * wks::BLOCK_FLOATS;
    std::vector<float> ws(nws, -1.f);                   // exactly the floats the slab count was computed for
    for (int slab = 0; slab < nsl; ++slab)
        for (int block = 0; block < nblocks; ++block) {
            float* const my = ws.data() + wks::flush_index(slab, nblocks, block, 0, 0, 0);
            for (int G = 0; G < 4; ++G)
                for (int j = 0; j < (G == 3 ? 6 : 7); ++j)
                    for (int reg = 0; reg < 16; ++reg)
                        for (int lane = 0; lane < 64; ++lane) {
                            const int r = lane & 31, hk = lane >> 5;
                            float& e = my[wks::flush_index(0, nblocks, 0, 7 * G + j, (reg & 3) + 8 * (reg >> 2) + 4 * hk, r)];
                            if (e != -1.f) { puts("flush: an element written twice"); return 1; }
                            e = (float)(slab + 1);
                        }
        }
    for (size_t i = 0; i < nws; ++i)
        if (ws[i] == -1.f) { puts("flush: an element never written"); return 1; }
    // ---- reduction: column q reads one float4 per slab and adds into four consecutive floats of dw (27 x Cout rows of dw_ld, first column col0)
    std::vector<float> dw((size_t)27 * Cout * dw_ld, 0.f);
    float* const dwp = dw.data() + col0;                 // the launch's dw pointer: already offset to its first column
    const long long ncol = (long long)nblocks * wks::BLOCK_F4;
    for (long long q = 0; q < ncol; ++q) {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < nsl; ++s) {
            const float* v = ws.data() + 4 * wks::reduce_src4(s, nblocks, q);
            for (int k = 0; k < 4; ++k) {
                if (v[k] != (float)(s + 1)) { puts("reduce: a column reads another slab's element"); return 1; }
                t[k] += v[k];
            }
        }
        float* d = dwp + wks::reduce_dst(q, ncib, Cout, dw_ld);
        for (int k = 0; k < 4; ++k) d[k] += t[k];
    }
    const float want = 0.5f * nsl * (nsl + 1);
    for (int row = 0; row < 27 * Cout; ++row)
        for (int c = 0; c < dw_ld; ++c) {
            const bool mine = c >= col0 && c < col0 + Cin;
            if (dw[(size_t)row * dw_ld + c] != (mine ? want : 0.f)) { printf("reduce: dw row %d column %d holds %g\n", row, c, dw[(size_t)row * dw_ld + c]); return 1; }
        }
    // the element (tap, co, ci) the kernel's block (cob, cib) register holds is the one the reduction adds to dw[tap][cob*32 + row][cib*32 + col]
    for (int block = 0; block < nblocks; ++block) {
        const long long f = wks::flush_index(0, nblocks, block, 26, 31, 28);
        const long long dst = wks::reduce_dst(f / 4, ncib, Cout, dw_ld);
        if (dst != ((long long)26 * Cout + (block / ncib) * 32 + 31) * dw_ld + (block % ncib) * 32 + 28) { puts("flush and reduction disagree on an element's home"); return 1; }
    }
    return 0;
}
