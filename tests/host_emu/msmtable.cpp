// CPU execution of the counting sort of the fixed-base table MSM (csrc/msmtable.hpp bodies, walked kernel by kernel as host_api.inc ptab_run
// launches k_ptab_hist / k_ptab_scan / k_ptab_scatter) for tests/test_msm_table_emu.py.  TEST INFRASTRUCTURE: never linked into the product
// library.
#include <cstring>
#include <vector>

#include "msmtable.hpp"
using namespace bls;

extern "C" {
// the signed digits of one scalar under fixed_win(wbits, nbits): digits[w], w < the returned number of windows (at most 64)
uint32_t emu_fixed_digits(const uint8_t scalar[32], size_t wbits, size_t nbits, int32_t* digits) {
    const plan::pip_win W = plan::fixed_win(wbits, nbits);
    uint32_t kw[8];
    memcpy(kw, scalar, 32);
    for (uint32_t w = 0; w < W.nwin; w++) digits[w] = fixed_digit(kw, W, w);
    return W.nwin;
}
// One pass over ALL k MSMs of the call (n points each; scalars: k n x 32 bytes) with S bucket sets per MSM.  Out: win[14], hist / offs_out
// (k S << cbk words each: counts and list positions), sorted (k n nwin words), gb (the global bucket pair p met in window w at [p nwin + w],
// 0xffffffff for a zero digit).  Returns the words of `sorted` the lists span, or -1 when an index left its array.
long emu_fixed_sort(const uint8_t* scalars, uint32_t k, uint32_t n, size_t wbits, size_t nbits, uint32_t S, uint32_t* win, uint32_t* hist, uint32_t* offs_out,
                    uint32_t* sorted, uint32_t* gb) {
    const plan::pip_win W = plan::fixed_win(wbits, nbits);
    if (S < 1 || S > W.nwin) return -1;
    memcpy(win, &W, 14 * 4);
    const uint32_t pairs = k * n, nw = W.nwin, nv = k * S, total = nv << W.cbk, nb = 1u << W.cbk;
    const fixed_addr A{pairs, n, nw, S, W.cbk};
    const size_t words = (size_t)pairs * nw;
    bool oob = false;
    std::vector<uint32_t> cursor(total);
    memset(hist, 0, (size_t)total * 4);
    const auto digit = [&](uint32_t p, uint32_t w) {
        uint32_t kw[8];
        memcpy(kw, scalars + (size_t)p * 32, 32);
        return fixed_digit(kw, W, w);
    };
    // k_ptab_hist
    for (uint32_t w = 0; w < nw; w++)
        for (uint32_t p = 0; p < pairs; p++) {
            const int32_t d = digit(p, w);
            gb[(size_t)p * nw + w] = 0xffffffffu;
            if (!d) continue;
            const uint32_t g = fixed_bucket(A, fixed_owner(A, p), w, (uint32_t)(d < 0 ? -d : d));
            oob |= g >= total;
            if (g < total) hist[g]++, gb[(size_t)p * nw + w] = g;
        }
    // k_ptab_scan
    for (uint32_t v = 0; v < nv; v++) {
        uint32_t run = fixed_list_start(A, v);
        for (uint32_t b = 0; b < nb; b++) {
            offs_out[((size_t)v << W.cbk) | b] = cursor[((size_t)v << W.cbk) | b] = run;
            run += hist[((size_t)v << W.cbk) | b];
        }
        oob |= run > (v + 1 < nv ? fixed_list_start(A, v + 1) : words);      // a set's list ends where the next one begins
    }
    // k_ptab_scatter
    for (size_t i = 0; i < words; i++) sorted[i] = 0xffffffffu;
    for (uint32_t w = 0; w < nw; w++)
        for (uint32_t p = 0; p < pairs; p++) {
            const int32_t d = digit(p, w);
            if (!d) continue;
            const uint32_t j = fixed_owner(A, p), g = fixed_bucket(A, j, w, (uint32_t)(d < 0 ? -d : d));
            if (g >= total) return -1;
            const uint32_t pos = cursor[g]++;
            oob |= pos >= words;
            if (pos < words) sorted[pos] = fixed_entry(A, w, fixed_point(A, p, j)) | (d < 0 ? 0x80000000u : 0u);
        }
    return oob ? -1 : (long)words;
}
}
