// CPU execution of the counting sort of k MSMs in one pass (csrc/msmmany.hpp bodies, walked kernel by kernel as host_api.inc msm_many_run
// launches k_pipm_hist / k_pipm_scan / k_pipm_scatter) for tests/test_msm_many_emu.py.  TEST INFRASTRUCTURE: never linked into the product
// library.
#include <cstring>
#include <vector>

#include "msmmany.hpp"
using namespace bls;

extern "C" {
// One pass over ALL k MSMs of the call (the caller keeps it inside a pass).  scalars: pairs x 32 bytes.  offs: k + 1 pass offsets (ragged) or
// NULL (shared: n points per MSM, pairs = k n).  Out: win[14] (the call's window plan), hist / offs_out (k nwin << cbk words each: counts and
// list positions), sorted (pairs x nwin words), gb (pairs x nwin: the global bucket pair p met in window w at [p nwin + w], 0xffffffff for a
// zero digit).  Returns the number of words of `sorted` the lists span, or -1 when an index left its array or the call is no single pass.
long emu_many_sort(const uint8_t* scalars, const uint32_t* offs, uint32_t pairs, uint32_t k, uint32_t n, size_t nbits, uint32_t* win, uint32_t* hist,
                   uint32_t* offs_out, uint32_t* sorted, uint32_t* gb) {
    std::vector<size_t> call_offs;
    if (offs) call_offs.assign(offs, offs + k + 1);
    const size_t npoints = offs ? pairs : n;
    const plan::msm_many_plan P = plan::msm_many_for(k, npoints, offs == nullptr, nbits);
    const plan::msm_many_pass s = plan::msm_many_next(P, offs ? call_offs.data() : nullptr, npoints, k, 0);
    if (s.single || s.j1 != k || s.pairs != pairs) return -1;
    memcpy(win, &P.W, 14 * 4);
    const many_addr A{pairs, k, offs ? 0u : n, P.W.nwin, P.W.cbk};
    const uint32_t nw = P.W.nwin, total = s.total, nb = 1u << P.W.cbk;
    const size_t words = (size_t)pairs * nw;
    bool oob = false;
    std::vector<uint32_t> cursor(total);
    memset(hist, 0, (size_t)total * 4);
    const auto digit = [&](uint32_t p, uint32_t w) {
        uint32_t kw[8];
        memcpy(kw, scalars + (size_t)p * 32, 32);
        return many_digit(kw, P.W, w);
    };
    // k_pipm_hist
    for (uint32_t w = 0; w < nw; w++)
        for (uint32_t p = 0; p < pairs; p++) {
            const int32_t d = digit(p, w);
            gb[(size_t)p * nw + w] = 0xffffffffu;
            if (!d) continue;
            const uint32_t g = many_bucket(A, many_owner(A, offs, p), w, (uint32_t)(d < 0 ? -d : d));
            oob |= g >= total;
            if (g < total) hist[g]++, gb[(size_t)p * nw + w] = g;
        }
    // k_pipm_scan
    for (uint32_t v = 0; v < s.nv; v++) {
        uint32_t run = many_list_start(A, offs, v);
        for (uint32_t b = 0; b < nb; b++) {
            offs_out[((size_t)v << P.W.cbk) | b] = cursor[((size_t)v << P.W.cbk) | b] = run;
            run += hist[((size_t)v << P.W.cbk) | b];
        }
        oob |= run > words;
    }
    // k_pipm_scatter
    for (size_t i = 0; i < words; i++) sorted[i] = 0xffffffffu;
    for (uint32_t w = 0; w < nw; w++)
        for (uint32_t p = 0; p < pairs; p++) {
            const int32_t d = digit(p, w);
            if (!d) continue;
            const uint32_t j = many_owner(A, offs, p), g = many_bucket(A, j, w, (uint32_t)(d < 0 ? -d : d));
            if (g >= total) return -1;
            const uint32_t pos = cursor[g]++;
            oob |= pos >= words;
            if (pos < words) sorted[pos] = many_point(A, p, j) | (d < 0 ? 0x80000000u : 0u);
        }
    return oob ? -1 : (long)words;
}
}
