// CPU execution of the G2 per-MSM tail's Horner walk (csrc/msmmany.hpp many_tail_walk, the schedule k_pip_tail_many_g2 runs) with the plain
// jac_dbl / jac_add formulas under the bounds tracker, and of the digits its window sums are made from, for tests/test_msm_many_g2_emu.py.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>
#include <vector>

#include "curve.hpp"
#include "msmmany.hpp"
using namespace bls;

namespace {
struct host_tail_ops {
    using point = g2_jac;
    const std::vector<g2_jac>* sums;
    uint32_t* counts;      // [0] doublings, [1] additions, [2] windows read
    g2_jac inf() const { return jac_inf<fp2>(); }
    bool is_inf(const g2_jac& p) const { return jac_is_inf(p); }
    g2_jac window(uint32_t w) const {
        counts[2]++;
        return sums->at(w);
    }
    g2_jac dbl(const g2_jac& p) const {
        counts[0]++;
        return jac_dbl(p);
    }
    g2_jac add(const g2_jac& a, const g2_jac& b) const {
        counts[1]++;
        return jac_add(a, b);
    }
};
}  // namespace

extern "C" {
// the window plan of a call whose width is taken from n_ref points: win[14] as the kernels take it, offs[w] = the bit offset of window w
uint32_t emu_g2_many_windows(size_t n_ref, size_t nbits, uint32_t* win, uint32_t* offs) {
    const plan::pip_win W = plan::pip_for(n_ref, nbits);
    memcpy(win, &W, 14 * 4);
    for (uint32_t w = 0; w <= W.nwin; w++) offs[w] = many_win_off(W, w);
    return W.nwin;
}
uint32_t emu_g2_many_digits(const uint8_t scalar[32], size_t n_ref, size_t nbits, int32_t* digits) {
    const plan::pip_win W = plan::pip_for(n_ref, nbits);
    uint32_t kw[8];
    memcpy(kw, scalar, 32);
    for (uint32_t w = 0; w < W.nwin; w++) digits[w] = many_digit(kw, W, w);
    return W.nwin;
}
// sums: nwin blst_p2 images (288 B each), window 0 first -> the walk's result as the kernel writes it (an infinite one: 288 zero bytes);
// counts[3]: doublings, additions, windows read
void emu_g2_tail_walk(const uint8_t* sums288, size_t n_ref, size_t nbits, uint8_t out288[288], uint32_t counts[3]) {
    const plan::pip_win W = plan::pip_for(n_ref, nbits);
    std::vector<g2_jac> sums(W.nwin);
    for (uint32_t w = 0; w < W.nwin; w++) sums[w] = g2_jac_load(sums288 + (size_t)w * 288);
    counts[0] = counts[1] = counts[2] = 0;
    const g2_jac r = many_tail_walk(W, host_tail_ops{&sums, counts});
    if (jac_is_inf(r)) memset(out288, 0, 288);
    else g2_jac_store(out288, r);
}
}
