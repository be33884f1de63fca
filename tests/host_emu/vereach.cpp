// CPU execution of the per-set verification body (csrc/vereach.hpp) for tests/test_vereach_emu.py, bounds tracked like tests/host_emu/emu.hip.
// TEST INFRASTRUCTURE: never linked into the product library.
#include "fp.hpp"
#include "tower.hpp"
#include "curve.hpp"
#include "h2c.hpp"
#include "pairing.hpp"
#include "vereach.hpp"
using namespace bls;

extern "C" {
// one 320-byte SignatureSet record -> verdict; out576 = final_exp(f) as a blst_fp12 image.  The lines of the two pairs are what the line
// kernels store: miller_lines of (pk, H(msg)) and of (-G1, sig), line_one() throughout for a pair with an operand at infinity.
int emu_vereach_set(const uint8_t* set320, uint8_t* out576) {
    static const uint8_t dst[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
    const g1_aff pk = g1_aff_load(set320);
    const g2_aff sig = g2_aff_load(set320 + 128);
    const g2_jac h = hash_to_g2(set320 + 96, 32, dst, sizeof(dst) - 1);
    static line_t A[N_LINES], B[N_LINES];
    miller_lines(jac_from_aff(pk), h, [&](int s, const line_t& l) { A[s] = l; });
    miller_lines(g1_jac{fp_from_const(k::G1_X), fp_from_const(k::G1_NEG_Y), fp_one()}, jac_from_aff(sig), [&](int s, const line_t& l) { B[s] = l; });
    const vereach_out o = vereach_set([&](int s) { return A[s]; }, [&](int s) { return B[s]; }, aff_is_inf(pk));
    fp12_store_le(out576, o.value);
    return o.ok ? 1 : 0;
}
}
