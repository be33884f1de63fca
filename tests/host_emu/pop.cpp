// CPU execution of popVerify's new arithmetic for tests/test_pop_emu.py, bounds tracked like tests/host_emu/emu.hip: G1 point compression
// (csrc/deser.hpp g1_compress), the prepared-constants hash_to_field for 48-byte messages (csrc/h2c.hpp) and the PoP hash-map body end to end.
// TEST INFRASTRUCTURE: never linked into the product library.
#include "fp.hpp"
#include "tower.hpp"
#include "curve.hpp"
#include "h2c.hpp"
#include "deser.hpp"
using namespace bls;

extern "C" {
// 96-byte blst_p1_affine image (all zero = infinity) -> 48 bytes
void emu_g1_compress(const uint8_t* pk96, uint8_t* out48) { g1_compress(out48, g1_aff_load(pk96)); }
// the generic expand_message_xmd path
void emu_hash_to_field(const uint8_t* m, uint32_t n, const uint8_t* dst, uint32_t dn, uint8_t* out192) {
    fp2 u0, u1; hash_to_field_fp2x2(u0, u1, m, n, dst, dn); fp2_store_le(out192, u0); fp2_store_le(out192 + 96, u1);
}
// the 48-byte prepared form; returns 0 (and writes nothing) when the DST length is outside its range
int emu_hash_to_field_msg48(const uint8_t* m48, const uint8_t* dst, uint32_t dn, uint8_t* out192) {
    const xmd48_consts c = xmd48_precompute(dst, dn);
    if (!c.valid) return 0;
    uint32_t mbe[12];
    xmd32_pack(mbe, m48, 12);
    fp2 u0, u1; hash_to_field_fp2x2_msg48(u0, u1, mbe, c); fp2_store_le(out192, u0); fp2_store_le(out192 + 96, u1);
    return 1;
}
// What a lane of the PoP hash-map kernels does with its record's key under any DST (kernels.hip msg_from_key): compress in words, the prepared
// form when the constants are valid, the generic path otherwise.  Returns which of the two ran (1 = prepared).
int emu_pop_hash_to_field(const uint8_t* pk96, const uint8_t* dst, uint32_t dn, uint8_t* out192) {
    const xmd48_consts c = xmd48_precompute(dst, dn);
    uint32_t mbe[12];
    g1_compress_words(mbe, g1_aff_load(pk96));
    fp2 u0, u1;
    if (c.valid) {
        hash_to_field_fp2x2_msg48(u0, u1, mbe, c);
    } else {
        uint8_t msg[48];
        for (int j = 0; j < 12; j++) { msg[4 * j] = mbe[j] >> 24; msg[4 * j + 1] = mbe[j] >> 16; msg[4 * j + 2] = mbe[j] >> 8; msg[4 * j + 3] = mbe[j]; }
        hash_to_field_fp2x2(u0, u1, msg, 48, dst, dn);
    }
    fp2_store_le(out192, u0); fp2_store_le(out192 + 96, u1);
    return c.valid ? 1 : 0;
}
// the PoP hash-map body end to end under DST_POP: both u mapped (SSWU + 3-isogeny), added, cleared (the formulas k_hash_clear runs) -> 288 B Jacobian
int emu_pop_hash_to_g2(const uint8_t* pk96, uint8_t* out288) {
    static const uint8_t dst[] = "BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";
    const xmd48_consts c = xmd48_precompute(dst, sizeof(dst) - 1);
    if (!c.valid) return 0;
    uint32_t mbe[12];
    g1_compress_words(mbe, g1_aff_load(pk96));
    fp2 u[2];
    hash_to_field_fp2x2_msg48(u[0], u[1], mbe, c);
    g2_jac q[2];
    for (int j = 0; j < 2; j++) q[j] = iso3_g2(sswu_g2(u[j]));
    g2_jac_store(out288, clear_cofactor_g2(jac_add(q[0], q[1])));
    return 1;
}
}
