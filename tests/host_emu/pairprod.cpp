// CPU execution of the pair-slot bodies of the pairing-product calls (csrc/pairprod.hpp: validation, the pair as the line kernels take it, the
// blinded form's key words and scalar expansion) for tests/test_pairprod_emu.py, bounds tracked like tests/host_emu/emu.hip.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <vector>
#include "fp.hpp"
#include "tower.hpp"
#include "curve.hpp"
#include "pairprod.hpp"
#include "plan.hpp"
using namespace bls;

extern "C" {
// What k_pairprod_setup's lanes do for n pairs (96-byte and 192-byte affine images).  validate: plan::PAIRPROD_VALIDATE or 0.
//   status   n bytes
//   p_out    n x 144 bytes, q_out n x 288 bytes: the Jacobian operands as the pair store gets them (blst images; Z = 0: infinity)
//   key_out  n x 96 bytes: the words the blinded form lays out for k_pkmul
void emu_pairprod_setup(const uint8_t* p1s, const uint8_t* q2s, size_t n, uint32_t validate, uint8_t* status, uint8_t* p_out, uint8_t* q_out, uint8_t* key_out) {
    for (size_t i = 0; i < n; i++) {
        const g1_aff p = g1_aff_load(p1s + i * 96);
        const g2_aff q = g2_aff_load(q2s + i * 192);
        const uint8_t st = (validate & plan::PAIRPROD_VALIDATE) ? pairprod_validate(p, q) : (uint8_t)PAIRPROD_OK;
        status[i] = st;
        const pairprod_pair pr = pairprod_operands(p, q, st);
        fp_store_le(p_out + i * 144, pr.p.x), fp_store_le(p_out + i * 144 + 48, pr.p.y), fp_store_le(p_out + i * 144 + 96, pr.p.z);
        fp2_store_le(q_out + i * 288, pr.q.x), fp2_store_le(q_out + i * 288 + 96, pr.q.y), fp2_store_le(q_out + i * 288 + 192, pr.q.z);
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p1s + i * 96);
        uint32_t* kw = reinterpret_cast<uint32_t*>(key_out + i * 96);
        for (int j = 0; j < 24; j++) kw[j] = pairprod_key_word(w, j, st);
    }
}
// The scalar of every pair slot of every slice of the blinded form, walked as the host layer walks it (plan::pairprod_blind_cut parts of cap
// pairs, plan::pairprod_real_groups' table per part): r_pair[pos] for all offsets[k] positions.  -> the number of parts
int emu_pairprod_expand(const size_t* offsets, size_t k, size_t cap, const uint64_t* r, uint64_t* r_pair) {
    const size_t n = offsets[k];
    int parts = 0;
    for (size_t pos = 0;;) {
        const plan::aggv_slice s = plan::pairprod_blind_cut(n, pos, cap);
        if (s.pairs() == 0) break;
        const plan::aggv_slice rs = plan::pairprod_real_groups(offsets, k, s.pos0, s.pos1);
        std::vector<plan::aggv_group> gr(rs.ng);
        plan::aggveach_groups(offsets, rs, gr.data());
        for (uint32_t i = 0; i < (uint32_t)s.pairs(); i++)
            r_pair[s.pos0 + i] = pairprod_scalar_of(i, rs.ng, [&](uint32_t l) { return gr[l].first; }, [&](uint32_t l) { return gr[l].g; }, r);
        parts++;
        pos = s.pos1;
    }
    return parts;
}
}
