// Per-group signature aggregation (mi355_bls_aggregate_signature_sets): aggregateAll on signatures (genAggregatorProcedures(AggregateSignature,
// Signature, p2), blst_min_pubkey_sig_core.nim:142-211) for MANY groups at once, then finish + serialize (bls_sig_io.nim:225-234) - the
// bodies of ONE item of the segmented sum that plan.hpp aggsets_measure / aggsets_fill lays out, written like aggsets.hpp so that one lane
// can carry an item and the host can run it.
//   level 0      up to AGG_C signatures of one group (blst_p2_affine images, through an optional index array into a table) -> one Jacobian partial
//   level >= 1   combsets.hpp combsets_sum_item<fp2>: up to AGG_C partials of one group -> one partial
//   finish       a group's last partial -> its affine image, its 96-byte wire form and its status byte
//   compress     one affine image -> its wire form (mi355_bls_compress_signatures)
// The additions are the complete ones of curve.hpp, so a group may hold a signature twice, a signature and its negative, or the affine
// infinity image (all zero: adds nothing, as in mi355_bls_g2_aggregate).  Where signatures and partials live is the caller's business: it
// hands in loaders.
#pragma once
#include "aggsets.hpp"
#include "deser.hpp"

namespace bls {

// signatures [first, first + count) of the call's signature sequence; idx == nullptr: the sequence is the table itself.  A position whose
// table index is not below n_table is never loaded: bad() is told, and the signature counts as the point at infinity.
template <class LoadSig, class Bad>
BLS_HD g2_jac aggsigs_l0_item(uint32_t first, uint32_t count, const uint32_t* idx, size_t n_table, LoadSig&& sig, Bad&& bad) {
    g2_jac acc = jac_inf<fp2>();
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < count; j++) {
        const size_t at = (size_t)first + j, t = idx ? (size_t)idx[at] : at;
        if (t >= n_table) {
            bad();
            continue;
        }
        acc = jac_add_aff(acc, sig(t));
    }
    return acc;
}

// the wire form as the 24 words that lie in memory (word i holds bytes 4 i .. 4 i + 3, lowest address in the low byte)
BLS_HD void aggsigs_compress_item(uint32_t (&wire)[24], const g2_aff& p) {
    uint32_t be[24];
    g2_compress_words(be, p);
#pragma unroll
    for (int i = 0; i < 24; i++) wire[i] = bswap32(be[i]);
}

// A group's end: `empty` = it has no member (then p is not read), `bad` = one of its indices was out of range.  status as aggsets.hpp's
// AGG_*, bad index first.  sig = the 48 words of the blst_p2_affine image of the sum, wire = its compressed form; both are the encodings of
// infinity (all zero; 0xc0 and 95 zero bytes) unless the status is AGG_OK - for AGG_INFINITY they are that sum's valid encodings.
struct aggsigs_end {
    uint32_t sig[48];
    uint32_t wire[24];
    uint8_t status;
};
BLS_HD aggsigs_end aggsigs_finish_item(bool empty, bool bad, const g2_jac& p) {
    aggsigs_end e;
    e.status = bad ? AGG_BAD_INDEX : empty ? AGG_EMPTY : jac_is_inf(p) ? AGG_INFINITY : AGG_OK;
    if (e.status != AGG_OK) {
        for (int i = 0; i < 48; i++) e.sig[i] = 0;
        for (int i = 0; i < 24; i++) e.wire[i] = 0;
        e.wire[0] = 0xc0u;
        return e;
    }
    const fp2 zi = fp2_inv(fp2_reduce(p.z)), zi2 = fp2_sqr(zi);
    const g2_aff a{fp2_mul(p.x, zi2), fp2_mul(p.y, fp2_mul(zi2, zi))};
    uint32_t w[12];
    const fp* c[4] = {&a.x.c0, &a.x.c1, &a.y.c0, &a.y.c1};
    for (int t = 0; t < 4; t++) {
        fp_to_blst(w, *c[t]);
        for (int i = 0; i < 12; i++) e.sig[12 * t + i] = w[i];
    }
    aggsigs_compress_item(e.wire, a);
    return e;
}

}  // namespace bls
