// Same-message pre-aggregation of MANY groups at once (mi355_bls_combine_sets): MultiSignatureSet.combine (bls_batch_verifier.nim:47-106,
// blst_min_pubkey_sig_core.nim:570-647) for k groups of 320-byte SignatureSet records in one device pass - the bodies one lane carries,
// written so that the host can run them.  Members are numbered by POSITION in the call's member sequence (group g = positions
// [first_g, first_g + len_g)); where a position's record lives is the caller's business: it hands in loaders.
//   chain        a group's scalars s_0 .. s_(L-1): the SHA-256 chain seeded with the group's own 32 random bytes (core :588-606)
//   mul item     [s]P for one member and a 64-bit scalar: signed 4-bit windows, the table of 1 .. 8 times P kept where the caller says
//   sum item     up to AGG_C Jacobian points of one group -> one partial (the items of plan.hpp aggsets_fill, over positions)
//   check item   the members of a level-0 item against the rules a combination needs: index in range, same message, key not at infinity
//   finish       a group's two sums -> its 320-byte record and its status byte
// All additions are the complete ones of curve.hpp, so a group may hold a member twice, two members whose terms are equal or opposite, or a
// signature at infinity (adds nothing).
#pragma once
#include "aggsets.hpp"
#include "sha256.hpp"

namespace bls {

constexpr uint8_t COMB_MIXED = 4, COMB_INF_KEY = 5;                       // status bytes beyond aggsets.hpp's AGG_*
constexpr uint32_t COMB_F_BAD = 1, COMB_F_MIXED = 2, COMB_F_INF_KEY = 4;  // a group's flag word, as the check items set it

// put(j, s_j) for j < n: u64 words 3, 2, 1, 0 of every digest of seed <- SHA256(seed), seed_0 = rnd, zero words skipped
template <class Put>
BLS_HD void combsets_chain(const uint8_t* rnd, size_t n, Put&& put) {
    uint32_t seed[8], nx[8];
    for (int i = 0; i < 8; i++) seed[i] = ((uint32_t)rnd[4 * i] << 24) | ((uint32_t)rnd[4 * i + 1] << 16) | ((uint32_t)rnd[4 * i + 2] << 8) | rnd[4 * i + 3];
    int avail = 0;
    for (size_t j = 0; j < n;) {
        if (avail == 0) {
            sha256_of_digest(seed, nx);
            for (int i = 0; i < 8; i++) seed[i] = nx[i];
            avail = 4;
        }
        avail--;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int q = 0; q < 4; q++)
            if (q == avail) lo = seed[2 * q], hi = seed[2 * q + 1];
        const uint64_t w = (uint64_t)bswap32(lo) | ((uint64_t)bswap32(hi) << 32);      // little-endian u64 word `avail`
        if (w != 0) put(j++, w);
    }
}

// [kk]P, the formulas and digits of curve.hpp jac_mul_u64_w4_body; the table T[i] = (i + 1) P goes through put(i, point) / get(i) (a lane's
// own slots of a device buffer: eight Jacobian points in registers beside the accumulator do not fit a lane).  kk == 0: infinity, no table.
template <class F, class Put, class Get>
BLS_HD jac<F> combsets_mul_item(const aff<F>& p, uint64_t kk, Put&& put, Get&& get) {
    if (kk == 0) return jac_inf<F>();
    put(0, jac_from_aff(p));
#pragma clang loop unroll(disable)
    for (int i = 1; i < 8; i++) {
        if (i & 1)
            put(i, jac_dbl(get(i >> 1)));              // 2, 4, 6, 8 times P
        else
            put(i, jac_add_aff(get(i - 1), p));        // 3, 5, 7 times P
    }
    // signed digits d_j in [-8, 8] from the least significant end, packed as d_j + 8 in five bits; the final carry is digit 16
    uint64_t lo = 0, hi = 0;
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        int32_t d = (int32_t)((kk >> (4 * j)) & 15u) + (int32_t)carry;
        carry = d > 8;
        const uint64_t e = (uint64_t)((carry ? d - 16 : d) + 8);
        if (j < 12) lo |= e << (5 * j);
        else hi |= e << (5 * (j - 12));
    }
    jac<F> acc = carry ? get(0) : jac_inf<F>();
#pragma clang loop unroll(disable)
    for (int j = 15; j >= 0; j--) {
#pragma clang loop unroll(disable)
        for (int k4 = 0; k4 < 4; k4++) acc = jac_dbl(acc);
        const int d = (int)((j < 12 ? lo >> (5 * j) : hi >> (5 * (j - 12))) & 31u) - 8;
        if (d != 0) {
            jac<F> t = get((d < 0 ? -d : d) - 1);
            if (d < 0) t = jac_neg(t);
            acc = jac_add_body(acc, t);
        }
    }
    return acc;
}

// points [first, first + count), count >= 1 (aggsets_ln_item for either group)
template <class F, class Load>
BLS_HD jac<F> combsets_sum_item(uint32_t first, uint32_t count, Load&& pt) {
    jac<F> acc = pt(first);
#pragma clang loop unroll(disable)
    for (uint32_t j = 1; j < count; j++) acc = jac_add_body(acc, pt(first + j));
    return acc;
}

// Members [first, first + count) of the group whose first member is at seg_first -> the flags they raise.  bad(pos): the position's table
// index is out of range (its record is then never read); rec(pos): the 80 words of the member's record.
template <class Bad, class Rec>
BLS_HD uint32_t combsets_check_item(uint32_t first, uint32_t count, uint32_t seg_first, Bad&& bad, Rec&& rec) {
    uint32_t flags = 0;
    const bool first_ok = !bad(seg_first);
    const uint32_t* r0 = first_ok ? rec(seg_first) : nullptr;
#pragma clang loop unroll(disable)
    for (uint32_t j = 0; j < count; j++) {
        if (bad(first + j)) {
            flags |= COMB_F_BAD;
            continue;
        }
        const uint32_t* r = rec(first + j);
        uint32_t any = 0, diff = 0;
        for (int i = 0; i < 24; i++) any |= r[i];
        if (r0)
            for (int i = 24; i < 32; i++) diff |= r[i] ^ r0[i];
        if (!any) flags |= COMB_F_INF_KEY;            // the blst_p1_affine image of infinity: all zero
        if (diff) flags |= COMB_F_MIXED;
    }
    return flags;
}

// A group's end.  len members, `flags` as its check items left them, pk / sg = the two sums (not read when len < 2), first = the record of its
// first member (nullptr: the group is empty, or that member's index is out of range).  Precedence 3 > 4 > 5 > 1 > 2.  A group of one is
// a passthrough: the member's record, unchanged (core :585-586).  Any status but 0: the infinity key, for which every verifier answers
// false, the first member's message where there is one, and the infinity signature.
struct combsets_end {
    uint32_t rec[80];
    uint8_t status;
};
BLS_HD combsets_end combsets_finish_item(uint32_t len, uint32_t flags, const g1_jac& pk, const g2_jac& sg, const uint32_t* first) {
    combsets_end e;
    e.status = (flags & COMB_F_BAD)       ? AGG_BAD_INDEX
               : (flags & COMB_F_MIXED)   ? COMB_MIXED
               : (flags & COMB_F_INF_KEY) ? COMB_INF_KEY
               : len == 0                 ? AGG_EMPTY
               : (len >= 2 && jac_is_inf(pk)) ? AGG_INFINITY
                                          : AGG_OK;
    for (int i = 0; i < 80; i++) e.rec[i] = 0;
    if (first)
        for (int i = 24; i < 32; i++) e.rec[i] = first[i];
    if (e.status != AGG_OK) return e;
    if (len == 1) {
        for (int i = 0; i < 80; i++) e.rec[i] = first[i];
        return e;
    }
    {
        const fp zi = fp_inv(pk.z), zi2 = fp_sqr(zi);
        uint32_t x[12], y[12];
        fp_to_blst(x, fp_mul(pk.x, zi2));
        fp_to_blst(y, fp_mul(pk.y, fp_mul(zi2, zi)));
        for (int i = 0; i < 12; i++) e.rec[i] = x[i], e.rec[12 + i] = y[i];
    }
    if (!jac_is_inf(sg)) {                             // a combined signature at infinity: 192 zero bytes
        const fp2 zi = fp2_inv(fp2_reduce(sg.z)), zi2 = fp2_sqr(zi);
        const fp2 x = fp2_mul(sg.x, zi2), y = fp2_mul(sg.y, fp2_mul(zi2, zi));
        uint32_t w[12];
        const fp* c[4] = {&x.c0, &x.c1, &y.c0, &y.c1};
        for (int t = 0; t < 4; t++) {
            fp_to_blst(w, *c[t]);
            for (int i = 0; i < 12; i++) e.rec[32 + 12 * t + i] = w[i];
        }
    }
    return e;
}

}  // namespace bls
