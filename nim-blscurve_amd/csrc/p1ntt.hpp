// Number-theoretic transforms of MANY vectors of curve points at once (mi355_bls_p1s_ntt_many): for k vectors of n = 2^m points P_j the
// sums sum_j [omega^(i j)] P_j, and the exact inverse map - the bodies one lane carries, written like lincomb.hpp and frntt.hpp so that the
// host can run them (tests/host_emu/p1ntt.cpp; csrc/kernels.hip k_p1ntt_*).  omega_n, rev_m and both flags are frntt.hpp's: for P_j = [a_j]G
// the result is [fr_ntt(a)_i]G under the same flags.
//   The k vectors of a slice are ONE array of k x n elements in the call's workspace, internal Jacobian images: bit b < m of an element's
//   index is bit b of its place in its vector, the bits from m up are the vector's number.  A radix-2 STAGE pairs the elements whose
//   indices differ in bit b (half-span h = 2^b), one lane per butterfly, over global memory - a butterfly is a 255-bit scalar
//   multiplication, about 2 800 Fp products, beside which its two loads and stores are nothing, so there is no LDS tiling:
//     decimation in frequency (DIF)   (a, b) -> (a + b, [w](a - b)), stages from bit m - 1 down to 0: natural order in, bit-reversed order out
//     decimation in time (DIT)        (a, b) -> (a + [w]b, a - [w]b), stages from bit 0 up to m - 1:  bit-reversed order in, natural order out
//   with w = root^(j 2^(m - 1 - b)), j = index mod h, read from ONE table of the n / 2 powers of root (omega, or 1 / omega for the inverse)
//   as canonical PLAIN scalars: the window walk needs integer digits.  Which one runs is frntt.hpp's rule (csrc/host_api.inc p1ntt_run):
//   forward with BITREV is DIF, inverse with BITREV is DIT over 1 / omega, without BITREV both are DIF and the last store - the finish -
//   permutes.  The first stage reads the caller's affine images, every stage writes the workspace, the finish writes the caller's output:
//   an in-place call is no special case.
//   TRIVIAL TWIDDLES: j = 0 means w = 1 and no multiplication - all of the stage at bit 0, half of the one at bit 1, ...: n - 1 of the
//   (n / 2) m butterflies of a vector.  The lanes of a stage are numbered TWIDDLE-MAJOR: lane = j Q + q, q < Q = k 2^(m - 1 - b) the
//   butterfly's block counted across the slice's vectors.  The Q lanes of one twiddle are neighbours, so butterflies without a
//   multiplication fill whole waves (up to one ragged wave per stage) instead of idling beside lanes that multiply, and wherever Q >= 64 a
//   wave walks ONE scalar: the same digits, the same table entries, no divergence in the window walk.
//   1 / n of the inverse is folded into the stage at bit m - 1, the one stage whose n / 2 twiddles are all different: its multiplier
//   becomes the plain product w / n (one Fr product per lane) and the other operand - the sum a + b of DIF, the a of DIT - is multiplied by
//   1 / n, a scalar every lane shares.  n / 2 multiplications more per vector where a pass over the elements costs n.
//   The finish turns a run of consecutive elements into canonical affine images with one shared inversion (toaffine.hpp to_affine_run)
//   and stores each at its place, bit-reversed in its vector where the store permutes.  n == 1 has no stage: the finish reads the
//   caller's images, the canonicalising copy.
// The additions a + t and a - t are the complete ones: infinity operands, a == t (a doubling) and a == -t (infinity) occur for ordinary
// inputs - constant vectors, vectors with one entry.  Variable time throughout: public points only.
#pragma once
#include "frntt.hpp"
#include "toaffine.hpp"

namespace bls {

// [k]P for a JACOBIAN base and a 256-bit scalar (8 little-endian words): curve.hpp jac_mul_256_w4_body's signed 4-bit windows, digits and
// carries (see there: bit j of `cin` is the carry INTO window j), with the table 1 .. 8 times P made by the doubling and the COMPLETE
// addition - the base has a Z of its own.  256 doublings and at most 65 additions; the accumulator can meet +- a table entry: complete
// additions there too.  A base at infinity gives infinity without a walk.  NOT constant time.
template <class F>
BLS_MID jac<F> jac_mul_256_w4_jac_body(const jac<F>& p, const uint32_t (&kk)[8]) {
    if (jac_is_inf(p)) return jac_inf<F>();
    jac<F> T[8];
    T[0] = p;
#pragma clang loop unroll(disable)
    for (int i = 1; i < 8; i++) {
        if (i & 1)
            T[i] = jac_dbl(T[i >> 1]);              // 2, 4, 6, 8 times P
        else
            T[i] = jac_add_body(T[i - 1], p);       // 3, 5, 7 times P
    }
    uint64_t cin = 0;
    uint32_t carry = 0;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        cin |= (uint64_t)carry << j;
        carry = ((kk[j >> 3] >> (4 * (j & 7))) & 15u) + carry > 8u;
    }
    jac<F> acc = jac_select(carry != 0, T[0], jac_inf<F>());      // the final carry: digit 64
#pragma clang loop unroll(disable)
    for (int w = 7; w >= 0; w--) {
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (q == w) word = kk[q];
#pragma clang loop unroll(disable)
        for (int n = 7; n >= 0; n--) {
#pragma clang loop unroll(disable)
            for (int k4 = 0; k4 < 4; k4++) acc = jac_dbl(acc);
            const int j = 8 * w + n;
            const int d = (int)((word >> (4 * n)) & 15u) + (int)((cin >> j) & 1u) - 16 * (int)carry;
            carry = (uint32_t)((cin >> j) & 1u);
            if (d != 0) {
                jac<F> t = T[(d < 0 ? -d : d) - 1];
                if (d < 0) t = jac_neg(t);
                acc = jac_add_body(acc, t);
            }
        }
    }
    return acc;
}

// ---- the twiddle table: root^j as a canonical PLAIN scalar, j < count = n / 2.  frntt_twiddle_run's scheme - lane `run` owns entries
// [run FRNTT_RUN, (run + 1) FRNTT_RUN) cut to count, one fr_pow_u64 and a running product - with each entry taken out of Montgomery form.
BLS_HD void p1ntt_twiddle_run(const fr& root, uint64_t run, uint64_t count, uint32_t* tw) {
    const uint64_t lo = run * FRNTT_RUN, hi = count - lo < FRNTT_RUN ? count : lo + FRNTT_RUN;
    if (lo >= count) return;
    fr p = fr_pow_u64(root, lo);
#pragma clang loop unroll(disable)
    for (uint64_t j = lo; j < hi; j++) {
        fropen_st(tw + j * 8, fr_from_mont(p));
        p = fr_mont_mul(p, root);
    }
}

// ---- a stage
// m: n = 2^m; k: the vectors of the slice; b: the index bit the stage pairs over.  scaled: the inverse's stage at bit m - 1, where 1 / n
// is folded in - s_mont is 1 / n in Montgomery form (a plain twiddle times it is the plain product), s its canonical plain words.
struct p1ntt_stage {
    uint32_t m, b;
    uint64_t k;
    bool scaled;
    fr s_mont;
    uint32_t s[8];
};
// the lanes of a stage: a butterfly each
BLS_HD uint64_t p1ntt_lanes(const p1ntt_stage& g) { return g.k << (g.m - 1); }
// lane -> its two elements in the k x n array and its twiddle's entry in the table (0: the twiddle is 1), twiddle-major
struct p1ntt_pair {
    uint64_t i0, i1, tw;
};
BLS_HD p1ntt_pair p1ntt_pair_of(const p1ntt_stage& g, uint64_t lane) {
    const uint64_t Q = g.k << (g.m - 1 - g.b), j = lane / Q, q = lane % Q;
    const uint64_t i0 = (q << (g.b + 1)) | j;
    return p1ntt_pair{i0, i0 | ((uint64_t)1 << g.b), j << (g.m - 1 - g.b)};
}
// (x, y) -> (x + y, x - y), complete.  One copy of the addition: the loop is not unrolled.
template <class F>
BLS_HD void p1ntt_sum_diff(jac<F>& x, jac<F>& y) {
    jac<F> s = x, d = x;
#pragma clang loop unroll(disable)
    for (int t = 0; t < 2; t++) {
        const jac<F> r = jac_add_body(x, t ? jac_neg(y) : y);
        if (t)
            d = r;
        else
            s = r;
    }
    x = s, y = d;
}
// The butterfly of `lane`: load(e) -> the Jacobian point of element e (the first stage: the caller's affine image), store(e, point) into
// the workspace, twiddle(t) -> entry t of the table.  One copy of the multiplication: x (by 1 / n, the scaled stage only) and y (by the
// twiddle, unless it is 1) go through the same loop.
template <bool DIT, class F, class Load, class Store, class Twiddle>
BLS_HD void p1ntt_butterfly(const p1ntt_stage& g, uint64_t lane, Load&& load, Store&& store, Twiddle&& twiddle) {
    const p1ntt_pair pr = p1ntt_pair_of(g, lane);
    jac<F> x = load(pr.i0), y = load(pr.i1);
    const bool mul_y = g.scaled || pr.tw != 0;
    uint32_t kw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) kw[i] = 0;
    if (mul_y) {
        fr w = twiddle(pr.tw);
        if (g.scaled) w = fr_mont_mul(w, g.s_mont);
#pragma unroll
        for (int i = 0; i < 8; i++) kw[i] = w.l[i];
    }
    if (!DIT) p1ntt_sum_diff(x, y);
#pragma clang loop unroll(disable)
    for (int t = 0; t < 2; t++) {
        if (t ? !mul_y : !g.scaled) continue;
        uint32_t kk[8];
#pragma unroll
        for (int i = 0; i < 8; i++) kk[i] = t ? kw[i] : g.s[i];
        const jac<F> r = jac_mul_256_w4_jac_body(t ? y : x, kk);
        if (t)
            y = r;
        else
            x = r;
    }
    if (DIT) p1ntt_sum_diff(x, y);
    store(pr.i0, x);
    store(pr.i1, y);
}

// ---- the finish: lane `lane` takes elements [lane run, (lane + 1) run) cut to total = k n, run <= plan::TOAFF_RUN_MAX, through
// to_affine_run; element e goes to slot e of the output, or with `permute` to the bit-reversed place in its vector.  load(e) -> the
// Jacobian point, store(slot, affine), store_inf(slot).
template <class F, class Load, class Store, class StoreInf>
BLS_HD void p1ntt_finish_run(uint64_t total, uint32_t m, bool permute, uint32_t run, uint64_t lane, Load&& load, Store&& store, StoreInf&& store_inf) {
    const uint64_t first = lane * run;
    if (run == 0 || run > plan::TOAFF_RUN_MAX || first >= total) return;
    const uint32_t count = (uint32_t)(total - first < run ? total - first : run);
    const uint64_t mask = ((uint64_t)1 << m) - 1;
    const auto slot = [&](uint32_t i) {
        const uint64_t e = first + i;
        return permute ? (e & ~mask) | frntt_rev(e & mask, m) : e;
    };
    to_affine_run<F>(
        count, [&](uint32_t i) { return load(first + i); }, [&](uint32_t i, const aff<F>& a) { store(slot(i), a); }, [&](uint32_t i) { store_inf(slot(i)); });
}

}  // namespace bls
