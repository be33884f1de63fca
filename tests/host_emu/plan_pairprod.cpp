// The plan of the pairing-product calls (csrc/plan.hpp: aggveach_cut / aggveach_groups / aggveach_measure / aggveach_fill with_sig = false,
// pairprod_for, pairprod_blind_cut, pairprod_real_groups, pairprod_sizes_for) as a host library for ctypes - tests/test_pairprod_plan.py.  Built a
// second time as a program of its own (-DPLAN_PAIRPROD_MAIN, with sanitizers): main walks the tests' sweep and checks the same properties.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstdio>
#include <vector>
#include "plan.hpp"
using namespace plan;

extern "C" {
uint32_t pairprod_plan_c(void) { return AGGV_C; }
uint32_t pairprod_plan_max_levels(void) { return AGGV_MAX_LEVELS; }
void pairprod_plan_flags(uint32_t out[5]) { out[0] = AGGV_FINAL, out[1] = AGGV_SIG, out[2] = AGGV_COUNT, out[3] = AGGV_OPEN_IN, out[4] = AGGV_OPEN_OUT; }
// Walks a call as pairprod_run does.  form: 0 the sig-less plan, 1 aggveach_fill's defaulted form (today's tables, with signature lines),
// 2 the defaulted form spelled out (with_sig = true).  Every array may be null (a first call for the counts).  Per slice, 10 size_t: g0, g1,
// pos0, pos1, ng, open_in, open_out, levels, items, partials; the slices' groups and items (4 words each) follow each other.  counts:
// slices, groups, items.
void pairprod_plan_walk(const size_t* offsets, size_t k, size_t cap, int form, size_t* slices, uint32_t* groups, uint32_t* items, size_t counts[3]) {
    size_t ns = 0, ngr = 0, nit = 0, g = 0, pos = k ? offsets[0] : 0;
    for (;;) {
        const aggv_slice s = aggveach_cut(offsets, k, g, pos, cap);
        if (s.pairs() == 0) break;
        std::vector<aggv_group> gr(s.ng);
        aggveach_groups(offsets, s, gr.data());
        const aggveach_tab t = aggveach_measure(gr.data(), s.ng);
        if (slices) {
            size_t* o = slices + ns * 10;
            o[0] = s.g0, o[1] = s.g1, o[2] = s.pos0, o[3] = s.pos1, o[4] = s.ng, o[5] = s.open_in, o[6] = s.open_out;
            o[7] = t.levels, o[8] = t.items, o[9] = t.partials;
        }
        if (groups)
            for (uint32_t i = 0; i < s.ng; i++) {
                uint32_t* o = groups + (ngr + i) * 4;
                o[0] = gr[i].g, o[1] = gr[i].first, o[2] = gr[i].count, o[3] = gr[i].flags;
            }
        if (items) {
            agg_item* dst = reinterpret_cast<agg_item*>(items + nit * 4);
            if (form == 0) aggveach_fill(t, gr.data(), s.ng, dst, AGGV_C, false);
            else if (form == 1) aggveach_fill(t, gr.data(), s.ng, dst);
            else aggveach_fill(t, gr.data(), s.ng, dst, AGGV_C, true);
        }
        ns++, ngr += s.ng, nit += t.items;
        g = s.next_g(), pos = s.pos1;
    }
    counts[0] = ns, counts[1] = ngr, counts[2] = nit;
}
// The blinded form: the parts of n = offsets[k] pairs and the real groups of each.  Per part 4 size_t: pos0, pos1, open_in, open_out, then
// 2: the real groups' count and where they start in `groups` (4 words each: g, first, count, flags).  counts: parts, groups.
void pairprod_plan_blind(const size_t* offsets, size_t k, size_t cap, size_t* parts, uint32_t* groups, size_t counts[2]) {
    const size_t n = k ? offsets[k] : 0;
    size_t np = 0, ngr = 0;
    for (size_t pos = 0;;) {
        const aggv_slice s = pairprod_blind_cut(n, pos, cap);
        if (s.pairs() == 0) break;
        const aggv_slice rs = pairprod_real_groups(offsets, k, s.pos0, s.pos1);
        if (parts) {
            size_t* o = parts + np * 6;
            o[0] = s.pos0, o[1] = s.pos1, o[2] = s.open_in, o[3] = s.open_out, o[4] = rs.ng, o[5] = ngr;
        }
        if (groups && rs.ng) {
            std::vector<aggv_group> gr(rs.ng);
            aggveach_groups(offsets, rs, gr.data());
            for (uint32_t i = 0; i < rs.ng; i++) {
                uint32_t* o = groups + (ngr + i) * 4;
                o[0] = gr[i].g, o[1] = gr[i].first, o[2] = gr[i].count, o[3] = gr[i].flags;
            }
        }
        np++, ngr += rs.ng;
        pos = s.pos1;
    }
    counts[0] = np, counts[1] = ngr;
}
// a slice's launch shapes: setup_grid, lines.main_pairs, pkmul_spread, tail_engine, tail_grid
void pairprod_plan_for(uint32_t slots, int coop, uint32_t pairs, uint32_t ng, int blinded, uint32_t out[5]) {
    const pairprod_plan p = pairprod_for(slots, coop != 0, pairs, ng, blinded != 0);
    out[0] = p.setup_grid, out[1] = p.lines.main_pairs + p.lines.extra_pairs, out[2] = p.pkmul_spread, out[3] = p.tail_engine, out[4] = p.tail_grid;
}
void pairprod_plan_sizes(size_t n, size_t k, int blinded, size_t out[3]) {
    const pairprod_sizes s = pairprod_sizes_for(n, k, blinded != 0);
    out[0] = s.status, out[1] = s.flags, out[2] = s.scalars;
}
uint32_t pairprod_plan_validate_bit(void) { return PAIRPROD_VALIDATE; }
}

#ifdef PLAN_PAIRPROD_MAIN
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            std::printf("plan_pairprod: %s failed at line %d\n", #c, __LINE__);  \
            return 1;                                                             \
        }                                                                         \
    } while (0)
// one call: the sig-less walk's properties, exact-size arrays so that the sanitizers see every write
static int walk_one(const std::vector<size_t>& lens, size_t cap) {
    const size_t k = lens.size();
    std::vector<size_t> offs(k + 1, 0);
    for (size_t i = 0; i < k; i++) offs[i + 1] = offs[i] + lens[i];
    size_t counts[3];
    pairprod_plan_walk(offs.data(), k, cap, 0, nullptr, nullptr, nullptr, counts);
    std::vector<size_t> sl(counts[0] * 10);
    std::vector<uint32_t> gr(counts[1] * 4), it(counts[2] * 4), it1(counts[2] * 4), it2(counts[2] * 4);
    pairprod_plan_walk(offs.data(), k, cap, 0, sl.data(), gr.data(), it.data(), counts);
    pairprod_plan_walk(offs.data(), k, cap, 1, nullptr, nullptr, it1.data(), counts);
    pairprod_plan_walk(offs.data(), k, cap, 2, nullptr, nullptr, it2.data(), counts);
    CHECK(it1 == it2);                                             // the defaulted form is with_sig = true
    std::vector<uint32_t> finals(k, 0), parts(k, 0);
    size_t ga = 0, ia = 0, pos = 0;
    for (size_t s = 0; s < counts[0]; s++) {
        const size_t* o = sl.data() + s * 10;
        const size_t P = o[3] - o[2], ng = o[4], items = o[8], partials = o[9];
        CHECK(o[2] == pos && P > 0 && P <= cap);
        pos = o[3];
        std::vector<uint32_t> covered(P, 0);
        const aggveach_tab t = [&] {
            std::vector<aggv_group> g(ng);
            for (size_t i = 0; i < ng; i++) g[i] = aggv_group{gr[(ga + i) * 4], gr[(ga + i) * 4 + 1], gr[(ga + i) * 4 + 2], gr[(ga + i) * 4 + 3]};
            return aggveach_measure(g.data(), (uint32_t)ng);
        }();
        CHECK(t.items == items && t.partials == partials);
        for (size_t i = 0; i < items; i++) {
            const uint32_t *a = it.data() + (ia + i) * 4, *b = it1.data() + (ia + i) * 4;
            CHECK(!(a[1] & AGGV_SIG));
            CHECK(a[0] == b[0] && a[1] == (b[1] & ~AGGV_SIG) && a[2] == b[2] && a[3] == b[3]);      // the same table but for the signature bit
            if (i < t.level_first[1])
                for (uint32_t j = 0; j < (a[1] & AGGV_COUNT); j++) {
                    CHECK(a[0] + j < P);
                    covered[a[0] + j]++;
                }
            if (a[1] & AGGV_FINAL) {
                CHECK(a[2] < ng);
                finals[gr[(ga + a[2]) * 4]]++;
            } else {
                CHECK(a[2] < partials);
            }
        }
        for (size_t i = 0; i < P; i++) CHECK(covered[i] == 1);
        for (size_t i = 0; i < ng; i++) parts[gr[(ga + i) * 4]]++;
        ga += ng, ia += items;
    }
    CHECK(pos == offs[k]);
    for (size_t g = 0; g < k; g++) {
        const uint32_t want = lens[g] == 0 ? 0 : (uint32_t)(lens[g] <= cap ? 1 : (lens[g] + cap - 1) / cap);
        CHECK(finals[g] == parts[g] && parts[g] == want);             // one final item per part: FINAL items equal the groups' parts
        CHECK((lens[g] == 0) == (parts[g] == 0));
    }
    // the blinded form: parts of cap pairs; the real groups tile each part
    size_t bc[2];
    pairprod_plan_blind(offs.data(), k, cap, nullptr, nullptr, bc);
    std::vector<size_t> bp(bc[0] * 6);
    std::vector<uint32_t> bg(bc[1] * 4);
    pairprod_plan_blind(offs.data(), k, cap, bp.data(), bg.data(), bc);
    CHECK(bc[0] == (offs[k] + cap - 1) / cap);
    pos = 0;
    for (size_t p = 0; p < bc[0]; p++) {
        const size_t* o = bp.data() + p * 6;
        CHECK(o[0] == pos && o[1] - o[0] <= cap && (o[1] - o[0] == cap || o[1] == offs[k]));
        CHECK((o[2] != 0) == (p > 0) && (o[3] != 0) == (p + 1 < bc[0]));
        uint32_t at = 0;
        for (size_t i = 0; i < o[4]; i++) {
            const uint32_t* g = bg.data() + (o[5] + i) * 4;
            CHECK(g[1] == at && g[2] > 0 && g[0] < k);
            CHECK(offs[g[0]] <= o[0] + g[1] && o[0] + g[1] + g[2] <= offs[g[0] + 1]);
            at += g[2];
        }
        CHECK(at == o[1] - o[0]);
        pos = o[1];
    }
    CHECK(pos == offs[k]);
    return 0;
}
int main() {
    const size_t lens[] = {1, 2, 7, 8, 9, 63, 64, 65, 513};
    size_t cases = 0;
    for (size_t cap : {(size_t)64, (size_t)171, (size_t)257, (size_t)513, (size_t)4096})      // 513 pairs in nine, three, two parts and one
        for (size_t a : lens)
            for (size_t b : lens) {
                if (walk_one({a}, cap) || walk_one({0, a, 0, b, 0}, cap) || walk_one({b, a, a}, cap)) return 1;
                cases += 3;
            }
    if (walk_one({}, 64) || walk_one({0, 0}, 64)) return 1;
    uint32_t out[5];
    pairprod_plan_for(1024, 0, 4096, 1, 1, out);
    CHECK(out[3] == 1 && out[4] == 1 && out[0] == 64 && out[1] == 4096);
    pairprod_plan_for(1024, 0, 4096, 700, 0, out);
    CHECK(out[3] == 0 && out[4] == 11);
    std::printf("plan_pairprod: %zu cases clean\n", cases + 2);
    return 0;
}
#endif
