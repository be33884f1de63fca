// The two host decisions of key admission of csrc/plan.hpp (admit_survivors, admit_merge) as a host library for ctypes -
// tests/test_key_table_plan.py.  With -DPLAN_KEYTABLE_MAIN the same file is a stand-alone program (its own main) that walks the cases of that
// test once, for a run under the host sanitizers (tests/host_emu/build_keytable.sh main).
#include "plan.hpp"
using namespace plan;

extern "C" {
uint32_t keytable_plan_bad_proof(void) { return ADMIT_BAD_PROOF; }
uint32_t keytable_plan_gather_threads(void) { return GATHER_THREADS; }
// the workgroups k_admit_records (80 words per record) and k_admit_zero_rows (24 words per row) are launched with
uint32_t keytable_plan_record_blocks(size_t m) { return gather_blocks_for(m * 80); }
uint32_t keytable_plan_zero_blocks(size_t m) { return gather_blocks_for(m * 24); }
// status bytes of the two decoders -> list (room for n entries); returns the number of survivors
size_t keytable_plan_survivors(const uint8_t* key_st, const uint8_t* proof_st, size_t n, uint32_t* list) { return admit_survivors(key_st, proof_st, n, list); }
// verdicts of the m packed pairs -> status (n bytes), zero (room for n entries): the refused rows whose key decoded; returns their number
size_t keytable_plan_merge(const uint8_t* key_st, const uint8_t* proof_st, size_t n, const uint32_t* list, const uint8_t* verdicts, size_t m, uint8_t* status,
                           uint32_t* zero) {
    return admit_merge(key_st, proof_st, n, list, verdicts, m, status, zero);
}
}

#ifdef PLAN_KEYTABLE_MAIN
#include <cstdio>
#include <vector>

// one table: row i decodes when keep(i); every second survivor's verdict is 0.  Buffers are exactly as large as the contract says.
template <class Keep>
static int walk(size_t n, Keep keep) {
    std::vector<uint8_t> ks(n), ps(n);
    size_t want = 0;
    for (size_t i = 0; i < n; i++) {
        const bool k = keep(i);
        ks[i] = k ? 0 : (i % 3 == 0 ? 1 : 0);
        ps[i] = k ? 0 : (uint8_t)(4 + i % 2);
        want += k;
    }
    std::vector<uint32_t> list(n);
    const size_t m = admit_survivors(ks.data(), ps.data(), n, list.data());
    if (m != want) return 1;
    std::vector<uint8_t> verdicts(m), status(n);
    for (size_t j = 0; j < m; j++) verdicts[j] = j % 2 ? 1 : 0;
    std::vector<uint32_t> zero(n);
    const size_t nz = admit_merge(ks.data(), ps.data(), n, list.data(), verdicts.data(), m, status.data(), zero.data());
    size_t j = 0, z = 0;
    for (size_t i = 0; i < n; i++) {
        uint8_t w = ks[i] ? ks[i] : ps[i];
        if (keep(i)) {
            if (list[j] != i) return 3;
            if (!verdicts[j]) w = ADMIT_BAD_PROOF;
            j++;
        }
        if (status[i] != w) return 5;
        if (w && !ks[i] && (z >= nz || zero[z++] != i)) return 4;
    }
    if (z != nz) return 2;
    return 0;
}

int main() {
    int rc = 0;
    const size_t slice = 64;
    for (size_t n : {(size_t)0, (size_t)1, (size_t)63, (size_t)64, (size_t)65, slice + 1, (size_t)150, (size_t)4097}) {
        rc |= walk(n, [](size_t) { return true; });
        rc |= walk(n, [](size_t) { return false; });
        rc |= walk(n, [](size_t i) { return i % 2 == 0; });
        rc |= walk(n, [](size_t i) { return i % 2 == 1; });
    }
    for (size_t m : {(size_t)63, (size_t)64, (size_t)65})          // that many survivors among 200 rows
        rc |= walk(200, [m](size_t i) { return i >= 7 && i < 7 + m; });
    if (gather_blocks_for((size_t)65 * 80) != 21 || gather_blocks_for(0) != 0) rc |= 8;
    std::printf("plan_keytable: %s\n", rc ? "FAILED" : "ok");
    return rc;
}
#endif
