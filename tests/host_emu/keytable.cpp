// CPU execution of the key-table decoder (csrc/deser.hpp deserialize_public_key: what a lane of k_deser_pks runs) and of key admission's
// record gather (csrc/keytable.hpp admit_record_word: what a lane of k_admit_records runs) for tests/test_key_table_emu.py, bounds tracked
// like tests/host_emu/emu.hip.
// TEST INFRASTRUCTURE: never linked into the product library.
#include <cstring>

#include "fp.hpp"
#include "curve.hpp"
#include "deser.hpp"
#include "keytable.hpp"
using namespace bls;

extern "C" {
// mi355_bls_deserialize_public_keys: deser.hpp deserialize_public_key per key; images zeroed where the status is not 0.  1: every status 0
int emu_deserialize_public_keys(const uint8_t* pks, size_t n, uint32_t flags, uint8_t* out96, uint8_t* status) {
    int all = 1;
    for (size_t i = 0; i < n; i++) {
        g1_aff pk;
        status[i] = deserialize_public_key(pk, pks + i * ((flags & DESER_F_PK_UNCOMPRESSED) ? 96 : 48), flags);
        all &= status[i] == DESER_OK;
        if (status[i] != DESER_OK) pk = g1_aff{fp_zero(), fp_zero()};
        fp_store_le(out96 + i * 96, pk.x);
        fp_store_le(out96 + i * 96 + 48, pk.y);
    }
    return all;
}
// the key column and the status of deserialize_tuple with a signature that decodes: the key half stayed what the tuple decoder does
uint8_t emu_tuple_key(const uint8_t* pk, const uint8_t* sig96, uint32_t flags, uint8_t* out96) {
    g1_aff p;
    g2_aff s;
    const uint8_t st = deserialize_tuple(p, s, pk, sig96, flags & ~DESER_F_SIG_UNCOMPRESSED);
    if (st != DESER_OK) p = g1_aff{fp_zero(), fp_zero()};
    fp_store_le(out96, p.x);
    fp_store_le(out96 + 48, p.y);
    return st;
}
// k_admit_records word by word: keys n x 96 B, proofs n x 192 B, list m row numbers -> recs m x 320 B
void emu_admit_records(const uint8_t* keys, const uint8_t* proofs, const uint32_t* list, size_t m, uint8_t* recs) {
    uint32_t* out = reinterpret_cast<uint32_t*>(recs);
    for (size_t j = 0; j < m * ADMIT_RECORD_WORDS; j++)
        out[j] = admit_record_word(reinterpret_cast<const uint32_t*>(keys), reinterpret_cast<const uint32_t*>(proofs), list, j / ADMIT_RECORD_WORDS,
                                   (uint32_t)(j % ADMIT_RECORD_WORDS));
}
// k_pop_records' body as kernels.hip has it, for m pairs laid out contiguously
void emu_pop_records(const uint8_t* keys, const uint8_t* proofs, size_t m, uint8_t* recs) {
    const uint32_t *pks = reinterpret_cast<const uint32_t*>(keys), *prs = reinterpret_cast<const uint32_t*>(proofs);
    uint32_t* out = reinterpret_cast<uint32_t*>(recs);
    for (size_t j = 0; j < m * 80; j++) {
        const size_t i = j / 80;
        const uint32_t w = (uint32_t)(j % 80);
        out[j] = w < 24 ? pks[i * 24 + w] : w < 32 ? 0u : prs[i * 48 + (w - 32)];
    }
}
}
