// Key admission (mi355_bls_admit_keys): the record gather behind the two decoders.  n keys and n proofs are decoded in place (row i of the
// key table, row i of the proof table); the rows whose status bytes are both 0 - the survivors, plan.hpp admit_survivors - go to popVerify's
// blinded batch check PACKED: record j of the pass is  key[list[j]] | 32 zero bytes | proof[list[j]],  the 80 words k_pop_records writes
// for pair j of a contiguous table, so everything behind the records (the PoP hash-map kernels, the slices, the verdict bytes) runs as for
// mi355_bls_batch_pop_verify_locate and a row that failed to decode costs the pass nothing.  One word of one record, written so that a lane
// can carry it and the host can run it; where the tables live is the caller's business.
#pragma once
#include <cstddef>
#include <cstdint>

#include "fp.hpp"

namespace bls {

constexpr uint32_t ADMIT_RECORD_WORDS = 80;      // 320 bytes: 24 words of key, 8 of (unused) message, 48 of proof

// word w of packed record j: keys n x 24 words, proofs n x 48 words, list = the survivors' row numbers
BLS_HD uint32_t admit_record_word(const uint32_t* keys, const uint32_t* proofs, const uint32_t* list, size_t j, uint32_t w) {
    const size_t row = list[j];
    return w < 24 ? keys[row * 24 + w] : w < 32 ? 0u : proofs[row * 48 + (w - 32)];
}

}  // namespace bls
