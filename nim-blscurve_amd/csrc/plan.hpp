// The host layer's launch plans: which kernel, what grid, which stream a stage of a call takes, as plain integer functions of the
// context's numbers (wave slots, capacity, mode) and the call's size.  host_api.inc asks for a plan and launches what it says; the CPU
// tests call the same functions through tests/host_emu/plan.cpp.  No device type, no context: numbers in, small structs out.
#ifndef BLS_PLAN_HPP
#define BLS_PLAN_HPP
#include <cstddef>
#include <cstdint>

namespace plan {

constexpr uint32_t WAVE = 64;                // lanes of a wavefront: the workgroup of every one-lane-per-item kernel
constexpr uint32_t N_LINES = 68;             // steps of the Miller loop (pairing.hpp)
constexpr uint32_t FP_WORDS = 16;            // 32-bit words of an Fp element in device buffers; a G1 Jacobian point takes 3, a G2 one 6, an Fp12 value 12 of them
constexpr uint32_t G1_WORDS = 3 * FP_WORDS, G2_WORDS = 6 * FP_WORDS, F12_WORDS = 12 * FP_WORDS;
constexpr uint32_t SIG_SLOTS_MAX = 2048;     // 8 windows x 256 digits: the most extra pairs a slice has
static_assert(((64u / 8) << 8) == SIG_SLOTS_MAX, "the buckets of the 8-bit digits");
constexpr size_t SIG_WIDE_MIN = 40000;       // from here 8-bit digits (2048 extra pairs, 8 additions per tuple) beat 4-bit ones (256, 15)
constexpr uint32_t FORK_ITEMS_PER_SLOT = 16; // [r]PK and the signature side on the two fork streams up to 16 sets per slot, the signature side's stream alone beyond

// Latency mode: how many messages / pairs the lane-team engine (16 lanes each, csrc/teamvm.hpp) takes before one lane each is the faster form.
// The engine spends ~4 x the instructions of the one-lane kernels per item (sixteen lanes run the same ~700-instruction round for one product
// each), so it wins exactly while the device has SIMDs to spare: `slots` = one wave per SIMD = 4 x slots items per 0.63 ms (clearing) / 0.33 ms
// (lines), against 2.9 ms / 1.9 ms per round of one-lane waves whatever their number.  Measured crossovers: profiles/r06_ab/team_sweep.txt.
constexpr uint32_t TEAM_CLEAR_ITEMS_PER_SLOT = 11, TEAM_LINES_ITEMS_PER_SLOT = 18;
inline uint32_t team_clear_max(uint32_t slots) { return slots * TEAM_CLEAR_ITEMS_PER_SLOT; }
inline uint32_t team_lines_max(uint32_t slots) { return slots * TEAM_LINES_ITEMS_PER_SLOT; }

// waves of a kernel that gives every item one lane
inline uint32_t waves_for(uint32_t count) { return (count + WAVE - 1) / WAVE; }
// the same for the one kernel whose workgroups are four waves (k_combsets_gather: a lane per word of 80-word records, so the count is a size_t)
constexpr uint32_t GATHER_THREADS = 256;
inline uint32_t gather_blocks_for(size_t count) { return (uint32_t)((count + GATHER_THREADS - 1) / GATHER_THREADS); }

// Which executor of the lane-team engine takes `count` items, the same ladder for clearing and Miller lines:
//   ROWS   the row executor (four waves per item) while the grid stays well inside one wave per SIMD;
//   ROWS2  the same at two workgroups per CU up to twice that: 240 sets 3.10 -> 2.72 ms, 400 3.15 -> 3.01, 448 3.16 -> 3.10
//          (profiles/r06_ab/ab_rows2.txt);
//   SPREAD one wave (four items) per SIMD while the waves fit the device's slots;
//   WIDE   the plain grid beyond.
enum team_form { TEAM_ROWS, TEAM_ROWS2, TEAM_SPREAD, TEAM_WIDE };
inline uint32_t team_rows_max(uint32_t slots) { return (slots - slots / 8) / 4; }      // room left for the fork streams' waves
inline team_form team_form_for(uint32_t slots, uint32_t count) {
    const uint32_t rows_max = team_rows_max(slots);
    if (count <= rows_max) return TEAM_ROWS;
    if (count <= 2 * rows_max) return TEAM_ROWS2;
    return (count + 3) / 4 <= slots ? TEAM_SPREAD : TEAM_WIDE;
}

// A stage that the engine (`team`: in `form`, `grid` workgroups of 256 lanes for the row forms, of one wave otherwise) or the one-lane
// kernel (`grid` waves) takes.
struct stage {
    bool team;
    team_form form;
    uint32_t grid;
};
inline stage team_stage(uint32_t slots, uint32_t count) {
    const team_form f = team_form_for(slots, count);
    return {true, f, f == TEAM_ROWS || f == TEAM_ROWS2 ? count : (count + 3) / 4};
}
inline stage one_lane_stage(uint32_t count) { return {false, TEAM_WIDE, waves_for(count)}; }

// 320-byte records -> the two mapped points of every message (two lanes per message)
enum hash_map_form { HASH_MAP_ROWS, HASH_MAP_SPREAD, HASH_MAP_PLAIN };
struct hash_map_plan {
    hash_map_form form;
    uint32_t grid;
};
inline hash_map_plan hash_map_for(uint32_t slots, bool coop, uint32_t n32) {
    const uint32_t waves = (2 * n32 + WAVE - 1) / WAVE;
    if (coop && (2 * n32 + 3) / 4 <= slots - slots / 8) return {HASH_MAP_ROWS, (2 * n32 + 3) / 4};      // a pair per row (room left for the fork streams' waves: a second round would double the time)
    if (coop && waves <= slots) return {HASH_MAP_SPREAD, waves};                                         // one wave per SIMD
    return {HASH_MAP_PLAIN, waves};
}

// popVerify's records (k_pop_records: a lane per word of n 80-word records, workgroups of four waves).  The PoP hash-map kernels take
// hash_map_for's plan as it is: same forms, same hand-over sizes.  POP_MAX_KEYS: what a context's capacity is bounded by, too.
constexpr size_t POP_MAX_KEYS = (size_t)1 << 30;
constexpr uint32_t POP_RECORD_THREADS = 256;
inline uint32_t pop_records_grid(size_t n) { return (uint32_t)((n * 80 + POP_RECORD_THREADS - 1) / POP_RECORD_THREADS); }

// Key admission (mi355_bls_admit_keys): the two host decisions between the decoders and the possession check.  key_st / proof_st are the
// status bytes k_deser_pks / k_deser_sigs wrote for the n rows (0 = decoded).
//   admit_survivors   the rows both decoders accepted, in row order -> list (room for n entries); returns their number m.  Only these rows
//                     go to the blinded batch check, packed (k_admit_records: gather_blocks_for(m * 80) workgroups), so a row that failed
//                     to decode never sends the others to the per-pair pass.
//   admit_merge       the verdict bytes of the m packed pairs go back to their rows.  status[i] = the key's status if it is not 0, else the
//                     proof's if it is not 0, else ADMIT_BAD_PROOF when the pair's verdict is not 1, else 0.  zero (room for n entries) takes
//                     the refused rows whose KEY decoded - a proof that did not decode, or one the check refused: the key decoder left an
//                     image there, and a refused row of the table is all zero (k_admit_zero_rows).  Returns their number.
constexpr uint8_t ADMIT_BAD_PROOF = 8;
inline size_t admit_survivors(const uint8_t* key_st, const uint8_t* proof_st, size_t n, uint32_t* list) {
    size_t m = 0;
    for (size_t i = 0; i < n; i++)
        if (key_st[i] == 0 && proof_st[i] == 0) list[m++] = (uint32_t)i;
    return m;
}
inline size_t admit_merge(const uint8_t* key_st, const uint8_t* proof_st, size_t n, const uint32_t* list, const uint8_t* verdicts, size_t m, uint8_t* status,
                          uint32_t* zero) {
    for (size_t i = 0; i < n; i++) status[i] = key_st[i] ? key_st[i] : proof_st[i];
    for (size_t j = 0; j < m; j++)
        if (verdicts[j] != 1) status[list[j]] = ADMIT_BAD_PROOF;
    size_t nz = 0;
    for (size_t i = 0; i < n; i++)
        if (status[i] != 0 && key_st[i] == 0) zero[nz++] = (uint32_t)i;
    return nz;
}

// cofactor clearing of n32 mapped point pairs: the engine (then k_clear_fix) or k_hash_clear
inline stage clear_for(uint32_t slots, bool coop, uint32_t n32) {
    return coop && n32 <= team_clear_max(slots) ? team_stage(slots, n32) : one_lane_stage(n32);
}

// Miller lines of pairs 0 .. npairs-1 (the last `extra` of them are the bucket pairs of the signature side): the engine while that does
// not take more waves than the device has slots.  Whole-device batches in latency mode (coop): the tuple pairs fill the device exactly, so the
// few extra pairs would be a second round of waves that takes as long as the first (2.2 ms at 3 % occupancy); on the engine they take
// ~1 ms instead.  In throughput mode (several batches in flight) that second round overlaps other batches' kernels and one lane per
// pair is the cheaper form.
// -> pairs [0, main_pairs) as `main` says, then pairs [main_pairs, main_pairs + extra_pairs) on the engine as `extra` says (none: extra_pairs = 0)
struct lines_plan {
    uint32_t main_pairs;
    stage main;
    uint32_t extra_pairs;
    stage extra;
};
inline lines_plan lines_for(uint32_t slots, bool coop, uint32_t npairs, uint32_t extra) {
    if (coop && npairs <= team_lines_max(slots)) return {npairs, team_stage(slots, npairs), 0, {}};
    if (coop && extra && extra < npairs && extra <= team_lines_max(slots) &&
        (npairs + WAVE - 1) / WAVE > slots * (((npairs - extra + WAVE - 1) / WAVE + slots - 1) / slots)) {
        // the extra pairs would start one more round of waves: a team of lanes each instead
        const uint32_t main_pairs = npairs - extra;
        return {main_pairs, one_lane_stage(main_pairs), extra, team_stage(slots, extra)};
    }
    return {npairs, one_lane_stage(npairs), 0, {}};
}

// One batch slice of n sets (what run_pairs follows).  The three producers of Miller pairs are independent until the lines: hashing,
// [r]PK and the signature side (bucket fold).
//   SIDE_NONE      everything on the caller's stream (throughput mode, or no fork stream could be created);
//   SIDE_FORK      a small batch in latency mode: [r]PK on a fork stream of its own, the signature side on the other, beside the hashing;
//   SIDE_FORK_SIG  a whole-device batch of one caller: only the signature side (and its extra pairs' lines) beside the hashing.
enum side_mode { SIDE_NONE, SIDE_FORK, SIDE_FORK_SIG };
// [r]PK of n sets: k_pkmul_spread (one wave per SIMD) while the grid is at most a wave per slot in latency mode | k_pkmul
inline bool pkmul_spread_for(uint32_t slots, bool coop, uint32_t n) { return coop && waves_for(n) <= slots; }
enum stream_role { STREAM_CALLER, STREAM_SIDE, STREAM_SIDE2 };
struct slice_plan {
    uint32_t nb;                       // waves of the one-lane-per-set kernels ([r]PK, the signature side's conversion, histogram, scatter)
    hash_map_plan hash_map;
    stage clear;
    bool pkmul_spread;                 // k_pkmul_spread (one wave per SIMD) | k_pkmul
    side_mode side;
    stream_role pk_stream, sig_stream; // [r]PK; the signature side (and the extra pairs' lines where they run apart)
    uint32_t cw, nwin, total;          // the signature side's digit width, its windows, its buckets = the extra Miller pairs
    uint32_t lshift, bucket_grid;      // k_sig_bucket: 2^lshift lanes per bucket
    bool extra_apart;                  // the extra pairs' lines follow the signature side on its stream; the caller's stream walks the tuple pairs alone
    stage extra_lines;                 //   their form there
    lines_plan lines;                  // the caller's stream: the tuple pairs (extra_apart) or all n + total pairs
};
inline slice_plan slice_for(uint32_t slots, bool coop, bool have_side, size_t n) {
    slice_plan p{};
    const uint32_t n32 = (uint32_t)n;
    p.nb = waves_for(n32);
    const bool fork = have_side && n32 <= FORK_ITEMS_PER_SLOT * slots;      // pk + signature side beside the hashing
    const bool fork_sig = !fork && have_side;
    p.side = fork ? SIDE_FORK : fork_sig ? SIDE_FORK_SIG : SIDE_NONE;
    p.pk_stream = fork ? STREAM_SIDE2 : STREAM_CALLER;
    p.sig_stream = (fork || fork_sig) ? STREAM_SIDE : STREAM_CALLER;
    p.hash_map = hash_map_for(slots, coop, n32);
    p.clear = clear_for(slots, coop, n32);
    p.pkmul_spread = pkmul_spread_for(slots, coop, n32);
    // the signature side as a bucket fold: `total` extra Miller pairs n .. n + total - 1 (every batch size: for a handful of tuples the
    // 256 nearly empty buckets are still cheaper than one 64-bit G2 multiplication per tuple)
    p.cw = n >= SIG_WIDE_MIN ? 8 : 4, p.nwin = 64 / p.cw, p.total = p.nwin << p.cw;
    uint32_t per = n32 >> p.cw, lshift = 0;                     // expected entries per bucket; ~16 per lane
    const uint32_t per_lane_min = coop ? 16u : 64u;             // throughput mode: fewer, longer lanes (the fold of a bucket's lanes is pure overhead)
    while (lshift < 6 && (per >> (lshift + 1)) >= per_lane_min) lshift++;
    // small batches leave most of the device idle: more lanes per bucket (down to ~2 entries per lane) shorten the kernel
    while (lshift < 6 && ((p.total << (lshift + 1)) <= 16 * slots) && (per >> (lshift + 1)) >= 2) lshift++;
    p.lshift = lshift;
    p.bucket_grid = ((p.total << lshift) + WAVE - 1) / WAVE;
    // the extra pairs' walk beside the hashing, on the engine where they fit it (one blocking 65 536-set call: 12.7 -> 12.0 ms); a forked
    // small batch whose extra pairs do not fit the engine leaves them to the caller's stream
    p.extra_apart = fork_sig || (fork && p.total <= team_lines_max(slots));
    p.extra_lines = p.total <= team_lines_max(slots) ? team_stage(slots, p.total) : one_lane_stage(p.total);
    p.lines = p.extra_apart ? lines_for(slots, coop, n32, 0) : lines_for(slots, coop, n32 + p.total, p.total);
    return p;
}

// The per-step products of the Miller lines of pairs 0 .. npairs-1: k_lineprod's grid (N_LINES x nblk, m pairs per lane), then the fold of
// the 64 x nblk partial products per step.  `fold` (latency mode, or a call alone on the device): k_fold on the lane-cooperative engine,
// two levels of about sqrt(live) dependent products each - nb1 blocks of `per`, then the nb1 block results (one caller, 65 536 tuples:
// 1.8 -> 0.35 ms); otherwise k_lineprod2's 68 waves, 15 sequential Fp12 products per lane + one shuffle tree (least total work).
struct lineprod_plan {
    uint32_t nblk, m;
    int per_lane;                      // 1: the assembly loop (32-bit byte offsets inside one step's 24 planes); 2: the compiled loop
    uint32_t live, per, nb1;           // fold only
};
inline lineprod_plan lineprod_for(uint32_t slots, uint32_t nblk_cap, uint32_t stride, uint32_t npairs, bool fold) {
    lineprod_plan p{};
    uint32_t nblk = slots / N_LINES;
    if (nblk < 1) nblk = 1;
    if (nblk > nblk_cap) nblk = nblk_cap;
    uint32_t m = (npairs + WAVE * nblk - 1) / (WAVE * nblk);
    if (m < 1) m = 1;
    nblk = (npairs + WAVE * m - 1) / (WAVE * m);
    p.nblk = nblk, p.m = m;
    p.per_lane = (uint64_t)stride * 16 * 24 + (uint64_t)npairs * 16 < (1ull << 32) ? 1 : 2;
    if (fold) {
        size_t first_last = (size_t)(nblk - 1) * WAVE * m;             // lanes past the last pair hold 1: not folded
        p.live = (nblk - 1) * WAVE + (npairs - first_last < WAVE ? (uint32_t)(npairs - first_last) : WAVE);
        p.per = 1;
        while (p.per * p.per < p.live) p.per++;
        p.nb1 = (p.live + p.per - 1) / p.per;
    }
    return p;
}

// The context's own sizes (ctx_build allocates what this says): `stride` pairs per plane of the pair store (the tuple pairs, the (-G1, sig) pair
// and the extra pairs of the signature side, in whole waves), `mstride` mapped points, the most pair ranges k_lineprod may be given (nblk <=
// slots / 68, at most 64, and never more ranges than waves of pairs), and d_lpart: per Miller step nblk_cap x 64 per-lane partial products of
// k_lineprod, then, from lpart_mid_words on, k_fold's first-level results (nb1 <= nblk_cap + 64 per step).  d_export holds `stride` exported G2
// points (288 bytes each) and, beside them, SUM_PARTS_BYTES for the partials of the point sums below and the images mi355_bls_p1s_add /
// p2s_add stage.
constexpr uint32_t LINEPROD_RANGES_MAX = 64, FOLD_MID_ROOM = 64;
constexpr uint32_t SUM_G2_PARTS_MAX = 2048;
constexpr size_t SUM_PARTS_BYTES = 2048 * 2 * G1_WORDS * 4;
static_assert((size_t)SUM_G2_PARTS_MAX * G2_WORDS * 4 == SUM_PARTS_BYTES, "2048 G2 partials, or twice as many G1 ones");
struct ctx_sizes {
    size_t stride, mstride;
    uint32_t nblk_cap;
    size_t lpart_words, lpart_mid_words;
    size_t export_bytes;
};
inline size_t lpart_mid_words(uint32_t nblk_cap) { return (size_t)N_LINES * nblk_cap * WAVE * F12_WORDS; }
inline ctx_sizes ctx_for(uint32_t slots, size_t max_sets) {
    ctx_sizes s{};
    s.stride = ((max_sets + 1 + SIG_SLOTS_MAX + WAVE - 1) / WAVE) * WAVE;
    s.mstride = ((2 * max_sets + WAVE - 1) / WAVE) * WAVE;
    const size_t nwaves = s.stride / WAVE;
    uint32_t nblk = slots / N_LINES;
    if (nblk < 1) nblk = 1;
    if (nblk > LINEPROD_RANGES_MAX) nblk = LINEPROD_RANGES_MAX;
    if (nblk > nwaves) nblk = (uint32_t)nwaves;
    s.nblk_cap = nblk;
    s.lpart_words = (size_t)N_LINES * (nblk * (WAVE + 1) + FOLD_MID_ROOM) * F12_WORDS;
    s.lpart_mid_words = lpart_mid_words(nblk);
    s.export_bytes = s.stride * 288 + SUM_PARTS_BYTES;
    return s;
}

// Point sums (k_g1_sum / k_g2_sum, then one wave over the partials): nblk waves, lane l of wave b sums points (64 b + l) + j 64 nblk, j < m -
// about 8 points per lane while the device has waves to give (G1: two per slot, G2: one), more per lane beyond.  Every wave leaves one partial
// at the start of d_export: G1_WORDS (G2_WORDS) words each, within SUM_PARTS_BYTES.
struct sum_plan {
    uint32_t nblk, m;
};
inline sum_plan sum_for(uint32_t nblk_max, uint32_t n) {
    uint32_t nblk = (n + WAVE * 8 - 1) / (WAVE * 8);
    if (nblk > nblk_max) nblk = nblk_max;
    if (nblk < 1) nblk = 1;
    return {nblk, (n + nblk * WAVE - 1) / (nblk * WAVE)};
}
inline sum_plan g1_sum_for(uint32_t slots, uint32_t n) { return sum_for(slots < SUM_G2_PARTS_MAX ? slots * 2 : SUM_G2_PARTS_MAX * 2, n); }
inline sum_plan g2_sum_for(uint32_t slots, uint32_t n) { return sum_for(slots < SUM_G2_PARTS_MAX ? slots : SUM_G2_PARTS_MAX, n); }

// aggregateVerify's greedy slice [a, b): at most cap pairs, and the staged bytes (n + 1 offsets | per pair a 96-byte key and the message)
// within the cap * 320 bytes of the staging buffer.  b == a: the message at `a` alone does not fit.
inline size_t aggv_cut(const uint32_t* msg_offsets, size_t n, size_t a, size_t cap) {
    const size_t budget = cap * 320;
    size_t b = a, bytes = 4;
    while (b < n && b - a < cap) {
        size_t add = 96 + 4 + (msg_offsets[b + 1] - msg_offsets[b]);
        if (bytes + add > budget) break;
        bytes += add;
        b++;
    }
    return b;
}
// every message of the slice 32 bytes long (signing roots): the batch path's hashing kernels can take it
inline bool aggv_all32(const uint32_t* offs, size_t n) {
    bool all32 = true;
    for (size_t i = 0; i < n && all32; i++) all32 = offs[i + 1] - offs[i] == 32;
    return all32;
}

// A shard of n tuples on a workspace of `cap`: ceil(n / cap) balanced slices (never a sliver at the end), pipelined over up to three
// workspaces - slice i of nslices on workspace (nslices - 1 - i) mod nl, so that the last slice runs on workspace 0, the caller's own.
inline size_t shard_nslices(size_t n, size_t cap) { return (n + cap - 1) / cap; }
inline int shard_workspaces(size_t nslices) { return nslices >= 3 ? 3 : 2; }
inline size_t shard_slice_count(size_t n, size_t done, size_t nslices, uint32_t slice) {
    size_t left = nslices - slice;
    return (n - done + left - 1) / left;
}
inline int shard_workspace_of(size_t nslices, uint32_t slice, int nl) { return (int)((nslices - 1 - slice) % (size_t)nl); }

// Per-set verification (mi355_bls_verify_each): n sets in balanced slices of at most `cap` sets.  A slice of m sets puts 2 m pairs through
// a line store of its own (2 cap pairs, made at the first such call): pair i = (pk_i, H(msg_i)), pair m + i = (-G1, sig_i), so a call of
// cap sets is ONE slice.  Hashing and Miller lines take the forms the batch path takes for the same counts (clear_for on m messages,
// lines_for on 2 m pairs: the lane-team engine up to each_team_clear_max / each_team_lines_max sets in latency mode, one lane per item
// beyond).  The tail - Horner, final exponentiation, comparison - has two forms: the lane-cooperative Fp12 engine, a workgroup per set and
// each_engine_grid workgroups at a time (two per CU: 66 KB of LDS each), in latency mode up to each_engine_max sets; one lane per set
// (k_each_tail) beyond and in throughput mode.  Measured around every hand-over: profiles/verify_each_sweep.txt.
constexpr uint32_t EACH_ENGINE_SETS_PER_SLOT = 7;      // 4.4 ms per S sets on the engine against the lane form's flat 36 ms: level near 8 S
inline size_t each_slice_max(size_t cap) { return cap; }
inline size_t each_stride(size_t cap) { return ((2 * cap + 63) / 64) * 64; }
inline size_t each_nslices(size_t n, size_t slice_max) { return shard_nslices(n, slice_max); }
inline size_t each_slice_count(size_t n, size_t done, size_t nslices, uint32_t slice) { return shard_slice_count(n, done, nslices, slice); }
inline uint32_t each_team_clear_max(uint32_t slots) { return team_clear_max(slots); }
inline uint32_t each_team_lines_max(uint32_t slots) { return team_lines_max(slots) / 2; }
inline uint32_t each_engine_max(uint32_t slots) { return slots * EACH_ENGINE_SETS_PER_SLOT; }
inline uint32_t each_engine_grid_max(uint32_t slots) { return slots / 2 ? slots / 2 : 1; }
struct each_plan {
    uint32_t setup_grid;               // k_each_setup: one lane per set
    lines_plan lines;                  // all 2 m pairs in one form
    bool tail_engine;                  // k_each_engine(_rows): tail_grid workgroups, each walks sets i, i + tail_grid, ... | k_each_tail: tail_grid waves
    uint32_t tail_grid;
};
inline each_plan each_for(uint32_t slots, bool coop, uint32_t m) {
    each_plan p{};
    p.setup_grid = waves_for(m);
    p.lines = lines_for(slots, coop, 2 * m, 0);
    p.tail_engine = coop && m <= each_engine_max(slots);
    p.tail_grid = p.tail_engine ? (m < each_engine_grid_max(slots) ? m : each_engine_grid_max(slots)) : waves_for(m);
    return p;
}

// Per-set key aggregation (mi355_bls_aggregate_sets): k segments of keys in CSR form (segment s = keys [offsets[s], offsets[s + 1])) summed
// in levels of one-lane items.  A level-0 item reads up to AGG_C consecutive keys of ONE segment and writes one Jacobian partial; an item of a
// higher level reads up to AGG_C consecutive partials of one segment (all written by the level below) and writes one.  A segment leaves the
// plan at the level that gives it a single partial, whose index is final_of[s] (AGG_NONE: the segment is empty and has no item at all), so
// the levels number ceil(log_C(longest segment)), at least one, and the work is sum ceil(len / C) + k however the lengths are spread: 65 536
// segments of one key are one level of 65 536 items, one segment of 2^20 keys is seven levels of 131 072, 16 384, ... 1 items.
// Partials are numbered like the items that write them (item i of the table writes partial i: dst == its position), level after level, so
// the partial buffer holds `items` points and nothing is overwritten while a later level still reads it.
constexpr uint32_t AGG_C = 8;                // keys / partials per item: the "~8 points per lane" of the single-aggregate sum
constexpr uint32_t AGG_MAX_LEVELS = 11;      // 8^11 > 2^32 keys
constexpr uint32_t AGG_NONE = 0xffffffffu;
static_assert(AGG_C >= 2, "a level must shrink a segment");
struct agg_item {
    uint32_t src_first, count, dst, seg;     // level 0: keys src_first .. + count of segment seg; above: partials; -> partial dst
};
struct aggsets_plan {
    bool ok;                                 // false: more than 2^32 - 2 keys or items (the tables are 32-bit), or offsets that decrease
    uint32_t levels;
    size_t level_first[AGG_MAX_LEVELS + 1];  // items [level_first[l], level_first[l + 1]) are level l
    size_t items;                            // = level_first[levels] = the partials the context's buffer must hold
};
inline size_t agg_ceil_div(size_t a) { return (a + AGG_C - 1) / AGG_C; }
// pass 1: the levels and their sizes (offsets: k + 1 entries, non-decreasing)
inline aggsets_plan aggsets_measure(const size_t* offsets, size_t k) {
    aggsets_plan p{};
    size_t per_level[AGG_MAX_LEVELS] = {};
    for (size_t s = 0; s < k; s++) {
        if (offsets[s + 1] < offsets[s]) return p;
        size_t n = offsets[s + 1] - offsets[s];
        if (offsets[s + 1] >= AGG_NONE) return p;
        uint32_t l = 0;
        while (n > 0) {                      // n things (keys, then partials) -> ceil(n / C) partials, until there is one
            n = agg_ceil_div(n);
            per_level[l++] += n;
            if (l > p.levels) p.levels = l;
            if (n == 1) break;
        }
    }
    for (uint32_t l = 0; l < p.levels; l++) p.level_first[l + 1] = p.level_first[l] + per_level[l];
    p.items = p.level_first[p.levels];
    p.ok = p.items < AGG_NONE;
    return p;
}
// pass 2: the item table (p.items entries) and final_of (k entries), one walk over the segments
inline void aggsets_fill(const aggsets_plan& p, const size_t* offsets, size_t k, agg_item* items, uint32_t* final_of) {
    size_t cur[AGG_MAX_LEVELS];
    for (uint32_t l = 0; l < AGG_MAX_LEVELS; l++) cur[l] = l < p.levels ? p.level_first[l] : 0;
    for (size_t s = 0; s < k; s++) {
        size_t n = offsets[s + 1] - offsets[s], src = offsets[s];
        final_of[s] = AGG_NONE;
        for (uint32_t l = 0; n > 0; l++) {
            const size_t m = agg_ceil_div(n), base = cur[l];
            for (size_t j = 0; j < m; j++) {
                const size_t left = n - j * AGG_C;
                items[base + j] = agg_item{(uint32_t)(src + j * AGG_C), (uint32_t)(left < AGG_C ? left : AGG_C), (uint32_t)(base + j), (uint32_t)s};
            }
            cur[l] += m;
            src = base, n = m;
            if (m == 1) {
                final_of[s] = (uint32_t)base;
                break;
            }
        }
    }
}

// Key aggregation by participation bits (mi355_bls_aggregate_sets_bits): m committees in CSR form (committee c = positions [c_offsets[c],
// c_offsets[c + 1]) of the key sequence) and k sets, set s naming committee which[s] and owning ceil(L / 8) bytes of the packed bit fields
// (L = its committee's length; SSZ order: position i is bit i % 8 of byte i / 8).  The same levelled one-lane-item segmented sum as
// aggsets_fill, laid over the committee POSITIONS of every set: the layout depends on the committee lengths alone, never on the bits, so
// the device form needs no read-back before it.  A level-0 item covers AGGB_P consecutive positions of one set - its src_first is the
// position of the first one in the key sequence, and, because at level 0 dst is the item's own number, that word carries the offset of the
// item's first byte in the bit fields instead (partial i is written by item i, as above).  Levels above are aggsets_fill's own: AGG_C
// partials per item.  Per set the table keeps where its field starts, its length, its committee and final_of (AGG_NONE only for a
// committee of length 0).
//   AGGB_P = 8: one byte of the field per lane, the first choice; no other value was tried (32, a word of bits per lane, is the one that
//   would halve the level-0 partials at four times the serial additions of a lane).
constexpr uint32_t AGGB_P = 8;
static_assert(AGGB_P % 8 == 0 && AGGB_P >= 8 && AGGB_P <= 32, "a level-0 item owns whole bytes of a field and selects through one 32-bit word");
struct aggb_set {
    uint32_t bits_first, len, committee, final_of;   // first byte of the set's field; committee length; committee; the set's last partial
};
struct aggbits_plan {
    bool ok;                                 // false: offsets decrease, a which[s] >= m, or 2^32 - 1 or more positions, sets, items or field bytes
    uint32_t levels;
    size_t level_first[AGG_MAX_LEVELS + 1];
    size_t items;
    size_t bits_bytes;                       // the packed fields of all k sets
};
inline aggbits_plan aggbits_measure(const size_t* c_offsets, size_t m, const uint32_t* which, size_t k) {
    aggbits_plan p{};
    for (size_t c = 0; c < m; c++)
        if (c_offsets[c + 1] < c_offsets[c]) return p;
    if (k >= AGG_NONE || (m && c_offsets[m] >= AGG_NONE)) return p;
    size_t per_level[AGG_MAX_LEVELS] = {};
    for (size_t s = 0; s < k; s++) {
        if (which[s] >= m) return p;
        const size_t len = c_offsets[which[s] + 1] - c_offsets[which[s]];
        p.bits_bytes += (len + 7) / 8;
        size_t n = (len + AGGB_P - 1) / AGGB_P;
        for (uint32_t l = 0; n > 0;) {       // ceil(len / P) partials, then aggsets_measure's levels until there is one
            per_level[l++] += n;
            if (l > p.levels) p.levels = l;
            if (n == 1) break;
            n = agg_ceil_div(n);
        }
        if (per_level[0] >= AGG_NONE || p.bits_bytes >= AGG_NONE) return p;      // (keeps the sums far from wrapping, whatever k is)
    }
    for (uint32_t l = 0; l < p.levels; l++) p.level_first[l + 1] = p.level_first[l] + per_level[l];
    p.items = p.level_first[p.levels];
    p.ok = p.items < AGG_NONE;
    return p;
}
// the item table (p.items entries) and the set table (k entries), one walk over the sets
inline void aggbits_fill(const aggbits_plan& p, const size_t* c_offsets, const uint32_t* which, size_t k, agg_item* items, aggb_set* sets) {
    size_t cur[AGG_MAX_LEVELS];
    for (uint32_t l = 0; l < AGG_MAX_LEVELS; l++) cur[l] = l < p.levels ? p.level_first[l] : 0;
    size_t byte = 0;
    for (size_t s = 0; s < k; s++) {
        const size_t first = c_offsets[which[s]], len = c_offsets[which[s] + 1] - first;
        sets[s] = aggb_set{(uint32_t)byte, (uint32_t)len, which[s], AGG_NONE};
        size_t n = (len + AGGB_P - 1) / AGGB_P, src = 0;
        for (uint32_t l = 0; n > 0; l++) {
            const size_t base = cur[l];
            if (l == 0) {
                for (size_t j = 0; j < n; j++) {
                    const size_t left = len - j * AGGB_P;
                    items[base + j] = agg_item{(uint32_t)(first + j * AGGB_P), (uint32_t)(left < AGGB_P ? left : AGGB_P), (uint32_t)(byte + j * (AGGB_P / 8)), (uint32_t)s};
                }
            } else {
                const size_t below = n;
                n = agg_ceil_div(below);
                for (size_t j = 0; j < n; j++) {
                    const size_t left = below - j * AGG_C;
                    items[base + j] = agg_item{(uint32_t)(src + j * AGG_C), (uint32_t)(left < AGG_C ? left : AGG_C), (uint32_t)(base + j), (uint32_t)s};
                }
            }
            cur[l] += n;
            src = base;
            if (n == 1) {
                sets[s].final_of = (uint32_t)base;
                break;
            }
        }
        byte += (len + 7) / 8;
    }
}

// Same-message pre-aggregation of k groups (mi355_bls_combine_sets): the members are positions [offsets[0], offsets[k]) of the call's member
// sequence, renumbered from 0; the two segmented sums run over aggsets_measure / aggsets_fill's tables for the renumbered offsets (level 0
// reads the per-member products by position).
//   Scalars: a group's SHA-256 chain is serial - one digest per four members, a few microseconds each on a lane - so one lane walks the chain
//   of a group of up to COMB_CHAIN_LANE_MAX members (all groups side by side), and the HOST walks a longer group's chain while the device
//   works on the lanes' (combsets_chain_on_host; mi355_bls_combine stays the call for one huge group).
//   Products: the per-member multiplications keep window tables in context buffers (2 560 bytes per key, 3 072 per signature), so they run in
//   chunks of COMB_MUL_CHUNK members and the tables never hold more than one chunk.
//   COMB_MEMBERS_MAX: k_pkmul takes the byte stride of a row of its SoA output as a 32-bit value.
constexpr uint32_t COMB_CHAIN_LANE_MAX = 1024;
constexpr size_t COMB_MUL_CHUNK = 65536, COMB_MEMBERS_MAX = (size_t)1 << 26;
inline bool combsets_chain_on_host(size_t len) { return len > COMB_CHAIN_LANE_MAX; }
struct combsets_plan {
    bool ok;                                 // false: offsets decrease, or more than COMB_MEMBERS_MAX members, or 2^32 - 1 groups or more
    size_t lo, members;                      // positions [lo, lo + members) of the member sequence
    size_t chunks, chunk_cap;                // multiplication launches per side; members the window tables hold
    size_t host_chains;                      // groups whose chain the host walks
};
inline combsets_plan combsets_measure(const size_t* offsets, size_t k) {
    combsets_plan p{};
    if (k >= AGG_NONE) return p;
    p.lo = k ? offsets[0] : 0;
    for (size_t g = 0; g < k; g++) {
        if (offsets[g + 1] < offsets[g]) return p;
        p.host_chains += combsets_chain_on_host(offsets[g + 1] - offsets[g]);
    }
    p.members = k ? offsets[k] - p.lo : 0;
    if (p.members > COMB_MEMBERS_MAX) return p;
    p.chunks = (p.members + COMB_MUL_CHUNK - 1) / COMB_MUL_CHUNK;
    p.chunk_cap = p.members < COMB_MUL_CHUNK ? (p.members + WAVE - 1) / WAVE * WAVE : COMB_MUL_CHUNK;
    p.ok = true;
    return p;
}

// Per-group signature aggregation (mi355_bls_aggregate_signature_sets): the segmented sum of aggsets_measure / aggsets_fill over G2.  Level 0
// keeps AGG_C signatures per item (at 65 536 members in groups of 16 that is 8 192 lanes, 128 waves: a smaller count would fill more of the
// chip at level 0 but add a level to every group longer than it; not measured, so the key side's value stands).  The workspace of a call,
// in bytes: a G2 partial per item (one at least), the item table with final_of behind it, a flag word and a status byte per group, and the
// host form's two output arrays.  Nothing here depends on the context's max_sets.
struct aggsigs_sizes {
    size_t part, tab, bad, status, out192, out96;
};
inline aggsigs_sizes aggsigs_sizes_for(const aggsets_plan& p, size_t k) {
    return {(p.items ? p.items : 1) * (size_t)G2_WORDS * 4, (p.items * 4 + k) * 4, k * 4, k, k * 192, k * 96};
}

// Threshold-signature recovery of k groups (mi355_bls_recover_signature_sets): one lane per member computes its Lagrange coefficient and
// its product [l]S (k_recover_mul: waves_for(members) workgroups of WAVE lanes), the products are summed per group by the segmented sum of
// aggsets_measure / aggsets_fill over the renumbered offsets (level 0 reads the products by position, as combine_sets does), and a lane per
// group finishes (k_recover_finish).
//   A product is an internal G2 image of 384 bytes, so a call runs in CHUNKS of whole groups and the workspace holds one chunk: a chunk takes
//   groups while it stays within REC_MEMBERS_CHUNK members and REC_MEMBERS_CHUNK groups (empty groups have no members to count), and a
//   group longer than that is a chunk of its own.  REC_MEMBERS_CHUNK is a MEMORY bound (24 MiB of products), not a tuned value: 65 536
//   lanes are already 1 024 waves, one per SIMD of the chip, so a larger chunk has nothing to win.
//   Refused: offsets that decrease, and what the 32-bit tables cannot address (2^32 - 1 positions or groups, or more).  Nothing for its size.
constexpr size_t REC_MEMBERS_CHUNK = 65536;
struct rec_item {
    uint32_t pos, seg_first, seg_len, seg;   // the member at position pos of the call; its group's first position, length and number within the chunk
};
// groups [g0, end) are the chunk that starts at group g0 < k (chunk: the product takes the constant; the CPU tests walk small ones)
inline size_t recover_chunk_end(const size_t* offsets, size_t k, size_t g0, size_t chunk = REC_MEMBERS_CHUNK) {
    size_t g = g0 + 1;                       // one group at least, however long
    while (g < k && g - g0 < chunk && offsets[g + 1] - offsets[g0] <= chunk) g++;
    return g;
}
struct recover_plan {
    bool ok;
    size_t lo, members;                      // positions [lo, lo + members) of the member sequence
    size_t chunks;
    size_t max_members, max_groups;          // of the largest chunk: what the workspace is sized by
};
inline recover_plan recover_measure(const size_t* offsets, size_t k, size_t chunk = REC_MEMBERS_CHUNK) {
    recover_plan p{};
    if (k >= AGG_NONE) return p;
    for (size_t g = 0; g < k; g++)
        if (offsets[g + 1] < offsets[g]) return p;
    if (k && offsets[k] >= AGG_NONE) return p;
    p.lo = k ? offsets[0] : 0;
    p.members = k ? offsets[k] - p.lo : 0;
    for (size_t g0 = 0; g0 < k;) {
        const size_t g1 = recover_chunk_end(offsets, k, g0, chunk), m = offsets[g1] - offsets[g0];
        if (m > p.max_members) p.max_members = m;
        if (g1 - g0 > p.max_groups) p.max_groups = g1 - g0;
        p.chunks++;
        g0 = g1;
    }
    p.ok = true;
    return p;
}
// the member items of a chunk (groups [g0, g1), m = offsets[g1] - offsets[g0] entries)
inline void recover_fill(const size_t* offsets, size_t g0, size_t g1, rec_item* items) {
    size_t at = 0;
    for (size_t g = g0; g < g1; g++)
        for (size_t pos = offsets[g]; pos < offsets[g + 1]; pos++)
            items[at++] = rec_item{(uint32_t)pos, (uint32_t)offsets[g], (uint32_t)(offsets[g + 1] - offsets[g]), (uint32_t)(g - g0)};
}
// The workspace of one chunk of `members` members in `groups` groups whose segmented sum is `p`, in bytes: the products, the sum's
// partials (one at least), the tables (member items | sum items | final_of | group lengths), a flag word and a status byte per group, and
// the host form's two output arrays.
struct recover_sizes {
    size_t prod, part, tab, flags, status, out192, out96;
};
inline recover_sizes recover_sizes_for(const aggsets_plan& p, size_t members, size_t groups) {
    return {(members ? members : 1) * (size_t)G2_WORDS * 4, (p.items ? p.items : 1) * (size_t)G2_WORDS * 4, ((members + p.items) * 4 + 2 * groups) * 4,
            groups * 4, groups, groups * 192, groups * 96};
}

// Short linear combinations per group (mi355_bls_p1s_lincomb_many / mi355_bls_p2s_lincomb_many): the recovery's shape with the caller's
// scalars - one lane per term multiplies (k_lincomb_mul<F>, k_lincomb_mul_psi: waves_for(terms) workgroups of WAVE lanes), the segmented sum
// of aggsets_measure / aggsets_fill over the renumbered offsets adds the products per group (level 0 reads them by position), a lane per
// group finishes (k_lincomb_finish<F>).  The term items are recover_fill's rec_item; the call runs in chunks of whole groups by
// recover_chunk_end's rule, and the workspace holds one chunk.
//   LINCOMB_TERMS_CHUNK is the recovery's MEMORY bound: 65 536 products are 24 MiB on G2 and 12 MiB on G1, and as many lanes are one wave
//   per SIMD of the chip.  Not tuned.  `forced` is the test hook's (mi355_bls_debug_lincomb_set_chunk; 0: the constant).
//   Refused: offsets that decrease, and what the 32-bit tables cannot address (2^32 - 1 positions or groups, or more).  Nothing for its size.
constexpr size_t LINCOMB_TERMS_CHUNK = REC_MEMBERS_CHUNK;
inline size_t lincomb_chunk(size_t forced) { return forced ? forced : LINCOMB_TERMS_CHUNK; }
inline recover_plan lincomb_measure(const size_t* offsets, size_t k, size_t forced = 0) { return recover_measure(offsets, k, lincomb_chunk(forced)); }
inline size_t lincomb_chunk_end(const size_t* offsets, size_t k, size_t g0, size_t forced = 0) { return recover_chunk_end(offsets, k, g0, lincomb_chunk(forced)); }
// The workspace of one chunk of `terms` terms in `groups` groups whose segmented sum is `p`, in bytes; g2: 384-byte Jacobian points and 192-byte
// images, else 192 and 96.  The products, the sum's partials (one at least), the tables (term items | sum items | final_of | group lengths), a
// flag word and a status byte per group, and the host form's output array.
struct lincomb_sizes {
    size_t prod, part, tab, flags, status, out;
};
inline lincomb_sizes lincomb_sizes_for(const aggsets_plan& p, size_t terms, size_t groups, bool g2) {
    const size_t jac = (size_t)(g2 ? G2_WORDS : G1_WORDS) * 4;
    return {(terms ? terms : 1) * jac, (p.items ? p.items : 1) * jac, ((terms + p.items) * 4 + 2 * groups) * 4, groups * 4, groups, groups * (g2 ? 192 : 96)};
}

// Openings of k polynomials of n scalars over Fr (mi355_bls_fr_open_many; csrc/fropen.hpp): one workgroup of 256 lanes per polynomial, in
// PASSES of whole polynomials, polynomials [first, first + count) each.  What bounds a pass:
//   FROPEN_POLYS_PASS   workgroups of one launch, 65 536: a status byte each, and a grid far inside what a launch takes.  Not tuned.
//   FROPEN_SCAN_BYTES   n x 32 bytes per polynomial of the pass, 256 MiB in all (2 048 polynomials of 4 096 a pass): the evaluation form's
//                       scan workspace (the running products of the differences, then their inverses), and in either form the host call's
//                       quotients on their way out.  One polynomial always fits a pass, whatever its length - a polynomial of 2^26 scalars
//                       asks for 2 GiB, and gets them or the allocation's error.  Not tuned.
//   `forced` is the test hook's (mi355_bls_debug_fropen_set_pass; 0: the rule above; it can only shorten a pass).
// The workspace: `domain`, the n domain elements in Montgomery form (evaluation form; once per call), `scan` as above, a status byte per
// polynomial of a pass; out_ys / out_quot: the host form's device outputs of one pass.  Refused (ok == false): n == 0, and in evaluation
// form n that is no power of two or above 2^32.  Nothing for its size: n up to 2^26 with k up to 2^20 stays far inside 64 bits.
constexpr size_t FROPEN_POLYS_PASS = 65536, FROPEN_SCAN_BYTES = (size_t)256 << 20;
struct fropen_sizes {
    bool ok;
    size_t per_pass, passes;                 // polynomials per pass (the last one may hold fewer), passes of the call
    uint32_t log2n;                          // evaluation form: n = 2^log2n
    size_t domain, scan, status, out_ys, out_quot;
};
inline fropen_sizes fropen_sizes_for(size_t n, size_t k, bool eval, size_t forced = 0) {
    fropen_sizes s{};
    if (n == 0 || n > ((size_t)1 << 58)) return s;                 // n x 32 bytes is a size_t
    if (eval) {
        if ((n & (n - 1)) || n > ((size_t)1 << 32)) return s;
        while (((size_t)1 << s.log2n) < n) s.log2n++;
    }
    size_t per = FROPEN_POLYS_PASS;
    if (FROPEN_SCAN_BYTES / (n * 32) < per) per = FROPEN_SCAN_BYTES / (n * 32);
    if (per == 0) per = 1;
    if (forced && forced < per) per = forced;
    if (per > k && k) per = k;
    s.ok = true;
    s.per_pass = per;
    s.passes = (k + per - 1) / per;
    s.domain = eval ? n * 32 : 0;
    s.scan = eval ? per * n * 32 : 0;
    s.status = per;
    s.out_ys = per * 32;
    s.out_quot = per * n * 32;
    return s;
}
// pass p of the call: polynomials [first, first + count)
inline void fropen_pass(const fropen_sizes& s, size_t k, size_t p, size_t& first, size_t& count) {
    first = p * s.per_pass;
    count = k - first < s.per_pass ? k - first : s.per_pass;
}

// Transforms of k vectors of n = 2^m scalars over Fr (mi355_bls_fr_ntt_many; csrc/frntt.hpp): m radix-2 stages in PASSES over global memory,
// each pass the next <= tile stages with the elements they connect in LDS, and the call in SLICES of whole vectors, vectors
// [first, first + count) each.
//   FRNTT_TILE_LOG2     the default tile, 2^10 elements = 32 KiB of LDS: four workgroups (sixteen waves) fit a CU's 160 KiB, and other
//                       waves cover the dependent chain of a lane's Montgomery product.  2^12 elements (FRNTT_TILE_MAX_LOG2, 128 KiB: one
//                       workgroup, four waves per CU) halve the passes of a long vector instead.  tools/bench_fr_ntt.py measures both
//                       through the hook; the default is the one that was faster at 64 x 4 096 (profiles/fr_ntt_bench.json, README.md).
//   passes              ceil(m / tile) of them, the stages spread evenly (the first ones take the odd stage): m = 16 at tile 10 is 8 + 8,
//                       not 10 + 6, so that BOTH passes leave LDS room for adjacent columns (frntt_geo_for) - a pass that fills the tile
//                       with its own stages reads single 32-byte elements a stride apart.
//   FRNTT_SLICE_BYTES   n x 32 bytes per vector of a slice, 256 MiB in all: the host form's staging, and the second buffer of a transform
//                       whose last store permutes (more than one pass, no BITREV).  One vector always fits.  FRNTT_SLICE_VECS: the status
//                       words of a slice, 2^20.  Not tuned.
//   forced_tile is the test hook's log2 (mi355_bls_debug_frntt_set_tile; 0: the default; it cannot exceed FRNTT_TILE_MAX_LOG2, the LDS a
//   workgroup may ask for), forced_vecs that of mi355_bls_debug_frntt_set_pass (0: the rule above; it can only shorten a slice).
// Refused (ok == false): n == 0, n that is no power of two or above 2^32.  Nothing for its size: n = 2^32 with k = 2^20 stays inside 64 bits.
constexpr uint32_t FRNTT_TILE_LOG2 = 10, FRNTT_TILE_MAX_LOG2 = 12, FRNTT_MAX_PASSES = 32;
constexpr size_t FRNTT_SLICE_VECS = (size_t)1 << 20, FRNTT_SLICE_BYTES = (size_t)256 << 20;
struct frntt_sizes {
    bool ok;
    uint32_t log2n, tile, passes;            // n = 2^log2n; log2 of the tile; the passes of one transform
    uint8_t stages[FRNTT_MAX_PASSES];        // the stages of each pass, in the order they run: they sum to log2n
    size_t vecs, slices;                     // vectors per slice (the last one may hold fewer), slices of the call
    size_t twiddles, status, staging;        // bytes: the n / 2 table entries, a status word per vector of a slice, a slice's elements
};
inline frntt_sizes frntt_sizes_for(size_t n, size_t k, uint32_t forced_tile = 0, size_t forced_vecs = 0) {
    frntt_sizes s{};
    if (n == 0 || (n & (n - 1)) || n > ((size_t)1 << 32)) return s;
    while (((size_t)1 << s.log2n) < n) s.log2n++;
    s.tile = forced_tile ? (forced_tile < FRNTT_TILE_MAX_LOG2 ? forced_tile : FRNTT_TILE_MAX_LOG2) : FRNTT_TILE_LOG2;
    s.passes = (s.log2n + s.tile - 1) / s.tile;
    for (uint32_t p = 0; p < s.passes; p++) s.stages[p] = (uint8_t)(s.log2n / s.passes + (p < s.log2n % s.passes));
    size_t per = FRNTT_SLICE_VECS;
    if (FRNTT_SLICE_BYTES / (n * 32) < per) per = FRNTT_SLICE_BYTES / (n * 32);
    if (per == 0) per = 1;
    if (forced_vecs && forced_vecs < per) per = forced_vecs;
    if (per > k && k) per = k;
    s.ok = true;
    s.vecs = per;
    s.slices = (k + per - 1) / per;
    s.twiddles = n / 2 * 32;
    s.status = per * 4;
    s.staging = per * n * 32;
    return s;
}
// slice i of the call: vectors [first, first + count)
inline void frntt_slice(const frntt_sizes& s, size_t k, size_t i, size_t& first, size_t& count) {
    first = i * s.vecs;
    count = k - first < s.vecs ? k - first : s.vecs;
}
// The shape of a pass over `vecs` vectors that takes `tp` stages from index bit `sigma` up (frntt.hpp frntt_geo): what is left of the tile
// goes to adjacent columns first (clo <= sigma), then to adjacent blocks (chi, no more than the pass has blocks).
struct frntt_shape {
    uint32_t clo, chi, L;
};
inline frntt_shape frntt_geo_for(uint32_t log2n, uint32_t tile, uint32_t sigma, uint32_t tp, size_t vecs) {
    frntt_shape g{};
    const uint32_t room = tile - tp;
    g.clo = room < sigma ? room : sigma;
    const uint64_t blocks = (uint64_t)vecs << (log2n - sigma - tp);
    uint32_t need = 0;
    while (need < 63 && ((uint64_t)1 << need) < blocks) need++;
    g.chi = room - g.clo < need ? room - g.clo : need;
    g.L = g.clo + tp + g.chi;
    return g;
}

// Per-group aggregateVerify (mi355_bls_aggregate_verify_each): k groups of (key, message) pairs in CSR form, one aggregate signature each.
// The call runs in SLICES of at most `cap` pairs of the per-set path's pair store (2 cap slots: the pairs, then one (-G1, sig) pair per
// group that ends in the slice - never more than the pairs, a group in a slice has a pair there).
//   Cutting (aggveach_cut): a slice takes whole groups while they fit; a group that does not fit the room left starts the next slice; a group
//   longer than a slice is walked in parts of `cap` pairs, each part a slice of its own, and its last part is followed by whole groups
//   again.  So at most one group is open at a slice boundary (open_out: the last group of the slice goes on; open_in: the first one came
//   from the slice before), and its Miller value so far waits in one Fp12 of device memory.  Empty groups occupy nothing: no pair, no
//   signature slot, no item; their verdict is 0.
//   Per Miller step the lines of a group's pairs, and the line of its signature pair in the part that ends it, are multiplied in levels of
//   one-lane items, like aggsets_fill's sums: a level-0 item takes up to C consecutive pairs of ONE group (and, the first item of a group
//   that ends here, its signature line), an item above up to C partials.  The item that leaves a group with one value is FINAL: it
//   writes the group's step value (dst = the group's number in the slice) instead of a partial, so a group of up to C pairs is one item
//   and has no partial at all.  Partials are numbered per slice, (group, level) after (group, level).
//   AGGV_C = 8: a partial is an Fp12 per Miller step, 68 x 768 bytes = 51 KiB, and only items that are not final write one - at most
//   P / (C - 1) of them for P pairs, so at C = 8 the partial store stays below a seventh of the slice's line store (68 x 384 bytes per
//   pair); C = 4 would take a third of it, C = 16 leaves a lane sixteen dependent products at level 0.  NOT MEASURED.
//   The tail takes each_for's rule with the slice's groups as m: the Fp12 engine up to each_engine_max(slots) groups in latency mode,
//   one lane per group beyond and in throughput mode (inherited from verify_each, not measured for this path).
constexpr uint32_t AGGV_C = 8;
constexpr uint32_t AGGV_MAX_LEVELS = 32;                 // C >= 2 and fewer than 2^30 pairs per slice
constexpr uint32_t AGGV_FINAL = 0x80000000u, AGGV_SIG = 0x40000000u, AGGV_COUNT = 0x3fffffffu;      // an item's count word
constexpr uint32_t AGGV_OPEN_IN = 1, AGGV_OPEN_OUT = 2;  // a group's flags word
struct aggv_slice {
    size_t g0, g1;                     // the slice's pairs belong to groups of [g0, g1) (empty ones among them have none)
    size_t pos0, pos1;                 // positions [pos0, pos1) of the call's pair sequence
    uint32_t ng;                       // groups with pairs in the slice
    bool open_in, open_out;
    size_t pairs() const { return pos1 - pos0; }
    uint32_t sigs() const { return ng - (open_out ? 1 : 0); }
    size_t next_g() const { return open_out ? g1 - 1 : g1; }
};
// the slice that starts at position pos, which belongs to group g or a later one (g == k or pairs() == 0: nothing is left)
inline aggv_slice aggveach_cut(const size_t* offsets, size_t k, size_t g, size_t pos, size_t cap) {
    aggv_slice s{};
    while (g < k && offsets[g + 1] <= pos) g++;             // finished and empty groups
    s.g0 = s.g1 = g, s.pos0 = s.pos1 = pos;
    if (g == k) return s;
    s.open_in = pos > offsets[g];
    for (; g < k; g++) {
        const size_t left = offsets[g + 1] - s.pos1, room = cap - (s.pos1 - s.pos0);
        if (left == 0) continue;
        if (left > room) {
            if (s.pos1 == s.pos0) s.pos1 += room, s.ng++, s.g1 = g + 1, s.open_out = true;      // a part of a group longer than a slice, alone
            break;
        }
        s.pos1 += left, s.ng++, s.g1 = g + 1;
    }
    return s;
}
struct aggv_group {
    uint32_t g, first, count, flags;   // the group's number in the call; its pairs first .. + count of the slice; AGGV_OPEN_*
};
// the slice's groups (s.ng entries)
inline void aggveach_groups(const size_t* offsets, const aggv_slice& s, aggv_group* out) {
    uint32_t at = 0;
    for (size_t g = s.g0; g < s.g1; g++) {
        const size_t a = offsets[g] > s.pos0 ? offsets[g] : s.pos0, b = offsets[g + 1] < s.pos1 ? offsets[g + 1] : s.pos1;
        if (b <= a) continue;
        out[at++] = aggv_group{(uint32_t)g, (uint32_t)(a - s.pos0), (uint32_t)(b - a),
                               (a > offsets[g] ? AGGV_OPEN_IN : 0u) | (b < offsets[g + 1] ? AGGV_OPEN_OUT : 0u)};
    }
}
struct aggveach_tab {
    uint32_t levels;
    size_t level_first[AGGV_MAX_LEVELS + 1];      // items [level_first[l], level_first[l + 1]) are level l
    size_t items, partials;
};
inline aggveach_tab aggveach_measure(const aggv_group* gr, uint32_t ng, uint32_t C = AGGV_C) {
    aggveach_tab t{};
    size_t per_level[AGGV_MAX_LEVELS] = {};
    for (uint32_t i = 0; i < ng; i++) {
        size_t n = gr[i].count;
        for (uint32_t l = 0;; l++) {
            n = (n + C - 1) / C;
            per_level[l] += n;
            if (l + 1 > t.levels) t.levels = l + 1;
            if (n == 1) break;
            t.partials += n;
        }
    }
    for (uint32_t l = 0; l < t.levels; l++) t.level_first[l + 1] = t.level_first[l] + per_level[l];
    t.items = t.level_first[t.levels];
    return t;
}
// the item table (t.items entries): src_first = a pair of the slice (level 0) or a partial (above), count = the operands | AGGV_FINAL |
// AGGV_SIG, dst = a partial, or the group's number in the slice for a FINAL item, seg = that number.  with_sig = false: the groups have
// no signature pair (the pairing-product calls below), so no item carries AGGV_SIG; everything else is the same table.
inline void aggveach_fill(const aggveach_tab& t, const aggv_group* gr, uint32_t ng, agg_item* items, uint32_t C = AGGV_C, bool with_sig = true) {
    size_t cur[AGGV_MAX_LEVELS], pcur = 0;
    for (uint32_t l = 0; l < AGGV_MAX_LEVELS; l++) cur[l] = l < t.levels ? t.level_first[l] : 0;
    for (uint32_t i = 0; i < ng; i++) {
        size_t n = gr[i].count, src = gr[i].first;
        for (uint32_t l = 0;; l++) {
            const size_t m = (n + C - 1) / C, base = cur[l];
            for (size_t j = 0; j < m; j++) {
                const size_t left = n - j * C;
                const uint32_t sig = with_sig && l == 0 && j == 0 && !(gr[i].flags & AGGV_OPEN_OUT) ? AGGV_SIG : 0u;
                items[base + j] = agg_item{(uint32_t)(src + j * C), (uint32_t)(left < C ? left : C) | sig | (m == 1 ? AGGV_FINAL : 0u),
                                           (uint32_t)(m == 1 ? i : pcur + j), i};
            }
            cur[l] += m;
            if (m == 1) break;
            src = pcur, pcur += m, n = m;
        }
    }
}
// One slice of `pairs` pairs and `sigs` signature pairs in `ng` groups: the record / pair-slot kernel (a lane per pair slot), the Miller
// lines of all pairs + sigs pairs in the form the per-set path takes for as many, and the tail by each_for's rule on ng.  A level of
// `count` items runs as (waves_for(count), N_LINES) waves: a lane per (item, step), the items of a step side by side in a wave.
struct aggveach_plan {
    uint32_t setup_grid;
    lines_plan lines;
    bool tail_engine;                  // k_aggveach_engine_rows: tail_grid workgroups, each walks groups i, i + tail_grid, ... | k_aggveach_tail: tail_grid waves
    uint32_t tail_grid;
};
inline aggveach_plan aggveach_for(uint32_t slots, bool coop, uint32_t pairs, uint32_t sigs, uint32_t ng) {
    aggveach_plan p{};
    p.setup_grid = waves_for(pairs + sigs);
    p.lines = lines_for(slots, coop, pairs + sigs, 0);
    p.tail_engine = coop && ng <= each_engine_max(slots);
    p.tail_grid = p.tail_engine ? (ng < each_engine_grid_max(slots) ? ng : each_engine_grid_max(slots)) : waves_for(ng);
    return p;
}
// the stores of one slice, in words: a partial and a group's step values are N_LINES internal Fp12 images (partial p of step s at
// (s x partials + p) x F12_WORDS; group i's step s at (i x N_LINES + s) x F12_WORDS, the 68 values the tail walks side by side)
inline size_t aggveach_part_words(size_t partials) { return (partials ? partials : 1) * (size_t)N_LINES * F12_WORDS; }
inline size_t aggveach_step_words(size_t ng) { return (ng ? ng : 1) * (size_t)N_LINES * F12_WORDS; }

// Pairing-product checks over caller-supplied pairs (mi355_bls_pairing_check_each, mi355_bls_pairing_products, mi355_bls_batch_pairing_check):
// k groups of (P, Q) pairs in CSR form.  A group is a group of the per-group path above WITHOUT a signature pair: the slices are
// aggveach_cut's over `cap` pairs (a slice's pairs are all the pair slots it uses), the tables aggveach_groups / aggveach_measure /
// aggveach_fill(with_sig = false), the carry of a group longer than a slice the same one.
//   The blinded form multiplies every pair's P by its group's scalar and forms ONE product over all pairs: the call's pairs are one group of
//   the per-group path (pairprod_blind_cut: parts of `cap` pairs, carried from part to part), and the setup lane of a pair needs the REAL
//   group it belongs to for its scalar (pairprod_real_groups: the call's groups cut at the part's ends, as aggveach_groups gives them).
//   The blinded form's tail is always the Fp12 engine: a slice has one Horner chain and one final exponentiation, which one lane of
//   k_aggveach_tail would walk alone while the chip waits (the engine's workgroup does not depend on the context's mode).  NOT MEASURED.
constexpr uint32_t PAIRPROD_VALIDATE = 1;                // the calls' flag bit (MI355_BLS_PAIR_VALIDATE)
struct pairprod_plan {
    uint32_t setup_grid;               // a lane per pair slot
    lines_plan lines;
    bool pkmul_spread;                 // the blinded form's [r]P: k_pkmul_spread | k_pkmul
    bool tail_engine;
    uint32_t tail_grid;
};
inline pairprod_plan pairprod_for(uint32_t slots, bool coop, uint32_t pairs, uint32_t ng, bool blinded) {
    pairprod_plan p{};
    const aggveach_plan a = aggveach_for(slots, coop, pairs, 0, ng);
    p.setup_grid = a.setup_grid, p.lines = a.lines;
    p.pkmul_spread = pkmul_spread_for(slots, coop, pairs);
    p.tail_engine = blinded ? true : a.tail_engine;
    p.tail_grid = blinded ? 1 : a.tail_grid;
    return p;
}
// the slice of the blinded form that starts at position pos of n pairs: one group, cut in parts of cap pairs
inline aggv_slice pairprod_blind_cut(size_t n, size_t pos, size_t cap) {
    const size_t one[2] = {0, n};
    return aggveach_cut(one, 1, 0, pos, cap);
}
// the call's groups that have pairs in positions [pos0, pos1), pos0 < pos1 <= offsets[k], as a slice aggveach_groups takes
inline aggv_slice pairprod_real_groups(const size_t* offsets, size_t k, size_t pos0, size_t pos1) {
    aggv_slice s{};
    size_t g = 0;
    while (g < k && offsets[g + 1] <= pos0) g++;
    s.g0 = g, s.pos0 = pos0, s.pos1 = pos1;
    s.open_in = g < k && pos0 > offsets[g];
    for (; g < k && offsets[g] < pos1; g++)
        if (offsets[g + 1] > offsets[g]) s.ng++, s.g1 = g + 1, s.open_out = offsets[g + 1] > pos1;
    if (s.ng == 0) s.g1 = s.g0;
    return s;
}
// the call's buffers in bytes: a status byte per pair, a bad word per group (one for the blinded form), the k scalars of the blinded form
struct pairprod_sizes {
    size_t status, flags, scalars;
};
inline pairprod_sizes pairprod_sizes_for(size_t n, size_t k, bool blinded) { return {n ? n : 1, (blinded ? 1 : k) * 4, blinded ? k * 8 : 0}; }
// a slice's table in 16-byte entries: groups | items | (the blinded form) the real groups
inline size_t pairprod_tab_entries(uint32_t ng, size_t items, uint32_t real_groups) { return (size_t)ng + items + real_groups; }

// Per-batch verdicts for many batches (mi355_bls_batch_verify_many_each): k batches of counts[b] sets, laid end to end.  Batch b is one
// GROUP of the per-group path above: its pairs are ([r_i]PK_i, H(m_i)) for its sets, its signature pair (-G1, sum [r_i]S_i), so the group
// tables, the item levels and the tail are aggveach_groups / aggveach_measure / aggveach_fill / aggveach_for as they stand; the per-batch
// signature sums are a segmented G2 sum over aggsets_measure / aggsets_fill's tables (manyeach_sum_offsets).
//   Cutting (manyeach_cut): a slice is a run of WHOLE consecutive batches.  It holds at most cap_sets sets (the hashing workspace, the
//   scalars and k_pkmul's tables are sized by the context's max_sets) and its sets plus one signature slot per non-empty batch fit
//   cap_pairs, the slots of the per-set path's pair store.  No batch is ever cut, so no group is open at a slice boundary.  A batch that
//   does not fit an empty slice (more than cap_sets sets, or sets + 1 > cap_pairs) is a slice by itself and is marked `single`: the host
//   layer gives it to the single-batch path, which slices internally.  Empty batches ride in the slice that meets them: no pair, no slot,
//   no lane; their verdict is 0.
struct manyeach_slice {
    size_t b0, b1;                     // batches [b0, b1) of the call
    size_t set0, sets;                 // their sets: [set0, set0 + sets) of the call's record sequence
    uint32_t nb;                       // non-empty batches among them = signature slots = groups
    bool single;                       // one batch that fits no slice: the single-batch path, alone (nb == 1)
    size_t pairs() const { return sets + nb; }
};
inline bool manyeach_fits_alone(size_t n, size_t cap_sets, size_t cap_pairs) { return n <= cap_sets && n + 1 <= cap_pairs; }
// the slice that starts at batch b, whose first set is set0 of the call (b == k: b1 == b0, nothing is left)
inline manyeach_slice manyeach_cut(const size_t* counts, size_t k, size_t b, size_t set0, size_t cap_sets, size_t cap_pairs) {
    manyeach_slice s{};
    s.b0 = s.b1 = b, s.set0 = set0;
    for (; b < k; b++) {
        const size_t n = counts[b];
        if (n == 0) {
            s.b1 = b + 1;
            continue;
        }
        if (!manyeach_fits_alone(n, cap_sets, cap_pairs)) {
            if (s.nb == 0) s.sets = n, s.nb = 1, s.b1 = b + 1, s.single = true;      // alone; behind whole batches it starts the next slice
            break;
        }
        if (s.sets + n > cap_sets || s.sets + n + s.nb + 1 > cap_pairs) break;
        s.sets += n, s.nb++, s.b1 = b + 1;
    }
    return s;
}
// the slice as the per-group path takes it: offsets = the k + 1 prefix sums of counts; no group is open at either end
inline aggv_slice manyeach_as_groups(const manyeach_slice& s) { return aggv_slice{s.b0, s.b1, s.set0, s.set0 + s.sets, s.nb, false, false}; }
// the signature sums' segments: group l of the slice = products [rel[l], rel[l + 1]) (rel: nb + 1 entries), from the slice's group table
inline void manyeach_sum_offsets(const aggv_group* gr, uint32_t nb, size_t* rel) {
    for (uint32_t l = 0; l < nb; l++) rel[l] = gr[l].first;
    rel[nb] = nb ? (size_t)gr[nb - 1].first + gr[nb - 1].count : 0;
}

// ------------------------------------------------------------------------------------------
// Pippenger MSM (blst_p1s_mult_pippenger / blst_p2s_mult_pippenger): what msm_enqueue follows, and what msm_reserve allocates.
// ------------------------------------------------------------------------------------------
// The windows of a call, as the kernels take them (a kernel argument: the layout is fixed).
struct pip_win {
    uint32_t nwin, wbase, wrem, nbits;      // nwin windows over nbits + 1 bits (widths differ by at most one bit)
    uint32_t cbk;                           // bucket index bits: 2^cbk buckets per window, cbk = widest window - 1
    uint32_t H[9];                          // the bias: 2^(len - 1) at every window but the top one
};
static_assert(sizeof(pip_win) == 14 * 4, "five words and the nine of the bias, no padding");
// buckets per running-sum segment of k_pip_segred.  Rounds 3-4 used 8 from 2^12 buckets per window on (shorter running sums while the
// segments still fill the chip); since the bucket kernel became the assembly loop (round 5) the reductions are what the MSM waits for and
// 16-bucket segments - half as many segment lanes competing with the other window group's bucket kernel - are ahead again at 2^20 points:
// 4.63 - 4.68 ms against 4.75 - 4.81, two in flight 3.77 - 3.80 against 3.88 - 4.03 (profiles/r05_ab/msm_knobs.txt).
constexpr uint32_t MSM_SEG = 16;
constexpr uint32_t MSM_ORD_PER = 16;         // buckets a lane of k_msm_order_hist / k_msm_order_scatter bins
// the counting sort with a window's counters in LDS: 1024-thread workgroups, one per (slice of the points, window); 2^15 counters are 128 KB
constexpr uint32_t PIP_SORT_THREADS = 1024, PIP_SORT_MAX_CBK = 15, PIP_SLICES = 32;
constexpr uint32_t PIP_SORT_MIN_CBK = 10, PIP_SORT_MIN_POINTS = 1u << 15;      // large inputs only; k_pip_scan_block gives a thread 2^cbk / 1024 buckets
static_assert((1u << PIP_SORT_MIN_CBK) % PIP_SORT_THREADS == 0, "k_pip_scan_block: whole buckets per thread");
constexpr uint32_t MSM_TEAM_LANES_MAX = 61440;     // lanes of a team reduction: 960 waves (see msm_for)
constexpr uint32_t MSM_TAIL_WAVES_MAX = 16;        // k_pip_rowtail: one workgroup of at most 1024 lanes
constexpr uint32_t MSM_SPLIT_MIN_WINDOWS = 4;
constexpr size_t MSM_SPLIT_MIN_WORK = (size_t)1 << 22;      // points x windows
// what the fixed-size buffers of the workspace are made for (msm_sizes_for); msm_extents says what a plan touches of them
constexpr uint32_t MSM_WINDOWS_MAX = 64;     // 52 windows at most (nbits 256 at 5-bit windows); also the window sums k_pip_rowtail keeps in LDS
constexpr uint32_t MSM_NSPLIT_MAX = 16, MSM_GROUPS_MAX = 2, MSM_CHIST_ROOM = 4;
constexpr size_t MSM_CHIST_BYTES = MSM_CHIST_ROOM * 256 * 4;       // k_msm_order_*: 256 bins of bucket loads per window group
static_assert(MSM_GROUPS_MAX <= MSM_CHIST_ROOM && MSM_TAIL_WAVES_MAX * WAVE <= 1024, "");

// Window plan for npoints x nbits: about log2(n) - 3 bits per window (signed digits: 2^(c-1) buckets), widths balanced.
inline pip_win pip_for(size_t npoints, size_t nbits) {
    uint32_t lg = 0;
    while ((1ull << (lg + 1)) <= npoints) lg++;
    int c = (int)lg - 3;
    if (c < 5) c = 5;                                   // at least one 16-bucket segment per window
    if (c > 16) c = 16;                                 // at most 2^15 buckets per window: the counters of the LDS counting sort
    pip_win W{};
    W.nbits = (uint32_t)nbits;
    uint32_t ext = (uint32_t)nbits + 1;                  // one extra (zero) top bit: the top window absorbs the carry of the bias
    W.nwin = (ext + c - 1) / c;
    W.wbase = ext / W.nwin;
    W.wrem = ext % W.nwin;
    uint32_t widest = W.wbase + (W.wrem ? 1 : 0);
    W.cbk = widest - 1;
    if (W.cbk < 4) W.cbk = 4;
    for (uint32_t w = 0; w + 1 < W.nwin; w++) {
        uint32_t off = w < W.wrem ? w * (W.wbase + 1) : W.wrem * (W.wbase + 1) + (w - W.wrem) * W.wbase;
        uint32_t len = w < W.wrem ? W.wbase + 1 : W.wbase;
        uint32_t bit = off + len - 1;                    // + 2^(len - 1) at window w
        W.H[bit >> 5] |= 1u << (bit & 31);
    }
    return W;
}

// One group of windows [w0, w1) = the pipeline behind the counting sort on a range of windows: buckets by load -> bucket sums -> segment sums
// -> window parts -> (G1) the row tail's Horner walk over the group, (G2) window sums.  Buckets [g0, g0 + gc), segments [t0, t0 + tc).
struct msm_group {
    uint32_t w0, w1, g0, gc, t0, tc;
    uint32_t order_grid;               // k_msm_order_hist / k_msm_order_scatter: MSM_ORD_PER buckets per lane
    uint32_t bucket_grid;              // k_pip_bucket: one lane per bucket
    uint32_t team, segred_grid;        // k_pip_segred_team<team> (4, 2) | k_pip_segred (1): `team` lanes per segment
    uint32_t tail_waves, tail_lanes;   // k_pip_rowtail's one workgroup (G1): a wave per window up to MSM_TAIL_WAVES_MAX
};
struct msm_plan {
    pip_win W;
    uint32_t n, total, segs_per_win, nseg;     // points; buckets and 16-bucket segments of all windows
    uint32_t nsplit;                   // k_pip_winpart: partial sums per window
    bool lds_sort;                     // k_pip_hist_lds / k_pip_slice_scan / k_pip_scan_block / k_pip_scatter_lds | k_pip_hist / k_msm_scan / k_pip_scatter
    uint32_t per;                      //   points per slice (lds_sort)
    uint32_t point_grid;               // k_pip_convert, and the x of k_pip_hist / k_pip_scatter: one lane per point
    uint32_t slice_scan_grid;          // k_pip_slice_scan: one lane per bucket of all windows
    uint32_t ngroups, cut[MSM_GROUPS_MAX + 1];      // group g = windows [cut[g + 1], cut[g]), from the high windows down
    msm_group group[MSM_GROUPS_MAX];
};
// allow_split: the caller lets the window groups use the context's fork stream; have_side: that stream exists
inline msm_plan msm_for(size_t npoints, size_t nbits, bool g2, bool allow_split, bool have_side) {
    msm_plan p{};
    p.W = pip_for(npoints, nbits);
    const pip_win& W = p.W;
    const uint32_t n = p.n = (uint32_t)npoints, nw = W.nwin;
    p.total = nw << W.cbk;
    p.segs_per_win = (1u << W.cbk) / MSM_SEG;
    p.nseg = nw * p.segs_per_win;
    p.nsplit = p.segs_per_win >= 1024 ? 16 : (p.segs_per_win >= 128 ? 4 : 1);
    p.lds_sort = W.cbk <= PIP_SORT_MAX_CBK && W.cbk >= PIP_SORT_MIN_CBK && n >= PIP_SORT_MIN_POINTS;      // counters of a window in LDS (large inputs)
    p.per = (n + PIP_SLICES - 1) / PIP_SLICES;
    p.point_grid = waves_for(n);
    p.slice_scan_grid = waves_for(p.total);
    // The counting sort covers all windows; then two groups of windows, each on its own stream: the HIGH windows first (their
    // results need the long doubling chains: up to nbits - c dependent doublings on one wave per window, ~1 ms of pure
    // latency), the LOW windows' bucket kernel behind the high one, so that the high group's serial tail runs beside the bucket
    // accumulation of the low group and only the short chains of the low windows are left at the end.  More groups lose more
    // in the bucket kernels' tails than they hide.  Large inputs only: a small MSM is latency-bound in every stage.
    const bool split = allow_split && nw >= MSM_SPLIT_MIN_WINDOWS && (size_t)n * nw >= MSM_SPLIT_MIN_WORK && have_side;
    // Groups [cut[g + 1], cut[g]) from the high windows down: two halves.  Measured at 2^20 x 255 bits, 16 windows
    // (profiles/r04_ab/msm_cuts.txt): cuts 5 .. 10 are within the noise of 8; three groups (10,4 / 11,5 / 12,6 / 9,3), whose last
    // group's exposed reduction is shorter, are 1 - 3 % SLOWER alone and 10 % slower with two MSMs in flight - every extra group's
    // bucket kernel has its own tail and shares the chip with one more reduction.
    p.ngroups = split ? 2 : 1;
    p.cut[0] = nw, p.cut[1] = split ? nw / 2 : 0, p.cut[2] = 0;
    for (uint32_t g = 0; g < p.ngroups; g++) {
        msm_group& G = p.group[g];
        G.w0 = p.cut[g + 1], G.w1 = p.cut[g];
        G.g0 = G.w0 << W.cbk, G.gc = (G.w1 - G.w0) << W.cbk;
        G.t0 = G.w0 * p.segs_per_win, G.tc = (G.w1 - G.w0) * p.segs_per_win;
        G.order_grid = (G.gc + WAVE * MSM_ORD_PER - 1) / (WAVE * MSM_ORD_PER);
        G.bucket_grid = waves_for(G.gc);
        // G1: 4 or 2 lanes per segment (lane teams) while the team waves stay well inside the chip's 1024 one-per-SIMD wave slots (<= 960 waves: a
        // kernel of exactly 1024 such waves finds a few SIMDs taken by the other group's reduction and runs a second round for the stragglers).
        // profiles/r04_ab/msm_team.txt: 2^14 points 2.70 -> 2.29 ms, 2^16 2.56 -> 2.28, 2^18 3.28 -> 3.10 (two lanes); 2^20 would need 1024 waves per
        // group and measured 5.2 - 5.4 ms against 5.1 - 5.2: one lane per segment there.
        G.team = g2 ? 1 : ((size_t)G.tc * 4 <= MSM_TEAM_LANES_MAX ? 4 : ((size_t)G.tc * 2 <= MSM_TEAM_LANES_MAX ? 2 : 1));
        G.segred_grid = waves_for(G.tc * G.team);
        G.tail_waves = G.w1 - G.w0 < MSM_TAIL_WAVES_MAX ? G.w1 - G.w0 : MSM_TAIL_WAVES_MAX;
        G.tail_lanes = G.tail_waves * WAVE;
    }
    return p;
}

// The workspace's buffers in bytes.  msm_sizes_for: what msm_reserve allocates for its two capacities, the bytes of the staged points and the
// buckets of all windows (hist.bytes / 4); it grows all of them or none.  msm_extents: what the kernels touch under a plan, read off their
// indexing - a plan fits a workspace when no extent exceeds its size (tests/test_msm_plan.py holds every plan to that).
struct msm_sizes {
    size_t d_pts, d_sc;                // the host entries' staging: affine images, 32-byte scalars
    size_t pts_int;                    // k_pip_convert: point i at word i x 2 coordinates x FP_WORDS (G2: x 2)
    size_t hist;                       // one word per bucket: hist, offs, cursor, order alike
    size_t chist;                      // group g's 256 bins at word 256 g
    size_t shist;                      // k_pip_hist_lds: ((window x PIP_SLICES + slice) << cbk) + bucket
    size_t part;                       // k_pip_winpart: a Jacobian point at (window x nsplit + part)
    size_t sorted;                     // window w's point indices from word w x n
    size_t buckets, segout;            // SoA Jacobian points: three (G2: six) coordinates of 64 bytes, rows of `total` / `nseg` points
    size_t winout;                     // G2: a Jacobian point per window (k_pip_winsum); G1: group g's 48-word accumulator at word 48 g (k_pip_rowtail)
    size_t out;                        // the blst_p1 / blst_p2 image
};
inline msm_sizes msm_sizes_for(size_t point_bytes, size_t buckets) {
    const size_t cn = point_bytes / 96;                  // point capacity counted in G1 points (a G2 point takes two)
    msm_sizes s{};
    s.d_pts = point_bytes;
    s.d_sc = cn * 32;
    s.pts_int = cn * 2 * FP_WORDS * 4;
    s.hist = buckets * 4;
    s.chist = MSM_CHIST_BYTES;
    s.shist = buckets * PIP_SLICES * 4;                  // per-slice counters of the LDS counting sort
    s.part = (size_t)MSM_WINDOWS_MAX * MSM_NSPLIT_MAX * G2_WORDS * 4;
    s.sorted = cn * MSM_WINDOWS_MAX * 4;
    s.buckets = buckets * 6 * 64;
    s.segout = (buckets / 4 + 64) * 6 * 64;
    s.winout = (size_t)MSM_WINDOWS_MAX * G2_WORDS * 4;
    s.out = 288;
    return s;
}
inline msm_sizes msm_extents(const msm_plan& p, bool g2) {
    const size_t n = p.n, coord = g2 ? 2 * FP_WORDS : FP_WORDS, jac = 3 * coord * 4;      // words of a coordinate; bytes of a Jacobian point
    msm_sizes s{};
    s.d_pts = n * (g2 ? 192 : 96);
    s.d_sc = n * 32;
    s.pts_int = n * 2 * coord * 4;
    s.hist = (size_t)p.total * 4;
    s.chist = (size_t)p.ngroups * 256 * 4;
    s.shist = p.lds_sort ? ((size_t)p.W.nwin * PIP_SLICES << p.W.cbk) * 4 : 0;
    s.part = (size_t)p.W.nwin * p.nsplit * jac;
    s.sorted = (size_t)p.W.nwin * n * 4;
    s.buckets = (size_t)p.total * jac;
    s.segout = (size_t)p.nseg * jac;
    s.winout = g2 ? (size_t)p.W.nwin * jac : (size_t)p.ngroups * 48 * 4;
    s.out = g2 ? 288 : 144;
    return s;
}

// ------------------------------------------------------------------------------------------
// k G1 MSMs in one device pass (mi355_bls_p1s_mult_pippenger_many; the G2 form mi355_bls_p2s_mult_pippenger_many: see MSM_MANY_G2_* below):
// what msm_many_run follows, and what it reserves.
// Every stage of the bucket method works on VIRTUAL windows v = j x nwin + w (MSM j of the pass, its window w): the counting sort gives each
// virtual window its buckets' point lists, and from there k_msm_order_*, k_pip_bucket, k_pip_segred(_team) and k_pip_winpart see one MSM of
// k x nwin windows; k_pip_rowtail_many then walks each MSM's own nwin window parts, one workgroup per MSM.
//   window width   ONE pip_win per call, whichever way the call is cut into passes: pip_for of the shared npoints, or - ragged - of the MEAN
//                  member length (npoints / k rounded up, at least 1).  The mean, not the largest: every member pays the reduction of all of its
//                  windows' buckets, full or empty.  Not measured against the other choices.
//   one pass       at most MSM_MANY_VWIN_MAX virtual windows (no grid axis of any kernel, whichever it puts them on, exceeds 65 535),
//                  MSM_MANY_BUCKETS_MAX buckets (the SoA bucket store: 192 bytes each) and MSM_MANY_PAIRS_MAX (point, scalar) pairs (a pass of
//                  that many pairs already runs at the large single MSM's throughput; list positions stay 32-bit words).  A call beyond that
//                  runs as consecutive passes over ranges of MSMs; a member that alone exceeds the pair bound is handed to msm_enqueue, and so
//                  is a call of one MSM.
//   counting sort  the global-counter form only (k_pipm_hist / k_pipm_scan / k_pipm_scatter).  The LDS-counter sort of large single MSMs is
//                  left out: its workgroups own (slice of the points, window), and a slice here would straddle members.
//   team, nsplit   msm_for's rules on the pass's segments / a window's segments.  Not measured for this call.
// The pass runs on the caller's stream alone (no window groups).
// ------------------------------------------------------------------------------------------
constexpr uint32_t MSM_MANY_VWIN_MAX = 65535;
constexpr uint32_t MSM_MANY_BUCKETS_MAX = 1u << 21;
constexpr uint32_t MSM_MANY_PAIRS_MAX = 1u << 20;
static_assert((uint64_t)MSM_MANY_PAIRS_MAX * MSM_WINDOWS_MAX < (1ull << 31), "a list position (pairs x windows) and a point index beside its sign bit fit a word");
static_assert((uint64_t)MSM_MANY_BUCKETS_MAX * 16 < (1ull << 32), "k_pip_bucket's 16-byte bucket offsets");
// The G2 form (mi355_bls_p2s_mult_pippenger_many): the same plan over 384-byte SoA points.  A pass takes HALF the buckets, so its bucket store
// is no larger than a G1 pass's; the reduction is k_pip_segred<fp2> alone (team = 1: the lane teams are G1 code); the per-MSM tail is
// k_pip_tail_many_g2, whose workgroup keeps an MSM's window sums in LDS (MSM_WINDOWS_MAX Jacobian points of G2_WORDS words: 24 KB) and is
// MSM_MANY_G2_TAIL_WAVES waves wide - one wave per SIMD of a CU, so that the walking wave has the whole register file; that wave count is a
// first choice, NOT MEASURED against others.  Its price: at ~340 registers a wave the workgroup needs all four SIMDs of a CU, three of which
// idle through wave 0's walk, so a CU runs ONE walk at a time; the waves beside wave 0 only copy window sums (nsplit == 1) or do nothing
// (nsplit > 1: Fp2 products may run in one wave of a workgroup at a time, fp.hpp bls_xchg).  A one-wave tail is the variant to measure next.  The window width stays pip_for's rule, made for G1 and NOT MEASURED for G2 (a G2 bucket
// addition costs about three G1 ones, which argues for narrower windows on small members; nobody has tried).
constexpr uint32_t MSM_MANY_G2_BUCKETS_MAX = MSM_MANY_BUCKETS_MAX / 2;
constexpr uint32_t MSM_MANY_G2_TAIL_WAVES = 4;
static_assert((uint64_t)MSM_MANY_G2_BUCKETS_MAX * G2_WORDS == (uint64_t)MSM_MANY_BUCKETS_MAX * G1_WORDS, "a G2 pass's bucket store is a G1 pass's");
static_assert((((256 + 1 + 15) / 16) << 15) <= MSM_MANY_G2_BUCKETS_MAX, "one MSM always fits a G2 pass: pip_for's widest plan is 17 windows of 2^15 buckets");
static_assert((size_t)MSM_WINDOWS_MAX * G2_WORDS * 4 <= 32 * 1024, "k_pip_tail_many_g2's window sums in LDS");
struct msm_many_plan {
    pip_win W;
    bool shared;                       // every MSM over all npoints points | MSM j over [offsets[j], offsets[j + 1])
    uint32_t n_ref;                    // what the window width was taken from
    uint32_t buckets_per_msm;          // nwin << cbk
    uint32_t segs_per_win, nsplit;     // as msm_plan's
    uint32_t tail_waves, tail_lanes;   // k_pip_rowtail_many's workgroup (one per MSM): a wave per window up to MSM_TAIL_WAVES_MAX
    uint32_t msms_max;                 // MSMs a pass takes at the most (virtual windows, buckets)
    bool g2;                           // the G2 form: what msm_many_next / msm_many_extents / msm_many_sizes_for read the field from
};
inline msm_many_plan msm_many_for(size_t k, size_t npoints, bool shared, size_t nbits, bool g2 = false) {
    msm_many_plan P{};
    P.shared = shared;
    P.g2 = g2;
    const size_t mean = shared || k == 0 ? npoints : (npoints + k - 1) / k;
    P.n_ref = (uint32_t)(mean < 1 ? 1 : (mean > MSM_MANY_PAIRS_MAX ? MSM_MANY_PAIRS_MAX : mean));
    P.W = pip_for(P.n_ref, nbits);
    P.buckets_per_msm = P.W.nwin << P.W.cbk;
    P.segs_per_win = (1u << P.W.cbk) / MSM_SEG;
    P.nsplit = P.segs_per_win >= 1024 ? 16 : (P.segs_per_win >= 128 ? 4 : 1);
    const uint32_t waves_max = g2 ? MSM_MANY_G2_TAIL_WAVES : MSM_TAIL_WAVES_MAX;
    P.tail_waves = P.W.nwin < waves_max ? P.W.nwin : waves_max;
    P.tail_lanes = P.tail_waves * WAVE;
    const uint32_t by_vwin = MSM_MANY_VWIN_MAX / P.W.nwin, by_buckets = (g2 ? MSM_MANY_G2_BUCKETS_MAX : MSM_MANY_BUCKETS_MAX) / P.buckets_per_msm;
    P.msms_max = by_vwin < by_buckets ? by_vwin : by_buckets;      // >= 1: 64 windows of 2^15 buckets are 2^21 (G2: pip_for's widest, 17 windows of 2^15, is below 2^20)
    return P;
}
// One step of a call: MSMs [j0, j1).  single: the one MSM j0 goes through msm_enqueue (the call has one MSM, or the member exceeds
// MSM_MANY_PAIRS_MAX); otherwise the pass below.
struct msm_many_pass {
    bool single;
    size_t j0, j1;
    size_t pair0;                      // the pass's first pair in the call's scalar array (ragged: in its point array as well)
    uint32_t pairs;                    // 0: every member is empty, the results are infinity and nothing is launched
    uint32_t points;                   // what k_pip_convert converts for it: the pass's pairs (ragged), all npoints once per call (shared)
    uint32_t nv, total, nseg;          // virtual windows, buckets, 16-bucket segments
    uint32_t pair_grid;                // x of k_pipm_hist / k_pipm_scatter (y: the nwin windows of an MSM): a lane per pair
    uint32_t order_grid, bucket_grid;  // k_msm_order_hist / _scatter, k_pip_bucket over all buckets of the pass
    uint32_t team, segred_grid;        // k_pip_segred_team<team> (4, 2) | k_pip_segred (1)
};
// offsets: the call's k + 1 (ragged) or nullptr (shared); the caller has checked them
inline msm_many_pass msm_many_next(const msm_many_plan& P, const size_t* offsets, size_t npoints, size_t k, size_t j0) {
    msm_many_pass s{};
    const auto len = [&](size_t j) { return offsets ? offsets[j + 1] - offsets[j] : npoints; };
    s.j0 = j0, s.j1 = j0 + 1;
    s.pair0 = offsets ? offsets[j0] : j0 * npoints;
    if (k == 1 || len(j0) > MSM_MANY_PAIRS_MAX) {
        s.single = true;
        return s;
    }
    size_t pairs = len(j0);
    while (s.j1 < k && s.j1 - j0 < P.msms_max && len(s.j1) <= MSM_MANY_PAIRS_MAX && pairs + len(s.j1) <= MSM_MANY_PAIRS_MAX) pairs += len(s.j1++);
    const uint32_t kp = (uint32_t)(s.j1 - j0);
    s.pairs = (uint32_t)pairs;
    s.points = offsets ? s.pairs : (uint32_t)npoints;
    s.nv = kp * P.W.nwin;
    s.total = kp * P.buckets_per_msm;
    s.nseg = s.nv * P.segs_per_win;
    s.pair_grid = waves_for(s.pairs);
    s.order_grid = (s.total + WAVE * MSM_ORD_PER - 1) / (WAVE * MSM_ORD_PER);
    s.bucket_grid = waves_for(s.total);
    s.team = P.g2 ? 1 : ((size_t)s.nseg * 4 <= MSM_TEAM_LANES_MAX ? 4 : ((size_t)s.nseg * 2 <= MSM_TEAM_LANES_MAX ? 2 : 1));
    s.segred_grid = waves_for(s.nseg * s.team);
    return s;
}
// The buffers of the workspace in bytes.  msm_many_extents: what the kernels of one pass touch, read off their indexing;
// msm_many_sizes_for: what msm_many_run grows the workspace to before a call - the largest extent over the call's passes
// (tests/test_msm_many_plan.py holds every pass to that).
struct msm_many_sizes {
    size_t pts_int;                    // k_pip_convert: point i at word i x 2 x FP_WORDS (G2: x 4)
    size_t offs_dev;                   // ragged: the pass's k + 1 offsets, relative to its first pair
    size_t hist;                       // one word per bucket: hist, offs, cursor, order alike
    size_t chist;                      // k_msm_order_*: 256 bins
    size_t sorted;                     // virtual window v's list from word msmmany.hpp many_list_start(v): pairs x nwin words in all
    size_t buckets, segout;            // SoA Jacobian points of G1_WORDS (G2: G2_WORDS) words: rows of `total` / `nseg`
    size_t part;                       // k_pip_winpart: a Jacobian point at (virtual window x nsplit + part)
};
inline msm_many_sizes msm_many_extents(const msm_many_plan& P, const msm_many_pass& s) {
    msm_many_sizes z{};
    if (s.single || s.pairs == 0) return z;
    const size_t jac = P.g2 ? G2_WORDS : G1_WORDS;
    z.pts_int = (size_t)s.points * (jac / 3 * 2) * 4;
    z.offs_dev = P.shared ? 0 : (s.j1 - s.j0 + 1) * 4;
    z.hist = (size_t)s.total * 4;
    z.chist = 256 * 4;
    z.sorted = (size_t)s.pairs * P.W.nwin * 4;
    z.buckets = (size_t)s.total * jac * 4;
    z.segout = (size_t)s.nseg * jac * 4;
    z.part = (size_t)s.nv * P.nsplit * jac * 4;
    return z;
}
inline msm_many_sizes msm_many_sizes_for(const msm_many_plan& P, const size_t* offsets, size_t npoints, size_t k) {
    msm_many_sizes m{};
    const auto up = [](size_t& a, size_t b) { a = a < b ? b : a; };
    for (size_t j = 0; j < k;) {
        const msm_many_pass s = msm_many_next(P, offsets, npoints, k, j);
        const msm_many_sizes z = msm_many_extents(P, s);
        up(m.pts_int, z.pts_int), up(m.offs_dev, z.offs_dev), up(m.hist, z.hist), up(m.chist, z.chist), up(m.sorted, z.sorted), up(m.buckets, z.buckets),
            up(m.segout, z.segout), up(m.part, z.part);
        j = s.j1;
    }
    return m;
}

// ------------------------------------------------------------------------------------------
// Jacobian images to affine images (mi355_bls_p1s_to_affine / mi355_bls_p2s_to_affine): what to_affine_run follows.  A lane of k_to_affine
// takes a RUN of `run` consecutive points and inverts once for all of them (csrc/toaffine.hpp): three products per point beside the one
// inversion, where a lane per point pays an inversion each.
//   run            one point per lane while the device has idle lanes (TOAFF_DEVICE_LANES: 256 CUs x 4 SIMDs x one wave of 64), then as many
//                  as spread the call over those lanes, capped at TOAFF_RUN_MAX (the lane keeps the run's prefix products in private
//                  memory).  Neither the rule nor the cap is MEASURED: a first choice.  force_run (the test hook
//                  mi355_bls_debug_to_affine_set_run) replaces the rule, capped all the same; 0: the rule.
//   one launch     at most TOAFF_CHUNK_POINTS points (point indices stay 32-bit words); a larger call is consecutive launches.
// ------------------------------------------------------------------------------------------
constexpr uint32_t TOAFF_DEVICE_LANES = 256 * 4 * WAVE;
constexpr uint32_t TOAFF_RUN_MAX = 8;
constexpr uint32_t TOAFF_CHUNK_POINTS = 1u << 24;
static_assert((uint64_t)TOAFF_CHUNK_POINTS * 288 < (1ull << 33) && TOAFF_CHUNK_POINTS % TOAFF_RUN_MAX == 0, "a chunk's byte offsets are size_t; whole runs per chunk");
struct to_affine_plan {
    uint32_t run;                      // points per lane
    uint32_t chunk;                    // points per launch
};
struct to_affine_launch {
    size_t first;                      // the launch's first point in the call
    uint32_t n;                        // its points
    uint32_t lanes, grid;              // ceil(n / run) lanes in waves of WAVE
};
inline to_affine_plan to_affine_for(size_t n, uint32_t force_run = 0) {
    to_affine_plan p{};
    size_t run = force_run ? force_run : (n + TOAFF_DEVICE_LANES - 1) / TOAFF_DEVICE_LANES;
    p.run = (uint32_t)(run < 1 ? 1 : (run > TOAFF_RUN_MAX ? TOAFF_RUN_MAX : run));
    p.chunk = TOAFF_CHUNK_POINTS;
    return p;
}
inline to_affine_launch to_affine_next(const to_affine_plan& p, size_t n, size_t first) {
    to_affine_launch l{};
    l.first = first;
    l.n = (uint32_t)(n - first < p.chunk ? n - first : p.chunk);
    l.lanes = (l.n + p.run - 1) / p.run;
    l.grid = waves_for(l.lanes);
    return l;
}

// Transforms of k vectors of n = 2^m G1 points (mi355_bls_p1s_ntt_many; csrc/p1ntt.hpp): m radix-2 stages over a workspace of internal
// Jacobian images in global memory, one lane per butterfly, then the finish to affine images; the call in SLICES of whole vectors, vectors
// [first, first + count) each.
//   P1NTT_SLICE_BYTES   n x G1_WORDS x 4 = n x 192 bytes per vector of a slice, 256 MiB in all: FRNTT_SLICE_BYTES' reasoning - a workspace
//                       the library can always ask for, far beyond the 2^16 lanes that fill the device - and like it NOT TUNED.  One
//                       vector always forms a slice, whatever its size.  The host form stages a slice's 96-byte images beside it.
//   forced_vecs         the test hook's vectors per slice (mi355_bls_debug_p1ntt_set_pass; 0: the rule above; it can only shorten a slice).
//   a stage             count x n / 2 lanes in workgroups of WAVE (p1ntt_launch_for): one vector of 2^32 points is 2^25 workgroups, and a
//                       slice of several vectors holds fewer elements than 2^21.
//   the finish          to_affine_for's run over the slice's count x n elements, a lane per run.
// Refused (ok == false): n == 0, n that is no power of two or above 2^32.  Nothing for its size.
constexpr size_t P1NTT_SLICE_BYTES = (size_t)256 << 20;
struct p1ntt_sizes {
    bool ok;
    uint32_t log2n;                          // n = 2^log2n: the stages of one transform
    size_t vecs, slices;                     // vectors per slice (the last one may hold fewer), slices of the call
    size_t twiddles, ws, staging;            // bytes: the n / 2 table entries, a slice's Jacobian images, a slice's affine images
};
inline p1ntt_sizes p1ntt_sizes_for(size_t n, size_t k, size_t forced_vecs = 0) {
    p1ntt_sizes s{};
    if (n == 0 || (n & (n - 1)) || n > ((size_t)1 << 32)) return s;
    while (((size_t)1 << s.log2n) < n) s.log2n++;
    size_t per = P1NTT_SLICE_BYTES / (n * G1_WORDS * 4);
    if (per == 0) per = 1;
    if (forced_vecs && forced_vecs < per) per = forced_vecs;
    if (per > k && k) per = k;
    s.ok = true;
    s.vecs = per;
    s.slices = (k + per - 1) / per;
    s.twiddles = n / 2 * 32;
    s.ws = per * n * G1_WORDS * 4;
    s.staging = per * n * 96;
    return s;
}
// slice i of the call: vectors [first, first + count)
inline void p1ntt_slice(const p1ntt_sizes& s, size_t k, size_t i, size_t& first, size_t& count) {
    first = i * s.vecs;
    count = k - first < s.vecs ? k - first : s.vecs;
}
// the launches of a slice of `count` vectors: workgroups of WAVE lanes of a stage, points per lane and workgroups of the finish
struct p1ntt_launch {
    uint32_t stage_grid, run, finish_grid;
};
inline p1ntt_launch p1ntt_launch_for(const p1ntt_sizes& s, size_t count) {
    p1ntt_launch l{};
    const uint64_t total = (uint64_t)count << s.log2n;
    l.stage_grid = (uint32_t)((total / 2 + WAVE - 1) / WAVE);
    l.run = to_affine_for((size_t)total).run;
    l.finish_grid = (uint32_t)(((total + l.run - 1) / l.run + WAVE - 1) / WAVE);
    return l;
}

// All openings of k polynomials of n = 2^m coefficients (mi355_bls_fk20_open_all_many; csrc/fk20.hpp): the call in PASSES of whole
// polynomials, polynomials [first, first + count) each.
//   FK20_PASS_BYTES     the workspace a pass may ask for, 256 MiB in all: per polynomial 2n internal Jacobian images (G1_WORDS x 4 = 192
//                       bytes each) and 2n scalars (32 bytes each), 448 n bytes.  P1NTT_SLICE_BYTES' reasoning, and like it NOT TUNED.  One
//                       polynomial always forms a pass, whatever its size: nothing is refused for its size.  The host form stages a pass's
//                       n coefficient images and n affine outputs per polynomial beside it.
//   forced              the test hook's polynomials per pass (mi355_bls_debug_fk20_set_pass; 0: the rule above; it can only shorten a pass).
//   the launches        (fk20_launch_for) the layout: a lane per run of FRNTT_RUN slots of the count x 2n array, FRNTT_LANES per workgroup;
//                       the pointwise product: a lane per slot; a stage of the inverse: count x n butterflies; a stage of the forward:
//                       count x n / 2; the finish: to_affine_for's run over count x n elements.  One polynomial of 2^31 coefficients is
//                       2^26 workgroups of WAVE lanes in the widest launch.
// Refused (ok == false): n == 0, n that is no power of two or above 2^31 - the transform of 2n points must fit p1ntt_sizes_for's bound.
constexpr size_t FK20_PASS_BYTES = (size_t)256 << 20;
constexpr size_t FK20_POLY_BYTES_PER_COEFF = 2 * (G1_WORDS * 4 + 32);
constexpr uint32_t FK20_CIRC_RUN = 16, FK20_CIRC_LANES = 256;            // frntt.hpp's FRNTT_RUN and FRNTT_LANES (asserted where both are seen)
struct fk20_sizes {
    bool ok;
    uint32_t log2n;                          // n = 2^log2n
    size_t per_pass, passes;                 // polynomials per pass (the last one may hold fewer), passes of the call
    size_t ws, scalars;                      // bytes: a pass's 2n Jacobian images and 2n scalars per polynomial
    size_t polys, out, status;               // bytes: a pass's coefficient images, its affine outputs, a status word per polynomial
    size_t tw_fr, tw_inv, tw_fwd;            // bytes: the tables of omega_2n (n entries), 1 / omega_2n (n entries) and omega_n (n / 2 entries)
};
inline fk20_sizes fk20_sizes_for(size_t n, size_t k, size_t forced = 0) {
    fk20_sizes s{};
    if (n == 0 || (n & (n - 1)) || n > ((size_t)1 << 31)) return s;
    while (((size_t)1 << s.log2n) < n) s.log2n++;
    size_t per = FK20_PASS_BYTES / (n * FK20_POLY_BYTES_PER_COEFF);
    if (per == 0) per = 1;
    if (forced && forced < per) per = forced;
    if (per > k && k) per = k;
    s.ok = true;
    s.per_pass = per;
    s.passes = (k + per - 1) / per;
    s.ws = per * 2 * n * G1_WORDS * 4;
    s.scalars = per * 2 * n * 32;
    s.polys = per * n * 32;
    s.out = per * n * 96;
    s.status = per * 4;
    s.tw_fr = n * 32;
    s.tw_inv = n * 32;
    s.tw_fwd = n / 2 * 32;
    return s;
}
// pass p of the call: polynomials [first, first + count)
inline void fk20_pass(const fk20_sizes& s, size_t k, size_t p, size_t& first, size_t& count) {
    first = p * s.per_pass;
    count = k - first < s.per_pass ? k - first : s.per_pass;
}
// the bytes of a setup handle's device memory: NTT_2n(s^) as 2n affine images; 0 where n is refused
inline size_t fk20_setup_bytes(size_t n) { return fk20_sizes_for(n, 1).ok ? 2 * n * 96 : 0; }
// the launches of a pass of `count` polynomials
struct fk20_launch {
    uint32_t circ_grid, point_grid, inv_grid, fwd_grid, run, finish_grid;
};
inline fk20_launch fk20_launch_for(const fk20_sizes& s, size_t count) {
    fk20_launch l{};
    const uint64_t half = (uint64_t)count << s.log2n, total = half << 1;
    const uint64_t runs_per_poly = ((total / count) + FK20_CIRC_RUN - 1) / FK20_CIRC_RUN;
    l.circ_grid = (uint32_t)((count * runs_per_poly + FK20_CIRC_LANES - 1) / FK20_CIRC_LANES);
    l.point_grid = (uint32_t)((total + WAVE - 1) / WAVE);
    l.inv_grid = (uint32_t)((half + WAVE - 1) / WAVE);
    l.fwd_grid = (uint32_t)((half / 2 + WAVE - 1) / WAVE);
    l.run = to_affine_for((size_t)half).run;
    l.finish_grid = (uint32_t)(((half + l.run - 1) / l.run + WAVE - 1) / WAVE);
    return l;
}

// The proofs of all cells of k polynomials (mi355_bls_fk20_open_cells_many; csrc/fk20cells.hpp): n = 2^m coefficients, cells of
// `cell` = l = 2^c points, q = n / l, N = q 2^ext cells; PASSES of whole polynomials under the same FK20_PASS_BYTES.  Per polynomial a pass
// holds 2n scalars (the l transforms of 2q), 2n product images and W = max(2q, N) workspace images: 448 n + 192 W bytes.  One polynomial
// always forms a pass, nothing is refused for its size, and `forced` (mi355_bls_debug_fk20_set_pass) only shortens a pass.
//   the launches        (fk20_cells_launch_for) the layout: a lane per run of FRNTT_RUN slots of the (count l) x 2q array; the product: a
//                       lane per term, count x 2n; level t of the sum (fk20_cells_sum_lanes): a lane per group of up to FK20_CELLS_FAN
//                       images, the last level count x 2q lanes; a stage of the inverse: count x q butterflies; the padding: a lane per
//                       element of count x N (none for N == q); a stage of the forward: count x N / 2; the finish: to_affine_for's run
//                       over count x N elements, with MI355_BLS_FK20_H over count x q.
// Refused (ok == false): what fk20_sizes_for refuses, a cell that is 0, no power of two or above n, ext_log2 with n 2^ext > 2^32 (so N and
// the transform of 2q both fit p1ntt_sizes_for's bound).
constexpr uint32_t FK20_CELLS_FAN_LOG2 = 3;                              // fk20cells.hpp's FK20C_FAN_LOG2 (asserted where both are seen)
struct fk20_cells_sizes {
    bool ok;
    uint32_t log2n, log2cell, log2q, log2cells, log2w;   // n, l, q = n / l, N = q 2^ext, W = max(2q, N)
    size_t per_pass, passes;                 // polynomials per pass (the last one may hold fewer), passes of the call
    size_t scalars, prod, ws;                // bytes: a pass's 2n scalars, 2n product images and W workspace images per polynomial
    size_t polys, out, status;               // bytes: a pass's coefficient images, its N affine outputs per polynomial, a status word each
    size_t tw_fr, tw_inv, tw_fwd;            // bytes: the tables of omega_2q (q entries), 1 / omega_2q (q entries) and omega_N (N / 2 entries)
};
inline fk20_cells_sizes fk20_cells_sizes_for(size_t n, size_t cell, size_t ext_log2, size_t k, size_t forced = 0) {
    fk20_cells_sizes s{};
    if (!fk20_sizes_for(n, 1).ok || cell == 0 || (cell & (cell - 1)) || cell > n) return s;
    while (((size_t)1 << s.log2n) < n) s.log2n++;
    if (ext_log2 > 32 || s.log2n + ext_log2 > 32) return s;
    while (((size_t)1 << s.log2cell) < cell) s.log2cell++;
    s.log2q = s.log2n - s.log2cell;
    s.log2cells = s.log2q + (uint32_t)ext_log2;
    s.log2w = s.log2cells > s.log2q + 1 ? s.log2cells : s.log2q + 1;
    const size_t w = (size_t)1 << s.log2w, cells = (size_t)1 << s.log2cells, q = (size_t)1 << s.log2q;
    size_t per = FK20_PASS_BYTES / (n * FK20_POLY_BYTES_PER_COEFF + w * G1_WORDS * 4);
    if (per == 0) per = 1;
    if (forced && forced < per) per = forced;
    if (per > k && k) per = k;
    s.ok = true;
    s.per_pass = per;
    s.passes = (k + per - 1) / per;
    s.scalars = per * 2 * n * 32;
    s.prod = per * 2 * n * G1_WORDS * 4;
    s.ws = per * w * G1_WORDS * 4;
    s.polys = per * n * 32;
    s.out = per * cells * 96;
    s.status = per * 4;
    s.tw_fr = q * 32;
    s.tw_inv = q * 32;
    s.tw_fwd = cells / 2 * 32;
    return s;
}
// pass p of the call: polynomials [first, first + count)
inline void fk20_cells_pass(const fk20_cells_sizes& s, size_t k, size_t p, size_t& first, size_t& count) {
    first = p * s.per_pass;
    count = k - first < s.per_pass ? k - first : s.per_pass;
}
// the levels of the sum over l = 2^log2cell terms, and the lanes of level t for `count` polynomials: level t adds groups of
// 2^min(FK20_CELLS_FAN_LOG2, what is left) images; l == 1 is one level, the copy
inline uint32_t fk20_cells_sum_levels(const fk20_cells_sizes& s) { return s.log2cell == 0 ? 1 : (s.log2cell + FK20_CELLS_FAN_LOG2 - 1) / FK20_CELLS_FAN_LOG2; }
inline uint64_t fk20_cells_sum_lanes(const fk20_cells_sizes& s, size_t count, uint32_t t) {
    const uint32_t done = (t + 1) * FK20_CELLS_FAN_LOG2 < s.log2cell ? (t + 1) * FK20_CELLS_FAN_LOG2 : s.log2cell;
    return (uint64_t)count << (s.log2q + 1 + s.log2cell - done);
}
struct fk20_cells_launch {
    uint32_t circ_grid, point_grid, inv_grid, pad_grid, fwd_grid, run, finish_grid, run_h, finish_h_grid;
};
inline fk20_cells_launch fk20_cells_launch_for(const fk20_cells_sizes& s, size_t count) {
    fk20_cells_launch l{};
    const uint64_t terms = (uint64_t)count << (s.log2n + 1), hs = (uint64_t)count << s.log2q, cells = (uint64_t)count << s.log2cells;
    const uint64_t runs_per_vec = (((uint64_t)2 << s.log2q) + FK20_CIRC_RUN - 1) / FK20_CIRC_RUN;
    l.circ_grid = (uint32_t)((((uint64_t)count << s.log2cell) * runs_per_vec + FK20_CIRC_LANES - 1) / FK20_CIRC_LANES);
    l.point_grid = (uint32_t)((terms + WAVE - 1) / WAVE);
    l.inv_grid = (uint32_t)((hs + WAVE - 1) / WAVE);
    l.pad_grid = s.log2cells > s.log2q ? (uint32_t)((cells + WAVE - 1) / WAVE) : 0;
    l.fwd_grid = (uint32_t)((cells / 2 + WAVE - 1) / WAVE);
    l.run = to_affine_for((size_t)cells).run;
    l.finish_grid = (uint32_t)(((cells + l.run - 1) / l.run + WAVE - 1) / WAVE);
    l.run_h = to_affine_for((size_t)hs).run;
    l.finish_h_grid = (uint32_t)(((hs + l.run_h - 1) / l.run_h + WAVE - 1) / WAVE);
    return l;
}

// ------------------------------------------------------------------------------------------
// Fixed-base G1 MSM over a precomputed window table (mi355_bls_p1s_table_* / mi355_bls_p1s_mult_table*): what ptab_run follows and reserves.
// The table holds, for point i and window w, the affine row T[w][i] = [2^(w wbits)] P_i at entry w x npoints + i (k_pip_convert's record).
// An MSM is sum_i sum_w d_(i,w) T[w][i] over the signed digits d of the existing sort: no window needs a Horner step, so all W windows of
// an MSM may share buckets.  MSM j of a pass owns S bucket SETS (1 <= S <= W), window w falls into set j S + w mod S; from the sort on,
// k_msm_order_*, k_pip_bucket, k_pip_segred(_team) and k_pip_winpart see one MSM of (MSMs of the pass) x S windows, and k_pip_rowtail_many,
// given a window plan of S windows of width 0, adds each MSM's S window parts without a doubling.
//   windows        UNIFORM: W = ceil((nbits + 1) / wbits) windows of wbits bits (fixed_win: wrem = 0, wbase = wbits), 2^(wbits - 1) buckets per
//                  set.  A table made for nbits serves every smaller nbits: its first W' <= W rows.
//   wbits          5 .. 16 (pip_for's limits), or the rule fixed_wbits_for: changed once after the first measurement, see there.
//   S              fixed_for: the fewest sets with which the buckets of one pass give k_pip_bucket two waves per SIMD.  A first choice: the
//                  benchmark has run with it, no other rule was tried.
//   one pass       a range of whole MSMs: at least one, further ones while the pairs stay within pairs_max (FIXED_PAIRS_MAX; a parameter so
//                  that a test can cut a small call) and the sets and buckets within msm_many's limits.  One MSM always fits: a table has at
//                  most FIXED_ENTRIES_MAX entries, so its W lists hold at most 2^31 positions.
// Measured with nim-blscurve_amd/tools/bench_msm_table.py (profiles/msm_table_bench.json; DESIGN.md 3.2.9 says where the call wins and loses).
// ------------------------------------------------------------------------------------------
constexpr uint32_t FIXED_WBITS_MIN = 5, FIXED_WBITS_MAX = 16;
// k_pip_bucket reads a sorted word as (record index & 0x7fffffff, sign = bit 31) and addresses the record at 128 x index in 64 bits: a table
// may hold at most 2^31 entries (W x npoints).
constexpr uint64_t FIXED_ENTRIES_MAX = 1ull << 31;
constexpr size_t FIXED_ENTRY_BYTES = 2 * FP_WORDS * 4;
constexpr uint32_t FIXED_PAIRS_MAX = MSM_MANY_PAIRS_MAX;
constexpr size_t FIXED_SCRATCH_BYTES = (size_t)256 << 20;      // k_ptab_rows: Z and prefix-product columns of one chunk of points
inline uint32_t fixed_nwin(size_t wbits, size_t nbits) { return (uint32_t)((nbits + 1 + wbits - 1) / wbits); }
// 8 bits below 2^14 points, 16 from there on.  Uniform windows leave the TOP window (nbits + 1) - (W - 1) wbits bits; where that is much less
// than wbits, all n points of that window crowd into its few buckets and k_pip_bucket's one lane per bucket adds them serially.  The first
// rule here, about log2(n) bits, chose 12 at 4 096 points: 255-bit scalars then have a 4-bit top window, and the bucket kernel took 4.9 ms of
// a 5.4 ms call (1.34 ms generic); 1.18 s at 2^20 points.  For 255- and 256-bit scalars the widths whose top window is full are 8 and 16;
// measured (profiles/msm_table_bench.json), 8 wins every 4 096-point shape and 16 wins at 2^16 points, where 8 has too few buckets (32 x 128)
// to fill the chip.  The hand-over between them, 2^14, is not measured.
constexpr size_t FIXED_WBITS_WIDE_FROM = (size_t)1 << 14;
inline uint32_t fixed_wbits_for(size_t npoints) { return npoints < FIXED_WBITS_WIDE_FROM ? 8 : 16; }
// what create accepts (wbits 0: the rule)
inline bool fixed_args_ok(size_t npoints, size_t wbits, size_t nbits) {
    if (npoints == 0 || nbits == 0 || nbits > 256 || (wbits != 0 && (wbits < FIXED_WBITS_MIN || wbits > FIXED_WBITS_MAX))) return false;
    if (npoints > FIXED_ENTRIES_MAX) return false;
    const uint64_t W = fixed_nwin(wbits ? wbits : fixed_wbits_for(npoints), nbits);
    return W * (uint64_t)npoints <= FIXED_ENTRIES_MAX;
}
// device bytes of a table; 0 for arguments create refuses
inline size_t fixed_table_bytes(size_t npoints, size_t wbits, size_t nbits) {
    if (!fixed_args_ok(npoints, wbits, nbits)) return 0;
    return (size_t)fixed_nwin(wbits ? wbits : fixed_wbits_for(npoints), nbits) * npoints * FIXED_ENTRY_BYTES;
}
// the windows of a call as the kernels take them; wbits in 5 .. 16, nbits in 1 .. 256
inline pip_win fixed_win(size_t wbits, size_t nbits) {
    pip_win W{};
    W.nbits = (uint32_t)nbits;
    W.nwin = fixed_nwin(wbits, nbits);
    W.wbase = (uint32_t)wbits, W.wrem = 0;
    W.cbk = (uint32_t)wbits - 1;
    for (uint32_t w = 0; w + 1 < W.nwin; w++) {
        const uint32_t bit = w * W.wbase + W.wbase - 1;      // + 2^(wbits - 1) at every window but the top one; bit < 272
        W.H[bit >> 5] |= 1u << (bit & 31);
    }
    return W;
}
// k_ptab_rows: points per launch, so that the two scratch columns of a chunk stay within FIXED_SCRATCH_BYTES (at least a wave)
inline uint32_t fixed_rows_chunk(size_t npoints, uint32_t nwin) {
    size_t c = FIXED_SCRATCH_BYTES / ((size_t)nwin * FIXED_ENTRY_BYTES);
    c = c / WAVE * WAVE;
    if (c < WAVE) c = WAVE;
    return (uint32_t)(c < npoints ? c : npoints);
}
struct fixed_plan {
    pip_win W;                         // of the CALL's nbits (the table's wbits)
    uint32_t n;                        // points = pairs per MSM
    uint32_t S;                        // bucket sets per MSM
    uint32_t buckets_per_msm;          // S << cbk
    uint32_t segs_per_set, nsplit;     // as msm_plan's per window
    uint32_t tail_waves, tail_lanes;   // k_pip_rowtail_many's workgroup (one per MSM): a wave per set up to MSM_TAIL_WAVES_MAX
    uint32_t pairs_max, msms_max;      // what a pass takes at the most (it always takes one MSM)
};
// W: fixed_win of the table's wbits and the call's nbits; slots: the device's wave slots at one wave per SIMD; force_S: a test's choice (0: the rule)
inline fixed_plan fixed_for(size_t npoints, const pip_win& W, size_t k, uint32_t slots, uint32_t pairs_max = FIXED_PAIRS_MAX, uint32_t force_S = 0) {
    fixed_plan P{};
    P.W = W;
    P.n = (uint32_t)npoints;
    P.pairs_max = pairs_max;
    size_t fit = npoints ? pairs_max / npoints : 1;      // MSMs of a pass by the pair bound
    if (fit < 1) fit = 1;
    if (fit > k && k) fit = k;
    // two waves per SIMD of one-lane-per-bucket work: 2 x slots x WAVE buckets in the pass
    const uint64_t want = 2ull * slots * WAVE, have = (uint64_t)fit << W.cbk;
    uint64_t S = (want + have - 1) / have;
    if (S < 1) S = 1;
    if (S > W.nwin) S = W.nwin;
    if (force_S) S = force_S > W.nwin ? W.nwin : force_S;
    P.S = (uint32_t)S;
    P.buckets_per_msm = P.S << W.cbk;
    P.segs_per_set = (1u << W.cbk) / MSM_SEG;
    P.nsplit = P.segs_per_set >= 1024 ? 16 : (P.segs_per_set >= 128 ? 4 : 1);
    P.tail_waves = P.S < MSM_TAIL_WAVES_MAX ? P.S : MSM_TAIL_WAVES_MAX;
    P.tail_lanes = P.tail_waves * WAVE;
    const uint32_t by_sets = MSM_MANY_VWIN_MAX / P.S, by_buckets = MSM_MANY_BUCKETS_MAX / P.buckets_per_msm;      // >= 1: 52 sets of 2^4, 17 of 2^15
    P.msms_max = by_sets < by_buckets ? by_sets : by_buckets;
    return P;
}
// One pass of a call: MSMs [j0, j1) of k
struct fixed_pass {
    size_t j0, j1;
    size_t pair0;                      // the pass's first pair in the call's scalar array
    uint32_t pairs;
    uint32_t nv, total, nseg;          // bucket sets, buckets, 16-bucket segments
    uint32_t pair_grid;                // x of k_ptab_hist / k_ptab_scatter (y: the W windows): a lane per pair
    uint32_t order_grid, bucket_grid;  // k_msm_order_hist / _scatter, k_pip_bucket over all buckets of the pass
    uint32_t team, segred_grid;        // k_pip_segred_team<team> (4, 2) | k_pip_segred (1)
};
inline fixed_pass fixed_next(const fixed_plan& P, size_t k, size_t j0) {
    fixed_pass s{};
    s.j0 = j0, s.j1 = j0 + 1;
    s.pair0 = j0 * (size_t)P.n;
    size_t pairs = P.n;
    while (s.j1 < k && s.j1 - j0 < P.msms_max && pairs + P.n <= P.pairs_max) pairs += P.n, s.j1++;
    const uint32_t kp = (uint32_t)(s.j1 - j0);
    s.pairs = (uint32_t)pairs;
    s.nv = kp * P.S;
    s.total = kp * P.buckets_per_msm;
    s.nseg = s.nv * P.segs_per_set;
    s.pair_grid = waves_for(s.pairs);
    s.order_grid = (s.total + WAVE * MSM_ORD_PER - 1) / (WAVE * MSM_ORD_PER);
    s.bucket_grid = waves_for(s.total);
    s.team = (size_t)s.nseg * 4 <= MSM_TEAM_LANES_MAX ? 4 : ((size_t)s.nseg * 2 <= MSM_TEAM_LANES_MAX ? 2 : 1);
    s.segred_grid = waves_for(s.nseg * s.team);
    return s;
}
// The buffers of the workspace in bytes.  fixed_extents: what the kernels of one pass touch, read off their indexing; fixed_sizes_for: what
// ptab_run grows the workspace to before a call - the largest extent over the call's passes (tests/test_msm_table_plan.py holds every pass
// to that).
struct fixed_sizes {
    size_t hist;                       // one word per bucket: hist, offs, cursor, order alike
    size_t chist;                      // k_msm_order_*: 256 bins
    size_t sorted;                     // set v's list from word msmtable.hpp fixed_list_start(v): pairs x W words in all
    size_t buckets, segout;            // SoA Jacobian G1 points: rows of `total` / `nseg`
    size_t part;                       // k_pip_winpart: a Jacobian point at (set x nsplit + part)
    size_t out;                        // a blst_p1 image per MSM of the pass
};
inline fixed_sizes fixed_extents(const fixed_plan& P, const fixed_pass& s) {
    fixed_sizes z{};
    z.hist = (size_t)s.total * 4;
    z.chist = 256 * 4;
    z.sorted = (size_t)s.pairs * P.W.nwin * 4;
    z.buckets = (size_t)s.total * G1_WORDS * 4;
    z.segout = (size_t)s.nseg * G1_WORDS * 4;
    z.part = (size_t)s.nv * P.nsplit * G1_WORDS * 4;
    z.out = (s.j1 - s.j0) * 144;
    return z;
}
inline fixed_sizes fixed_sizes_for(const fixed_plan& P, size_t k) {
    // every pass takes as many MSMs as the first one, but the last, which takes the rest: the first pass bounds them all
    return k ? fixed_extents(P, fixed_next(P, k, 0)) : fixed_sizes{};
}

// chunk of the parallel_chunks partition (parallel_chunks.nim:42-66) that tuple t of n_total falls into, B chunks
inline uint32_t chunk_of_tuple(size_t n_total, uint32_t B, size_t t) {
    size_t base = n_total / B, rem = n_total % B, cut = (base + 1) * rem;
    return (uint32_t)(t < cut ? t / (base + 1) : rem + (t - cut) / base);
}

// ------------------------------------------------------------------------------------------
// batchVerify by message (mi355_bls_batch_verify_by_message): one slice of n sets that the device grouping found to hold k distinct messages.
// The per-SET stages - [r]PK, the signature side with its `total` extra pairs, and the streams they take - are slice_for's for n; the
// per-PAIR stages - hashing, clearing, Miller lines - are the same deciders asked for k (the latency forms where k is small), with the
// extra pairs behind them at slots k .. k + total.  slice_for itself is not touched.
//   ordinary: k == n, nothing is shared: the call runs run_pairs as it stands (same result, none of the grouped pass's extra kernels).
//   BYMSG_MIN_SHARED is the hook for a "not worth grouping" threshold: n - k below it would also take the ordinary path.  UNSET (0):
//   nobody has measured where the grouped pass stops paying for its sums, and no value is invented here.
//   table_slots: the open-addressing table of the grouping, a power of two of at least 2 n slots (csrc/bymsg.hpp).
// ------------------------------------------------------------------------------------------
constexpr size_t BYMSG_MIN_SHARED = 0;
constexpr uint32_t bymsg_table_slots(size_t n) {
    uint32_t s = 2;
    while (s < 2 * (uint64_t)n) s <<= 1;
    return s;
}
struct grouped_plan {
    bool ordinary;
    uint32_t table_slots;
    uint32_t grid_n, grid_k;           // waves of the one-lane-per-set / one-lane-per-group kernels
    slice_plan sets;                   // slice_for(n): nb, pkmul_spread, side, the streams, cw / nwin / total, lshift, bucket_grid
    hash_map_plan hash_map;            // k messages
    stage clear;
    bool extra_apart;                  // as in slice_plan, for the pairs of this pass
    stage extra_lines;
    lines_plan lines;                  // the caller's stream: the k group pairs (extra_apart) or all k + total pairs
};
inline grouped_plan slice_for_grouped(uint32_t slots, bool coop, bool have_side, size_t n, size_t k) {
    grouped_plan g{};
    const uint32_t k32 = (uint32_t)k;
    g.ordinary = k == n || n - k + 1 <= BYMSG_MIN_SHARED;      // (n - k < the hook, written so that 0 switches it off)
    g.table_slots = bymsg_table_slots(n);
    g.grid_n = waves_for((uint32_t)n), g.grid_k = waves_for(k32);
    g.sets = slice_for(slots, coop, have_side, n);
    g.hash_map = hash_map_for(slots, coop, k32);
    g.clear = clear_for(slots, coop, k32);
    const uint32_t total = g.sets.total;
    g.extra_apart = g.sets.side == SIDE_FORK_SIG || (g.sets.side == SIDE_FORK && total <= team_lines_max(slots));
    g.extra_lines = total <= team_lines_max(slots) ? team_stage(slots, total) : one_lane_stage(total);
    g.lines = g.extra_apart ? lines_for(slots, coop, k32, 0) : lines_for(slots, coop, k32 + total, total);
    return g;
}

// The host inputs of a grouped call in ONE staging buffer: the parts in the order given, each at the next multiple of 4 bytes behind the one
// before (the kernels load words, and hand a part on as a table of its own).  A part of zero bytes takes no room.  total: what to reserve -
// the end of the last part and a word, so that the word a byte-aligned last part ends in lies inside and an empty call still has an address.
constexpr size_t PACK_PARTS_MAX = 6;
struct pack_layout {
    size_t at[PACK_PARTS_MAX];
    size_t total;
};
// n <= PACK_PARTS_MAX; more parts than the layout can name give total == 0, which no call with parts has
inline pack_layout pack_for(const size_t* bytes, size_t n) {
    pack_layout p{};
    if (n > PACK_PARTS_MAX) return p;
    size_t end = 0;
    for (size_t i = 0; i < n; i++) {
        p.at[i] = (end + 3) & ~(size_t)3;
        end = p.at[i] + bytes[i];
    }
    p.total = end + 4;
    return p;
}

// The per-row calls' staging.  The context's two staging buffers hold cap_io rows of ROW_BYTES each (io_reserve); an array a call stages is a
// COLUMN: `width` bytes per row (its widest form: a compressed key takes 48 of a key column's 96), starting at buffer + cap_io * start, so columns
// apart in a row are apart in the buffer whatever cap_io is.  Calls that use a buffer from offset 0 as one array (records, the decoders' output,
// fastAggregateVerify, combine, the MSM host forms) have none.  X(name, call, column, buffer, start, width, the column of that call it shares bytes with):
constexpr size_t ROW_BYTES = 320;
enum row_buf { ROW_COMP, ROW_SETS };         // d_comp, d_sets
struct row_col {
    row_buf buf;
    uint32_t start, width;
};
#define BLS_ROW_COLUMNS(X)                                                                      \
    X(CPK_IN, "compress_public_keys", "keys in", ROW_COMP, 0, 96, nullptr)                      \
    X(CPK_OUT, "compress_public_keys", "out", ROW_COMP, 96, 48, nullptr)                        \
    X(CSIG_IN, "compress_signatures", "signatures in", ROW_COMP, 0, 192, nullptr)               \
    X(CSIG_OUT, "compress_signatures", "out", ROW_COMP, 192, 96, nullptr)                       \
    X(DSIG_WIRE, "deserialize_signatures", "wire", ROW_COMP, 0, 192, nullptr)                   \
    X(DPK_WIRE, "deserialize_public_keys", "wire", ROW_COMP, 0, 96, nullptr)                    \
    X(POP_KEYS, "pop_verify", "keys", ROW_COMP, 0, 96, nullptr) /* the host forms: pop_stage */ \
    X(POP_PROOFS, "pop_verify", "proofs", ROW_COMP, 96, 192, nullptr)                           \
    X(ADMIT_KEYS, "admit_keys", "decoded keys", ROW_COMP, 0, 96, nullptr) /* host form only */  \
    X(ADMIT_PROOFS, "admit_keys", "decoded proofs", ROW_COMP, 96, 192, nullptr)                 \
    X(ADMIT_LIST, "admit_keys", "row list", ROW_COMP, 288, 4, nullptr)                          \
    X(ADMIT_PROOF_ST, "admit_keys", "proof status", ROW_COMP, 292, 1, nullptr)                  \
    X(ADMIT_WIRE_KEYS, "admit_keys", "wire keys", ROW_SETS, 0, 96, nullptr) /* host form */     \
    X(ADMIT_WIRE_PROOFS, "admit_keys", "wire proofs", ROW_SETS, 96, 192, nullptr)               \
    X(SETS_KEYS, "deserialize_sets", "keys", ROW_COMP, 0, 96, nullptr) /* and _ex, batch_verify_compressed */ \
    X(SETS_MSGS, "deserialize_sets", "messages", ROW_COMP, 96, 32, nullptr)                     \
    X(SETS_SIGS, "deserialize_sets", "signatures", ROW_COMP, 128, 192, nullptr)                 \
    X(SIGN_SKS, "sign_sets", "scalars", ROW_COMP, 0, 32, nullptr)                               \
    X(SIGN_MSGS, "sign_sets", "messages", ROW_COMP, 48, 32, nullptr)                            \
    X(PROVE_KEYS, "pop_prove", "keys out", ROW_COMP, 0, 96, nullptr)                            \
    X(PROVE_PROOFS, "pop_prove", "proofs out", ROW_COMP, 96, 192, nullptr)                      \
    X(PROVE_SKS, "pop_prove", "scalars", ROW_COMP, 288, 32, nullptr)                            \
    X(PROVE_ZERO_MSGS, "pop_prove", "zero messages", ROW_COMP, 96, 32, "proofs out")
// The one sharing: the zero messages k_sign_pk copies into pop_prove's records (device form) lie in the proofs' column; k_pop_prove_sig writes
// the host form's proofs there behind k_sign_pk, the zero bytes' only reader, on the same stream.
namespace cols {
#define X(name, call, column, buf, start, width, shares) constexpr row_col name{buf, start, width};
BLS_ROW_COLUMNS(X)
#undef X
}  // namespace cols
// the same by call, for the check below and tests/test_pack_plan.py: the columns of one call in one buffer are live together
struct row_col_entry {
    const char *call, *column;
    row_col col;
    const char* shares;
};
#define X(name, call, column, buf, start, width, shares) {call, column, cols::name, shares},
constexpr row_col_entry ROW_COLUMNS[] = {BLS_ROW_COLUMNS(X)};
#undef X
constexpr size_t ROW_COLUMN_COUNT = sizeof(ROW_COLUMNS) / sizeof(ROW_COLUMNS[0]);
constexpr bool same_text(const char* a, const char* b) {
    while (a && b && *a && *a == *b) a++, b++;
    return a && b && *a == *b;
}
constexpr bool row_columns_ok() {
    for (size_t i = 0; i < ROW_COLUMN_COUNT; i++) {
        const row_col_entry& a = ROW_COLUMNS[i];
        if (a.col.width == 0 || a.col.start + a.col.width > ROW_BYTES) return false;
        for (size_t j = 0; j < i; j++) {
            const row_col_entry& b = ROW_COLUMNS[j];
            const bool apart = a.col.start + a.col.width <= b.col.start || b.col.start + b.col.width <= a.col.start;
            if (same_text(a.call, b.call) && a.col.buf == b.col.buf && !apart && !same_text(a.shares, b.column) && !same_text(b.shares, a.column)) return false;
        }
    }
    return true;
}
static_assert(row_columns_ok(), "a column of the per-row staging ends behind its 320-byte row, or two columns of one call overlap undeclared");

}  // namespace plan
#endif
