// Host layer of the MI355X batch-verification library: contexts, the C ABI declared in include/blscurve_mi355x.h, the slice pipeline
// of batches larger than a workspace, the multi-device drivers, the Pippenger host side.  Included by kernels.hip (same translation
// unit: the kernels it launches live in that file's anonymous namespace); not a stand-alone source.
#pragma once
#include "plan.hpp"      // which kernel, what grid, which stream: every size decision of this file
#include "devres.hpp"    // the owners of device buffers, events, streams and pinned memory
using plan::SIG_SLOTS_MAX;
namespace cols = plan::cols;      // the columns of the per-row calls' staging
static_assert(plan::WAVE == (uint32_t)WAVE && plan::N_LINES == (uint32_t)N_LINES, "plan.hpp restates the wave size and the Miller loop's step count");
static_assert(plan::FP_WORDS == (uint32_t)FPW && plan::G1_WORDS == (uint32_t)G1W && plan::G2_WORDS == (uint32_t)G2W && plan::F12_WORDS == (uint32_t)F12W,
              "plan.hpp restates the words of an element in device buffers");

// ------------------------------------------------------------------------------------------
// Context
// ------------------------------------------------------------------------------------------
struct msm_ws {
    dev_buf<uint8_t> d_pts, d_sc;     // d_pts.bytes is the point capacity; hist.bytes / 4 the bucket capacity (msm_reserve)
    dev_buf<uint32_t> pts_int;
    dev_buf<uint32_t> hist, offs, cursor, sorted, order, chist, winout, out, part, shist;
    dev_event ev_fork, ev_bucketed, ev_g[2], ev_tail[2];
    dev_buf<uint4> buckets, segout;
};
// k MSMs in one pass (mi355_bls_p1s_mult_pippenger_many): buffers of its own, each grown to the call's extent (plan::msm_many_sizes_for)
struct msm_many_ws {
    dev_buf<uint8_t> d_pts, d_sc;     // the host entry's staging
    dev_buf<uint32_t> pts_int, offs_dev, hist, offs, cursor, order, chist, sorted, part, out;
    dev_buf<uint4> buckets, segout;
};
// MSMs over a fixed-base window table (mi355_bls_p1s_mult_table*): each buffer grown to the call's largest pass (plan::fixed_sizes_for); the
// scratch columns of k_ptab_rows (mi355_bls_p1s_table_create)
struct ptab_ws {
    dev_buf<uint32_t> scratch, hist, offs, cursor, order, chist, sorted, part, out;
    dev_buf<uint4> buckets, segout;
    uint32_t last_plan[3] = {0, 0, 0};              // (W, S, buckets per set) of the last mult call (mi355_bls_debug_p1s_table_last_plan)
    uint32_t force_S = 0, pairs_max = 0;            // test hook (mi355_bls_debug_p1s_table_set_plan); 0: the plan's own
};

// What the "k groups in one device pass" calls share: every buffer is sized by the call, never by max_sets, grown on demand with a quarter of
// slack (grouped_upload, stage_inputs), and free again when the call returns - each of them drains its stream first.  Who uses what:
//   items / d_items, d_flag     every one: aggregate_sets, aggregate_sets_bits (items | sets; two route counters behind the k flag words),
//                               combine_sets, aggregate_signature_sets, recover_signature_sets, by_message (table only); aggregate_verify_each
//                               has tables of its own and takes the flag words alone
//   d_status, status_h          all but by_message and aggregate_verify_each
//   d_g1_part                   aggregate_sets, aggregate_sets_bits, combine_sets (key side), by_message
//   d_g1_prod                   p1s_lincomb_many ([s_p]P_p; its partials are in d_g1_part)
//   d_g2_prod                   combine_sets ([s_j]S_j), recover_signature_sets ([l_j]S_j), p2s_lincomb_many ([s_p]Q_p)
//   d_g2_part                   combine_sets (signature side), aggregate_signature_sets, recover_signature_sets, p2s_lincomb_many
//   d_rec                       aggregate_sets, aggregate_sets_bits, combine_sets: the forms that verify their records, and the host forms
//   d_in                        the host forms of all but by_message
//   d_g2_out                    the host forms of aggregate_signature_sets, recover_signature_sets and the two lincomb_many calls
struct grouped_ws {
    std::vector<uint32_t> items;     // the item table of the call in flight (the feature's words behind it): the async copy reads it
    dev_buf<uint32_t> d_items;       // ... on the device
    dev_buf<uint32_t> d_g1_part;     // the plan's G1 partials, G1W words each
    dev_buf<uint32_t> d_g1_prod;     // a G1 product per term, G1W words each
    dev_buf<uint32_t> d_g2_prod;     // a G2 product per member, G2W words each
    dev_buf<uint32_t> d_g2_part;     // the plan's G2 partials, G2W words each
    dev_buf<uint32_t> d_flag;        // per group: an index was out of range (or what else the feature's kernels raise)
    dev_buf<uint8_t> d_status;       // per group: the status byte
    std::vector<uint8_t> status_h;   // ... on the host, for the forms that gate a verification on it
    dev_buf<uint8_t> d_rec;          // k 320-byte records
    dev_buf<uint8_t> d_in;           // host inputs staged (plan.hpp pack_for)
    dev_buf<uint8_t> d_g2_out;       // k x 192 bytes | k x 96 bytes: aggregated or recovered signatures on their way to the host
};

// the buffers Miller pairs live in, as the stage launchers take them: a view, it owns nothing
struct pair_store {
    uint4 *H, *P, *lines;
    size_t stride;
};

// Ownership: the members own (csrc/devres.hpp) and go with the context; views and raw pointers handed to launchers do not.  A routine that
// grows buffers builds the new ones in locals and swaps them in, so a failure leaves the context as it was.
struct mi355_bls_ctx {
    int device = 0;
    size_t cap = 0;          // sets the pipeline workspace holds at once (larger batches are sliced)
    size_t cap_io = 0;       // sets the staging buffers d_sets / d_comp / d_status / d_r hold (>= cap; grown on demand, io_reserve)
    size_t stride = 0;       // pairs capacity (cap + 1 rounded up to 64)
    uint32_t num_threads = 4096;
    uint32_t nblk_cap = 64;
    // device buffers
    dev_buf<uint8_t> d_sets;         // staging for host-pointer calls
    dev_buf<uint8_t> d_rnd;
    dev_buf<uint64_t> d_r;
    dev_buf<uint4> d_H;
    dev_buf<uint4> d_M;              // the two mapped points per message before cofactor clearing (2 x cap Jacobian slots)
    size_t mstride = 0;
    dev_buf<uint4> d_P;
    dev_buf<uint4> d_lines;
    dev_buf<uint8_t> d_pktab;        // k_pkmul's window tables: 8 multiples of the key with Z^2, Z^3 per set (PKTAB_BYTES each)
    // bucket fold of the signatures (batches of >= SIG_BUCKET_MIN tuples)
    dev_buf<uint32_t> d_sig_pts;     // signatures in the device representation, cap x 4 x FPW words
    dev_buf<uint32_t> d_sig_sorted;  // counting sort by digit: nwin x cap tuple indices
    dev_buf<uint32_t> d_sig_hist;    // 3 x SIG_SLOTS_MAX: histogram, offsets, cursors
    dev_buf<uint32_t> d_sig_consts;  // -[d 2^(cw)]G1 for the window widths c = 4 and c = 8
    uint32_t sig_c = 0, sig_slots = 0; // window width / bucket slots of the last batch (0: per-tuple multiplications)
    bool agg_valid = false;
    dev_buf<uint32_t> d_agg;
    dev_buf<uint32_t> d_agg1;        // G1 aggregate (blst_p1 image)
    dev_buf<uint8_t> d_msg;          // message (<= 4096 B) + signature staging
    dev_buf<uint8_t> d_comp;         // staging of the per-row calls: cap_io rows of plan::ROW_BYTES, in columns (plan.hpp cols, col_at)
    dev_buf<uint8_t> d_status;       // per-tuple deserialisation status
    dev_event ev_deser0, ev_deser1;
    float deser_ms = 0.f;
    dev_buf<uint32_t> d_lpart;
    dev_buf<uint32_t> d_L;
    dev_buf<uint32_t> d_states;      // up to 64 committed states (slot 0 = own)
    dev_buf<uint32_t> d_gt;
    dev_buf<uint32_t> d_blob;        // shard state + ok word for the device-resident exchange (MI355_BLS_BLOB_BYTES)
    uint32_t* d_blob_out = nullptr;  // where shard submits write the blob: d_blob, or a caller's device buffer (set_shard_blob_device)
    bool fv_pending = false;         // a finalverify_blobs submit has not been waited for
    hipStream_t fv_stream = nullptr;
    dev_buf<uint32_t> d_flags;       // [0] = update-failed flag, [1] = verdict, [2] = some tuple failed to deserialise / sign, [3] = verdict of finalverify_blobs
                                     // (a word and a GT buffer of its own: a blob merge may be in flight on another stream while this context takes the next shard)
    dev_buf<uint32_t> d_gt_fv;       // GT of the last finalverify_blobs
    bool gt_is_fv = false;           // fetch_stage(4): the last GT came from finalverify_blobs
    dev_buf<uint32_t> d_carry;       // 2 x 8 seed words: blinding-chain state of the chunk that a slice boundary cuts (capacity-free batches)
    bool fail_next_enqueue = false;  // test hook (mi355_bls_debug_fail_next_enqueue)
    pinned_words h_flags;            // pinned host copy of d_flags[0..1] (asynchronous submit / wait)
    bool pending = false;            // a submitted batch has not been waited for yet
    bool alone = false;              // this call was enqueued while no other batch of the process was in flight (see g_in_flight)
    int fold_form = -1;              // the fold the last call enqueued: 1 = k_fold (Fp12 engine), 0 = k_lineprod2 (mi355_bls_last_fold_form)
    bool coop = true;                // small batches: lane-cooperative kernels (latency) instead of one lane per item (throughput)
    bool wide_recorded = false;      // ev_lp (end of the whole-chip kernels) has been recorded at least once
    hipStream_t pending_stream = nullptr;      // the caller's: not owned
    dev_stream side;                 // fork / join stream of latency-mode calls (independent stages beside each other)
    dev_stream side2;                // a second one: [r]PK of a small batch beside its signature side (both beside the hashing)
    dev_buf<uint32_t> d_export;
    dev_event ev[9];
    // A batch larger than the workspace runs in slices; the slices of ONE call are pipelined over up to three workspaces - this
    // context's and two internal ones (lanes), created at the first sliced call, each on a stream of its own - like the batches of
    // three callers (run_shard).
    std::unique_ptr<mi355_bls_ctx> lane[2];
    dev_stream lane_st[2];
    dev_event lane_ev[2];
    dev_event ev_sl0, ev_blind[3];
    bool is_lane = false;
    dev_event ev_hm, ev_lp;       // inside the hash stage (after k_hash_map) and the line-product stage (after k_lineprod)
    dev_event ev_s0, ev_l0;       // start of the signature side (on its stream) and of the tuple pairs' Miller lines: the stage timers of forked calls
    float ktimes[4] = {};         // k_hash_map, k_hash_clear, k_lineprod, k_lineprod2 of the last batch call
    uint32_t slots = 1024;        // wave slots at one wave per SIMD: 4 x CUs
    // the sets of the last batch slice and the tuple pairs it left in the pair store.  Every path assigns the sets (`last_n = n`), which makes
    // the pairs as many; the by-message pass then says how many group pairs it left (fetch_stage 1 .. 3 read `pairs`).
    struct last_count {
        size_t n = 0, pairs = 0;
        last_count& operator=(size_t v) {
            n = pairs = v;
            return *this;
        }
        operator size_t() const { return n; }
    } last_n;
    bool have_gt = false;
    float timings[8] = {};
    dst_t dst;
    xmd32_consts xmd;                // message-independent SHA-256 words of expand_message_xmd for this DST
    dst_t dst_pop;                   // popVerify's tag and its constants for 48-byte messages (compressed keys): the PoP calls pass them, `dst` / `xmd` never change
    xmd48_consts xmd_pop;
    std::vector<uint64_t> h_r;       // host-computed scalar chains (serial blinding chain, combine)
    msm_ws msm;                      // lazily sized MSM workspace
    std::vector<uint8_t> av_pks, av_msgs;      // streaming aggregateVerify (mi355_bls_aggv_*): the pairs collected so far
    std::vector<uint32_t> av_offs;
    bool av_failed = false;
    msm_ws msm2;                     // a second one: combine runs its G1 and its G2 Pippenger side by side
    // per-set verification (mi355_bls_verify_each): one verdict byte per set of the call, and the values of the debug hook; grown on demand
    dev_buf<uint8_t> d_each_v;
    dev_buf<uint32_t> d_each_gt;
    dev_buf<uint4> d_each_H, d_each_P, d_each_lines;      // pairs of a slice: 2 x cap, made at the first per-set call
    dev_buf<uint32_t> d_each_work;   // the engine form's step values and results, one block per workgroup
    size_t each_stride = 0;
    int each_passes = 0;             // per-set passes made on this context (mi355_bls_debug_verify_each_passes)
    grouped_ws grp;                  // what the grouped calls share (above)
    // key aggregation by participation bits (mi355_bls_aggregate_sets_bits)
    dev_buf<uint8_t> d_aggb_mode;    // per set: the mode byte (aggbits.hpp AGGB_*)
    uint32_t aggb_routes[2] = {0, 0};      // sets of the last bits call summed directly / by exclusion (mi355_bls_debug_aggregate_bits_routes)
    // same-message pre-aggregation (mi355_bls_combine_sets): sized by the call
    dev_buf<uint64_t> d_comb_s;      // s_j by position: blinding material, cleared before every return
    dev_buf<uint8_t> d_comb_rnd;     // the groups' random bytes (cleared likewise)
    dev_buf<uint32_t> d_comb_gather; // the member records by position, when the call addresses them through indices
    dev_buf<uint4> d_comb_P;         // [s_j]PK_j, SoA Jacobian as k_pkmul writes it
    dev_buf<uint8_t> d_comb_pktab;   // the window tables of one chunk of members: k_pkmul's ...
    dev_buf<uint4> d_comb_g2tab;     // ... and k_combsets_g2mul's
    dev_buf<uint32_t> d_comb_pkflag; // k_pkmul's infinity-key word (the check items report such a key per group)
    std::vector<uint64_t> comb_s_h;  // the chains the host walks, until the call's synchronisation
    // per-group aggregateVerify (mi355_bls_aggregate_verify_each): sized by the largest SLICE of a call (plan.hpp aggveach_*), grown on demand;
    // it runs in the per-set path's pair store, verdict bytes and values
    dev_buf<uint32_t> d_aggv_part;   // the partials of a slice: per Miller step an Fp12 each
    dev_buf<uint32_t> d_aggv_step;   // the step values of a slice's groups: N_LINES x F12W words per group
    dev_buf<uint32_t> d_aggv_tab;    // a slice's groups | items
    dev_buf<uint32_t> d_aggv_carry;  // the open group's Miller value (a blst_fp12 image), and a second slot for the engine form's part
    dev_buf<uint32_t> d_aggv_work;   // the engine form's block per workgroup
    std::vector<uint32_t> aggv_tab;  // the tables of every slice of the call in flight: the async copies read them
    // batchVerify by message (mi355_bls_batch_verify_by_message): sized by the slice, grown with the call
    dev_buf<uint32_t> d_bm_tab;      // the open-addressing table: plan::bymsg_table_slots(n) set indices
    dev_buf<uint32_t> d_bm_work;     // the word arrays of the grouping (bymsg_arrays)
    dev_buf<uint4> d_bm_P;           // [r_i]PK_i of all n sets, SoA Jacobian as k_pkmul writes it
    dev_buf<uint8_t> d_bm_rec;       // the records of the k representatives, for the hashing kernels
    dev_event ev_bm;                 // the offsets are on the host
    std::vector<uint32_t> bm_offs;
    int bm_groups = -1;              // k of the last by-message slice (mi355_bls_last_message_groups)
    // k MSMs in one pass (mi355_bls_p1s_mult_pippenger_many): made at the first such call
    msm_many_ws msm_many;
    msm_many_ws msm_many2;           // ... and the G2 form's (mi355_bls_p2s_mult_pippenger_many): the same buffers over 384-byte points
    // Jacobian images to affine (mi355_bls_p1s_to_affine / mi355_bls_p2s_to_affine): the host forms' staging, and the test hook's run length
    dev_buf<uint8_t> d_toaff_in, d_toaff_out;
    uint32_t toaff_run = 0;          // mi355_bls_debug_to_affine_set_run; 0: the plan's own
    std::vector<uint32_t> many_offs; // the ragged passes' offsets of the call in flight: the async copies read them
    size_t lincomb_chunk = 0;        // mi355_bls_debug_lincomb_set_chunk: terms per chunk of the lincomb_many calls; 0: the plan's own
    // openings over Fr (mi355_bls_fr_open_many): the domain in Montgomery form | the scan workspace of a pass; the host form's outputs of a pass
    dev_buf<uint32_t> d_fro_ws, d_fro_out;
    size_t fropen_pass = 0;          // mi355_bls_debug_fropen_set_pass: polynomials per pass of the fr_open_many calls; 0: the plan's own
    // transforms over Fr (mi355_bls_fr_ntt_many): the twiddle table of the call | a slice's elements (the host form's staging; the second buffer
    // of a transform whose last store permutes) | a status word per vector of a slice
    dev_buf<uint32_t> d_ntt_tw, d_ntt_io, d_ntt_st;
    uint32_t frntt_tile = 0;         // mi355_bls_debug_frntt_set_tile: log2 of the tile of the fr_ntt_many calls; 0: the plan's own
    size_t frntt_vecs = 0;           // mi355_bls_debug_frntt_set_pass: vectors per slice of the fr_ntt_many calls; 0: the plan's own
    // transforms over G1 (mi355_bls_p1s_ntt_many): the twiddle table of the call | a slice's internal Jacobian images | the host form's
    // staging of a slice's affine images
    dev_buf<uint32_t> d_p1n_tw, d_p1n_ws, d_p1n_io;
    size_t p1ntt_vecs = 0;           // mi355_bls_debug_p1ntt_set_pass: vectors per slice of the p1s_ntt_many calls; 0: the plan's own
    // all openings (mi355_bls_fk20_open_all_many) run in the two transforms' buffers: scalars and staged coefficients in d_ntt_io, the two
    // point twiddle tables in d_p1n_tw, the Jacobian workspace in d_p1n_ws, the host form's outputs in d_p1n_io
    size_t fk20_polys = 0;           // mi355_bls_debug_fk20_set_pass: polynomials per pass of the fk20 calls; 0: the plan's own
    ptab_ws ptab;                    // MSMs over a fixed-base window table: made at the first such call
    // per-batch verdicts for many batches (mi355_bls_batch_verify_many_each): sized by the largest slice of a call; it runs in the per-set path's
    // pair store with the per-group path's tables, partials and step values (d_aggv_*) and combine_sets' G2 products and tables (grp, d_comb_*)
    dev_buf<uint8_t> d_me_meta;      // k_blind_many's table of a slice's parallel batches
    std::vector<many_meta> me_meta;  // ... of every slice of the call in flight: the async copies read them
    std::vector<uint8_t> me_rr;      // those batches' random bytes, and
    std::vector<uint64_t> me_r;      // the serial batches' chains by set: blinding material, wiped before the call returns
    int me_passes = 0;               // per-batch passes made on this context (mi355_bls_debug_batch_verify_many_each_passes)
    // pairing-product checks (mi355_bls_pairing_check_each, _products, batch_pairing_check): sized by the call (plan::pairprod_sizes_for); they
    // run in the per-set path's pair store with the per-group path's tables, partials and step values (d_aggv_*) and the grouped calls' flag words
    dev_buf<uint8_t> d_pp_status;    // a status byte per pair of the call
    dev_buf<uint64_t> d_pp_r;        // the blinded form's k group scalars: blinding material, cleared before every return
    std::vector<uint64_t> pp_r;      // ... on the host, until the call's synchronisation

    // the batch workspace's pair store (ctx_build makes it; it never changes) and the per-set path's (each_reserve)
    pair_store batch_pairs() const { return {d_H, d_P, d_lines, stride}; }
    pair_store each_pairs() const { return {d_each_H, d_each_P, d_each_lines, each_stride}; }
    // the lanes' streams drain before anything they use goes; then the lanes; then the members, in reverse order
    ~mi355_bls_ctx() {
        (void)hipSetDevice(device);
        for (int k = 0; k < 2; k++) {
            if (lane_st[k]) (void)hipStreamSynchronize(lane_st[k]);
            lane_st[k].reset();
            lane[k].reset();
        }
    }
};
// one batch per context at a time: every entry point that enqueues on a context refuses while a submitted batch is unwaited
static bool ctx_busy(const mi355_bls_ctx* c) {
    if (c->pending) g_err = "a batch submitted on this context has not been waited for";
    return c->pending;
}

// ---- the grouped calls' plumbing (grouped_ws)
// The levels of a segmented sum laid out by plan.hpp (aggsets_plan, aggbits_plan, aggveach_tab): level 0 reads the feature's operands,
// every higher level the partials of the one below.  Each callable launches `cnt` items that start at `it`.
template <class Plan, class L0, class Ln>
static void launch_levels(const Plan& p, const uint4* items, L0 level0, Ln higher) {
    for (uint32_t l = 0; l < p.levels; l++) {
        const uint32_t cnt = (uint32_t)(p.level_first[l + 1] - p.level_first[l]);
        if (l == 0) level0(items, cnt);
        else higher(items + p.level_first[l], cnt);
    }
}
// The table the feature has laid out in grp.items goes to the device on `st`, with the flag words cleared in front of it.  Table, flag words
// and status bytes grow with a quarter of slack; a count of zero leaves its buffer alone.
static int grouped_upload(mi355_bls_ctx* c, size_t tab_bytes, size_t flag_bytes, size_t status_bytes, hipStream_t st) {
    grouped_ws& g = c->grp;
    int rc = g.d_items.reserve(tab_bytes, tab_bytes / 4);
    if (!rc) rc = g.d_flag.reserve(flag_bytes, flag_bytes / 4);
    if (!rc) rc = g.d_status.reserve(status_bytes, status_bytes / 4);
    if (rc) return rc;
    if (flag_bytes) HIPCHK(hipMemsetAsync(g.d_flag, 0, flag_bytes, st));
    HIPCHK(hipMemcpyAsync(g.d_items, g.items.data(), tab_bytes, hipMemcpyHostToDevice, st));
    return 0;
}
// A host array of a call.  row != 0: rows of `row` bytes that lie `pitch` bytes apart at the source and are packed on the device.
struct host_part {
    const void* p;      // null: the call has no such part
    size_t bytes;
    size_t row = 0, pitch = 0;
};
// The host forms' inputs -> grp.d_in at the places plan::pack_for names (every part 4-byte aligned: a byte-aligned part goes last), one copy
// per non-empty part on `st`.  d[i]: where part i is on the device, null for a part the call does not have.
template <size_t N>
static int stage_inputs(mi355_bls_ctx* c, const host_part (&parts)[N], hipStream_t st, const uint8_t* (&d)[N]) {
    static_assert(N <= plan::PACK_PARTS_MAX, "plan::pack_layout holds that many offsets");
    size_t len[N];
    for (size_t i = 0; i < N; i++) len[i] = parts[i].p ? parts[i].bytes : 0;
    const plan::pack_layout L = plan::pack_for(len, N);
    HIPCHK(hipSetDevice(c->device));
    if (int rc = c->grp.d_in.reserve(L.total, L.total / 4)) return rc;
    for (size_t i = 0; i < N; i++) {
        uint8_t* at = c->grp.d_in + L.at[i];
        d[i] = parts[i].p ? at : nullptr;
        if (!len[i]) continue;
        if (parts[i].row) HIPCHK(hipMemcpy2DAsync(at, parts[i].row, parts[i].p, parts[i].pitch, parts[i].row, len[i] / parts[i].row, hipMemcpyHostToDevice, st));
        else HIPCHK(hipMemcpyAsync(at, parts[i].p, len[i], hipMemcpyHostToDevice, st));
    }
    return 0;
}
// offsets: k + 1 entries that never decrease
static bool agg_offsets_ok(const size_t* offsets, size_t k) {
    for (size_t s = 0; s < k; s++)
        if (offsets[s + 1] < offsets[s]) return false;
    return true;
}
// a sequence addressed without an index array is the table itself: it holds offsets[k] positions, or the call is refused with `msg`
static bool table_holds(bool have_idx, const size_t* offsets, size_t k, size_t n_table, const char* msg) {
    if (have_idx || offsets[k] <= n_table) return true;
    g_err = msg;
    return false;
}

constexpr size_t PKTAB_BYTES = 8 * 5 * 64;   // per set: 8 table entries x (X, Y, Z, Z^2, Z^3) x 64 bytes (tools/gen_pkmul_asm.py LANE_BYTES)

// The context's two fork streams (latency-mode batches, fastAggregateVerify's key sum, the window groups of a large MSM, combine's second
// Pippenger), created with the context.  They get the device's HIGHEST stream priority: HIP spreads the streams of one priority over
// GPU_MAX_HW_QUEUES hardware queues in creation order, and a fork stream that lands on the queue of the caller's stream runs strictly in turn with
// it - the forked stages then serialise (measured: the same 64-set call 3.21 or 3.81 ms depending on how many streams the process had created
// before, tests/gpu_probe_ctx.py).  Streams of another priority live on queues of their own, so a caller's (normal-priority) stream never shares
// one with them.  (Creating them lazily, at the first call that forks, was tried and dropped: same-box, the 2^20-point MSM of bench.py's long-lived
// process took 5.2 ms instead of 4.8 with streams created that late - profiles/r06_ab/fork_streams.txt; a stream that is never used costs nothing,
// HIP attaches a hardware queue at first use.)
static bool ensure_side(mi355_bls_ctx* c) {
    if (c->side && c->side2) return true;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;
    for (dev_stream* sp : {&c->side, &c->side2})
        if (!*sp) (void)sp->create(&greatest);
    return c->side != nullptr;         // side2 missing: [r]PK shares the first fork stream
}

// HIP spreads streams over GPU_MAX_HW_QUEUES hardware queues (default 4), and streams that share a queue run strictly in turn: a host
// with many SMALL batches in flight (one context + stream each) gets 1.4 M verifications/s with 4 queues and 2.3 M/s with 8
// (tests/gpu_probe_small.py; more than 8 abort in the runtime).  The variable is read when the HIP runtime initialises.  The library
// does NOT touch the process environment on its own (round 3 did, from a load-time constructor: setenv is not thread-safe, it changed
// queue behaviour for every HIP user of the process, and it silently did nothing when HIP was already up): the host sets
// GPU_MAX_HW_QUEUES=8 itself, or calls this ONCE, from its main thread, before anything initialises HIP.
extern "C" int mi355_bls_recommend_hw_queues(void) {
    const char* no = getenv("MI355_BLS_NO_ENV");
    if (no && no[0] == '1') return 0;                             // the host forbids environment edits
    return setenv("GPU_MAX_HW_QUEUES", "8", 0) == 0 ? 1 : 0;       // 0 = overwrite flag: a value the host has set stays
}

static const char DST_SIG[] = "BLS_SIG_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";   // bls_sig_min_pubkey.nim:31
static const char DST_POP[] = "BLS_POP_BLS12381G2_XMD:SHA-256_SSWU_RO_POP_";   // bls_sig_min_pubkey.nim:32

extern "C" const char* mi355_bls_last_error(void) { return g_err.c_str(); }
// Batches submitted and not yet waited for, over all contexts of the process.  A batch enqueued while this is zero has the chip to itself
// until the host submits another: nothing can run in the shadow of its few-wave kernels, so the fold of the line products takes the
// low-latency form (k_fold on the Fp12 engine: 0.35 ms, 2.4 % more chip time) instead of k_lineprod2 (1.8 ms on 68 waves, least work).  Callers
// that keep several batches in flight (bench.py's three) see the count at 1 or 2 on every submit and keep the throughput form; both forms give
// the same GT bytes.  A heuristic read without a lock - a stale value costs time, never correctness.
static std::atomic<int> g_in_flight{0};
extern "C" int mi355_bls_debug_batches_in_flight(void) { return g_in_flight.load(std::memory_order_relaxed); }
extern "C" int mi355_bls_last_fold_form(mi355_bls_ctx* c) { return c ? c->fold_form : MI355_BLS_ERR_ARG; }

// How this library was built (build.sh passes the three macros to the host compile): "aligned=1 dpp_combine=off stamp=<sha256 of the
// sources>".  aligned=0 means the instruction-alignment post-pass (tools/align_isa.py) was skipped - an 8-byte VALU stream then issues
// ~23 % slower - which build.sh only does when BLS_NO_ALIGN=1 asks for it; bench.py prints the string with its numbers.
#ifndef BLS_BUILD_ALIGNED
#define BLS_BUILD_ALIGNED -1
#endif
#ifndef BLS_BUILD_STAMP
#define BLS_BUILD_STAMP "unknown"
#endif
#define BLS_STR2(x) #x
#define BLS_STR(x) BLS_STR2(x)
extern "C" const char* mi355_bls_build_info(void) { return "aligned=" BLS_STR(BLS_BUILD_ALIGNED) " dpp_combine=off stamp=" BLS_BUILD_STAMP; }

extern "C" int mi355_bls_debug_live_resources(void) { return g_live_resources.load(std::memory_order_relaxed); }
extern "C" void mi355_bls_ctx_destroy(mi355_bls_ctx* c) {
    if (!c) return;
    if (c->pending) g_in_flight.fetch_sub(1, std::memory_order_relaxed);      // destroyed with a batch submitted and never waited for
    delete c;
}

// everything of ctx_create that can fail after the context object exists: any failure destroys it (no leaked device buffers)
static int ctx_build(mi355_bls_ctx* c, int device, size_t max_sets) {
    c->device = device;
    c->cap = max_sets;
    c->cap_io = max_sets;
    std::memset(&c->dst, 0, sizeof(c->dst));
    c->dst.len = sizeof(DST_SIG) - 1;
    std::memcpy(c->dst.b, DST_SIG, c->dst.len);
    c->xmd = xmd32_precompute(c->dst.b, c->dst.len);
    std::memset(&c->dst_pop, 0, sizeof(c->dst_pop));
    c->dst_pop.len = sizeof(DST_POP) - 1;
    std::memcpy(c->dst_pop.b, DST_POP, c->dst_pop.len);
    c->xmd_pop = xmd48_precompute(c->dst_pop.b, c->dst_pop.len);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    c->slots = 4u * (uint32_t)prop.multiProcessorCount;
    const plan::ctx_sizes sz = plan::ctx_for(c->slots, max_sets);
    c->stride = sz.stride;                         // tuple pairs + the extra pair(s) of the signature side
    c->nblk_cap = sz.nblk_cap;
    c->mstride = sz.mstride;
    int rc = 0;                                    // the first failure: nothing is created behind it
    const auto alloc = [&rc](auto& buf, size_t bytes) { rc = rc ? rc : buf.alloc(bytes); };
    alloc(c->d_sets, max_sets * plan::ROW_BYTES);   // records, or rows of staging columns (plan.hpp cols)
    alloc(c->d_rnd, 32);
    alloc(c->d_r, c->stride * 8);
    alloc(c->d_H, c->stride * 6 * 64);
    alloc(c->d_M, c->mstride * 6 * 64);
    alloc(c->d_P, c->stride * 3 * 64);
    alloc(c->d_lines, c->stride * 6 * 64 * (size_t)N_LINES);
    alloc(c->d_pktab, max_sets * PKTAB_BYTES);
    alloc(c->d_sig_pts, max_sets * 4 * FPW * 4);
    alloc(c->d_sig_sorted, max_sets * 16 * 4);
    alloc(c->d_sig_hist, 3 * SIG_SLOTS_MAX * 4);
    alloc(c->d_sig_consts, 2 * SIG_SLOTS_MAX * G1W * 4);
    alloc(c->d_agg, 288);
    alloc(c->d_agg1, 144);
    alloc(c->d_msg, 4096 + 192 + 64 + 288);      // message | affine signature | pad | Jacobian signature (AggregateSignature overloads)
    alloc(c->d_comp, max_sets * plan::ROW_BYTES);   // rows of staging columns
    alloc(c->d_status, max_sets);
    alloc(c->d_lpart, sz.lpart_words * 4);         // per-lane partial products of k_lineprod (+ k_fold's first-level results)
    alloc(c->d_L, (size_t)N_LINES * F12W * 4);
    alloc(c->d_states, 64 * 576);
    alloc(c->d_gt, 576);
    alloc(c->d_gt_fv, 576);
    alloc(c->d_carry, 64);
    alloc(c->d_blob, MI355_BLS_BLOB_BYTES);
    alloc(c->d_flags, 16);
    alloc(c->d_export, sz.export_bytes);
    if (rc) return rc;
    c->d_blob_out = c->d_blob;
    (void)ensure_side(c);                          // the fork streams (a context without them still works: nothing forks)
    rc = c->h_flags.alloc(1024);                   // words 0..3 flags, 4..11 staging copy of rnd, 16..159 shard state
    for (auto& e : c->ev) rc = rc ? rc : e.create();
    for (dev_event* e : {&c->ev_hm, &c->ev_lp, &c->ev_s0, &c->ev_l0, &c->ev_deser0, &c->ev_deser1}) rc = rc ? rc : e->create();
    if (rc) return rc;
    k_sig_consts<<<plan::waves_for(256), WAVE>>>(4, 256, c->d_sig_consts);
    k_sig_consts<<<plan::waves_for(2048), WAVE>>>(8, 2048, c->d_sig_consts + (size_t)SIG_SLOTS_MAX * G1W);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    return 0;
}

extern "C" int mi355_bls_ctx_create(mi355_bls_ctx** out, int device, size_t max_sets) {
    if (!out || max_sets == 0 || max_sets > (1u << 30)) return MI355_BLS_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) {
        g_err = "no such HIP device";
        return MI355_BLS_ERR_HIP;
    }
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<mi355_bls_ctx> c(new mi355_bls_ctx());
    int rc = ctx_build(c.get(), device, max_sets);
    if (rc) return rc;                             // the context goes, with whatever it had got; g_err stays
    *out = c.release();
    return 0;
}

// The staging buffers of the entry points around the batch path (wire-format arrays, keys of fastAggregateVerify, the records
// fromBytes writes, combine's inputs and scalars) grow on demand: like the reference's procs, which take any openArray, no entry
// point refuses an input for its size.  (The pipeline workspace itself stays at max_sets: larger batches are sliced, run_shard.)
static int io_reserve(mi355_bls_ctx* c, size_t n) {
    if (n <= c->cap_io) return 0;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    size_t want = n + n / 4;
    HIPCHK(hipSetDevice(c->device));
    // the new buffers first, in locals: if one allocation fails the context keeps its old buffers and capacity (entry points that take
    // device-resident input never come through here and would otherwise launch on null pointers)
    dev_buf<uint8_t> sets, comp, status;
    dev_buf<uint64_t> r;
    int rc = sets.alloc(want * plan::ROW_BYTES);
    if (!rc) rc = comp.alloc(want * plan::ROW_BYTES);
    if (!rc) rc = status.alloc(want);
    if (!rc) rc = r.alloc((want > c->stride ? want : c->stride) * 8);
    if (rc) return rc;
    // only this context's own work can still read the old buffers, and no call is pending (checked above; blocking calls return after
    // their stream has drained): the fork stream and the stream of the last call are waited for, never the whole device (other
    // contexts keep running)
    // (pending_stream is cleared by every wait: a handle kept from an earlier call may belong to a stream the host has destroyed since)
    if (c->side) HIPCHK(hipStreamSynchronize(c->side));
    if (c->side2) HIPCHK(hipStreamSynchronize(c->side2));
    if (c->pending_stream) HIPCHK(hipStreamSynchronize(c->pending_stream));
    c->d_sets.swap(sets), c->d_comp.swap(comp), c->d_status.swap(status), c->d_r.swap(r);      // the old ones go with the locals
    c->cap_io = want;
    return 0;
}
// where a column of the staging layout (plan.hpp cols) starts: it moves whenever io_reserve grows the buffers, so it is asked for after that
static uint8_t* col_at(const mi355_bls_ctx* c, plan::row_col col) { return (col.buf == plan::ROW_SETS ? c->d_sets : c->d_comp) + c->cap_io * col.start; }
// The status pass a per-row call ends in, on `st`: [ev0,] the flag words cleared, what `enqueue` launches, [ev1,] then d_flags, `bytes` from d_also to `also`
// and the n status bytes (each where the caller asked) to the host, and the stream drained.  1: every row's status is 0; 0: some row failed; < 0: an error.
template <class Enqueue>
static int status_pass(mi355_bls_ctx* c, hipStream_t st, size_t n, uint8_t* status, hipEvent_t ev0, hipEvent_t ev1, Enqueue enqueue, void* also = nullptr,
                       const void* d_also = nullptr, size_t bytes = 0) {
    if (ev0) HIPCHK(hipEventRecord(ev0, st));
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 12, st));
    enqueue();
    HIPCHK(hipGetLastError());
    if (ev1) HIPCHK(hipEventRecord(ev1, st));
    uint32_t fl[4];
    HIPCHK(hipMemcpyAsync(fl, c->d_flags, 16, hipMemcpyDeviceToHost, st));
    if (also) HIPCHK(hipMemcpyAsync(also, d_also, bytes, hipMemcpyDeviceToHost, st));
    if (status) HIPCHK(hipMemcpyAsync(status, c->d_status, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return fl[2] ? 0 : 1;
}
// the timings of a call that was one stage, between ev[0] and ev[1], and is waited for: the stage in slot 0 and the total, 0 elsewhere; rc: the stage's result
static int one_stage_timings(mi355_bls_ctx* c, int rc = 0) {
    if (rc < 0) return rc;
    for (int i = 0; i < 8; i++) c->timings[i] = 0;
    HIPCHK(hipEventElapsedTime(&c->timings[0], c->ev[0], c->ev[1]));
    c->timings[7] = c->timings[0];
    return rc;
}

// 320-byte records -> d_M: the two mapped points of every message (two lanes per message)
// pop (here and in every routine below that takes it): the records are popVerify's, key | unused | proof - the message of record i is its own
// key in compressed form, hashed under DST_POP.  Same plan, same grids: the PoP kernels are the same bodies with another message source.
static void launch_hash_map(mi355_bls_ctx* c, const uint8_t* d_sets, uint32_t n32, hipStream_t st, bool pop = false) {
    const plan::hash_map_plan p = plan::hash_map_for(c->slots, c->coop, n32);
    if (pop) {
        switch (p.form) {
            case plan::HASH_MAP_ROWS: k_hash_map_rows_pop<<<p.grid, WAVE, 0, st>>>(d_sets, n32, c->dst_pop, c->xmd_pop, c->d_M, c->mstride); break;
            case plan::HASH_MAP_SPREAD: k_hash_map_spread_pop<<<p.grid, WAVE, 0, st>>>(d_sets, n32, c->dst_pop, c->xmd_pop, c->d_M, c->mstride); break;
            case plan::HASH_MAP_PLAIN: k_hash_map_pop<<<p.grid, WAVE, 0, st>>>(d_sets, n32, c->dst_pop, c->xmd_pop, c->d_M, c->mstride); break;
        }
        return;
    }
    switch (p.form) {
        case plan::HASH_MAP_ROWS: k_hash_map_rows<<<p.grid, WAVE, 0, st>>>(d_sets, n32, c->dst, c->xmd, c->d_M, c->mstride); break;
        case plan::HASH_MAP_SPREAD: k_hash_map_spread<<<p.grid, WAVE, 0, st>>>(d_sets, n32, c->dst, c->xmd, c->d_M, c->mstride); break;
        case plan::HASH_MAP_PLAIN: k_hash_map<<<p.grid, WAVE, 0, st>>>(d_sets, n32, c->dst, c->xmd, c->d_M, c->mstride); break;
    }
}
// d_M (two mapped points per message) -> ps.H = H(m_i): the engine, then the (all but always idle) pass that recomputes a message whose
// incomplete additions met an exceptional case; or k_hash_clear
static void launch_hash_clear(mi355_bls_ctx* c, const pair_store& ps, uint32_t n32, hipStream_t st) {
    const plan::stage p = plan::clear_for(c->slots, c->coop, n32);
    if (p.team) {
        switch (p.form) {       // the lane-team engine (16 lanes per message, csrc/teamvm.hpp)
            case plan::TEAM_ROWS: k_team_clear_rows<<<p.grid, 256, 0, st>>>(c->d_M, c->mstride, n32, ps.H, ps.stride); break;
            case plan::TEAM_ROWS2: k_team_clear_rows2<<<p.grid, 256, 0, st>>>(c->d_M, c->mstride, n32, ps.H, ps.stride); break;
            case plan::TEAM_SPREAD: k_team_clear_spread<<<p.grid, WAVE, 0, st>>>(c->d_M, c->mstride, n32, ps.H, ps.stride); break;      // one wave per SIMD (see the kernel)
            case plan::TEAM_WIDE: k_team_clear<<<p.grid, WAVE, 0, st>>>(c->d_M, c->mstride, n32, ps.H, ps.stride); break;
        }
        k_clear_fix<<<plan::waves_for(n32), WAVE, 0, st>>>(c->d_M, c->mstride, n32, ps.H, ps.stride);
    } else {
        k_hash_clear<<<p.grid, WAVE, 0, st>>>(c->d_M, c->mstride, n32, ps.H, ps.stride, ps.lines);
    }
}

// TEST HOOK: out[i] = clear_cofactor(q0_i + q1_i) for n pairs of blst_p2 images in HOST memory, through the kernels of the batch path themselves
// (same launch shapes): k_hash_clear on a throughput-mode context, the lane-team engine (k_team_clear + k_clear_fix) on a latency-mode one -
// lets the tests put points through them that no hash produces
extern "C" int mi355_bls_debug_g2_clear_cofactor(mi355_bls_ctx* c, const uint8_t* in_pairs, size_t n, uint8_t* out_p2) {
    if (!c || !in_pairs || !out_p2 || n == 0 || n > c->cap) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    dev_buf<uint32_t> d_in;
    if (int rc = d_in.alloc(n * 576)) return rc;
    HIPCHK(hipMemcpy(d_in, in_pairs, n * 576, hipMemcpyHostToDevice));
    const pair_store ps = c->batch_pairs();
    const uint32_t n32 = (uint32_t)n;
    k_debug_to_soa<<<plan::waves_for(2 * n32), WAVE>>>(d_in, 2 * n32, c->d_M, c->mstride);
    launch_hash_clear(c, ps, n32, nullptr);                       // the kernels the batch path would launch for this context and size
    k_export_g2<<<plan::waves_for(n32), WAVE>>>(ps.H, ps.stride, n32, c->d_export);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out_p2, c->d_export, n * 288, hipMemcpyDeviceToHost));      // blocking: d_in is idle when it goes
    return 0;
}

// TEST HOOK: out = hash_to_G2(msg, dst) as a blst_p2 image (Jacobian, 288 B), computed by k_hash_one - the one-message kernel of fastAggregateVerify /
// verify (two SSWU maps side by side, the addition and the cofactor clearing on the lane-team engine) - under ANY domain separation tag: lets the
// tests hold the device against published hash-to-curve vectors, whose DST is not the signature scheme's.
extern "C" int mi355_bls_debug_hash_to_g2(mi355_bls_ctx* c, const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, uint8_t out_p2[288]) {
    if (!c || (!msg && msg_len) || !dst || dst_len == 0 || dst_len > 64 || msg_len > 4096 || !out_p2) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    dst_t d;
    std::memset(&d, 0, sizeof(d));
    d.len = (uint32_t)dst_len;
    std::memcpy(d.b, dst, dst_len);
    const xmd32_consts xc = xmd32_precompute(d.b, d.len);
    if (msg_len) HIPCHK(hipMemcpy(c->d_msg, msg, msg_len, hipMemcpyHostToDevice));
    const pair_store ps = c->batch_pairs();
    k_hash_one<<<1, 256>>>(c->d_msg, (uint32_t)msg_len, d, xc, ps.H, ps.stride, 0);
    k_export_g2<<<1, 64>>>(ps.H, ps.stride, 1, c->d_export);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out_p2, c->d_export, 288, hipMemcpyDeviceToHost));
    return 0;
}

// TEST HOOK: out[i] = op(a[i], b[i]) on raw fp images (14 words each, host memory) through the device's own arithmetic bodies: k_debug_fp_lane for the
// lane operations, k_debug_fp_rows for the DPP row forms (see the header for the codes and FP_DOT2's two images per operand)
extern "C" int mi355_bls_debug_fp_op(mi355_bls_ctx* c, int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out) {
    if (!c || !a || !b || !out || n == 0 || n > c->cap) return MI355_BLS_ERR_ARG;
    const bool lane = op >= MI355_BLS_FPOP_FP_MUL && op <= MI355_BLS_FPOP_PRED, rows = op >= MI355_BLS_FPOP_ROW_MUL && op <= MI355_BLS_FPOP_POW_TWO_ROWS;
    if (!lane && !rows) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const size_t in_bytes = n * FP_N * 4 * (op == MI355_BLS_FPOP_FP_DOT2 ? 2 : 1), out_bytes = n * FP_N * 4;
    dev_buf<uint32_t> d_a, d_b, d_out;
    if (int rc = d_a.alloc(in_bytes)) return rc;
    if (int rc = d_b.alloc(in_bytes)) return rc;
    if (int rc = d_out.alloc(out_bytes)) return rc;
    HIPCHK(hipMemcpy(d_a, a, in_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_b, b, in_bytes, hipMemcpyHostToDevice));
    const uint32_t n32 = (uint32_t)n;
    if (lane)
        k_debug_fp_lane<<<plan::waves_for(n32), WAVE>>>(op, d_a, d_b, n32, d_out);
    else
        k_debug_fp_rows<<<op == MI355_BLS_FPOP_POW_TWO_ROWS ? (n32 + 1) / 2 : (n32 + 3) / 4, WAVE>>>(op, d_a, d_b, n32, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));             // blocking: the buffers are idle when they go
    return 0;
}

// TEST HOOK: n pairs (u0, u1) of Fp2 elements as raw images -> the 2n mapped points iso3(sswu(u)) (Jacobian blst_p2 images), through the map's body in
// the form the batch path would launch for this context and n: hash_map_for's plan and grid, the kernels' launch bounds, d_M as the destination
extern "C" int mi355_bls_debug_map_to_g2(mi355_bls_ctx* c, const uint32_t* us, size_t n, uint8_t* out_p2) {
    if (!c || !us || !out_p2 || n == 0 || n > c->cap) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    std::vector<uint8_t> rec(n * 320, 0);                                        // a "record" per message, as hash_map_body addresses them: the four images, then padding
    for (size_t i = 0; i < n; i++) std::memcpy(rec.data() + i * 320, us + i * 4 * FP_N, 4 * FP_N * 4);
    dev_buf<uint8_t> d_us;
    dev_buf<uint32_t> d_out;
    if (int rc = d_us.alloc(n * 320)) return rc;
    if (int rc = d_out.alloc(2 * n * 288)) return rc;
    HIPCHK(hipMemcpy(d_us, rec.data(), n * 320, hipMemcpyHostToDevice));
    const uint32_t n32 = (uint32_t)n;
    const plan::hash_map_plan p = plan::hash_map_for(c->slots, c->coop, n32);
    switch (p.form) {
        case plan::HASH_MAP_ROWS: k_debug_map_rows<<<p.grid, WAVE>>>(d_us, n32, c->d_M, c->mstride); break;
        case plan::HASH_MAP_SPREAD: k_debug_map_spread<<<p.grid, WAVE>>>(d_us, n32, c->d_M, c->mstride); break;
        case plan::HASH_MAP_PLAIN: k_debug_map<<<p.grid, WAVE>>>(d_us, n32, c->d_M, c->mstride); break;
    }
    k_export_g2<<<plan::waves_for(2 * n32), WAVE>>>(c->d_M, c->mstride, 2 * n32, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out_p2, d_out, 2 * n * 288, hipMemcpyDeviceToHost));        // blocking, as above
    return 0;
}

extern "C" int mi355_bls_ctx_set_num_threads(mi355_bls_ctx* c, uint32_t nt) {
    if (!c || nt == 0) return MI355_BLS_ERR_ARG;
    c->num_threads = nt;
    return 0;
}

extern "C" int mi355_bls_ctx_set_cooperative(mi355_bls_ctx* c, int on) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->coop = on != 0;
    return 0;
}

extern "C" void mi355_bls_chunk_range(size_t n_total, uint32_t num_threads, uint32_t lo, uint32_t hi, size_t* first, size_t* count) {
    size_t B = n_total < num_threads ? n_total : num_threads;
    if (B == 0 || lo >= hi) {
        *first = 0;
        *count = 0;
        return;
    }
    if (hi > B) hi = (uint32_t)B;
    size_t base = n_total / B, rem = n_total % B;
    auto off = [&](size_t c) { return c < rem ? (base + 1) * c : base * c + rem; };
    *first = off(lo);
    *count = off(hi) - off(lo);      // off(B) == n_total
}

// The two inherently serial SHA-256 chains of the reference run on the HOST (one GPU lane needs ~4 us per compression:
// 65 536 links = a quarter of a second; one CPU core does them in a few milliseconds):
//   batchVerifySerial's single blinding chain (core :502-505, :545-556): seed = SHA256(rnd), then per tuple
//   seed <- SHA256(seed) until the low u64 is non-zero;
//   combine's chain (core :588-606): seeded with rnd itself, u64 words 3,2,1,0 of every digest, zeros skipped.
static void host_sha256_32(const uint32_t (&in)[8], uint32_t (&out)[8]) {        // SHA-256 of 32 bytes given as 8 big-endian words
    uint32_t w[16] = {in[0], in[1], in[2], in[3], in[4], in[5], in[6], in[7], 0x80000000u, 0, 0, 0, 0, 0, 0, 256};
    sha256_init(out);
    sha256_compress_core(out, w);
}
static void host_serial_chain(const uint8_t rnd[32], size_t n, uint64_t* out) {
    uint32_t seed[8], nx[8];
    for (int i = 0; i < 8; i++) nx[i] = ((uint32_t)rnd[4 * i] << 24) | ((uint32_t)rnd[4 * i + 1] << 16) | ((uint32_t)rnd[4 * i + 2] << 8) | rnd[4 * i + 3];
    host_sha256_32(nx, seed);
    for (size_t j = 0; j < n; j++) {
        uint64_t r;
        do {
            host_sha256_32(seed, nx);
            for (int i = 0; i < 8; i++) seed[i] = nx[i];
            r = digest_low_u64_le(seed);
        } while (r == 0);
        out[j] = r;
    }
}
static void host_combine_chain(const uint8_t rnd[32], size_t n, uint64_t* out) {
    uint32_t seed[8], nx[8];
    for (int i = 0; i < 8; i++) seed[i] = ((uint32_t)rnd[4 * i] << 24) | ((uint32_t)rnd[4 * i + 1] << 16) | ((uint32_t)rnd[4 * i + 2] << 8) | rnd[4 * i + 3];
    int avail = 0;
    for (size_t i = 0; i < n; i++) {
        for (;;) {
            if (avail == 0) {
                host_sha256_32(seed, nx);
                for (int j = 0; j < 8; j++) seed[j] = nx[j];
                avail = 4;
            }
            avail--;
            uint64_t w = (uint64_t)bswap32(seed[2 * avail]) | ((uint64_t)bswap32(seed[2 * avail + 1]) << 32);   // LE u64 word `avail`
            if (w != 0) {
                out[i] = w;
                break;
            }
        }
    }
}

// k_tail for this context: latency mode takes the form with the cyclotomic squarings on row arithmetic (five waves), throughput mode the engine's three
static inline void launch_k_tail(const mi355_bls_ctx* c, hipStream_t st, const uint32_t* L, uint32_t* states, uint32_t kk, int mode, uint32_t* gt_out,
                                 uint32_t* verdict, uint32_t sstride, int blob) {
    if (c->coop) k_tail_rows<<<1, K_TAIL_THREADS, 0, st>>>(L, states, kk, mode, gt_out, verdict, sstride, blob);
    else k_tail<<<1, TAIL_THREADS, 0, st>>>(L, states, kk, mode, gt_out, verdict, sstride, blob);
}
// the Miller lines of pairs first .. first + count - 1 as `t` says: on the lane-team engine or one lane each (k_lines)
static void launch_lines_at(const pair_store& ps, const plan::stage& t, uint32_t first, uint32_t count, hipStream_t st) {
    if (!t.team) {
        k_lines<<<t.grid, WAVE, 0, st>>>(ps.P, ps.H, first, count, ps.stride, ps.lines);
        return;
    }
    switch (t.form) {
        case plan::TEAM_ROWS: k_team_lines_rows<<<t.grid, 256, 0, st>>>(ps.P, ps.H, first, count, ps.stride, ps.lines); break;
        case plan::TEAM_ROWS2: k_team_lines_rows2<<<t.grid, 256, 0, st>>>(ps.P, ps.H, first, count, ps.stride, ps.lines); break;
        case plan::TEAM_SPREAD: k_team_lines_spread<<<t.grid, WAVE, 0, st>>>(ps.P, ps.H, first, count, ps.stride, ps.lines); break;
        case plan::TEAM_WIDE: k_team_lines<<<t.grid, WAVE, 0, st>>>(ps.P, ps.H, first, count, ps.stride, ps.lines); break;
    }
}
// pairs 0 .. main_pairs - 1, then the extra pairs behind them where the plan gives them a form of their own (plan.hpp lines_for)
static void launch_lines(const pair_store& ps, const plan::lines_plan& p, hipStream_t st) {
    launch_lines_at(ps, p.main, 0, p.main_pairs, st);
    if (p.extra_pairs) launch_lines_at(ps, p.extra, p.main_pairs, p.extra_pairs, st);
}

// The per-step products of the Miller lines of pairs 0 .. npairs-1 -> d_L (68 step products).  mid_ev: recorded between the wide
// kernel and the fold of its partials.
static int enqueue_line_products(mi355_bls_ctx* c, const pair_store& ps, uint32_t npairs, hipStream_t st, hipEvent_t mid_ev) {
    c->fold_form = (c->coop || c->alone) ? 1 : 0;
    const plan::lineprod_plan p = plan::lineprod_for(c->slots, c->nblk_cap, ps.stride, npairs, c->fold_form != 0);
    // every lane hands its partial product over (64 x nblk per step); what folds them: plan.hpp lineprod_for
    k_lineprod<<<dim3(N_LINES, p.nblk), WAVE, 0, st>>>(ps.lines, npairs, ps.stride, p.m, c->d_lpart, p.nblk, p.per_lane);
    if (mid_ev) HIPCHK(hipEventRecord(mid_ev, st));
    if (c->fold_form) {
        uint32_t* mid = c->d_lpart + plan::lpart_mid_words(c->nblk_cap);
        k_fold<<<dim3(N_LINES, p.nb1), TAIL_THREADS, 0, st>>>(c->d_lpart, p.nblk * WAVE, p.per, p.live - (p.nb1 - 1) * p.per, p.nb1 > 1 ? mid : c->d_L);
        if (p.nb1 > 1) k_fold<<<dim3(N_LINES, 1), TAIL_THREADS, 0, st>>>(mid, p.nb1, p.nb1, p.nb1, c->d_L);
    } else {
        k_lineprod2<<<N_LINES, WAVE, 0, st>>>(c->d_lpart, p.nblk * WAVE, c->d_L);
    }
    return 0;
}

// Enqueues everything up to the committed state (d_states slot 0) of ONE SLICE of a shard: tuples [tuple_base, tuple_base + n) of the
// global batch, n <= capacity, records at d_sets (device memory).  chunk_lo / chunk_cnt: the blinding chains that overlap the slice.
// The three producers of Miller pairs are independent until the lines: hashing (k_hash_map, k_hash_clear), [r]PK (k_pkmul) and
// the signature side (bucket fold).  A batch that fills the chip runs them one after the other on the caller's stream (each is a
// whole-chip kernel).  A small batch in latency mode runs the last two on the context's side stream beside the hashing: they
// are all latency-bound there (a few waves each), so this takes about a millisecond off the call.
static int run_pairs(mi355_bls_ctx* c, const uint8_t* d_sets, size_t n, hipStream_t st, bool pop = false);
// c: the workspace this slice runs in (the caller's context or one of its lanes); p: the caller's context, which holds what the slices
// of one call share - the random bytes, the carried chain state, the host-computed serial chain.  blind_done (may be null) is
// recorded behind the blinding kernel: the next slice's chains continue from the state this one leaves.
static int run_slice(mi355_bls_ctx* c, mi355_bls_ctx* p, const uint8_t* d_sets, size_t n_total, uint32_t nchunks, uint32_t chunk_lo, uint32_t chunk_cnt,
                     size_t tuple_base, size_t n, int serial, size_t serial_off, uint32_t slice, hipStream_t st, hipEvent_t blind_done, bool pop = false) {
    HIPCHK(hipEventRecord(c->ev[0], st));
    if (serial) {
        HIPCHK(hipMemcpyAsync(c->d_r, p->h_r.data() + serial_off, n * 8, hipMemcpyHostToDevice, st));
    } else {
        k_blind<<<plan::waves_for(chunk_cnt), WAVE, 0, st>>>(p->d_rnd, n_total, nchunks, chunk_lo, chunk_cnt, tuple_base, n, p->d_carry + 8 * (slice & 1),
                                                                p->d_carry + 8 * ((slice + 1) & 1), c->d_r);
    }
    if (blind_done) HIPCHK(hipEventRecord(blind_done, st));
    return run_pairs(c, d_sets, n, st, pop);
}
// Everything behind the blinding scalars (d_r[0 .. n) are ready on `st`): hashing, [r]PK, the signature side, Miller lines, line
// products, the committed state of these n tuples in d_states slot 0.
static int run_pairs(mi355_bls_ctx* c, const uint8_t* d_sets, size_t n, hipStream_t st, bool pop) {
    const uint32_t n32 = (uint32_t)n;
    const pair_store ps = c->batch_pairs();
    HIPCHK(hipEventRecord(c->ev[1], st));
    const plan::slice_plan p = plan::slice_for(c->slots, c->coop, c->coop && ensure_side(c), n);
    const uint32_t nb = p.nb, cw = p.cw, nwin = p.nwin, total = p.total;
    // SIDE_FORK_SIG - a whole-chip batch of ONE caller (latency mode): the signature side and the Miller lines of its extra pairs run on the
    // side stream beside the hashing.  The tuple pairs then fill the chip's wave slots exactly once; behind them the extra pairs
    // would be a second round of waves (or ~1 ms of the 8-lanes-per-pair kernel).  Throughput mode keeps everything on the
    // caller's stream: with several batches in flight the nearly empty second round overlaps other batches' kernels, and
    // folding the 2048 bucket sums further (to 64 per-bit sums, or to one sum per window) so that fewer extra pairs remain was
    // measured SLOWER per pipelined batch (+0.5 ms and +2.5 ms: the fold is a chain of small dependent kernels on the batch's
    // critical path, the 2048 extra pairs are 3 % more of two embarrassingly parallel kernels).
    // SIDE_FORK - round 6: a small batch's [r]PK runs on a fork stream of its OWN, beside the signature side instead of in front of it (they do not
    // depend on each other; in a row they outlasted the hashing they were meant to hide in: 0.75 + 0.8 ms against 0.9 + 0.66), and the
    // Miller lines of the extra pairs follow the signature side on its stream, so that the tuple pairs alone - at 4 096 sets exactly one
    // engine wave per SIMD - are what the caller's stream still has to walk.
    const bool fork = p.side == plan::SIDE_FORK, fork_sig = p.side == plan::SIDE_FORK_SIG;
    const auto stream_of = [&](plan::stream_role r) { return r == plan::STREAM_CALLER ? st : r == plan::STREAM_SIDE2 && c->side2 ? c->side2 : c->side; };
    hipStream_t sd = stream_of(p.pk_stream);                            // [r]PK
    hipStream_t ss = stream_of(p.sig_stream);                           // signature side
    if (fork || fork_sig) HIPCHK(hipStreamWaitEvent(c->side, c->ev[1], 0));
    if (fork && sd != c->side) HIPCHK(hipStreamWaitEvent(sd, c->ev[1], 0));
    // ---- hashing (caller's stream)
    launch_hash_map(c, d_sets, n32, st, pop);
    HIPCHK(hipEventRecord(c->ev_hm, st));
    launch_hash_clear(c, ps, n32, st);
    HIPCHK(hipEventRecord(c->ev[2], st));
    // ---- [r]PK
    if (p.pkmul_spread) k_pkmul_spread<<<nb, WAVE, 0, sd>>>(d_sets, n32, c->d_r, ps.P, ps.stride, c->d_flags, c->d_pktab);      // one wave per SIMD
    else k_pkmul<<<nb, WAVE, 0, sd>>>(d_sets, n32, c->d_r, ps.P, ps.stride, c->d_flags, c->d_pktab);
    HIPCHK(hipEventRecord(c->ev[3], sd));
    // ---- signature side as a bucket fold: sig_slots extra Miller pairs n .. n + sig_slots - 1 (every batch size: for a
    // handful of tuples the 256 nearly empty buckets are still cheaper than one 64-bit G2 multiplication per tuple, which is a
    // 3 ms chain of doublings when nothing hides its latency)
    {
        msm_win W{nwin, cw, 0};
        uint32_t *hist = c->d_sig_hist, *offs = hist + SIG_SLOTS_MAX, *cursor = offs + SIG_SLOTS_MAX;
        HIPCHK(hipEventRecord(c->ev_s0, ss));
        HIPCHK(hipMemsetAsync(hist, 0, (size_t)total * 4, ss));
        k_sig_convert<<<nb, WAVE, 0, ss>>>(d_sets, n32, c->d_sig_pts);
        k_msm_hist<<<dim3(nb, nwin), WAVE, 0, ss>>>(reinterpret_cast<const uint8_t*>(c->d_r.p), 8, n32, W, cw, hist);
        k_msm_scan<<<nwin, WAVE, 0, ss>>>(hist, cw, offs, cursor);
        k_msm_scatter<<<dim3(nb, nwin), WAVE, 0, ss>>>(reinterpret_cast<const uint8_t*>(c->d_r.p), 8, n32, W, cw, cursor, c->d_sig_sorted);
        k_sig_bucket<<<p.bucket_grid, WAVE, 0, ss>>>(c->d_sig_pts, c->d_sig_sorted, offs, hist, n32, cw, p.lshift, total,
                                                     c->d_sig_consts + (cw == 8 ? (size_t)SIG_SLOTS_MAX * G1W : 0), ps.H, ps.P, ps.stride, (size_t)n32);
        c->sig_c = cw;
        c->sig_slots = total;
        c->agg_valid = false;
    }
    // ---- Miller lines and their products per step
    uint32_t npairs = n32 + total;
    // the extra pairs' walk on the signature side's stream, beside the hashing (round 6, on the lane-team engine: 512 waves for 0.35 ms instead of 32
    // one-lane waves for 1.9 ms - the signature side is out of the way 1.4 ms earlier and no longer displaces the waves of [r]PK behind the hashing)
    if (p.extra_apart) launch_lines_at(ps, p.extra_lines, n32, total, ss);
    HIPCHK(hipEventRecord(c->ev[4], ss));
    if (fork) {
        HIPCHK(hipStreamWaitEvent(st, c->ev[4], 0));                    // join: the signature side ...
        HIPCHK(hipStreamWaitEvent(st, c->ev[3], 0));                    // ... and [r]PK
    }
    HIPCHK(hipEventRecord(c->ev_l0, st));
    launch_lines(ps, p.lines, st);                                       // the tuple pairs, and the extra pairs where they did not run apart
    if (fork_sig) HIPCHK(hipStreamWaitEvent(st, c->ev[4], 0));          // join behind the tuple pairs' lines
    HIPCHK(hipEventRecord(c->ev[5], st));
    {
        int rcp = enqueue_line_products(c, ps, npairs, st, c->ev_lp);
        if (rcp) return rcp;
    }
    c->wide_recorded = true;
    HIPCHK(hipEventRecord(c->ev[6], st));
    launch_k_tail(c, st, c->d_L, c->d_states, 1, 1, c->d_gt, c->d_flags + 1, 144, 0);
    HIPCHK(hipEventRecord(c->ev[7], st));
    HIPCHK(hipGetLastError());
    c->last_n = n;
    c->have_gt = false;
    c->gt_is_fv = false;
    return 0;
}

// the internal workspaces of pipelined slices: same device, same capacity, throughput mode (no fork streams: the slices overlap each other)
// Returns the number of lanes usable (0 .. want): a lane is published only when its workspace, its stream and its event all exist,
// and a lane that cannot be created (out of memory: a workspace is ~29 KB per set) is not an error - the slices then run on fewer
// workspaces, down to this context's own (the serial slice loop of round 3).  Negative: the events every sliced call needs failed.
static int ensure_lanes(mi355_bls_ctx* c, int want) {
    for (dev_event* e : {&c->ev_sl0, &c->ev_blind[0], &c->ev_blind[1], &c->ev_blind[2]})
        if (!*e)
            if (int rc = e->create(hipEventDisableTiming)) return rc;
    int have = 0;
    for (int k = 0; k < want && k < 2; k++) {
        if (c->lane[k]) {
            have = k + 1;
            continue;
        }
        mi355_bls_ctx* raw = nullptr;
        dev_stream s;
        dev_event e;
        if (mi355_bls_ctx_create(&raw, c->device, c->cap) != 0) raw = nullptr;
        std::unique_ptr<mi355_bls_ctx> x(raw);
        if (!x || !s.create() || e.create(hipEventDisableTiming) != 0) {
            x.reset();                              // what was made goes with the locals
            (void)hipGetLastError();                // an out-of-memory error is sticky until read
            (void)hipSetDevice(c->device);
            break;
        }
        x->is_lane = true;
        x->coop = false;
        c->lane_st[k] = std::move(s);
        c->lane_ev[k] = std::move(e);
        c->lane[k] = std::move(x);
        have = k + 1;
    }
    return have;
}
// A shard = chunks [chunk_lo, chunk_lo + chunk_cnt) = tuples [tuple_base, tuple_base + n) of the global batch -> committed state in
// d_states slot 0.  The reference's cache holds per-thread pairing contexts only and accepts any input.len
// (bls_batch_verifier.nim:108-119,141); here the workspace is sized for `cap` tuples, so a larger shard is processed in
// ceil(n / cap) balanced SLICES on the same stream: every slice commits its own state (its own signature-side pairs folded in),
// the running product is kept in slot 1 (blst_pairing_merge, blst_abi.nim:508), the blinding chain of a chunk that a slice
// boundary cuts is carried over (k_blind).  src_dev: the shard's records in device memory, or src_host: in host memory
// (staged slice by slice through d_sets).  After a sliced call fetch_stage(0..3) shows the LAST slice.
static int run_shard(mi355_bls_ctx* c, const uint8_t* src_dev, const uint8_t* src_host, size_t n_total, uint32_t nchunks, uint32_t chunk_lo, uint32_t chunk_cnt,
                     size_t tuple_base, size_t n, int serial, const uint8_t rnd[32], hipStream_t st, bool pop = false, const uint64_t* chosen_r = nullptr) {
    (void)chunk_lo; (void)chunk_cnt;
    HIPCHK(hipSetDevice(c->device));
    if (c->fail_next_enqueue) {                                 // test hook: an enqueue failure after earlier shards of a multi-device call went out
        c->fail_next_enqueue = false;
        g_err = "injected enqueue failure (mi355_bls_debug_fail_next_enqueue)";
        return MI355_BLS_ERR_HIP;
    }
    std::memcpy(c->h_flags + 4, rnd, 32);                      // pinned staging: the copy below is then truly asynchronous
    HIPCHK(hipMemcpyAsync(c->d_rnd, c->h_flags + 4, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 12, st));
    if (serial) {
        c->h_r.resize(n);
        if (chosen_r) std::memcpy(c->h_r.data(), chosen_r, n * 8);      // test hook (mi355_bls_debug_batch_verify_scalars): the caller's scalars in the chain's place
        else host_serial_chain(rnd, n, c->h_r.data());
    }
    const size_t nslices = plan::shard_nslices(n, c->cap);
    c->alone = nslices == 1 && g_in_flight.load(std::memory_order_relaxed) == 0;       // slices of one call overlap each other: throughput form
    if (nslices == 1) {
        const uint8_t* d = src_dev ? src_dev : c->d_sets;
        if (!src_dev) HIPCHK(hipMemcpyAsync(c->d_sets, src_host, n * 320, hipMemcpyHostToDevice, st));
        uint32_t c_lo = serial ? 0 : plan::chunk_of_tuple(n_total, nchunks, tuple_base), c_hi = serial ? 1 : plan::chunk_of_tuple(n_total, nchunks, tuple_base + n - 1) + 1;
        return run_slice(c, c, d, n_total, nchunks, c_lo, c_hi - c_lo, tuple_base, n, serial, 0, 0, st, nullptr, pop);
    }
    // ---- several slices: pipelined over the workspaces of this context and of up to two lanes, each on its own stream.  Slice i starts
    // when slice i - 1 (on another workspace) has finished hashing and its public-key multiplications, exactly as bench.py staggers the
    // batches of three callers (`after`): the slices then sit at different stages and the serial tail of one runs beside the wide
    // kernels of another.  What orders them: the blinding chains (a chunk cut by a slice boundary continues from the state the previous
    // slice's k_blind left: ev_blind), and each workspace's own stream.  Every workspace keeps the running product of ITS slices in
    // slot 1 of its d_states; at the end the lanes' products are copied over and multiplied in (an Fp12 product commutes).  The last
    // slice always runs in this context's own workspace, so fetch_stage(0..3) shows it as before.
    int nl = plan::shard_workspaces(nslices);                 // workspaces used, this context's included
    {
        int have = ensure_lanes(c, nl - 1);
        if (have < 0) return have;
        nl = have + 1;                                         // fewer lanes than wanted (memory): fewer slices in flight, down to one after the other
    }
    HIPCHK(hipEventRecord(c->ev_sl0, st));                     // rnd uploaded, flags cleared
    for (int k = 0; k < nl - 1; k++) {
        mi355_bls_ctx* x = c->lane[k].get();
        x->num_threads = c->num_threads;
        x->dst = c->dst;
        x->xmd = c->xmd;
        HIPCHK(hipStreamWaitEvent(c->lane_st[k], c->ev_sl0, 0));
        HIPCHK(hipMemsetAsync(x->d_flags, 0, 12, c->lane_st[k]));
    }
    bool used[3] = {false, false, false};
    mi355_bls_ctx* prev = nullptr;
    size_t done = 0;
    for (uint32_t slice = 0; done < n; slice++) {
        size_t cnt = plan::shard_slice_count(n, done, nslices, slice);              // balanced: never a sliver at the end
        size_t t0 = tuple_base + done;
        uint32_t c_lo = serial ? 0 : plan::chunk_of_tuple(n_total, nchunks, t0), c_hi = serial ? 1 : plan::chunk_of_tuple(n_total, nchunks, t0 + cnt - 1) + 1;
        const int L = plan::shard_workspace_of(nslices, slice, nl);                 // the last slice on this context's own workspace
        mi355_bls_ctx* x = L ? c->lane[L - 1].get() : c;
        hipStream_t sx = L ? c->lane_st[L - 1] : st;
        if (slice) {
            if (!serial) HIPCHK(hipStreamWaitEvent(sx, c->ev_blind[(slice - 1) % 3], 0));       // the chain state this slice continues from
            if (prev != x) HIPCHK(hipStreamWaitEvent(sx, prev->ev[3], 0));                      // stagger: behind the previous slice's hashing and [r]PK
        }
        const uint8_t* d = src_dev ? src_dev + 320 * done : x->d_sets;
        if (!src_dev) HIPCHK(hipMemcpyAsync(x->d_sets, src_host + 320 * done, cnt * 320, hipMemcpyHostToDevice, sx));
        int rc = run_slice(x, c, d, n_total, nchunks, c_lo, c_hi - c_lo, t0, cnt, serial, done, slice, sx, c->ev_blind[slice % 3], pop);
        if (rc) {
            // earlier slices are still running on the lane streams and read the caller's records and this context's chain state: drain
            // them before the error goes back (the caller may free its buffers then); the error of the failed enqueue is what is reported
            std::string keep = g_err;
            for (int k = 0; k < nl - 1; k++) (void)hipStreamSynchronize(c->lane_st[k]);
            (void)hipStreamSynchronize(st);
            g_err = keep;
            return rc;
        }
        k_state_mul<<<1, TAIL_THREADS, 0, sx>>>(x->d_states, 1, used[L] ? 1 : 0, used[L] ? 0 : -1);
        used[L] = true;
        prev = x;
        done += cnt;
    }
    for (int k = 0; k < nl - 1; k++) {
        if (!used[k + 1]) continue;
        mi355_bls_ctx* x = c->lane[k].get();
        HIPCHK(hipEventRecord(c->lane_ev[k], c->lane_st[k]));
        HIPCHK(hipStreamWaitEvent(st, c->lane_ev[k], 0));
        HIPCHK(hipMemcpyAsync(c->d_states + (size_t)(2 + k) * 144, x->d_states + 144, 576, hipMemcpyDeviceToDevice, st));
        k_or_flag<<<1, 1, 0, st>>>(c->d_flags, x->d_flags);                         // an infinity public key in a lane's slice fails the call
        k_state_mul<<<1, TAIL_THREADS, 0, st>>>(c->d_states, 1, 1, 2 + k);
    }
    k_state_mul<<<1, TAIL_THREADS, 0, st>>>(c->d_states, 0, 1, -1);
    HIPCHK(hipGetLastError());
    return 0;
}

static int collect_timings(mi355_bls_ctx* c, int last_ev) {
    for (int i = 0; i < 8; i++) c->timings[i] = 0;
    for (int i = 0; i < 4; i++) c->ktimes[i] = 0;
    if (last_ev == 7) {                           // batch path: per-kernel split of the two-kernel stages
        HIPCHK(hipEventElapsedTime(&c->ktimes[0], c->ev[1], c->ev_hm));
        HIPCHK(hipEventElapsedTime(&c->ktimes[1], c->ev_hm, c->ev[2]));
        HIPCHK(hipEventElapsedTime(&c->ktimes[2], c->ev[5], c->ev_lp));
        HIPCHK(hipEventElapsedTime(&c->ktimes[3], c->ev_lp, c->ev[6]));
    }
    for (int i = 0; i < last_ev; i++) {
        HIPCHK(hipEventElapsedTime(&c->timings[i], c->ev[i], c->ev[i + 1]));
        if (c->timings[i] < 0) c->timings[i] = 0;              // stages that ran side by side on the fork stream
    }
    if (last_ev == 7) {                           // batch path: the signature side and the lines by their own start events (forked calls)
        HIPCHK(hipEventElapsedTime(&c->timings[3], c->ev_s0, c->ev[4]));
        HIPCHK(hipEventElapsedTime(&c->timings[4], c->ev_l0, c->ev[5]));
    }
    HIPCHK(hipEventElapsedTime(&c->timings[7], c->ev[0], c->ev[last_ev]));
    return 0;
}

// Enqueue a whole batch verification (nothing is waited for); the verdict lands in the context's pinned host words.
static int verify_enqueue(mi355_bls_ctx* c, const uint8_t* d_sets, const uint8_t* h_sets, size_t n, const uint8_t rnd[32], int serial, hipStream_t st, bool pop = false,
                          const uint64_t* chosen_r = nullptr) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if ((!d_sets && !h_sets) || n == 0) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    uint32_t B = (uint32_t)(n < c->num_threads ? n : c->num_threads);
    int rc = run_shard(c, d_sets, h_sets, n, B, 0, serial ? 1 : B, 0, n, serial, rnd, st, pop, chosen_r);
    if (rc) return rc;
    launch_k_tail(c, st, c->d_L, c->d_states, 1, 2, c->d_gt, c->d_flags + 1, 144, 0);
    HIPCHK(hipEventRecord(c->ev[8], st));
    HIPCHK(hipMemcpyAsync(c->h_flags, c->d_flags, 8, hipMemcpyDeviceToHost, st));
    c->pending = true;
    g_in_flight.fetch_add(1, std::memory_order_relaxed);
    c->pending_stream = st;
    return 0;
}
static int verify_wait(mi355_bls_ctx* c) {
    if (!c || !c->pending) return MI355_BLS_ERR_ARG;
    c->pending = false;
    g_in_flight.fetch_sub(1, std::memory_order_relaxed);
    HIPCHK(hipSetDevice(c->device));
    {
        hipStream_t ps = c->pending_stream;
        c->pending_stream = nullptr;              // the host may destroy its stream after this call: never keep the handle
        HIPCHK(hipStreamSynchronize(ps));
    }
    c->have_gt = true;
    float fin = 0;
    int rc = collect_timings(c, 7);
    if (rc) return rc;
    HIPCHK(hipEventElapsedTime(&fin, c->ev[7], c->ev[8]));
    c->timings[6] += fin;
    c->timings[7] += fin;
    return (c->h_flags[0] == 0 && c->h_flags[1] == 1) ? 1 : 0;
}
static int verify_common(mi355_bls_ctx* c, const uint8_t* d_sets, const uint8_t* h_sets, size_t n, const uint8_t rnd[32], int serial, hipStream_t st, bool pop = false) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;                      // bls_batch_verifier.nim:137-139, :312-314
    int rc = verify_enqueue(c, d_sets, h_sets, n, rnd, serial, st, pop);
    if (rc) return rc;
    return verify_wait(c);
}

extern "C" int mi355_bls_batch_submit_device(mi355_bls_ctx* c, const void* d_sets, size_t n, const uint8_t rnd[32], void* stream, mi355_bls_ctx* after) {
    if (after && after != c && after->wide_recorded) {
        // software pipelining: this batch starts when `after`'s batch has finished hashing and its public-key multiplications (ev[3]; the best of the
        // stage boundaries tried: 13.3 ms per batch against 13.7 one stage earlier and 17 one later), so the batches in flight sit
        // at different stages and the serial tail of one always runs beside whole-chip kernels of another (batches that
        // start together stay in phase: their tails coincide and leave the chip idle)
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipStreamWaitEvent((hipStream_t)stream, after->ev[3], 0));
    }
    return verify_enqueue(c, (const uint8_t*)d_sets, nullptr, n, rnd, 0, (hipStream_t)stream);
}
extern "C" int mi355_bls_batch_wait(mi355_bls_ctx* c) { return verify_wait(c); }

extern "C" int mi355_bls_batch_verify_device(mi355_bls_ctx* c, const void* d_sets, size_t n, const uint8_t rnd[32], void* stream) {
    return verify_common(c, (const uint8_t*)d_sets, nullptr, n, rnd, 0, (hipStream_t)stream);
}

static int verify_host(mi355_bls_ctx* c, const void* sets, size_t n, const uint8_t rnd[32], int serial) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!sets) return MI355_BLS_ERR_ARG;
    return verify_common(c, nullptr, (const uint8_t*)sets, n, rnd, serial, nullptr);      // staged through d_sets, slice by slice when n exceeds the capacity
}

extern "C" int mi355_bls_batch_verify(mi355_bls_ctx* c, const void* sets, size_t n, const uint8_t rnd[32]) { return verify_host(c, sets, n, rnd, 0); }
extern "C" int mi355_bls_batch_verify_serial(mi355_bls_ctx* c, const void* sets, size_t n, const uint8_t rnd[32]) { return verify_host(c, sets, n, rnd, 1); }

// TEST HOOK: mi355_bls_batch_verify_serial of one slice (1 <= n <= max_sets, host memory) with the blinding scalars r[0 .. n) of the CALLER'S choice where
// that call computes its SHA-256 chain: the serial branch of run_shard / run_slice with h_r filled from r, so the plan, the kernels behind the
// scalars ([r]PK, the signature side's sort and buckets), the forks and the verdict are that call's.  A zero scalar is refused: the chain never
// yields one, and the kernels are not taken outside their contract.
extern "C" int mi355_bls_debug_batch_verify_scalars(mi355_bls_ctx* c, const void* sets, size_t n, const uint64_t r[]) {
    if (!c || !sets || !r || n == 0 || n > c->cap) return MI355_BLS_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (r[i] == 0) return MI355_BLS_ERR_ARG;
    static const uint8_t no_rnd[32] = {0};                               // the serial branch reads no random bytes on the device
    int rc = verify_enqueue(c, nullptr, (const uint8_t*)sets, n, no_rnd, 1, nullptr, false, r);      // refuses a busy context
    if (rc) return rc;
    return verify_wait(c);
}

// ------------------------------------------------------------------------------------------
// batchVerify by message (mi355_bls_batch_verify_by_message): batchVerify's check with batchVerify's scalars, but the sets of a slice that
// share a message are found on the device (csrc/bymsg.hpp) and their blinded keys summed, e([r_1]PK_1, H(m)) e([r_2]PK_2, H(m)) =
// e([r_1]PK_1 + [r_2]PK_2, H(m)): hashing, clearing and the Miller loop run for ONE pair per distinct message.  The signature side is
// run_pairs' own, over all n sets, with its extra pairs behind the k group pairs.  The value after the final exponentiation is the same
// field element, so verdict and fetch_stage(4) are batchVerify's.  Blocking; any n (slices one after the other on this context's own
// workspace, cut where run_shard cuts them; a group that a boundary cuts is two groups).
// ------------------------------------------------------------------------------------------
// the word arrays of the grouping of n sets, in d_bm_work
struct bymsg_arrays {
    uint32_t *slot_of, *rep, *flag, *rank, *gid, *counts, *cursor, *n_inf, *offsets, *members, *reps;
    static size_t words(size_t n) { return 10 * n + 8; }
};
static bymsg_arrays bymsg_view(uint32_t* w, size_t n) {
    bymsg_arrays a;
    a.slot_of = w, a.rep = a.slot_of + n, a.flag = a.rep + n, a.rank = a.flag + n;            // rank: n + 1
    a.gid = a.rank + n + 1;
    a.counts = a.gid + n, a.cursor = a.counts + n + 1, a.n_inf = a.cursor + n + 1;             // counts | cursor | n_inf: cleared together
    a.offsets = a.n_inf + 1, a.members = a.offsets + n + 1, a.reps = a.members + n;           // offsets: n + 1
    return a;
}
static int bymsg_reserve(mi355_bls_ctx* c, size_t n) {
    const size_t tab = (size_t)plan::bymsg_table_slots(n) * 4, work = bymsg_arrays::words(n) * 4, stride = (n + 63) / 64 * 64;
    int rc = c->d_bm_tab.reserve(tab, 0);
    if (!rc) rc = c->d_bm_work.reserve(work, work / 4);
    if (!rc) rc = c->d_bm_P.reserve(stride * 3 * 64, stride * 48);
    if (!rc && !c->ev_bm) rc = c->ev_bm.create(hipEventDisableTiming);
    return rc;
}
// run_pairs' sibling: everything behind the blinding scalars (d_r[0 .. n) ready on `st`) for a slice whose sets are first grouped by message.
// Two host waits: the number of groups k (four bytes; k == n hands the slice to run_pairs itself), and the k + 1 offsets the segmented sum's
// item table is built from (plan.hpp aggsets_fill, as combine_sets builds it) - awaited while the hashing kernels already run.
static int run_pairs_grouped(mi355_bls_ctx* c, const uint8_t* d_sets, size_t n, hipStream_t st) {
    const uint32_t n32 = (uint32_t)n, nb = plan::waves_for(n32);
    if (int rc = bymsg_reserve(c, n)) return rc;
    const bymsg_arrays A = bymsg_view(c->d_bm_work, n);
    const uint32_t* sets32 = reinterpret_cast<const uint32_t*>(d_sets);
    const uint32_t slots = plan::bymsg_table_slots(n);
    // ---- grouping: table, representatives, ranks, counts
    HIPCHK(hipMemsetAsync(c->d_bm_tab, 0xff, (size_t)slots * 4, st));
    HIPCHK(hipMemsetAsync(A.counts, 0, (2 * (n + 1) + 1) * 4, st));
    k_bymsg_insert<<<nb, WAVE, 0, st>>>(sets32, n32, slots, c->d_bm_tab, A.slot_of);
    k_bymsg_flag<<<nb, WAVE, 0, st>>>(c->d_bm_tab, A.slot_of, n32, A.rep, A.flag);
    k_bymsg_scan<<<1, WAVE, 0, st>>>(A.flag, n32, A.rank);
    k_bymsg_group<<<nb, WAVE, 0, st>>>(A.rep, A.rank, A.flag, n32, A.gid, A.counts, A.reps);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_flags + 200, A.rank + n, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const size_t k = c->h_flags[200];
    const uint32_t k32 = (uint32_t)k;
    if (k == 0 || k > n) {
        g_err = "by_message: the grouping returned an impossible group count";
        return MI355_BLS_ERR_HIP;
    }
    c->bm_groups = (int)k;
    const plan::grouped_plan gp = plan::slice_for_grouped(c->slots, c->coop, c->coop && ensure_side(c), n, k);
    if (gp.ordinary) return run_pairs(c, d_sets, n, st);
    // ---- offsets and member lists; the offsets start their way to the host
    k_bymsg_scan<<<1, WAVE, 0, st>>>(A.counts, k32, A.offsets);
    k_bymsg_scatter<<<nb, WAVE, 0, st>>>(A.gid, n32, A.offsets, A.cursor, A.members);
    c->bm_offs.resize(k + 1);
    HIPCHK(hipMemcpyAsync(c->bm_offs.data(), A.offsets, (k + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(c->ev_bm, st));
    if (int rc = c->d_bm_rec.reserve(k * 320, k * 80)) return rc;
    const pair_store ps = c->batch_pairs();
    HIPCHK(hipEventRecord(c->ev[1], st));
    const plan::slice_plan& p = gp.sets;
    const uint32_t cw = p.cw, nwin = p.nwin, total = p.total;
    const bool fork = p.side == plan::SIDE_FORK, fork_sig = p.side == plan::SIDE_FORK_SIG;
    const auto stream_of = [&](plan::stream_role r) { return r == plan::STREAM_CALLER ? st : r == plan::STREAM_SIDE2 && c->side2 ? c->side2 : c->side; };
    hipStream_t sd = stream_of(p.pk_stream);                            // [r]PK and the group sums
    hipStream_t ss = stream_of(p.sig_stream);                           // signature side
    if (fork || fork_sig) HIPCHK(hipStreamWaitEvent(c->side, c->ev[1], 0));
    if (fork && sd != c->side) HIPCHK(hipStreamWaitEvent(sd, c->ev[1], 0));
    // ---- hashing of the k representatives' messages (caller's stream)
    k_combsets_gather<<<plan::gather_blocks_for(k * 80), plan::GATHER_THREADS, 0, st>>>(sets32, n, A.reps, k32, reinterpret_cast<uint32_t*>(c->d_bm_rec.p));
    launch_hash_map(c, c->d_bm_rec, k32, st);
    HIPCHK(hipEventRecord(c->ev_hm, st));
    launch_hash_clear(c, ps, k32, st);
    HIPCHK(hipEventRecord(c->ev[2], st));
    // ---- [r]PK of all n sets into the pass's own buffer
    const size_t P_stride = c->d_bm_P.bytes / (3 * 64);
    if (p.pkmul_spread) k_pkmul_spread<<<nb, WAVE, 0, sd>>>(d_sets, n32, c->d_r, c->d_bm_P, P_stride, c->d_flags, c->d_pktab);
    else k_pkmul<<<nb, WAVE, 0, sd>>>(d_sets, n32, c->d_r, c->d_bm_P, P_stride, c->d_flags, c->d_pktab);
    // ---- signature side: run_pairs' own, its extra pairs at slots k .. k + total
    {
        msm_win W{nwin, cw, 0};
        uint32_t *hist = c->d_sig_hist, *offs = hist + SIG_SLOTS_MAX, *cursor = offs + SIG_SLOTS_MAX;
        HIPCHK(hipEventRecord(c->ev_s0, ss));
        HIPCHK(hipMemsetAsync(hist, 0, (size_t)total * 4, ss));
        k_sig_convert<<<nb, WAVE, 0, ss>>>(d_sets, n32, c->d_sig_pts);
        k_msm_hist<<<dim3(nb, nwin), WAVE, 0, ss>>>(reinterpret_cast<const uint8_t*>(c->d_r.p), 8, n32, W, cw, hist);
        k_msm_scan<<<nwin, WAVE, 0, ss>>>(hist, cw, offs, cursor);
        k_msm_scatter<<<dim3(nb, nwin), WAVE, 0, ss>>>(reinterpret_cast<const uint8_t*>(c->d_r.p), 8, n32, W, cw, cursor, c->d_sig_sorted);
        k_sig_bucket<<<p.bucket_grid, WAVE, 0, ss>>>(c->d_sig_pts, c->d_sig_sorted, offs, hist, n32, cw, p.lshift, total,
                                                     c->d_sig_consts + (cw == 8 ? (size_t)SIG_SLOTS_MAX * G1W : 0), ps.H, ps.P, ps.stride, (size_t)k32);
        c->sig_c = cw;
        c->sig_slots = total;
        c->agg_valid = false;
    }
    if (gp.extra_apart) launch_lines_at(ps, gp.extra_lines, k32, total, ss);
    HIPCHK(hipEventRecord(c->ev[4], ss));
    // ---- the group sums: item table from the offsets (the device is busy meanwhile), levels, finish into pair slots 0 .. k - 1
    HIPCHK(hipEventSynchronize(c->ev_bm));
    {
        std::vector<size_t> offsets(c->bm_offs.begin(), c->bm_offs.end());
        const plan::aggsets_plan ap = offsets[k] == n ? plan::aggsets_measure(offsets.data(), k) : plan::aggsets_plan{};
        if (!ap.ok || ap.items == 0) {
            g_err = "by_message: the grouping returned offsets that do not cover the slice";
            (void)hipStreamSynchronize(sd), (void)hipStreamSynchronize(ss), (void)hipStreamSynchronize(st);
            return MI355_BLS_ERR_HIP;
        }
        c->grp.items.resize(ap.items * 4 + k);
        plan::aggsets_fill(ap, offsets.data(), k, reinterpret_cast<plan::agg_item*>(c->grp.items.data()), c->grp.items.data() + ap.items * 4);
        int rc = c->grp.d_g1_part.reserve(ap.items * (size_t)G1W * 4, ap.items * (size_t)G1W);
        if (!rc) rc = grouped_upload(c, c->grp.items.size() * 4, 0, 0, sd);      // the table alone: this pass has no flag words and no status bytes
        if (rc) {
            (void)hipStreamSynchronize(sd), (void)hipStreamSynchronize(ss), (void)hipStreamSynchronize(st);
            return rc;
        }
        uint32_t* part = c->grp.d_g1_part;
        launch_levels(ap, reinterpret_cast<const uint4*>(c->grp.d_items.p),
                      [&](const uint4* it, uint32_t cnt) { k_bymsg_l0<<<plan::waves_for(cnt), WAVE, 0, sd>>>(it, cnt, c->d_bm_P, P_stride, A.members, part); },
                      [&](const uint4* it, uint32_t cnt) { k_aggsets_ln<<<plan::waves_for(cnt), WAVE, 0, sd>>>(it, cnt, part); });
        k_bymsg_finish<<<gp.grid_k, WAVE, 0, sd>>>(c->grp.d_items + ap.items * 4, k32, c->grp.d_g1_part, ps.P, ps.stride, A.n_inf);
    }
    HIPCHK(hipEventRecord(c->ev[3], sd));
    // ---- Miller lines and their products per step: k + total pairs
    const uint32_t npairs = k32 + total;
    if (fork) {
        HIPCHK(hipStreamWaitEvent(st, c->ev[4], 0));
        HIPCHK(hipStreamWaitEvent(st, c->ev[3], 0));
    }
    HIPCHK(hipEventRecord(c->ev_l0, st));
    launch_lines(ps, gp.lines, st);
    if (fork_sig) HIPCHK(hipStreamWaitEvent(st, c->ev[4], 0));
    HIPCHK(hipEventRecord(c->ev[5], st));
    if (int rcp = enqueue_line_products(c, ps, npairs, st, c->ev_lp)) return rcp;
    c->wide_recorded = true;
    HIPCHK(hipEventRecord(c->ev[6], st));
    launch_k_tail(c, st, c->d_L, c->d_states, 1, 1, c->d_gt, c->d_flags + 1, 144, 0);
    HIPCHK(hipEventRecord(c->ev[7], st));
    HIPCHK(hipGetLastError());
    c->last_n = n;
    c->last_n.pairs = k;                       // fetch_stage(1 .. 3): k group pairs, the extra pairs behind them
    c->have_gt = false;
    c->gt_is_fv = false;
    return 0;
}
// the whole call: run_shard's preamble and slice cuts, the slices one after the other on this context's workspace, verify_enqueue's end
static int bymsg_verify(mi355_bls_ctx* c, const uint8_t* d_src, const uint8_t* h_src, size_t n, const uint8_t rnd[32], int serial, hipStream_t st,
                        const uint64_t* chosen_r = nullptr) {
    if (!c || !rnd || (!d_src && !h_src) || n == 0) return MI355_BLS_ERR_ARG;
    if ((uintptr_t)d_src & 3) {
        g_err = "by_message: records must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const uint32_t B = (uint32_t)(n < c->num_threads ? n : c->num_threads);
    std::memcpy(c->h_flags + 4, rnd, 32);
    HIPCHK(hipMemcpyAsync(c->d_rnd, c->h_flags + 4, 32, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 12, st));
    if (serial) {
        c->h_r.resize(n);
        if (chosen_r) std::memcpy(c->h_r.data(), chosen_r, n * 8);
        else host_serial_chain(rnd, n, c->h_r.data());
    }
    const size_t nslices = plan::shard_nslices(n, c->cap);
    c->alone = nslices == 1 && g_in_flight.load(std::memory_order_relaxed) == 0;
    size_t done = 0;
    for (uint32_t slice = 0; done < n; slice++) {
        const size_t cnt = plan::shard_slice_count(n, done, nslices, slice);
        const uint32_t c_lo = serial ? 0 : plan::chunk_of_tuple(n, B, done), c_hi = serial ? 1 : plan::chunk_of_tuple(n, B, done + cnt - 1) + 1;
        const uint8_t* d = d_src ? d_src + 320 * done : c->d_sets;
        if (!d_src) HIPCHK(hipMemcpyAsync(c->d_sets, h_src + 320 * done, cnt * 320, hipMemcpyHostToDevice, st));
        HIPCHK(hipEventRecord(c->ev[0], st));
        if (serial) HIPCHK(hipMemcpyAsync(c->d_r, c->h_r.data() + done, cnt * 8, hipMemcpyHostToDevice, st));
        else k_blind<<<plan::waves_for(c_hi - c_lo), WAVE, 0, st>>>(c->d_rnd, n, B, c_lo, c_hi - c_lo, done, cnt, c->d_carry + 8 * (slice & 1), c->d_carry + 8 * ((slice + 1) & 1), c->d_r);
        if (int rc = run_pairs_grouped(c, d, cnt, st)) return rc;
        if (nslices > 1) k_state_mul<<<1, TAIL_THREADS, 0, st>>>(c->d_states, 1, slice ? 1 : 0, slice ? 0 : -1);      // the running product in slot 1
        done += cnt;
    }
    if (nslices > 1) k_state_mul<<<1, TAIL_THREADS, 0, st>>>(c->d_states, 0, 1, -1);
    HIPCHK(hipGetLastError());
    launch_k_tail(c, st, c->d_L, c->d_states, 1, 2, c->d_gt, c->d_flags + 1, 144, 0);
    HIPCHK(hipEventRecord(c->ev[8], st));
    HIPCHK(hipMemcpyAsync(c->h_flags, c->d_flags, 8, hipMemcpyDeviceToHost, st));
    c->pending = true;
    g_in_flight.fetch_add(1, std::memory_order_relaxed);
    c->pending_stream = st;
    return verify_wait(c);
}
extern "C" int mi355_bls_batch_verify_by_message_device(mi355_bls_ctx* c, const void* d_sets, size_t n, const uint8_t rnd[32], void* stream) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;                      // batchVerify's rule
    return bymsg_verify(c, (const uint8_t*)d_sets, nullptr, n, rnd, 0, (hipStream_t)stream);
}
extern "C" int mi355_bls_batch_verify_by_message(mi355_bls_ctx* c, const void* sets, size_t n, const uint8_t rnd[32]) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!sets) return MI355_BLS_ERR_ARG;
    return bymsg_verify(c, nullptr, (const uint8_t*)sets, n, rnd, 0, nullptr);
}
extern "C" int mi355_bls_last_message_groups(mi355_bls_ctx* c) { return c && c->bm_groups >= 0 ? c->bm_groups : MI355_BLS_ERR_ARG; }
// TEST HOOK: mi355_bls_debug_batch_verify_scalars' contract (serial, one slice, host memory, no zero scalar) for the by-message pass
extern "C" int mi355_bls_debug_batch_verify_by_message_scalars(mi355_bls_ctx* c, const void* sets, size_t n, const uint64_t r[]) {
    if (!c || !sets || !r || n == 0 || n > c->cap) return MI355_BLS_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (r[i] == 0) return MI355_BLS_ERR_ARG;
    static const uint8_t no_rnd[32] = {0};
    return bymsg_verify(c, nullptr, (const uint8_t*)sets, n, no_rnd, 1, nullptr, r);
}

// ------------------------------------------------------------------------------------------
// Per-set verdicts: verify (bls_sig_min_pubkey.nim:108-125 -> coreVerifyNoGroupCheck, core :269-297) applied to every set of the input in
// one device pass.  No blinding, no random bytes: verdict i is a function of set i alone.  Any n: slices of at most max_sets sets
// follow each other on the caller's stream (hashing, pair setup, Miller lines of the 2 m pairs in a pair store of the path's own, the
// per-set tail in the form plan::each_for names); the verdict bytes of all slices collect in d_each_v and come back in one copy.
// ------------------------------------------------------------------------------------------
static int each_reserve(mi355_bls_ctx* c, size_t n, bool want_gt) {
    if (int rc = c->d_each_v.reserve(n, n / 4)) return rc;
    if (!c->each_stride) {      // the pair store: all four buffers or none
        const size_t st = plan::each_stride(c->cap);
        dev_buf<uint4> H, P, lines;
        dev_buf<uint32_t> work;
        int rc = H.alloc(st * 6 * 64);
        if (!rc) rc = P.alloc(st * 3 * 64);
        if (!rc) rc = lines.alloc(st * 6 * 64 * (size_t)N_LINES);
        if (!rc) rc = work.alloc((size_t)plan::each_engine_grid_max(c->slots) * EACH_WORK_WORDS * 4);
        if (rc) return rc;
        c->d_each_H = std::move(H), c->d_each_P = std::move(P), c->d_each_lines = std::move(lines), c->d_each_work = std::move(work);
        c->each_stride = st;
    }
    return want_gt ? c->d_each_gt.reserve(n * 576, 0) : 0;
}
static int each_run(mi355_bls_ctx* c, const uint8_t* d_src, const uint8_t* h_src, size_t n, uint8_t verdicts[], uint8_t* gt_out, hipStream_t st, bool pop = false) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;                      // nothing verified, nothing written
    if (!verdicts || (!d_src && !h_src)) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    int rc = each_reserve(c, n, gt_out != nullptr);
    if (rc) return rc;
    const size_t slice_max = plan::each_slice_max(c->cap), nslices = plan::each_nslices(n, slice_max);
    const pair_store ps = c->each_pairs();       // the per-set path's own (2 x cap pairs): the batch workspace keeps what it holds
    HIPCHK(hipEventRecord(c->ev[0], st));
    size_t done = 0;
    for (uint32_t sl = 0; sl < nslices; sl++) {
        const size_t m = plan::each_slice_count(n, done, nslices, sl);
        const uint32_t m32 = (uint32_t)m;
        const uint8_t* src = d_src ? d_src + done * 320 : c->d_sets;
        if (!d_src) HIPCHK(hipMemcpyAsync(c->d_sets, h_src + done * 320, m * 320, hipMemcpyHostToDevice, st));      // behind the last slice's kernels on the same stream
        const plan::each_plan p = plan::each_for(c->slots, c->coop, m32);
        launch_hash_map(c, src, m32, st, pop);                             // H(msg_i) -> pair slot i, in the forms the batch path takes for m messages
        launch_hash_clear(c, ps, m32, st);
        k_each_setup<<<p.setup_grid, WAVE, 0, st>>>(src, m32, ps.H, ps.P, ps.stride);
        launch_lines(ps, p.lines, st);
        uint8_t* dv = c->d_each_v + done;
        uint32_t* dg = gt_out ? c->d_each_gt + done * 144 : nullptr;
        if (!p.tail_engine) k_each_tail<<<p.tail_grid, WAVE, 0, st>>>(ps.lines, ps.stride, m32, src, dv, dg);
        else if (c->coop) k_each_engine_rows<<<p.tail_grid, K_TAIL_THREADS, 0, st>>>(ps.lines, ps.stride, m32, src, dv, dg, c->d_each_work);
        else k_each_engine<<<p.tail_grid, TAIL_THREADS, 0, st>>>(ps.lines, ps.stride, m32, src, dv, dg, c->d_each_work);
        done += m;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[1], st));
    HIPCHK(hipMemcpyAsync(verdicts, c->d_each_v, n, hipMemcpyDeviceToHost, st));
    if (gt_out) HIPCHK(hipMemcpyAsync(gt_out, c->d_each_gt, n * 576, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->each_passes++;
    c->last_n = 0;                             // fetch_stage shows the last call, and this one left no batch stages
    c->sig_slots = 0;
    c->agg_valid = false;
    c->have_gt = false;
    rc = collect_timings(c, 1);
    if (rc) return rc;
    int all = 1;
    for (size_t i = 0; i < n; i++) all &= verdicts[i] == 1;
    return all;
}
extern "C" int mi355_bls_verify_each(mi355_bls_ctx* c, const void* sets, size_t n, uint8_t verdicts[]) {
    return each_run(c, nullptr, (const uint8_t*)sets, n, verdicts, nullptr, nullptr);
}
extern "C" int mi355_bls_verify_each_device(mi355_bls_ctx* c, const void* d_sets, size_t n, uint8_t verdicts[], void* stream) {
    return each_run(c, (const uint8_t*)d_sets, nullptr, n, verdicts, nullptr, (hipStream_t)stream);
}
// TEST HOOKS: the same pass with the 576-byte value of every set (what mi355_bls_fetch_stage(4) is to the batch paths); the number of
// per-set passes this context has made
extern "C" int mi355_bls_debug_verify_each_gt(mi355_bls_ctx* c, const void* sets, size_t n, uint8_t verdicts[], uint8_t* gt_out) {
    if (!gt_out) return MI355_BLS_ERR_ARG;
    return each_run(c, nullptr, (const uint8_t*)sets, n, verdicts, gt_out, nullptr);
}
extern "C" int mi355_bls_debug_verify_each_passes(mi355_bls_ctx* c) { return c ? c->each_passes : MI355_BLS_ERR_ARG; }

// batchVerify first; only a failing batch pays for the per-set pass
static int locate_run(mi355_bls_ctx* c, const uint8_t* d_src, const uint8_t* h_src, size_t n, const uint8_t rnd[32], uint8_t verdicts[], hipStream_t st, bool pop = false) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!verdicts || (!d_src && !h_src)) return MI355_BLS_ERR_ARG;
    int rc = verify_common(c, d_src, h_src, n, rnd, 0, st, pop);
    if (rc < 0) return rc;
    if (rc == 1) {
        std::memset(verdicts, 1, n);
        return 1;
    }
    rc = each_run(c, d_src, h_src, n, verdicts, nullptr, st, pop);
    return rc < 0 ? rc : 0;
}
extern "C" int mi355_bls_batch_verify_locate(mi355_bls_ctx* c, const void* sets, size_t n, const uint8_t rnd[32], uint8_t verdicts[]) {
    return locate_run(c, nullptr, (const uint8_t*)sets, n, rnd, verdicts, nullptr);
}
extern "C" int mi355_bls_batch_verify_locate_device(mi355_bls_ctx* c, const void* d_sets, size_t n, const uint8_t rnd[32], uint8_t verdicts[], void* stream) {
    return locate_run(c, (const uint8_t*)d_sets, nullptr, n, rnd, verdicts, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// popVerify for a table of keys (bls_sig_min_pubkey.nim:60-74: coreVerifyNoGroupCheck(publicKey, compress(publicKey), proof, DST_POP)), the check
// the reference's proof-taking overloads (:104, :148, :220-225) loop over key by key.  n keys and n proofs become n records in the staging
// buffer (k_pop_records); the per-set pass, the blinded batch pass and the locate form then run on them with `pop` set, i.e. with the PoP
// forms of the hash-map kernels and nothing else changed: slicing, stages, verdict bytes as for SignatureSets.
// ------------------------------------------------------------------------------------------
// keys | proofs (host memory when `host`, staged through their columns; else device memory) -> n records at c->d_sets, enqueued on `st`
static int pop_stage(mi355_bls_ctx* c, const void* pks, const void* proofs, size_t n, bool host, hipStream_t st) {
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    if (int rc = io_reserve(c, n)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const uint8_t *dk = (const uint8_t*)pks, *dp = (const uint8_t*)proofs;
    if (host) {
        HIPCHK(hipMemcpyAsync(col_at(c, cols::POP_KEYS), pks, n * 96, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(col_at(c, cols::POP_PROOFS), proofs, n * 192, hipMemcpyHostToDevice, st));
        dk = col_at(c, cols::POP_KEYS), dp = col_at(c, cols::POP_PROOFS);
    }
    k_pop_records<<<plan::pop_records_grid(n), 256, 0, st>>>(reinterpret_cast<const uint32_t*>(dk), reinterpret_cast<const uint32_t*>(dp), n,
                                                             reinterpret_cast<uint32_t*>(c->d_sets.p));
    HIPCHK(hipGetLastError());
    return 0;
}
static int pop_each(mi355_bls_ctx* c, const void* pks, const void* proofs, size_t n, uint8_t verdicts[], uint8_t* gt_out, bool host, hipStream_t st) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;                      // nothing verified, nothing written
    if (!pks || !proofs || !verdicts || n > plan::POP_MAX_KEYS) return MI355_BLS_ERR_ARG;
    if (int rc = pop_stage(c, pks, proofs, n, host, st)) return rc;
    return each_run(c, c->d_sets, nullptr, n, verdicts, gt_out, st, true);
}
static int pop_batch(mi355_bls_ctx* c, const void* pks, const void* proofs, size_t n, const uint8_t rnd[32], uint8_t* verdicts, bool locate, bool host, hipStream_t st) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!pks || !proofs || (locate && !verdicts) || n > plan::POP_MAX_KEYS) return MI355_BLS_ERR_ARG;
    if (int rc = pop_stage(c, pks, proofs, n, host, st)) return rc;
    return locate ? locate_run(c, c->d_sets, nullptr, n, rnd, verdicts, st, true) : verify_common(c, c->d_sets, nullptr, n, rnd, 0, st, true);
}
extern "C" int mi355_bls_pop_verify_each(mi355_bls_ctx* c, const void* pks96, const void* proofs192, size_t n, uint8_t verdicts[]) {
    return pop_each(c, pks96, proofs192, n, verdicts, nullptr, true, nullptr);
}
extern "C" int mi355_bls_pop_verify_each_device(mi355_bls_ctx* c, const void* d_pks96, const void* d_proofs192, size_t n, uint8_t verdicts[], void* stream) {
    return pop_each(c, d_pks96, d_proofs192, n, verdicts, nullptr, false, (hipStream_t)stream);
}
extern "C" int mi355_bls_debug_pop_verify_each_gt(mi355_bls_ctx* c, const void* pks96, const void* proofs192, size_t n, uint8_t verdicts[], uint8_t* gt_out) {
    if (!gt_out) return MI355_BLS_ERR_ARG;
    return pop_each(c, pks96, proofs192, n, verdicts, gt_out, true, nullptr);
}
extern "C" int mi355_bls_batch_pop_verify(mi355_bls_ctx* c, const void* pks96, const void* proofs192, size_t n, const uint8_t rnd[32]) {
    return pop_batch(c, pks96, proofs192, n, rnd, nullptr, false, true, nullptr);
}
extern "C" int mi355_bls_batch_pop_verify_device(mi355_bls_ctx* c, const void* d_pks96, const void* d_proofs192, size_t n, const uint8_t rnd[32], void* stream) {
    return pop_batch(c, d_pks96, d_proofs192, n, rnd, nullptr, false, false, (hipStream_t)stream);
}
extern "C" int mi355_bls_batch_pop_verify_locate(mi355_bls_ctx* c, const void* pks96, const void* proofs192, size_t n, const uint8_t rnd[32], uint8_t verdicts[]) {
    return pop_batch(c, pks96, proofs192, n, rnd, verdicts, true, true, nullptr);
}
extern "C" int mi355_bls_batch_pop_verify_locate_device(mi355_bls_ctx* c, const void* d_pks96, const void* d_proofs192, size_t n, const uint8_t rnd[32],
                                                        uint8_t verdicts[], void* stream) {
    return pop_batch(c, d_pks96, d_proofs192, n, rnd, verdicts, true, false, (hipStream_t)stream);
}
// The two compressors: rawFromPublic / serialize for n keys (bls_sig_io.nim:203-211), serialize for n signatures (:225-234).  The device form leaves the
// bytes in device memory and returns when they are there.  aligned: an input or output off a multiple of 4 bytes is refused (the signatures' is, the keys' not).
template <class In>
static int compress_device(mi355_bls_ctx* c, void (*kernel)(const In*, uint32_t, uint32_t*), bool aligned, const void* d_in, size_t n, void* d_out, hipStream_t st) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!d_in || !d_out || n > plan::POP_MAX_KEYS || (aligned && (((uintptr_t)d_in | (uintptr_t)d_out) & 3))) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    kernel<<<plan::waves_for((uint32_t)n), WAVE, 0, st>>>((const In*)d_in, (uint32_t)n, (uint32_t*)d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
static int compress_host(mi355_bls_ctx* c, int (*device_form)(mi355_bls_ctx*, const void*, size_t, void*, void*), plan::row_col in_col, plan::row_col out_col,
                         const void* in, size_t n, uint8_t* out) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!in || !out || n > plan::POP_MAX_KEYS) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    if (int rc = io_reserve(c, n)) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(col_at(c, in_col), in, n * in_col.width, hipMemcpyHostToDevice, nullptr));
    if (int rc = device_form(c, col_at(c, in_col), n, col_at(c, out_col), nullptr)) return rc;
    HIPCHK(hipMemcpy(out, col_at(c, out_col), n * out_col.width, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int mi355_bls_compress_public_keys_device(mi355_bls_ctx* c, const void* d_pks96, size_t n, void* d_out48, void* stream) {
    return compress_device(c, k_compress_pks, false, d_pks96, n, d_out48, (hipStream_t)stream);
}
extern "C" int mi355_bls_compress_public_keys(mi355_bls_ctx* c, const void* pks96, size_t n, uint8_t out48[]) {
    return compress_host(c, mi355_bls_compress_public_keys_device, cols::CPK_IN, cols::CPK_OUT, pks96, n, out48);
}
extern "C" int mi355_bls_compress_signatures_device(mi355_bls_ctx* c, const void* d_sigs192, size_t n, void* d_out96, void* stream) {
    return compress_device(c, k_compress_sigs, true, d_sigs192, n, d_out96, (hipStream_t)stream);
}
extern "C" int mi355_bls_compress_signatures(mi355_bls_ctx* c, const void* sigs192, size_t n, uint8_t out96[]) {
    return compress_host(c, mi355_bls_compress_signatures_device, cols::CSIG_IN, cols::CSIG_OUT, sigs192, n, out96);
}

// ------------------------------------------------------------------------------------------
// Per-set key aggregation: aggregateAll (blst_min_pubkey_sig_core.nim:179-195) for the key list of every set of a batch in one device pass,
// the step fastAggregateVerify (bls_sig_min_pubkey.nim:234-258) runs in front of its pairing.  k key lists in CSR form (list s = positions
// [offsets[s], offsets[s + 1]) of the key sequence; the sequence is the key table itself, or - with an index array - table entries picked by
// index, so a validator key table can stay on the device) become k ordinary 320-byte SignatureSet records in device memory, which the batch
// and the per-set paths take unchanged.  The host lays the segmented sum out (plan.hpp aggsets_fill: levels of items of up to AGG_C
// operands, no item across two lists) and sends the table with one copy; a kernel per level and k_aggsets_finish follow on the caller's stream.
// ------------------------------------------------------------------------------------------
static_assert(sizeof(plan::agg_item) == 16, "k_aggsets_l0 / k_aggsets_ln load an item as one uint4");
// device addresses of a call's inputs
struct agg_in {
    const uint8_t* keys;
    const uint32_t* idx;
    const uint8_t *msgs, *sigs;
};
// aggregation of k > 0 lists enqueued on st: records at d_out, status bytes in c->grp.d_status
static int aggsets_enqueue(mi355_bls_ctx* c, const agg_in& in, size_t n_table, const size_t* offsets, size_t k, uint8_t* d_out, hipStream_t st) {
    if (!in.keys || !in.msgs || !in.sigs || !offsets || !d_out) return MI355_BLS_ERR_ARG;
    if (((uintptr_t)in.keys | (uintptr_t)in.msgs | (uintptr_t)in.sigs | (uintptr_t)in.idx | (uintptr_t)d_out) & 3) {
        g_err = "aggregate_sets: keys, messages, signatures, indices and records must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const plan::aggsets_plan p = k < plan::AGG_NONE ? plan::aggsets_measure(offsets, k) : plan::aggsets_plan{};
    if (!p.ok) {
        g_err = "aggregate_sets: offsets decrease, or more than 2^32 - 2 keys or lists";
        return MI355_BLS_ERR_ARG;
    }
    if (!table_holds(in.idx, offsets, k, n_table, "aggregate_sets: offsets[k] exceeds the number of keys")) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    c->grp.items.resize(p.items * 4 + k);
    plan::aggsets_fill(p, offsets, k, reinterpret_cast<plan::agg_item*>(c->grp.items.data()), c->grp.items.data() + p.items * 4);
    const size_t pb = (p.items ? p.items : 1) * (size_t)G1W * 4;
    int rc = c->grp.d_g1_part.reserve(pb, pb / 4);
    if (!rc) rc = grouped_upload(c, c->grp.items.size() * 4, k * 4, k, st);
    if (rc) return rc;
    uint32_t* part = c->grp.d_g1_part;
    launch_levels(p, reinterpret_cast<const uint4*>(c->grp.d_items.p),
                  [&](const uint4* it, uint32_t cnt) { k_aggsets_l0<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, in.keys, n_table, in.idx, part, c->grp.d_flag); },
                  [&](const uint4* it, uint32_t cnt) { k_aggsets_ln<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, part); });
    k_aggsets_finish<<<plan::waves_for((uint32_t)k), WAVE, 0, st>>>(c->grp.d_items + p.items * 4, (uint32_t)k, part, c->grp.d_flag,
                                                                   reinterpret_cast<const uint32_t*>(in.msgs), reinterpret_cast<const uint32_t*>(in.sigs),
                                                                   reinterpret_cast<uint32_t*>(d_out), c->grp.d_status);
    HIPCHK(hipGetLastError());
    return 0;
}
// The status bytes back (a grouped call's synchronisation): 1 when every group's is 0.  The chains combine_sets walked on the host are blinding
// material: they are wiped and dropped here, on every way out, so a call that left none (every other feature's) has nothing to fill.
static int grouped_status(mi355_bls_ctx* c, size_t k, uint8_t* status, hipStream_t st) {
    struct wipe {
        std::vector<uint64_t>& v;
        ~wipe() { std::fill(v.begin(), v.end(), 0), v.clear(); }
    } at_return{c->comb_s_h};
    HIPCHK(hipMemcpyAsync(status, c->grp.d_status, k, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int all = 1;
    for (size_t s = 0; s < k; s++) all &= status[s] == 0;
    return all;
}
// What is done with the k records of aggregate_sets, aggregate_sets_bits and combine_sets.  enqueue(d_out, st): the feature's pass, k records to
// d_out on st, status bytes to grp.d_status.
template <class Enqueue>
static int records_enqueue(mi355_bls_ctx* c, size_t k, hipStream_t st, Enqueue enqueue) {
    if (int rc = c->grp.d_rec.reserve(k * 320, k * 80)) return rc;
    return enqueue(c->grp.d_rec.p, st);
}
// the host forms: records and status bytes to the host
template <class Enqueue>
static int records_to_host(mi355_bls_ctx* c, size_t k, void* out_records, uint8_t* status, Enqueue enqueue) {
    if (int rc = records_enqueue(c, k, nullptr, enqueue)) return rc;
    HIPCHK(hipMemcpyAsync(out_records, c->grp.d_rec, k * 320, hipMemcpyDeviceToHost, nullptr));
    return grouped_status(c, k, status, nullptr);
}
// verify (fastAggregateVerify, bls_sig_min_pubkey.nim:234-258) per record: the per-set pass on them.  A group that gave no key (no member, an
// index out of range, the sum at infinity) has the infinity key in its record: verdict 0.
template <class Enqueue>
static int records_each(mi355_bls_ctx* c, size_t k, uint8_t* out, hipStream_t st, Enqueue enqueue) {
    if (int rc = records_enqueue(c, k, st, enqueue)) return rc;
    return each_run(c, c->grp.d_rec, nullptr, k, out, nullptr, st);
}
// batchVerify over the records: a group that gives none (any status but 0) ends the call with 0 before any verification pass - the
// reference's caller would not have obtained a SignatureSet for it.
template <class Enqueue>
static int records_batch(mi355_bls_ctx* c, size_t k, const uint8_t rnd[32], hipStream_t st, Enqueue enqueue) {
    int rc = records_enqueue(c, k, st, enqueue);
    if (rc) return rc;
    c->grp.status_h.resize(k);
    rc = grouped_status(c, k, c->grp.status_h.data(), st);
    if (rc != 1) return rc;
    return verify_common(c, c->grp.d_rec, nullptr, k, rnd, 0, st);
}
// host inputs -> the staged inputs: keys | signatures | messages | indices (every part 4-byte aligned)
static int agg_stage(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k, const void* msgs, size_t msg_bytes,
                     const void* sigs, hipStream_t st, agg_in* out) {
    if (!keys || !offsets || !msgs || !sigs || !agg_offsets_ok(offsets, k)) return MI355_BLS_ERR_ARG;
    const uint8_t* d[4];
    if (int rc = stage_inputs(c, {{keys, n_table * 96}, {sigs, k * 192}, {msgs, msg_bytes}, {idx, offsets[k] * 4}}, st, d)) return rc;
    *out = agg_in{d[0], reinterpret_cast<const uint32_t*>(d[3]), d[2], d[1]};
    return 0;
}
extern "C" int mi355_bls_aggregate_sets_device(mi355_bls_ctx* c, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k,
                                               const void* d_msgs32, const void* d_sigs192, void* d_out_records, uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing aggregated, nothing written
    if (!status) return MI355_BLS_ERR_ARG;
    const agg_in in{(const uint8_t*)d_keys, d_idx, (const uint8_t*)d_msgs32, (const uint8_t*)d_sigs192};
    int rc = aggsets_enqueue(c, in, n_table, offsets, k, (uint8_t*)d_out_records, (hipStream_t)stream);
    if (rc) return rc;
    return grouped_status(c, k, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_aggregate_sets(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                        const void* msgs32, const void* sigs192, void* out_records, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!out_records || !status) return MI355_BLS_ERR_ARG;
    agg_in in;
    if (int rc = agg_stage(c, keys, n_table, idx, offsets, k, msgs32, k * 32, sigs192, nullptr, &in)) return rc;
    return records_to_host(c, k, out_records, status, [&](uint8_t* d_out, hipStream_t st) { return aggsets_enqueue(c, in, n_table, offsets, k, d_out, st); });
}
// fastAggregateVerify for every list (records_each)
extern "C" int mi355_bls_fast_aggregate_verify_each_device(mi355_bls_ctx* c, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                                           size_t k, const void* d_msgs32, const void* d_sigs192, uint8_t* out, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!out) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const agg_in in{(const uint8_t*)d_keys, d_idx, (const uint8_t*)d_msgs32, (const uint8_t*)d_sigs192};
    return records_each(c, k, out, (hipStream_t)stream, [&](uint8_t* d_out, hipStream_t st) { return aggsets_enqueue(c, in, n_table, offsets, k, d_out, st); });
}
extern "C" int mi355_bls_fast_aggregate_verify_each(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                                    const void* msgs32, const void* sigs192, uint8_t* out) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!out) return MI355_BLS_ERR_ARG;
    agg_in in;
    if (int rc = agg_stage(c, keys, n_table, idx, offsets, k, msgs32, k * 32, sigs192, nullptr, &in)) return rc;
    return records_each(c, k, out, nullptr, [&](uint8_t* d_out, hipStream_t st) { return aggsets_enqueue(c, in, n_table, offsets, k, d_out, st); });
}
// batchVerify over the sets (aggregateAll(keys_s), msg_s, sig_s) (records_batch)
extern "C" int mi355_bls_batch_fast_aggregate_verify_device(mi355_bls_ctx* c, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                                            size_t k, const void* d_msgs32, const void* d_sigs192, const uint8_t rnd[32], void* stream) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    const agg_in in{(const uint8_t*)d_keys, d_idx, (const uint8_t*)d_msgs32, (const uint8_t*)d_sigs192};
    return records_batch(c, k, rnd, (hipStream_t)stream, [&](uint8_t* d_out, hipStream_t st) { return aggsets_enqueue(c, in, n_table, offsets, k, d_out, st); });
}
extern "C" int mi355_bls_batch_fast_aggregate_verify(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                                     const void* msgs32, const void* sigs192, const uint8_t rnd[32]) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    agg_in in;
    if (int rc = agg_stage(c, keys, n_table, idx, offsets, k, msgs32, k * 32, sigs192, nullptr, &in)) return rc;
    return records_batch(c, k, rnd, nullptr, [&](uint8_t* d_out, hipStream_t st) { return aggsets_enqueue(c, in, n_table, offsets, k, d_out, st); });
}

// ------------------------------------------------------------------------------------------
// Key aggregation by participation bits: the records of aggregate_sets for k sets given as (committee number, one bit per committee
// position) over m fixed committees - aggregateAll over the keys whose bit is set, or, where the committee's own aggregate is given and more
// than half of it signed, subtractAll (blst_min_pubkey_sig_core.nim:197-209) of the absentees from that aggregate.  The plan (plan.hpp
// aggbits_fill) depends on the committee lengths alone: one table copy, k_aggbits_mode, k_aggbits_l0, the levels of k_aggsets_ln and
// k_aggbits_finish follow on the caller's stream without a read-back in between.
// ------------------------------------------------------------------------------------------
static_assert(sizeof(plan::aggb_set) == 16, "k_aggbits_mode / k_aggbits_finish load a set as one uint4");
// device addresses of a call's inputs beyond agg_in's (aggs == nullptr: no bases)
struct aggb_in {
    agg_in a;
    const uint8_t* aggs;
    size_t agg_stride;
    const uint8_t* bits;
};
static bool aggb_args_ok(size_t n_table, bool have_idx, const size_t* c_offsets, size_t m, const void* aggs, size_t agg_stride, const uint32_t* which, size_t k) {
    if (!c_offsets || !which) return false;
    if (aggs && (agg_stride < 96 || agg_stride % 4)) {
        g_err = "aggregate_sets_bits: agg_stride is at least 96 and a multiple of 4";
        return false;
    }
    if (!agg_offsets_ok(c_offsets, m) || (!have_idx && m && c_offsets[m] > n_table)) {
        g_err = "aggregate_sets_bits: committee offsets decrease, or c_offsets[m] exceeds the number of keys";
        return false;
    }
    for (size_t s = 0; s < k; s++)
        if (which[s] >= m) {
            g_err = "aggregate_sets_bits: a set names a committee that is not there";
            return false;
        }
    return true;
}
// aggregation of k > 0 sets enqueued on st: records at d_out, status bytes in c->grp.d_status, the route census on its way to c->aggb_routes
static int aggbits_enqueue(mi355_bls_ctx* c, const aggb_in& in, size_t n_table, const size_t* c_offsets, size_t m, const uint32_t* which, size_t k, uint8_t* d_out,
                           hipStream_t st) {
    if (!in.a.keys || !in.a.msgs || !in.a.sigs || !in.bits || !d_out) return MI355_BLS_ERR_ARG;
    if (((uintptr_t)in.a.keys | (uintptr_t)in.a.msgs | (uintptr_t)in.a.sigs | (uintptr_t)in.a.idx | (uintptr_t)in.aggs | (uintptr_t)d_out) & 3) {
        g_err = "aggregate_sets_bits: keys, messages, signatures, indices, committee aggregates and records must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (!aggb_args_ok(n_table, in.a.idx != nullptr, c_offsets, m, in.aggs, in.agg_stride, which, k)) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const plan::aggbits_plan p = plan::aggbits_measure(c_offsets, m, which, k);
    if (!p.ok) {
        g_err = "aggregate_sets_bits: more than 2^32 - 2 positions, sets or level-0 items";
        return MI355_BLS_ERR_ARG;
    }
    HIPCHK(hipSetDevice(c->device));
    c->grp.items.resize((p.items + k) * 4);
    plan::aggbits_fill(p, c_offsets, which, k, reinterpret_cast<plan::agg_item*>(c->grp.items.data()), reinterpret_cast<plan::aggb_set*>(c->grp.items.data() + p.items * 4));
    const size_t pb = (p.items ? p.items : 1) * (size_t)G1W * 4;
    int rc = c->grp.d_g1_part.reserve(pb, pb / 4);
    if (!rc) rc = c->d_aggb_mode.reserve(k, k / 4);
    if (!rc) rc = c->grp.d_flag.reserve((k + 2) * 4, k);      // the two route counters behind the k flag words take no part in the slack
    if (!rc) rc = grouped_upload(c, c->grp.items.size() * 4, (k + 2) * 4, k, st);
    if (rc) return rc;
    const uint4* items = reinterpret_cast<const uint4*>(c->grp.d_items.p);
    const uint4* sets = items + p.items;
    uint32_t *part = c->grp.d_g1_part, *routes = c->grp.d_flag + k;
    k_aggbits_mode<<<plan::waves_for((uint32_t)k), WAVE, 0, st>>>(sets, (uint32_t)k, in.bits, in.aggs, in.agg_stride, c->d_aggb_mode, routes);
    launch_levels(p, items,
                  [&](const uint4* it, uint32_t cnt) {
                      k_aggbits_l0<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, in.a.keys, n_table, in.a.idx, in.bits, c->d_aggb_mode, part, c->grp.d_flag);
                  },
                  [&](const uint4* it, uint32_t cnt) { k_aggsets_ln<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, part); });
    k_aggbits_finish<<<plan::waves_for((uint32_t)k), WAVE, 0, st>>>(sets, (uint32_t)k, c->grp.d_g1_part, c->grp.d_flag, c->d_aggb_mode, in.aggs, in.agg_stride,
                                                                   reinterpret_cast<const uint32_t*>(in.a.msgs), reinterpret_cast<const uint32_t*>(in.a.sigs),
                                                                   reinterpret_cast<uint32_t*>(d_out), c->grp.d_status);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->aggb_routes, routes, 8, hipMemcpyDeviceToHost, st));      // there when grouped_status has synchronised
    return 0;
}
// host inputs -> the staged inputs: keys | signatures | messages | indices | committee aggregates, packed | bits (the byte-aligned part, last)
static int aggb_stage(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* c_offsets, size_t m, const void* aggs, size_t agg_stride,
                      const uint32_t* which, const void* bits, size_t k, const void* msgs, const void* sigs, hipStream_t st, aggb_in* out) {
    if (!keys || !msgs || !sigs || !bits || !aggb_args_ok(n_table, idx != nullptr, c_offsets, m, aggs, agg_stride, which, k)) return MI355_BLS_ERR_ARG;
    const plan::aggbits_plan p = plan::aggbits_measure(c_offsets, m, which, k);
    if (!p.ok) {
        g_err = "aggregate_sets_bits: more than 2^32 - 2 positions, sets or level-0 items";
        return MI355_BLS_ERR_ARG;
    }
    const uint8_t* d[6];
    if (int rc = stage_inputs(c, {{keys, n_table * 96}, {sigs, k * 192}, {msgs, k * 32}, {idx, c_offsets[m] * 4}, {aggs, m * 96, 96, agg_stride}, {bits, p.bits_bytes}}, st, d))
        return rc;
    *out = aggb_in{agg_in{d[0], reinterpret_cast<const uint32_t*>(d[3]), d[2], d[1]}, d[4], 96, d[5]};
    return 0;
}
// the device forms' inputs
static aggb_in aggb_device_in(const void* d_keys, const uint32_t* d_idx, const void* d_aggs, size_t agg_stride, const void* d_bits, const void* d_msgs, const void* d_sigs) {
    return aggb_in{agg_in{(const uint8_t*)d_keys, d_idx, (const uint8_t*)d_msgs, (const uint8_t*)d_sigs}, (const uint8_t*)d_aggs, agg_stride, (const uint8_t*)d_bits};
}
extern "C" int mi355_bls_aggregate_sets_bits_device(mi355_bls_ctx* c, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* c_offsets, size_t m,
                                                    const void* d_committee_aggs, size_t agg_stride, const uint32_t* which, const void* d_bits, size_t k,
                                                    const void* d_msgs32, const void* d_sigs192, void* d_out_records, uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing aggregated, nothing written
    if (!status) return MI355_BLS_ERR_ARG;
    const aggb_in in = aggb_device_in(d_keys, d_idx, d_committee_aggs, agg_stride, d_bits, d_msgs32, d_sigs192);
    int rc = aggbits_enqueue(c, in, n_table, c_offsets, m, which, k, (uint8_t*)d_out_records, (hipStream_t)stream);
    if (rc) return rc;
    return grouped_status(c, k, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_aggregate_sets_bits(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* c_offsets, size_t m,
                                             const void* committee_aggs, size_t agg_stride, const uint32_t* which, const void* bits, size_t k, const void* msgs32,
                                             const void* sigs192, void* out_records, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!out_records || !status) return MI355_BLS_ERR_ARG;
    aggb_in in;
    if (int rc = aggb_stage(c, keys, n_table, idx, c_offsets, m, committee_aggs, agg_stride, which, bits, k, msgs32, sigs192, nullptr, &in)) return rc;
    return records_to_host(c, k, out_records, status,
                           [&](uint8_t* d_out, hipStream_t st) { return aggbits_enqueue(c, in, n_table, c_offsets, m, which, k, d_out, st); });
}
// fastAggregateVerify for every set, as for key lists (records_each)
extern "C" int mi355_bls_fast_aggregate_verify_each_bits_device(mi355_bls_ctx* c, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* c_offsets,
                                                                size_t m, const void* d_committee_aggs, size_t agg_stride, const uint32_t* which, const void* d_bits,
                                                                size_t k, const void* d_msgs32, const void* d_sigs192, uint8_t* out, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!out) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const aggb_in in = aggb_device_in(d_keys, d_idx, d_committee_aggs, agg_stride, d_bits, d_msgs32, d_sigs192);
    return records_each(c, k, out, (hipStream_t)stream,
                        [&](uint8_t* d_out, hipStream_t st) { return aggbits_enqueue(c, in, n_table, c_offsets, m, which, k, d_out, st); });
}
extern "C" int mi355_bls_fast_aggregate_verify_each_bits(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* c_offsets, size_t m,
                                                         const void* committee_aggs, size_t agg_stride, const uint32_t* which, const void* bits, size_t k,
                                                         const void* msgs32, const void* sigs192, uint8_t* out) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!out) return MI355_BLS_ERR_ARG;
    aggb_in in;
    if (int rc = aggb_stage(c, keys, n_table, idx, c_offsets, m, committee_aggs, agg_stride, which, bits, k, msgs32, sigs192, nullptr, &in)) return rc;
    return records_each(c, k, out, nullptr, [&](uint8_t* d_out, hipStream_t st) { return aggbits_enqueue(c, in, n_table, c_offsets, m, which, k, d_out, st); });
}
// batchVerify over the records, as for key lists (records_batch)
extern "C" int mi355_bls_batch_fast_aggregate_verify_bits_device(mi355_bls_ctx* c, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* c_offsets,
                                                                 size_t m, const void* d_committee_aggs, size_t agg_stride, const uint32_t* which, const void* d_bits,
                                                                 size_t k, const void* d_msgs32, const void* d_sigs192, const uint8_t rnd[32], void* stream) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    const aggb_in in = aggb_device_in(d_keys, d_idx, d_committee_aggs, agg_stride, d_bits, d_msgs32, d_sigs192);
    return records_batch(c, k, rnd, (hipStream_t)stream,
                         [&](uint8_t* d_out, hipStream_t st) { return aggbits_enqueue(c, in, n_table, c_offsets, m, which, k, d_out, st); });
}
extern "C" int mi355_bls_batch_fast_aggregate_verify_bits(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* c_offsets, size_t m,
                                                          const void* committee_aggs, size_t agg_stride, const uint32_t* which, const void* bits, size_t k,
                                                          const void* msgs32, const void* sigs192, const uint8_t rnd[32]) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    aggb_in in;
    if (int rc = aggb_stage(c, keys, n_table, idx, c_offsets, m, committee_aggs, agg_stride, which, bits, k, msgs32, sigs192, nullptr, &in)) return rc;
    return records_batch(c, k, rnd, nullptr, [&](uint8_t* d_out, hipStream_t st) { return aggbits_enqueue(c, in, n_table, c_offsets, m, which, k, d_out, st); });
}
extern "C" int mi355_bls_debug_aggregate_bits_routes(mi355_bls_ctx* c, uint32_t out[2]) {
    if (!c || !out) return MI355_BLS_ERR_ARG;
    out[0] = c->aggb_routes[0], out[1] = c->aggb_routes[1];
    return 0;
}

// ------------------------------------------------------------------------------------------
// Per-group aggregateVerify: aggregateVerify (bls_sig_min_pubkey.nim:127-199 -> ContextCoreAggregateVerify, core :305-414) for k groups of
// (key, message) pairs with one aggregate signature each, in one device pass.  The keys are addressed as aggregate_sets addresses them; the
// messages are 32 bytes each and follow the POSITIONS (never the indices).  The call runs in slices of at most max_sets pairs (plan.hpp
// aggveach_cut): per slice one copy of its tables, the records and pair slots (k_aggveach_records), hashing and Miller lines in the forms the
// per-set path takes, the segmented line product level by level, and the tail in the form plan::aggveach_for names.  A group longer than a
// slice hands its Miller value from part to part in d_aggv_carry.  The verdict bytes of all slices collect in d_each_v and come back in one
// copy: the call's only synchronisation.
// ------------------------------------------------------------------------------------------
static_assert(sizeof(plan::aggv_group) == 16, "k_aggveach_* load a group as one uint4");
static int aggveach_run(mi355_bls_ctx* c, const agg_in& in, size_t n_table, const size_t* offsets, size_t k, uint8_t* out, uint8_t* gt_out, hipStream_t st) {
    if (!in.keys || !in.msgs || !in.sigs || !offsets || !out) return MI355_BLS_ERR_ARG;
    if (((uintptr_t)in.keys | (uintptr_t)in.msgs | (uintptr_t)in.sigs | (uintptr_t)in.idx) & 3) {
        g_err = "aggregate_verify_each: keys, messages, signatures and indices must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    if (k >= plan::AGG_NONE || !agg_offsets_ok(offsets, k) || offsets[k] >= plan::AGG_NONE) {
        g_err = "aggregate_verify_each: offsets decrease, or more than 2^32 - 2 pairs or groups";
        return MI355_BLS_ERR_ARG;
    }
    if (!table_holds(in.idx, offsets, k, n_table, "aggregate_verify_each: offsets[k] exceeds the number of keys")) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    // pass 1: the slices and their tables (groups | items, slice after slice), and what the largest slice needs
    struct slice_rec {
        plan::aggv_slice s;
        plan::aggveach_tab t;
        size_t tab_at;
    };
    std::vector<slice_rec> slices;
    c->aggv_tab.clear();
    size_t max_part = 0, max_ng = 0, max_tab = 0;
    for (size_t g = 0, pos = offsets[0];;) {
        const plan::aggv_slice s = plan::aggveach_cut(offsets, k, g, pos, c->cap);
        if (s.pairs() == 0) break;
        const size_t at = c->aggv_tab.size();
        c->aggv_tab.resize(at + (size_t)s.ng * 4);
        plan::aggveach_groups(offsets, s, reinterpret_cast<plan::aggv_group*>(c->aggv_tab.data() + at));
        const plan::aggveach_tab t = plan::aggveach_measure(reinterpret_cast<const plan::aggv_group*>(c->aggv_tab.data() + at), s.ng);
        c->aggv_tab.resize(at + ((size_t)s.ng + t.items) * 4);
        plan::aggveach_fill(t, reinterpret_cast<const plan::aggv_group*>(c->aggv_tab.data() + at), s.ng,
                            reinterpret_cast<plan::agg_item*>(c->aggv_tab.data() + at + (size_t)s.ng * 4));
        slices.push_back({s, t, at});
        if (t.partials > max_part) max_part = t.partials;
        if (s.ng > max_ng) max_ng = s.ng;
        if (((size_t)s.ng + t.items) * 4 > max_tab) max_tab = ((size_t)s.ng + t.items) * 4;
        g = s.next_g(), pos = s.pos1;
    }
    int rc = each_reserve(c, k, gt_out != nullptr);
    const size_t pw = plan::aggveach_part_words(max_part) * 4, sw = plan::aggveach_step_words(max_ng) * 4;
    if (!rc) rc = c->grp.d_flag.reserve(k * 4, k);
    if (!rc) rc = c->d_aggv_part.reserve(pw, pw / 4);
    if (!rc) rc = c->d_aggv_step.reserve(sw, sw / 4);
    if (!rc) rc = c->d_aggv_tab.reserve(max_tab * 4 + 16, max_tab);
    if (!rc) rc = c->d_aggv_carry.reserve(2 * 576, 0);
    if (!rc) rc = c->d_aggv_work.reserve((size_t)plan::each_engine_grid_max(c->slots) * AGGV_WORK_WORDS * 4, 0);
    if (rc) return rc;
    const pair_store ps = c->each_pairs();
    HIPCHK(hipEventRecord(c->ev[0], st));
    HIPCHK(hipMemsetAsync(c->grp.d_flag, 0, k * 4, st));
    HIPCHK(hipMemsetAsync(c->d_each_v, 0, k, st));                     // an empty group has no lane: its verdict is 0, its value zero bytes
    if (gt_out) HIPCHK(hipMemsetAsync(c->d_each_gt, 0, k * 576, st));
    uint32_t* dg = gt_out ? c->d_each_gt.p : nullptr;
    for (const slice_rec& sr : slices) {
        const plan::aggv_slice& s = sr.s;
        const uint32_t P = (uint32_t)s.pairs(), nsig = s.sigs();
        const plan::aggveach_plan p = plan::aggveach_for(c->slots, c->coop, P, nsig, s.ng);
        HIPCHK(hipMemcpyAsync(c->d_aggv_tab, c->aggv_tab.data() + sr.tab_at, ((size_t)s.ng + sr.t.items) * 16, hipMemcpyHostToDevice, st));
        const uint4* gtab = reinterpret_cast<const uint4*>(c->d_aggv_tab.p);
        const uint4* items = gtab + s.ng;
        k_aggveach_records<<<p.setup_grid, WAVE, 0, st>>>(in.keys, n_table, in.idx, s.pos0, P, reinterpret_cast<const uint32_t*>(in.msgs), gtab, s.ng, nsig,
                                                          reinterpret_cast<const uint32_t*>(in.sigs), reinterpret_cast<uint32_t*>(c->d_sets.p), ps.H, ps.P,
                                                          ps.stride, c->grp.d_flag);
        launch_hash_map(c, c->d_sets, P, st);                              // H(msg_i) -> pair slot i, in the forms the batch path takes for P messages
        launch_hash_clear(c, ps, P, st);
        launch_lines(ps, p.lines, st);
        const uint32_t n_part = (uint32_t)(sr.t.partials ? sr.t.partials : 1);
        uint32_t *part = c->d_aggv_part, *step = c->d_aggv_step;
        launch_levels(sr.t, items,
                      [&](const uint4* it, uint32_t cnt) {
                          k_aggveach_l0<<<dim3(plan::waves_for(cnt), N_LINES), WAVE, 0, st>>>(it, cnt, ps.lines, ps.stride, P, part, n_part, step);
                      },
                      [&](const uint4* it, uint32_t cnt) { k_aggveach_ln<<<dim3(plan::waves_for(cnt), N_LINES), WAVE, 0, st>>>(it, cnt, part, n_part, step); });
        if (!p.tail_engine) {
            k_aggveach_tail<<<p.tail_grid, WAVE, 0, st>>>(c->d_aggv_step, gtab, s.ng, c->grp.d_flag, c->d_aggv_carry, c->d_each_v, dg);
        } else {
            k_aggveach_engine_rows<<<p.tail_grid, K_TAIL_THREADS, 0, st>>>(c->d_aggv_step, gtab, s.ng, c->grp.d_flag, c->d_aggv_carry, c->d_each_v, dg, c->d_aggv_work);
            if (s.open_in && s.open_out) k_state_mul<<<1, TAIL_THREADS, 0, st>>>(c->d_aggv_carry, 0, 0, 1);      // the part's value into the carried one
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[1], st));
    HIPCHK(hipMemcpyAsync(out, c->d_each_v, k, hipMemcpyDeviceToHost, st));
    if (gt_out) HIPCHK(hipMemcpyAsync(gt_out, c->d_each_gt, k * 576, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->last_n = 0;                             // fetch_stage shows the last call, and this one left no batch stages
    c->sig_slots = 0;
    c->agg_valid = false;
    c->have_gt = false;
    rc = collect_timings(c, 1);
    if (rc) return rc;
    int all = 1;
    for (size_t g = 0; g < k; g++) all &= out[g] == 1;
    return all;
}
extern "C" int mi355_bls_aggregate_verify_each_device(mi355_bls_ctx* c, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k,
                                                      const void* d_msgs32, const void* d_sigs192, uint8_t* out, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing verified, nothing written
    return aggveach_run(c, agg_in{(const uint8_t*)d_keys, d_idx, (const uint8_t*)d_msgs32, (const uint8_t*)d_sigs192}, n_table, offsets, k, out, nullptr,
                        (hipStream_t)stream);
}
// host inputs staged as aggregate_sets stages them (the messages follow the positions), then the device form
static int aggveach_host(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k, const void* msgs32,
                         const void* sigs192, uint8_t* out, uint8_t* gt_out) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!keys || !offsets || !msgs32 || !sigs192 || !out || !agg_offsets_ok(offsets, k)) return MI355_BLS_ERR_ARG;
    if (offsets[k] >= plan::AGG_NONE || (!idx && offsets[k] > n_table)) {      // before anything is staged (aggveach_run says the same)
        g_err = "aggregate_verify_each: offsets[k] exceeds the number of keys, or 2^32 - 2 pairs";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    agg_in in;
    if (int rc = agg_stage(c, keys, n_table, idx, offsets, k, msgs32, offsets[k] * 32, sigs192, nullptr, &in)) return rc;
    return aggveach_run(c, in, n_table, offsets, k, out, gt_out, nullptr);
}
extern "C" int mi355_bls_aggregate_verify_each(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                               const void* msgs32, const void* sigs192, uint8_t* out) {
    return aggveach_host(c, keys, n_table, idx, offsets, k, msgs32, sigs192, out, nullptr);
}
// TEST HOOK: the same pass with the 576-byte value of every group (zero bytes for an empty group)
extern "C" int mi355_bls_debug_aggregate_verify_each_gt(mi355_bls_ctx* c, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                                        const void* msgs32, const void* sigs192, uint8_t* out, uint8_t* gt_out) {
    if (k && !gt_out) return MI355_BLS_ERR_ARG;
    return aggveach_host(c, keys, n_table, idx, offsets, k, msgs32, sigs192, out, gt_out);
}

// ------------------------------------------------------------------------------------------
// Pairing-product checks over caller-supplied pairs (blst_miller_loop_n + blst_final_exp + blst_fp12_finalverify, blst_abi.nim:294,317,453-461,
// for k groups in one device pass).  Group g = pairs [offsets[g], offsets[g + 1]) of two packed arrays of affine images.  One driver:
//   r == nullptr   pairing_check_each / pairing_products: the groups are groups of the per-group path without a signature pair (plan.hpp
//                  aggveach_cut over `cap` pairs, aggveach_fill with_sig = false); verdict bytes and values by the group's number in the call
//   r != nullptr   the blinded form: ALL pairs are one group of that path (plan::pairprod_blind_cut), P of every pair multiplied by its own
//                  group's scalar (k_pairprod_setup expands r to the pair slots and lays the keys out for k_pkmul); one verdict, one value
// Per slice: one copy of its tables, k_pairprod_setup, [k_pkmul,] the Miller lines, the line product level by level, the tail.  No hashing
// kernel runs.  Verdicts, values and status bytes come back behind the last slice: the call's only synchronisation.  The empty groups, which
// have no lane, are fixed up on the host: verdict 1, the image of one.
// ------------------------------------------------------------------------------------------
// the rules that are decided before the context is looked into (c != nullptr and k != 0 are the caller's)
static int pairprod_args(const void* p1, const void* q2, const size_t* offsets, size_t k, uint32_t flags, const uint8_t* status, bool device) {
    if (!offsets || offsets[0] != 0 || !agg_offsets_ok(offsets, k)) {
        g_err = "pairing_check: offsets are missing, do not start at 0, or decrease";
        return MI355_BLS_ERR_ARG;
    }
    if (offsets[k] && (!p1 || !q2)) return MI355_BLS_ERR_ARG;
    if (flags & ~(uint32_t)MI355_BLS_PAIR_VALIDATE) {
        g_err = "pairing_check: unknown flag bits";
        return MI355_BLS_ERR_ARG;
    }
    if ((flags & MI355_BLS_PAIR_VALIDATE) && !status) {
        g_err = "pairing_check: MI355_BLS_PAIR_VALIDATE needs the status array";
        return MI355_BLS_ERR_ARG;
    }
    if (device && (((uintptr_t)p1 | (uintptr_t)q2) & 3)) {
        g_err = "pairing_check: device pointers must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (k >= plan::AGG_NONE || offsets[k] >= plan::AGG_NONE) {
        g_err = "pairing_check: more than 2^32 - 2 pairs or groups (the tables are 32-bit)";
        return MI355_BLS_ERR_ARG;
    }
    return 0;
}
static_assert(MI355_BLS_PAIR_VALIDATE == plan::PAIRPROD_VALIDATE && MI355_BLS_PAIR_Q_NOT_IN_G2 == PAIRPROD_Q_NOT_IN_G2, "the header restates pairprod.hpp's codes");
// out: k verdict bytes (r == nullptr) or one; gt_out (may be null): as many 576-byte values.  d_p1 / d_q2: device memory (null when there is no pair).
static int pairprod_run(mi355_bls_ctx* c, const uint8_t* d_p1, const uint8_t* d_q2, const size_t* offsets, size_t k, uint32_t flags, uint8_t* status,
                        uint8_t* out, uint8_t* gt_out, const uint64_t* r, hipStream_t st) {
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const bool blinded = r != nullptr;
    const size_t n = offsets[k], nres = blinded ? 1 : k;
    // pass 1: the slices and their tables (groups | items | the blinded form's real groups, slice after slice), and what the largest needs
    struct slice_rec {
        plan::aggv_slice s;
        plan::aggveach_tab t;
        size_t tab_at;
        uint32_t real;
    };
    std::vector<slice_rec> slices;
    c->aggv_tab.clear();
    size_t max_part = 0, max_ng = 0, max_tab = 0, max_pairs = 0;
    const size_t one[2] = {0, n};
    for (size_t g = 0, pos = 0;;) {
        const plan::aggv_slice s = blinded ? plan::pairprod_blind_cut(n, pos, c->cap) : plan::aggveach_cut(offsets, k, g, pos, c->cap);
        if (s.pairs() == 0) break;
        const size_t at = c->aggv_tab.size();
        c->aggv_tab.resize(at + (size_t)s.ng * 4);
        plan::aggveach_groups(blinded ? one : offsets, s, reinterpret_cast<plan::aggv_group*>(c->aggv_tab.data() + at));
        const plan::aggveach_tab t = plan::aggveach_measure(reinterpret_cast<const plan::aggv_group*>(c->aggv_tab.data() + at), s.ng);
        c->aggv_tab.resize(at + ((size_t)s.ng + t.items) * 4);
        plan::aggveach_fill(t, reinterpret_cast<const plan::aggv_group*>(c->aggv_tab.data() + at), s.ng,
                            reinterpret_cast<plan::agg_item*>(c->aggv_tab.data() + at + (size_t)s.ng * 4), plan::AGGV_C, false);
        uint32_t real = 0;
        if (blinded) {
            const plan::aggv_slice rs = plan::pairprod_real_groups(offsets, k, s.pos0, s.pos1);
            real = rs.ng;
            const size_t rat = c->aggv_tab.size();
            c->aggv_tab.resize(rat + (size_t)real * 4);
            plan::aggveach_groups(offsets, rs, reinterpret_cast<plan::aggv_group*>(c->aggv_tab.data() + rat));
        }
        slices.push_back({s, t, at, real});
        const size_t entries = plan::pairprod_tab_entries(s.ng, t.items, real);
        if (t.partials > max_part) max_part = t.partials;
        if (s.ng > max_ng) max_ng = s.ng;
        if (entries * 4 > max_tab) max_tab = entries * 4;
        if (s.pairs() > max_pairs) max_pairs = s.pairs();
        g = s.next_g(), pos = s.pos1;
    }
    const plan::pairprod_sizes sz = plan::pairprod_sizes_for(n, k, blinded);
    int rc = each_reserve(c, nres, gt_out != nullptr);
    const size_t pw = plan::aggveach_part_words(max_part) * 4, sw = plan::aggveach_step_words(max_ng) * 4;
    if (!rc) rc = c->grp.d_flag.reserve(sz.flags, sz.flags / 4);
    if (!rc) rc = c->d_pp_status.reserve(sz.status, sz.status / 4);
    if (!rc && blinded) rc = c->d_pp_r.reserve(sz.scalars, sz.scalars / 4);
    if (!rc && blinded) rc = c->d_comb_pkflag.reserve(4, 0);
    if (!rc) rc = c->d_aggv_part.reserve(pw, pw / 4);
    if (!rc) rc = c->d_aggv_step.reserve(sw, sw / 4);
    if (!rc) rc = c->d_aggv_tab.reserve(max_tab * 4 + 16, max_tab);
    if (!rc) rc = c->d_aggv_carry.reserve(2 * 576, 0);
    if (!rc) rc = c->d_aggv_work.reserve((size_t)plan::each_engine_grid_max(c->slots) * AGGV_WORK_WORDS * 4, 0);
    if (rc) return rc;
    const pair_store ps = c->each_pairs();
    HIPCHK(hipEventRecord(c->ev[0], st));
    HIPCHK(hipMemsetAsync(c->grp.d_flag, 0, sz.flags, st));
    HIPCHK(hipMemsetAsync(c->d_each_v, 0, nres, st));                  // a group without pairs has no lane: fixed up on the host below
    if (gt_out) HIPCHK(hipMemsetAsync(c->d_each_gt, 0, nres * 576, st));
    if (blinded) HIPCHK(hipMemcpyAsync(c->d_pp_r, r, k * 8, hipMemcpyHostToDevice, st));
    uint32_t* dg = gt_out ? c->d_each_gt.p : nullptr;
    uint8_t* d_status = status ? c->d_pp_status.p : nullptr;
    for (const slice_rec& sr : slices) {
        const plan::aggv_slice& s = sr.s;
        const uint32_t P = (uint32_t)s.pairs();
        const plan::pairprod_plan p = plan::pairprod_for(c->slots, c->coop, P, s.ng, blinded);
        HIPCHK(hipMemcpyAsync(c->d_aggv_tab, c->aggv_tab.data() + sr.tab_at, plan::pairprod_tab_entries(s.ng, sr.t.items, sr.real) * 16, hipMemcpyHostToDevice, st));
        const uint4* gtab = reinterpret_cast<const uint4*>(c->d_aggv_tab.p);
        const uint4* items = gtab + s.ng;
        const uint4* real = blinded ? items + sr.t.items : gtab;
        k_pairprod_setup<<<p.setup_grid, WAVE, 0, st>>>(reinterpret_cast<const uint32_t*>(d_p1), reinterpret_cast<const uint32_t*>(d_q2), s.pos0, P, real,
                                                        blinded ? sr.real : s.ng, flags, blinded ? c->d_pp_r.p : nullptr, reinterpret_cast<uint32_t*>(c->d_sets.p),
                                                        c->d_r, ps.H, ps.P, ps.stride, d_status, c->grp.d_flag);
        if (blinded) {
            HIPCHK(hipMemsetAsync(c->d_comb_pkflag, 0, 4, st));           // k_pkmul's word for an infinity key: such a pair contributes 1 here, nothing reads it
            if (p.pkmul_spread) k_pkmul_spread<<<plan::waves_for(P), WAVE, 0, st>>>(c->d_sets, P, c->d_r, ps.P, ps.stride, c->d_comb_pkflag, c->d_pktab);
            else k_pkmul<<<plan::waves_for(P), WAVE, 0, st>>>(c->d_sets, P, c->d_r, ps.P, ps.stride, c->d_comb_pkflag, c->d_pktab);
        }
        launch_lines(ps, p.lines, st);
        const uint32_t n_part = (uint32_t)(sr.t.partials ? sr.t.partials : 1);
        uint32_t *part = c->d_aggv_part, *step = c->d_aggv_step;
        launch_levels(sr.t, items,
                      [&](const uint4* it, uint32_t cnt) {
                          k_aggveach_l0<<<dim3(plan::waves_for(cnt), N_LINES), WAVE, 0, st>>>(it, cnt, ps.lines, ps.stride, P, part, n_part, step);
                      },
                      [&](const uint4* it, uint32_t cnt) { k_aggveach_ln<<<dim3(plan::waves_for(cnt), N_LINES), WAVE, 0, st>>>(it, cnt, part, n_part, step); });
        if (!p.tail_engine) {
            k_aggveach_tail<<<p.tail_grid, WAVE, 0, st>>>(step, gtab, s.ng, c->grp.d_flag, c->d_aggv_carry, c->d_each_v, dg);
        } else {
            k_aggveach_engine_rows<<<p.tail_grid, K_TAIL_THREADS, 0, st>>>(step, gtab, s.ng, c->grp.d_flag, c->d_aggv_carry, c->d_each_v, dg, c->d_aggv_work);
            if (s.open_in && s.open_out) k_state_mul<<<1, TAIL_THREADS, 0, st>>>(c->d_aggv_carry, 0, 0, 1);      // the part's value into the carried one
        }
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[1], st));
    HIPCHK(hipMemcpyAsync(out, c->d_each_v, nres, hipMemcpyDeviceToHost, st));
    if (gt_out) HIPCHK(hipMemcpyAsync(gt_out, c->d_each_gt, nres * 576, hipMemcpyDeviceToHost, st));
    if (status && n) HIPCHK(hipMemcpyAsync(status, c->d_pp_status, n, hipMemcpyDeviceToHost, st));
    if (blinded) {                                                     // blinding material: nothing of it stays on the device
        HIPCHK(hipMemsetAsync(c->d_pp_r, 0, k * 8, st));
        if (max_pairs) HIPCHK(hipMemsetAsync(c->d_r, 0, max_pairs * 8, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    c->last_n = 0;                             // fetch_stage shows the last call, and this one left no batch stages
    c->sig_slots = 0;
    c->agg_valid = false;
    c->have_gt = false;
    rc = collect_timings(c, 1);
    if (rc) return rc;
    // the empty product: a group without pairs (the blinded form: a call without pairs) has verdict 1 and the value one
    uint8_t one_image[576];
    if (gt_out) fp12_store_le(one_image, fp12_one());
    for (size_t g = 0; g < nres; g++) {
        if (blinded ? n != 0 : offsets[g + 1] != offsets[g]) continue;
        out[g] = 1;
        if (gt_out) std::memcpy(gt_out + g * 576, one_image, 576);
    }
    int all = 1;
    for (size_t g = 0; g < nres; g++) all &= out[g] == 1;
    return all;
}
// the two arrays of a host form staged (the existing stager: p1s96 | q2s192 in grp.d_in), or the device form's pointers as they are
static int pairprod_stage(mi355_bls_ctx* c, const void* p1, const void* q2, size_t n, bool host, const uint8_t** d_p1, const uint8_t** d_q2) {
    if (!host || n == 0) {
        *d_p1 = n ? (const uint8_t*)p1 : nullptr, *d_q2 = n ? (const uint8_t*)q2 : nullptr;
        return 0;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const host_part parts[2] = {{p1, n * 96}, {q2, n * 192}};
    const uint8_t* d[2];
    if (int rc = stage_inputs(c, parts, nullptr, d)) return rc;
    *d_p1 = d[0], *d_q2 = d[1];
    return 0;
}
static int pairprod_each(mi355_bls_ctx* c, const void* p1, const void* q2, const size_t* offsets, size_t k, uint32_t flags, uint8_t* out, uint8_t* status,
                         uint8_t* gt_out, bool want_gt, bool host, hipStream_t st) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing checked, nothing written
    if (!out || (want_gt && !gt_out)) return MI355_BLS_ERR_ARG;
    if (int rc = pairprod_args(p1, q2, offsets, k, flags, status, !host)) return rc;
    const uint8_t *d_p1, *d_q2;
    if (int rc = pairprod_stage(c, p1, q2, offsets[k], host, &d_p1, &d_q2)) return rc;
    return pairprod_run(c, d_p1, d_q2, offsets, k, flags, status, out, gt_out, nullptr, st);
}
// The blinded driver.  r: the k scalars (the hook's), or null: the serial chain from rnd32.  out != nullptr: the locate form.
static int pairprod_blind(mi355_bls_ctx* c, const void* p1, const void* q2, const size_t* offsets, size_t k, uint32_t flags, const uint8_t* rnd32,
                          const uint64_t* r, uint8_t* status, uint8_t* out, bool locate, uint8_t* gt_out, bool host, hipStream_t st) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if ((!rnd32 && !r) || (locate && !out)) return MI355_BLS_ERR_ARG;
    if (int rc = pairprod_args(p1, q2, offsets, k, flags, status, !host)) return rc;
    const uint8_t *d_p1, *d_q2;
    if (int rc = pairprod_stage(c, p1, q2, offsets[k], host, &d_p1, &d_q2)) return rc;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    c->pp_r.resize(k);
    if (r) std::memcpy(c->pp_r.data(), r, k * 8);
    else host_serial_chain(rnd32, k, c->pp_r.data());
    uint8_t verdict = 0;
    int rc = pairprod_run(c, d_p1, d_q2, offsets, k, flags, status, &verdict, gt_out, c->pp_r.data(), st);
    std::fill(c->pp_r.begin(), c->pp_r.end(), 0);      // pairprod_run has drained the stream: the copy that read them is done
    if (rc < 0 || !locate) return rc;
    if (rc == 1) {
        std::memset(out, 1, k);
        return 1;
    }
    rc = pairprod_run(c, d_p1, d_q2, offsets, k, flags, status, out, nullptr, nullptr, st);      // only behind a failure
    return rc < 0 ? rc : 0;
}
extern "C" int mi355_bls_pairing_check_each(mi355_bls_ctx* c, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags, uint8_t* out,
                                            uint8_t* status) {
    return pairprod_each(c, p1s96, q2s192, offsets, k, flags, out, status, nullptr, false, true, nullptr);
}
extern "C" int mi355_bls_pairing_check_each_device(mi355_bls_ctx* c, const void* d_p1s96, const void* d_q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                                   uint8_t* out, uint8_t* status, void* stream) {
    return pairprod_each(c, d_p1s96, d_q2s192, offsets, k, flags, out, status, nullptr, false, false, (hipStream_t)stream);
}
extern "C" int mi355_bls_pairing_products(mi355_bls_ctx* c, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags, uint8_t* out,
                                          uint8_t* status, uint8_t* gt_out) {
    return pairprod_each(c, p1s96, q2s192, offsets, k, flags, out, status, gt_out, true, true, nullptr);
}
extern "C" int mi355_bls_pairing_products_device(mi355_bls_ctx* c, const void* d_p1s96, const void* d_q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                                 uint8_t* out, uint8_t* status, uint8_t* gt_out, void* stream) {
    return pairprod_each(c, d_p1s96, d_q2s192, offsets, k, flags, out, status, gt_out, true, false, (hipStream_t)stream);
}
extern "C" int mi355_bls_batch_pairing_check(mi355_bls_ctx* c, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                             const uint8_t rnd32[32], uint8_t* status) {
    return pairprod_blind(c, p1s96, q2s192, offsets, k, flags, rnd32, nullptr, status, nullptr, false, nullptr, true, nullptr);
}
extern "C" int mi355_bls_batch_pairing_check_device(mi355_bls_ctx* c, const void* d_p1s96, const void* d_q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                                    const uint8_t rnd32[32], uint8_t* status, void* stream) {
    return pairprod_blind(c, d_p1s96, d_q2s192, offsets, k, flags, rnd32, nullptr, status, nullptr, false, nullptr, false, (hipStream_t)stream);
}
extern "C" int mi355_bls_batch_pairing_check_locate(mi355_bls_ctx* c, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                                    const uint8_t rnd32[32], uint8_t* status, uint8_t* out) {
    return pairprod_blind(c, p1s96, q2s192, offsets, k, flags, rnd32, nullptr, status, out, true, nullptr, true, nullptr);
}
extern "C" int mi355_bls_batch_pairing_check_locate_device(mi355_bls_ctx* c, const void* d_p1s96, const void* d_q2s192, const size_t* offsets, size_t k,
                                                           uint32_t flags, const uint8_t rnd32[32], uint8_t* status, uint8_t* out, void* stream) {
    return pairprod_blind(c, d_p1s96, d_q2s192, offsets, k, flags, rnd32, nullptr, status, out, true, nullptr, false, (hipStream_t)stream);
}
// TEST HOOK: the blinded form with the test's k scalars and the 576-byte value of the one product
extern "C" int mi355_bls_debug_batch_pairing_check_scalars(mi355_bls_ctx* c, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                                           const uint64_t* r, uint8_t* status, uint8_t* gt_out) {
    if (c && k && (!r || !gt_out)) return MI355_BLS_ERR_ARG;
    return pairprod_blind(c, p1s96, q2s192, offsets, k, flags, nullptr, r, status, nullptr, false, gt_out, true, nullptr);
}

// ------------------------------------------------------------------------------------------
// Per-group signature aggregation: aggregateAll on signatures (genAggregatorProcedures(AggregateSignature, Signature, p2),
// blst_min_pubkey_sig_core.nim:142-211) for k groups in one device pass, each finished to its blst_p2_affine image and serialised
// (bls_sig_io.nim:225-234).  The addressing, the plan and the item table are aggregate_sets' (group g = positions [offsets[g], offsets[g + 1])
// of the signature sequence: the table itself, or table entries picked by index); level 0 is k_aggsigs_l0, higher levels k_combsets_g2_sum,
// then k_aggsigs_finish, all on the caller's stream.
// ------------------------------------------------------------------------------------------
// aggregation of k > 0 groups enqueued on st: images at d_out192, wire forms at d_out96 (either may be null), status bytes in c->grp.d_status
static int aggsigs_enqueue(mi355_bls_ctx* c, const uint8_t* d_sigs, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k, uint8_t* d_out192,
                           uint8_t* d_out96, hipStream_t st) {
    if (!d_sigs || !offsets || (!d_out192 && !d_out96)) return MI355_BLS_ERR_ARG;
    if (((uintptr_t)d_sigs | (uintptr_t)d_idx | (uintptr_t)d_out192 | (uintptr_t)d_out96) & 3) {
        g_err = "aggregate_signature_sets: signatures, indices and outputs must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const plan::aggsets_plan p = k < plan::AGG_NONE ? plan::aggsets_measure(offsets, k) : plan::aggsets_plan{};
    if (!p.ok) {
        g_err = "aggregate_signature_sets: offsets decrease, or more than 2^32 - 2 signatures or groups";
        return MI355_BLS_ERR_ARG;
    }
    if (!table_holds(d_idx, offsets, k, n_table, "aggregate_signature_sets: offsets[k] exceeds the number of signatures")) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    c->grp.items.resize(p.items * 4 + k);
    plan::aggsets_fill(p, offsets, k, reinterpret_cast<plan::agg_item*>(c->grp.items.data()), c->grp.items.data() + p.items * 4);
    const plan::aggsigs_sizes sz = plan::aggsigs_sizes_for(p, k);
    int rc = c->grp.d_g2_part.reserve(sz.part, sz.part / 4);
    if (!rc) rc = grouped_upload(c, sz.tab, sz.bad, sz.status, st);
    if (rc) return rc;
    uint32_t* part = c->grp.d_g2_part;
    launch_levels(p, reinterpret_cast<const uint4*>(c->grp.d_items.p),
                  [&](const uint4* it, uint32_t cnt) {
                      k_aggsigs_l0<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, reinterpret_cast<const uint32_t*>(d_sigs), n_table, d_idx, part, c->grp.d_flag);
                  },
                  [&](const uint4* it, uint32_t cnt) { k_combsets_g2_sum<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, part, part); });
    k_aggsigs_finish<<<plan::waves_for((uint32_t)k), WAVE, 0, st>>>(c->grp.d_items + p.items * 4, (uint32_t)k, c->grp.d_g2_part, c->grp.d_flag,
                                                                   reinterpret_cast<uint32_t*>(d_out192), reinterpret_cast<uint32_t*>(d_out96), c->grp.d_status);
    HIPCHK(hipGetLastError());
    return 0;
}
extern "C" int mi355_bls_aggregate_signature_sets_device(mi355_bls_ctx* c, const void* d_sigs192, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                                         size_t k, void* d_out_sigs192, void* d_out_sigs96, uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing aggregated, nothing written
    if (!status) return MI355_BLS_ERR_ARG;
    int rc = aggsigs_enqueue(c, (const uint8_t*)d_sigs192, n_table, d_idx, offsets, k, (uint8_t*)d_out_sigs192, (uint8_t*)d_out_sigs96, (hipStream_t)stream);
    if (rc) return rc;
    return grouped_status(c, k, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_aggregate_signature_sets(mi355_bls_ctx* c, const void* sigs192, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                                  void* out_sigs192, void* out_sigs96, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!sigs192 || !offsets || !status || (!out_sigs192 && !out_sigs96) || !agg_offsets_ok(offsets, k)) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const uint8_t* d[2];      // signatures | indices
    int rc = stage_inputs(c, {{sigs192, n_table * 192}, {idx, offsets[k] * 4}}, nullptr, d);
    if (!rc) rc = c->grp.d_g2_out.reserve(k * 288, k * 72);
    if (rc) return rc;
    uint8_t *o192 = c->grp.d_g2_out, *o96 = o192 + k * 192;
    rc = aggsigs_enqueue(c, d[0], n_table, reinterpret_cast<const uint32_t*>(d[1]), offsets, k, out_sigs192 ? o192 : nullptr, out_sigs96 ? o96 : nullptr, nullptr);
    if (rc) return rc;
    if (out_sigs192) HIPCHK(hipMemcpyAsync(out_sigs192, o192, k * 192, hipMemcpyDeviceToHost, nullptr));
    if (out_sigs96) HIPCHK(hipMemcpyAsync(out_sigs96, o96, k * 96, hipMemcpyDeviceToHost, nullptr));
    return grouped_status(c, k, status, nullptr);
}

// ------------------------------------------------------------------------------------------
// Threshold-signature recovery: recover(signs, ids) (blst_recovery.nim:150-156; lagrangeInterpolation :90-121 in the exponent) for k groups
// in one device pass.  The addressing is aggregate_signature_sets' (a table of blst_p2_affine images, optional indices, k + 1 host offsets);
// ids holds 32 bytes per sequence position.  The call runs in the chunks of plan.hpp recover_chunk_end: per chunk k_recover_mul (a lane per
// member), the segmented sum (k_combsets_g2_sum at every level, level 0 over the products) and k_recover_finish, all on the caller's stream,
// then the chunk's status bytes come back (its synchronisation: the host table of the next chunk reuses the vector).
// ------------------------------------------------------------------------------------------
static_assert(sizeof(plan::rec_item) == 16, "k_recover_mul loads an item as one uint4");
// h_out192 / h_out96: the host form - the device outputs are then the chunk's own (grp.d_g2_out) and copied out chunk by chunk
static int recover_run(mi355_bls_ctx* c, const uint8_t* d_sigs, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k, const uint8_t* d_ids,
                       uint8_t* d_out192, uint8_t* d_out96, uint8_t* h_out192, uint8_t* h_out96, uint8_t* status, hipStream_t st) {
    const bool host_out = h_out192 || h_out96;
    if (!d_sigs || !offsets || !d_ids || !status || (!host_out && !d_out192 && !d_out96)) return MI355_BLS_ERR_ARG;
    if (((uintptr_t)d_sigs | (uintptr_t)d_idx | (uintptr_t)d_ids | (uintptr_t)d_out192 | (uintptr_t)d_out96) & 3) {
        g_err = "recover_signature_sets: signatures, indices, ids and outputs must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const plan::recover_plan rp = plan::recover_measure(offsets, k);
    if (!rp.ok) {
        g_err = "recover_signature_sets: offsets decrease, or 2^32 - 1 positions or groups, or more";
        return MI355_BLS_ERR_ARG;
    }
    if (!table_holds(d_idx, offsets, k, n_table, "recover_signature_sets: offsets[k] exceeds the number of signatures")) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (host_out) {
        if (int rc = c->grp.d_g2_out.reserve(rp.max_groups * 288, rp.max_groups * 72)) return rc;
    }
    std::vector<size_t> ro;
    int all = 1;
    for (size_t g0 = 0; g0 < k;) {
        const size_t g1 = plan::recover_chunk_end(offsets, k, g0), kc = g1 - g0, base = offsets[g0], m = offsets[g1] - base;
        ro.resize(kc + 1);
        for (size_t i = 0; i <= kc; i++) ro[i] = offsets[g0 + i] - base;
        const plan::aggsets_plan p = plan::aggsets_measure(ro.data(), kc);
        if (!p.ok) return MI355_BLS_ERR_ARG;           // cannot happen below 2^32 - 1 positions
        const plan::recover_sizes sz = plan::recover_sizes_for(p, m, kc);
        c->grp.items.resize(sz.tab / 4);
        uint32_t* tab = c->grp.items.data();
        const size_t t_items = m * 4, t_final = t_items + p.items * 4, t_len = t_final + kc;
        plan::recover_fill(offsets, g0, g1, reinterpret_cast<plan::rec_item*>(tab));
        plan::aggsets_fill(p, ro.data(), kc, reinterpret_cast<plan::agg_item*>(tab + t_items), tab + t_final);
        for (size_t i = 0; i < kc; i++) tab[t_len + i] = (uint32_t)(ro[i + 1] - ro[i]);
        // never beyond what the largest chunk needs; the previous chunk has drained the stream
        int rc = c->grp.d_g2_prod.reserve(sz.prod, sz.prod / 4);
        if (!rc) rc = c->grp.d_g2_part.reserve(sz.part, sz.part / 4);
        if (!rc) rc = grouped_upload(c, sz.tab, sz.flags, sz.status, st);
        if (rc) return rc;
        const uint4* items = reinterpret_cast<const uint4*>(c->grp.d_items.p);
        uint32_t *prod = c->grp.d_g2_prod, *part = c->grp.d_g2_part;
        if (m)
            k_recover_mul<<<plan::waves_for((uint32_t)m), WAVE, 0, st>>>(items, (uint32_t)m, reinterpret_cast<const uint32_t*>(d_sigs), n_table, d_idx,
                                                                        reinterpret_cast<const uint32_t*>(d_ids), (uint32_t)base, prod, c->grp.d_flag);
        launch_levels(p, items + m,      // one kernel at every level: level 0 sums the products, the levels above it the partials
                      [&](const uint4* it, uint32_t cnt) { k_combsets_g2_sum<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, prod, part); },
                      [&](const uint4* it, uint32_t cnt) { k_combsets_g2_sum<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, part, part); });
        uint8_t* o192 = host_out ? (h_out192 ? c->grp.d_g2_out.p : nullptr) : (d_out192 ? d_out192 + g0 * 192 : nullptr);
        uint8_t* o96 = host_out ? (h_out96 ? c->grp.d_g2_out.p + kc * 192 : nullptr) : (d_out96 ? d_out96 + g0 * 96 : nullptr);
        k_recover_finish<<<plan::waves_for((uint32_t)kc), WAVE, 0, st>>>(c->grp.d_items + t_final, c->grp.d_items + t_len, (uint32_t)kc, c->grp.d_g2_part, c->grp.d_flag,
                                                                        reinterpret_cast<uint32_t*>(o192), reinterpret_cast<uint32_t*>(o96), c->grp.d_status);
        HIPCHK(hipGetLastError());
        if (h_out192) HIPCHK(hipMemcpyAsync(h_out192 + g0 * 192, o192, kc * 192, hipMemcpyDeviceToHost, st));
        if (h_out96) HIPCHK(hipMemcpyAsync(h_out96 + g0 * 96, o96, kc * 96, hipMemcpyDeviceToHost, st));
        const int ok = grouped_status(c, kc, status + g0, st);
        if (ok < 0) return ok;
        all &= ok;
        g0 = g1;
    }
    return all;
}
extern "C" int mi355_bls_recover_signature_sets_device(mi355_bls_ctx* c, const void* d_sigs192, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                                       size_t k, const void* d_ids32, void* d_out_sigs192, void* d_out_sigs96, uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing recovered, nothing written
    return recover_run(c, (const uint8_t*)d_sigs192, n_table, d_idx, offsets, k, (const uint8_t*)d_ids32, (uint8_t*)d_out_sigs192, (uint8_t*)d_out_sigs96, nullptr,
                       nullptr, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_recover_signature_sets(mi355_bls_ctx* c, const void* sigs192, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                                const void* ids32, void* out_sigs192, void* out_sigs96, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!sigs192 || !offsets || !ids32 || !status || (!out_sigs192 && !out_sigs96) || !agg_offsets_ok(offsets, k)) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const uint8_t* d[3];      // signatures | ids | indices
    if (int rc = stage_inputs(c, {{sigs192, n_table * 192}, {ids32, offsets[k] * 32}, {idx, offsets[k] * 4}}, nullptr, d)) return rc;
    return recover_run(c, d[0], n_table, reinterpret_cast<const uint32_t*>(d[2]), offsets, k, d[1], nullptr, nullptr, (uint8_t*)out_sigs192, (uint8_t*)out_sigs96, status,
                       nullptr);
}

// ------------------------------------------------------------------------------------------
// Short linear combinations per group with the caller's scalars (mi355_bls_p1s_lincomb_many / mi355_bls_p2s_lincomb_many): the recovery's
// walk - chunks of whole groups (plan.hpp lincomb_chunk_end), per chunk a lane per term (k_lincomb_mul<F>, or k_lincomb_mul_psi under
// MI355_BLS_LINCOMB_SUBGROUP), the segmented sum over the products and k_lincomb_finish<F>, all on the caller's stream, then the chunk's
// status bytes come back (its synchronisation: the host table of the next chunk reuses the vector).
// ------------------------------------------------------------------------------------------
template <class F>
static bool lincomb_args_ok(size_t nbits, uint32_t flags) {
    const uint32_t known = sizeof(F) != sizeof(fp) ? (uint32_t)MI355_BLS_LINCOMB_SUBGROUP : 0u;
    if (nbits >= 1 && nbits <= 256 && !(flags & ~known)) return true;
    g_err = "lincomb_many: nbits is 1..256; the only flag is MI355_BLS_LINCOMB_SUBGROUP, on the p2s call";
    return false;
}
// h_out: the host form - the device output is then the chunk's own (grp.d_g2_out) and copied out chunk by chunk
template <class F>
static int lincomb_run(mi355_bls_ctx* c, const uint8_t* d_pts, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k, const uint8_t* d_sc,
                       size_t nbits, uint32_t flags, uint8_t* d_out, uint8_t* h_out, uint8_t* status, hipStream_t st) {
    constexpr bool G2 = sizeof(F) != sizeof(fp);
    constexpr size_t AFFB = G2 ? 192 : 96;
    if (!d_pts || !offsets || !d_sc || !status || (!h_out && !d_out) || !lincomb_args_ok<F>(nbits, flags)) return MI355_BLS_ERR_ARG;
    if (((uintptr_t)d_pts | (uintptr_t)d_idx | (uintptr_t)d_sc | (uintptr_t)d_out) & 3) {
        g_err = "lincomb_many: points, indices, scalars and outputs must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const plan::recover_plan rp = plan::lincomb_measure(offsets, k, c->lincomb_chunk);
    if (!rp.ok) {
        g_err = "lincomb_many: offsets decrease, or 2^32 - 1 positions or groups, or more";
        return MI355_BLS_ERR_ARG;
    }
    if (!table_holds(d_idx, offsets, k, n_table, "lincomb_many: offsets[k] exceeds the number of points")) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (h_out) {
        if (int rc = c->grp.d_g2_out.reserve(rp.max_groups * AFFB, rp.max_groups * AFFB / 4)) return rc;
    }
    const bool psi = G2 && (flags & MI355_BLS_LINCOMB_SUBGROUP);
    dev_buf<uint32_t>& prod_buf = G2 ? c->grp.d_g2_prod : c->grp.d_g1_prod;
    dev_buf<uint32_t>& part_buf = G2 ? c->grp.d_g2_part : c->grp.d_g1_part;
    std::vector<size_t> ro;
    int all = 1;
    for (size_t g0 = 0; g0 < k;) {
        const size_t g1 = plan::lincomb_chunk_end(offsets, k, g0, c->lincomb_chunk), kc = g1 - g0, base = offsets[g0], m = offsets[g1] - base;
        ro.resize(kc + 1);
        for (size_t i = 0; i <= kc; i++) ro[i] = offsets[g0 + i] - base;
        const plan::aggsets_plan p = plan::aggsets_measure(ro.data(), kc);
        if (!p.ok) return MI355_BLS_ERR_ARG;           // cannot happen below 2^32 - 1 positions
        const plan::lincomb_sizes sz = plan::lincomb_sizes_for(p, m, kc, G2);
        c->grp.items.resize(sz.tab / 4);
        uint32_t* tab = c->grp.items.data();
        const size_t t_items = m * 4, t_final = t_items + p.items * 4, t_len = t_final + kc;
        plan::recover_fill(offsets, g0, g1, reinterpret_cast<plan::rec_item*>(tab));
        plan::aggsets_fill(p, ro.data(), kc, reinterpret_cast<plan::agg_item*>(tab + t_items), tab + t_final);
        for (size_t i = 0; i < kc; i++) tab[t_len + i] = (uint32_t)(ro[i + 1] - ro[i]);
        // never beyond what the largest chunk needs; the previous chunk has drained the stream
        int rc = prod_buf.reserve(sz.prod, sz.prod / 4);
        if (!rc) rc = part_buf.reserve(sz.part, sz.part / 4);
        if (!rc) rc = grouped_upload(c, sz.tab, sz.flags, sz.status, st);
        if (rc) return rc;
        const uint4* items = reinterpret_cast<const uint4*>(c->grp.d_items.p);
        const uint32_t *pts = reinterpret_cast<const uint32_t*>(d_pts), *sc = reinterpret_cast<const uint32_t*>(d_sc);
        uint32_t *prod = prod_buf, *part = part_buf;
        if (m) {
            if constexpr (G2) {
                if (psi) k_lincomb_mul_psi<<<plan::waves_for((uint32_t)m), WAVE, 0, st>>>(items, (uint32_t)m, pts, n_table, d_idx, sc, (uint32_t)nbits, (uint32_t)base, prod, c->grp.d_flag);
                else k_lincomb_mul<fp2><<<plan::waves_for((uint32_t)m), WAVE, 0, st>>>(items, (uint32_t)m, pts, n_table, d_idx, sc, (uint32_t)nbits, (uint32_t)base, prod, c->grp.d_flag);
            } else {
                k_lincomb_mul<fp><<<plan::waves_for((uint32_t)m), WAVE, 0, st>>>(items, (uint32_t)m, pts, n_table, d_idx, sc, (uint32_t)nbits, (uint32_t)base, prod, c->grp.d_flag);
            }
        }
        const auto sum = [&](const uint4* it, uint32_t cnt, const uint32_t* src) {      // one kernel at every level: level 0 sums the products, the levels above it the partials
            if constexpr (G2) k_combsets_g2_sum<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, src, part);
            else k_lincomb_g1_sum<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, src, part);
        };
        launch_levels(p, items + m, [&](const uint4* it, uint32_t cnt) { sum(it, cnt, prod); }, [&](const uint4* it, uint32_t cnt) { sum(it, cnt, part); });
        uint8_t* o = h_out ? c->grp.d_g2_out.p : d_out + g0 * AFFB;
        k_lincomb_finish<F><<<plan::waves_for((uint32_t)kc), WAVE, 0, st>>>(c->grp.d_items + t_final, c->grp.d_items + t_len, (uint32_t)kc, part, c->grp.d_flag,
                                                                           reinterpret_cast<uint32_t*>(o), c->grp.d_status);
        HIPCHK(hipGetLastError());
        if (h_out) HIPCHK(hipMemcpyAsync(h_out + g0 * AFFB, o, kc * AFFB, hipMemcpyDeviceToHost, st));
        const int ok = grouped_status(c, kc, status + g0, st);
        if (ok < 0) return ok;
        all &= ok;
        g0 = g1;
    }
    return all;
}
template <class F>
static int lincomb_device(mi355_bls_ctx* c, const void* d_pts, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k, const void* d_sc, size_t nbits,
                          uint32_t flags, void* d_out, uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing computed, nothing written
    return lincomb_run<F>(c, (const uint8_t*)d_pts, n_table, d_idx, offsets, k, (const uint8_t*)d_sc, nbits, flags, (uint8_t*)d_out, nullptr, status, (hipStream_t)stream);
}
template <class F>
static int lincomb_host(mi355_bls_ctx* c, const void* pts, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k, const void* sc, size_t nbits,
                        uint32_t flags, void* out, uint8_t* status) {
    constexpr size_t AFFB = sizeof(F) == sizeof(fp) ? 96 : 192;
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!pts || !offsets || !sc || !status || !out || !agg_offsets_ok(offsets, k) || !lincomb_args_ok<F>(nbits, flags)) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const uint8_t* d[3];      // points | scalars | indices
    if (int rc = stage_inputs(c, {{pts, n_table * AFFB}, {sc, offsets[k] * 32}, {idx, offsets[k] * 4}}, nullptr, d)) return rc;
    return lincomb_run<F>(c, d[0], n_table, reinterpret_cast<const uint32_t*>(d[2]), offsets, k, d[1], nbits, flags, nullptr, (uint8_t*)out, status, nullptr);
}
extern "C" int mi355_bls_p1s_lincomb_many(mi355_bls_ctx* c, const void* points96, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                          const void* scalars32, size_t nbits, uint32_t flags, void* out96, uint8_t* status) {
    return lincomb_host<fp>(c, points96, n_table, idx, offsets, k, scalars32, nbits, flags, out96, status);
}
extern "C" int mi355_bls_p1s_lincomb_many_device(mi355_bls_ctx* c, const void* d_points96, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k,
                                                 const void* d_scalars32, size_t nbits, uint32_t flags, void* d_out96, uint8_t* status, void* stream) {
    return lincomb_device<fp>(c, d_points96, n_table, d_idx, offsets, k, d_scalars32, nbits, flags, d_out96, status, stream);
}
extern "C" int mi355_bls_p2s_lincomb_many(mi355_bls_ctx* c, const void* points192, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                          const void* scalars32, size_t nbits, uint32_t flags, void* out192, uint8_t* status) {
    return lincomb_host<fp2>(c, points192, n_table, idx, offsets, k, scalars32, nbits, flags, out192, status);
}
extern "C" int mi355_bls_p2s_lincomb_many_device(mi355_bls_ctx* c, const void* d_points192, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k,
                                                 const void* d_scalars32, size_t nbits, uint32_t flags, void* d_out192, uint8_t* status, void* stream) {
    return lincomb_device<fp2>(c, d_points192, n_table, d_idx, offsets, k, d_scalars32, nbits, flags, d_out192, status, stream);
}
// TEST HOOK: the terms per chunk of the following lincomb_many calls on this context (0: the plan's own)
extern "C" int mi355_bls_debug_lincomb_set_chunk(mi355_bls_ctx* c, size_t members) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->lincomb_chunk = members;
    return 0;
}

// ------------------------------------------------------------------------------------------
// Openings of k polynomials over Fr (mi355_bls_fr_open_many): passes of whole polynomials (plan.hpp fropen_sizes_for), per pass one workgroup
// per polynomial (k_fropen_coef, or k_fropen_eval over the domain k_fropen_domain has brought to Montgomery form once), all on the caller's
// stream, then the pass's status bytes come back (its synchronisation).  h_ys / h_quot: the host form - the device outputs are then the
// pass's own (d_fro_out: the values, then the quotients) and copied out pass by pass.  -> the polynomials with FROPEN_ST_REDUCED set.
// ------------------------------------------------------------------------------------------
static int fropen_run(mi355_bls_ctx* c, const uint8_t* d_polys, size_t n, const uint8_t* d_zs, size_t k, uint32_t flags, const uint8_t* d_domain, uint8_t* d_ys,
                      uint8_t* d_quot, uint8_t* h_ys, uint8_t* h_quot, uint8_t* status, hipStream_t st) {
    const bool eval = flags & MI355_BLS_FR_OPEN_EVAL;
    const plan::fropen_sizes sz = plan::fropen_sizes_for(n, k, eval, c->fropen_pass);
    if (!sz.ok) {
        g_err = "fr_open_many: n is at least 1; in evaluation form a power of two, at most 2^32";
        return MI355_BLS_ERR_ARG;
    }
    if (((uintptr_t)d_polys | (uintptr_t)d_zs | (uintptr_t)d_domain | (uintptr_t)d_ys | (uintptr_t)d_quot) & 3) {
        g_err = "fr_open_many: polynomials, points, domain and outputs must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const bool host = h_ys || h_quot;
    int rc = c->grp.d_status.reserve(sz.status, sz.status / 4);
    if (!rc && eval) rc = c->d_fro_ws.reserve(sz.domain + sz.scan, 0);
    if (!rc && host) rc = c->d_fro_out.reserve(sz.out_ys + (h_quot ? sz.out_quot : 0), 0);
    if (rc) return rc;
    const uint32_t *polys = reinterpret_cast<const uint32_t*>(d_polys), *zs = reinterpret_cast<const uint32_t*>(d_zs);
    uint32_t *ws_dom = c->d_fro_ws, *ws_scan = eval ? c->d_fro_ws + n * 8 : nullptr;
    fr ninv{};
    if (eval) {
        const uint32_t nw[8] = {(uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0, 0, 0, 0, 0, 0};
        ninv = fr_inv(fr_from_words(nw));
        k_fropen_domain<<<(unsigned)((n + FROPEN_LANES - 1) / FROPEN_LANES), FROPEN_LANES, 0, st>>>(reinterpret_cast<const uint32_t*>(d_domain), n, ws_dom);
    }
    std::vector<uint8_t> st_own;
    if (!status) st_own.resize(sz.per_pass);
    int reduced = 0;
    for (size_t p = 0; p < sz.passes; p++) {
        size_t g0, kc;
        plan::fropen_pass(sz, k, p, g0, kc);
        uint32_t* ys = host ? (h_ys ? c->d_fro_out.p : nullptr) : d_ys ? reinterpret_cast<uint32_t*>(d_ys) + g0 * 8 : nullptr;
        uint32_t* quot = host ? (h_quot ? c->d_fro_out.p + sz.out_ys / 4 : nullptr) : d_quot ? reinterpret_cast<uint32_t*>(d_quot) + g0 * n * 8 : nullptr;
        if (eval) k_fropen_eval<<<(unsigned)kc, FROPEN_LANES, 0, st>>>(polys + g0 * n * 8, n, sz.log2n, ws_dom, zs + g0 * 8, ninv, ws_scan, ys, quot, c->grp.d_status);
        else k_fropen_coef<<<(unsigned)kc, FROPEN_LANES, 0, st>>>(polys + g0 * n * 8, n, zs + g0 * 8, ys, quot, c->grp.d_status);
        HIPCHK(hipGetLastError());
        if (h_ys) HIPCHK(hipMemcpyAsync(h_ys + g0 * 32, ys, kc * 32, hipMemcpyDeviceToHost, st));
        if (h_quot) HIPCHK(hipMemcpyAsync(h_quot + g0 * n * 32, quot, kc * n * 32, hipMemcpyDeviceToHost, st));
        uint8_t* sb = status ? status + g0 : st_own.data();
        HIPCHK(hipMemcpyAsync(sb, c->grp.d_status, kc, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t i = 0; i < kc; i++) reduced += (sb[i] & FROPEN_ST_REDUCED) != 0;
    }
    return reduced;
}
static bool fropen_args_ok(const void* polys, size_t n, const void* zs, uint32_t flags, const void* domain, const void* ys, const void* quot, const uint8_t* status) {
    if (polys && zs && n && !(flags & ~(uint32_t)MI355_BLS_FR_OPEN_EVAL) && ((flags & MI355_BLS_FR_OPEN_EVAL) != 0) == (domain != nullptr) && (ys || quot || status))
        return true;
    g_err = "fr_open_many: NULL inputs, n == 0, every output NULL, a flag other than MI355_BLS_FR_OPEN_EVAL, or a domain without that flag (the flag without a domain)";
    return false;
}
extern "C" int mi355_bls_fr_open_many_device(mi355_bls_ctx* c, const void* d_polys32, size_t n, const void* d_zs32, size_t k, uint32_t flags, const void* d_domain32,
                                             void* d_out_ys32, void* d_out_quot32, uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing computed, nothing written
    if (!fropen_args_ok(d_polys32, n, d_zs32, flags, d_domain32, d_out_ys32, d_out_quot32, status)) return MI355_BLS_ERR_ARG;
    return fropen_run(c, (const uint8_t*)d_polys32, n, (const uint8_t*)d_zs32, k, flags, (const uint8_t*)d_domain32, (uint8_t*)d_out_ys32, (uint8_t*)d_out_quot32, nullptr,
                      nullptr, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_fr_open_many(mi355_bls_ctx* c, const void* polys32, size_t n, const void* zs32, size_t k, uint32_t flags, const void* domain32, uint8_t* out_ys32,
                                      uint8_t* out_quot32, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!fropen_args_ok(polys32, n, zs32, flags, domain32, out_ys32, out_quot32, status)) return MI355_BLS_ERR_ARG;
    if (!plan::fropen_sizes_for(n, k, flags & MI355_BLS_FR_OPEN_EVAL).ok) {
        g_err = "fr_open_many: in evaluation form n is a power of two, at most 2^32";
        return MI355_BLS_ERR_ARG;
    }
    if (!out_ys32 && !out_quot32) {
        g_err = "fr_open_many: the host form computes values or quotients";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const uint8_t* d[3];      // polynomials | points | domain
    if (int rc = stage_inputs(c, {{polys32, k * n * 32}, {zs32, k * 32}, {domain32, n * 32}}, nullptr, d)) return rc;
    return fropen_run(c, d[0], n, d[1], k, flags, d[2], nullptr, nullptr, out_ys32, out_quot32, status, nullptr);
}
// TEST HOOK: the polynomials per pass of the following fr_open_many calls on this context (0: the plan's own; it can only shorten a pass)
extern "C" int mi355_bls_debug_fropen_set_pass(mi355_bls_ctx* c, size_t polys_per_pass) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->fropen_pass = polys_per_pass;
    return 0;
}

// ------------------------------------------------------------------------------------------
// Transforms of k vectors over Fr (mi355_bls_fr_ntt_many): slices of whole vectors (plan.hpp frntt_sizes_for); per call the twiddle table
// (k_frntt_twiddle), per slice the passes (k_frntt_pass<DIT>) with the elementwise kernel in front of them (forward: the shift powers, or
// the copy of n = 1) or behind them (inverse: g^-j / n), all on the caller's stream, then the slice's status words come back (its
// synchronisation).  Which transform runs: frntt.hpp.  A transform whose last store permutes and that has more than one pass runs its
// earlier passes in a second buffer (d_ntt_io), so that the permuting pass never stores where another workgroup has yet to load.
// h_in / h_out: the host form - a slice is staged in d_ntt_io, transformed there and copied out.  -> the vectors with FRNTT_ST_REDUCED set.
// ------------------------------------------------------------------------------------------
static bool frntt_args_ok(const void* in, size_t n, uint32_t flags, const void* out) {
    if (in && out && n && !(n & (n - 1)) && n <= ((size_t)1 << 32) && !(flags & ~(uint32_t)(MI355_BLS_FR_NTT_INVERSE | MI355_BLS_FR_NTT_BITREV))) return true;
    g_err = "fr_ntt_many: NULL input or output, n that is no power of two in 1 .. 2^32, or a flag other than MI355_BLS_FR_NTT_INVERSE and MI355_BLS_FR_NTT_BITREV";
    return false;
}
template <bool DIT>
static int frntt_launch_pass(const frntt_geo& g, const uint32_t* src, bool raw, const uint32_t* tw, bool permute, uint32_t* dst, uint32_t* status, hipStream_t st) {
    const uint64_t wgs = frntt_workgroups(g);
    const size_t lds = (size_t)32 << g.L;
    if (wgs > 0x7fffffffu) {
        g_err = "fr_ntt_many: a pass of more than 2^31 - 1 workgroups";
        return MI355_BLS_ERR_ARG;
    }
    if (lds > (64u << 10)) HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(&k_frntt_pass<DIT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    k_frntt_pass<DIT><<<(unsigned)wgs, FRNTT_LANES, lds, st>>>(g, src, raw, tw, permute, dst, status);
    return 0;
}
static int frntt_run(mi355_bls_ctx* c, const uint8_t* d_in, const uint8_t* h_in, size_t n, size_t k, uint32_t flags, const uint8_t* shift32, uint8_t* d_out, uint8_t* h_out,
                     uint8_t* status, hipStream_t st) {
    const plan::frntt_sizes sz = plan::frntt_sizes_for(n, k, c->frntt_tile, c->frntt_vecs);
    if (!sz.ok) {
        g_err = "fr_ntt_many: n is a power of two, 1 .. 2^32";
        return MI355_BLS_ERR_ARG;
    }
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 3) {
        g_err = "fr_ntt_many: input and output must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    fr gm{};
    if (shift32) {
        uint32_t w[8];
        for (int i = 0; i < 8; i++) w[i] = (uint32_t)shift32[4 * i] | ((uint32_t)shift32[4 * i + 1] << 8) | ((uint32_t)shift32[4 * i + 2] << 16) | ((uint32_t)shift32[4 * i + 3] << 24);
        bool reduced;
        gm = fr_to_mont(fr_canon_words(w, reduced));
        if (fr_is_zero(gm)) {
            g_err = "fr_ntt_many: the shift is 0 mod r";
            return MI355_BLS_ERR_ARG;
        }
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const bool inverse = flags & MI355_BLS_FR_NTT_INVERSE, bitrev = flags & MI355_BLS_FR_NTT_BITREV, host = h_out != nullptr;
    const uint32_t m = sz.log2n;
    const bool dit = inverse && bitrev, permute = !bitrev, second = permute && sz.passes > 1;
    int rc = c->d_ntt_tw.reserve(sz.twiddles, 0);
    if (!rc) rc = c->d_ntt_st.reserve(sz.status, sz.status / 4);
    if (!rc) rc = c->d_ntt_io.reserve((host ? sz.staging : 0) + (second ? sz.staging : 0), 0);
    if (rc) return rc;
    fr root = frntt_omega(m);
    if (inverse) root = fr_inv(root);
    if (n > 1) {
        const uint64_t runs = (n / 2 + FRNTT_RUN - 1) / FRNTT_RUN;
        k_frntt_twiddle<<<(unsigned)((runs + FRNTT_LANES - 1) / FRNTT_LANES), FRNTT_LANES, 0, st>>>(root, n / 2, c->d_ntt_tw);
    }
    frntt_scale_args sa{};
    sa.m = m;
    if (inverse) {
        const uint32_t nw[8] = {(uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0, 0, 0, 0, 0, 0};
        sa.base = fr_inv(fr_from_words(nw));
        sa.ratio = shift32 ? fr_inv(gm) : fr_one();
        sa.mult = true, sa.use_ratio = shift32 != nullptr;
    } else {
        sa.base = fr_one(), sa.ratio = gm;
        sa.mult = sa.use_ratio = shift32 != nullptr;
    }
    const bool scale_first = !inverse && (shift32 || sz.passes == 0), scale_last = inverse;
    const uint64_t runs_per_vec = (n + FRNTT_RUN - 1) / FRNTT_RUN;
    std::vector<uint32_t> words(sz.vecs);
    int reduced = 0;
    for (size_t i = 0; i < sz.slices; i++) {
        size_t g0, kc;
        plan::frntt_slice(sz, k, i, g0, kc);
        uint32_t* io = c->d_ntt_io;
        const uint32_t* src = host ? io : reinterpret_cast<const uint32_t*>(d_in) + g0 * n * 8;
        uint32_t* out = host ? io : reinterpret_cast<uint32_t*>(d_out) + g0 * n * 8;
        uint32_t* mid = second ? io + (host ? sz.staging / 4 : 0) : out;
        if (host) HIPCHK(hipMemcpyAsync(io, h_in + g0 * n * 32, kc * n * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(c->d_ntt_st, 0, kc * 4, st));
        const unsigned scale_grid = (unsigned)((kc * runs_per_vec + FRNTT_LANES - 1) / FRNTT_LANES);
        sa.k = kc;
        bool raw = true;
        if (scale_first) {
            sa.raw = true;
            k_frntt_scale<<<scale_grid, FRNTT_LANES, 0, st>>>(sa, src, mid, c->d_ntt_st);
            src = mid, raw = false;
        }
        uint32_t done = 0;
        for (uint32_t p = 0; p < sz.passes; p++) {
            const uint32_t tp = sz.stages[p], sigma = dit ? done : m - done - tp;
            const plan::frntt_shape sh = plan::frntt_geo_for(m, sz.tile, sigma, tp, kc);
            const frntt_geo g{m, sigma, tp, sh.clo, sh.chi, sh.L, kc};
            const bool last = p + 1 == sz.passes;
            uint32_t* dst = last ? out : mid;
            rc = dit ? frntt_launch_pass<true>(g, src, raw, c->d_ntt_tw, false, dst, c->d_ntt_st, st)
                     : frntt_launch_pass<false>(g, src, raw, c->d_ntt_tw, permute && last, dst, c->d_ntt_st, st);
            if (rc) return rc;
            src = dst, raw = false, done += tp;
        }
        if (scale_last) {
            sa.raw = raw;
            k_frntt_scale<<<scale_grid, FRNTT_LANES, 0, st>>>(sa, src, out, c->d_ntt_st);
        }
        HIPCHK(hipGetLastError());
        if (host) HIPCHK(hipMemcpyAsync(h_out + g0 * n * 32, out, kc * n * 32, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(words.data(), c->d_ntt_st, kc * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t v = 0; v < kc; v++) {
            if (status) status[g0 + v] = (uint8_t)words[v];
            reduced += (words[v] & FRNTT_ST_REDUCED) != 0;
        }
    }
    return reduced;
}
extern "C" int mi355_bls_fr_ntt_many_device(mi355_bls_ctx* c, const void* d_in32, size_t n, size_t k, uint32_t flags, const uint8_t* shift32, void* d_out32,
                                            uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing computed, nothing written
    if (!frntt_args_ok(d_in32, n, flags, d_out32)) return MI355_BLS_ERR_ARG;
    return frntt_run(c, (const uint8_t*)d_in32, nullptr, n, k, flags, shift32, (uint8_t*)d_out32, nullptr, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_fr_ntt_many(mi355_bls_ctx* c, const void* in32, size_t n, size_t k, uint32_t flags, const uint8_t* shift32, uint8_t* out32, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!frntt_args_ok(in32, n, flags, out32)) return MI355_BLS_ERR_ARG;
    return frntt_run(c, nullptr, (const uint8_t*)in32, n, k, flags, shift32, nullptr, out32, status, nullptr);
}
// The domain both calls speak of: omega_n^i, or omega_n^rev_m(i) with BITREV, as n canonical images (k_frntt_domain); h_out: the host form,
// through d_ntt_io.  Both forms return after the stream has drained.
static int frntt_domain(mi355_bls_ctx* c, size_t n, uint32_t flags, uint8_t* d_out, uint8_t* h_out, hipStream_t st) {
    if (!c || !(d_out || h_out) || n == 0 || (n & (n - 1)) || n > ((size_t)1 << 32) || (flags & ~(uint32_t)MI355_BLS_FR_NTT_BITREV) || ((uintptr_t)d_out & 3)) {
        g_err = "fr_domain: a NULL context or output, n that is no power of two in 1 .. 2^32, a flag other than MI355_BLS_FR_NTT_BITREV, or a misaligned device pointer";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    if (h_out)
        if (int rc = c->d_ntt_io.reserve(n * 32, 0)) return rc;
    uint32_t* out = h_out ? c->d_ntt_io.p : reinterpret_cast<uint32_t*>(d_out);
    uint32_t m = 0;
    while (((size_t)1 << m) < n) m++;
    const uint64_t runs = (n + FRNTT_RUN - 1) / FRNTT_RUN;
    k_frntt_domain<<<(unsigned)((runs + FRNTT_LANES - 1) / FRNTT_LANES), FRNTT_LANES, 0, st>>>(frntt_omega(m), m, (flags & MI355_BLS_FR_NTT_BITREV) != 0, out);
    HIPCHK(hipGetLastError());
    if (h_out) HIPCHK(hipMemcpyAsync(h_out, out, n * 32, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
extern "C" int mi355_bls_fr_domain(mi355_bls_ctx* c, size_t n, uint32_t flags, uint8_t* out32) { return frntt_domain(c, n, flags, nullptr, out32, nullptr); }
extern "C" int mi355_bls_fr_domain_device(mi355_bls_ctx* c, size_t n, uint32_t flags, void* d_out32, void* stream) {
    return frntt_domain(c, n, flags, (uint8_t*)d_out32, nullptr, (hipStream_t)stream);
}
// TEST HOOKS: log2 of the tile (0: the plan's own; at most plan::FRNTT_TILE_MAX_LOG2) and the vectors per slice (0: the plan's own; it can
// only shorten a slice) of the following fr_ntt_many calls on this context
extern "C" int mi355_bls_debug_frntt_set_tile(mi355_bls_ctx* c, uint32_t log2_tile) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->frntt_tile = log2_tile;
    return 0;
}
extern "C" int mi355_bls_debug_frntt_set_pass(mi355_bls_ctx* c, size_t vectors_per_pass) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->frntt_vecs = vectors_per_pass;
    return 0;
}

// ------------------------------------------------------------------------------------------
// Transforms of k vectors of G1 points (mi355_bls_p1s_ntt_many): slices of whole vectors (plan.hpp p1ntt_sizes_for); per call the twiddle
// table (k_p1ntt_twiddle), per slice the m stages (k_p1ntt_stage<DIT>, the first reading the caller's images, all writing d_p1n_ws) and the
// finish (k_p1ntt_finish), all on the caller's stream, which is waited for once at the end.  Which transform runs: p1ntt.hpp.
// h_in / h_out: the host form - a slice is staged in d_p1n_io, transformed there and copied out, slice by slice.
// ------------------------------------------------------------------------------------------
static int p1ntt_run(mi355_bls_ctx* c, const uint8_t* d_in, const uint8_t* h_in, size_t n, size_t k, uint32_t flags, uint8_t* d_out, uint8_t* h_out, hipStream_t st) {
    const plan::p1ntt_sizes sz = plan::p1ntt_sizes_for(n, k, c->p1ntt_vecs);
    if (!(d_in || h_in) || !(d_out || h_out) || !sz.ok || (flags & ~(uint32_t)(MI355_BLS_P1S_NTT_INVERSE | MI355_BLS_P1S_NTT_BITREV))) {
        g_err = "p1s_ntt_many: NULL points or output, n that is no power of two in 1 .. 2^32, or a flag other than MI355_BLS_P1S_NTT_INVERSE and MI355_BLS_P1S_NTT_BITREV";
        return MI355_BLS_ERR_ARG;
    }
    if (((uintptr_t)d_in | (uintptr_t)d_out) & 3) {
        g_err = "p1s_ntt_many: points and output must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    const bool inverse = flags & MI355_BLS_P1S_NTT_INVERSE, bitrev = flags & MI355_BLS_P1S_NTT_BITREV, host = h_out != nullptr;
    const uint32_t m = sz.log2n;
    const bool dit = inverse && bitrev, permute = !bitrev;
    int rc = c->d_p1n_tw.reserve(sz.twiddles, 0);
    if (!rc && m) rc = c->d_p1n_ws.reserve(sz.ws, 0);
    if (!rc && host) rc = c->d_p1n_io.reserve(sz.staging, 0);
    if (rc) return rc;
    p1ntt_stage g{};
    g.m = m;
    if (m) {
        fr root = frntt_omega(m);
        if (inverse) root = fr_inv(root);
        const uint64_t runs = (n / 2 + FRNTT_RUN - 1) / FRNTT_RUN;
        k_p1ntt_twiddle<<<(unsigned)((runs + FRNTT_LANES - 1) / FRNTT_LANES), FRNTT_LANES, 0, st>>>(root, n / 2, c->d_p1n_tw);
    }
    if (inverse) {
        const uint32_t nw[8] = {(uint32_t)n, (uint32_t)((uint64_t)n >> 32), 0, 0, 0, 0, 0, 0};
        g.s_mont = fr_inv(fr_from_words(nw));
        fr_to_words(g.s, g.s_mont);
    }
    for (size_t i = 0; i < sz.slices; i++) {
        size_t g0, kc;
        plan::p1ntt_slice(sz, k, i, g0, kc);
        const plan::p1ntt_launch l = plan::p1ntt_launch_for(sz, kc);
        const uint32_t* src = host ? c->d_p1n_io.p : reinterpret_cast<const uint32_t*>(d_in + g0 * n * 96);
        uint32_t* out = host ? c->d_p1n_io.p : reinterpret_cast<uint32_t*>(d_out + g0 * n * 96);
        if (host) HIPCHK(hipMemcpyAsync(c->d_p1n_io, h_in + g0 * n * 96, kc * n * 96, hipMemcpyHostToDevice, st));
        g.k = kc;
        for (uint32_t s = 0; s < m; s++) {
            g.b = dit ? s : m - 1 - s;
            g.scaled = inverse && g.b == m - 1;
            const uint32_t* in_aff = s == 0 ? src : nullptr;
            if (dit) k_p1ntt_stage<true><<<l.stage_grid, WAVE, 0, st>>>(g, in_aff, c->d_p1n_ws, c->d_p1n_tw);
            else k_p1ntt_stage<false><<<l.stage_grid, WAVE, 0, st>>>(g, in_aff, c->d_p1n_ws, c->d_p1n_tw);
        }
        k_p1ntt_finish<<<l.finish_grid, WAVE, 0, st>>>(m ? c->d_p1n_ws.p : src, m == 0, (uint64_t)kc << m, m, permute, l.run, out);
        HIPCHK(hipGetLastError());
        if (host) {
            HIPCHK(hipMemcpyAsync(h_out + g0 * n * 96, out, kc * n * 96, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    if (!host) HIPCHK(hipStreamSynchronize(st));
    return 0;
}
extern "C" int mi355_bls_p1s_ntt_many_device(mi355_bls_ctx* c, const void* d_points96, size_t n, size_t k, uint32_t flags, void* d_out96, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing computed, nothing written
    return p1ntt_run(c, (const uint8_t*)d_points96, nullptr, n, k, flags, (uint8_t*)d_out96, nullptr, (hipStream_t)stream);
}
extern "C" int mi355_bls_p1s_ntt_many(mi355_bls_ctx* c, const void* points96, size_t n, size_t k, uint32_t flags, void* out96) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    return p1ntt_run(c, nullptr, (const uint8_t*)points96, n, k, flags, nullptr, (uint8_t*)out96, nullptr);
}
// TEST HOOK: the vectors per slice of the following p1s_ntt_many calls on this context (0: the plan's own; it can only shorten a slice)
extern "C" int mi355_bls_debug_p1ntt_set_pass(mi355_bls_ctx* c, size_t vectors_per_pass) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->p1ntt_vecs = vectors_per_pass;
    return 0;
}

// ------------------------------------------------------------------------------------------
// All openings of k polynomials over the n-th roots of unity (mi355_bls_fk20_open_all_many): csrc/fk20.hpp's route.  The setup handle is one
// p1ntt_run of 2n points (forward, BITREV, in place in the handle's memory).  A call makes its three twiddle tables once, then per pass of
// whole polynomials (plan.hpp fk20_sizes_for): the layout (k_fk20_circ), the Fr transform's forward passes in place (k_frntt_pass<false>,
// frntt_sizes_for's tile and stages for 2n), the pointwise product (k_fk20_pointwise), the m + 1 DIT stages of the inverse
// (k_p1ntt_stage<true>), the m DIF stages of the forward (k_fk20_stage) unless MI355_BLS_FK20_H, and the finish (k_fk20_finish), all on the
// caller's stream; then the pass's status words come back (its synchronisation).  h_polys / h_out: the host form, staged pass by pass.
// -> the polynomials with FK20_ST_REDUCED set.
// ------------------------------------------------------------------------------------------
static_assert(plan::FK20_CIRC_RUN == FRNTT_RUN && plan::FK20_CIRC_LANES == FRNTT_LANES, "fk20_launch_for counts k_fk20_circ's lanes");
extern "C" size_t mi355_bls_fk20_setup_sizeof(size_t n) { return plan::fk20_setup_bytes(n); }
extern "C" void mi355_bls_fk20_setup_destroy(mi355_bls_fk20_setup* s) { delete s; }
extern "C" int mi355_bls_fk20_setup_create_device(mi355_bls_ctx* c, mi355_bls_fk20_setup** out, const void* d_srs96, size_t n, void* stream) {
    if (!c || !out || !d_srs96 || !plan::fk20_sizes_for(n, 1).ok || ((uintptr_t)d_srs96 & 3)) {
        g_err = "fk20_setup_create: a NULL argument, n that is no power of two in 1 .. 2^31, or a misaligned device pointer";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    std::unique_ptr<mi355_bls_fk20_setup> s(new mi355_bls_fk20_setup());
    s->device = c->device, s->n = n;
    if (int rc = s->x.alloc(plan::fk20_setup_bytes(n))) return rc;
    k_fk20_setup_layout<<<(unsigned)((2 * n + FRNTT_LANES - 1) / FRNTT_LANES), FRNTT_LANES, 0, st>>>(reinterpret_cast<const uint32_t*>(d_srs96), n, s->x);
    HIPCHK(hipGetLastError());
    if (int rc = p1ntt_run(c, reinterpret_cast<const uint8_t*>(s->x.p), nullptr, 2 * n, 1, MI355_BLS_P1S_NTT_BITREV, reinterpret_cast<uint8_t*>(s->x.p), nullptr, st)) return rc;
    *out = s.release();
    return 0;
}
// host array -> staging -> create_device on the null stream
extern "C" int mi355_bls_fk20_setup_create(mi355_bls_ctx* c, mi355_bls_fk20_setup** out, const void* srs96, size_t n) {
    if (!c || !out || !srs96 || !plan::fk20_sizes_for(n, 1).ok) {
        g_err = "fk20_setup_create: a NULL argument, or n that is no power of two in 1 .. 2^31";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const uint8_t* d[1];
    if (int rc = stage_inputs(c, {{srs96, n * 96}}, nullptr, d)) return rc;
    return mi355_bls_fk20_setup_create_device(c, out, d[0], n, nullptr);
}
static int fk20_run(mi355_bls_ctx* c, const mi355_bls_fk20_setup* setup, const uint8_t* d_polys, const uint8_t* h_polys, size_t k, uint32_t flags, uint8_t* d_out,
                    uint8_t* h_out, uint8_t* status, hipStream_t st) {
    if (!setup || !(d_polys || h_polys) || !(d_out || h_out) || (flags & ~(uint32_t)(MI355_BLS_FK20_BITREV | MI355_BLS_FK20_H)) || setup->device != c->device) {
        g_err = "fk20_open_all_many: a NULL setup, polynomials or output, a flag other than MI355_BLS_FK20_BITREV and MI355_BLS_FK20_H, or a setup of another device";
        return MI355_BLS_ERR_ARG;
    }
    if (((uintptr_t)d_polys | (uintptr_t)d_out) & 3) {
        g_err = "fk20_open_all_many: polynomials and output must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (setup->cell != 1) {
        g_err = "fk20_open_all_many: the setup was made for cells (mi355_bls_fk20_setup_create_cells with cell > 1)";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const size_t n = setup->n;
    const plan::fk20_sizes sz = plan::fk20_sizes_for(n, k, c->fk20_polys);
    const plan::frntt_sizes fsz = plan::frntt_sizes_for(2 * n, sz.per_pass, c->frntt_tile, 0);
    if (!sz.ok || !fsz.ok) return MI355_BLS_ERR_ARG;           // a handle holds no such n
    HIPCHK(hipSetDevice(c->device));
    const bool want_h = flags & MI355_BLS_FK20_H, host = h_out != nullptr;
    const bool permute = !want_h && !(flags & MI355_BLS_FK20_BITREV);
    const uint32_t m = sz.log2n, M = m + 1;
    int rc = c->d_ntt_tw.reserve(sz.tw_fr, 0);
    if (!rc) rc = c->d_ntt_st.reserve(sz.status, sz.status / 4);
    if (!rc) rc = c->d_ntt_io.reserve(sz.scalars + (host ? sz.polys : 0), 0);
    if (!rc) rc = c->d_p1n_tw.reserve(sz.tw_inv + sz.tw_fwd, 0);
    if (!rc) rc = c->d_p1n_ws.reserve(sz.ws, 0);
    if (!rc && host) rc = c->d_p1n_io.reserve(sz.out, 0);
    if (rc) return rc;
    uint32_t* const tw_inv = c->d_p1n_tw;
    uint32_t* const tw_fwd = tw_inv + sz.tw_inv / 4;
    uint32_t* const scal = c->d_ntt_io;
    uint32_t* const staged = scal + sz.scalars / 4;
    {
        const fr w2n = frntt_omega(M);
        const unsigned grid = (unsigned)(((n + FRNTT_RUN - 1) / FRNTT_RUN + FRNTT_LANES - 1) / FRNTT_LANES);
        k_frntt_twiddle<<<grid, FRNTT_LANES, 0, st>>>(w2n, n, c->d_ntt_tw);
        k_p1ntt_twiddle<<<grid, FRNTT_LANES, 0, st>>>(fr_inv(w2n), n, tw_inv);
        if (n > 1) k_p1ntt_twiddle<<<(unsigned)(((n / 2 + FRNTT_RUN - 1) / FRNTT_RUN + FRNTT_LANES - 1) / FRNTT_LANES), FRNTT_LANES, 0, st>>>(frntt_omega(m), n / 2, tw_fwd);
    }
    const uint32_t n2w[8] = {(uint32_t)(2 * (uint64_t)n), (uint32_t)((2 * (uint64_t)n) >> 32), 0, 0, 0, 0, 0, 0};
    const fr inv2n = fr_inv(fr_from_words(n2w));
    std::vector<uint32_t> words(sz.per_pass);
    int reduced = 0;
    for (size_t p = 0; p < sz.passes; p++) {
        size_t g0, kc;
        plan::fk20_pass(sz, k, p, g0, kc);
        const plan::fk20_launch l = plan::fk20_launch_for(sz, kc);
        const uint32_t* src = host ? staged : reinterpret_cast<const uint32_t*>(d_polys + g0 * n * 32);
        uint32_t* out = host ? c->d_p1n_io.p : reinterpret_cast<uint32_t*>(d_out + g0 * n * 96);
        if (host) HIPCHK(hipMemcpyAsync(staged, h_polys + g0 * n * 32, kc * n * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(c->d_ntt_st, 0, kc * 4, st));
        k_fk20_circ<<<l.circ_grid, FRNTT_LANES, 0, st>>>(m, kc, inv2n, src, scal, c->d_ntt_st);
        uint32_t done = 0;
        for (uint32_t q = 0; q < fsz.passes; q++) {
            const uint32_t tp = fsz.stages[q], sigma = M - done - tp;
            const plan::frntt_shape sh = plan::frntt_geo_for(M, fsz.tile, sigma, tp, kc);
            const frntt_geo g{M, sigma, tp, sh.clo, sh.chi, sh.L, kc};
            if ((rc = frntt_launch_pass<false>(g, scal, false, c->d_ntt_tw, false, scal, c->d_ntt_st, st))) return rc;
            done += tp;
        }
        k_fk20_pointwise<<<l.point_grid, WAVE, 0, st>>>((uint64_t)kc << M, ((uint64_t)1 << M) - 1, scal, setup->x, c->d_p1n_ws);
        p1ntt_stage g{};
        g.k = kc, g.m = M;
        for (uint32_t b = 0; b < M; b++) {
            g.b = b;
            k_p1ntt_stage<true><<<l.inv_grid, WAVE, 0, st>>>(g, nullptr, c->d_p1n_ws, tw_inv);
        }
        g.m = m;
        for (uint32_t s = 0; s < m && !want_h; s++) {
            g.b = m - 1 - s;
            k_fk20_stage<<<l.fwd_grid, WAVE, 0, st>>>(g, c->d_p1n_ws, tw_fwd);
        }
        k_fk20_finish<<<l.finish_grid, WAVE, 0, st>>>(c->d_p1n_ws, (uint64_t)kc << m, m, permute, l.run, out);
        HIPCHK(hipGetLastError());
        if (host) HIPCHK(hipMemcpyAsync(h_out + g0 * n * 96, out, kc * n * 96, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(words.data(), c->d_ntt_st, kc * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t v = 0; v < kc; v++) {
            if (status) status[g0 + v] = (uint8_t)words[v];
            reduced += (words[v] & FK20_ST_REDUCED) != 0;
        }
    }
    return reduced;
}
extern "C" int mi355_bls_fk20_open_all_many_device(mi355_bls_ctx* c, const mi355_bls_fk20_setup* setup, const void* d_polys32, size_t k, uint32_t flags, void* d_out96,
                                                   uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing computed, nothing written
    return fk20_run(c, setup, (const uint8_t*)d_polys32, nullptr, k, flags, (uint8_t*)d_out96, nullptr, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_fk20_open_all_many(mi355_bls_ctx* c, const mi355_bls_fk20_setup* setup, const void* polys32, size_t k, uint32_t flags, void* out96,
                                            uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    return fk20_run(c, setup, nullptr, (const uint8_t*)polys32, k, flags, nullptr, (uint8_t*)out96, status, nullptr);
}
// ------------------------------------------------------------------------------------------
// The proofs of all cells of k polynomials (mi355_bls_fk20_open_cells_many): csrc/fk20cells.hpp's route.  The setup handle for cells of l
// points: the l vectors s^(v) laid out one after the other in the point transform's staging (k_fk20c_setup_layout), one p1ntt_run of l
// vectors of 2q points (forward, BITREV, in place), and k_fk20c_setup_place into the handle; l == 1 is fk20_setup_create's own path.  A
// call makes its three twiddle tables once, then per pass of whole polynomials (plan.hpp fk20_cells_sizes_for): the layout (k_fk20c_circ),
// the Fr transform's forward passes of 2q over count x l vectors in place, the products (k_fk20c_pointwise), the levels of the sum
// (k_fk20c_sum), the inverse's stages (k_p1ntt_stage<true> where a vector is 2q images wide, k_fk20c_stage<true> where it is wider), and
// unless MI355_BLS_FK20_H the padding (k_fk20c_pad) and the forward's stages (k_fk20c_stage<false>); then the finish (k_fk20c_finish), all
// on the caller's stream; then the pass's status words come back (its synchronisation).  -> the polynomials with FK20_ST_REDUCED set.
// ------------------------------------------------------------------------------------------
static_assert(plan::FK20_CELLS_FAN_LOG2 == FK20C_FAN_LOG2, "fk20_cells_sum_lanes counts k_fk20c_sum's lanes");
extern "C" int mi355_bls_fk20_setup_create_cells_device(mi355_bls_ctx* c, mi355_bls_fk20_setup** out, const void* d_srs96, size_t n, size_t cell, void* stream) {
    const plan::fk20_cells_sizes sz = plan::fk20_cells_sizes_for(n, cell, 0, 1);
    if (!c || !out || !d_srs96 || !sz.ok || ((uintptr_t)d_srs96 & 3)) {
        g_err = "fk20_setup_create_cells: a NULL argument, n that is no power of two in 1 .. 2^31, a cell that is no power of two in 1 .. n, or a misaligned device pointer";
        return MI355_BLS_ERR_ARG;
    }
    if (cell == 1) return mi355_bls_fk20_setup_create_device(c, out, d_srs96, n, stream);
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    std::unique_ptr<mi355_bls_fk20_setup> s(new mi355_bls_fk20_setup());
    s->device = c->device, s->n = n, s->cell = cell;
    if (int rc = s->x.alloc(plan::fk20_setup_bytes(n))) return rc;
    dev_buf<uint32_t> tmp;                               // the l vectors before and after the transform, a second 2n x 96 bytes until create
                                                         // returns; p1ntt_run waits for the stream
    if (int rc = tmp.alloc(plan::fk20_setup_bytes(n))) return rc;
    const unsigned grid = (unsigned)((2 * n + FRNTT_LANES - 1) / FRNTT_LANES);
    k_fk20c_setup_layout<<<grid, FRNTT_LANES, 0, st>>>(reinterpret_cast<const uint32_t*>(d_srs96), 2 * (uint64_t)n, sz.log2q, sz.log2cell, tmp);
    HIPCHK(hipGetLastError());
    if (int rc = p1ntt_run(c, reinterpret_cast<const uint8_t*>(tmp.p), nullptr, 2 * (n / cell), cell, MI355_BLS_P1S_NTT_BITREV, reinterpret_cast<uint8_t*>(tmp.p), nullptr, st)) return rc;
    k_fk20c_setup_place<<<grid, FRNTT_LANES, 0, st>>>(tmp, 2 * (uint64_t)n, sz.log2q, sz.log2cell, s->x);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    *out = s.release();
    return 0;
}
// host array -> staging -> create_cells_device on the null stream
extern "C" int mi355_bls_fk20_setup_create_cells(mi355_bls_ctx* c, mi355_bls_fk20_setup** out, const void* srs96, size_t n, size_t cell) {
    if (!c || !out || !srs96 || !plan::fk20_cells_sizes_for(n, cell, 0, 1).ok) {
        g_err = "fk20_setup_create_cells: a NULL argument, n that is no power of two in 1 .. 2^31, or a cell that is no power of two in 1 .. n";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const uint8_t* d[1];
    if (int rc = stage_inputs(c, {{srs96, n * 96}}, nullptr, d)) return rc;
    return mi355_bls_fk20_setup_create_cells_device(c, out, d[0], n, cell, nullptr);
}
static int fk20_cells_run(mi355_bls_ctx* c, const mi355_bls_fk20_setup* setup, const uint8_t* d_polys, const uint8_t* h_polys, size_t k, size_t ext_log2, uint32_t flags,
                          uint8_t* d_out, uint8_t* h_out, uint8_t* status, hipStream_t st) {
    if (!setup || !(d_polys || h_polys) || !(d_out || h_out) || (flags & ~(uint32_t)(MI355_BLS_FK20_BITREV | MI355_BLS_FK20_H)) || setup->device != c->device) {
        g_err = "fk20_open_cells_many: a NULL setup, polynomials or output, a flag other than MI355_BLS_FK20_BITREV and MI355_BLS_FK20_H, or a setup of another device";
        return MI355_BLS_ERR_ARG;
    }
    if (((uintptr_t)d_polys | (uintptr_t)d_out) & 3) {
        g_err = "fk20_open_cells_many: polynomials and output must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    const size_t n = setup->n;
    const plan::fk20_cells_sizes sz = plan::fk20_cells_sizes_for(n, setup->cell, ext_log2, k, c->fk20_polys);
    if (!sz.ok) {
        g_err = "fk20_open_cells_many: ext_log2 with n 2^ext_log2 above 2^32";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const uint32_t mq = sz.log2q, cl = sz.log2cell, M = mq + 1, a = sz.log2cells, w = sz.log2w;
    const size_t q = (size_t)1 << mq, cells = (size_t)1 << a;
    const plan::frntt_sizes fsz = plan::frntt_sizes_for(2 * q, sz.per_pass << cl, c->frntt_tile, 0);
    if (!fsz.ok) {                                               // a handle holds no such n
        g_err = "fk20_open_cells_many: the Fr transform refuses the length 2n / cell";
        return MI355_BLS_ERR_ARG;
    }
    HIPCHK(hipSetDevice(c->device));
    const bool want_h = flags & MI355_BLS_FK20_H, host = h_out != nullptr;
    const bool permute = !want_h && !(flags & MI355_BLS_FK20_BITREV);
    const size_t rows = want_h ? q : cells;                      // the images a polynomial gives
    int rc = c->d_ntt_tw.reserve(sz.tw_fr, 0);
    if (!rc) rc = c->d_ntt_st.reserve(sz.status, sz.status / 4);
    if (!rc) rc = c->d_ntt_io.reserve(sz.scalars + (host ? sz.polys : 0), 0);
    if (!rc) rc = c->d_p1n_tw.reserve(sz.tw_inv + sz.tw_fwd, 0);
    if (!rc) rc = c->d_p1n_ws.reserve(sz.ws + sz.prod, 0);
    if (!rc && host) rc = c->d_p1n_io.reserve(sz.out, 0);
    if (rc) return rc;
    uint32_t* const tw_inv = c->d_p1n_tw;
    uint32_t* const tw_fwd = tw_inv + sz.tw_inv / 4;
    uint32_t* const scal = c->d_ntt_io;
    uint32_t* const staged = scal + sz.scalars / 4;
    uint32_t* const ws = c->d_p1n_ws;
    uint32_t* const prod = ws + sz.ws / 4;
    {
        const fr w2q = frntt_omega(M);
        const unsigned grid = (unsigned)(((q + FRNTT_RUN - 1) / FRNTT_RUN + FRNTT_LANES - 1) / FRNTT_LANES);
        k_frntt_twiddle<<<grid, FRNTT_LANES, 0, st>>>(w2q, q, c->d_ntt_tw);
        k_p1ntt_twiddle<<<grid, FRNTT_LANES, 0, st>>>(fr_inv(w2q), q, tw_inv);
        if (cells > 1 && !want_h)
            k_p1ntt_twiddle<<<(unsigned)(((cells / 2 + FRNTT_RUN - 1) / FRNTT_RUN + FRNTT_LANES - 1) / FRNTT_LANES), FRNTT_LANES, 0, st>>>(frntt_omega(a), cells / 2, tw_fwd);
    }
    const uint32_t q2w[8] = {(uint32_t)(2 * (uint64_t)q), (uint32_t)((2 * (uint64_t)q) >> 32), 0, 0, 0, 0, 0, 0};
    const fr inv2q = fr_inv(fr_from_words(q2w));
    const uint32_t levels = plan::fk20_cells_sum_levels(sz);
    std::vector<uint32_t> words(sz.per_pass);
    int reduced = 0;
    for (size_t p = 0; p < sz.passes; p++) {
        size_t g0, kc;
        plan::fk20_cells_pass(sz, k, p, g0, kc);
        const plan::fk20_cells_launch l = plan::fk20_cells_launch_for(sz, kc);
        const uint32_t* src = host ? staged : reinterpret_cast<const uint32_t*>(d_polys + g0 * n * 32);
        uint32_t* out = host ? c->d_p1n_io.p : reinterpret_cast<uint32_t*>(d_out + g0 * rows * 96);
        if (host) HIPCHK(hipMemcpyAsync(staged, h_polys + g0 * n * 32, kc * n * 32, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(c->d_ntt_st, 0, kc * 4, st));
        k_fk20c_circ<<<l.circ_grid, FRNTT_LANES, 0, st>>>(mq, cl, kc, inv2q, src, scal, c->d_ntt_st);
        const size_t vecs = kc << cl;
        uint32_t done = 0;
        for (uint32_t i = 0; i < fsz.passes; i++) {
            const uint32_t tp = fsz.stages[i], sigma = M - done - tp;
            const plan::frntt_shape sh = plan::frntt_geo_for(M, fsz.tile, sigma, tp, vecs);
            const frntt_geo g{M, sigma, tp, sh.clo, sh.chi, sh.L, vecs};
            if ((rc = frntt_launch_pass<false>(g, scal, false, c->d_ntt_tw, false, scal, c->d_ntt_st, st))) return rc;
            done += tp;
        }
        k_fk20c_pointwise<<<l.point_grid, WAVE, 0, st>>>((uint64_t)kc << (sz.log2n + 1), mq, cl, scal, setup->x, prod);
        for (uint32_t t = 0; t < levels; t++) {
            const uint64_t lanes = plan::fk20_cells_sum_lanes(sz, kc, t);
            k_fk20c_sum<<<(unsigned)((lanes + WAVE - 1) / WAVE), WAVE, 0, st>>>(lanes, t * FK20C_FAN_LOG2, fk20c_level_bits(cl, t), prod, t + 1 == levels, M, w, ws);
        }
        p1ntt_stage g{};
        g.k = kc, g.m = M;
        for (uint32_t b = 0; b < M; b++) {
            g.b = b;
            if (w == M) k_p1ntt_stage<true><<<l.inv_grid, WAVE, 0, st>>>(g, nullptr, ws, tw_inv);
            else k_fk20c_stage<true><<<l.inv_grid, WAVE, 0, st>>>(g, w, ws, tw_inv);
        }
        if (!want_h) {
            if (l.pad_grid) k_fk20c_pad<<<l.pad_grid, WAVE, 0, st>>>((uint64_t)kc << a, mq, a, w, ws);
            g.m = a;
            for (uint32_t s = 0; s < a; s++) {
                g.b = a - 1 - s;
                k_fk20c_stage<false><<<l.fwd_grid, WAVE, 0, st>>>(g, w, ws, tw_fwd);
            }
            k_fk20c_finish<<<l.finish_grid, WAVE, 0, st>>>(ws, (uint64_t)kc << a, a, w, permute, l.run, out);
        } else {
            k_fk20c_finish<<<l.finish_h_grid, WAVE, 0, st>>>(ws, (uint64_t)kc << mq, mq, w, false, l.run_h, out);
        }
        HIPCHK(hipGetLastError());
        if (host) HIPCHK(hipMemcpyAsync(h_out + g0 * rows * 96, out, kc * rows * 96, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(words.data(), c->d_ntt_st, kc * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t v = 0; v < kc; v++) {
            if (status) status[g0 + v] = (uint8_t)words[v];
            reduced += (words[v] & FK20_ST_REDUCED) != 0;
        }
    }
    return reduced;
}
extern "C" int mi355_bls_fk20_open_cells_many_device(mi355_bls_ctx* c, const mi355_bls_fk20_setup* setup, const void* d_polys32, size_t k, size_t ext_log2,
                                                     uint32_t flags, void* d_out96, uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing computed, nothing written
    return fk20_cells_run(c, setup, (const uint8_t*)d_polys32, nullptr, k, ext_log2, flags, (uint8_t*)d_out96, nullptr, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_fk20_open_cells_many(mi355_bls_ctx* c, const mi355_bls_fk20_setup* setup, const void* polys32, size_t k, size_t ext_log2, uint32_t flags,
                                              void* out96, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    return fk20_cells_run(c, setup, nullptr, (const uint8_t*)polys32, k, ext_log2, flags, nullptr, (uint8_t*)out96, status, nullptr);
}
// TEST HOOK: the polynomials per pass of the following fk20 calls - all openings and cells - on this context (0: the plan's own; it can only
// shorten a pass)
extern "C" int mi355_bls_debug_fk20_set_pass(mi355_bls_ctx* c, size_t polys_per_pass) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->fk20_polys = polys_per_pass;
    return 0;
}

// The two decoders, k_deser's halves: Signature.fromBytes (bls_sig_io.nim:42-58) for n signatures without key or message, PublicKey.fromBytes (:81-121)
// for n keys without signature or message.  The device form leaves the images in device memory (n x 192 bytes; n x 96, the key table every
// table-addressed call takes) and brings the status bytes to the host; 1 when every status is 0.  refused: the other decoder's DESER_F_* bit.
using deser_kernel = void (*)(const uint8_t*, uint32_t, uint32_t, uint32_t*, uint8_t*, uint32_t*);
static int deser_rows_device(mi355_bls_ctx* c, deser_kernel kernel, uint32_t refused, const void* d_wire, size_t n, uint32_t dflags, void* d_out, uint8_t* status,
                             hipStream_t st) {
    if (!c || dflags > 7 || (dflags & refused)) return MI355_BLS_ERR_ARG;
    if (n == 0) return 1;
    if (!d_wire || !d_out || n > plan::POP_MAX_KEYS || ((uintptr_t)d_out & 3)) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    if (int rc = io_reserve(c, n)) return rc;                     // the status bytes' device buffer
    HIPCHK(hipSetDevice(c->device));
    return status_pass(c, st, n, status, nullptr, nullptr, [&] {
        kernel<<<plan::waves_for((uint32_t)n), WAVE, 0, st>>>((const uint8_t*)d_wire, (uint32_t)n, dflags, (uint32_t*)d_out, c->d_status, c->d_flags);
    });
}
// wire: the column the host's bytes wait in, as wide as an image; uncompressed: the DESER_F_* bit under which a row on the wire is that wide, not half
static int deser_rows_host(mi355_bls_ctx* c, deser_kernel kernel, uint32_t refused, plan::row_col wire, uint32_t uncompressed, const uint8_t* in, size_t n,
                           uint32_t dflags, void* out, uint8_t* status) {
    if (!c || dflags > 7 || (dflags & refused)) return MI355_BLS_ERR_ARG;
    if (n == 0) return 1;
    if (!in || n > plan::POP_MAX_KEYS) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    if (int rc = io_reserve(c, n)) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(col_at(c, wire), in, n * ((dflags & uncompressed) ? wire.width : wire.width / 2), hipMemcpyHostToDevice, nullptr));
    int rc = deser_rows_device(c, kernel, refused, col_at(c, wire), n, dflags, c->d_sets, status, nullptr);
    if (rc < 0) return rc;
    if (out) HIPCHK(hipMemcpy(out, c->d_sets, n * wire.width, hipMemcpyDeviceToHost));
    return rc;
}
extern "C" int mi355_bls_deserialize_signatures_device(mi355_bls_ctx* c, const void* d_sigs, size_t n, uint32_t dflags, void* d_out_sigs192, uint8_t* status,
                                                       void* stream) {
    return deser_rows_device(c, k_deser_sigs, DESER_F_PK_UNCOMPRESSED, d_sigs, n, dflags, d_out_sigs192, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_deserialize_signatures(mi355_bls_ctx* c, const uint8_t* sigs, size_t n, uint32_t dflags, void* out_sigs192, uint8_t* status) {
    return deser_rows_host(c, k_deser_sigs, DESER_F_PK_UNCOMPRESSED, cols::DSIG_WIRE, DESER_F_SIG_UNCOMPRESSED, sigs, n, dflags, out_sigs192, status);
}
extern "C" int mi355_bls_deserialize_public_keys_device(mi355_bls_ctx* c, const void* d_pks, size_t n, uint32_t dflags, void* d_out_pks96, uint8_t* status,
                                                        void* stream) {
    return deser_rows_device(c, k_deser_pks, DESER_F_SIG_UNCOMPRESSED, d_pks, n, dflags, d_out_pks96, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_deserialize_public_keys(mi355_bls_ctx* c, const uint8_t* pks, size_t n, uint32_t dflags, void* out_pks96, uint8_t* status) {
    return deser_rows_host(c, k_deser_pks, DESER_F_SIG_UNCOMPRESSED, cols::DPK_WIRE, DESER_F_PK_UNCOMPRESSED, pks, n, dflags, out_pks96, status);
}

// ------------------------------------------------------------------------------------------
// Key admission: PublicKey.fromBytes, Signature.fromBytes and popVerify (bls_sig_io.nim:42-58, 81-99; bls_sig_min_pubkey.nim:60-74) for n
// (key, proof) rows on the wire, one status byte per row.  Both columns are decoded where they stand (k_deser_pks, k_deser_sigs); the status
// bytes come to the host; the rows both decoders accepted (plan::admit_survivors) are packed into popVerify records through a device list of
// their row numbers (k_admit_records) and only they run the blinded batch check and, if it fails, the per-pair pass (locate_run, pop): a row
// that does not decode costs the others nothing.  The verdicts go back to their rows (plan::admit_merge) and the refused rows whose key had
// decoded are zeroed in the table on the device (k_admit_zero_rows).  What a row holds in the staging buffers meanwhile: plan.hpp cols::ADMIT_*.
// ------------------------------------------------------------------------------------------
// d_pks | d_proofs: device memory, wire form; d_out: n x 96 B of device memory; the staging buffers hold n rows (io_reserve)
static int admit_run(mi355_bls_ctx* c, const uint8_t* d_pks, const uint8_t* d_proofs, size_t n, uint32_t dflags, const uint8_t rnd[32], uint32_t* d_out,
                     uint8_t* status, hipStream_t st) {
    uint32_t* d_prf = reinterpret_cast<uint32_t*>(col_at(c, cols::ADMIT_PROOFS));
    uint32_t* d_list = reinterpret_cast<uint32_t*>(col_at(c, cols::ADMIT_LIST));
    uint8_t* d_pst = col_at(c, cols::ADMIT_PROOF_ST);
    const uint32_t n32 = (uint32_t)n;
    std::vector<uint8_t> key_st(n), proof_st(n);
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 12, st));
    k_deser_pks<<<plan::waves_for(n32), WAVE, 0, st>>>(d_pks, n32, dflags & DESER_F_PK_UNCOMPRESSED, d_out, c->d_status, c->d_flags);
    k_deser_sigs<<<plan::waves_for(n32), WAVE, 0, st>>>(d_proofs, n32, dflags & DESER_F_SIG_UNCOMPRESSED, d_prf, d_pst, c->d_flags);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(key_st.data(), c->d_status, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(proof_st.data(), d_pst, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<uint32_t> list(n);
    const size_t m = plan::admit_survivors(key_st.data(), proof_st.data(), n, list.data());
    std::vector<uint8_t> verdicts(m);
    if (m) {                                   // no survivor: no pairing work at all
        HIPCHK(hipMemcpyAsync(d_list, list.data(), m * 4, hipMemcpyHostToDevice, st));
        k_admit_records<<<plan::gather_blocks_for(m * 80), plan::GATHER_THREADS, 0, st>>>(d_out, d_prf, d_list, m, reinterpret_cast<uint32_t*>(c->d_sets.p));
        HIPCHK(hipGetLastError());
        const int rc = locate_run(c, c->d_sets, nullptr, m, rnd, verdicts.data(), st, true);      // sliced by max_sets like every pop call
        if (rc < 0) return rc;
    }
    std::vector<uint32_t> zero(n);
    const size_t nz = plan::admit_merge(key_st.data(), proof_st.data(), n, list.data(), verdicts.data(), m, status, zero.data());
    if (nz) {                                  // the key decoder left an image in these rows
        HIPCHK(hipMemcpyAsync(d_list, zero.data(), nz * 4, hipMemcpyHostToDevice, st));
        k_admit_zero_rows<<<plan::gather_blocks_for(nz * 24), plan::GATHER_THREADS, 0, st>>>(d_list, nz, d_out);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    int all = 1;
    for (size_t i = 0; i < n; i++) all &= status[i] == 0;
    return all;
}
static int admit_args(mi355_bls_ctx* c, const void* pks, const void* proofs, size_t n, uint32_t dflags, const uint8_t rnd[32], const uint8_t* status) {
    if (!c || !rnd || !status || dflags > 7 || (dflags & DESER_F_KNOWN_ON_CURVE)) return MI355_BLS_ERR_ARG;      // admission is the full check
    if (n == 0) return 1;
    if (!pks || !proofs || n > plan::POP_MAX_KEYS) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    return 0;
}
extern "C" int mi355_bls_admit_keys_device(mi355_bls_ctx* c, const void* d_pks, const void* d_proofs, size_t n, uint32_t dflags, const uint8_t rnd[32],
                                           void* d_out_pks96, uint8_t* status, void* stream) {
    if (int rc = admit_args(c, d_pks, d_proofs, n, dflags, rnd, status)) return rc;
    if (!d_out_pks96 || ((uintptr_t)d_out_pks96 & 3)) return MI355_BLS_ERR_ARG;
    if (int rc = io_reserve(c, n)) return rc;
    HIPCHK(hipSetDevice(c->device));
    return admit_run(c, (const uint8_t*)d_pks, (const uint8_t*)d_proofs, n, dflags, rnd, (uint32_t*)d_out_pks96, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_admit_keys(mi355_bls_ctx* c, const uint8_t* pks, const uint8_t* proofs, size_t n, uint32_t dflags, const uint8_t rnd[32], void* out_pks96,
                                    uint8_t* status) {
    if (int rc = admit_args(c, pks, proofs, n, dflags, rnd, status)) return rc;
    if (int rc = io_reserve(c, n)) return rc;
    HIPCHK(hipSetDevice(c->device));
    // the wire forms wait in the record buffer: the decoders have read them before the gather writes there
    uint8_t *d_wk = col_at(c, cols::ADMIT_WIRE_KEYS), *d_wp = col_at(c, cols::ADMIT_WIRE_PROOFS), *d_keys = col_at(c, cols::ADMIT_KEYS);
    HIPCHK(hipMemcpyAsync(d_wk, pks, n * ((dflags & DESER_F_PK_UNCOMPRESSED) ? 96 : 48), hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(d_wp, proofs, n * ((dflags & DESER_F_SIG_UNCOMPRESSED) ? 192 : 96), hipMemcpyHostToDevice, nullptr));
    const int rc = admit_run(c, d_wk, d_wp, n, dflags, rnd, reinterpret_cast<uint32_t*>(d_keys), status, nullptr);
    if (rc < 0) return rc;
    if (out_pks96) HIPCHK(hipMemcpy(out_pks96, d_keys, n * 96, hipMemcpyDeviceToHost));
    return rc;
}

// ------------------------------------------------------------------------------------------
// Same-message pre-aggregation: MultiSignatureSet.combine (bls_batch_verifier.nim:47-106, core :570-647) for k groups of SignatureSet records
// in one device pass.  Group g = positions [offsets[g], offsets[g + 1]) of the member sequence (the record table itself, or table entries
// picked by index: the addressing of aggregate_sets) becomes ONE record - key sum [s_j]PK_j, the members' message, signature sum [s_j]S_j,
// s_j from the chain seeded with rnds[g] - and a status byte.  Per member two 64-bit multiplications, per group two segmented sums over
// the plan's item tables and a finish lane (kernels.hip, csrc/combsets.hpp); the key side on the caller's stream, the signature side on
// the context's fork stream beside it.  The scalars and the random bytes are cleared on the device before the call returns.
// ------------------------------------------------------------------------------------------
// combination of k > 0 groups enqueued on st: records at d_out, status bytes in c->grp.d_status
static int combsets_enqueue(mi355_bls_ctx* c, const uint8_t* d_sets, size_t n_sets, const uint32_t* d_idx, const size_t* offsets, size_t k, const uint8_t* rnds,
                            uint8_t* d_out, hipStream_t st) {
    if (!d_sets || !offsets || !rnds || !d_out) return MI355_BLS_ERR_ARG;
    if (((uintptr_t)d_sets | (uintptr_t)d_idx | (uintptr_t)d_out) & 3) {
        g_err = "combine_sets: records and indices must be 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    const plan::combsets_plan cp = plan::combsets_measure(offsets, k);
    if (!cp.ok) {
        g_err = "combine_sets: offsets decrease, or more than 2^26 members or 2^32 - 2 groups";
        return MI355_BLS_ERR_ARG;
    }
    if (!table_holds(d_idx, offsets, k, n_sets, "combine_sets: offsets[k] exceeds the number of records")) return MI355_BLS_ERR_ARG;
    const size_t N = cp.members;
    std::vector<size_t> rel(k + 1);
    for (size_t g = 0; g <= k; g++) rel[g] = offsets[g] - cp.lo;
    const plan::aggsets_plan p = plan::aggsets_measure(rel.data(), k);
    if (!p.ok) {
        g_err = "combine_sets: too many members";
        return MI355_BLS_ERR_ARG;
    }
    HIPCHK(hipSetDevice(c->device));
    // item table | final_of | first position | length of every group
    c->grp.items.resize(p.items * 4 + 3 * k);
    uint32_t *h_final = c->grp.items.data() + p.items * 4, *h_first = h_final + k, *h_len = h_first + k;
    plan::aggsets_fill(p, rel.data(), k, reinterpret_cast<plan::agg_item*>(c->grp.items.data()), h_final);
    for (size_t g = 0; g < k; g++) h_first[g] = (uint32_t)rel[g], h_len[g] = (uint32_t)(rel[g + 1] - rel[g]);
    const size_t n1 = N ? N : 1, it1 = p.items ? p.items : 1, stride = (n1 + 63) / 64 * 64, tcap = cp.chunk_cap ? cp.chunk_cap : WAVE;
    int rc = c->grp.d_g1_part.reserve(it1 * (size_t)G1W * 4, it1 * (size_t)G1W);
    if (!rc) rc = c->grp.d_g2_part.reserve(it1 * (size_t)G2W * 4, it1 * (size_t)G2W);
    if (!rc) rc = c->d_comb_s.reserve(n1 * 8, n1 * 2);
    if (!rc) rc = c->d_comb_rnd.reserve(k * 32, k * 8);
    if (!rc) rc = c->d_comb_P.reserve(stride * 3 * 64, stride * 48);
    if (!rc) rc = c->grp.d_g2_prod.reserve(n1 * (size_t)G2W * 4, n1 * (size_t)G2W);
    if (!rc) rc = c->d_comb_pktab.reserve(tcap * PKTAB_BYTES, 0);
    if (!rc) rc = c->d_comb_g2tab.reserve(tcap * 8 * 6 * 64, 0);
    if (!rc) rc = c->d_comb_pkflag.reserve(4, 0);
    if (!rc && d_idx) rc = c->d_comb_gather.reserve(n1 * 320, n1 * 80);
    if (!rc) rc = grouped_upload(c, c->grp.items.size() * 4, k * 4, k, st);
    if (rc) return rc;
    const size_t P_stride = c->d_comb_P.bytes / (3 * 64), g2tcap = c->d_comb_g2tab.bytes / (8 * 6 * 64);      // what the buffers hold (they may be larger than this call needs)
    uint32_t *g1_part = c->grp.d_g1_part, *g2_part = c->grp.d_g2_part;
    HIPCHK(hipMemcpyAsync(c->d_comb_rnd, rnds, k * 32, hipMemcpyHostToDevice, st));
    const uint4* items = reinterpret_cast<const uint4*>(c->grp.d_items.p);
    const uint32_t *d_final = c->grp.d_items + p.items * 4, *d_first = d_final + k, *d_len = d_first + k;
    const uint32_t* idx = d_idx ? d_idx + cp.lo : nullptr;
    const uint32_t* recs = reinterpret_cast<const uint32_t*>(d_sets) + (d_idx ? 0 : cp.lo * 80);
    const uint32_t k32 = (uint32_t)k, N32 = (uint32_t)N;
    if (N) {
        if (idx) {
            k_combsets_gather<<<plan::gather_blocks_for(N * 80), plan::GATHER_THREADS, 0, st>>>(reinterpret_cast<const uint32_t*>(d_sets), n_sets, idx, N32, c->d_comb_gather);
            recs = c->d_comb_gather;
        }
        k_combsets_scalars<<<plan::waves_for(k32), WAVE, 0, st>>>(d_first, d_len, k32, c->d_comb_rnd, plan::COMB_CHAIN_LANE_MAX, c->d_comb_s);
        if (cp.host_chains) {                    // the long groups' chains, walked here while the device walks the others'
            c->comb_s_h.clear();
            size_t total = 0;
            for (size_t g = 0; g < k; g++)
                if (plan::combsets_chain_on_host(h_len[g])) total += h_len[g];
            c->comb_s_h.resize(total);
            size_t at = 0;
            for (size_t g = 0; g < k; g++) {
                if (!plan::combsets_chain_on_host(h_len[g])) continue;
                uint64_t* o = c->comb_s_h.data() + at;
                combsets_chain(rnds + g * 32, h_len[g], [&](size_t j, uint64_t v) { o[j] = v; });
                HIPCHK(hipMemcpyAsync(c->d_comb_s + h_first[g], o, (size_t)h_len[g] * 8, hipMemcpyHostToDevice, st));
                at += h_len[g];
            }
        }
        // fork: the signature side on the context's first fork stream, the key side here
        hipStream_t s2 = ensure_side(c) ? (hipStream_t)c->side : st;
        if (s2 != st) {
            HIPCHK(hipEventRecord(c->ev[0], st));
            HIPCHK(hipStreamWaitEvent(s2, c->ev[0], 0));
        }
        for (size_t a = 0; a < N; a += plan::COMB_MUL_CHUNK) {
            const uint32_t m = (uint32_t)(N - a < plan::COMB_MUL_CHUNK ? N - a : plan::COMB_MUL_CHUNK);
            k_combsets_g2mul<<<plan::waves_for(m), WAVE, 0, s2>>>(recs + a * 80, m, c->d_comb_s + a, c->d_comb_g2tab, g2tcap, c->grp.d_g2_prod + a * (size_t)G2W);
        }
        launch_levels(p, items,      // one kernel at every level: level 0 sums the products, the levels above it the partials
                      [&](const uint4* it, uint32_t cnt) { k_combsets_g2_sum<<<plan::waves_for(cnt), WAVE, 0, s2>>>(it, cnt, c->grp.d_g2_prod, g2_part); },
                      [&](const uint4* it, uint32_t cnt) { k_combsets_g2_sum<<<plan::waves_for(cnt), WAVE, 0, s2>>>(it, cnt, g2_part, g2_part); });
        if (s2 != st) HIPCHK(hipEventRecord(c->ev[2], s2));
        HIPCHK(hipMemsetAsync(c->d_comb_pkflag, 0, 4, st));
        for (size_t a = 0; a < N; a += plan::COMB_MUL_CHUNK) {
            const uint32_t m = (uint32_t)(N - a < plan::COMB_MUL_CHUNK ? N - a : plan::COMB_MUL_CHUNK);
            k_pkmul<<<plan::waves_for(m), WAVE, 0, st>>>(reinterpret_cast<const uint8_t*>(recs + a * 80), m, c->d_comb_s + a, c->d_comb_P + a, P_stride, c->d_comb_pkflag,
                                                         c->d_comb_pktab);
        }
        launch_levels(p, items,
                      [&](const uint4* it, uint32_t cnt) {
                          k_combsets_g1_l0<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, c->d_comb_P, P_stride, recs, idx, n_sets, d_first, g1_part, c->grp.d_flag);
                      },
                      [&](const uint4* it, uint32_t cnt) { k_aggsets_ln<<<plan::waves_for(cnt), WAVE, 0, st>>>(it, cnt, g1_part); });
        if (s2 != st) HIPCHK(hipStreamWaitEvent(st, c->ev[2], 0));
    }
    k_combsets_finish<<<plan::waves_for(k32), WAVE, 0, st>>>(d_final, d_first, d_len, k32, c->grp.d_g1_part, c->grp.d_g2_part, c->grp.d_flag, recs, idx, n_sets,
                                                             reinterpret_cast<uint32_t*>(d_out), c->grp.d_status);
    HIPCHK(hipGetLastError());
    // the scalars are blinding material: nothing of them stays on the device
    if (N) HIPCHK(hipMemsetAsync(c->d_comb_s, 0, N * 8, st));
    HIPCHK(hipMemsetAsync(c->d_comb_rnd, 0, k * 32, st));
    return 0;
}
// host records (and indices) -> the staged inputs
static int combsets_stage(mi355_bls_ctx* c, const void* sets, size_t n_sets, const uint32_t* idx, const size_t* offsets, size_t k, hipStream_t st,
                          const uint8_t** d_sets, const uint32_t** d_idx) {
    if (!sets || !offsets || !agg_offsets_ok(offsets, k)) return MI355_BLS_ERR_ARG;
    const uint8_t* d[2];
    if (int rc = stage_inputs(c, {{sets, n_sets * 320}, {idx, offsets[k] * 4}}, st, d)) return rc;
    *d_sets = d[0], *d_idx = reinterpret_cast<const uint32_t*>(d[1]);
    return 0;
}
extern "C" int mi355_bls_combine_sets_device(mi355_bls_ctx* c, const void* d_sets, size_t n_sets, const uint32_t* d_idx, const size_t* offsets, size_t k,
                                             const uint8_t* rnds, void* d_out_records, uint8_t* status, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;                      // nothing combined, nothing written
    if (!status) return MI355_BLS_ERR_ARG;
    int rc = combsets_enqueue(c, (const uint8_t*)d_sets, n_sets, d_idx, offsets, k, rnds, (uint8_t*)d_out_records, (hipStream_t)stream);
    if (rc) return rc;
    return grouped_status(c, k, status, (hipStream_t)stream);
}
extern "C" int mi355_bls_combine_sets(mi355_bls_ctx* c, const void* sets, size_t n_sets, const uint32_t* idx, const size_t* offsets, size_t k, const uint8_t* rnds,
                                      void* out_records, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    if (!out_records || !status) return MI355_BLS_ERR_ARG;
    const uint8_t* d_sets;
    const uint32_t* d_idx;
    if (int rc = combsets_stage(c, sets, n_sets, idx, offsets, k, nullptr, &d_sets, &d_idx)) return rc;
    return records_to_host(c, k, out_records, status,
                           [&](uint8_t* d_out, hipStream_t st) { return combsets_enqueue(c, d_sets, n_sets, d_idx, offsets, k, rnds, d_out, st); });
}
// batchVerify over the k combined records (records_batch)
extern "C" int mi355_bls_batch_verify_combined_device(mi355_bls_ctx* c, const void* d_sets, size_t n_sets, const uint32_t* d_idx, const size_t* offsets, size_t k,
                                                      const uint8_t* rnds, const uint8_t rnd[32], void* stream) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    return records_batch(c, k, rnd, (hipStream_t)stream, [&](uint8_t* d_out, hipStream_t st) {
        return combsets_enqueue(c, (const uint8_t*)d_sets, n_sets, d_idx, offsets, k, rnds, d_out, st);
    });
}
extern "C" int mi355_bls_batch_verify_combined(mi355_bls_ctx* c, const void* sets, size_t n_sets, const uint32_t* idx, const size_t* offsets, size_t k,
                                               const uint8_t* rnds, const uint8_t rnd[32]) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (k == 0) return 0;
    const uint8_t* d_sets;
    const uint32_t* d_idx;
    if (int rc = combsets_stage(c, sets, n_sets, idx, offsets, k, nullptr, &d_sets, &d_idx)) return rc;
    return records_batch(c, k, rnd, nullptr, [&](uint8_t* d_out, hipStream_t st) { return combsets_enqueue(c, d_sets, n_sets, d_idx, offsets, k, rnds, d_out, st); });
}
// Host only, no GPU: the records of a flat batch grouped by their 32-byte message, stably - groups in the order their message first appears,
// members in input order.  idx: n positions, offsets: n + 1 entries of which k + 1 are written.
extern "C" int mi355_bls_group_by_message(const void* sets, size_t n, uint32_t* idx, size_t* offsets, size_t* k) {
    if (!offsets || !k || (n && (!sets || !idx)) || n >= 0xffffffffu) return MI355_BLS_ERR_ARG;
    const uint8_t* b = (const uint8_t*)sets;
    std::unordered_map<std::string, uint32_t> group_of;
    std::vector<uint32_t> of(n), count;
    for (size_t i = 0; i < n; i++) {
        const auto it = group_of.emplace(std::string((const char*)b + i * 320 + 96, 32), (uint32_t)count.size());
        if (it.second) count.push_back(0);
        of[i] = it.first->second;
        count[of[i]]++;
    }
    offsets[0] = 0;
    for (size_t g = 0; g < count.size(); g++) offsets[g + 1] = offsets[g] + count[g];
    std::vector<size_t> cur(offsets, offsets + count.size());
    for (size_t i = 0; i < n; i++) idx[cur[of[i]]++] = (uint32_t)i;
    *k = count.size();
    return 0;
}

// ------------------------------------------------------------------------------------------
// Many independent batches in ONE device pass.  A host that verifies many SMALL batches (a few thousand sets each: one per block or
// gossip aggregate) cannot fill the chip with one of them, and the number of HIP hardware queues caps how many calls run side by
// side (DESIGN.md section 4, "Other rows").  Here the k batches are verified as the union of their tuples with every tuple keeping
// the blinding scalar it has in its OWN batch (its own secureRandomBytes, its own chain partition, batchVerify's dispatch rule per
// batch): the merged product is the product of the k batch products, so it is one iff every batch verifies - up to the 2^-64 of
// the random linear combination, which is the reference's own soundness bound for ONE batch.  If the merged check passes, every
// verdict is true (the common case, at whole-chip throughput); if it fails, the batches are verified one by one to find the
// culprits - the optimistic scheme clients already wrap around batchVerify.  Verdicts are exactly those of k separate calls.
// ------------------------------------------------------------------------------------------
// The merged pass over the union of `total` > 0 sets, where it may run: *passed = the union's product is one and no key is at infinity.
// It does not run (and *passed stays false) when two non-empty batches carry the same random bytes, when the union exceeds the workspace or
// when k > 65 536.  0, or a negative error.
static int many_merged_pass(mi355_bls_ctx* c, const uint8_t* d_src, const uint8_t* h_src, const size_t counts[], const uint8_t* rnds, size_t k, size_t total,
                            hipStream_t st, bool* passed) {
    bool merged_ok = false;
    *passed = false;
    // The merged check is sound only if the batches' blinding scalars are independent.  They are a deterministic SHA-256 chain of
    // (rnd_b, chain id): two batches with the SAME secureRandomBytes and the same count get identical r_i at identical indices, and a
    // forger who knows that can make errors cancel across them (sig + D at index i of one, sig' - D at index i of the other: the
    // merged product is 1, both verdicts would be true, while k separate calls reject both).  A host that reuses one rnd for all its
    // batches is a plausible mistake and harmless with separate calls, so it must be harmless here: any two equal rnds among the
    // non-empty batches -> no merged pass, the batches are verified one by one.
    bool rnds_distinct = true;
    {
        std::vector<const uint8_t*> rs;
        for (size_t b = 0; b < k; b++)
            if (counts[b]) rs.push_back(rnds + 32 * b);
        std::sort(rs.begin(), rs.end(), [](const uint8_t* x, const uint8_t* y) { return memcmp(x, y, 32) < 0; });
        for (size_t i = 1; i < rs.size(); i++)
            if (memcmp(rs[i - 1], rs[i], 32) == 0) rnds_distinct = false;
    }
    if (rnds_distinct && total <= c->cap && k <= 65536) {
        // ---- merged pass
        std::vector<many_meta> meta;
        std::vector<uint8_t> rr;
        uint32_t lanes = 0;
        size_t first = 0;
        c->h_r.assign(total, 0);
        bool any_serial = false;
        for (size_t b = 0; b < k; b++) {
            size_t nb_ = counts[b];
            if (nb_ == 0) continue;                               // an empty batch is false by itself and takes no part
            const bool parallel = c->num_threads > 1 && nb_ >= 3; // batchVerify's dispatch (bls_batch_verifier.nim:440)
            if (parallel) {
                uint32_t B = (uint32_t)(nb_ < c->num_threads ? nb_ : c->num_threads);
                meta.push_back(many_meta{first, nb_, B, lanes});
                rr.insert(rr.end(), rnds + 32 * b, rnds + 32 * b + 32);
                lanes += B;
            } else {
                host_serial_chain(rnds + 32 * b, nb_, c->h_r.data() + first);
                any_serial = true;
            }
            first += nb_;
        }
        {   // meta and the per-batch random bytes ride in the wire-format staging buffer (unused on this path)
            int rcr = io_reserve(c, (meta.size() * (sizeof(many_meta) + 32) + 64 + 319) / 320 + 1);
            if (rcr) return rcr;
        }
        const uint8_t* d_sets = d_src;
        if (!d_sets) {
            HIPCHK(hipMemcpyAsync(c->d_sets, h_src, total * 320, hipMemcpyHostToDevice, st));
            d_sets = c->d_sets;
        }
        HIPCHK(hipMemsetAsync(c->d_flags, 0, 12, st));
        HIPCHK(hipEventRecord(c->ev[0], st));
        if (any_serial) HIPCHK(hipMemcpyAsync(c->d_r, c->h_r.data(), total * 8, hipMemcpyHostToDevice, st));      // serial batches' scalars (zeros elsewhere, overwritten below)
        if (lanes) {
            many_meta* d_meta = reinterpret_cast<many_meta*>(c->d_comp.p);
            uint8_t* d_rr = c->d_comp + ((meta.size() * sizeof(many_meta) + 63) / 64) * 64;
            HIPCHK(hipMemcpyAsync(d_meta, meta.data(), meta.size() * sizeof(many_meta), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_rr, rr.data(), rr.size(), hipMemcpyHostToDevice, st));
            k_blind_many<<<plan::waves_for(lanes), WAVE, 0, st>>>(d_rr, d_meta, (uint32_t)meta.size(), lanes, c->d_r);
        }
        int rc = run_pairs(c, d_sets, total, st);
        if (rc) return rc;
        launch_k_tail(c, st, c->d_L, c->d_states, 1, 2, c->d_gt, c->d_flags + 1, 144, 0);
        HIPCHK(hipEventRecord(c->ev[8], st));
        uint32_t fl[2];
        HIPCHK(hipMemcpyAsync(fl, c->d_flags, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));                         // also: meta / rr / h_r (host vectors) have been consumed
        c->have_gt = true;
        c->gt_is_fv = false;
        (void)collect_timings(c, 7);
        merged_ok = fl[0] == 0 && fl[1] == 1;
    }
    *passed = merged_ok;
    return 0;
}
// the arguments every k-batch call checks, its verdicts cleared: the sets of the call, or a negative error
static int many_args(mi355_bls_ctx* c, const uint8_t* d_src, const uint8_t* h_src, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                     size_t* total) {
    if (!c || !counts || !rnds || !verdicts || (!d_src && !h_src)) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    *total = 0;
    for (size_t b = 0; b < k; b++) {
        verdicts[b] = 0;
        *total += counts[b];
    }
    return 0;
}
// every non-empty batch verified: 1 iff there is no empty one
static int many_all_pass(const size_t counts[], size_t k, uint8_t verdicts[]) {
    int all = 1;
    for (size_t b = 0; b < k; b++) {
        verdicts[b] = counts[b] ? 1 : 0;
        all &= verdicts[b];
    }
    return all;
}
static int verify_many(mi355_bls_ctx* c, const uint8_t* d_src, const uint8_t* h_src, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                       hipStream_t st) {
    size_t total = 0;
    if (int rc = many_args(c, d_src, h_src, counts, rnds, k, verdicts, &total)) return rc;
    if (total == 0) return 0;                                     // every batch empty: every verdict false (bls_batch_verifier.nim:137-139)
    HIPCHK(hipSetDevice(c->device));
    bool merged_ok = false;
    if (int rc = many_merged_pass(c, d_src, h_src, counts, rnds, k, total, st, &merged_ok)) return rc;
    if (merged_ok) return many_all_pass(counts, k, verdicts);
    // ---- some batch fails (or the union exceeds the workspace): one by one, exactly as k separate batchVerify calls
    int all = 1;
    size_t first = 0;
    for (size_t b = 0; b < k; b++) {
        size_t nb_ = counts[b];
        int v = 0;
        if (nb_) {
            const int serial = (c->num_threads > 1 && nb_ >= 3) ? 0 : 1;
            v = verify_common(c, d_src ? d_src + 320 * first : nullptr, d_src ? nullptr : h_src + 320 * first, nb_, rnds + 32 * b, serial, st);
            if (v < 0) return v;
        }
        verdicts[b] = (uint8_t)v;
        all &= v;
        first += nb_;
    }
    return all;
}
extern "C" int mi355_bls_batch_verify_many(mi355_bls_ctx* c, const void* sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[]) {
    return verify_many(c, nullptr, (const uint8_t*)sets, counts, rnds, k, verdicts, nullptr);
}
extern "C" int mi355_bls_batch_verify_many_device(mi355_bls_ctx* c, const void* d_sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                                                  void* stream) {
    return verify_many(c, (const uint8_t*)d_sets, nullptr, counts, rnds, k, verdicts, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------
// Per-batch verdicts for many batches in ONE device pass: what verify_many's fallback finds with k single-batch calls.  Batch b is one group
// of the per-group path (aggveach_run): its pairs are ([r_i]PK_i, H(m_i)), r_i the scalar set i has in its own batch (k_blind_many for
// the parallel batches, host_serial_chain for the serial ones: verify_many's rule), its signature pair (-G1, sum [r_i]S_i).  The call runs in
// slices of whole batches (plan.hpp manyeach_cut); per slice one copy of its tables, the scalars, hashing and [r]PK into the per-set
// path's pair store on the caller's stream and, beside them on the context's fork stream, one 64-bit G2 multiplication per set
// (k_combsets_g2mul) and the segmented sum per batch (k_combsets_g2_sum); k_manyeach_setup joins the two, then the Miller lines, the
// segmented line product and the tail of the per-group path.  A batch that fits no slice takes verify_common, in its turn.  No product is
// shared between batches, so equal random bytes in two batches need no special case.  The verdict bytes of all slices collect in d_each_v
// and come back in one copy; the scalars and the random bytes are cleared on the device before the call returns.
// ------------------------------------------------------------------------------------------
static int manyeach_run(mi355_bls_ctx* c, const uint8_t* d_src, const uint8_t* h_src, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                        uint8_t* gt_out, hipStream_t st) {
    size_t total = 0;
    if (int rc = many_args(c, d_src, h_src, counts, rnds, k, verdicts, &total)) return rc;
    if (k >= plan::AGG_NONE || ((uintptr_t)d_src & 3)) {
        g_err = "batch_verify_many_each: more than 2^32 - 2 batches, or records that are not 4-byte aligned";
        return MI355_BLS_ERR_ARG;
    }
    if (gt_out) std::memset(gt_out, 0, k * 576);
    if (total == 0) return 0;                                     // every batch empty: every verdict false
    HIPCHK(hipSetDevice(c->device));
    int rc = each_reserve(c, k, gt_out != nullptr);               // the verdict bytes, the values, and the pair store at its first use
    if (rc) return rc;
    const pair_store ps = c->each_pairs();
    // pass 1: the slices, their tables (groups | line-product items in aggv_tab; G2 sum items | final_of in grp.items), the scalars' sources
    struct slice_rec {
        plan::manyeach_slice s;
        plan::aggveach_tab t;
        plan::aggsets_plan sum;
        size_t tab_at, sum_at, meta_at, n_meta;
        uint32_t lanes;
        bool any_serial;
    };
    std::vector<slice_rec> slices;
    std::vector<size_t> offs(k + 1), rel;
    offs[0] = 0;
    for (size_t b = 0; b < k; b++) offs[b + 1] = offs[b] + counts[b];
    c->aggv_tab.clear(), c->grp.items.clear(), c->me_meta.clear(), c->me_rr.clear();
    c->me_r.assign(total, 0);
    size_t max_sets = 0, max_part = 0, max_ng = 0, max_tab = 0, max_sum_tab = 0, max_sum_items = 0, max_meta = 0;
    for (size_t b = 0; b < k;) {
        slice_rec sr{};
        sr.s = plan::manyeach_cut(counts, k, b, offs[b], c->cap, ps.stride);
        const plan::manyeach_slice& s = sr.s;
        b = s.b1;
        if (s.nb == 0) continue;                                  // empty batches alone
        if (!s.single) {
            const uint32_t ng = s.nb;
            sr.tab_at = c->aggv_tab.size();
            c->aggv_tab.resize(sr.tab_at + (size_t)ng * 4);
            plan::aggveach_groups(offs.data(), plan::manyeach_as_groups(s), reinterpret_cast<plan::aggv_group*>(c->aggv_tab.data() + sr.tab_at));
            sr.t = plan::aggveach_measure(reinterpret_cast<const plan::aggv_group*>(c->aggv_tab.data() + sr.tab_at), ng);
            c->aggv_tab.resize(sr.tab_at + ((size_t)ng + sr.t.items) * 4);
            const plan::aggv_group* gr = reinterpret_cast<const plan::aggv_group*>(c->aggv_tab.data() + sr.tab_at);
            plan::aggveach_fill(sr.t, gr, ng, reinterpret_cast<plan::agg_item*>(c->aggv_tab.data() + sr.tab_at + (size_t)ng * 4));
            rel.resize((size_t)ng + 1);
            plan::manyeach_sum_offsets(gr, ng, rel.data());
            sr.sum = plan::aggsets_measure(rel.data(), ng);
            if (!sr.sum.ok) return MI355_BLS_ERR_ARG;             // (a slice is far below 2^32 sets)
            sr.sum_at = c->grp.items.size();
            c->grp.items.resize(sr.sum_at + sr.sum.items * 4 + ng);
            plan::aggsets_fill(sr.sum, rel.data(), ng, reinterpret_cast<plan::agg_item*>(c->grp.items.data() + sr.sum_at),
                               c->grp.items.data() + sr.sum_at + sr.sum.items * 4);
            // the scalars: batchVerify's dispatch per batch (bls_batch_verifier.nim:440), addressed within the slice
            sr.meta_at = c->me_meta.size();
            for (uint32_t l = 0; l < ng; l++) {
                const size_t nb_ = gr[l].count;
                const uint8_t* rnd = rnds + 32 * (size_t)gr[l].g;
                if (c->num_threads > 1 && nb_ >= 3) {
                    const uint32_t B = (uint32_t)(nb_ < c->num_threads ? nb_ : c->num_threads);
                    c->me_meta.push_back(many_meta{gr[l].first, nb_, B, sr.lanes});
                    c->me_rr.insert(c->me_rr.end(), rnd, rnd + 32);
                    sr.lanes += B;
                } else {
                    host_serial_chain(rnd, nb_, c->me_r.data() + s.set0 + gr[l].first);
                    sr.any_serial = true;
                }
            }
            sr.n_meta = c->me_meta.size() - sr.meta_at;
            if (s.sets > max_sets) max_sets = s.sets;
            if (sr.t.partials > max_part) max_part = sr.t.partials;
            if (ng > max_ng) max_ng = ng;
            if (((size_t)ng + sr.t.items) * 4 > max_tab) max_tab = ((size_t)ng + sr.t.items) * 4;
            if (sr.sum.items * 4 + ng > max_sum_tab) max_sum_tab = sr.sum.items * 4 + ng;
            if (sr.sum.items > max_sum_items) max_sum_items = sr.sum.items;
            if (sr.n_meta > max_meta) max_meta = sr.n_meta;
        }
        slices.push_back(sr);
    }
    const size_t n1 = max_sets ? max_sets : 1, it1 = max_sum_items ? max_sum_items : 1, m1 = max_meta ? max_meta : 1;
    const size_t tcap = n1 < plan::COMB_MUL_CHUNK ? (n1 + WAVE - 1) / WAVE * WAVE : plan::COMB_MUL_CHUNK;
    const size_t pw = plan::aggveach_part_words(max_part) * 4, sw = plan::aggveach_step_words(max_ng) * 4;
    rc = c->grp.d_flag.reserve(k * 4, k);
    if (!rc) rc = c->grp.d_items.reserve(max_sum_tab * 4 + 16, max_sum_tab);
    if (!rc) rc = c->grp.d_g2_prod.reserve(n1 * (size_t)G2W * 4, n1 * (size_t)G2W);
    if (!rc) rc = c->grp.d_g2_part.reserve(it1 * (size_t)G2W * 4, it1 * (size_t)G2W);
    if (!rc) rc = c->d_comb_g2tab.reserve(tcap * 8 * 6 * 64, 0);
    if (!rc) rc = c->d_comb_pkflag.reserve(4, 0);
    if (!rc) rc = c->d_comb_rnd.reserve(m1 * 32, m1 * 8);
    if (!rc) rc = c->d_me_meta.reserve(m1 * sizeof(many_meta), m1 * sizeof(many_meta) / 4);
    if (!rc) rc = c->d_aggv_part.reserve(pw, pw / 4);
    if (!rc) rc = c->d_aggv_step.reserve(sw, sw / 4);
    if (!rc) rc = c->d_aggv_tab.reserve(max_tab * 4 + 16, max_tab);
    if (!rc) rc = c->d_aggv_carry.reserve(2 * 576, 0);
    if (!rc) rc = c->d_aggv_work.reserve((size_t)plan::each_engine_grid_max(c->slots) * AGGV_WORK_WORDS * 4, 0);
    if (rc) return rc;
    const size_t g2tcap = c->d_comb_g2tab.bytes / (8 * 6 * 64);      // what the buffer holds (it may be larger than this call needs)
    HIPCHK(hipEventRecord(c->ev[0], st));
    HIPCHK(hipMemsetAsync(c->grp.d_flag, 0, k * 4, st));
    HIPCHK(hipMemsetAsync(c->d_each_v, 0, k, st));                     // an empty batch has no lane: its verdict is 0, its value zero bytes
    if (gt_out) HIPCHK(hipMemsetAsync(c->d_each_gt, 0, k * 576, st));
    uint32_t* dg = gt_out ? c->d_each_gt.p : nullptr;
    struct single_rec {
        size_t b;
        int v;
        uint8_t gt[576];
    };
    std::vector<single_rec> singles;
    // pass 2: slice after slice on the caller's stream
    for (const slice_rec& sr : slices) {
        const plan::manyeach_slice& s = sr.s;
        if (s.single) {                                                // the single-batch path, which slices internally; blocking
            size_t b = s.b0;
            while (counts[b] == 0) b++;
            const int serial = (c->num_threads > 1 && s.sets >= 3) ? 0 : 1;
            single_rec r{b, 0, {}};
            r.v = verify_common(c, d_src ? d_src + 320 * s.set0 : nullptr, d_src ? nullptr : h_src + 320 * s.set0, s.sets, rnds + 32 * b, serial, st);
            if (r.v < 0) return r.v;
            if (gt_out) HIPCHK(hipMemcpy(r.gt, c->d_gt, 576, hipMemcpyDeviceToHost));      // stage 4 of that call
            singles.push_back(r);
            continue;
        }
        const uint32_t n32 = (uint32_t)s.sets, ng = s.nb;
        const plan::aggveach_plan p = plan::aggveach_for(c->slots, c->coop, n32, ng, ng);
        const uint8_t* src = d_src ? d_src + s.set0 * 320 : c->d_sets;
        if (!d_src) HIPCHK(hipMemcpyAsync(c->d_sets, h_src + s.set0 * 320, s.sets * 320, hipMemcpyHostToDevice, st));      // behind the last slice's kernels
        HIPCHK(hipMemcpyAsync(c->d_aggv_tab, c->aggv_tab.data() + sr.tab_at, ((size_t)ng + sr.t.items) * 16, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(c->grp.d_items, c->grp.items.data() + sr.sum_at, (sr.sum.items * 4 + ng) * 4, hipMemcpyHostToDevice, st));
        const uint4* gtab = reinterpret_cast<const uint4*>(c->d_aggv_tab.p);
        const uint4* items = gtab + ng;
        const uint4* sum_items = reinterpret_cast<const uint4*>(c->grp.d_items.p);
        const uint32_t* d_final = c->grp.d_items + sr.sum.items * 4;
        // ---- scalars (verify_many's): the serial batches' from the host, zeros elsewhere, then the parallel batches' chains over them
        if (sr.any_serial) HIPCHK(hipMemcpyAsync(c->d_r, c->me_r.data() + s.set0, s.sets * 8, hipMemcpyHostToDevice, st));
        if (sr.lanes) {
            many_meta* d_meta = reinterpret_cast<many_meta*>(c->d_me_meta.p);
            HIPCHK(hipMemcpyAsync(d_meta, c->me_meta.data() + sr.meta_at, sr.n_meta * sizeof(many_meta), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(c->d_comb_rnd, c->me_rr.data() + sr.meta_at * 32, sr.n_meta * 32, hipMemcpyHostToDevice, st));
            k_blind_many<<<plan::waves_for(sr.lanes), WAVE, 0, st>>>(c->d_comb_rnd, d_meta, (uint32_t)sr.n_meta, sr.lanes, c->d_r);
        }
        // ---- fork: the signature side on the context's first fork stream, hashing and [r]PK here
        hipStream_t s2 = ensure_side(c) ? (hipStream_t)c->side : st;
        if (s2 != st) {
            HIPCHK(hipEventRecord(c->ev[2], st));
            HIPCHK(hipStreamWaitEvent(s2, c->ev[2], 0));
        }
        const uint32_t* recs = reinterpret_cast<const uint32_t*>(src);
        for (size_t a = 0; a < s.sets; a += plan::COMB_MUL_CHUNK) {
            const uint32_t m = (uint32_t)(s.sets - a < plan::COMB_MUL_CHUNK ? s.sets - a : plan::COMB_MUL_CHUNK);
            k_combsets_g2mul<<<plan::waves_for(m), WAVE, 0, s2>>>(recs + a * 80, m, c->d_r + a, c->d_comb_g2tab, g2tcap, c->grp.d_g2_prod + a * (size_t)G2W);
        }
        uint32_t* g2_part = c->grp.d_g2_part;
        launch_levels(sr.sum, sum_items,
                      [&](const uint4* it, uint32_t cnt) { k_combsets_g2_sum<<<plan::waves_for(cnt), WAVE, 0, s2>>>(it, cnt, c->grp.d_g2_prod, g2_part); },
                      [&](const uint4* it, uint32_t cnt) { k_combsets_g2_sum<<<plan::waves_for(cnt), WAVE, 0, s2>>>(it, cnt, g2_part, g2_part); });
        if (s2 != st) HIPCHK(hipEventRecord(c->ev[3], s2));
        launch_hash_map(c, src, n32, st);                                  // H(m_i) -> pair slot i, in the forms the batch path takes for n messages
        launch_hash_clear(c, ps, n32, st);
        HIPCHK(hipMemsetAsync(c->d_comb_pkflag, 0, 4, st));               // k_pkmul's one word for all keys: the batches' own words are k_manyeach_setup's
        if (plan::pkmul_spread_for(c->slots, c->coop, n32))
            k_pkmul_spread<<<plan::waves_for(n32), WAVE, 0, st>>>(src, n32, c->d_r, ps.P, ps.stride, c->d_comb_pkflag, c->d_pktab);
        else k_pkmul<<<plan::waves_for(n32), WAVE, 0, st>>>(src, n32, c->d_r, ps.P, ps.stride, c->d_comb_pkflag, c->d_pktab);
        if (s2 != st) HIPCHK(hipStreamWaitEvent(st, c->ev[3], 0));        // join
        k_manyeach_setup<<<p.setup_grid, WAVE, 0, st>>>(recs, n32, gtab, ng, d_final, g2_part, ps.H, ps.P, ps.stride, c->grp.d_flag);
        launch_lines(ps, p.lines, st);
        const uint32_t n_part = (uint32_t)(sr.t.partials ? sr.t.partials : 1);
        uint32_t *part = c->d_aggv_part, *step = c->d_aggv_step;
        launch_levels(sr.t, items,
                      [&](const uint4* it, uint32_t cnt) {
                          k_aggveach_l0<<<dim3(plan::waves_for(cnt), N_LINES), WAVE, 0, st>>>(it, cnt, ps.lines, ps.stride, n32, part, n_part, step);
                      },
                      [&](const uint4* it, uint32_t cnt) { k_aggveach_ln<<<dim3(plan::waves_for(cnt), N_LINES), WAVE, 0, st>>>(it, cnt, part, n_part, step); });
        if (!p.tail_engine) k_aggveach_tail<<<p.tail_grid, WAVE, 0, st>>>(step, gtab, ng, c->grp.d_flag, c->d_aggv_carry, c->d_each_v, dg);
        else k_aggveach_engine_rows<<<p.tail_grid, K_TAIL_THREADS, 0, st>>>(step, gtab, ng, c->grp.d_flag, c->d_aggv_carry, c->d_each_v, dg, c->d_aggv_work);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(c->ev[1], st));
    HIPCHK(hipMemcpyAsync(verdicts, c->d_each_v, k, hipMemcpyDeviceToHost, st));
    if (gt_out) HIPCHK(hipMemcpyAsync(gt_out, c->d_each_gt, k * 576, hipMemcpyDeviceToHost, st));
    // the scalars and the random bytes are blinding material: nothing of them stays on the device, or in the context's host vectors
    if (max_sets) HIPCHK(hipMemsetAsync(c->d_r, 0, max_sets * 8, st));
    if (max_meta) HIPCHK(hipMemsetAsync(c->d_comb_rnd, 0, max_meta * 32, st));
    HIPCHK(hipStreamSynchronize(st));
    std::fill(c->me_r.begin(), c->me_r.end(), 0);
    std::fill(c->me_rr.begin(), c->me_rr.end(), 0);
    for (const single_rec& r : singles) {
        verdicts[r.b] = (uint8_t)r.v;
        if (gt_out) std::memcpy(gt_out + r.b * 576, r.gt, 576);
    }
    c->me_passes++;
    c->last_n = 0;                             // fetch_stage shows the last call, and this one left no batch stages
    c->sig_slots = 0;
    c->agg_valid = false;
    c->have_gt = false;
    rc = collect_timings(c, 1);
    if (rc) return rc;
    int all = 1;
    for (size_t b = 0; b < k; b++) all &= verdicts[b] == 1;
    return all;
}
extern "C" int mi355_bls_batch_verify_many_each(mi355_bls_ctx* c, const void* sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[]) {
    return manyeach_run(c, nullptr, (const uint8_t*)sets, counts, rnds, k, verdicts, nullptr, nullptr);
}
extern "C" int mi355_bls_batch_verify_many_each_device(mi355_bls_ctx* c, const void* d_sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                                                       void* stream) {
    return manyeach_run(c, (const uint8_t*)d_sets, nullptr, counts, rnds, k, verdicts, nullptr, (hipStream_t)stream);
}
// TEST HOOKS: the host form with the 576-byte value of every batch (zero bytes for an empty one; stage 4 of the single-batch call for a
// batch that took that path); the number of per-batch passes this context has made
extern "C" int mi355_bls_debug_batch_verify_many_each_gt(mi355_bls_ctx* c, const void* sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                                                         uint8_t* gt_out) {
    if (k && !gt_out) return MI355_BLS_ERR_ARG;
    return manyeach_run(c, nullptr, (const uint8_t*)sets, counts, rnds, k, verdicts, gt_out, nullptr);
}
extern "C" int mi355_bls_debug_batch_verify_many_each_passes(mi355_bls_ctx* c) { return c ? c->me_passes : MI355_BLS_ERR_ARG; }

// The merged pass of batch_verify_many first, where it may run; only a call in which it fails (or cannot run) pays for the per-batch pass
static int many_locate(mi355_bls_ctx* c, const uint8_t* d_src, const uint8_t* h_src, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                       hipStream_t st) {
    size_t total = 0;
    if (int rc = many_args(c, d_src, h_src, counts, rnds, k, verdicts, &total)) return rc;
    if (total == 0) return 0;
    HIPCHK(hipSetDevice(c->device));
    bool merged_ok = false;
    if (int rc = many_merged_pass(c, d_src, h_src, counts, rnds, k, total, st, &merged_ok)) return rc;
    if (merged_ok) return many_all_pass(counts, k, verdicts);
    return manyeach_run(c, d_src, h_src, counts, rnds, k, verdicts, nullptr, st);      // (1 where the merged pass could not run and every batch verifies)
}
extern "C" int mi355_bls_batch_verify_many_locate(mi355_bls_ctx* c, const void* sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[]) {
    return many_locate(c, nullptr, (const uint8_t*)sets, counts, rnds, k, verdicts, nullptr);
}
extern "C" int mi355_bls_batch_verify_many_locate_device(mi355_bls_ctx* c, const void* d_sets, const size_t counts[], const uint8_t* rnds, size_t k,
                                                         uint8_t verdicts[], void* stream) {
    return many_locate(c, (const uint8_t*)d_sets, nullptr, counts, rnds, k, verdicts, (hipStream_t)stream);
}

static int shard_enqueue(mi355_bls_ctx* c, const void* d_sets, const uint8_t* h_sets, size_t n_total, uint32_t chunk_lo, uint32_t chunk_hi, const uint8_t rnd[32],
                         hipStream_t st, mi355_bls_ctx* after) {
    if (!c || !rnd || n_total == 0 || (!d_sets && !h_sets)) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    uint32_t B = (uint32_t)(n_total < c->num_threads ? n_total : c->num_threads);
    if (chunk_hi > B) chunk_hi = B;
    if (chunk_lo >= chunk_hi) return MI355_BLS_ERR_ARG;
    size_t first, count;
    mi355_bls_chunk_range(n_total, c->num_threads, chunk_lo, chunk_hi, &first, &count);
    if (after && after != c && after->wide_recorded) {
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipStreamWaitEvent(st, after->ev[3], 0));          // see mi355_bls_batch_submit_device
    }
    int rc = run_shard(c, (const uint8_t*)d_sets, h_sets, n_total, B, chunk_lo, chunk_hi - chunk_lo, first, count, 0, rnd, st);
    if (rc) return rc;
    k_pack_blob<<<1, WAVE, 0, st>>>(c->d_states, c->d_flags, c->d_blob_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_flags + 16, c->d_states, 576, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(c->h_flags, c->d_flags, 4, hipMemcpyDeviceToHost, st));
    c->pending = true;
    g_in_flight.fetch_add(1, std::memory_order_relaxed);
    c->pending_stream = st;
    return 0;
}
static int shard_wait(mi355_bls_ctx* c, uint8_t out_fp12[576], int* out_ok) {
    if (!c || !out_fp12 || !out_ok || !c->pending) return MI355_BLS_ERR_ARG;
    c->pending = false;
    g_in_flight.fetch_sub(1, std::memory_order_relaxed);
    HIPCHK(hipSetDevice(c->device));
    {
        hipStream_t ps = c->pending_stream;
        c->pending_stream = nullptr;
        HIPCHK(hipStreamSynchronize(ps));
    }
    std::memcpy(out_fp12, c->h_flags + 16, 576);
    *out_ok = c->h_flags[0] == 0 ? 1 : 0;
    return collect_timings(c, 7);
}
extern "C" int mi355_bls_batch_shard_device(mi355_bls_ctx* c, const void* d_sets, size_t n_total, uint32_t chunk_lo, uint32_t chunk_hi,
                                            const uint8_t rnd[32], void* stream, uint8_t out_fp12[576], int* out_ok) {
    if (!out_fp12 || !out_ok) return MI355_BLS_ERR_ARG;
    int rc = shard_enqueue(c, d_sets, nullptr, n_total, chunk_lo, chunk_hi, rnd, (hipStream_t)stream, nullptr);
    if (rc) return rc;
    return shard_wait(c, out_fp12, out_ok);
}
extern "C" int mi355_bls_batch_shard_submit_device(mi355_bls_ctx* c, const void* d_sets, size_t n_total, uint32_t chunk_lo, uint32_t chunk_hi,
                                                   const uint8_t rnd[32], void* stream, mi355_bls_ctx* after) {
    return shard_enqueue(c, d_sets, nullptr, n_total, chunk_lo, chunk_hi, rnd, (hipStream_t)stream, after);
}
extern "C" int mi355_bls_batch_shard_wait(mi355_bls_ctx* c, uint8_t out_fp12[576], int* out_ok) { return shard_wait(c, out_fp12, out_ok); }

extern "C" int mi355_bls_finalverify_shards(mi355_bls_ctx* c, const uint8_t* fp12s, size_t kk) {
    if (!c || !fp12s || kk == 0 || kk > 64) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->d_states, fp12s, kk * 576, hipMemcpyHostToDevice, nullptr));
    launch_k_tail(c, nullptr, c->d_L, c->d_states, (uint32_t)kk, 2, c->d_gt, c->d_flags + 1, 144, 0);
    HIPCHK(hipGetLastError());
    uint32_t v = 0;
    HIPCHK(hipMemcpyAsync(&v, c->d_flags + 1, 4, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    c->have_gt = true;
    c->gt_is_fv = false;
    return v == 1 ? 1 : 0;
}

extern "C" int mi355_bls_ctx_shard_blob_device(mi355_bls_ctx* c, void** d_blob) {
    if (!c || !d_blob) return MI355_BLS_ERR_ARG;
    *d_blob = c->d_blob_out;
    return 0;
}
extern "C" int mi355_bls_ctx_set_shard_blob_device(mi355_bls_ctx* c, void* d_blob) {
    if (!c || ((uintptr_t)d_blob & 15)) return MI355_BLS_ERR_ARG;
    c->d_blob_out = d_blob ? (uint32_t*)d_blob : c->d_blob;
    return 0;
}

// merge + finalVerify on k shard blobs resident in DEVICE memory (e.g. the output of an RCCL all_gather of every rank's
// mi355_bls_ctx_shard_blob_device buffer): nothing crosses PCIe but the verdict word.
extern "C" int mi355_bls_finalverify_blobs_submit_device(mi355_bls_ctx* c, const void* d_blobs, size_t kk, size_t stride_bytes, void* stream) {
    if (!c || !d_blobs || kk == 0 || kk > 1024 || stride_bytes < 580 || (stride_bytes & 3)) return MI355_BLS_ERR_ARG;
    if (c->fv_pending) {
        g_err = "a finalverify submitted on this context has not been waited for";
        return MI355_BLS_ERR_ARG;
    }
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    launch_k_tail(c, st, c->d_L, const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(d_blobs)), (uint32_t)kk, 2, c->d_gt_fv, c->d_flags + 3,
                               (uint32_t)(stride_bytes / 4), 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->h_flags + 3, c->d_flags + 3, 4, hipMemcpyDeviceToHost, st));
    c->fv_pending = true;
    c->fv_stream = st;
    return 0;
}
extern "C" int mi355_bls_finalverify_wait(mi355_bls_ctx* c) {
    if (!c || !c->fv_pending) return MI355_BLS_ERR_ARG;
    c->fv_pending = false;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->fv_stream));
    c->have_gt = true;
    c->gt_is_fv = true;
    return c->h_flags[3] == 1 ? 1 : 0;
}

// Contiguous, balanced blocks of chunks per device (the +-1 rule parallel_chunks uses for tuples, applied to chunks).
extern "C" int mi355_bls_shard_plan(size_t n_total, uint32_t num_threads, uint32_t world, uint32_t rank, uint32_t* chunk_lo, uint32_t* chunk_hi,
                                    size_t* first, size_t* count) {
    if (world == 0 || rank >= world || num_threads == 0 || !chunk_lo || !chunk_hi || !first || !count) return MI355_BLS_ERR_ARG;
    uint32_t B = (uint32_t)(n_total < num_threads ? n_total : num_threads);
    uint32_t base = B / world, rem = B % world;
    uint32_t lo = rank < rem ? (base + 1) * rank : base * rank + rem, hi = lo + base + (rank < rem ? 1 : 0);
    *chunk_lo = lo;
    *chunk_hi = hi;
    if (lo < hi) {
        mi355_bls_chunk_range(n_total, num_threads, lo, hi, first, count);
    } else {                                                  // more devices than chunks: an empty shard at the end of the batch
        size_t f0;
        mi355_bls_chunk_range(n_total, num_threads, 0, lo, &f0, first);
        *count = 0;
    }
    return 0;
}

// batchVerifyParallel over several GPUs from ONE host thread (bls_batch_verifier.nim:296-371 with devices in place of threads):
// device g takes a contiguous block of chunks (its processSingleChunk work, :326-357), all shards are enqueued asynchronously,
// the 576-byte committed states come back through pinned host memory, and device 0 merges them and runs the one final
// exponentiation (:360-371).  d_sets[g] != nullptr: shard g's records are already resident on device g.
// host time (us after the call began) at which each device's shard was handed to its stream in the last multi-device call of this thread
static thread_local float g_multi_enq_us[64];
static thread_local size_t g_multi_enq_n = 0;
extern "C" size_t mi355_bls_debug_multi_enqueue_us(float* out, size_t cap) {
    size_t k = g_multi_enq_n < cap ? g_multi_enq_n : cap;
    for (size_t i = 0; i < k; i++) out[i] = g_multi_enq_us[i];
    return g_multi_enq_n;
}
extern "C" int mi355_bls_debug_fail_next_enqueue(mi355_bls_ctx* c) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->fail_next_enqueue = true;
    return 0;
}
static int verify_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, const uint8_t* sets, const void* const d_sets[], size_t n, const uint8_t rnd[32]) {
    if (!ctxs || ngpu == 0 || ngpu > 64 || !rnd || (!sets && !d_sets)) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    // first pass: the whole plan is validated before anything is enqueued, so that no argument error can strand a live shard
    struct plan_t { uint32_t lo, hi; size_t first, count; } plan[64];
    for (size_t g = 0; g < ngpu; g++) {
        if (!ctxs[g] || ctxs[g]->num_threads != ctxs[0]->num_threads) return MI355_BLS_ERR_ARG;
        if (ctx_busy(ctxs[g])) return MI355_BLS_ERR_ARG;
        mi355_bls_shard_plan(n, ctxs[0]->num_threads, (uint32_t)ngpu, (uint32_t)g, &plan[g].lo, &plan[g].hi, &plan[g].first, &plan[g].count);
        if (plan[g].count && !(d_sets && d_sets[g]) && !sets) return MI355_BLS_ERR_ARG;
    }
    // Host records: the caller's range is page-locked for the duration of the call, so that every device's copy is a real
    // asynchronous DMA and device g does not wait for device g - 1's staging (from pageable memory hipMemcpyAsync blocks the host
    // thread until the copy has been staged: 42 MB per 131 072-tuple shard).  If the range cannot be registered the copies are
    // simply synchronous.
    bool registered = false;
    if (sets) {
        bool any_host = false;
        for (size_t g = 0; g < ngpu; g++) any_host = any_host || (plan[g].count && !(d_sets && d_sets[g]));
        if (any_host) {
            registered = hipHostRegister(const_cast<uint8_t*>(sets), n * 320, hipHostRegisterPortable) == hipSuccess;
            if (!registered) (void)hipGetLastError();
        }
    }
    bool live[64] = {};
    int rc_keep = 0;
    g_multi_enq_n = 0;
    const auto t_start = std::chrono::steady_clock::now();
    for (size_t g = 0; g < ngpu && !rc_keep; g++) {
        g_multi_enq_us[g_multi_enq_n++] = std::chrono::duration<float, std::micro>(std::chrono::steady_clock::now() - t_start).count();
        if (plan[g].count == 0) continue;                          // more devices than chunks
        mi355_bls_ctx* c = ctxs[g];
        const void* src = d_sets ? d_sets[g] : nullptr;
        // shard_enqueue stages host records itself (slice by slice when the shard exceeds the context's capacity)
        int rc = shard_enqueue(c, src, src ? nullptr : sets + 320 * plan[g].first, n, plan[g].lo, plan[g].hi, rnd, nullptr, nullptr);
        if (rc) rc_keep = rc;                                      // the shards already enqueued are waited for below
        else live[g] = true;
    }
    std::string err_keep = g_err;
    std::vector<uint8_t> states;
    bool all_ok = true;
    for (size_t g = 0; g < ngpu; g++) {
        if (!live[g]) continue;
        uint8_t st[576];
        int ok = 0;
        int rc = shard_wait(ctxs[g], st, &ok);                    // every enqueued shard is waited for, also after a failure
        if (rc && !rc_keep) {
            rc_keep = rc;
            err_keep = g_err;
        }
        all_ok = all_ok && ok;
        states.insert(states.end(), st, st + 576);
    }
    if (registered) (void)hipHostUnregister(const_cast<uint8_t*>(sets));
    if (rc_keep) {
        g_err = err_keep;
        return rc_keep;
    }
    if (!all_ok) return 0;                                        // some update() failed (infinity public key)
    return mi355_bls_finalverify_shards(ctxs[0], states.data(), states.size() / 576);
}
extern "C" int mi355_bls_batch_verify_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, const void* sets, size_t n, const uint8_t rnd[32]) {
    if (n && !sets) return MI355_BLS_ERR_ARG;
    return verify_multi(ctxs, ngpu, (const uint8_t*)sets, nullptr, n, rnd);
}
extern "C" int mi355_bls_batch_verify_multi_device(mi355_bls_ctx* const ctxs[], size_t ngpu, const void* const d_sets[], size_t n, const uint8_t rnd[32]) {
    if (n && !d_sets) return MI355_BLS_ERR_ARG;
    return verify_multi(ctxs, ngpu, nullptr, d_sets, n, rnd);
}

// Process-wide default context for the entry points that take no context (the reference's cache-less overloads allocate a
// cache per call, bls_batch_verifier.nim:399-416, :475-495; blst_p1s_mult_pippenger takes only a scratch pointer): created on
// first use on HIP device $MI355_BLS_DEVICE (default 0), regrown when a call needs more capacity; calls are serialised.
static std::mutex g_default_mu;
static mi355_bls_ctx* g_default_ctx = nullptr;
static int default_ctx_locked(size_t need_sets, mi355_bls_ctx** out) {
    if (need_sets < 1024) need_sets = 1024;
    // every entry point is capacity-free (a larger batch runs in slices, run_shard), so the default context never grows beyond two
    // whole-chip batches: mi355_bls_batch_verify_once on 2^20 sets allocates ~4 GB of workspace, not ~30
    if (need_sets > 131072) need_sets = 131072;
    if (g_default_ctx && g_default_ctx->cap >= need_sets) {
        *out = g_default_ctx;
        return 0;
    }
    if (g_default_ctx) {
        mi355_bls_ctx_destroy(g_default_ctx);
        g_default_ctx = nullptr;
    }
    const char* e = getenv("MI355_BLS_DEVICE");
    int rc = mi355_bls_ctx_create(&g_default_ctx, e ? atoi(e) : 0, need_sets);
    if (rc) return rc;
    *out = g_default_ctx;
    return 0;
}
extern "C" int mi355_bls_batch_verify_once(const void* sets, size_t n, const uint8_t rnd[32], uint32_t num_threads) {
    if (!rnd || num_threads == 0) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!sets) return MI355_BLS_ERR_ARG;
    std::lock_guard<std::mutex> lk(g_default_mu);
    mi355_bls_ctx* c;
    int rc = default_ctx_locked(n, &c);
    if (rc) return rc;
    c->num_threads = num_threads;
    // batchVerify's dispatch (bls_batch_verifier.nim:475-495): parallel iff numThreads > 1 and n >= 3
    return verify_host(c, sets, n, rnd, (num_threads > 1 && n >= 3) ? 0 : 1);
}
extern "C" void mi355_bls_default_ctx_release(void) {
    std::lock_guard<std::mutex> lk(g_default_mu);
    if (g_default_ctx) mi355_bls_ctx_destroy(g_default_ctx);
    g_default_ctx = nullptr;
}

extern "C" int mi355_bls_fetch_stage(mi355_bls_ctx* c, int what, void* out, size_t out_bytes) {
    if (!c || !out) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    size_t n = c->last_n;
    const size_t np = c->last_n.pairs;       // the tuple pairs in front of the signature side's: n, or the k groups of a by-message slice
    uint32_t nb = plan::waves_for((uint32_t)np);
    switch (what) {
        case 0:
            if (out_bytes < n * 8) return MI355_BLS_ERR_ARG;
            HIPCHK(hipMemcpy(out, c->d_r, n * 8, hipMemcpyDeviceToHost));
            return 0;
        case 1:
            if (out_bytes < np * 288 || np == 0) return MI355_BLS_ERR_ARG;
            k_export_g2<<<nb, WAVE>>>(c->d_H, c->stride, (uint32_t)np, c->d_export);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy(out, c->d_export, np * 288, hipMemcpyDeviceToHost));
            return 0;
        case 2:
            if (out_bytes < np * 144 || np == 0) return MI355_BLS_ERR_ARG;
            k_export_g1<<<nb, WAVE>>>(c->d_P, c->stride, (uint32_t)np, c->d_export);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy(out, c->d_export, np * 144, hipMemcpyDeviceToHost));
            return 0;
        case 3:
            if (out_bytes < 288) return MI355_BLS_ERR_ARG;
            if (!c->agg_valid && c->sig_slots) {                     // bucket path: fold the bucket sums now
                k_sig_fold<<<1, WAVE>>>(c->d_H, c->stride, (uint32_t)np, 64 / c->sig_c, c->sig_c, c->d_agg);
                HIPCHK(hipGetLastError());
                c->agg_valid = true;
            }
            HIPCHK(hipMemcpy(out, c->d_agg, 288, hipMemcpyDeviceToHost));
            return 0;
        case 4:
            if (out_bytes < 576 || !c->have_gt) return MI355_BLS_ERR_ARG;
            HIPCHK(hipMemcpy(out, c->gt_is_fv ? c->d_gt_fv : c->d_gt, 576, hipMemcpyDeviceToHost));
            return 0;
        case 5:
            if (out_bytes < 576) return MI355_BLS_ERR_ARG;
            HIPCHK(hipMemcpy(out, c->d_states, 576, hipMemcpyDeviceToHost));
            return 0;
    }
    return MI355_BLS_ERR_ARG;
}

extern "C" int mi355_bls_last_kernel_timings(mi355_bls_ctx* c, float out[4]) {
    if (!c || !out) return MI355_BLS_ERR_ARG;
    for (int i = 0; i < 4; i++) out[i] = c->ktimes[i];
    return 0;
}

extern "C" int mi355_bls_last_timings(mi355_bls_ctx* c, float out[8]) {
    if (!c || !out) return MI355_BLS_ERR_ARG;
    for (int i = 0; i < 8; i++) out[i] = c->timings[i];
    return 0;
}

static int g1_sum_enqueue(mi355_bls_ctx* c, const uint8_t* d_pts, size_t n, hipStream_t st) {
    // result (blst_p1 image, 144 B) lands in d_agg1
    const uint32_t n32 = (uint32_t)n;
    const plan::sum_plan p = plan::g1_sum_for(c->slots, n32);
    k_g1_sum<<<p.nblk, WAVE, 0, st>>>(d_pts, n32, p.m, c->d_export);
    k_g1_sum2<<<1, WAVE, 0, st>>>(c->d_export, p.nblk, c->d_agg1);
    HIPCHK(hipGetLastError());
    return 0;
}

extern "C" int mi355_bls_g1_aggregate_device(mi355_bls_ctx* c, const void* d_pks, size_t n, void* stream, uint8_t out_p1[144]) {
    if (!c || !d_pks || !out_p1 || n == 0 || n > (1u << 30)) return MI355_BLS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->ev[0], st));
    int rc = g1_sum_enqueue(c, (const uint8_t*)d_pks, n, st);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[1], st));
    HIPCHK(hipMemcpyAsync(out_p1, c->d_agg1, 144, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return one_stage_timings(c);
}

extern "C" int mi355_bls_g2_aggregate_device(mi355_bls_ctx* c, const void* d_sigs, size_t n, void* stream, uint8_t out_p2[288]) {
    if (!c || !d_sigs || !out_p2 || n == 0 || n > (1u << 30)) return MI355_BLS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventRecord(c->ev[0], st));
    const uint32_t n32 = (uint32_t)n;
    const plan::sum_plan p = plan::g2_sum_for(c->slots, n32);
    k_g2_sum<<<p.nblk, WAVE, 0, st>>>((const uint8_t*)d_sigs, n32, p.m, c->d_export);
    k_g2_sum2<<<1, WAVE, 0, st>>>(c->d_export, p.nblk, c->d_agg);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[1], st));
    HIPCHK(hipMemcpyAsync(out_p2, c->d_agg, 288, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return one_stage_timings(c);
}
extern "C" int mi355_bls_g2_aggregate(mi355_bls_ctx* c, const void* sigs, size_t n, uint8_t out_p2[288]) {
    if (!c || !sigs || !out_p2 || n == 0) return MI355_BLS_ERR_ARG;
    {
        int rcr = io_reserve(c, (n * 192 + 319) / 320);
        if (rcr) return rcr;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->d_sets, sigs, n * 192, hipMemcpyHostToDevice, nullptr));
    return mi355_bls_g2_aggregate_device(c, c->d_sets, n, nullptr, out_p2);
}
extern "C" int mi355_bls_g1_aggregate(mi355_bls_ctx* c, const void* pks, size_t n, uint8_t out_p1[144]) {
    if (!c || !pks || !out_p1 || n == 0) return MI355_BLS_ERR_ARG;
    {
        int rcr = io_reserve(c, (n * 96 + 319) / 320);
        if (rcr) return rcr;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->d_sets, pks, n * 96, hipMemcpyHostToDevice, nullptr));
    return mi355_bls_g1_aggregate_device(c, c->d_sets, n, nullptr, out_p1);
}

// coreVerifyNoGroupCheck with the aggregate key (core :269-297).  d_pks != nullptr: the n keys are summed first (aggregateAll,
// beside the hash of the message in latency mode); d_pks == nullptr: the aggregate is already in d_agg1 (the multi-device form).
static int fav_run(mi355_bls_ctx* c, const void* d_pks, size_t n, const uint8_t* msg, size_t msg_len, const void* sig, hipStream_t st) {
    HIPCHK(hipSetDevice(c->device));
    const pair_store ps = c->batch_pairs();
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 12, st));
    HIPCHK(hipMemcpyAsync(c->d_msg, msg, msg_len, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(c->d_msg + 4096, sig, 192, hipMemcpyHostToDevice, st));
    HIPCHK(hipEventRecord(c->ev[0], st));
    // the key sum and the hash of the message are independent: side by side in latency mode
    hipStream_t sd = (d_pks && c->coop && ensure_side(c)) ? c->side : st;
    if (sd != st) HIPCHK(hipStreamWaitEvent(sd, c->ev[0], 0));
    if (d_pks) {
        int rc = g1_sum_enqueue(c, (const uint8_t*)d_pks, n, sd);
        if (rc) return rc;
    }
    HIPCHK(hipEventRecord(c->ev[1], sd));
    k_hash_one<<<1, 256, 0, st>>>(c->d_msg, (uint32_t)msg_len, c->dst, c->xmd, ps.H, ps.stride, 0);
    if (sd != st) HIPCHK(hipStreamWaitEvent(st, c->ev[1], 0));
    k_fav_setup<<<1, 1, 0, st>>>(c->d_agg1, reinterpret_cast<const uint32_t*>(c->d_msg + 4096), ps.H, ps.P, ps.stride, c->d_flags);
    HIPCHK(hipEventRecord(c->ev[2], st));
    launch_lines(ps, plan::lines_for(c->slots, c->coop, 2, 0), st);
    HIPCHK(hipEventRecord(c->ev[3], st));
    k_lineprod<<<dim3(N_LINES, 1), WAVE, 0, st>>>(ps.lines, 2, ps.stride, 1, c->d_lpart, 1, 0);
    k_lineprod2<<<N_LINES, WAVE, 0, st>>>(c->d_lpart, 1, c->d_L);
    HIPCHK(hipEventRecord(c->ev[4], st));
    launch_k_tail(c, st, c->d_L, c->d_states, 1, 3, c->d_gt, c->d_flags + 1, 144, 0);
    HIPCHK(hipEventRecord(c->ev[5], st));
    uint32_t fl[2];
    HIPCHK(hipMemcpyAsync(fl, c->d_flags, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->have_gt = true;
    c->gt_is_fv = false;
    c->last_n = 0;
    int rc = collect_timings(c, 5);      // [0] g1 sum, [1] hash+setup, [2] lines, [3] products, [4] tail
    if (rc) return rc;
    return (fl[0] == 0 && fl[1] == 1) ? 1 : 0;
}
extern "C" int mi355_bls_fast_aggregate_verify_device(mi355_bls_ctx* c, const void* d_pks, size_t n, const uint8_t* msg, size_t msg_len,
                                                      const void* sig, void* stream) {
    if (!c || !sig || (!msg && msg_len) || msg_len > 4096 || n > (1u << 30)) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;                                     // bls_sig_min_pubkey.nim:251-253
    if (!d_pks) return MI355_BLS_ERR_ARG;
    return fav_run(c, d_pks, n, msg, msg_len, sig, (hipStream_t)stream);
}

// coreVerifyNoGroupCheck on an aggregate the caller already holds (blst_min_pubkey_sig_core.nim:269-297 with an AggregatePublicKey:
// the `finish`-less form): agg_p1 = blst_p1 (Jacobian, 144 B), e.g. the sum of the per-rank partial key sums of a key-sharded
// fastAggregateVerify (mi355_bls_g1_aggregate_device per rank, mi355_bls_p1s_add on rank 0).  Aggregate at infinity -> 0.
extern "C" int mi355_bls_verify_aggregate(mi355_bls_ctx* c, const uint8_t agg_p1[144], const uint8_t* msg, size_t msg_len, const void* sig) {
    if (!c || !agg_p1 || !sig || (!msg && msg_len) || msg_len > 4096) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(c->d_agg1, agg_p1, 144, hipMemcpyHostToDevice));
    return fav_run(c, nullptr, 1, msg, msg_len, sig, nullptr);
}

// fastAggregateVerify with the keys sharded over several devices (SURVEY.md section 8(e)): device g sums keys [first_g, first_g +
// count_g) (mi355_bls_msm_shard_range), the 144-byte partial sums return through pinned host memory, ctxs[0] adds them and runs the
// one pairing check.  At 3 MB of keys one device is the sensible default; this is the same call for key sets that are not.
extern "C" int mi355_bls_fast_aggregate_verify_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, const void* pks, size_t n, const uint8_t* msg,
                                                     size_t msg_len, const void* sig) {
    if (!ctxs || ngpu == 0 || ngpu > 64 || !sig || (!msg && msg_len) || msg_len > 4096 || n > (1u << 30)) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!pks) return MI355_BLS_ERR_ARG;
    for (size_t g = 0; g < ngpu; g++)
        if (!ctxs[g]) return MI355_BLS_ERR_ARG;
    const uint8_t* p = (const uint8_t*)pks;
    bool live[64] = {};
    int rc = 0;
    for (size_t g = 0; g < ngpu && !rc; g++) {
        size_t first, count;
        mi355_bls_msm_shard_range(n, (uint32_t)ngpu, (uint32_t)g, &first, &count);
        if (count == 0) continue;
        mi355_bls_ctx* c = ctxs[g];
        rc = io_reserve(c, (count * 96 + 319) / 320);
        if (rc) break;
        if (hipSetDevice(c->device) != hipSuccess || hipMemcpyAsync(c->d_sets, p + 96 * first, count * 96, hipMemcpyHostToDevice, nullptr) != hipSuccess) {
            g_err = "staging of a key shard failed";
            rc = MI355_BLS_ERR_HIP;
            break;
        }
        rc = g1_sum_enqueue(c, c->d_sets, count, nullptr);
        if (rc) break;
        if (hipMemcpyAsync(c->h_flags + 160, c->d_agg1, 144, hipMemcpyDeviceToHost, nullptr) != hipSuccess) { g_err = "hipMemcpyAsync (key-sum partial)"; rc = MI355_BLS_ERR_HIP; break; }
        live[g] = true;
    }
    std::vector<uint8_t> parts;
    for (size_t g = 0; g < ngpu; g++) {                  // every device that was handed work is waited for, also after a failure
        if (!live[g]) continue;
        (void)hipSetDevice(ctxs[g]->device);
        if (hipStreamSynchronize(nullptr) != hipSuccess && !rc) { g_err = "hipStreamSynchronize (key shard)"; rc = MI355_BLS_ERR_HIP; }
        const uint8_t* h = reinterpret_cast<const uint8_t*>(ctxs[g]->h_flags + 160);
        parts.insert(parts.end(), h, h + 144);
    }
    if (rc) return rc;
    mi355_bls_ctx* c0 = ctxs[0];
    HIPCHK(hipSetDevice(c0->device));
    HIPCHK(hipMemcpyAsync(c0->d_export, parts.data(), parts.size(), hipMemcpyHostToDevice, nullptr));
    k_jac_sum_blst<fp><<<1, WAVE, 0, nullptr>>>(c0->d_export, (uint32_t)(parts.size() / 144), 36, c0->d_agg1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));               // `parts` (pageable) has been consumed
    return fav_run(c0, nullptr, n, msg, msg_len, sig, nullptr);
}

extern "C" int mi355_bls_fast_aggregate_verify(mi355_bls_ctx* c, const void* pks, size_t n, const uint8_t* msg, size_t msg_len, const void* sig) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!pks) return MI355_BLS_ERR_ARG;
    {
        int rcr = io_reserve(c, (n * 96 + 319) / 320);
        if (rcr) return rcr;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->d_sets, pks, n * 96, hipMemcpyHostToDevice, nullptr));
    return mi355_bls_fast_aggregate_verify_device(c, c->d_sets, n, msg, msg_len, sig, nullptr);
}

// ------------------------------------------------------------------------------------------
// blst_p1s_mult_pippenger / blst_p2s_mult_pippenger replacement (host side)
// ------------------------------------------------------------------------------------------
extern "C" size_t mi355_bls_p1s_mult_pippenger_scratch_sizeof(size_t npoints) {
    (void)npoints;
    return 0;          // blst_p1s_mult_pippenger_scratch_sizeof (blst_abi.nim:336): the workspace lives on the device
}

// workspace for npoints points of `affb`-byte affine images (96: G1, 192: G2) under window plan W: every buffer as plan::msm_sizes_for gives it
static int msm_reserve(msm_ws* m, size_t n, const plan::pip_win& W, size_t affb) {
    uint32_t total = W.nwin << W.cbk, cap_total = (uint32_t)(m->hist.bytes / 4);
    size_t pts_bytes = n * affb;
    if (pts_bytes <= m->d_pts.bytes && total <= cap_total) return 0;
    const plan::msm_sizes sz = plan::msm_sizes_for(pts_bytes > m->d_pts.bytes ? pts_bytes : m->d_pts.bytes, total > cap_total ? total : cap_total);
    *m = msm_ws();                                       // everything goes first: a failed grow leaves an empty workspace
    msm_ws w;
    int rc = 0;                                          // the first failure: nothing is created behind it
    const auto alloc = [&rc](auto& buf, size_t bytes) { rc = rc ? rc : buf.alloc(bytes); };
    alloc(w.d_pts, sz.d_pts);
    alloc(w.d_sc, sz.d_sc);
    alloc(w.pts_int, sz.pts_int);
    alloc(w.hist, sz.hist);
    alloc(w.offs, sz.hist);
    alloc(w.cursor, sz.hist);
    alloc(w.order, sz.hist);
    alloc(w.chist, sz.chist);
    alloc(w.shist, sz.shist);
    alloc(w.part, sz.part);
    alloc(w.sorted, sz.sorted);
    alloc(w.buckets, sz.buckets);
    alloc(w.segout, sz.segout);
    alloc(w.winout, sz.winout);
    alloc(w.out, sz.out);
    for (dev_event* e : {&w.ev_fork, &w.ev_bucketed, &w.ev_g[0], &w.ev_tail[0], &w.ev_g[1], &w.ev_tail[1]}) rc = rc ? rc : e->create(hipEventDisableTiming);
    if (rc) return rc;
    *m = std::move(w);
    return 0;
}

// Everything up to the result in m->out (blst_p1 / blst_p2 image, device memory) is ENQUEUED on `st` with workspace m; nothing is
// waited for: a walk over plan::msm_for's plan.  timed: record the context's stage events.  allow_split: the window groups may use the
// context's side stream (asked for only when the plan would split).
template <class F>
static int msm_enqueue(mi355_bls_ctx* c, msm_ws* m, const void* d_points, size_t npoints, const void* d_scalars, uint32_t sbytes, size_t nbits,
                       hipStream_t st, bool timed, bool allow_split) {
    constexpr bool G2 = sizeof(F) != sizeof(fp);
    plan::msm_plan p = plan::msm_for(npoints, nbits, G2, allow_split, true);
    if (p.ngroups > 1 && !ensure_side(c)) p = plan::msm_for(npoints, nbits, G2, allow_split, false);
    int rc = msm_reserve(m, npoints, p.W, G2 ? 192 : 96);
    if (rc) return rc;
    const pip_win W{p.W};
    const uint32_t n = p.n, nw = W.nwin, total = p.total;
    const uint8_t* pts = (const uint8_t*)d_points;
    const uint8_t* sc = (const uint8_t*)d_scalars;
    auto order_group = [&](const plan::msm_group& G, uint32_t gi, hipStream_t s) {      // the group's buckets by load (indices relative to g0)
        uint32_t* chist = m->chist + 256 * gi;
        k_msm_order_hist<<<G.order_grid, WAVE, 0, s>>>(m->hist + G.g0, G.gc, chist);
        k_msm_order_scan<<<1, 1, 0, s>>>(chist);
        k_msm_order_scatter<<<G.order_grid, WAVE, 0, s>>>(m->hist + G.g0, G.gc, chist, m->order + G.g0);
    };
    auto bucket_group = [&](const plan::msm_group& G, hipStream_t s) {
        k_pip_bucket<F><<<G.bucket_grid, WAVE, 0, s>>>(m->pts_int, m->sorted, m->offs, m->hist, m->order, n, W.cbk, total, G.g0, G.gc, m->buckets);
    };
    auto reduce_group = [&](const plan::msm_group& G, hipStream_t s, uint32_t g) {
        if (G.team == 4) k_pip_segred_team<4><<<G.segred_grid, WAVE, 0, s>>>(m->buckets, total, W.cbk, plan::MSM_SEG, p.nseg, G.t0, G.tc, m->segout);
        else if (G.team == 2) k_pip_segred_team<2><<<G.segred_grid, WAVE, 0, s>>>(m->buckets, total, W.cbk, plan::MSM_SEG, p.nseg, G.t0, G.tc, m->segout);
        else k_pip_segred<F><<<G.segred_grid, WAVE, 0, s>>>(m->buckets, total, W.cbk, plan::MSM_SEG, p.nseg, G.t0, G.tc, m->segout);
        k_pip_winpart<F><<<dim3(G.w1 - G.w0, p.nsplit), WAVE, 0, s>>>(m->segout, p.nseg, p.segs_per_win, G.w0, m->part);
        if constexpr (!G2) {
            // G1: the parts' sums and ONE Horner walk over the group's windows on the row arithmetic, continuing the walk of the group above (it runs
            // on another stream: ev_tail[g - 1]); the last group writes the result.  No per-window doubling chains, no k_pip_final.
            if (g) HIPCHK(hipStreamWaitEvent(s, m->ev_tail[g - 1], 0));
            k_pip_rowtail<<<1, G.tail_lanes, 0, s>>>(m->part, p.nsplit, W, G.w0, G.w1, g ? m->winout + 48 * (g - 1) : nullptr, m->winout + 48 * g, m->out);
            HIPCHK(hipEventRecord(m->ev_tail[g], s));
        } else {
            k_pip_winsum<F><<<G.w1 - G.w0, WAVE, 0, s>>>(m->part, p.nsplit, W, G.w0, m->winout);      // G2: window sums, then k_pip_final's Horner walk
        }
        return 0;
    };
    HIPCHK(hipMemsetAsync(m->hist, 0, (size_t)total * 4, st));
    HIPCHK(hipMemsetAsync(m->chist, 0, plan::MSM_CHIST_BYTES, st));
    if (timed) HIPCHK(hipEventRecord(c->ev[0], st));
    k_pip_convert<F><<<p.point_grid, WAVE, 0, st>>>(pts, n, m->pts_int);
    // the counting sort covers all windows
    if (p.lds_sort) {
        k_pip_hist_lds<<<dim3(PIP_SLICES, nw), PIP_SORT_THREADS, 0, st>>>(sc, sbytes, n, W, 0, p.per, m->shist);
        k_pip_slice_scan<<<p.slice_scan_grid, WAVE, 0, st>>>(m->shist, PIP_SLICES, W.cbk, 0, total, m->hist);
        k_pip_scan_block<<<nw, PIP_SORT_THREADS, 0, st>>>(m->hist, W.cbk, m->offs);
        k_pip_scatter_lds<<<dim3(PIP_SLICES, nw), PIP_SORT_THREADS, 0, st>>>(sc, sbytes, n, W, 0, p.per, m->shist, m->offs, m->sorted);
    } else {
        k_pip_hist<<<dim3(p.point_grid, nw), WAVE, 0, st>>>(sc, sbytes, n, W, 0, m->hist);
        k_msm_scan<<<nw, WAVE, 0, st>>>(m->hist, W.cbk, m->offs, m->cursor);
        k_pip_scatter<<<dim3(p.point_grid, nw), WAVE, 0, st>>>(sc, sbytes, n, W, 0, m->cursor, m->sorted);
    }
    // group g runs on its own stream, its bucket kernel behind the bucket kernel of group g - 1: the (latency-bound, few-wave)
    // reduction of a group is dispatched before the next group's bucket kernel and runs beside it.  (Both bucket kernels enqueued at
    // once, the second on a lowest-priority stream so that its waves would only fill the tail of the first - 26 % of a bucket
    // kernel's wave slots idle on average, profiles/r03_pmc_summary_msm.json - was measured 3 % SLOWER: the 512-register reduction
    // waves of the first group then wait for whole SIMDs that the second group's 256-register waves keep half full.)
    hipStream_t gs[2] = {st, c->side};
    for (uint32_t g = 0; g < p.ngroups; g++) order_group(p.group[g], g, st);
    if (timed) HIPCHK(hipEventRecord(c->ev[1], st));
    for (uint32_t g = 0; g < p.ngroups; g++) {
        if (g) HIPCHK(hipStreamWaitEvent(gs[g], m->ev_g[g - 1], 0));
        bucket_group(p.group[g], gs[g]);
        HIPCHK(hipEventRecord(m->ev_g[g], gs[g]));
        if (g == 0 && timed) HIPCHK(hipEventRecord(c->ev[2], st));
        if (int rc2 = reduce_group(p.group[g], gs[g], g)) return rc2;
        if (g == 0 && timed) HIPCHK(hipEventRecord(c->ev[3], st));
    }
    for (uint32_t g = 1; g < p.ngroups; g++) {
        HIPCHK(hipEventRecord(m->ev_g[g], gs[g]));
        HIPCHK(hipStreamWaitEvent(st, m->ev_g[g], 0));
    }
    if constexpr (G2) k_pip_final<F><<<1, WAVE, 0, st>>>(m->winout, nw, m->out);
    if (timed) HIPCHK(hipEventRecord(c->ev[4], st));
    HIPCHK(hipGetLastError());
    return 0;
}
// sum_i [k_i mod 2^nbits] P_i on the device.  sbytes: distance between scalars (32 for blst_scalar images; blst's own
// convention is (nbits + 7) / 8).  ret: blst_p1 (144 B) or blst_p2 (288 B), host memory.
template <class F>
static int msm_run(mi355_bls_ctx* c, uint8_t* ret, const void* d_points, size_t npoints, const void* d_scalars, uint32_t sbytes, size_t nbits, void* stream) {
    constexpr size_t JACB = (sizeof(F) == sizeof(fp) ? 96 : 192) / 2 * 3;
    if (!c || !ret || nbits == 0 || nbits > 256 || npoints > (1u << 28) || (size_t)sbytes * 8 < nbits || sbytes > 32) return MI355_BLS_ERR_ARG;
    if (npoints == 0) {
        memset(ret, 0, JACB);
        return 0;
    }
    if (!d_points || !d_scalars) return MI355_BLS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    int rc = msm_enqueue<F>(c, &c->msm, d_points, npoints, d_scalars, sbytes, nbits, st, true, true);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ret, c->msm.out, JACB, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return collect_timings(c, 4);       // [0] sort, [1] bucket accumulation, [2] segment reduction, [3] window sums + doublings
}
extern "C" int mi355_bls_p1s_mult_pippenger_device(mi355_bls_ctx* c, uint8_t ret_p1[144], const void* d_points, size_t npoints, const void* d_scalars,
                                                   size_t nbits, void* stream) {
    return msm_run<fp>(c, ret_p1, d_points, npoints, d_scalars, 32, nbits, stream);
}
extern "C" int mi355_bls_p2s_mult_pippenger_device(mi355_bls_ctx* c, uint8_t ret_p2[288], const void* d_points, size_t npoints, const void* d_scalars,
                                                   size_t nbits, void* stream) {
    return msm_run<fp2>(c, ret_p2, d_points, npoints, d_scalars, 32, nbits, stream);
}

// host arrays (contiguous) -> staging -> msm_run
template <class F>
static int msm_host(mi355_bls_ctx* c, uint8_t* ret, const uint8_t* pts, size_t npoints, const uint8_t* scalars, uint32_t sbytes, size_t nbits) {
    constexpr size_t AFFB = sizeof(F) == sizeof(fp) ? 96 : 192;
    if (!c || nbits == 0 || nbits > 256 || npoints > (1u << 28)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    int rc = msm_reserve(&c->msm, npoints, plan::pip_for(npoints, nbits), AFFB);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->msm.d_pts, pts, npoints * AFFB, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(c->msm.d_sc, scalars, npoints * sbytes, hipMemcpyHostToDevice, nullptr));
    return msm_run<F>(c, ret, c->msm.d_pts, npoints, c->msm.d_sc, sbytes, nbits, nullptr);
}

// Same shape as blst_p1s_mult_pippenger incl. the NULL-terminated pointer-to-array convention
// (blst+nim.h:70-72; benchmarks/bls12381_msm_g1.nim:52-59), but with a context, an int result and 32-byte scalar images
// (blst_scalar arrays) whatever nbits is: points[0] / scalars[0] are contiguous arrays in HOST memory.
extern "C" int mi355_bls_p1s_mult_pippenger(mi355_bls_ctx* c, uint8_t ret_p1[144], const void* const points[], size_t npoints,
                                            const uint8_t* const scalars[], size_t nbits) {
    if (!c || !ret_p1) return MI355_BLS_ERR_ARG;
    if (npoints == 0) {
        memset(ret_p1, 0, 144);
        return 0;
    }
    if (!points || !points[0] || !scalars || !scalars[0] || nbits == 0 || nbits > 256) return MI355_BLS_ERR_ARG;
    return msm_host<fp>(c, ret_p1, (const uint8_t*)points[0], npoints, scalars[0], 32, nbits);
}
extern "C" int mi355_bls_p2s_mult_pippenger(mi355_bls_ctx* c, uint8_t ret_p2[288], const void* const points[], size_t npoints,
                                            const uint8_t* const scalars[], size_t nbits) {
    if (!c || !ret_p2) return MI355_BLS_ERR_ARG;
    if (npoints == 0) {
        memset(ret_p2, 0, 288);
        return 0;
    }
    if (!points || !points[0] || !scalars || !scalars[0] || nbits == 0 || nbits > 256) return MI355_BLS_ERR_ARG;
    return msm_host<fp2>(c, ret_p2, (const uint8_t*)points[0], npoints, scalars[0], 32, nbits);
}

// ------------------------------------------------------------------------------------------
// k G1 MSMs in one device pass (mi355_bls_p1s_mult_pippenger_many), and k G2 MSMs (mi355_bls_p2s_mult_pippenger_many): a walk over
// plan::msm_many_for / msm_many_next.  One driver over the field: F = fp is the G1 call's launch sequence as it was before the G2 form
// existed; F = fp2 differs where the plan says so (384-byte points, k_pip_segred<fp2> alone, k_pip_tail_many_g2).
// ------------------------------------------------------------------------------------------
// The argument rules of both entries, made without looking into the context: 0 go on, 1 nothing to do (k == 0), or the error.
static int msm_many_check(const mi355_bls_ctx* c, const void* ret, const void* d_out, const void* points, size_t npoints, const void* scalars, const size_t* offsets,
                          size_t k, size_t nbits) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 1;
    if ((!ret && !d_out) || nbits == 0 || nbits > 256) return MI355_BLS_ERR_ARG;
    if (offsets) {
        if (offsets[0] != 0 || offsets[k] != npoints) return MI355_BLS_ERR_ARG;
        for (size_t j = 0; j < k; j++)
            if (offsets[j + 1] < offsets[j] || offsets[j + 1] - offsets[j] > ((size_t)1 << 28)) return MI355_BLS_ERR_ARG;      // (the single call's limit on one MSM)
    } else if (npoints > ((size_t)1 << 28)) {
        return MI355_BLS_ERR_ARG;
    }
    if (npoints && (!points || !scalars)) return MI355_BLS_ERR_ARG;
    return 0;
}
// Arguments checked (msm_many_check returned 0).  Every pass is enqueued on `st`; the results land in d_out (or the workspace's own k x 144
// (G2: 288) bytes), are copied to ret, and the stream is waited for, as the single call does.
template <class F>
static int msm_many_run(mi355_bls_ctx* c, uint8_t* ret, void* d_out, const void* d_points, size_t npoints, const void* d_scalars, const size_t* offsets, size_t k,
                        size_t nbits, hipStream_t st) {
    constexpr bool G2 = sizeof(F) != sizeof(fp);
    constexpr size_t AFFB = G2 ? 192 : 96, JACB = AFFB / 2 * 3, JACW = JACB / 4;
    msm_many_ws* m = G2 ? &c->msm_many2 : &c->msm_many;
    const plan::msm_many_plan P = plan::msm_many_for(k, npoints, offsets == nullptr, nbits, G2);
    const plan::msm_many_sizes sz = plan::msm_many_sizes_for(P, offsets, npoints, k);
    int rc = 0;
    const auto grow = [&rc](auto& buf, size_t bytes) { rc = rc ? rc : buf.reserve(bytes, 0); };
    grow(m->pts_int, sz.pts_int), grow(m->offs_dev, sz.offs_dev), grow(m->hist, sz.hist), grow(m->offs, sz.hist), grow(m->cursor, sz.hist), grow(m->order, sz.hist);
    grow(m->chist, sz.chist), grow(m->sorted, sz.sorted), grow(m->buckets, sz.buckets), grow(m->segout, sz.segout), grow(m->part, sz.part);
    if (!d_out) grow(m->out, k * JACB);
    if (rc) return rc;
    uint32_t* dst = d_out ? (uint32_t*)d_out : m->out.p;
    const uint8_t* pts = (const uint8_t*)d_points;
    const uint8_t* sc = (const uint8_t*)d_scalars;
    const pip_win W{P.W};
    const uint32_t nw = W.nwin;
    // the offsets of every ragged pass, relative to its first pair: one array that no pass of the call moves
    size_t words = 0;
    if (offsets)
        for (size_t j = 0; j < k;) {
            const plan::msm_many_pass s = plan::msm_many_next(P, offsets, npoints, k, j);
            words += s.single ? 0 : s.j1 - s.j0 + 1;
            j = s.j1;
        }
    c->many_offs.assign(words, 0);
    size_t used = 0;
    bool converted = false, timed = false;
    for (size_t j = 0; j < k;) {
        const plan::msm_many_pass s = plan::msm_many_next(P, offsets, npoints, k, j);
        j = s.j1;
        uint32_t* out = dst + s.j0 * JACW;
        if (s.single) {
            const size_t n = offsets ? offsets[s.j0 + 1] - offsets[s.j0] : npoints;
            if (n == 0) {
                HIPCHK(hipMemsetAsync(out, 0, JACB, st));
                continue;
            }
            rc = msm_enqueue<F>(c, &c->msm, pts + (offsets ? s.pair0 * AFFB : 0), n, sc + s.pair0 * 32, 32, nbits, st, false, true);
            if (rc) return rc;
            HIPCHK(hipMemcpyAsync(out, c->msm.out, JACB, hipMemcpyDeviceToDevice, st));
            continue;
        }
        const uint32_t kp = (uint32_t)(s.j1 - s.j0);
        if (s.pairs == 0) {
            HIPCHK(hipMemsetAsync(out, 0, (size_t)kp * JACB, st));
            continue;
        }
        const many_addr A{s.pairs, kp, offsets ? 0u : (uint32_t)npoints, nw, W.cbk};
        if (offsets) {
            uint32_t* rel = c->many_offs.data() + used;
            for (uint32_t i = 0; i <= kp; i++) rel[i] = (uint32_t)(offsets[s.j0 + i] - s.pair0);
            used += kp + 1;
            HIPCHK(hipMemcpyAsync(m->offs_dev, rel, ((size_t)kp + 1) * 4, hipMemcpyHostToDevice, st));
        }
        const uint8_t* psc = sc + s.pair0 * 32;
        HIPCHK(hipMemsetAsync(m->hist, 0, (size_t)s.total * 4, st));
        HIPCHK(hipMemsetAsync(m->chist, 0, 256 * 4, st));
        const bool t = !timed;
        timed = true;
        if (t) HIPCHK(hipEventRecord(c->ev[0], st));
        if (offsets) k_pip_convert<F><<<plan::waves_for(s.points), WAVE, 0, st>>>(pts + s.pair0 * AFFB, s.points, m->pts_int);
        else if (!converted) k_pip_convert<F><<<plan::waves_for(s.points), WAVE, 0, st>>>(pts, s.points, m->pts_int);      // the shared points: once per call
        converted = true;
        k_pipm_hist<<<dim3(s.pair_grid, nw), WAVE, 0, st>>>(psc, A, m->offs_dev, W, m->hist);
        k_pipm_scan<<<s.nv, WAVE, 0, st>>>(m->hist, A, m->offs_dev, m->offs, m->cursor);
        k_pipm_scatter<<<dim3(s.pair_grid, nw), WAVE, 0, st>>>(psc, A, m->offs_dev, W, m->cursor, m->sorted);
        k_msm_order_hist<<<s.order_grid, WAVE, 0, st>>>(m->hist, s.total, m->chist);
        k_msm_order_scan<<<1, 1, 0, st>>>(m->chist);
        k_msm_order_scatter<<<s.order_grid, WAVE, 0, st>>>(m->hist, s.total, m->chist, m->order);
        if (t) HIPCHK(hipEventRecord(c->ev[1], st));
        // offs holds positions in `sorted` itself (k_pipm_scan): n = 0 takes k_pip_bucket's own window x n out
        k_pip_bucket<F><<<s.bucket_grid, WAVE, 0, st>>>(m->pts_int, m->sorted, m->offs, m->hist, m->order, 0, W.cbk, s.total, 0, s.total, m->buckets);
        if (t) HIPCHK(hipEventRecord(c->ev[2], st));
        if (!G2 && s.team == 4) k_pip_segred_team<4><<<s.segred_grid, WAVE, 0, st>>>(m->buckets, s.total, W.cbk, plan::MSM_SEG, s.nseg, 0, s.nseg, m->segout);
        else if (!G2 && s.team == 2) k_pip_segred_team<2><<<s.segred_grid, WAVE, 0, st>>>(m->buckets, s.total, W.cbk, plan::MSM_SEG, s.nseg, 0, s.nseg, m->segout);
        else k_pip_segred<F><<<s.segred_grid, WAVE, 0, st>>>(m->buckets, s.total, W.cbk, plan::MSM_SEG, s.nseg, 0, s.nseg, m->segout);
        k_pip_winpart<F><<<dim3(s.nv, P.nsplit), WAVE, 0, st>>>(m->segout, s.nseg, P.segs_per_win, 0, m->part);
        if (t) HIPCHK(hipEventRecord(c->ev[3], st));
        if constexpr (G2) k_pip_tail_many_g2<<<kp, P.tail_lanes, 0, st>>>(m->part, P.nsplit, W, out);      // one Horner walk per MSM, the G2 way
        else k_pip_rowtail_many<<<kp, P.tail_lanes, 0, st>>>(m->part, P.nsplit, W, out);
        if (t) HIPCHK(hipEventRecord(c->ev[4], st));
        HIPCHK(hipGetLastError());
    }
    if (ret) HIPCHK(hipMemcpyAsync(ret, dst, k * JACB, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (timed) return collect_timings(c, 4);       // the first pass's stages: [0] sort and order, [1] bucket accumulation, [2] reductions, [3] the tails
    for (float& t : c->timings) t = 0;             // every step took the single path (untimed here): no stale stages of an earlier call
    return 0;
}
extern "C" int mi355_bls_p1s_mult_pippenger_many_device(mi355_bls_ctx* c, uint8_t* ret, void* d_out, const void* d_points, size_t npoints, const void* d_scalars,
                                                        const size_t* offsets, size_t k, size_t nbits, void* stream) {
    const int chk = msm_many_check(c, ret, d_out, d_points, npoints, d_scalars, offsets, k, nbits);
    if (chk) return chk < 0 ? chk : 0;
    HIPCHK(hipSetDevice(c->device));
    return msm_many_run<fp>(c, ret, d_out, d_points, npoints, d_scalars, offsets, k, nbits, (hipStream_t)stream);
}
// host arrays -> staging -> msm_many_run on the null stream
template <class F>
static int msm_many_host(mi355_bls_ctx* c, uint8_t* ret, const void* points, size_t npoints, const void* scalars, const size_t* offsets, size_t k, size_t nbits) {
    constexpr bool G2 = sizeof(F) != sizeof(fp);
    constexpr size_t AFFB = G2 ? 192 : 96, JACB = AFFB / 2 * 3;
    const int chk = msm_many_check(c, ret, ret, points, npoints, scalars, offsets, k, nbits);
    if (chk) return chk < 0 ? chk : 0;
    if (npoints == 0) {
        memset(ret, 0, k * JACB);
        return 0;
    }
    HIPCHK(hipSetDevice(c->device));
    msm_many_ws* m = G2 ? &c->msm_many2 : &c->msm_many;
    const size_t nsc = offsets ? npoints : npoints * k;
    int rc = m->d_pts.reserve(npoints * AFFB, 0);
    rc = rc ? rc : m->d_sc.reserve(nsc * 32, 0);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(m->d_pts, points, npoints * AFFB, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(m->d_sc, scalars, nsc * 32, hipMemcpyHostToDevice, nullptr));
    return msm_many_run<F>(c, ret, nullptr, m->d_pts, npoints, m->d_sc, offsets, k, nbits, nullptr);
}
extern "C" int mi355_bls_p1s_mult_pippenger_many(mi355_bls_ctx* c, uint8_t* ret, const void* points, size_t npoints, const void* scalars, const size_t* offsets,
                                                 size_t k, size_t nbits) {
    return msm_many_host<fp>(c, ret, points, npoints, scalars, offsets, k, nbits);
}
// the G2 form: 192-byte blst_p2_affine images in, blst_p2 images (288 B) out; a d_out that is not 4-byte aligned is refused with the other rules
extern "C" int mi355_bls_p2s_mult_pippenger_many_device(mi355_bls_ctx* c, uint8_t* ret, void* d_out, const void* d_points, size_t npoints, const void* d_scalars,
                                                        const size_t* offsets, size_t k, size_t nbits, void* stream) {
    const int chk = msm_many_check(c, ret, d_out, d_points, npoints, d_scalars, offsets, k, nbits);
    if (chk) return chk < 0 ? chk : 0;
    if ((uintptr_t)d_out & 3) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    return msm_many_run<fp2>(c, ret, d_out, d_points, npoints, d_scalars, offsets, k, nbits, (hipStream_t)stream);
}
extern "C" int mi355_bls_p2s_mult_pippenger_many(mi355_bls_ctx* c, uint8_t* ret, const void* points, size_t npoints, const void* scalars, const size_t* offsets,
                                                 size_t k, size_t nbits) {
    return msm_many_host<fp2>(c, ret, points, npoints, scalars, offsets, k, nbits);
}

// ------------------------------------------------------------------------------------------
// Jacobian images to affine images, n at once (blst_p1s_to_affine / blst_p2s_to_affine, blst_abi.nim:323, :345): a walk over
// plan::to_affine_for / to_affine_next, one k_to_affine launch per chunk, all on `st`, waited for once.
// ------------------------------------------------------------------------------------------
template <class F>
static int to_affine_run_dev(mi355_bls_ctx* c, const void* d_in, size_t n, void* d_out, hipStream_t st) {
    constexpr size_t AFFB = sizeof(F) == sizeof(fp) ? 96 : 192, JACB = AFFB / 2 * 3;
    const plan::to_affine_plan p = plan::to_affine_for(n, c->toaff_run);
    for (size_t first = 0; first < n;) {
        const plan::to_affine_launch l = plan::to_affine_next(p, n, first);
        k_to_affine<F><<<l.grid, WAVE, 0, st>>>((const uint32_t*)((const uint8_t*)d_in + first * JACB), l.n, p.run, (uint32_t*)((uint8_t*)d_out + first * AFFB));
        first += l.n;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return 0;
}
template <class F>
static int to_affine_device(mi355_bls_ctx* c, const void* d_in, size_t n, void* d_out, void* stream) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!d_in || !d_out || (((uintptr_t)d_in | (uintptr_t)d_out) & 3)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    return to_affine_run_dev<F>(c, d_in, n, d_out, (hipStream_t)stream);
}
template <class F>
static int to_affine_host(mi355_bls_ctx* c, const uint8_t* in, size_t n, uint8_t* out) {
    constexpr size_t AFFB = sizeof(F) == sizeof(fp) ? 96 : 192, JACB = AFFB / 2 * 3;
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!in || !out) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    int rc = c->d_toaff_in.reserve(n * JACB, 0);
    rc = rc ? rc : c->d_toaff_out.reserve(n * AFFB, 0);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(c->d_toaff_in, in, n * JACB, hipMemcpyHostToDevice, nullptr));
    rc = to_affine_run_dev<F>(c, c->d_toaff_in, n, c->d_toaff_out, nullptr);
    if (rc) return rc;
    HIPCHK(hipMemcpy(out, c->d_toaff_out, n * AFFB, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int mi355_bls_p1s_to_affine(mi355_bls_ctx* c, const uint8_t* in144, size_t n, uint8_t* out96) { return to_affine_host<fp>(c, in144, n, out96); }
extern "C" int mi355_bls_p2s_to_affine(mi355_bls_ctx* c, const uint8_t* in288, size_t n, uint8_t* out192) { return to_affine_host<fp2>(c, in288, n, out192); }
extern "C" int mi355_bls_p1s_to_affine_device(mi355_bls_ctx* c, const void* d_in144, size_t n, void* d_out96, void* stream) {
    return to_affine_device<fp>(c, d_in144, n, d_out96, stream);
}
extern "C" int mi355_bls_p2s_to_affine_device(mi355_bls_ctx* c, const void* d_in288, size_t n, void* d_out192, void* stream) {
    return to_affine_device<fp2>(c, d_in288, n, d_out192, stream);
}
extern "C" int mi355_bls_debug_to_affine_set_run(mi355_bls_ctx* c, uint32_t run) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->toaff_run = run;
    return 0;
}

// ------------------------------------------------------------------------------------------
// Fixed-base G1 MSM over a precomputed window table (blst_p1s_mult_wbits_precompute / blst_p1s_mult_wbits, blst_abi.nim:327-335): a walk
// over plan::fixed_for / fixed_next
// ------------------------------------------------------------------------------------------
extern "C" size_t mi355_bls_p1s_table_sizeof(size_t npoints, size_t wbits, size_t nbits) { return plan::fixed_table_bytes(npoints, wbits, nbits); }
extern "C" void mi355_bls_p1s_table_destroy(mi355_bls_p1s_table* tab) { delete tab; }
extern "C" int mi355_bls_p1s_table_create_device(mi355_bls_ctx* c, mi355_bls_p1s_table** out, const void* d_points, size_t npoints, size_t wbits, size_t nbits,
                                                 void* stream) {
    if (!c || !out || !d_points || !plan::fixed_args_ok(npoints, wbits, nbits)) return MI355_BLS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    std::unique_ptr<mi355_bls_p1s_table> t(new mi355_bls_p1s_table());
    t->device = c->device, t->npoints = npoints, t->nbits = (uint32_t)nbits;
    t->wbits = wbits ? (uint32_t)wbits : plan::fixed_wbits_for(npoints);
    t->nwin = plan::fixed_nwin(t->wbits, nbits);
    const uint32_t chunk = plan::fixed_rows_chunk(npoints, t->nwin);
    int rc = t->rows.alloc(plan::fixed_table_bytes(npoints, t->wbits, nbits));
    rc = rc ? rc : c->ptab.scratch.reserve((size_t)chunk * t->nwin * plan::FIXED_ENTRY_BYTES, 0);
    if (rc) return rc;
    for (size_t i0 = 0; i0 < npoints; i0 += chunk) {
        const uint32_t cnt = (uint32_t)(npoints - i0 < chunk ? npoints - i0 : chunk);
        k_ptab_rows<<<plan::waves_for(cnt), WAVE, 0, st>>>((const uint8_t*)d_points, (uint32_t)npoints, (uint32_t)i0, cnt, t->nwin, t->wbits, t->rows, c->ptab.scratch);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    *out = t.release();
    return 0;
}
// host array -> staging -> create_device on the null stream
extern "C" int mi355_bls_p1s_table_create(mi355_bls_ctx* c, mi355_bls_p1s_table** out, const void* points96, size_t npoints, size_t wbits, size_t nbits) {
    if (!c || !out || !points96 || !plan::fixed_args_ok(npoints, wbits, nbits)) return MI355_BLS_ERR_ARG;
    const uint8_t* d[1];
    if (int rc = stage_inputs(c, {{points96, npoints * 96}}, nullptr, d)) return rc;
    return mi355_bls_p1s_table_create_device(c, out, d[0], npoints, wbits, nbits, nullptr);
}
// The argument rules of the mult entries, made without looking into the context: 0 go on, 1 nothing to do (k == 0), or the error.
static int ptab_check(const mi355_bls_ctx* c, const void* ret, const void* d_out, const mi355_bls_p1s_table* tab, const void* scalars, size_t k, size_t nbits) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (k == 0) return 1;
    if (!tab || !scalars || (!ret && !d_out) || nbits == 0 || nbits > 256 || nbits > tab->nbits || tab->device != c->device) return MI355_BLS_ERR_ARG;
    return 0;
}
// Arguments checked (ptab_check returned 0).  Every pass is enqueued on `st`; the results land in d_out (or the workspace's own k x 144 bytes),
// are copied to ret, and the stream is waited for once.
static int ptab_run(mi355_bls_ctx* c, uint8_t* ret, void* d_out, const mi355_bls_p1s_table* tab, const void* d_scalars, size_t k, size_t nbits, hipStream_t st) {
    ptab_ws* m = &c->ptab;
    const plan::fixed_plan P = plan::fixed_for(tab->npoints, plan::fixed_win(tab->wbits, nbits), k, c->slots, m->pairs_max ? m->pairs_max : plan::FIXED_PAIRS_MAX, m->force_S);
    const plan::fixed_sizes sz = plan::fixed_sizes_for(P, k);
    int rc = 0;
    const auto grow = [&rc](auto& buf, size_t bytes) { rc = rc ? rc : buf.reserve(bytes, 0); };
    grow(m->hist, sz.hist), grow(m->offs, sz.hist), grow(m->cursor, sz.hist), grow(m->order, sz.hist), grow(m->chist, sz.chist), grow(m->sorted, sz.sorted);
    grow(m->buckets, sz.buckets), grow(m->segout, sz.segout), grow(m->part, sz.part);
    if (!d_out) grow(m->out, k * 144);
    if (rc) return rc;
    m->last_plan[0] = P.W.nwin, m->last_plan[1] = P.S, m->last_plan[2] = 1u << P.W.cbk;
    uint32_t* dst = d_out ? (uint32_t*)d_out : m->out.p;
    const uint8_t* sc = (const uint8_t*)d_scalars;
    const pip_win W{P.W};
    pip_win Wsum{};                                      // S windows of width 0: k_pip_rowtail_many's walk adds an MSM's S parts and doubles nothing
    Wsum.nwin = P.S;
    bool timed = false;
    for (size_t j = 0; j < k;) {
        const plan::fixed_pass s = plan::fixed_next(P, k, j);
        j = s.j1;
        const uint32_t kp = (uint32_t)(s.j1 - s.j0);
        const fixed_addr A{s.pairs, P.n, W.nwin, P.S, W.cbk};
        const uint8_t* psc = sc + s.pair0 * 32;
        HIPCHK(hipMemsetAsync(m->hist, 0, (size_t)s.total * 4, st));
        HIPCHK(hipMemsetAsync(m->chist, 0, 256 * 4, st));
        const bool t = !timed;
        timed = true;
        if (t) HIPCHK(hipEventRecord(c->ev[0], st));
        k_ptab_hist<<<dim3(s.pair_grid, W.nwin), WAVE, 0, st>>>(psc, A, W, m->hist);
        k_ptab_scan<<<s.nv, WAVE, 0, st>>>(m->hist, A, m->offs, m->cursor);
        k_ptab_scatter<<<dim3(s.pair_grid, W.nwin), WAVE, 0, st>>>(psc, A, W, m->cursor, m->sorted);
        k_msm_order_hist<<<s.order_grid, WAVE, 0, st>>>(m->hist, s.total, m->chist);
        k_msm_order_scan<<<1, 1, 0, st>>>(m->chist);
        k_msm_order_scatter<<<s.order_grid, WAVE, 0, st>>>(m->hist, s.total, m->chist, m->order);
        if (t) HIPCHK(hipEventRecord(c->ev[1], st));
        // the records are the table's rows; offs holds positions in `sorted` itself (k_ptab_scan): n = 0 takes k_pip_bucket's own window x n out
        k_pip_bucket<fp><<<s.bucket_grid, WAVE, 0, st>>>(tab->rows, m->sorted, m->offs, m->hist, m->order, 0, W.cbk, s.total, 0, s.total, m->buckets);
        if (t) HIPCHK(hipEventRecord(c->ev[2], st));
        if (s.team == 4) k_pip_segred_team<4><<<s.segred_grid, WAVE, 0, st>>>(m->buckets, s.total, W.cbk, plan::MSM_SEG, s.nseg, 0, s.nseg, m->segout);
        else if (s.team == 2) k_pip_segred_team<2><<<s.segred_grid, WAVE, 0, st>>>(m->buckets, s.total, W.cbk, plan::MSM_SEG, s.nseg, 0, s.nseg, m->segout);
        else k_pip_segred<fp><<<s.segred_grid, WAVE, 0, st>>>(m->buckets, s.total, W.cbk, plan::MSM_SEG, s.nseg, 0, s.nseg, m->segout);
        k_pip_winpart<fp><<<dim3(s.nv, P.nsplit), WAVE, 0, st>>>(m->segout, s.nseg, P.segs_per_set, 0, m->part);
        if (t) HIPCHK(hipEventRecord(c->ev[3], st));
        k_pip_rowtail_many<<<kp, P.tail_lanes, 0, st>>>(m->part, P.nsplit, Wsum, dst + s.j0 * 36);
        if (t) HIPCHK(hipEventRecord(c->ev[4], st));
        HIPCHK(hipGetLastError());
    }
    if (ret) HIPCHK(hipMemcpyAsync(ret, dst, k * 144, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return collect_timings(c, 4);       // the first pass's stages: [0] sort and order, [1] bucket accumulation, [2] reductions, [3] the sums
}
extern "C" int mi355_bls_p1s_mult_table_many_device(mi355_bls_ctx* c, uint8_t* ret, void* d_out, const mi355_bls_p1s_table* tab, const void* d_scalars, size_t k,
                                                    size_t nbits, void* stream) {
    const int chk = ptab_check(c, ret, d_out, tab, d_scalars, k, nbits);
    if (chk) return chk < 0 ? chk : 0;
    HIPCHK(hipSetDevice(c->device));
    return ptab_run(c, ret, d_out, tab, d_scalars, k, nbits, (hipStream_t)stream);
}
// host array -> staging -> ptab_run on the null stream
extern "C" int mi355_bls_p1s_mult_table_many(mi355_bls_ctx* c, uint8_t* ret, const mi355_bls_p1s_table* tab, const void* scalars32, size_t k, size_t nbits) {
    const int chk = ptab_check(c, ret, nullptr, tab, scalars32, k, nbits);
    if (chk) return chk < 0 ? chk : 0;
    const uint8_t* d[1];
    if (int rc = stage_inputs(c, {{scalars32, k * tab->npoints * 32}}, nullptr, d)) return rc;
    return ptab_run(c, ret, nullptr, tab, d[0], k, nbits, nullptr);
}
extern "C" int mi355_bls_p1s_mult_table_device(mi355_bls_ctx* c, uint8_t ret_p1[144], const mi355_bls_p1s_table* tab, const void* d_scalars, size_t nbits, void* stream) {
    if (!ret_p1) return MI355_BLS_ERR_ARG;
    return mi355_bls_p1s_mult_table_many_device(c, ret_p1, nullptr, tab, d_scalars, 1, nbits, stream);
}
extern "C" int mi355_bls_p1s_mult_table(mi355_bls_ctx* c, uint8_t ret_p1[144], const mi355_bls_p1s_table* tab, const void* scalars32, size_t nbits) {
    if (!ret_p1) return MI355_BLS_ERR_ARG;
    return mi355_bls_p1s_mult_table_many(c, ret_p1, tab, scalars32, 1, nbits);
}
extern "C" int mi355_bls_debug_p1s_table_rows(const mi355_bls_p1s_table* tab, size_t w0, size_t nw, size_t i0, size_t ni, uint8_t* out96) {
    if (!tab || !out96 || w0 > tab->nwin || nw > tab->nwin - w0 || i0 > tab->npoints || ni > tab->npoints - i0 || nw * ni > ((size_t)1 << 24)) return MI355_BLS_ERR_ARG;
    if (nw * ni == 0) return 0;
    HIPCHK(hipSetDevice(tab->device));
    dev_buf<uint32_t> d;
    if (int rc = d.alloc(nw * ni * 96)) return rc;
    k_debug_ptab_rows<<<plan::waves_for((uint32_t)(nw * ni)), WAVE, 0, nullptr>>>(tab->rows, (uint32_t)tab->npoints, (uint32_t)w0, (uint32_t)nw, (uint32_t)i0, (uint32_t)ni, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out96, d, nw * ni * 96, hipMemcpyDeviceToHost));
    return 0;
}
extern "C" int mi355_bls_debug_p1s_table_last_plan(mi355_bls_ctx* c, uint32_t out[3]) {
    if (!c || !out) return MI355_BLS_ERR_ARG;
    for (int i = 0; i < 3; i++) out[i] = c->ptab.last_plan[i];
    return 0;
}
extern "C" int mi355_bls_debug_p1s_table_set_plan(mi355_bls_ctx* c, uint32_t force_sets, uint32_t pairs_max) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->ptab.force_S = force_sets, c->ptab.pairs_max = pairs_max;
    return 0;
}

// blst's list convention (blst_p1s_mult_pippenger and friends): list[0] points at element 0; for every following element the
// next list entry is used if it is non-NULL, otherwise the element follows the previous one in memory.  [ptr, NULL] is one
// contiguous array (what the reference passes, benchmarks/bls12381_msm_g1.nim:52-55, core :613-616); npoints pointers
// address every element individually.  Returns a contiguous view (gathered into tmp when needed).
static const uint8_t* gather_list(const void* const list[], size_t n, size_t elem, std::vector<uint8_t>& tmp) {
    const uint8_t* cur = (const uint8_t*)list[0];
    if (n <= 1 || list[1] == nullptr) return cur;
    tmp.resize(n * elem);
    std::memcpy(tmp.data(), cur, elem);
    size_t li = 1;
    for (size_t i = 1; i < n; i++) {
        if (list[li]) cur = (const uint8_t*)list[li++];
        else cur += elem;
        std::memcpy(tmp.data() + i * elem, cur, elem);
    }
    return tmp.data();
}
[[noreturn]] static void die_no_error_channel(const char* fn) {
    std::fprintf(stderr, "%s: %s (this entry point has blst's void signature, so a runtime failure cannot be returned; aborting rather than "
                 "handing back a wrong point)\n", fn, g_err.c_str());
    std::abort();
}

// EXACTLY blst_p1s_mult_pippenger / blst_p2s_mult_pippenger (blst+nim.h:70-72,90-92; blst_abi.nim:336-340,358-362): no context
// (the process-wide default one), void, scalars (nbits + 7) / 8 bytes apart, scratch ignored (the workspace lives on the device).
template <class F>
static void blst_shaped_pippenger(const char* fn, void* ret, const void* const points[], size_t npoints, const uint8_t* const scalars[], size_t nbits) {
    constexpr size_t AFFB = sizeof(F) == sizeof(fp) ? 96 : 192, JACB = AFFB / 2 * 3;
    if (!ret) return;
    if (npoints == 0) {
        std::memset(ret, 0, JACB);
        return;
    }
    if (!points || !points[0] || !scalars || !scalars[0] || nbits == 0 || nbits > 256) {
        g_err = "bad arguments";
        die_no_error_channel(fn);
    }
    std::lock_guard<std::mutex> lk(g_default_mu);
    mi355_bls_ctx* c;
    uint32_t sbytes = (uint32_t)((nbits + 7) / 8);
    std::vector<uint8_t> tp, ts;
    const uint8_t* P = gather_list(points, npoints, AFFB, tp);
    const uint8_t* S = gather_list(reinterpret_cast<const void* const*>(scalars), npoints, sbytes, ts);
    int rc = default_ctx_locked(1024, &c);
    if (!rc) rc = msm_host<F>(c, (uint8_t*)ret, P, npoints, S, sbytes, nbits);
    if (rc) die_no_error_channel(fn);
}
extern "C" size_t mi355_p1s_mult_pippenger_scratch_sizeof(size_t npoints) {
    (void)npoints;
    return 8;                       // never 0: callers malloc() it (benchmarks/bls12381_msm_g1.nim:50) and index scratch[0] (core :633)
}
extern "C" size_t mi355_p2s_mult_pippenger_scratch_sizeof(size_t npoints) {
    (void)npoints;
    return 8;
}
extern "C" void mi355_p1s_mult_pippenger(void* ret, const void* const points[], size_t npoints, const uint8_t* const scalars[], size_t nbits, void* scratch) {
    (void)scratch;
    blst_shaped_pippenger<fp>("mi355_p1s_mult_pippenger", ret, points, npoints, scalars, nbits);
}
extern "C" void mi355_p2s_mult_pippenger(void* ret, const void* const points[], size_t npoints, const uint8_t* const scalars[], size_t nbits, void* scratch) {
    (void)scratch;
    blst_shaped_pippenger<fp2>("mi355_p2s_mult_pippenger", ret, points, npoints, scalars, nbits);
}

// ------------------------------------------------------------------------------------------
// Wire-format entry points: batched fromBytes (+ batchVerify)
// ------------------------------------------------------------------------------------------
// k_deser over n rows of device memory -> the records at d_sets (and at out_sets, where the caller gave it), as a status pass between ev0 and ev1
static int deser_pass(mi355_bls_ctx* c, const void* d_pks, const void* d_msgs, const void* d_sigs, size_t n, uint32_t dflags, hipStream_t st, void* out_sets,
                      uint8_t* status, hipEvent_t ev0, hipEvent_t ev1) {
    if (int rc = io_reserve(c, n)) return rc;
    if (dflags > 7) return MI355_BLS_ERR_ARG;
    const uint8_t *pk = (const uint8_t*)d_pks, *ms = (const uint8_t*)d_msgs, *sg = (const uint8_t*)d_sigs;
    const auto enqueue = [&] { k_deser<<<plan::waves_for((uint32_t)n), WAVE, 0, st>>>(pk, ms, sg, (uint32_t)n, dflags, c->d_sets, c->d_status, c->d_flags); };
    return status_pass(c, st, n, status, ev0, ev1, enqueue, out_sets, c->d_sets, n * 320);
}

extern "C" int mi355_bls_deserialize_sets_ex_device(mi355_bls_ctx* c, const void* d_pks48, const void* d_msgs32, const void* d_sigs96, size_t n, uint32_t dflags,
                                                    void* stream, void* out_sets, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 1;
    if (!d_pks48 || !d_msgs32 || !d_sigs96) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    return one_stage_timings(c, deser_pass(c, d_pks48, d_msgs32, d_sigs96, n, dflags, (hipStream_t)stream, out_sets, status, c->ev[0], c->ev[1]));
}
extern "C" int mi355_bls_deserialize_sets_device(mi355_bls_ctx* c, const void* d_pks48, const void* d_msgs32, const void* d_sigs96, size_t n, void* stream,
                                                 void* out_sets, uint8_t* status) {
    return mi355_bls_deserialize_sets_ex_device(c, d_pks48, d_msgs32, d_sigs96, n, 0, stream, out_sets, status);
}

// host wire-format arrays -> their columns
static int stage_compressed(mi355_bls_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint8_t* sigs, size_t n, uint32_t dflags) {
    if (int rc = io_reserve(c, n)) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(col_at(c, cols::SETS_KEYS), pks, n * ((dflags & DESER_F_PK_UNCOMPRESSED) ? 96 : 48), hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(col_at(c, cols::SETS_MSGS), msgs, n * 32, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(col_at(c, cols::SETS_SIGS), sigs, n * ((dflags & DESER_F_SIG_UNCOMPRESSED) ? 192 : 96), hipMemcpyHostToDevice, nullptr));
    return 0;
}
extern "C" int mi355_bls_deserialize_sets_ex(mi355_bls_ctx* c, const uint8_t* pks, const uint8_t* msgs32, const uint8_t* sigs, size_t n, uint32_t dflags,
                                             void* out_sets, uint8_t* status) {
    if (!c || dflags > 7) return MI355_BLS_ERR_ARG;
    if (n == 0) return 1;
    if (!pks || !msgs32 || !sigs) return MI355_BLS_ERR_ARG;
    if (int rc = stage_compressed(c, pks, msgs32, sigs, n, dflags)) return rc;
    return mi355_bls_deserialize_sets_ex_device(c, col_at(c, cols::SETS_KEYS), col_at(c, cols::SETS_MSGS), col_at(c, cols::SETS_SIGS), n, dflags, nullptr, out_sets,
                                                status);
}
extern "C" int mi355_bls_deserialize_sets(mi355_bls_ctx* c, const uint8_t* pks48, const uint8_t* msgs32, const uint8_t* sigs96, size_t n, void* out_sets,
                                          uint8_t* status) {
    return mi355_bls_deserialize_sets_ex(c, pks48, msgs32, sigs96, n, 0, out_sets, status);
}

extern "C" int mi355_bls_batch_verify_compressed_device(mi355_bls_ctx* c, const void* d_pks48, const void* d_msgs32, const void* d_sigs96, size_t n,
                                                        const uint8_t rnd[32], void* stream, uint8_t* status) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!d_pks48 || !d_msgs32 || !d_sigs96) return MI355_BLS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    const int ok = deser_pass(c, d_pks48, d_msgs32, d_sigs96, n, 0, st, nullptr, status, c->ev_deser0, c->ev_deser1);
    if (ok < 0) return ok;
    HIPCHK(hipEventElapsedTime(&c->deser_ms, c->ev_deser0, c->ev_deser1));
    if (!ok) return 0;                                     // some fromBytes failed: the caller never gets to batchVerify
    return verify_common(c, c->d_sets, nullptr, n, rnd, 0, st);
}

extern "C" int mi355_bls_batch_verify_compressed(mi355_bls_ctx* c, const uint8_t* pks48, const uint8_t* msgs32, const uint8_t* sigs96, size_t n,
                                                 const uint8_t rnd[32], uint8_t* status) {
    if (!c || !rnd) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;
    if (!pks48 || !msgs32 || !sigs96) return MI355_BLS_ERR_ARG;
    if (int rc = stage_compressed(c, pks48, msgs32, sigs96, n, 0)) return rc;
    return mi355_bls_batch_verify_compressed_device(c, col_at(c, cols::SETS_KEYS), col_at(c, cols::SETS_MSGS), col_at(c, cols::SETS_SIGS), n, rnd, nullptr, status);
}

extern "C" float mi355_bls_last_deser_ms(mi355_bls_ctx* c) { return c ? c->deser_ms : 0.f; }

// ------------------------------------------------------------------------------------------
// Batch signer (test / bench input generation)
// ------------------------------------------------------------------------------------------
extern "C" int mi355_bls_sign_sets_device(mi355_bls_ctx* c, const void* d_sks32, const void* d_msgs32, size_t n, void* d_out_sets, void* stream,
                                          uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 1;
    if (!d_sks32 || !d_msgs32 || !d_out_sets) return MI355_BLS_ERR_ARG;
    if (int rc = io_reserve(c, n)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    const uint32_t nb = plan::waves_for((uint32_t)n);
    return one_stage_timings(c, status_pass(c, st, n, status, c->ev[0], c->ev[1], [&] {
        k_sign_pk<<<nb, WAVE, 0, st>>>((const uint8_t*)d_sks32, (const uint8_t*)d_msgs32, (uint32_t)n, (uint8_t*)d_out_sets, c->d_status, c->d_flags);
        k_sign_sig<<<nb, WAVE, 0, st>>>((const uint8_t*)d_sks32, (const uint8_t*)d_msgs32, (uint32_t)n, c->dst, (uint8_t*)d_out_sets);
    }));
}

extern "C" int mi355_bls_sign_sets(mi355_bls_ctx* c, const uint8_t* sks32, const uint8_t* msgs32, size_t n, void* out_sets, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 1;
    if (!sks32 || !msgs32 || !out_sets) return MI355_BLS_ERR_ARG;
    if (int rc = io_reserve(c, n)) return rc;
    HIPCHK(hipSetDevice(c->device));
    uint8_t *d_sk = col_at(c, cols::SIGN_SKS), *d_msg = col_at(c, cols::SIGN_MSGS);
    HIPCHK(hipMemcpyAsync(d_sk, sks32, n * 32, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(d_msg, msgs32, n * 32, hipMemcpyHostToDevice, nullptr));
    int rc = mi355_bls_sign_sets_device(c, d_sk, d_msg, n, c->d_sets, nullptr, status);
    if (rc < 0) return rc;
    HIPCHK(hipMemcpy(out_sets, c->d_sets, n * 320, hipMemcpyDeviceToHost));
    HIPCHK(hipMemsetAsync(d_sk, 0, n * 32, nullptr));               // do not leave the scalars in the staging buffer
    HIPCHK(hipStreamSynchronize(nullptr));
    return rc;
}

// popProve (bls_sig_min_pubkey.nim:34-58) for n secret keys: the keys by k_sign_pk (into the staging records, with zero messages), the proofs by
// k_pop_prove_sig, which also packs the keys.  Variable time: test / bench input generation only, like the signer above.
extern "C" int mi355_bls_pop_prove_device(mi355_bls_ctx* c, const void* d_sks32, size_t n, void* d_out_pks96, void* d_out_proofs192, void* stream, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 1;
    if (!d_sks32 || !d_out_pks96 || !d_out_proofs192 || n > plan::POP_MAX_KEYS) return MI355_BLS_ERR_ARG;
    if (ctx_busy(c)) return MI355_BLS_ERR_ARG;
    if (int rc = io_reserve(c, n)) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    uint8_t* d_zero = col_at(c, cols::PROVE_ZERO_MSGS);            // n x 32 zero bytes: k_sign_pk copies a message into every record
    HIPCHK(hipMemsetAsync(d_zero, 0, n * 32, st));
    const uint32_t nb = plan::waves_for((uint32_t)n);
    return one_stage_timings(c, status_pass(c, st, n, status, c->ev[0], c->ev[1], [&] {
        k_sign_pk<<<nb, WAVE, 0, st>>>((const uint8_t*)d_sks32, d_zero, (uint32_t)n, c->d_sets, c->d_status, c->d_flags);
        k_pop_prove_sig<<<nb, WAVE, 0, st>>>((const uint8_t*)d_sks32, c->d_sets, (uint32_t)n, c->dst_pop, (uint8_t*)d_out_pks96, (uint8_t*)d_out_proofs192);
    }));
}
extern "C" int mi355_bls_pop_prove(mi355_bls_ctx* c, const uint8_t* sks32, size_t n, void* out_pks96, void* out_proofs192, uint8_t* status) {
    if (!c) return MI355_BLS_ERR_ARG;
    if (n == 0) return 1;
    if (!sks32 || !out_pks96 || !out_proofs192 || n > plan::POP_MAX_KEYS) return MI355_BLS_ERR_ARG;
    if (int rc = io_reserve(c, n)) return rc;
    HIPCHK(hipSetDevice(c->device));
    uint8_t *d_sk = col_at(c, cols::PROVE_SKS), *d_keys = col_at(c, cols::PROVE_KEYS), *d_proofs = col_at(c, cols::PROVE_PROOFS);
    HIPCHK(hipMemcpyAsync(d_sk, sks32, n * 32, hipMemcpyHostToDevice, nullptr));
    int rc = mi355_bls_pop_prove_device(c, d_sk, n, d_keys, d_proofs, nullptr, status);
    if (rc < 0) return rc;
    HIPCHK(hipMemcpy(out_pks96, d_keys, n * 96, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(out_proofs192, d_proofs, n * 192, hipMemcpyDeviceToHost));
    HIPCHK(hipMemsetAsync(d_sk, 0, n * 32, nullptr));               // do not leave the scalars in the staging buffer
    HIPCHK(hipStreamSynchronize(nullptr));
    return rc;
}

// ------------------------------------------------------------------------------------------
// combine
// ------------------------------------------------------------------------------------------
extern "C" int mi355_bls_combine(mi355_bls_ctx* c, const uint8_t rnd[32], const void* pks, const void* sigs, size_t n, uint8_t out_pk[96], uint8_t out_sig[192]) {
    if (!c || !rnd || !pks || !sigs || !out_pk || !out_sig || n == 0) return MI355_BLS_ERR_ARG;     // n == 0: the reference raises (core :584)
    if (n == 1) {                                                                                      // passthrough, no scalars (core :585-586)
        memcpy(out_pk, pks, 96);
        memcpy(out_sig, sigs, 192);
        return 0;
    }
    {
        int rcr = io_reserve(c, n);
        if (rcr) return rcr;
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = nullptr;
    uint8_t* d_pk = c->d_sets;                    // staging: n x 96 then n x 192 (<= n x 320)
    uint8_t* d_sg = c->d_sets + n * 96;
    HIPCHK(hipMemcpyAsync(d_pk, pks, n * 96, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_sg, sigs, n * 192, hipMemcpyHostToDevice, st));
    c->h_r.resize(n);
    host_combine_chain(rnd, n, c->h_r.data());
    HIPCHK(hipMemcpyAsync(c->d_r, c->h_r.data(), n * 8, hipMemcpyHostToDevice, st));
    // the reference's two 64-bit Pippenger calls (core :629-646): 8-byte scalars, nbits = 64
    // The two runs are independent: G1 on the caller's stream, G2 on the context's side stream with a workspace of its own, results
    // left on the device for `finish`; one synchronisation at the end (two blocking calls in a row: 7.2 ms at n = 4096).
    hipStream_t s2 = ensure_side(c) ? c->side : st;
    HIPCHK(hipEventRecord(c->ev[0], st));
    if (s2 != st) HIPCHK(hipStreamWaitEvent(s2, c->ev[0], 0));            // the staged inputs
    int rc = msm_enqueue<fp2>(c, &c->msm2, d_sg, n, c->d_r, 8, 64, s2, false, false);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[2], s2));
    rc = msm_enqueue<fp>(c, &c->msm, d_pk, n, c->d_r, 8, 64, st, false, s2 == st);
    if (rc) return rc;
    HIPCHK(hipEventRecord(c->ev[1], st));
    if (s2 != st) HIPCHK(hipStreamWaitEvent(st, c->ev[2], 0));
    // `finish` (to affine, core :172-177)
    uint32_t* d_out = reinterpret_cast<uint32_t*>(c->d_msg.p);
    k_finish_affine<<<1, 1, 0, st>>>(c->msm.out, c->msm2.out, d_out, d_out + 24);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(c->ev[3], st));
    HIPCHK(hipMemcpyAsync(out_pk, d_out, 96, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_sig, d_out + 24, 192, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int i = 0; i < 8; i++) c->timings[i] = 0;
    HIPCHK(hipEventElapsedTime(&c->timings[1], c->ev[0], c->ev[1]));       // G1 Pippenger
    HIPCHK(hipEventElapsedTime(&c->timings[2], c->ev[0], c->ev[2]));       // G2 Pippenger (beside it)
    HIPCHK(hipEventElapsedTime(&c->timings[7], c->ev[0], c->ev[3]));
    c->last_n = n;                  // fetch_stage(0) returns the combine scalars
    return 0;
}

// ------------------------------------------------------------------------------------------
// aggregateVerify
// ------------------------------------------------------------------------------------------
// One slice: pairs [0, n) of the slice (keys, rebased offsets and messages staged in d_sets), `with_sig`: the (-G1, sig) pair rides in
// this slice.  Leaves the slice's committed state in d_states slot 0 (final: also runs the final exponentiation, one-slice calls).
static int aggv_slice(mi355_bls_ctx* c, const uint8_t* pks, const uint8_t* msgs, const uint32_t* offs, size_t n, bool with_sig, bool final, hipStream_t st) {
    size_t total = offs[n];
    const pair_store ps = c->batch_pairs();
    uint8_t* d_pk = c->d_sets;
    uint32_t* d_off = reinterpret_cast<uint32_t*>(c->d_sets + n * 96);
    uint8_t* d_msgs = c->d_sets + n * 96 + (n + 1) * 4;
    HIPCHK(hipMemcpyAsync(d_pk, pks, n * 96, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_off, offs, (n + 1) * 4, hipMemcpyHostToDevice, st));
    if (total) HIPCHK(hipMemcpyAsync(d_msgs, msgs, total, hipMemcpyHostToDevice, st));
    uint32_t n32 = (uint32_t)n, nb = plan::waves_for(n32), npairs = n32 + (with_sig ? 1u : 0u), nb1 = plan::waves_for(npairs);
    HIPCHK(hipEventRecord(c->ev[0], st));
    const bool all32 = c->xmd.valid && plan::aggv_all32(offs, n);       // every message 32 bytes long (signing roots): the batch path's hashing kernels
    if (all32) {
        // k_hash_map reads the message at offset 96 of a 320-byte record: the 32-byte messages are spread to that layout on the device
        // side of the staging buffer (keys | offsets | messages are packed at its start; the records go to d_comp)
        k_aggv_records<<<nb, WAVE, 0, st>>>(d_msgs, n32, c->d_comp);
        launch_hash_map(c, c->d_comp, n32, st);
        launch_hash_clear(c, ps, n32, st);
    } else {
        k_hash_var<<<nb, WAVE, 0, st>>>(d_msgs, d_off, n32, c->dst, ps.H, ps.stride);
    }
    HIPCHK(hipEventRecord(c->ev[1], st));
    k_aggv_setup<<<nb1, WAVE, 0, st>>>(d_pk, n32, with_sig ? 1 : 0, reinterpret_cast<const uint32_t*>(c->d_msg + 4096), ps.H, ps.P, ps.stride, c->d_flags);
    HIPCHK(hipEventRecord(c->ev[2], st));
    launch_lines(ps, plan::lines_for(c->slots, c->coop, npairs, 0), st);
    HIPCHK(hipEventRecord(c->ev[3], st));
    {
        int rcp = enqueue_line_products(c, ps, npairs, st, nullptr);
        if (rcp) return rcp;
    }
    HIPCHK(hipEventRecord(c->ev[4], st));
    launch_k_tail(c, st, c->d_L, c->d_states, 1, final ? 3 : 1, c->d_gt, c->d_flags + 1, 144, 0);
    HIPCHK(hipEventRecord(c->ev[5], st));
    HIPCHK(hipGetLastError());
    return 0;
}

// Any number of pairs: more than the context's capacity (pairs, or staged bytes: keys + offsets + messages share d_sets) are
// processed in slices whose committed states are multiplied on the engine (k_state_mul), as for batchVerify.
static int aggregate_verify_impl(mi355_bls_ctx* c, const void* pks, const uint8_t* msgs, const uint32_t* msg_offsets, size_t n, const void* sig, bool sig_is_p2) {
    if (!c || !sig) return MI355_BLS_ERR_ARG;
    if (n == 0) return 0;                                   // "Spec precondition" (bls_sig_min_pubkey.nim:165-167)
    if (!pks || !msgs || !msg_offsets) return MI355_BLS_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (msg_offsets[i] > msg_offsets[i + 1]) return MI355_BLS_ERR_ARG;      // offsets must be non-decreasing (lengths are differences)
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = nullptr;
    HIPCHK(hipMemsetAsync(c->d_flags, 0, 12, st));
    if (sig_is_p2) {                                        // AggregateSignature (blst_p2, Jacobian): to affine on the device, as finish() does
        HIPCHK(hipMemcpyAsync(c->d_msg + 4096 + 256, sig, 288, hipMemcpyHostToDevice, st));
        k_p2_to_affine<<<1, 1, 0, st>>>(reinterpret_cast<const uint32_t*>(c->d_msg + 4096 + 256), reinterpret_cast<uint32_t*>(c->d_msg + 4096));
    } else {
        HIPCHK(hipMemcpyAsync(c->d_msg + 4096, sig, 192, hipMemcpyHostToDevice, st));
    }
    std::vector<uint32_t> offs;
    size_t a = 0;
    uint32_t slice = 0;
    bool single = true;
    while (a < n) {
        const size_t b = plan::aggv_cut(msg_offsets, n, a, c->cap);      // greedy slice [a, b): at most cap pairs, staged bytes within d_sets
        if (b == a) {
            g_err = "one message does not fit the context's staging buffer";
            return MI355_BLS_ERR_CAPACITY;
        }
        const bool last = b == n;
        if (slice == 0) single = last;
        offs.resize(b - a + 1);
        for (size_t i = a; i <= b; i++) offs[i - a] = msg_offsets[i] - msg_offsets[a];
        int rc = aggv_slice(c, (const uint8_t*)pks + 96 * a, msgs + msg_offsets[a], offs.data(), b - a, last, single, st);
        if (rc) return rc;
        if (!single) {
            k_state_mul<<<1, TAIL_THREADS, 0, st>>>(c->d_states, 1, slice ? 1 : 0, slice ? 0 : -1);
            HIPCHK(hipStreamSynchronize(st));              // offs (host vector) and the staging buffer are reused by the next slice
        }
        a = b;
        slice++;
    }
    if (!single) {
        k_state_mul<<<1, TAIL_THREADS, 0, st>>>(c->d_states, 0, 1, -1);
        launch_k_tail(c, st, c->d_L, c->d_states, 1, 2, c->d_gt, c->d_flags + 1, 144, 0);
        HIPCHK(hipEventRecord(c->ev[5], st));
        HIPCHK(hipGetLastError());
    }
    uint32_t fl[2];
    HIPCHK(hipMemcpyAsync(fl, c->d_flags, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->have_gt = true;
    c->gt_is_fv = false;
    c->last_n = 0;
    int rc = collect_timings(c, 5);
    if (rc) return rc;
    return (fl[0] == 0 && fl[1] == 1) ? 1 : 0;
}

extern "C" int mi355_bls_aggregate_verify(mi355_bls_ctx* c, const void* pks, const uint8_t* msgs, const uint32_t* msg_offsets, size_t n, const void* sig) {
    return aggregate_verify_impl(c, pks, msgs, msg_offsets, n, sig, false);
}
// the same with the signature as an AggregateSignature (blst_p2, Jacobian, 288 B): finish(AggregateSignature), core :357
extern "C" int mi355_bls_aggregate_verify_p2(mi355_bls_ctx* c, const void* pks, const uint8_t* msgs, const uint32_t* msg_offsets, size_t n, const void* sig_p2) {
    return aggregate_verify_impl(c, pks, msgs, msg_offsets, n, sig_p2, true);
}

// ContextCoreAggregateVerify (blst_min_pubkey_sig_core.nim:305-414), the streaming form: init / update(publicKey, message) /
// finish(signature).  The pairs are collected on the host (176 bytes + the message each) and verified by ONE device call at
// finish - the reference's update also only queues work that commit / finalVerify later complete (blst's N_MAX = 8 pair buffer).
// update returns 0 for the infinity public key (BLST_PK_IS_INFINITY: the reference's update returns false) and the context
// stays failed until the next init.
extern "C" int mi355_bls_aggv_init(mi355_bls_ctx* c) {
    if (!c) return MI355_BLS_ERR_ARG;
    c->av_pks.clear();
    c->av_msgs.clear();
    c->av_offs.assign(1, 0u);
    c->av_failed = false;
    return 0;
}
extern "C" int mi355_bls_aggv_update(mi355_bls_ctx* c, const void* pk, const uint8_t* msg, size_t msg_len) {
    if (!c || !pk || (!msg && msg_len) || c->av_offs.empty() || msg_len > (1u << 30)) return MI355_BLS_ERR_ARG;
    const uint8_t* p = (const uint8_t*)pk;
    bool inf = true;
    for (int i = 0; i < 96; i++) inf = inf && p[i] == 0;
    if (inf) {
        c->av_failed = true;
        return 0;
    }
    if (c->av_msgs.size() + msg_len > 0xffffffffull) {   // message offsets are 32-bit: refuse instead of wrapping (the context stays usable)
        g_err = "mi355_bls_aggv_update: more than 4 GiB of messages in one aggregateVerify";
        return MI355_BLS_ERR_CAPACITY;
    }
    c->av_pks.insert(c->av_pks.end(), p, p + 96);
    if (msg_len) c->av_msgs.insert(c->av_msgs.end(), msg, msg + msg_len);
    c->av_offs.push_back((uint32_t)c->av_msgs.size());
    return 1;
}
static int aggv_finish_impl(mi355_bls_ctx* c, const void* sig, bool sig_is_p2) {
    if (!c || !sig || c->av_offs.empty()) return MI355_BLS_ERR_ARG;
    size_t n = c->av_offs.size() - 1;
    int rc = 0;
    // no pair seen: blst's finalverify has no GT accumulator set -> false; a failed update -> false
    if (!c->av_failed && n) {
        uint8_t dummy = 0;
        rc = aggregate_verify_impl(c, c->av_pks.data(), c->av_msgs.empty() ? &dummy : c->av_msgs.data(), c->av_offs.data(), n, sig, sig_is_p2);
    }
    c->av_offs.clear();                                  // finish consumes the context: init again before the next use
    c->av_pks.clear();
    c->av_msgs.clear();
    return rc;
}
extern "C" int mi355_bls_aggv_finish(mi355_bls_ctx* c, const void* sig) { return aggv_finish_impl(c, sig, false); }
// finish(signature: AggregateSignature) (blst_min_pubkey_sig_core.nim:357): the Jacobian blst_p2 image, 288 B
extern "C" int mi355_bls_aggv_finish_p2(mi355_bls_ctx* c, const void* sig_p2) { return aggv_finish_impl(c, sig_p2, true); }

// ------------------------------------------------------------------------------------------
// Point-sharded MSM across devices (SURVEY.md section 8(e), "MSM"): every device computes the full-width partial sum of its
// share of the points (blst_p1 / blst_p2, Jacobian), the partials are added (blst_p1_add_or_double, blst_abi.nim:278) - 144 or
// 288 bytes per device is all that is exchanged.
// ------------------------------------------------------------------------------------------
template <class F>
static int jac_sum_device(mi355_bls_ctx* c, uint8_t* ret, const void* d_parts, size_t k, size_t stride_bytes, hipStream_t st) {
    constexpr size_t JACB = (sizeof(F) == sizeof(fp) ? 96 : 192) / 2 * 3;
    if (!c || !ret || !d_parts || k == 0 || k > 4096 || stride_bytes < JACB || (stride_bytes & 3)) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    k_jac_sum_blst<F><<<1, WAVE, 0, st>>>((const uint32_t*)d_parts, (uint32_t)k, (uint32_t)(stride_bytes / 4), c->d_agg);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ret, c->d_agg, JACB, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    c->agg_valid = false;                                // d_agg doubles as the batch path's aggregate-signature buffer
    return 0;
}
template <class F>
static int jac_sum_host(mi355_bls_ctx* c, uint8_t* ret, const uint8_t* parts, size_t k) {
    constexpr size_t JACB = (sizeof(F) == sizeof(fp) ? 96 : 192) / 2 * 3;
    if (!c || !ret || !parts || k == 0 || k * JACB > plan::SUM_PARTS_BYTES) return MI355_BLS_ERR_ARG;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->d_export, parts, k * JACB, hipMemcpyHostToDevice, nullptr));
    return jac_sum_device<F>(c, ret, c->d_export, k, JACB, nullptr);
}
extern "C" int mi355_bls_p1s_add(mi355_bls_ctx* c, uint8_t ret_p1[144], const uint8_t* parts, size_t k) { return jac_sum_host<fp>(c, ret_p1, parts, k); }
extern "C" int mi355_bls_p2s_add(mi355_bls_ctx* c, uint8_t ret_p2[288], const uint8_t* parts, size_t k) { return jac_sum_host<fp2>(c, ret_p2, parts, k); }
extern "C" int mi355_bls_p1s_add_device(mi355_bls_ctx* c, uint8_t ret_p1[144], const void* d_parts, size_t k, size_t stride_bytes, void* stream) {
    return jac_sum_device<fp>(c, ret_p1, d_parts, k, stride_bytes, (hipStream_t)stream);
}
// this device's partial of a point-sharded MSM, left in DEVICE memory (d_out_p1, 144 B) behind everything else on `stream`: the
// send buffer of the collective that gathers the partials; nothing is waited for
extern "C" int mi355_bls_p1s_mult_pippenger_partial_device(mi355_bls_ctx* c, void* d_out_p1, const void* d_points, size_t npoints, const void* d_scalars,
                                                           size_t nbits, void* stream) {
    if (!c || !d_out_p1 || nbits == 0 || nbits > 256 || npoints > (1u << 28)) return MI355_BLS_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(hipSetDevice(c->device));
    if (npoints == 0) {
        HIPCHK(hipMemsetAsync(d_out_p1, 0, 144, st));
        return 0;
    }
    if (!d_points || !d_scalars) return MI355_BLS_ERR_ARG;
    int rc = msm_enqueue<fp>(c, &c->msm, d_points, npoints, d_scalars, 32, nbits, st, false, true);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(d_out_p1, c->msm.out, 144, hipMemcpyDeviceToDevice, st));
    return 0;
}

// One host thread, ngpu contexts (one per device): device g takes points [off_g, off_g + cnt_g) (balanced contiguous blocks), all
// partial MSMs are enqueued before any is waited for, the partials return through pinned host memory and ctxs[0] adds them.
// Host arrays (pts / sc) or per-device resident arrays (d_pts[g] / d_sc[g] hold shard g).
template <class F>
static int msm_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, uint8_t* ret, const uint8_t* pts, const uint8_t* sc, const void* const d_pts[],
                     const void* const d_sc[], size_t npoints, size_t nbits) {
    constexpr size_t AFFB = sizeof(F) == sizeof(fp) ? 96 : 192, JACB = AFFB / 2 * 3;
    if (!ctxs || ngpu == 0 || ngpu > 64 || !ret || nbits == 0 || nbits > 256 || npoints > (1u << 28)) return MI355_BLS_ERR_ARG;
    if (npoints == 0) {
        std::memset(ret, 0, JACB);
        return 0;
    }
    for (size_t g = 0; g < ngpu; g++)
        if (!ctxs[g]) return MI355_BLS_ERR_ARG;
    if (!(pts && sc) && !(d_pts && d_sc)) return MI355_BLS_ERR_ARG;
    size_t base = npoints / ngpu, rem = npoints % ngpu;
    bool reg_p = false, reg_s = false;
    if (pts) {                                           // page-lock the caller's arrays: every device's copy is then a real asynchronous DMA
        reg_p = hipHostRegister(const_cast<uint8_t*>(pts), npoints * AFFB, hipHostRegisterPortable) == hipSuccess;
        reg_s = hipHostRegister(const_cast<uint8_t*>(sc), npoints * 32, hipHostRegisterPortable) == hipSuccess;
        (void)hipGetLastError();
    }
    bool live[64] = {};
    int rc = 0;
    for (size_t g = 0; g < ngpu && !rc; g++) {
        size_t off = g < rem ? (base + 1) * g : base * g + rem, cnt = base + (g < rem ? 1 : 0);
        if (cnt == 0) continue;
        mi355_bls_ctx* c = ctxs[g];
        if (hipSetDevice(c->device) != hipSuccess) { g_err = "hipSetDevice"; rc = MI355_BLS_ERR_HIP; break; }
        const void *dp = d_pts ? d_pts[g] : nullptr, *ds = d_sc ? d_sc[g] : nullptr;
        if (!dp || !ds) {
            if (!pts || !sc) { rc = MI355_BLS_ERR_ARG; break; }
            rc = msm_reserve(&c->msm, cnt, plan::pip_for(cnt, nbits), AFFB);
            if (rc) break;
            if (hipMemcpyAsync(c->msm.d_pts, pts + off * AFFB, cnt * AFFB, hipMemcpyHostToDevice, nullptr) != hipSuccess ||
                hipMemcpyAsync(c->msm.d_sc, sc + off * 32, cnt * 32, hipMemcpyHostToDevice, nullptr) != hipSuccess) {
                g_err = "hipMemcpyAsync (MSM shard staging)";
                rc = MI355_BLS_ERR_HIP;
                break;
            }
            dp = c->msm.d_pts;
            ds = c->msm.d_sc;
        }
        rc = msm_enqueue<F>(c, &c->msm, dp, cnt, ds, 32, nbits, nullptr, false, true);
        if (rc) break;
        if (hipMemcpyAsync(c->h_flags + 160, c->msm.out, JACB, hipMemcpyDeviceToHost, nullptr) != hipSuccess) { g_err = "hipMemcpyAsync (MSM partial)"; rc = MI355_BLS_ERR_HIP; break; }
        live[g] = true;
    }
    std::vector<uint8_t> parts;
    for (size_t g = 0; g < ngpu; g++) {                  // every device that was handed work is waited for, also after a failure
        if (!live[g]) continue;
        (void)hipSetDevice(ctxs[g]->device);
        if (hipStreamSynchronize(nullptr) != hipSuccess && !rc) { g_err = "hipStreamSynchronize (MSM shard)"; rc = MI355_BLS_ERR_HIP; }
        const uint8_t* h = reinterpret_cast<const uint8_t*>(ctxs[g]->h_flags + 160);
        parts.insert(parts.end(), h, h + JACB);
    }
    if (reg_p) (void)hipHostUnregister(const_cast<uint8_t*>(pts));
    if (reg_s) (void)hipHostUnregister(const_cast<uint8_t*>(sc));
    if (rc) return rc;
    return jac_sum_host<F>(ctxs[0], ret, parts.data(), parts.size() / JACB);
}
extern "C" int mi355_bls_p1s_mult_pippenger_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, uint8_t ret_p1[144], const void* const points[], size_t npoints,
                                                  const uint8_t* const scalars[], size_t nbits) {
    if (npoints && (!points || !points[0] || !scalars || !scalars[0])) return MI355_BLS_ERR_ARG;
    return msm_multi<fp>(ctxs, ngpu, ret_p1, npoints ? (const uint8_t*)points[0] : nullptr, npoints ? scalars[0] : nullptr, nullptr, nullptr, npoints, nbits);
}
extern "C" int mi355_bls_p2s_mult_pippenger_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, uint8_t ret_p2[288], const void* const points[], size_t npoints,
                                                  const uint8_t* const scalars[], size_t nbits) {
    if (npoints && (!points || !points[0] || !scalars || !scalars[0])) return MI355_BLS_ERR_ARG;
    return msm_multi<fp2>(ctxs, ngpu, ret_p2, npoints ? (const uint8_t*)points[0] : nullptr, npoints ? scalars[0] : nullptr, nullptr, nullptr, npoints, nbits);
}
extern "C" int mi355_bls_p1s_mult_pippenger_multi_device(mi355_bls_ctx* const ctxs[], size_t ngpu, uint8_t ret_p1[144], const void* const d_points[], size_t npoints,
                                                         const void* const d_scalars[], size_t nbits) {
    if (npoints && (!d_points || !d_scalars)) return MI355_BLS_ERR_ARG;
    return msm_multi<fp>(ctxs, ngpu, ret_p1, nullptr, nullptr, d_points, d_scalars, npoints, nbits);
}
/* how mi355_bls_p1s_mult_pippenger_multi cuts npoints into ngpu contiguous shards */
extern "C" void mi355_bls_msm_shard_range(size_t npoints, uint32_t world, uint32_t rank, size_t* first, size_t* count) {
    size_t base = world ? npoints / world : 0, rem = world ? npoints % world : 0;
    *first = rank < rem ? (base + 1) * rank : base * rank + rem;
    *count = base + (rank < rem ? 1 : 0);
}
