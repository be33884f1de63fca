/* C ABI of the MI355X-native BLS12-381 batch-verification path.
 *
 * Drop-in boundary: these entry points are what nim-blscurve's batch layer would bind (importc)
 * instead of driving BLST tuple by tuple.  Every function cites the reference interface it
 * replaces (paths relative to the nim-blscurve tree).  Plain pointers and sizes only.
 *
 * Data layouts are the reference's in-memory ones (BLST structs, Montgomery limbs R = 2^384,
 * little-endian u64 x 6 per Fp; blscurve/blst/blst_abi.nim:87-122):
 *   blst_p1_affine  96 B (x, y)          blst_p1  144 B (x, y, z)   Jacobian
 *   blst_p2_affine 192 B (x.c0,x.c1,y.c0,y.c1)   blst_p2 288 B      Jacobian
 *   blst_fp12      576 B
 *   SignatureSet   320 B = pubkey @0 (96) | message @96 (32) | signature @128 (192)
 *                  (blscurve/bls_batch_verifier.nim:34; affine infinity = all-zero bytes)
 *
 * Return convention: 1 = verified (Nim `true`), 0 = not verified (Nim `false`), negative = runtime
 * failure (no GPU, HIP error, capacity); the reference API only has bool, the Nim shim maps <0 to
 * a Defect.  The library never falls back to a CPU path.
 */
#ifndef BLSCURVE_MI355X_H
#define BLSCURVE_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI355_BLS_SIGSET_BYTES 320
#define MI355_BLS_FP12_BYTES 576
#define MI355_BLS_P1_BYTES 144
#define MI355_BLS_P2_BYTES 288
#define MI355_BLS_BLOB_BYTES 640     /* device-resident shard blob: 576-byte state | u32 ok word | zero padding */

#define MI355_BLS_ERR_HIP (-1)       /* a HIP call failed; see mi355_bls_last_error() */
#define MI355_BLS_ERR_CAPACITY (-2)  /* n exceeds the context's capacity (never returned by the batchVerify / aggregateVerify entry points:
                                        they process larger inputs in slices) */
#define MI355_BLS_ERR_ARG (-3)

typedef struct mi355_bls_ctx mi355_bls_ctx;

/* BatchedBLSVerifierCache.init / init(tp) (bls_batch_verifier.nim:108-119): persistent device
 * workspace on HIP device `device`.  One context per concurrent caller, reusable across calls
 * (bls_batch_verifier.nim:389-391).  max_sets sizes the workspace (about 32 KB of HBM per set), it does NOT bound
 * input.len: like the reference's cache (per-thread contexts only, :108-119,:141) every batchVerify entry point accepts
 * any n - a batch (or shard) larger than max_sets is processed in ceil(n / max_sets) balanced slices on the same stream,
 * whose committed states are merged on the device (blst_pairing_merge semantics).  Size it for the batches you expect:
 * a slice that fills the chip (>= 65 536 sets) runs at full throughput. */
int mi355_bls_ctx_create(mi355_bls_ctx** out, int device, size_t max_sets);
void mi355_bls_ctx_destroy(mi355_bls_ctx* ctx);
const char* mi355_bls_last_error(void);
/* How the loaded library was built: "aligned=1 dpp_combine=off stamp=<sha256 of its sources>".  aligned=0 = built without the
 * instruction-alignment post-pass (BLS_NO_ALIGN=1; ~23 % lower issue rate of the multiply-add streams): a measurement taken with
 * such a library says so (bench.py prints the string and refuses aligned=0 unless asked).  Static string, never NULL. */
const char* mi355_bls_build_info(void);

/* HIP hardware queues.  HIP spreads a process's streams over GPU_MAX_HW_QUEUES hardware queues (default 4); streams that share a
 * queue run strictly in turn.  Whole-chip batches do not care; a host that keeps MANY SMALL batches in flight (one context + stream
 * each; 4 096-tuple batches: 1.4 M verifications/s with 4 queues, 2.3 M/s with 8; more than 8 abort in the runtime) should run with
 * GPU_MAX_HW_QUEUES=8.  The variable is read when the HIP runtime initialises, so it is the HOST's to set - in its environment, or by
 * calling this helper ONCE from its main thread before anything in the process touches HIP (setenv is not thread-safe, and the
 * setting changes queue behaviour for every HIP user of the process: torch, RCCL).  The library never edits the environment on its
 * own.  Returns 1 if GPU_MAX_HW_QUEUES is now set (an existing value is kept), 0 if MI355_BLS_NO_ENV=1 forbids it or setenv failed. */
int mi355_bls_recommend_hw_queues(void);

/* Taskpool.numThreads analogue (bls_batch_verifier.nim:316): the number of blinding-scalar hash
 * chains ("virtual threads") B = min(n, num_threads) the parallel path splits a batch into; chunk c
 * is seeded SHA256(rnd || LE64(c)) exactly as processSingleChunk does (:333-336).  Default 4096. */
int mi355_bls_ctx_set_num_threads(mi355_bls_ctx* ctx, uint32_t num_threads);

/* Latency mode (on = 1, the default) or throughput mode (on = 0) of a context.
 * Latency mode shortens ONE call at the price of some extra lane-work: batches of up to ~11 000 sets (which do not fill the chip
 * with one lane per set) run their cofactor clearing and Miller lines on the lane-team engine, 16 lanes per set (4 096 sets:
 * 15 ms in round 1, 5.35 in round 5, 3.9 ms now), with [r]PK and the signature side on two fork streams beside the hashing;
 * whole-chip batches run the signature side and the Miller lines of its extra pairs on a second stream beside the hashing, so
 * that no nearly empty round of waves follows a full one; the partial line products are folded on the lane-cooperative Fp12
 * engine, whose workgroups have three waves in this mode.
 * Throughput mode does the least total work: for a caller that keeps several batches in flight (one context each), where
 * the nearly empty rounds of one batch overlap the wide kernels of another.  Verdicts and GT values are the same. */
int mi355_bls_ctx_set_cooperative(mi355_bls_ctx* ctx, int on);

/* batchVerifyParallel / batchVerify raw-pointer overloads (bls_batch_verifier.nim:296-302,420-426):
 * sets = n x 320-byte SignatureSet records in HOST memory, rnd = secureRandomBytes. n == 0 -> 0.
 * WHEN TO CALL IT: one blocking call costs about 2.3 ms for any n up to ~200 and 3.0 ms up to ~1 000 (latency-bound chains: hash-to-G2,
 * Miller walk, final exponentiation), 3.5 ms at 4 096, 12.4 ms at 65 536 (11 ms per batch when three are kept in flight).  A CPU BLST verifies a small
 * batch faster than that: below about 5 sets per host core (~80 sets on 16 cores; bench.py's `crossover`, INTEGRATION.md "When to call the
 * GPU") a host should keep its CPU path, as the Nim shim of INTEGRATION.md does (Mi355MinSets).  Many small batches at once:
 * mi355_bls_batch_verify_many. */
int mi355_bls_batch_verify(mi355_bls_ctx* ctx, const void* sets, size_t n, const uint8_t rnd[32]);

/* batchVerifySerial (bls_batch_verifier.nim:121-160): same check with the serial scalar chain
 * (seed = SHA256(rnd), one chain over the whole batch).  The chain is inherently sequential: it is computed on the calling
 * host thread (about 0.3 us per tuple) and uploaded; everything else runs on the device as in the parallel path. */
int mi355_bls_batch_verify_serial(mi355_bls_ctx* ctx, const void* sets, size_t n, const uint8_t rnd[32]);

/* Same as mi355_bls_batch_verify with the records already resident in device memory (HBM) and
 * work enqueued on `stream` (hipStream_t, may be NULL); synchronises the stream before returning. */
int mi355_bls_batch_verify_device(mi355_bls_ctx* ctx, const void* d_sets, size_t n, const uint8_t rnd[32], void* stream);

/* Asynchronous form of mi355_bls_batch_verify_device, for a caller that keeps several batches in flight from ONE host
 * thread (one context + one stream per batch in flight, cf. "one cache per concurrent caller",
 * bls_batch_verifier.nim:389-391): submit enqueues the whole verification on `stream` and returns at once (0, or a
 * negative error; n == 0 is an error here); wait blocks until that batch is done and returns its verdict (1 / 0) exactly
 * as mi355_bls_batch_verify_device would.  One batch per context at a time; d_sets must stay valid until wait returns;
 * rnd is consumed at submit.  `after` (optional): another context whose batch was submitted earlier; this batch then
 * starts when that batch has finished hashing and multiplying its public keys, so the batches in flight sit at different
 * stages and the serial tail of one (a few waves: step products, Horner, final exponentiation) always runs beside
 * whole-chip kernels of another - deterministic software pipelining; three contexts are enough. */
int mi355_bls_batch_submit_device(mi355_bls_ctx* ctx, const void* d_sets, size_t n, const uint8_t rnd[32], void* stream,
                                  mi355_bls_ctx* after);
int mi355_bls_batch_wait(mi355_bls_ctx* ctx);

/* Many independent batches in ONE device pass (no reference counterpart: the reference verifies one batch per call and gets its
 * concurrency from caller threads; on the device, small batches cannot fill the chip and the number of HIP hardware queues caps
 * how many calls run side by side).  sets: the tuples of batch 0, then batch 1, ... (counts[b] of them each, 320-byte records),
 * rnds: k x 32 bytes, one secureRandomBytes per batch; verdicts[b] receives what mi355_bls_batch_verify_once(batch b, rnd b,
 * num_threads) would return (an empty batch: 0).  Every tuple keeps the blinding scalar it has in its own batch (own chain
 * partition B = min(n_b, num_threads), serial chain for n_b < 3 or num_threads = 1, bls_batch_verifier.nim:440); the union is
 * verified at once, and the product of the k batch checks is one iff every batch verifies (up to the 2^-64 of the random linear
 * combination, the reference's own bound).  If it is not, or if the union exceeds the context's capacity, the batches are
 * verified one by one.  Returns 1 when every batch verified, 0 otherwise, negative on runtime failure.
 * REQUIREMENT for the merged pass: the k secureRandomBytes must be pairwise independent.  The library checks what it can: if any two
 * non-empty batches carry the SAME 32 bytes (their blinding chains would coincide and errors could cancel ACROSS batches, which k
 * separate calls would not allow), no merged pass is made and the batches are verified one by one - the verdicts stay those of k
 * separate calls, only the speed-up is lost.  Draw one fresh rnd per batch.
 * COST: a passing call is one whole-chip pass.  A call in which some batch fails costs that pass PLUS k single-batch calls (about
 * twice the latency; the calls are synchronous): an adversary who can place one bad signature per call forces the slow path for all
 * k batches - hosts that expect failures should keep k small or verify suspicious batches separately.  mi355_bls_batch_verify_many_locate
 * (below) answers a failing call with ONE per-batch pass instead of the k calls.
*/
int mi355_bls_batch_verify_many(mi355_bls_ctx* ctx, const void* sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[]);
int mi355_bls_batch_verify_many_device(mi355_bls_ctx* ctx, const void* d_sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                                       void* stream);

/* Per-batch verdicts for many batches in ONE device pass: what the failing case of mi355_bls_batch_verify_many finds with k single-batch
 * calls.  Arguments and layout are those of mi355_bls_batch_verify_many (records laid end to end; counts, rnds and the k verdict bytes in host
 * memory).
 *   many_each:   verdicts[b] = what mi355_bls_batch_verify_once(batch b, rnds[b], num_threads) returns, computed as batch b's OWN product:
 *                prod_i e([r_i]PK_i, H(m_i)) * e(-G1, sum_i [r_i]S_i) over the sets of batch b, r_i the scalar set i has in its own batch
 *                (chain partition B = min(n_b, num_threads), serial chain for n_b < 3 or num_threads = 1).  An empty batch gives 0 and
 *                takes no lane; a batch that holds an infinity public key gives 0 and the other batches are not affected; an infinity
 *                signature adds nothing to its batch's sum.  Nothing is sticky across batches, and since NO PRODUCT IS SHARED between
 *                batches, two batches with the same 32 random bytes need no special case: errors cannot cancel across batches here.
 *                Returns 1 iff every verdict is 1 (k == 0 or every batch empty: 0, every verdict 0), negative on a runtime failure,
 *                MI355_BLS_ERR_ARG under the rules of mi355_bls_batch_verify_many (a context with a submitted batch pending among them).
 *   many_locate: the merged pass of mi355_bls_batch_verify_many first, under its conditions (distinct rnds, union within the capacity,
 *                k <= 65 536).  If it passes: every non-empty batch 1 and no per-batch pass.  If it fails or cannot run: one many_each pass.
 * No input is refused for its size: the call runs in slices of whole consecutive batches, as many as fit max_sets sets and, sets plus one
 * signature slot per batch, the per-set path's pair store; a batch that alone does not fit takes the single-batch path, which slices
 * internally.  The blinding scalars and the random bytes are cleared from device memory before the call returns.  Synchronous.
 * COST on one MI355X against mi355_bls_batch_verify_many_device on the same input in the same run (profiles/verify_many_each_bench.json,
 * nim-blscurve_amd/tools/bench_verify_many_each.py: 65 536 device-resident sets on a 65 536-set context, median of 5 blocking calls, every
 * min .. max within 4 % of its median), at 16 x 4 096 / 64 x 1 024 / 256 x 256 / 1 024 x 64 batches x sets:
 *   failing case (one forged batch): many_each 21.6 / 19.9 / 19.1 / 21.8 ms and many_locate 33.8 / 32.0 / 31.0 / 33.8 ms against the k-call
 *   fallback's 66.7 / 199 / 615 / 2 250 ms: 3.1 / 10 / 32 / 103 times and 2.0 / 6.2 / 20 / 67 times faster - the new calls lose at none
 *   of the four shapes;
 *   passing case (all valid): many_each 21.3 / 19.8 / 19.0 / 21.9 ms against the merged pass's 11.9 / 12.2 / 12.2 / 12.3 ms - asking "which
 *   one?" up front costs 1.79 / 1.63 / 1.56 / 1.78 times the merged pass, its time does not depend on the input - and many_locate IS the
 *   merged pass there (0.98 - 1.00 of it).
 * So: many_locate where failures are rare, many_each where a bad batch per call is to be expected (it beats many_locate's failing case by
 * the merged pass).  Nothing inside the library switches on these numbers. */
int mi355_bls_batch_verify_many_each(mi355_bls_ctx* ctx, const void* sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[]);
int mi355_bls_batch_verify_many_each_device(mi355_bls_ctx* ctx, const void* d_sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                                            void* stream);
int mi355_bls_batch_verify_many_locate(mi355_bls_ctx* ctx, const void* sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[]);
int mi355_bls_batch_verify_many_locate_device(mi355_bls_ctx* ctx, const void* d_sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                                              void* stream);
/* TEST HOOKS: the host form of many_each with, for every batch, the 576-byte blst_fp12 image of the value after the final exponentiation
 * (gt_out: k x 576 bytes; an empty batch: zero bytes) - the per-batch counterpart of mi355_bls_fetch_stage(4); the number of per-batch passes
 * this context has made. */
int mi355_bls_debug_batch_verify_many_each_gt(mi355_bls_ctx* ctx, const void* sets, const size_t counts[], const uint8_t* rnds, size_t k, uint8_t verdicts[],
                                              uint8_t* gt_out);
int mi355_bls_debug_batch_verify_many_each_passes(mi355_bls_ctx* ctx);

/* Per-set verdicts in one device pass: verdicts[i] = verify(pk_i, msg_i, sig_i) (bls_sig_min_pubkey.nim:108-125 ->
 * coreVerifyNoGroupCheck, blst_min_pubkey_sig_core.nim:269-297) for every 320-byte SignatureSet record of the input - what a host does
 * set by set after a batch has failed, to find the culprits.  No blinding and no random bytes: verdict i depends on set i alone, not on
 * n, on its position, on the other sets or on num_threads; nothing is sticky.  Infinity rules as BLST's: an infinity public key gives 0;
 * an infinity signature contributes no pair (0 for a valid key).  Preconditions as the reference's: points decoded and group-checked.
 * Any n (larger inputs run in slices).  Returns 1 when every set verified, 0 otherwise (n == 0: 0, nothing written), negative on a
 * runtime failure.  verdicts: n bytes, host memory.  Synchronous. */
int mi355_bls_verify_each(mi355_bls_ctx* ctx, const void* sets, size_t n, uint8_t verdicts[]);
int mi355_bls_verify_each_device(mi355_bls_ctx* ctx, const void* d_sets, size_t n, uint8_t verdicts[], void* stream);
/* batchVerify first (mi355_bls_batch_verify with rnd); if it passes: 1 and every verdict 1, no per-set pass.  If it fails: one
 * mi355_bls_verify_each pass, returns 0 with the per-set verdicts.
 * COST: a passing call is the batch pass alone.  A failing call costs the batch pass PLUS the per-set pass, whose time does not depend on
 * how many sets are bad: at 65 536 sets 12.7 ms + 72.3 ms (profiles/verify_each_bench.json; one device call per set: 141 s). */
int mi355_bls_batch_verify_locate(mi355_bls_ctx* ctx, const void* sets, size_t n, const uint8_t rnd[32], uint8_t verdicts[]);
int mi355_bls_batch_verify_locate_device(mi355_bls_ctx* ctx, const void* d_sets, size_t n, const uint8_t rnd[32], uint8_t verdicts[], void* stream);

/* Proofs of possession for a table of keys in one device pass: popVerify (bls_sig_min_pubkey.nim:60-74) is
 * coreVerifyNoGroupCheck(publicKey, rawFromPublic(publicKey), proof, DST_POP) - the check every aggregate entry point of this header
 * leaves to the caller, and the one the reference's proof-taking overloads of verify / aggregateVerify / fastAggregateVerify
 * (:104, :148, :220-225) loop over key by key.  pks96: n x 96-byte blst_p1_affine images; proofs192: n x 192-byte blst_p2_affine images
 * (a ProofOfPossession is a Signature: 96 bytes on the wire, decoded by mi355_bls_deserialize_sets like any signature; the message column
 * of that call is not used here).  The message of pair i is the 48-byte compressed form of key i, computed on the device.
 *   pop_verify_each:  verdicts[i] = popVerify(pk_i, proof_i) exactly.  No blinding, no random bytes: verdict i depends on pair i alone.
 *                     Infinity rules as mi355_bls_verify_each: an infinity key gives 0, an infinity proof gives 0 for a valid key.
 *                     Preconditions as the reference's: points decoded and group-checked.  Any n (larger inputs run in slices).
 *                     Returns 1 iff every verdict is 1 (n == 0: 0, nothing written), negative on a runtime failure.  Synchronous.
 *   batch_pop_verify: NO reference counterpart (like mi355_bls_batch_verify_many): the blinded check of mi355_bls_batch_verify over the sets
 *                     (pk_i, compress(pk_i), proof_i) under DST_POP, with the scalars drawn exactly as mi355_bls_batch_verify draws them for
 *                     n sets and rnd (num_threads chains); mi355_bls_fetch_stage shows its stages as for any batch call.  1 / 0 / negative.
 *   batch_pop_verify_locate:  the batch check first; if it passes: 1 and every verdict 1, no per-pair pass; if it fails: one
 *                     pop_verify_each pass, returns 0 with the verdicts.
 * The _device forms take the two arrays in device memory and a stream; verdicts stay host memory.
 * COST at 65 536 keys on one MI355X (profiles/pop_verify_bench.json; ordinary signature sets over the same keys in the same run beside them):
 * not measured yet: run nim-blscurve_amd/tools/bench_pop.py on an MI355X, which writes the four timings and the two ratios. */
int mi355_bls_pop_verify_each(mi355_bls_ctx* ctx, const void* pks96, const void* proofs192, size_t n, uint8_t verdicts[]);
int mi355_bls_pop_verify_each_device(mi355_bls_ctx* ctx, const void* d_pks96, const void* d_proofs192, size_t n, uint8_t verdicts[], void* stream);
int mi355_bls_batch_pop_verify(mi355_bls_ctx* ctx, const void* pks96, const void* proofs192, size_t n, const uint8_t rnd[32]);
int mi355_bls_batch_pop_verify_device(mi355_bls_ctx* ctx, const void* d_pks96, const void* d_proofs192, size_t n, const uint8_t rnd[32], void* stream);
int mi355_bls_batch_pop_verify_locate(mi355_bls_ctx* ctx, const void* pks96, const void* proofs192, size_t n, const uint8_t rnd[32], uint8_t verdicts[]);
int mi355_bls_batch_pop_verify_locate_device(mi355_bls_ctx* ctx, const void* d_pks96, const void* d_proofs192, size_t n, const uint8_t rnd[32],
                                             uint8_t verdicts[], void* stream);
/* rawFromPublic (blst_min_pubkey_sig_core.nim:135-137) / serialize(PublicKey) (bls_sig_io.nim:203-211), i.e. blst_p1_affine_compress, for n
 * keys: 96-byte blst_p1_affine images in, 48 bytes each out (ZCash form: big-endian x, bit 7 of byte 0 set, bit 5 set when y is the
 * lexicographically larger root; the all-zero infinity image gives 0xc0 and 47 zero bytes).  The device form writes device memory
 * (d_out48: n x 48 B) and returns when the bytes are there.  Returns 0, negative on failure. */
int mi355_bls_compress_public_keys(mi355_bls_ctx* ctx, const void* pks96, size_t n, uint8_t out48[]);
int mi355_bls_compress_public_keys_device(mi355_bls_ctx* ctx, const void* d_pks96, size_t n, void* d_out48, void* stream);

/* Multi-GPU sharding (replaces processSingleChunk + merge, bls_batch_verifier.nim:326-369).
 * The global batch of n_total sets is cut into B = min(n_total, num_threads) chunks by
 * parallel_chunks (parallel_chunks.nim:42-66); this call processes chunks [chunk_lo, chunk_hi),
 * whose records start at d_sets (device memory), and returns the shard's committed pairing state:
 *   out_fp12 = prod_{i in shard} ML(H(m_i), [r_i]PK_i) * ML(sum [r_i]S_i, -G1)   (576 B, pre final-exp)
 *   *out_ok  = 0 if an update failed (infinity public key), else 1.
 * The signature-side pair is folded per shard, so merging shards is an Fp12 product only
 * (blst_pairing_merge, blst_abi.nim:508). */
int mi355_bls_batch_shard_device(mi355_bls_ctx* ctx, const void* d_sets, size_t n_total, uint32_t chunk_lo, uint32_t chunk_hi,
                                 const uint8_t rnd[32], void* stream, uint8_t out_fp12[576], int* out_ok);
/* asynchronous form (see mi355_bls_batch_submit_device / mi355_bls_batch_wait) */
int mi355_bls_batch_shard_submit_device(mi355_bls_ctx* ctx, const void* d_sets, size_t n_total, uint32_t chunk_lo, uint32_t chunk_hi,
                                        const uint8_t rnd[32], void* stream, mi355_bls_ctx* after);
int mi355_bls_batch_shard_wait(mi355_bls_ctx* ctx, uint8_t out_fp12[576], int* out_ok);

/* merge + finalVerify (blst_min_pubkey_sig_core.nim:657-672): product of k shard states (host
 * memory, k x 576 B), one final exponentiation on the device, == 1. */
int mi355_bls_finalverify_shards(mi355_bls_ctx* ctx, const uint8_t* fp12s, size_t k);

/* Device-resident exchange for one-process-per-GPU callers (the multi-GPU bench): every shard submit also writes the shard's
 * state + ok word into the context's blob buffer (MI355_BLS_BLOB_BYTES, device memory) on the submit's stream.  The caller
 * gathers the blobs of all ranks with a collective on device buffers (RCCL all_gather) and hands the gathered buffer to
 * finalverify_blobs: merge (blst_pairing_merge, core :657-666) + finalVerify (:670-672) on k blobs `stride_bytes` apart in
 * DEVICE memory, enqueued on `stream`; finalverify_wait blocks and returns the verdict (1 only if every shard's ok word is 1
 * and the product is one).  Nothing but the verdict word crosses PCIe.  (The collective may be enqueued right behind the
 * submit on the same stream; the bench waits for the shard first - mi355_bls_batch_shard_wait, a host synchronisation - because
 * torch issues collectives on a stream of its own, where one that waits for a whole batch blocks a hardware queue.)
 * finalverify_blobs keeps its verdict word and GT value apart from the batch path's, so a context may take its next shard
 * while a merge submitted on it is still in flight on another stream. */
int mi355_bls_ctx_shard_blob_device(mi355_bls_ctx* ctx, void** d_blob);
/* Redirect the blob to the caller's own device buffer (MI355_BLS_BLOB_BYTES, 16-byte aligned; e.g. the send buffer of the
 * collective, so no copy is needed); NULL restores the context's internal buffer. */
int mi355_bls_ctx_set_shard_blob_device(mi355_bls_ctx* ctx, void* d_blob);
int mi355_bls_finalverify_blobs_submit_device(mi355_bls_ctx* ctx, const void* d_blobs, size_t k, size_t stride_bytes, void* stream);
int mi355_bls_finalverify_wait(mi355_bls_ctx* ctx);

/* Which chunks device `rank` of `world` takes: contiguous balanced blocks of the B = min(n_total, num_threads) chunks,
 * and the tuple range they cover. */
int mi355_bls_shard_plan(size_t n_total, uint32_t num_threads, uint32_t world, uint32_t rank, uint32_t* chunk_lo, uint32_t* chunk_hi,
                         size_t* first, size_t* count);

/* batchVerifyParallel across several GPUs of one node from ONE host thread (bls_batch_verifier.nim:296-371 with devices in
 * place of taskpool threads): ctxs[g] is a context on device g (all with the same num_threads; a shard larger than its
 * context's capacity is sliced, the largest shard is mi355_bls_shard_plan(...).count of rank 0); shard g = the chunk block
 * mi355_bls_shard_plan gives rank g.  The plan and every context are validated before anything is enqueued; the caller's
 * host range is page-locked for the call so that all shards' copies and kernels are enqueued asynchronously (:342-357) and
 * device g does not wait for device g - 1's staging; the 576-byte states return through pinned host memory, ctxs[0] merges
 * them and runs the one final exponentiation (:360-371).  If enqueuing a shard fails, the shards already submitted are waited
 * for before the error is returned, so every context stays usable.  `sets`: n x 320 B in host memory; the _device form takes
 * d_sets[g] = shard g's records already resident on device g.  n == 0 -> 0. */
int mi355_bls_batch_verify_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, const void* sets, size_t n, const uint8_t rnd[32]);
int mi355_bls_batch_verify_multi_device(mi355_bls_ctx* const ctxs[], size_t ngpu, const void* const d_sets[], size_t n, const uint8_t rnd[32]);

/* The cache-less overloads batchVerifyParallel(tp, input, rnd) / batchVerify(tp, input, rnd) (bls_batch_verifier.nim:399-416,
 * :475-495), which build a BatchedBLSVerifierCache per call: here a process-wide default context (HIP device
 * $MI355_BLS_DEVICE, default 0) created on first use and regrown on demand; calls are serialised by a mutex.
 * num_threads = tp.numThreads; dispatch as batchVerify: parallel iff num_threads > 1 and n >= 3, else the serial chain. */
int mi355_bls_batch_verify_once(const void* sets, size_t n, const uint8_t rnd[32], uint32_t num_threads);
void mi355_bls_default_ctx_release(void);

/* Helper: tuple range [*first, *first + *count) covered by chunks [chunk_lo, chunk_hi) of a batch of
 * n_total sets split into num_threads chunks (parallel_chunks.nim:42-66). */
void mi355_bls_chunk_range(size_t n_total, uint32_t num_threads, uint32_t chunk_lo, uint32_t chunk_hi, size_t* first, size_t* count);

/* aggregateAll on G1 (blst_min_pubkey_sig_core.nim:179-195: blst_p1_from_affine + a serial loop of
 * blst_p1_add_or_double_affine): sum of n blst_p1_affine points -> blst_p1 (Jacobian, 144 B; the
 * caller finishes with blst_p1_to_affine as the reference's `finish` does).  Host or device input. */
int mi355_bls_g1_aggregate(mi355_bls_ctx* ctx, const void* pks, size_t n, uint8_t out_p1[144]);
int mi355_bls_g1_aggregate_device(mi355_bls_ctx* ctx, const void* d_pks, size_t n, void* stream, uint8_t out_p1[144]);
/* aggregateAll on signatures (genAggregatorProcedures(AggregateSignature, Signature, p2), blst_min_pubkey_sig_core.nim:179-195,211):
 * sigs: n x 192 B blst_p2_affine (infinity = all zero contributes nothing), out_p2: the sum as blst_p2 (Jacobian, 288 B) - what
 * mi355_bls_aggregate_verify_p2 / mi355_bls_aggv_finish_p2 take.  n == 0: MI355_BLS_ERR_ARG (the reference's openArray form
 * returns false before touching its output). */
int mi355_bls_g2_aggregate(mi355_bls_ctx* ctx, const void* sigs, size_t n, uint8_t out_p2[288]);
int mi355_bls_g2_aggregate_device(mi355_bls_ctx* ctx, const void* d_sigs, size_t n, void* stream, uint8_t out_p2[288]);

/* fastAggregateVerify(publicKeys, message, signature) (bls_sig_min_pubkey.nim:234-258): aggregate the
 * n public keys on the device, then coreVerifyNoGroupCheck (core :269-297): e(agg, H(msg)) == e(G1, sig).
 * pks: n x 96 B blst_p1_affine, sig: 192 B blst_p2_affine (host memory), msg_len <= 4096.
 * n == 0 -> 0; aggregate at infinity -> 0. */
int mi355_bls_fast_aggregate_verify(mi355_bls_ctx* ctx, const void* pks, size_t n, const uint8_t* msg, size_t msg_len, const void* sig);
int mi355_bls_fast_aggregate_verify_device(mi355_bls_ctx* ctx, const void* d_pks, size_t n, const uint8_t* msg, size_t msg_len,
                                           const void* sig, void* stream);
/* The same with the keys sharded over the GPUs of one node: ctxs[g] on device g sums the contiguous block of
 * keys mi355_bls_msm_shard_range(n, ngpu, g) gives it (aggregateAll, core :179-195), the 144-byte partial sums are added on ctxs[0]
 * (blst_p1_add_or_double), which runs the one pairing check.  pks: n x 96 B in host memory. */
int mi355_bls_fast_aggregate_verify_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, const void* pks, size_t n, const uint8_t* msg,
                                          size_t msg_len, const void* sig);
/* fastAggregateVerify for MANY sets: the key aggregation of every set in ONE device pass.  In the batch verifier's workload (attestations,
 * sync-committee messages) a set's public key is not on the wire: it is aggregateAll (blst_min_pubkey_sig_core.nim:179-195; the first step
 * of fastAggregateVerify, bls_sig_min_pubkey.nim:234-258) over a committee.  These calls take k key lists at once and leave k ordinary
 * 320-byte SignatureSet records (aggregate key | message | signature) in device memory, which every batch and per-set entry point takes
 * unchanged.
 *   keys      n_table x 96-byte blst_p1_affine images: the key table (e.g. the validator registry, kept resident on the device)
 *   idx       NULL: list s is keys [offsets[s], offsets[s+1]) of the table itself (offsets[k] <= n_table);
 *             else: list s is keys idx[offsets[s]] .. idx[offsets[s+1] - 1] of the table (offsets[k] = the length of idx; repeats allowed)
 *   offsets   k + 1 entries in HOST memory (also in the _device forms), non-decreasing; an empty list is allowed
 *   msgs32    k x 32 bytes, sigs192: k x 192-byte blst_p2_affine images, packed, one per list
 *   status    k bytes, host memory: 0 ok, 1 empty list, 2 the aggregate is the point at infinity, 3 an index was >= n_table (it is never
 *             dereferenced; 3 wins over 1 and 2).  The record of a list whose status is not 0 carries the infinity key (96 zero bytes), for
 *             which every verifier answers 0.
 * An affine infinity image among the keys adds nothing, as in mi355_bls_g1_aggregate (fromBytes never yields one).  Device pointers are
 * 4-byte aligned.  Preconditions as the reference's: keys decoded and group-checked, proofs of possession verified by the caller.
 * Any k and any list lengths up to 2^32 - 2 keys in all; nothing here is bounded by max_sets (the verification passes slice as always).
 * aggregate_sets:  returns 1 when every status is 0, else 0; k == 0: 0, nothing written.  MI355_BLS_ERR_ARG for decreasing offsets,
 *                  offsets[k] > n_table without idx, NULL pointers.  The _device form enqueues on `stream` and synchronises it once, for
 *                  the status bytes; d_out_records: k x 320 bytes of device memory.
 * fast_aggregate_verify_each:   out[s] = fastAggregateVerify(keys of list s, msg_s, sig_s) for every s (an empty list: 0,
 *                  bls_sig_min_pubkey.nim:251-253) - the aggregation, then the mi355_bls_verify_each pass on the records.  Returns 1 iff all are 1.
 * batch_fast_aggregate_verify:  batchVerify (mi355_bls_batch_verify with rnd) over the sets (aggregateAll(keys_s), msg_s, sig_s); if any
 *                  status is not 0 the result is 0 and no verification pass is run. */
int mi355_bls_aggregate_sets(mi355_bls_ctx* ctx, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                             const void* msgs32, const void* sigs192, void* out_records, uint8_t* status);
int mi355_bls_aggregate_sets_device(mi355_bls_ctx* ctx, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k,
                                    const void* d_msgs32, const void* d_sigs192, void* d_out_records, uint8_t* status, void* stream);
int mi355_bls_fast_aggregate_verify_each(mi355_bls_ctx* ctx, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                         const void* msgs32, const void* sigs192, uint8_t* out);
int mi355_bls_fast_aggregate_verify_each_device(mi355_bls_ctx* ctx, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                                size_t k, const void* d_msgs32, const void* d_sigs192, uint8_t* out, void* stream);
int mi355_bls_batch_fast_aggregate_verify(mi355_bls_ctx* ctx, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                          const void* msgs32, const void* sigs192, const uint8_t rnd[32]);
int mi355_bls_batch_fast_aggregate_verify_device(mi355_bls_ctx* ctx, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                                 size_t k, const void* d_msgs32, const void* d_sigs192, const uint8_t rnd[32], void* stream);
/* The same records from the form the host holds: m fixed committees (index lists into the key table, the same for an epoch) and, per set, a
 * committee number and one bit per committee position (aggregation_bits of an attestation, sync_committee_bits of a sync aggregate).  The
 * key of set s is aggregateAll (blst_min_pubkey_sig_core.nim:179-195) over the keys of committee which[s] whose bit is 1, in committee
 * order - the first step of fastAggregateVerify (bls_sig_min_pubkey.nim:234-258) - and record s is byte for byte what
 * mi355_bls_aggregate_sets writes for the expanded index list.
 *   keys, n_table, idx   the key table and the optional index array, as above
 *   c_offsets   m + 1 entries in HOST memory, non-decreasing: committee c is positions [c_offsets[c], c_offsets[c+1]) (of idx, or of the table)
 *   which       k committee numbers (< m) in HOST memory, also in the _device forms; repeats in any order (sixteen aggregators of one
 *               committee are sixteen sets)
 *   bits        the k fields packed end to end in set order; a set whose committee has L positions owns exactly ceil(L / 8) bytes, SSZ bit
 *               order: position i is bit i % 8 of byte i / 8.  Bits at positions >= L of the last byte are ignored (a bitlist's delimiter
 *               bit may stay).  Byte-aligned; every other device pointer is 4-byte aligned.
 *   committee_aggs   NULL, or the aggregate key of every committee: m 96-byte blst_p1_affine images agg_stride bytes apart (96: packed; 320:
 *               the records mi355_bls_aggregate_sets(_device) wrote for the committees themselves with the same idx and c_offsets - how
 *               a host makes them, once per epoch).  agg_stride >= 96 and a multiple of 4.  With them, a set of which more than half
 *               signed (2 * popcount > L) and whose committee's image is not all zero is computed as subtractAll
 *               (blst_min_pubkey_sig_core.nim:197-209): the committee's aggregate minus the keys whose bit is 0.  Every other set - a
 *               tie at exactly half included - is summed directly.  The route never shows in a record or a status byte.
 *               PRECONDITION, like a decoded key: an image that is not all zero IS the aggregate of its committee.
 *   status      as above: 0 ok, 1 no bit set (also a committee of length 0), 2 the sum is the point at infinity, 3 a participating position
 *               holds an index >= n_table (never dereferenced; 3 wins over 1 and 2; on both routes every index is checked before it is used)
 * Returns and k == 0 as the calls above.  MI355_BLS_ERR_ARG for decreasing c_offsets, c_offsets[m] > n_table without idx, a which[s] >= m,
 * NULL pointers, a bad agg_stride, or more than 2^32 - 2 level-0 items (one per 8 positions of a set).  Nothing is bounded by max_sets.
 * COST: one lane per 8 positions of a set, whose time is its number of selected keys; the levels above and the finish as aggregate_sets.
 *       Measured figures: profiles/aggregate_bits_bench.json, DESIGN.md 3.2.2a.
 * debug_aggregate_bits_routes: TEST HOOK - out[0] / out[1] = sets of the context's last bits call summed directly / by exclusion. */
int mi355_bls_aggregate_sets_bits(mi355_bls_ctx* ctx, const void* keys, size_t n_table, const uint32_t* idx, const size_t* c_offsets, size_t m,
                                  const void* committee_aggs, size_t agg_stride, const uint32_t* which, const void* bits, size_t k, const void* msgs32,
                                  const void* sigs192, void* out_records, uint8_t* status);
int mi355_bls_aggregate_sets_bits_device(mi355_bls_ctx* ctx, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* c_offsets, size_t m,
                                         const void* d_committee_aggs, size_t agg_stride, const uint32_t* which, const void* d_bits, size_t k,
                                         const void* d_msgs32, const void* d_sigs192, void* d_out_records, uint8_t* status, void* stream);
int mi355_bls_fast_aggregate_verify_each_bits(mi355_bls_ctx* ctx, const void* keys, size_t n_table, const uint32_t* idx, const size_t* c_offsets, size_t m,
                                              const void* committee_aggs, size_t agg_stride, const uint32_t* which, const void* bits, size_t k,
                                              const void* msgs32, const void* sigs192, uint8_t* out);
int mi355_bls_fast_aggregate_verify_each_bits_device(mi355_bls_ctx* ctx, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* c_offsets,
                                                     size_t m, const void* d_committee_aggs, size_t agg_stride, const uint32_t* which, const void* d_bits,
                                                     size_t k, const void* d_msgs32, const void* d_sigs192, uint8_t* out, void* stream);
int mi355_bls_batch_fast_aggregate_verify_bits(mi355_bls_ctx* ctx, const void* keys, size_t n_table, const uint32_t* idx, const size_t* c_offsets, size_t m,
                                               const void* committee_aggs, size_t agg_stride, const uint32_t* which, const void* bits, size_t k,
                                               const void* msgs32, const void* sigs192, const uint8_t rnd[32]);
int mi355_bls_batch_fast_aggregate_verify_bits_device(mi355_bls_ctx* ctx, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* c_offsets,
                                                      size_t m, const void* d_committee_aggs, size_t agg_stride, const uint32_t* which, const void* d_bits,
                                                      size_t k, const void* d_msgs32, const void* d_sigs192, const uint8_t rnd[32], void* stream);
int mi355_bls_debug_aggregate_bits_routes(mi355_bls_ctx* ctx, uint32_t out[2]);

/* aggregateAll on signatures for MANY groups in ONE device pass: the signature half of the same template
 * (genAggregatorProcedures(AggregateSignature, Signature, p2), blst_min_pubkey_sig_core.nim:142-211), each sum finished to its affine image
 * (blst_p2_to_affine) and serialised (serialize(Signature), bls_sig_io.nim:225-234) - what a node that aggregates the unaggregated
 * attestations of a slot sends.  mi355_bls_g2_aggregate takes one group per call and leaves a Jacobian point; a device call costs about
 * 2.2 ms whatever its size, so k groups that way cost k times that.
 *   sigs192   n_table x 192-byte blst_p2_affine images: the signature table
 *   idx, offsets   the addressing of mi355_bls_aggregate_sets (idx == NULL: group g is signatures [offsets[g], offsets[g+1]) of the table)
 *   out_sigs192    k x 192 bytes: the blst_p2_affine image of aggregateAll(signatures of group g), packed by group
 *   out_sigs96     k x 96 bytes: that aggregate's compressed wire form.  Either output may be NULL, not both.
 *   status    k bytes, host memory:
 *             0 ok;
 *             1 empty group (the reference returns false): both outputs are the infinity encodings;
 *             2 the sum is the point at infinity - a legal signature (bls_sig_io.nim:56), so the outputs are its valid encodings (192 zero
 *               bytes; 0xc0 and 95 zero bytes); flagged so that a caller can tell;
 *             3 an index was >= n_table: it is never dereferenced, 3 wins over 1 and 2, the outputs are the infinity encodings.
 * An all-zero member (the affine infinity image) adds nothing, as in mi355_bls_g2_aggregate.  Device pointers are 4-byte aligned.
 * Preconditions as the reference's: signatures decoded and group-checked (mi355_bls_deserialize_signatures).  Any k and any group lengths
 * up to 2^32 - 2 signatures in all; nothing here is bounded by max_sets.
 * Returns 1 when every status is 0, else 0; k == 0: 0, nothing written.  MI355_BLS_ERR_ARG for decreasing offsets, offsets[k] > n_table
 * without idx, NULL inputs, both outputs NULL.  The _device form enqueues on `stream` and synchronises it once, for the status bytes; its
 * d_out_sigs192 (k x 192 bytes, packed) is exactly the d_sigs192 argument of mi355_bls_aggregate_sets_device and
 * mi355_bls_batch_fast_aggregate_verify_device, so wire signatures in, grouped aggregates out and their verification against committee keys
 * all stay on the device.
 * Level 0 of the sum keeps the key side's 8 signatures per lane (csrc/plan.hpp AGG_C); a smaller count was not tried.
 * COST for k groups against one mi355_bls_g2_aggregate_device call per group (profiles/aggregate_signatures_bench.json):
 * not measured yet: run nim-blscurve_amd/tools/bench_aggsigs.py on an MI355X, which writes both timings, the host oracle's and the spread. */
int mi355_bls_aggregate_signature_sets(mi355_bls_ctx* ctx, const void* sigs192, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                       void* out_sigs192, void* out_sigs96, uint8_t* status);
int mi355_bls_aggregate_signature_sets_device(mi355_bls_ctx* ctx, const void* d_sigs192, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                              size_t k, void* d_out_sigs192, void* d_out_sigs96, uint8_t* status, void* stream);
/* aggregateVerify for MANY groups in ONE device pass: aggregateVerify(publicKeys, messages, signature) (bls_sig_min_pubkey.nim:127-199 ->
 * ContextCoreAggregateVerify, blst_min_pubkey_sig_core.nim:305-414) for k groups of (key, message) pairs with DISTINCT messages, each under one
 * aggregate signature: out[g] = [ e(-G1, sig_g) * prod_j e(pk_gj, H(m_gj)) == 1 ].  mi355_bls_aggregate_verify checks one aggregate per call
 * and pays a device call and a synchronisation for each.
 *   keys, n_table, idx, offsets   the addressing of mi355_bls_aggregate_sets: a table of 96-byte blst_p1_affine images; idx == NULL: group g is
 *             keys [offsets[g], offsets[g+1]) of the table (offsets[k] <= n_table); else group g is keys idx[offsets[g]] ..
 *             idx[offsets[g+1] - 1] (offsets[k] = the length of idx; repeats allowed).  offsets: k + 1 entries in HOST memory, non-decreasing.
 *   msgs32    offsets[k] x 32 bytes: the message of every POSITION p at byte 32 p - by position, never through idx.  Messages are 32 bytes
 *             (signing roots) as in every batched entry point; other lengths stay with mi355_bls_aggregate_verify, one aggregate per call.
 *   sigs192   k x 192-byte blst_p2_affine images, packed, one per group: the very buffer mi355_bls_aggregate_signature_sets_device writes.
 *   out       k bytes, host memory: 0 or 1.  0 for an empty group (bls_sig_min_pubkey.nim:167-169), for a group with a key at infinity (update
 *             returns false) and for a group with an index >= n_table, which is never dereferenced.  A signature at infinity contributes
 *             e(-G1, inf) = 1, as in mi355_bls_verify_each.
 * Device pointers are 4-byte aligned.  Preconditions as the reference's: keys and signatures decoded and group-checked, proofs of possession
 * verified by the caller.  No input is refused for its size: the call runs in slices of at most max_sets pairs - whole groups while they fit,
 * a longer group in parts whose Miller values are multiplied together on the device - and the workspace is sized by a slice, not by the call
 * (up to 2^32 - 2 pairs and groups: the tables are 32-bit).
 * Returns 1 iff every out[g] is 1; k == 0: 0, nothing written.  MI355_BLS_ERR_ARG for decreasing offsets, offsets[k] > n_table without idx,
 * NULL pointers.  The _device form enqueues on `stream` and synchronises it once, for the verdict bytes.
 * The width of the per-step line products (csrc/plan.hpp AGGV_C = 8) and the hand-over between the two tail forms (verify_each's) are not
 * measured for this path.  COST against one mi355_bls_aggregate_verify call per group: nim-blscurve_amd/tools/bench_aggverify_each.py
 * writes profiles/aggregate_verify_each_bench.json on an MI355X; README.md says whether it has been run.
 * debug_aggregate_verify_each_gt: TEST HOOK, the host form with gt_out = k x 576 bytes, the blst_fp12 image of every group's final
 * exponentiation (zero bytes for an empty group). */
int mi355_bls_aggregate_verify_each(mi355_bls_ctx* ctx, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                    const void* msgs32, const void* sigs192, uint8_t* out);
int mi355_bls_aggregate_verify_each_device(mi355_bls_ctx* ctx, const void* d_keys, size_t n_table, const uint32_t* d_idx, const size_t* offsets, size_t k,
                                           const void* d_msgs32, const void* d_sigs192, uint8_t* out, void* stream);
int mi355_bls_debug_aggregate_verify_each_gt(mi355_bls_ctx* ctx, const void* keys, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                             const void* msgs32, const void* sigs192, uint8_t* out, uint8_t* gt_out);
/* PAIRING-PRODUCT CHECKS over pairs the caller already holds, k at once: the batched device counterpart of blst_miller_loop_n + blst_final_exp +
 * blst_fp12_finalverify with blst_p1_affine_in_g1 / blst_p2_affine_in_g2 in front (blst_abi.nim:294,317,453-461).  Every verifier above builds
 * its own pairs, (pk, H(m)) and (-G1, sig); these calls take any (P, Q) - what a caller who commits on the device (mi355_bls_p1s_mult_table_many)
 * needs to verify openings, e.g. e(C - [y]G1, G2) * e(-pi, [tau - z]G2) == 1.
 *   p1s96     n x 96-byte blst_p1_affine images;  q2s192: n x 192-byte blst_p2_affine images.  All zero: the point at infinity.  Pair i is
 *             (p1s96[i], q2s192[i]).  Coordinates are canonical Montgomery images, as blst writes them.
 *   offsets   k + 1 entries in HOST memory, non-decreasing, offsets[0] == 0, offsets[k] == n: group g is pairs [offsets[g], offsets[g+1]).
 *   flags     0: the caller vouches that every operand is on its curve and in G1 / G2 - the precondition of every verifier of this library.
 *             MI355_BLS_PAIR_VALIDATE: the device checks every finite operand for both (the comparison and the endomorphism tests of the
 *             uncompressed decoders); a failing pair never reaches the Miller loop with its own coordinates (it is given infinite operands)
 *             and forces the verdict of its group to 0.
 *   status    n bytes, host memory: MI355_BLS_PAIR_* per pair (P is checked first).  May be NULL when flags == 0 (all zero if given); required
 *             under MI355_BLS_PAIR_VALIDATE.
 * pairing_check_each:  out[g] = [ final_exp( prod_j miller(P_gj, Q_gj) ) == 1 ], k bytes of host memory.  A pair with an operand at infinity
 *             contributes 1 (blst_miller_loop_n skips it).  An EMPTY group is the empty product: verdict 1 - on purpose unlike the
 *             signature-level calls above, whose 0 for empty input is the reference's scheme-level rule (bls_sig_min_pubkey.nim:167-169), not
 *             arithmetic.  Returns 1 iff every out[g] is 1; k == 0: 0, nothing written.
 * pairing_products:    the same, and gt_out (k x 576 bytes, host memory) receives the blst_fp12 image of every group's value after the final
 *             exponentiation - the library's fixed exponent, the one oracle/bls12381_py.py final_exp defines and every other path of
 *             this library uses, so two values are comparable with each other and with the debug hooks' values.  An empty group: the image of one.  Compare e(A, B) with e(C, D) through it.
 * batch_pairing_check: ONE verdict for all k checks: [ final_exp( prod_g prod_j miller([r_g]P_gj, Q_gj) ) == 1 ], r_g the g-th 64-bit scalar of
 *             the serial blinding chain from rnd32 (the chain mi355_bls_batch_verify_serial gives set g; nonzero by construction).  The G1
 *             side is multiplied; G2 is not touched.  Empty groups contribute nothing; every group empty: 1; k == 0: 0.  The scalars are
 *             cleared from host and device memory before the call returns.  SOUNDNESS: a false check passes with probability 2^-64 only when
 *             every operand is in G1 / G2 - vouched for (flags == 0) or checked (MI355_BLS_PAIR_VALIDATE); a failing pair makes the verdict 0.
 * batch_pairing_check_locate: batch_pairing_check first; out (k bytes) is all 1 when it passes, else pairing_check_each fills it.  Returns the
 *             first call's verdict.
 * debug_batch_pairing_check_scalars: TEST HOOK, batch_pairing_check with k scalars of the test's choice and the 576-byte value in gt_out.
 * No call is refused for its size: a call runs in slices of at most max_sets pairs - whole groups while they fit, a longer group in parts
 * whose Miller values are multiplied together on the device.  MI355_BLS_ERR_ARG, before anything is launched, for a NULL context (first),
 * NULL arrays with work to do, offsets that decrease or do not start at 0, a device pointer that is not 4-byte aligned, unknown flag bits,
 * status == NULL under MI355_BLS_PAIR_VALIDATE.  The _device forms take p1s96 / q2s192 in device memory, enqueue on `stream` and synchronise
 * it once.  The width of the per-step line products (AGGV_C = 8) and the tail hand-over are inherited from aggregate_verify_each and were not
 * re-measured.  COST: nim-blscurve_amd/tools/bench_pairing_check.py writes profiles/pairing_check_bench.json; README.md says whether it has run. */
#define MI355_BLS_PAIR_VALIDATE 1u
#define MI355_BLS_PAIR_OK 0
#define MI355_BLS_PAIR_P_OFF_CURVE 1
#define MI355_BLS_PAIR_P_NOT_IN_G1 2
#define MI355_BLS_PAIR_Q_OFF_CURVE 3
#define MI355_BLS_PAIR_Q_NOT_IN_G2 4
int mi355_bls_pairing_check_each(mi355_bls_ctx* ctx, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags, uint8_t* out,
                                 uint8_t* status);
int mi355_bls_pairing_check_each_device(mi355_bls_ctx* ctx, const void* d_p1s96, const void* d_q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                        uint8_t* out, uint8_t* status, void* stream);
int mi355_bls_pairing_products(mi355_bls_ctx* ctx, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags, uint8_t* out,
                               uint8_t* status, uint8_t* gt_out);
int mi355_bls_pairing_products_device(mi355_bls_ctx* ctx, const void* d_p1s96, const void* d_q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                      uint8_t* out, uint8_t* status, uint8_t* gt_out, void* stream);
int mi355_bls_batch_pairing_check(mi355_bls_ctx* ctx, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                  const uint8_t rnd32[32], uint8_t* status);
int mi355_bls_batch_pairing_check_device(mi355_bls_ctx* ctx, const void* d_p1s96, const void* d_q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                         const uint8_t rnd32[32], uint8_t* status, void* stream);
int mi355_bls_batch_pairing_check_locate(mi355_bls_ctx* ctx, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                         const uint8_t rnd32[32], uint8_t* status, uint8_t* out);
int mi355_bls_batch_pairing_check_locate_device(mi355_bls_ctx* ctx, const void* d_p1s96, const void* d_q2s192, const size_t* offsets, size_t k,
                                                uint32_t flags, const uint8_t rnd32[32], uint8_t* status, uint8_t* out, void* stream);
int mi355_bls_debug_batch_pairing_check_scalars(mi355_bls_ctx* ctx, const void* p1s96, const void* q2s192, const size_t* offsets, size_t k, uint32_t flags,
                                                const uint64_t* r, uint8_t* status, uint8_t* gt_out);
/* serialize(Signature) (bls_sig_io.nim:225-234), i.e. blst_p2_affine_compress, for n signatures: 192-byte blst_p2_affine images in, 96 bytes
 * each out (ZCash form: big-endian x.c1 then x.c0, bit 7 of byte 0 set, bit 5 set when y is the lexicographically larger root - decided by
 * y.c1 unless it is zero, then by y.c0; the all-zero infinity image gives 0xc0 and 95 zero bytes).  The device form writes device memory
 * (d_out96: n x 96 B, 4-byte aligned like d_sigs192) and returns when the bytes are there.  Returns 0, negative on failure. */
int mi355_bls_compress_signatures(mi355_bls_ctx* ctx, const void* sigs192, size_t n, uint8_t out96[]);
int mi355_bls_compress_signatures_device(mi355_bls_ctx* ctx, const void* d_sigs192, size_t n, void* d_out96, void* stream);
/* Signature.fromBytes (bls_sig_io.nim:42-58) for n signatures that arrive without a key or a message (an attestation's signature): the
 * signature half of mi355_bls_deserialize_sets_ex, by the same decoder.  sigs: n x 96 bytes, or n x 192 with
 * MI355_BLS_DESER_SIG_UNCOMPRESSED; MI355_BLS_DESER_KNOWN_ON_CURVE skips the subgroup check; MI355_BLS_DESER_PK_UNCOMPRESSED is
 * MI355_BLS_ERR_ARG (flags are defined with that call, below).  out_sigs192: n x 192-byte blst_p2_affine images, zeroed where status[i] is not 0;
 * status[i]: 0 ok, 4 bad encoding, 5 not in G2, as mi355_bls_deserialize_sets gives them.  The infinity signature is allowed (status 0, the
 * all-zero image).  Returns 1 when every status is 0, else 0 (n == 0: 1); negative on failure.  Any n.  The host form's out_sigs192 and
 * both forms' status may be NULL; the _device form reads d_sigs and writes d_out_sigs192 (4-byte aligned) in device memory, status stays
 * host memory. */
int mi355_bls_deserialize_signatures(mi355_bls_ctx* ctx, const uint8_t* sigs, size_t n, uint32_t flags, void* out_sigs192, uint8_t* status);
int mi355_bls_deserialize_signatures_device(mi355_bls_ctx* ctx, const void* d_sigs, size_t n, uint32_t flags, void* d_out_sigs192, uint8_t* status,
                                            void* stream);
/* PublicKey.fromBytes / fromBytesKnownOnCurve (bls_sig_io.nim:81-121) for n keys that arrive without a signature or a message (a validator
 * key table in its wire form): the key half of mi355_bls_deserialize_sets_ex, by the same decoder.  This is the call that MAKES the
 * device-resident key table the table-addressed calls take (aggregate_sets[_bits], fast_aggregate_verify_each, aggregate_verify_each, the pop
 * calls): the _device form's d_out_pks96 is their d_keys / d_pks96 argument as it stands.  pks: n x 48 bytes, or n x 96 with
 * MI355_BLS_DESER_PK_UNCOMPRESSED; MI355_BLS_DESER_KNOWN_ON_CURVE skips the subgroup check; MI355_BLS_DESER_SIG_UNCOMPRESSED is
 * MI355_BLS_ERR_ARG (flags are defined with mi355_bls_deserialize_sets_ex, below).  out_pks96: n x 96-byte blst_p1_affine images, all zero
 * where status[i] is not 0; status[i]: 0 ok, 1 bad encoding, 3 infinity, 2 not in G1, in that precedence, as mi355_bls_deserialize_sets
 * gives them.  Returns 1 when every status is 0, else 0 (n == 0: 1); negative on failure.  Any n.  The host form's out_pks96 and both
 * forms' status may be NULL; the _device form reads d_pks and writes d_out_pks96 (4-byte aligned) in device memory, status stays host memory.
 * COST on one MI355X, device-resident, median of 5 blocking calls (profiles/key_table_bench.json): 1.49 / 1.76 / 23.7 ms at 4 096 / 65 536 / 2^20
 * keys, against 3.45 / 3.59 / 55.7 ms for mi355_bls_deserialize_sets_ex_device over the same keys with one valid signature repeated in every row. */
int mi355_bls_deserialize_public_keys(mi355_bls_ctx* ctx, const uint8_t* pks, size_t n, uint32_t flags, void* out_pks96, uint8_t* status);
int mi355_bls_deserialize_public_keys_device(mi355_bls_ctx* ctx, const void* d_pks, size_t n, uint32_t flags, void* d_out_pks96, uint8_t* status,
                                             void* stream);
/* Key admission: what a deposit needs before its key may enter the table - PublicKey.fromBytes, Signature.fromBytes and popVerify
 * (bls_sig_io.nim:42-58, 81-99; bls_sig_min_pubkey.nim:60-74) - for n (key, proof of possession) rows in their wire forms, one status per row.
 * pks: n x 48 bytes, or n x 96 with MI355_BLS_DESER_PK_UNCOMPRESSED; proofs: n x 96 bytes, or n x 192 with MI355_BLS_DESER_SIG_UNCOMPRESSED;
 * MI355_BLS_DESER_KNOWN_ON_CURVE is MI355_BLS_ERR_ARG (admission is the full check).  status[i] is the first that applies of: the key's status
 * 1, 3 or 2 (mi355_bls_deserialize_public_keys); the proof's status 4 or 5 (mi355_bls_deserialize_signatures); MI355_BLS_KEY_BAD_PROOF when
 * both decode and popVerify(pk_i, proof_i) is false (the infinity proof included); 0.  status[i] == 0 iff the reference's three calls all
 * succeed on row i; it depends on row i alone, whatever rnd is (rnd blinds the batch check as in mi355_bls_batch_pop_verify_locate, whose
 * per-pair pass decides every row of a failing batch).  out_pks96: n x 96-byte images, row i the key where status[i] is 0 and all zero
 * elsewhere - a table to use as it is.  Only the rows that decode reach the possession check, packed: a row that does not decode costs
 * the others nothing, and a call in which no row decodes does no pairing work.  Returns 1 when every status is 0, else 0 (n == 0: 1,
 * nothing written); negative on failure.  Any n (the check runs in slices of the context's capacity).  status and rnd are required; the host
 * form's out_pks96 may be NULL.  The _device form reads d_pks and d_proofs and writes d_out_pks96 (4-byte aligned) in device memory.
 * COST on one MI355X, device-resident, median of 5 blocking calls (profiles/key_table_bench.json), at 4 096 / 65 536 / 2^20 rows: 7.0 / 15.4 /
 * 253 ms all valid, 7.0 / 16.0 / 251 ms with 1 % of the keys undecodable.  mi355_bls_deserialize_sets_ex_device, a host split of the records and
 * mi355_bls_batch_pop_verify_locate_device over the same rows: 7.3 / 19.8 / 337 ms all valid, 26.6 / 91.1 / 1 461 ms on the 1 % table (its zeroed
 * rows fail the batch, so every row pays the per-pair pass). */
#define MI355_BLS_KEY_BAD_PROOF 8
int mi355_bls_admit_keys(mi355_bls_ctx* ctx, const uint8_t* pks, const uint8_t* proofs, size_t n, uint32_t flags, const uint8_t rnd[32], void* out_pks96,
                         uint8_t* status);
int mi355_bls_admit_keys_device(mi355_bls_ctx* ctx, const void* d_pks, const void* d_proofs, size_t n, uint32_t flags, const uint8_t rnd[32],
                                void* d_out_pks96, uint8_t* status, void* stream);
/* recover(signs, ids) (blst_recovery.nim:150-156: lagrangeInterpolation, :90-121, at 0 in the exponent) for k groups of threshold-signature
 * shares in one device pass: group g's t_g shares, made with Shamir shares of one secret key, give the signature of that key.
 *   sigs192, n_table, idx, offsets   the addressing of mi355_bls_aggregate_signature_sets: a table of 192-byte blst_p2_affine images, an
 *                  optional index array, k + 1 host offsets (group g = positions [offsets[g], offsets[g+1]) of the share sequence)
 *   ids32          32 bytes per SEQUENCE POSITION: ids32[32 p ..] belongs to position p of the index array, or of the table when idx is NULL;
 *                  offsets[k] x 32 bytes in all
 *   out_sigs192    k x 192 bytes: the blst_p2_affine image of the recovered signature, packed by group
 *   out_sigs96     k x 96 bytes: its compressed wire form.  Either output may be NULL, not both.
 *   status    k bytes, host memory, in this precedence:
 *             3 an index was >= n_table (never dereferenced);
 *             1 empty group (the reference: "invalid inputs");
 *             6 MI355_BLS_REC_ZERO_ID: two or more shares and an id that is 0 mod r (the reference tests this before duplicates);
 *             7 MI355_BLS_REC_DUP_ID: two or more shares and two ids equal mod r;
 *             2 the interpolated point is the point at infinity: its valid encodings are returned (192 zero bytes; 0xc0 and 95 zero bytes);
 *             0 recovered.  Any status but 0 and 2 also yields the infinity encodings.
 * CONTRACT FOR AN ID: the 32 little-endian bytes of a blst_scalar (ID.fromUint32(a) lays word a[0] lowest, so the reference test's
 * [0, .., 0, x] is x 2^224), and the id's VALUE is that 256-bit integer mod r - blst_fr_from_scalar is a Montgomery multiplication by R^2,
 * which reduces.  This is this library's contract; the reference's own tests only use ids below r.
 * A group of one share returns that share whatever its id, 0 included (the reference returns before it looks at the id).  An all-zero share
 * (the infinity image) contributes nothing.  Device pointers are 4-byte aligned.  Shares are decoded and group-checked by the caller
 * (mi355_bls_deserialize_signatures).  VARIABLE TIME: signature shares and public ids only - the secret-key half of blst_recovery.nim
 * (genSecretShare, recover(secrets, ids), add) is not offered and stays on the CPU.
 * Any k and any group lengths below 2^32 - 1 positions in all: the call runs in chunks of whole groups (csrc/plan.hpp REC_MEMBERS_CHUNK),
 * so its device workspace does not grow with the call; nothing is bounded by max_sets.  Work is O(t^2) field products per group, as in the
 * reference, beside t G2 multiplications by 255-bit scalars, one lane per share.
 * Returns 1 when every status is 0, else 0; k == 0: 0, nothing written.  MI355_BLS_ERR_ARG for decreasing offsets, offsets[k] > n_table
 * without idx, NULL inputs, both outputs NULL.  The _device form enqueues on `stream` and synchronises it once per chunk, for the status
 * bytes; its d_out_sigs192 (k x 192 bytes, packed) is exactly the d_sigs192 argument of mi355_bls_aggregate_sets_device and
 * mi355_bls_batch_fast_aggregate_verify_device - that is why the call exists: decoded shares in, recovered signatures out and their
 * verification all stay on the device.
 * COST (profiles/recover_signatures_bench.json, nim-blscurve_amd/tools/bench_recover.py): 256 groups of 3 .. 7 shares 7.7 - 7.9 ms, 65 536 groups
 * 38 - 73 ms, device-resident; the floor is one wave's 255-bit multiplication, about 7.5 ms, so for ONE group a single
 * mi355_bls_p2s_mult_pippenger call with host coefficients (about 5 ms) is the faster route. */
#define MI355_BLS_REC_ZERO_ID 6
#define MI355_BLS_REC_DUP_ID 7
int mi355_bls_recover_signature_sets(mi355_bls_ctx* ctx, const void* sigs192, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                                     const void* ids32, void* out_sigs192, void* out_sigs96, uint8_t* status);
int mi355_bls_recover_signature_sets_device(mi355_bls_ctx* ctx, const void* d_sigs192, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                            size_t k, const void* d_ids32, void* d_out_sigs192, void* d_out_sigs96, uint8_t* status, void* stream);

/* coreVerifyNoGroupCheck on an AggregatePublicKey the caller already holds (core :269-297): agg_p1 = blst_p1 (Jacobian, 144 B), e.g.
 * mi355_bls_p1s_add of the per-rank mi355_bls_g1_aggregate_device partial sums of a key-sharded fastAggregateVerify (one process per
 * GPU).  Aggregate at infinity -> 0. */
int mi355_bls_verify_aggregate(mi355_bls_ctx* ctx, const uint8_t agg_p1[144], const uint8_t* msg, size_t msg_len, const void* sig);

/* blst_p1s_mult_pippenger (blst_abi.nim:336-340; blst+nim.h:70-72; call sites benchmarks/bls12381_msm_g1.nim:50-59,
 * blst_min_pubkey_sig_core.nim:629): ret = sum_i [k_i mod 2^nbits] P_i as blst_p1 (Jacobian, 144 B).
 * points[0] -> npoints contiguous blst_p1_affine, scalars[0] -> npoints 32-byte little-endian scalars, both
 * NULL-terminated pointer lists in HOST memory exactly as the reference passes them; nbits in 1..256.
 * The device workspace is (re)sized inside the context on first use, so the scratch size is 0. */
size_t mi355_bls_p1s_mult_pippenger_scratch_sizeof(size_t npoints);
int mi355_bls_p1s_mult_pippenger(mi355_bls_ctx* ctx, uint8_t ret_p1[144], const void* const points[], size_t npoints,
                                 const uint8_t* const scalars[], size_t nbits);
/* EXACTLY blst_p1s_mult_pippenger / blst_p1s_mult_pippenger_scratch_sizeof (blst+nim.h:70-72; blst_abi.nim:336-340): same
 * argument list and void result, so `importc: "mi355_p1s_mult_pippenger"` replaces the BLST symbol with no other change at
 * the call sites (benchmarks/bls12381_msm_g1.nim:47-59; blst_min_pubkey_sig_core.nim:629-636).  blst's conventions:
 *   points[] / scalars[]: list[0] points at element 0; each following element is taken from the next list entry if that is
 *     non-NULL, else it follows the previous element in memory ([ptr, NULL] = one contiguous array; npoints pointers = one
 *     per element);
 *   scalars are little-endian, (nbits + 7) / 8 bytes each (32 for nbits = 255, 8 for the u64 scalars of `combine`);
 *   ret: blst_p1 (Jacobian, 144 B); scratch: ignored (the workspace lives on the device; scratch_sizeof returns 8).
 * Runs on the process-wide default context.  A runtime failure (no GPU, HIP error) cannot be returned through a void
 * signature: the function prints the error and aborts. */
size_t mi355_p1s_mult_pippenger_scratch_sizeof(size_t npoints);
void mi355_p1s_mult_pippenger(void* ret, const void* const points[], size_t npoints, const uint8_t* const scalars[], size_t nbits, void* scratch);
/* EXACTLY blst_p2s_mult_pippenger / ..._scratch_sizeof (blst+nim.h:90-92; blst_abi.nim:358-362; call site
 * blst_min_pubkey_sig_core.nim:639-646): the same on G2 (points: blst_p2_affine, 192 B; ret: blst_p2, 288 B). */
size_t mi355_p2s_mult_pippenger_scratch_sizeof(size_t npoints);
void mi355_p2s_mult_pippenger(void* ret, const void* const points[], size_t npoints, const uint8_t* const scalars[], size_t nbits, void* scratch);
/* context forms on G2 (32-byte scalar images, host or device arrays), as the mi355_bls_p1s_* pair */
int mi355_bls_p2s_mult_pippenger(mi355_bls_ctx* ctx, uint8_t ret_p2[288], const void* const points[], size_t npoints,
                                 const uint8_t* const scalars[], size_t nbits);
int mi355_bls_p2s_mult_pippenger_device(mi355_bls_ctx* ctx, uint8_t ret_p2[288], const void* d_points, size_t npoints,
                                        const void* d_scalars, size_t nbits, void* stream);

/* same with both arrays resident in device memory */
int mi355_bls_p1s_mult_pippenger_device(mi355_bls_ctx* ctx, uint8_t ret_p1[144], const void* d_points, size_t npoints,
                                        const void* d_scalars, size_t nbits, void* stream);

/* k G1 MSMs in one device pass: ret[j] = the blst_p1 image (Jacobian, 144 B) of MSM j.  A single MSM of a few thousand points costs about as
 * much as one sixteen times its size (the floor of a device call); k of them here share the stages of one bucket method over k x (windows of
 * one MSM) virtual windows, with one Horner walk per MSM at the end.  Points, scalars and nbits (1..256) mean what they mean in
 * mi355_bls_p1s_mult_pippenger_device: 96-byte blst_p1_affine images (all-zero = infinity; subgroup membership is not assumed), 32-byte
 * little-endian scalar images of which the low nbits count.  Two addressing forms:
 *   ragged (offsets != NULL)   k + 1 host values, offsets[0] == 0, non-decreasing, offsets[k] == npoints: MSM j is over points and scalars
 *                              [offsets[j], offsets[j + 1]), point i with scalar i; an empty range gives infinity (144 zero bytes)
 *   shared base (offsets == NULL)   every MSM is over all npoints points; the scalar array holds k x npoints scalars, MSM j uses
 *                              [j npoints, (j + 1) npoints); the points are read and converted once
 * No call is refused for its size - only a single MSM of more than 2^28 points is (MI355_BLS_ERR_ARG before anything is launched), as in
 * the single call: a call beyond what one pass holds (csrc/plan.hpp MSM_MANY_*) runs as consecutive passes over ranges of
 * MSMs, a member that alone exceeds a pass takes the single-MSM path, and so does a call with k == 1.  An infinite result is 144 zero bytes
 * when a pass of this call made it; compare results as points, as with the single call.
 *   _many          host arrays (contiguous, not pointer lists), results to ret (k x 144 B)
 *   _many_device   arrays in device memory; results to ret (host, may be NULL) and / or d_out (device, k x 144 B, 4-byte aligned, may be NULL),
 *                  every pass enqueued on `stream` alone (a member handed to the single path runs as the single call does), and waited
 *                  for before the call returns
 * k == 0 returns 0 and touches nothing.  MI355_BLS_ERR_ARG: a NULL context (before any other rule), NULL arrays with work to do, bad
 * offsets, nbits outside 1..256, no output, an MSM of more than 2^28 points. */
int mi355_bls_p1s_mult_pippenger_many(mi355_bls_ctx* ctx, uint8_t* ret, const void* points, size_t npoints, const void* scalars, const size_t* offsets,
                                      size_t k, size_t nbits);
int mi355_bls_p1s_mult_pippenger_many_device(mi355_bls_ctx* ctx, uint8_t* ret, void* d_out, const void* d_points, size_t npoints, const void* d_scalars,
                                             const size_t* offsets, size_t k, size_t nbits, void* stream);

/* k G2 MSMs in one device pass (blst_p2s_mult_pippenger, blst_abi.nim:358-362, k at once): the G2 counterpart of
 * mi355_bls_p1s_mult_pippenger_many, with the same two addressing forms (ragged with k + 1 host offsets; shared base with offsets == NULL and
 * k x npoints scalars), the same argument rules and the same error rules.  Points are 192-byte blst_p2_affine images (all-zero = infinity;
 * subgroup membership is not assumed), scalars 32-byte little-endian images of which the low nbits count, nbits in 1..256; ret[j] / d_out[j] is
 * the blst_p2 image (Jacobian, 288 B) of MSM j, an infinite result made by a pass 288 zero bytes; compare results as points, or normalise them
 * with mi355_bls_p2s_to_affine.  What it is for: the k tiny linear combinations [tau - z_g]G2 of k openings, or one recovery with host
 * coefficients per group - each of them a floor of a device call when made through mi355_bls_p2s_mult_pippenger_device.  The stages are the
 * G1 call's over 384-byte points (csrc/plan.hpp MSM_MANY_G2_*: half the buckets per pass, one lane per segment), and ONE Horner walk per MSM at
 * the end (k_pip_tail_many_g2: nbits doublings per MSM in all, one workgroup per MSM).
 *   _many          host arrays (contiguous, not pointer lists), results to ret (k x 288 B)
 *   _many_device   arrays in device memory; results to ret (host, may be NULL) and / or d_out (device, k x 288 B, 4-byte aligned, may be NULL),
 *                  every pass enqueued on `stream` alone, and waited for before the call returns
 * k == 0 returns 0 and touches nothing; k == 1, and a member of more than 2^20 pairs, take the single G2 path unchanged.  No call is refused
 * for its size - only a single MSM of more than 2^28 points is.  MI355_BLS_ERR_ARG, before anything is launched: a NULL context (before any
 * other rule), NULL arrays with work to do, bad offsets, nbits outside 1..256, no output, a d_out that is not 4-byte aligned, an MSM of more
 * than 2^28 points.  Variable time, like every MSM here.  The window width is the G1 rule (pip_for) and was not measured for G2.
 * COST (one MI355X, device-resident, 255 bits, median of 5 blocking calls; nim-blscurve_amd/tools/bench_msm_g2_many.py, a PARTIAL run: the rows
 * named in profiles/msm_g2_many_bench.json): 64 MSMs of 4 096 points 10.8 - 10.9 ms, shared or ragged, against 395 - 398 ms for 64 single
 * calls and 8.3 ms for one MSM over all pairs; 4 096 MSMs of 2 points 232 ms: 82 x faster than single calls (measured on 64, scaled) but 37 x
 * one MSM over the same 8 192 pairs - SLOW for tiny members (52 five-bit windows each).  Other rows not measured yet: run the tool. */
int mi355_bls_p2s_mult_pippenger_many(mi355_bls_ctx* ctx, uint8_t* ret, const void* points, size_t npoints, const void* scalars, const size_t* offsets,
                                      size_t k, size_t nbits);
int mi355_bls_p2s_mult_pippenger_many_device(mi355_bls_ctx* ctx, uint8_t* ret, void* d_out, const void* d_points, size_t npoints, const void* d_scalars,
                                             const size_t* offsets, size_t k, size_t nbits, void* stream);

/* blst_p1s_to_affine / blst_p2s_to_affine (blst_abi.nim:323, :345) for n CONTIGUOUS Jacobian images (not pointer lists: the device forms
 * cannot take those): n x 144 B blst_p1 -> n x 96 B blst_p1_affine, n x 288 B blst_p2 -> n x 192 B blst_p2_affine.  Every MSM call here
 * returns Jacobian images and every consumer takes affine ones; with these calls the results need not visit the host in between: the d_out
 * of a _device form is, as it stands, the d_p1s96 / d_q2s192 argument of the pairing calls, the d_keys argument of the table-addressed calls
 * and the input of mi355_bls_compress_public_keys_device / mi355_bls_compress_signatures_device.
 *   Z == 0 gives the all-zero image: the library's affine infinity, what the pairing calls skip.  Output bytes are canonical Montgomery
 *   images.  Input and output must NOT overlap (a lane reads its points twice).  A lane takes a run of consecutive points and shares one
 *   inversion among them (csrc/toaffine.hpp; the run length is csrc/plan.hpp to_affine_for's: neither the rule nor its cap of 8 is measured).
 *   _device: both arrays in device memory, 4-byte aligned; every launch is enqueued on `stream`, which is waited for once.  Any n: beyond one
 *   launch's reach the library loops over chunks.
 * n == 0 returns 0 and touches nothing.  MI355_BLS_ERR_ARG for a NULL context (first), NULL arrays with work to do, or a device pointer that
 * is not 4-byte aligned.  Variable time (public points).
 * COST (the same partial run, n = 4 096): 0.089 ms (G1) and 0.112 ms (G2) per blocking call, against 0.072 and 0.175 ms for the two copies
 * of the same bytes (an earlier run of the same rows: 0.088 and 0.140) - on G1 the call is SLOWER than the copies it replaces, on G2 faster.
 * Blocking calls this short are mostly launch and synchronise latency: what the caller saves is the host arithmetic between the copies, which
 * these rows do not time.  n = 64 and 65 536 not measured yet: run nim-blscurve_amd/tools/bench_msm_g2_many.py.
 * debug_to_affine_set_run: TEST HOOK, the points per lane of the following to_affine calls on this context (capped at 8; 0: the plan's own). */
int mi355_bls_p1s_to_affine(mi355_bls_ctx* ctx, const uint8_t* in144, size_t n, uint8_t* out96);
int mi355_bls_p1s_to_affine_device(mi355_bls_ctx* ctx, const void* d_in144, size_t n, void* d_out96, void* stream);
int mi355_bls_p2s_to_affine(mi355_bls_ctx* ctx, const uint8_t* in288, size_t n, uint8_t* out192);
int mi355_bls_p2s_to_affine_device(mi355_bls_ctx* ctx, const void* d_in288, size_t n, void* d_out192, void* stream);
int mi355_bls_debug_to_affine_set_run(mi355_bls_ctx* ctx, uint32_t run);

/* Short linear combinations for k groups in one device pass, with the CALLER's scalars: out[g] = sum_p [s_p mod 2^nbits] P_(t(p)) over the
 * positions p of group g, as the canonical affine image (96-byte blst_p1_affine / 192-byte blst_p2_affine, Montgomery form; all zero =
 * infinity) - what the pairing calls, the compress calls and the table-addressed calls take, with no to_affine call in between.  One lane
 * per term multiplies (signed 4-bit windows, walked from window ceil(nbits / 4): 64-bit scalars pay 64 doublings), a segmented sum adds the
 * products of a group, one inversion per group finishes.  This is the call for MANY SHORT groups - k openings [tau - z_g]G2, recoveries with
 * host coefficients; mi355_bls_p?s_mult_pippenger_many stays the call for members of hundreds of points and more (its bucket method needs
 * them to pay for 52 windows per member).
 *   points, n_table, idx, offsets   the addressing of mi355_bls_aggregate_sets: a table of n_table affine images, an optional index array
 *                  (repeats allowed: a fixed base such as the G2 generator is a one-row table with idx all 0), k + 1 host offsets, non-decreasing
 *                  (group g = positions [offsets[g], offsets[g+1]) of the sequence)
 *   scalars32      32 little-endian bytes per SEQUENCE POSITION, never taken through idx; offsets[k] x 32 bytes in all
 *   nbits          1..256: only the low nbits bits of a scalar count
 *   flags          0: subgroup membership is NOT assumed, the scalar acts as an integer (as in the MSM calls).
 *                  MI355_BLS_LINCOMB_SUBGROUP (p2s only): the caller vouches that every point is in G2.  The scalar is then reduced mod r and
 *                  written in base |x| (four digits below 2^64); psi acts on G2 as [x], so one four-way walk of 64 doublings replaces the
 *                  256 of the plain route.  For a point outside G2 the result of this route is NOT the integer multiple.
 *   out            k x 96 / k x 192 bytes, packed by group
 *   status         k bytes, host memory: 3 an index was >= n_table (never dereferenced; wins over 1 and 2); 1 empty group; 2 the sum is the
 *                  point at infinity (the all-zero image is its valid image); 0 ok.  Any status but 0 gives the all-zero image.
 * An all-zero point and a zero scalar contribute nothing.  Device pointers are 4-byte aligned.
 * Returns 1 when every status is 0, else 0; k == 0: 0, nothing written.  MI355_BLS_ERR_ARG: a NULL context (before any other rule), NULL
 * arrays, decreasing offsets, offsets[k] > n_table without idx, a device pointer that is not 4-byte aligned, a busy context, nbits outside
 * 1..256, an unknown flag bit, MI355_BLS_LINCOMB_SUBGROUP on the p1s call.  No call is refused for its size: it runs in chunks of whole
 * groups (csrc/plan.hpp LINCOMB_TERMS_CHUNK), the workspace is sized by a chunk, nothing is bounded by max_sets.  The _device form enqueues
 * on `stream` and synchronises it once per chunk, for the status bytes.
 * VARIABLE TIME: public scalars only.
 * COST (one MI355X, device-resident, median of 5 blocking calls; profiles/lincomb_bench.json, nim-blscurve_amd/tools/bench_lincomb.py; plain /
 * MI355_BLS_LINCOMB_SUBGROUP / mi355_bls_p?s_mult_pippenger_many_device + mi355_bls_p?s_to_affine_device over the same terms):
 *   G2, 255 bits: 4 096 x 2 over a one-row table (openings) 7.37 / 5.17 / 172 ms; 256 x 3: 7.25 / 5.04 / 12.3 ms (recover_signature_sets_device
 *   over the same shares: 7.74 ms); 65 536 x 1: 11.3 / 8.66 / 2 662 ms; 4 096 x 16: 8.55 / 6.16 / 173 ms.  G2, 64 bits, 4 096 x 2: 2.28 / 2.45 /
 *   41.5 ms.  G1: 4 096 x 2 at 255 bits 3.23 ms against 58.2, at 64 bits 1.13 against 33.6; 65 536 x 1: 6.18 ms against 8 770.
 * WHICH CALL: this one for groups of up to some tens of terms - it won every measured row, 1.7 x to 1 400 x; larger members were not measured
 * against mi355_bls_p?s_mult_pippenger_many, whose bucket method is made for them.  WHICH ROUTE on G2: MI355_BLS_LINCOMB_SUBGROUP for scalars
 * wider than 64 bits when every point is known to be in G2 (1.3 - 1.4 x faster at 255 bits); flags 0 otherwise - at nbits = 64 the subgroup
 * route is the SLOWER one (0.93 x).  The floor of a call is one lane's walk: 7.2 ms for 256 doublings, 5.0 ms for the subgroup route, 2.3 ms
 * at 64 bits.
 * debug_lincomb_set_chunk: TEST HOOK, the terms per chunk of the following lincomb_many calls on this context (0: the plan's own). */
#define MI355_BLS_LINCOMB_SUBGROUP 1u
int mi355_bls_p1s_lincomb_many(mi355_bls_ctx* ctx, const void* points96, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                               const void* scalars32, size_t nbits, uint32_t flags, void* out96, uint8_t* status);
int mi355_bls_p1s_lincomb_many_device(mi355_bls_ctx* ctx, const void* d_points96, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                      size_t k, const void* d_scalars32, size_t nbits, uint32_t flags, void* d_out96, uint8_t* status, void* stream);
int mi355_bls_p2s_lincomb_many(mi355_bls_ctx* ctx, const void* points192, size_t n_table, const uint32_t* idx, const size_t* offsets, size_t k,
                               const void* scalars32, size_t nbits, uint32_t flags, void* out192, uint8_t* status);
int mi355_bls_p2s_lincomb_many_device(mi355_bls_ctx* ctx, const void* d_points192, size_t n_table, const uint32_t* d_idx, const size_t* offsets,
                                      size_t k, const void* d_scalars32, size_t nbits, uint32_t flags, void* d_out192, uint8_t* status, void* stream);
int mi355_bls_debug_lincomb_set_chunk(mi355_bls_ctx* ctx, size_t members);

/* Openings of k polynomials over the scalar field Fr in one device pass: for polynomial g of n scalars and its point z_g, the value
 * y_g = p_g(z_g) and the quotient q_g(X) = (p_g(X) - y_g) / (X - z_g), written as canonical 32-byte little-endian images in the scalar layout
 * the MSM calls read - a proof is mi355_bls_fr_open_many_device followed by mi355_bls_p1s_mult_table_many_device, or by
 * mi355_bls_p1s_mult_pippenger_many_device, over the quotients, with no scalar visiting the host.
 *   polys32        k x n 32-byte little-endian images; polynomial g is images [g n, (g + 1) n)
 *   zs32           k images
 *                  ANY 256-bit image is accepted and acts as its value mod r.
 *   out_ys32       k images in [0, r)
 *   out_quot32     k x n images in [0, r), laid out like polys32
 *   status         k bytes, HOST memory, may be NULL.  Both bits are informational - the outputs are valid whenever the call returns >= 0:
 *                  bit 0 (1): z lies in the domain (evaluation form only); bit 1 (2): an image of this polynomial, or its z, was >= r and
 *                  was reduced.
 *   Each output may be NULL on its own (it is then not computed or not stored); all three NULL is MI355_BLS_ERR_ARG, and so is the host form
 *   without out_ys32 and out_quot32.  Outputs must not overlap inputs.  Device pointers are 4-byte aligned (16-byte aligned ones are read
 *   and written 16 bytes at a time).
 * flags == 0, COEFFICIENT form: p_g = sum c_i X^i, domain32 must be NULL.  Quotient slot i holds q_i for i < n - 1 (q_(i-1) = c_i + z q_i);
 *   slot n - 1 holds 0, the PADDING SLOT: the n-point table that committed to p_g serves q_g as it stands.
 * MI355_BLS_FR_OPEN_EVAL, EVALUATION form: domain32 is required, n images x_i shared by all k polynomials - the n distinct n-th roots of unity
 *   of Fr, in the caller's order (natural, bit-reversed, any).  THAT THE DOMAIN IS THIS SET IS A PRECONDITION AND IS NOT CHECKED; with another
 *   set the outputs mean nothing (no fault).  n must be a power of two, at most 2^32: checked.  polys32 holds f_i = p_g(x_i).  For z outside
 *   the domain y = (z^n - 1) / n * sum f_i x_i / (z - x_i) and q_i = (f_i - y) / (x_i - z); for z = x_j: y = f_j, the other slots as before,
 *   q_j = sum over i != j of (f_i - y) x_i / (z (z - x_i)).
 * Returns the number of polynomials with status bit 1 set (0: none), k == 0: 0, nothing touched.  MI355_BLS_ERR_ARG, before anything is
 * launched: a NULL context (before the k == 0 rule), NULL inputs, n == 0, a flag other than MI355_BLS_FR_OPEN_EVAL, a domain without the flag or
 * the flag without a domain, n that is no power of two (or above 2^32) in evaluation form, a misaligned device pointer, a busy context.
 * Nothing else is refused for its size: k x n beyond one pass is cut into passes of whole polynomials (csrc/plan.hpp fropen_sizes_for); the
 * _device form enqueues on `stream` and synchronises it once per pass, for the status bytes.
 * One workgroup of 256 lanes owns one polynomial (csrc/fropen.hpp: two products per element in coefficient form, six in evaluation form
 * with ONE field inversion per polynomial).  A SINGLE very long polynomial (k = 1, n = 2^20) therefore runs on one workgroup: correct, slow;
 * a form that spreads one polynomial over several workgroups is not built.
 * VARIABLE TIME: public polynomials only.
 * COST: profiles/fr_open_bench.json (nim-blscurve_amd/tools/bench_fr_open.py), reported row by row in README.md.
 * debug_fropen_set_pass: TEST HOOK, the polynomials per pass of the following fr_open_many calls on this context (0: the plan's own; it
 * can only shorten a pass). */
#define MI355_BLS_FR_OPEN_EVAL 1u
int mi355_bls_fr_open_many(mi355_bls_ctx* ctx, const void* polys32, size_t n, const void* zs32, size_t k, uint32_t flags, const void* domain32,
                           uint8_t* out_ys32, uint8_t* out_quot32, uint8_t* status);
int mi355_bls_fr_open_many_device(mi355_bls_ctx* ctx, const void* d_polys32, size_t n, const void* d_zs32, size_t k, uint32_t flags,
                                  const void* d_domain32, void* d_out_ys32, void* d_out_quot32, uint8_t* status, void* stream);
int mi355_bls_debug_fropen_set_pass(mi355_bls_ctx* ctx, size_t polys_per_pass);

/* Number-theoretic transforms of k vectors over the scalar field Fr in one device pass, and the domain they and mi355_bls_fr_open_many's
 * evaluation form speak of: the link between that call's two forms, with no scalar visiting the host.
 *   r the group order, omega_n = 7^((r - 1) / n) mod r for n = 2^m, 0 <= m <= 32 (7 generates Fr*); rev_m(i) is i with its m low bits reversed.
 *   FORWARD  out[i] = sum_j in[j] (g omega_n^i)^j: coefficients in, values over the domain (g = 1) or over the coset g x domain out.
 *   MI355_BLS_FR_NTT_INVERSE  the exact inverse map: values in, coefficients out, the factor 1 / n and g^-j included.
 *   MI355_BLS_FR_NTT_BITREV   the EVALUATION side (the forward output, the inverse input) is in bit-reversed order: slot i holds the value at
 *                  omega_n^rev_m(i).  The coefficient side is always in natural order.  With the flag no permutation is made (forward:
 *                  decimation in frequency, inverse: decimation in time); without it the last store permutes.
 *   in32 / out32   k x n 32-byte little-endian images; vector g is images [g n, (g + 1) n) - the layout fr_open_many and the MSM calls read.
 *                  ANY 256-bit input image acts as its value mod r; every output image is in [0, r).
 *   shift32        ONE image in HOST memory in both forms, shared by the k vectors, acting as its value mod r; NULL: g = 1.
 *   status         k bytes, HOST memory, may be NULL: bit 1 (2) an image of this vector was >= r and was reduced (informational; the shift sets
 *                  no bit).  Returns the number of such vectors; k == 0: 0, nothing touched.  n == 1 is the identity up to reduction.
 *   IN PLACE       d_out32 == d_in32 exactly is allowed in the _device form; any other overlap is a precondition violation.
 * MI355_BLS_ERR_ARG, before anything is launched: a NULL context (before the k == 0 rule), NULL in or out, n == 0, n that is no power of two or
 * above 2^32, an unknown flag bit, a shift that is 0 mod r, a misaligned device pointer (4-byte aligned; 16-byte aligned ones are read and
 * written 16 bytes at a time), a busy context.  Nothing else is refused for its size: k x n beyond one slice is cut into slices of whole
 * vectors (csrc/plan.hpp frntt_sizes_for); the _device form enqueues on `stream` and synchronises it once per slice, for the status bytes.
 * A transform whose last store permutes and that is longer than a tile uses a library buffer of one slice.
 * The m radix-2 stages run in passes of at most `tile` stages with their elements in LDS (csrc/frntt.hpp; one twiddle table per call).
 * fr_domain writes omega_n^i, or omega_n^rev_m(i) with MI355_BLS_FR_NTT_BITREV (no other flag), as n canonical images: a valid domain32
 * argument of mi355_bls_fr_open_many.  Both forms return when the images are written.
 * VARIABLE TIME: public vectors only.
 * COST: profiles/fr_ntt_bench.json (nim-blscurve_amd/tools/bench_fr_ntt.py), reported row by row in README.md.
 * debug_frntt_set_tile: TEST HOOK, log2 of the tile of the following fr_ntt_many calls on this context (0: the plan's own; it can only shrink
 * the tile below the largest one a workgroup's LDS holds, 2^12 elements).  debug_frntt_set_pass: the vectors per slice (0: the plan's own; it
 * can only shorten a slice). */
#define MI355_BLS_FR_NTT_INVERSE 1u
#define MI355_BLS_FR_NTT_BITREV 2u
int mi355_bls_fr_ntt_many(mi355_bls_ctx* ctx, const void* in32, size_t n, size_t k, uint32_t flags, const uint8_t* shift32, uint8_t* out32,
                          uint8_t* status);
int mi355_bls_fr_ntt_many_device(mi355_bls_ctx* ctx, const void* d_in32, size_t n, size_t k, uint32_t flags, const uint8_t* shift32,
                                 void* d_out32, uint8_t* status, void* stream);
int mi355_bls_fr_domain(mi355_bls_ctx* ctx, size_t n, uint32_t flags, uint8_t* out32);
int mi355_bls_fr_domain_device(mi355_bls_ctx* ctx, size_t n, uint32_t flags, void* d_out32, void* stream);
int mi355_bls_debug_frntt_set_tile(mi355_bls_ctx* ctx, uint32_t log2_tile);
int mi355_bls_debug_frntt_set_pass(mi355_bls_ctx* ctx, size_t vectors_per_pass);

/* Number-theoretic transforms of k vectors of G1 POINTS in one device pass: what mi355_bls_fr_ntt_many does to scalars, done to points.  The
 * inverse transform of the monomial table [tau^j]G is the Lagrange table that commits to values (mi355_bls_fr_open_many's evaluation form);
 * the forward transform is the last step of an all-openings (FK20-style) computation.
 *   omega_n, rev_m and both flags are mi355_bls_fr_ntt_many's: n = 2^m, 0 <= m <= 32, omega_n = 7^((r - 1) / n) mod r.
 *   FORWARD  out[i] = sum_j [omega_n^(i j)] P_j.
 *   MI355_BLS_P1S_NTT_INVERSE  the exact inverse map: [1 / n] sum_i [omega_n^(-i j)] P_i.
 *   MI355_BLS_P1S_NTT_BITREV   the EVALUATION side (the forward output, the inverse input) is in bit-reversed order; with the flag no
 *                  permutation is made, without it the last store permutes.
 *   So for P_j = [a_j]G the result is [fr_ntt(a)_i]G under the same flags.  There is no coset shift.
 *   points96       k x n 96-byte blst_p1_affine images; vector g is images [g n, (g + 1) n); the all-zero image is infinity.  The points
 *                  must be in G1, the prime-order subgroup: this is NOT checked - with other points the outputs mean nothing, but nothing faults.
 *   out96          k x n canonical affine images in the same form, all zero: infinity - what p1s_lincomb_many writes and every consumer reads.
 *   IN PLACE       d_out96 == d_points96 exactly is allowed in the _device form; any other overlap is a precondition violation.
 * Returns 0; k == 0: 0, nothing touched.  n == 1 is the canonicalising copy.
 * MI355_BLS_ERR_ARG, before anything is launched: a NULL context (before the k == 0 rule), NULL points or output, n == 0, n that is no power
 * of two or above 2^32, an unknown flag bit, a misaligned device pointer (4-byte aligned), a busy context.  Nothing else is refused for its
 * size: k x n beyond one slice is cut into slices of whole vectors, and one vector always forms a slice (csrc/plan.hpp p1ntt_sizes_for; the
 * workspace is the library's own: 192 bytes per point of a slice).  The _device form enqueues on `stream` and waits for it once at the end.
 * The m radix-2 stages run over global memory, one lane per butterfly (csrc/p1ntt.hpp): a butterfly is a 255-bit scalar multiplication by
 * signed 4-bit windows, except where its twiddle is 1; the inverse's 1 / n is folded into one stage.
 * VARIABLE TIME: public points only.
 * COST: profiles/p1s_ntt_bench.json (nim-blscurve_amd/tools/bench_p1s_ntt.py), reported row by row in README.md.
 * debug_p1ntt_set_pass: TEST HOOK, the vectors per slice of the following p1s_ntt_many calls on this context (0: the plan's own; it can only
 * shorten a slice). */
#define MI355_BLS_P1S_NTT_INVERSE 1u
#define MI355_BLS_P1S_NTT_BITREV 2u
int mi355_bls_p1s_ntt_many(mi355_bls_ctx* ctx, const void* points96, size_t n, size_t k, uint32_t flags, void* out96);
int mi355_bls_p1s_ntt_many_device(mi355_bls_ctx* ctx, const void* d_points96, size_t n, size_t k, uint32_t flags, void* d_out96, void* stream);
int mi355_bls_debug_p1ntt_set_pass(mi355_bls_ctx* ctx, size_t vectors_per_pass);

/* ALL n openings of each of k polynomials over the n-th roots of unity in one device pass (the Feist-Khovratovich route, "FK20", over G1):
 * O(n log n) scalar multiplications per polynomial where mi355_bls_fr_open_many over the whole domain followed by n MSMs needs n^2.
 *   DEFINITION, for ANY G1 points S_0 .. S_(n-1), n = 2^m, 0 <= m <= 31, coefficients c_0 .. c_(n-1) and mi355_bls_fr_ntt_many's omega_n:
 *       h_t  = sum_{i=0}^{n-2-t} [c_(i+t+1)] S_i     t = 0 .. n-2,   h_(n-1) = infinity
 *       pi_l = sum_{t=0}^{n-1} [omega_n^(l t)] h_t   l = 0 .. n-1
 *   For an SRS S_j = [tau^j]G, pi_l is the commitment to (p(X) - p(omega_n^l)) / (X - omega_n^l): the KZG proof at z = omega_n^l, what
 *   mi355_bls_fr_open_many followed by an MSM over the SRS gives for that z.
 *   THE SETUP is a library-owned handle in device memory, 2n x 96 bytes (mi355_bls_fk20_setup_sizeof; 0 for an n that create refuses): the
 *   transform of length 2n of the reversed, zero-extended setup points as affine images in bit-reversed order.  Creating it is one
 *   mi355_bls_p1s_ntt_many-style transform of 2n points.  srs96: n 96-byte blst_p1_affine images, all zero: infinity; the points must be in
 *   G1, which is NOT checked.  Ownership, device and lifetime are mi355_bls_p1s_table's: the handle belongs to its caller, not to the context
 *   that made it, any context of the same device may use it, and mi355_bls_fk20_setup_destroy releases it (NULL: no-op).
 *   polys32        k x n 32-byte little-endian coefficient images, polynomial g at [g n, (g + 1) n).  An image >= r acts as its value mod r
 *                  and is reported as mi355_bls_fr_ntt_many reports it: status[g] bit 1 (value 2), and the return value counts such g.
 *   out96          k x n canonical affine images; image g n + l is pi_l of polynomial g; all zero: infinity.
 *   status         k bytes, or NULL.
 *   MI355_BLS_FK20_BITREV   the proofs in bit-reversed order (slot l holds pi_rev_m(l)), MI355_BLS_P1S_NTT_BITREV's meaning: no permutation
 *                  is made.
 *   MI355_BLS_FK20_H        write h_0 .. h_(n-1) in natural order instead of the proofs, stopping before the last transform: for the caller
 *                  who wants the proofs on a larger domain (transform h there).  MI355_BLS_FK20_BITREV changes nothing beside it.
 * Returns the number of polynomials with status bit 1; k == 0: 0, nothing touched.  n == 1 is legal: every output is infinity.
 * MI355_BLS_ERR_ARG, before anything is launched: a NULL context (before the k == 0 rule), a NULL setup, polynomials, output or (create)
 * srs96 / handle pointer, n == 0, n that is no power of two or above 2^31 (the transform of 2n points must fit mi355_bls_p1s_ntt_many's
 * bound), an unknown flag bit, a setup of another device, a misaligned device pointer (4-byte aligned), a busy context.  Nothing is refused
 * for its size: k beyond one pass runs as passes of whole polynomials, and one polynomial always forms a pass (csrc/plan.hpp fk20_sizes_for:
 * 448 n bytes of the library's workspace per polynomial of a pass, 256 MiB per pass, not tuned).  The _device forms enqueue on `stream`;
 * open_all waits for it once per pass (the status words), create once at the end.
 * The route (csrc/fk20.hpp): the coefficients laid out as a circulant's first column and scaled by 1 / (2n), one Fr transform of length 2n,
 * a scalar multiplication per element of the setup, the inverse point transform of length 2n and the forward one of length n with no affine
 * image in between: 2m + 2 dependent 255-bit multiplications deep, whatever k.
 * VARIABLE TIME: public polynomials only.
 * COST: profiles/fk20_bench.json (nim-blscurve_amd/tools/bench_fk20.py), reported row by row in README.md.
 * debug_fk20_set_pass: TEST HOOK, the polynomials per pass of the following fk20_open_all_many calls on this context (0: the plan's own; it
 * can only shorten a pass). */
#define MI355_BLS_FK20_BITREV 2u
#define MI355_BLS_FK20_H 4u
typedef struct mi355_bls_fk20_setup mi355_bls_fk20_setup;
size_t mi355_bls_fk20_setup_sizeof(size_t n);
int mi355_bls_fk20_setup_create(mi355_bls_ctx* ctx, mi355_bls_fk20_setup** out, const void* srs96, size_t n);
int mi355_bls_fk20_setup_create_device(mi355_bls_ctx* ctx, mi355_bls_fk20_setup** out, const void* d_srs96, size_t n, void* stream);
void mi355_bls_fk20_setup_destroy(mi355_bls_fk20_setup* setup);
int mi355_bls_fk20_open_all_many(mi355_bls_ctx* ctx, const mi355_bls_fk20_setup* setup, const void* polys32, size_t k, uint32_t flags, void* out96, uint8_t* status);
int mi355_bls_fk20_open_all_many_device(mi355_bls_ctx* ctx, const mi355_bls_fk20_setup* setup, const void* d_polys32, size_t k, uint32_t flags, void* d_out96,
                                        uint8_t* status, void* stream);
int mi355_bls_debug_fk20_set_pass(mi355_bls_ctx* ctx, size_t polys_per_pass);

/* The proofs of ALL CELLS of each of k polynomials in one device pass (the Feist-Khovratovich route over cosets): a cell is a coset of
 * l = `cell` evaluation points of a domain that may be larger than the polynomial - PeerDAS: n = 4 096 coefficients, cell = 64, ext_log2 = 1,
 * 128 cells on the domain of 8 192.  One proof per cell where the definition route divides by X^l - a on the host and runs an MSM of about n
 * points per cell.
 *   DEFINITION, for ANY G1 points S_0 .. S_(n-1), n = 2^m, 0 <= m <= 31, coefficients c_0 .. c_(n-1), l = 2^c with 1 <= l <= n, q = n / l,
 *   N = q 2^ext_log2 cells with n 2^ext_log2 <= 2^32, and mi355_bls_fr_ntt_many's omega_N:
 *       h_s  = sum_{i=0}^{n-1-l(s+1)} [c_(i + l(s+1))] S_i     s = 0 .. q-2,   h_(q-1) = infinity
 *       pi_j = sum_{s=0}^{q-1} [omega_N^(j s)] h_s              j = 0 .. N-1
 *   For an SRS S_i = [tau^i]G, pi_j is the commitment to the polynomial quotient p(X) div (X^l - omega_N^j): the KZG multi-proof for the
 *   coset {x : x^l = omega_N^j} = {omega_(l N)^(j + N u), u < l} of the domain of n 2^ext_log2 points.  cell == 1 and ext_log2 == 0 is
 *   mi355_bls_fk20_open_all_many's definition, and the outputs are the same bytes.
 *   THE SETUP is the same handle type, made by mi355_bls_fk20_setup_create_cells for ONE cell size: the l transforms of length 2q of the
 *   reversed, zero-extended sub-setups S_(l u + v), 2n x 96 bytes as before (mi355_bls_fk20_setup_sizeof), the l images of a slot adjacent.
 *   Creating a handle with cell > 1 takes a second 2n x 96 bytes of device memory, released before create returns: twice the handle at peak.
 *   cell == 1 gives mi355_bls_fk20_setup_create's handle, byte for byte.  Ownership, device, lifetime and destroy are unchanged.  A handle
 *   made with cell > 1 serves mi355_bls_fk20_open_cells_many only: mi355_bls_fk20_open_all_many refuses it.  The points must be in G1, which
 *   is NOT checked.
 *   polys32        k x n 32-byte little-endian coefficient images; an image >= r acts as its value mod r: status[g] bit 1 (value 2), and
 *                  the return value counts such g, as in mi355_bls_fk20_open_all_many.
 *   out96          k x N canonical affine images; image g N + j is pi_j of polynomial g; all zero: infinity.
 *   MI355_BLS_FK20_BITREV   slot j holds pi_rev(j), rev over log2 N bits; no permutation is made.  For n = 4 096, cell = 64, ext_log2 = 1 this
 *                  is PeerDAS' cell order: cell i of the bit-reversed extended evaluation is the coset x^64 = omega_128^rev7(i).
 *   MI355_BLS_FK20_H        out96 is k x q images h_0 .. h_(q-1) in natural order, stopping before the last transform; ext_log2 is still
 *                  validated.  MI355_BLS_FK20_BITREV changes nothing beside it.
 * Returns the number of polynomials with status bit 1; k == 0: 0, nothing touched.  cell == n is legal (q = 1: every output is infinity), and
 * so is n == 1.
 * MI355_BLS_ERR_ARG, before anything is launched: what mi355_bls_fk20_open_all_many refuses (a NULL context before the k == 0 rule, a NULL
 * setup, polynomials, output or (create) srs96 / handle pointer, n == 0, n that is no power of two or above 2^31, an unknown flag bit, a
 * setup of another device, a misaligned device pointer, a busy context); (create) a cell that is 0, no power of two or above n; ext_log2
 * with n 2^ext_log2 > 2^32.  Nothing is refused for its size: passes of whole polynomials under the same bound (csrc/plan.hpp
 * fk20_cells_sizes_for: 448 n + 192 max(2q, N) bytes of the library's workspace per polynomial), one polynomial always forms a pass, and
 * mi355_bls_debug_fk20_set_pass shortens these passes too.  The _device forms enqueue on `stream`; open_cells waits for it once per pass,
 * create at the end.
 * The route (csrc/fk20cells.hpp): l Fr transforms of length 2q per polynomial, a scalar multiplication per element of the setup (2n), an
 * l-fold sum per slot, ONE inverse point transform of length 2q and the forward one of length N: log2(2q) + log2 N + 1 dependent 255-bit
 * multiplications deep, whatever k and l.
 * VARIABLE TIME: public polynomials only.
 * COST: profiles/fk20_cells_bench.json (nim-blscurve_amd/tools/bench_fk20_cells.py), reported row by row in README.md. */
int mi355_bls_fk20_setup_create_cells(mi355_bls_ctx* ctx, mi355_bls_fk20_setup** out, const void* srs96, size_t n, size_t cell);
int mi355_bls_fk20_setup_create_cells_device(mi355_bls_ctx* ctx, mi355_bls_fk20_setup** out, const void* d_srs96, size_t n, size_t cell, void* stream);
int mi355_bls_fk20_open_cells_many(mi355_bls_ctx* ctx, const mi355_bls_fk20_setup* setup, const void* polys32, size_t k, size_t ext_log2, uint32_t flags, void* out96,
                                   uint8_t* status);
int mi355_bls_fk20_open_cells_many_device(mi355_bls_ctx* ctx, const mi355_bls_fk20_setup* setup, const void* d_polys32, size_t k, size_t ext_log2, uint32_t flags,
                                          void* d_out96, uint8_t* status, void* stream);

/* Fixed-base G1 MSM over a precomputed window table: blst_p1s_mult_wbits_precompute(_sizeof) and blst_p1s_mult_wbits (blst_abi.nim:327-335)
 * for callers whose point set does not change - k commitments over one SRS or Lagrange table.  A table is a library-owned handle that keeps, in
 * device memory, the rows [2^(w wbits)] P_i for w = 0 .. W - 1, W = ceil((nbits + 1) / wbits), W x npoints x 128 bytes
 * (mi355_bls_p1s_table_sizeof), and carries its parameters.  An MSM is then sum_i sum_w d_(i,w) T[w][i] over the signed wbits-bit digits d of
 * the scalars: no window needs a doubling chain, and the W windows of an MSM share S <= W bucket sets (csrc/plan.hpp fixed_for), so the
 * reductions shrink by W / S.  Points, scalars, nbits and results mean what they mean in mi355_bls_p1s_mult_pippenger_device: 96-byte
 * blst_p1_affine images (all-zero = infinity, contributes nothing; subgroup membership is not assumed), 32-byte little-endian scalar images of
 * which the low nbits count, nbits in 1..256, results blst_p1 (Jacobian, 144 B), an infinite one 144 zero bytes; compare results as points.
 *   wbits     5 .. 16 (at least one 16-bucket segment, at most 2^15 buckets per set), or 0: the plan chooses from npoints (8 below 2^14 points,
 *             16 from there on: csrc/plan.hpp fixed_wbits_for).  Choose a width that leaves the top window, (nbits + 1) - (W - 1) wbits bits, about as
 *             wide as the others: a narrow one crowds every point into its few buckets (12-bit windows on 255-bit scalars: 4x slower than the generic call).
 *             Windows are uniform; digits are the signed digits of the Pippenger sort over nbits + 1 bits.
 *   reuse     a table made for nbits serves every mult call with nbits at most the table's; a larger nbits is MI355_BLS_ERR_ARG.  The table is
 *             memory of the creating context's device and usable through any context on that device: the ctx of a mult call supplies
 *             workspace and streams only.  Destroying the context that made a table does not free it; mi355_bls_p1s_table_destroy does
 *             (NULL: a no-op).
 *   _create / _mult_table / _mult_table_many          host arrays (contiguous), staged and run on the null stream
 *   _create_device / _mult_table(_many)_device        arrays in device memory; everything is enqueued on `stream` and waited for once
 *   _many     k MSMs over the one table - the shared-base form of mi355_bls_p1s_mult_pippenger_many: scalars k x npoints x 32 bytes, MSM j uses
 *             [j npoints, (j + 1) npoints); results to ret (host, k x 144 B, may be NULL in the device form) and / or d_out (device, 4-byte
 *             aligned, may be NULL).  k == 0 returns 0 and touches nothing; k == 1 is the single call.
 * MI355_BLS_ERR_ARG, before anything is launched: NULL arguments, npoints == 0 at create, wbits outside {0, 5..16}, nbits outside 1..256, more
 * than 2^31 table entries (W x npoints; csrc/plan.hpp FIXED_ENTRIES_MAX: a sorted index word names an entry in 31 bits beside the digit's sign),
 * a table of another device.  No other call is refused for its size: a call beyond one pass runs as consecutive passes over ranges of MSMs
 * inside the library.  Variable time, like every MSM here.
 * Cost (one MI355X, device-resident, 255 bits, median of 5 blocking calls, against the generic call in the same run, the plan's own wbits;
 * nim-blscurve_amd/tools/bench_msm_table.py, profiles/msm_table_bench.json): FASTER at 4 096 points (0.99 against 1.34 ms), at 2^16 (1.14
 * against 1.58) and for k = 8 / 64 / 512 MSMs over 4 096 points (1.09 / 2.45 / 14.5 against 1.42 / 2.64 / 17.9 ms); SLOWER at 2^20 points (5.00
 * against 4.36 ms).  Create: 2.1 - 2.6 ms up to 2^16 points, 28 ms at 2^20 (2 GB); paid for after 5 - 12 uses where the call wins. */
typedef struct mi355_bls_p1s_table mi355_bls_p1s_table;
size_t mi355_bls_p1s_table_sizeof(size_t npoints, size_t wbits, size_t nbits);      /* device bytes a table takes; 0 for arguments create refuses */
int mi355_bls_p1s_table_create(mi355_bls_ctx* ctx, mi355_bls_p1s_table** out, const void* points96, size_t npoints, size_t wbits, size_t nbits);
int mi355_bls_p1s_table_create_device(mi355_bls_ctx* ctx, mi355_bls_p1s_table** out, const void* d_points96, size_t npoints, size_t wbits, size_t nbits,
                                      void* stream);
void mi355_bls_p1s_table_destroy(mi355_bls_p1s_table* tab);
int mi355_bls_p1s_mult_table(mi355_bls_ctx* ctx, uint8_t ret_p1[144], const mi355_bls_p1s_table* tab, const void* scalars32, size_t nbits);
int mi355_bls_p1s_mult_table_device(mi355_bls_ctx* ctx, uint8_t ret_p1[144], const mi355_bls_p1s_table* tab, const void* d_scalars32, size_t nbits,
                                    void* stream);
int mi355_bls_p1s_mult_table_many(mi355_bls_ctx* ctx, uint8_t* ret, const mi355_bls_p1s_table* tab, const void* scalars32, size_t k, size_t nbits);
int mi355_bls_p1s_mult_table_many_device(mi355_bls_ctx* ctx, uint8_t* ret, void* d_out, const mi355_bls_p1s_table* tab, const void* d_scalars32, size_t k,
                                         size_t nbits, void* stream);
/* TEST HOOKS: rows [w0, w0 + nw) x points [i0, i0 + ni) of the table as 96-byte blst_p1_affine images (all-zero = infinity), row-major; the
 * (W, S, buckets per set) the last mult call on this context ran with; and the plan's parameters for the following mult calls on this context:
 * force_sets bucket sets per MSM (capped at W) and at most pairs_max (point, scalar) pairs per pass beyond a pass's first MSM (0: the plan's own). */
int mi355_bls_debug_p1s_table_rows(const mi355_bls_p1s_table* tab, size_t w0, size_t nw, size_t i0, size_t ni, uint8_t* out96);
int mi355_bls_debug_p1s_table_last_plan(mi355_bls_ctx* ctx, uint32_t out[3]);
int mi355_bls_debug_p1s_table_set_plan(mi355_bls_ctx* ctx, uint32_t force_sets, uint32_t pairs_max);

/* Point-sharded MSM across the GPUs of one node (blst_p1s_mult_pippenger, blst_abi.nim:336-340, over devices; the bench shape
 * benchmarks/bls12381_msm_g1.nim:47-59): device g computes the full-width partial sum of points [first_g, first_g + count_g)
 * (mi355_bls_msm_shard_range: balanced contiguous blocks), the 144-byte partials are added (blst_p1_add_or_double,
 * blst_abi.nim:278).
 *   _multi         one host thread, ctxs[g] on device g, host arrays as mi355_bls_p1s_mult_pippenger (32-byte scalar images);
 *                  all shards are enqueued before any is waited for, ctxs[0] adds the partials
 *   _multi_device  d_points[g] / d_scalars[g] = shard g's arrays already resident on device g
 *   _partial_device + p1s_add(_device)   one process per GPU: every rank leaves its partial in device memory (the send buffer
 *                  of an RCCL all_gather), rank 0 adds the gathered partials (k x stride_bytes in device memory, or k x 144 B in
 *                  host memory) */
void mi355_bls_msm_shard_range(size_t npoints, uint32_t world, uint32_t rank, size_t* first, size_t* count);
int mi355_bls_p1s_mult_pippenger_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, uint8_t ret_p1[144], const void* const points[], size_t npoints,
                                       const uint8_t* const scalars[], size_t nbits);
int mi355_bls_p2s_mult_pippenger_multi(mi355_bls_ctx* const ctxs[], size_t ngpu, uint8_t ret_p2[288], const void* const points[], size_t npoints,
                                       const uint8_t* const scalars[], size_t nbits);
int mi355_bls_p1s_mult_pippenger_multi_device(mi355_bls_ctx* const ctxs[], size_t ngpu, uint8_t ret_p1[144], const void* const d_points[], size_t npoints,
                                              const void* const d_scalars[], size_t nbits);
int mi355_bls_p1s_mult_pippenger_partial_device(mi355_bls_ctx* ctx, void* d_out_p1, const void* d_points, size_t npoints, const void* d_scalars,
                                                size_t nbits, void* stream);
int mi355_bls_p1s_add(mi355_bls_ctx* ctx, uint8_t ret_p1[144], const uint8_t* parts, size_t k);
int mi355_bls_p2s_add(mi355_bls_ctx* ctx, uint8_t ret_p2[288], const uint8_t* parts, size_t k);
int mi355_bls_p1s_add_device(mi355_bls_ctx* ctx, uint8_t ret_p1[144], const void* d_parts, size_t k, size_t stride_bytes, void* stream);

/* Batched PublicKey.fromBytes / Signature.fromBytes (blscurve/blst/bls_sig_io.nim:42-58, 81-99) on the device:
 * n compressed public keys (48 B each), 32-byte messages and compressed signatures (96 B each), ZCash format.
 * Per tuple: blst_p1_uncompress, "public key is not infinity", blst_p1_affine_in_g1, blst_p2_uncompress,
 * blst_p2_affine_in_g2 (an infinity signature is allowed).  status[i] (optional, n bytes): 0 ok, 1 bad pk
 * encoding / x >= p / not on the curve, 2 pk not in G1, 3 pk infinity, 4 bad sig encoding, 5 sig not in G2.
 * out_sets (optional): n x 320-byte SignatureSet records (failed tuples are zeroed).
 * Returns 1 when every tuple deserialised, 0 when some did not, negative on runtime failure. */
int mi355_bls_deserialize_sets(mi355_bls_ctx* ctx, const uint8_t* pks48, const uint8_t* msgs32, const uint8_t* sigs96, size_t n,
                               void* out_sets, uint8_t* status);
int mi355_bls_deserialize_sets_device(mi355_bls_ctx* ctx, const void* d_pks48, const void* d_msgs32, const void* d_sigs96, size_t n,
                                      void* stream, void* out_sets, uint8_t* status);

/* The other forms of fromBytes (bls_sig_io.nim:42-121), selected per side by `flags`:
 *   MI355_BLS_DESER_PK_UNCOMPRESSED   keys are 96-byte images   -> blst_p1_deserialize (:88-91)
 *   MI355_BLS_DESER_SIG_UNCOMPRESSED  signatures are 192-byte images -> blst_p2_deserialize (:49-52)
 *   MI355_BLS_DESER_KNOWN_ON_CURVE    fromBytesKnownOnCurve (:60-79, :101-121): no subgroup checks (the infinity public key is
 *                                     still rejected)
 * blst_pN_deserialize [blst-upstream]: top bits of byte 0 = 000 uncompressed big-endian coordinates (G2: x.c1, x.c0, y.c1, y.c0),
 * each < p, point on the curve; 1xx a compressed encoding in the first half; 01x infinity (0x40 followed by zeros only).
 * pks: n x 48 or 96 bytes, sigs: n x 96 or 192 bytes; status codes and results as mi355_bls_deserialize_sets. */
#define MI355_BLS_DESER_PK_UNCOMPRESSED 1u
#define MI355_BLS_DESER_SIG_UNCOMPRESSED 2u
#define MI355_BLS_DESER_KNOWN_ON_CURVE 4u
int mi355_bls_deserialize_sets_ex(mi355_bls_ctx* ctx, const uint8_t* pks, const uint8_t* msgs32, const uint8_t* sigs, size_t n, uint32_t flags,
                                  void* out_sets, uint8_t* status);
int mi355_bls_deserialize_sets_ex_device(mi355_bls_ctx* ctx, const void* d_pks, const void* d_msgs32, const void* d_sigs, size_t n, uint32_t flags,
                                         void* stream, void* out_sets, uint8_t* status);

/* fromBytes for every tuple followed by batchVerify (bls_batch_verifier.nim:420-495), all on the device:
 * the wire format (176 B per tuple) is the only thing that crosses PCIe.  Returns 0 if any tuple fails to
 * deserialise (the caller would not have obtained a SignatureSet) or the batch does not verify. */
int mi355_bls_batch_verify_compressed(mi355_bls_ctx* ctx, const uint8_t* pks48, const uint8_t* msgs32, const uint8_t* sigs96, size_t n,
                                      const uint8_t rnd[32], uint8_t* status);
int mi355_bls_batch_verify_compressed_device(mi355_bls_ctx* ctx, const void* d_pks48, const void* d_msgs32, const void* d_sigs96, size_t n,
                                             const uint8_t rnd[32], void* stream, uint8_t* status);
float mi355_bls_last_deser_ms(mi355_bls_ctx* ctx);   /* duration of the deserialisation kernel of the last compressed call */

/* combine(secureRandomBytes, publicKeys, signatures) (blst_min_pubkey_sig_core.nim:570-647; called by
 * MultiSignatureSet.combine, bls_batch_verifier.nim:100-106): linear combination of n signatures on ONE message.
 * Scalars: chain seeded with rnd itself, taking the u64 words 3,2,1,0 of each SHA-256 output, zeros skipped
 * (:588-606); out_pk = sum [s_i]PK_i and out_sig = sum [s_i]S_i as affine BLST images: two 64-bit Pippenger runs on the
 * device (G1 and G2 bucket kernels, the reference's blst_p1s/p2s_mult_pippenger calls, :629-646) + finish.  The scalar chain
 * is sequential SHA-256: it runs on the calling host thread.  n == 1: passthrough; n == 0: MI355_BLS_ERR_ARG (the reference asserts).
 * pks: n x 96 B, sigs: n x 192 B, host memory.  Returns 0 on success. */
int mi355_bls_combine(mi355_bls_ctx* ctx, const uint8_t rnd[32], const void* pks, const void* sigs, size_t n, uint8_t out_pk[96],
                      uint8_t out_sig[192]);
/* combine for MANY groups in ONE device pass: k groups of SignatureSet records that carry the same message (gossip: hundreds of
 * unaggregated attestations per message) become k ordinary 320-byte records, so that hashing, cofactor clearing and the Miller lines of a
 * following batchVerify run once per message instead of once per signature.  mi355_bls_combine stays the call for one huge group.
 *   sets      n_sets x 320-byte SignatureSet records: the member table
 *   idx       NULL: group g is records [offsets[g], offsets[g+1]) of the table itself (offsets[k] <= n_sets);
 *             else: group g is records idx[offsets[g]] .. idx[offsets[g+1] - 1] (offsets[k] = the length of idx; repeats allowed)
 *   offsets   k + 1 entries in HOST memory (also in the _device forms), non-decreasing
 *   rnds      k x 32 bytes in HOST memory (also in the _device forms): secureRandomBytes of every group
 *   status    k bytes, host memory: 0 ok, 1 empty group (the reference asserts), 2 the combined key is the point at infinity, 3 an index was
 *             >= n_sets (it is never dereferenced), 4 the members' messages are not all equal (the combination would be unsound), 5 a
 *             member's public key is the infinity image (the reference assumes there is none); precedence 3 > 4 > 5 > 1 > 2.  The record
 *             of a group whose status is not 0 carries the infinity key (96 zero bytes), for which every verifier answers 0, and the
 *             infinity signature.
 * Record g is byte for byte the reference's combine(rnds[g], pks_g, sigs_g) with the first member's message: for L >= 2 members the scalars
 * s_0 .. s_(L-1) of the chain seeded with rnds[g] (as mi355_bls_combine draws them) in list order, key = affine(sum [s_j]PK_j), signature =
 * affine(sum [s_j]S_j) (192 zero bytes if that is infinity; an infinity signature among the members adds nothing); L == 1: the member's
 * record, no scalar drawn.  The chain is per group: a record depends neither on the group's position nor on how its members are addressed.
 * At most 2^26 members per call; nothing is bounded by max_sets.  Device pointers are 4-byte aligned.  The scalars and the random bytes are
 * cleared from device memory before a call returns.
 * Measured on one MI355X, 65 536 members (profiles/combine_sets_bench.json): combine_sets_device alone takes 4.2 - 5.6 ms for groups of 2 to
 * 512; batch_verify_combined_device end to end against mi355_bls_batch_verify_device over the uncombined sets: groups of 4: 11.4 against
 * 12.3 ms, 16: 7.4 against 12.3, 64: 7.7 against 11.8, 512: 7.7 against 11.8.  At groups of 2 the combined route LOSES (14.2 against
 * 12.3 ms): send such batches through batch_verify as they are.
 * combine_sets:  returns 1 when every status is 0, else 0; k == 0: 0, nothing written.  MI355_BLS_ERR_ARG for decreasing offsets, offsets[k] >
 *                n_sets without idx, NULL pointers.  The _device form enqueues on `stream` (and the context's fork stream) and synchronises
 *                once, for the status bytes; d_out_records: k x 320 bytes of device memory.
 * batch_verify_combined:  combine_sets, then - if every status is 0 - mi355_bls_batch_verify with rnd over the k records; any other status: 0
 *                and no verification pass.
 * group_by_message:  host only, no GPU.  Groups the n records of a flat batch by their 32-byte message, stably: groups in the order their
 *                message first appears, members in input order.  idx: n entries, offsets: room for n + 1 of which *k + 1 are written. */
int mi355_bls_combine_sets(mi355_bls_ctx* ctx, const void* sets, size_t n_sets, const uint32_t* idx, const size_t* offsets, size_t k,
                           const uint8_t* rnds, void* out_records, uint8_t* status);
int mi355_bls_combine_sets_device(mi355_bls_ctx* ctx, const void* d_sets, size_t n_sets, const uint32_t* d_idx, const size_t* offsets, size_t k,
                                  const uint8_t* rnds, void* d_out_records, uint8_t* status, void* stream);
int mi355_bls_batch_verify_combined(mi355_bls_ctx* ctx, const void* sets, size_t n_sets, const uint32_t* idx, const size_t* offsets, size_t k,
                                    const uint8_t* rnds, const uint8_t rnd[32]);
int mi355_bls_batch_verify_combined_device(mi355_bls_ctx* ctx, const void* d_sets, size_t n_sets, const uint32_t* d_idx, const size_t* offsets,
                                           size_t k, const uint8_t* rnds, const uint8_t rnd[32], void* stream);
int mi355_bls_group_by_message(const void* sets, size_t n, uint32_t* idx, size_t* offsets, size_t* k);

/* batchVerify BY MESSAGE: mi355_bls_batch_verify's arguments, scalars, verdict and final value, with hashing and the Miller loop run once per
 * DISTINCT message of a slice.  The sets that share a 32-byte message are found on the device (an open-addressing table of set indices, all
 * 32 bytes compared; csrc/bymsg.hpp), and because e([r_1]PK_1, H(m)) e([r_2]PK_2, H(m)) = e([r_1]PK_1 + [r_2]PK_2, H(m)) the blinded keys of
 * a group are summed into ONE Miller pair.  Set i gets exactly the scalar mi355_bls_batch_verify gives it (same chains, same dispatch), the
 * signature side is that call's, and the value after the final exponentiation is the same field element: the return value and
 * mi355_bls_fetch_stage(4) equal mi355_bls_batch_verify's for every input (n == 0: 0; an infinity key: 0).  A group whose summed key is the
 * point at infinity contributes the factor 1 and does not fail the batch.  Unlike batch_verify_combined it needs no grouping from the host,
 * no second set of scalars and no G2 multiplication per member.
 * Any n: a batch beyond max_sets runs in slices cut where mi355_bls_batch_verify cuts them, one after the other; a group that a boundary cuts
 * is two groups.  A slice whose messages are all distinct runs the ordinary pass.  Blocking (the call waits twice per slice for a few words:
 * the number of groups and their offsets); there is no submit / wait, sharded or multi-device form.
 * Stages after the call (last slice): 0 = r_i, n x 8 bytes; 1 = H(m_g) of the k distinct messages in the order each first appears
 * (mi355_bls_group_by_message's group order); 2 = the k group sums as Jacobian images (compare them as points: the order of additions inside
 * a group is free); 3, 4, 5 as after mi355_bls_batch_verify.
 * by_message_device: d_sets in device memory (4-byte aligned), kernels on `stream` and the context's fork streams.
 * last_message_groups: k of the last such call's last slice; MI355_BLS_ERR_ARG before the first one.
 * debug_..._scalars: TEST HOOK, mi355_bls_debug_batch_verify_scalars' contract (serial, one slice, host memory, r[i] != 0) for this pass. */
int mi355_bls_batch_verify_by_message(mi355_bls_ctx* ctx, const void* sets, size_t n, const uint8_t rnd[32]);
int mi355_bls_batch_verify_by_message_device(mi355_bls_ctx* ctx, const void* d_sets, size_t n, const uint8_t rnd[32], void* stream);
int mi355_bls_last_message_groups(mi355_bls_ctx* ctx);
int mi355_bls_debug_batch_verify_by_message_scalars(mi355_bls_ctx* ctx, const void* sets, size_t n, const uint64_t r[]);

/* aggregateVerify(publicKeys, messages, signature) (bls_sig_min_pubkey.nim:153-199; ContextCoreAggregateVerify,
 * blst_min_pubkey_sig_core.nim:305-414): e(G1, sig) == prod_i e(pk_i, H(m_i)) for n (public key, message) pairs
 * with messages of arbitrary length: message i = msgs[msg_offsets[i] .. msg_offsets[i+1]) (n + 1 offsets).
 * pks: n x 96 B, sig: 192 B, host memory.  n == 0 -> 0; infinity public key -> 0.  The proofs of possession
 * must have been checked by the caller, as for the reference's two-argument overloads.  Any n: inputs beyond the
 * context's capacity are processed in slices.  A single message must fit the context's staging buffer (max_sets * 320 - 104
 * bytes), else MI355_BLS_ERR_CAPACITY. */
int mi355_bls_aggregate_verify(mi355_bls_ctx* ctx, const void* pks, const uint8_t* msgs, const uint32_t* msg_offsets, size_t n,
                               const void* sig);
/* the same with the signature as an AggregateSignature (blst_p2, Jacobian, 288 B): finish(signature: AggregateSignature),
 * blst_min_pubkey_sig_core.nim:357 - converted to affine on the device (blst_p2_to_affine) before the pairing */
int mi355_bls_aggregate_verify_p2(mi355_bls_ctx* ctx, const void* pks, const uint8_t* msgs, const uint32_t* msg_offsets, size_t n,
                                  const void* sig_p2);

/* The streaming form, ContextCoreAggregateVerify.init / update / finish (blst_min_pubkey_sig_core.nim:321-414; driven by
 * bls_sig_min_pubkey.nim:127-199 for the AoS and SoA overloads): init resets the context's pair list; update(publicKey,
 * message) appends one pair and returns 1, or 0 for the infinity public key (the reference's update returns false:
 * BLST_PK_IS_INFINITY) after which finish returns 0; finish(signature) = commit + finalVerify: one device call over the
 * collected pairs, returns the verdict (0 when no pair was added) and consumes the context (init again before reuse).
 * pk: 96-byte blst_p1_affine, sig: 192-byte blst_p2_affine, any message length. */
int mi355_bls_aggv_init(mi355_bls_ctx* ctx);
int mi355_bls_aggv_update(mi355_bls_ctx* ctx, const void* pk, const uint8_t* msg, size_t msg_len);
int mi355_bls_aggv_finish(mi355_bls_ctx* ctx, const void* sig);
/* finish(signature: AggregateSignature) (core :357): sig_p2 = blst_p2, Jacobian, 288 B.  update returns MI355_BLS_ERR_CAPACITY (and
 * appends nothing) once the collected messages would exceed 4 GiB (offsets are 32-bit). */
int mi355_bls_aggv_finish_p2(mi355_bls_ctx* ctx, const void* sig_p2);

/* Batch signer / input generator.  Per tuple i, from a 32-byte little-endian secret scalar
 * (blst_scalar image, SecretKey, blst_min_pubkey_sig_core.nim:43-66) and a 32-byte message:
 *   publicFromSecret (core :118-133): sk == 0 or sk >= r -> status[i] = 1 and a zeroed record; pk = affine([sk]G1)
 *   coreSign (core :230-251) with the signature DST (bls_sig_min_pubkey.nim:31): sig = affine([sk]H(msg))
 * written as the 320-byte SignatureSet record (pk, msg, sig).  Returns 1 when every key was valid, 0 otherwise.
 * The scalar multiplications are VARIABLE TIME: this exists to synthesise test and bench inputs (the reference
 * does the same with sign() in benchmarks/bls_signature.nim:258-268), never to sign with real keys. */
int mi355_bls_sign_sets(mi355_bls_ctx* ctx, const uint8_t* sks32, const uint8_t* msgs32, size_t n, void* out_sets, uint8_t* status);
int mi355_bls_sign_sets_device(mi355_bls_ctx* ctx, const void* d_sks32, const void* d_msgs32, size_t n, void* d_out_sets, void* stream,
                               uint8_t* status);

/* popProve (bls_sig_min_pubkey.nim:34-58) for n secret keys, the input generator of the PoP calls: pk_i = affine([sk_i]G1) as a 96-byte
 * image, proof_i = affine([sk_i] hash_to_g2(rawFromPublic(pk_i), DST_POP)) as a 192-byte image.  sk == 0 or sk >= r: status[i] = 1 and zeroed
 * outputs, as mi355_bls_sign_sets.  Returns 1 when every key was valid, 0 otherwise.  VARIABLE TIME like the signer above: for tests and
 * benchmarks only, never for real keys. */
int mi355_bls_pop_prove(mi355_bls_ctx* ctx, const uint8_t* sks32, size_t n, void* out_pks96, void* out_proofs192, uint8_t* status);
int mi355_bls_pop_prove_device(mi355_bls_ctx* ctx, const void* d_sks32, size_t n, void* d_out_pks96, void* d_out_proofs192, void* stream,
                               uint8_t* status);

/* Stage outputs of the LAST batch call on this context, for parity tests (no reference
 * counterpart: BLST keeps these inside blst_pairing).  `what`:
 *   0: blinding scalars r_i           n x 8 B  (LE u64)
 *   1: H(m_i) Jacobian                n x 288 B (blst_p2)
 *   2: [r_i]PK_i Jacobian             n x 144 B (blst_p1)
 *   3: sum [r_i]S_i Jacobian          288 B
 *   4: GT after final exponentiation  576 B   (f^(3 (p^12-1)/r))
 *   5: Miller-loop product before final exponentiation 576 B */
int mi355_bls_fetch_stage(mi355_bls_ctx* ctx, int what, void* out, size_t out_bytes);

/* Kernel timing of the last batch call, ms per stage measured with HIP events on the call's stream:
 * out[0..7] = blinding, hash_to_g2, pk_mul, sig_mul+sum, miller_lines, line_products, final, total. */
int mi355_bls_last_timings(mi355_bls_ctx* ctx, float out[8]);
/* Per-kernel split of the two-kernel stages of the last batch call (ms): k_hash_map, k_hash_clear (hash_to_g2),
 * k_lineprod, k_lineprod2 (line_products). */
int mi355_bls_last_kernel_timings(mi355_bls_ctx* ctx, float out[4]);

/* TEST HOOK: out[i] = clear_cofactor(q0_i + q1_i) (RFC 9380 G.3, the last stage of hash-to-G2) for n <= max_sets pairs of blst_p2 images
 * (2 x 288 B per pair, host memory), computed by the kernels the batch path would launch for this context (k_hash_clear on a throughput-mode context, the lane-team engine on a
 * latency-mode one) - lets the tests put points through them that no hash produces
 * (the point at infinity, equal or opposite points: the cases its incomplete addition formulas flag and recompute). */
int mi355_bls_debug_g2_clear_cofactor(mi355_bls_ctx* ctx, const uint8_t* in_pairs, size_t n, uint8_t* out_p2);

/* TEST HOOK: out_p2 = hash_to_G2(msg, dst) (blst_p2 image, Jacobian) computed by the one-message kernel of fastAggregateVerify / verify under ANY
 * domain separation tag (1 .. 64 bytes): holds the device against published hash-to-curve vectors (RFC 9380 J.10.1), whose DST is not the scheme's. */
int mi355_bls_debug_hash_to_g2(mi355_bls_ctx* ctx, const uint8_t* msg, size_t msg_len, const uint8_t* dst, size_t dst_len, uint8_t out_p2[288]);

/* TEST HOOK: the device's field arithmetic bodies on CHOSEN operands.  An operand is a RAW fp image: 14 signed 28-bit limbs in 14 uint32 words,
 * the in-register form (csrc/fp.hpp), not blst bytes; results come back raw as well (14 words each), so that a test can check the documented
 * output bounds.  a, b, out: host memory, n <= max_sets operands each.  The caller keeps every operand inside the contract of the operation
 * (tests/fp_operands.py; tests/test_fp_operands_emu.py proves it on the bounds-tracked CPU build).
 *   lane operations (one operand pair per lane, the out-of-line bodies the product calls, in a kernel compiled for 256 registers like k_hash_map):
 *     FP_MUL a b, FP_SQR a, FP_SQR_N1 / FP_SQR_N4 fp_sqr_n(a, 1 / 4), FP_REDUCE a, FP_INV a, FP_POW fp_recip_sqrt_pow(a) (the assembly body);
 *     FP_DOT2: a and b hold TWO images per result, out[i] = a[2i] b[2i] + a[2i+1] b[2i+1];
 *     PRED: word 0 of out[i] = fp_is_zero(a[i]) | fp_eq(a[i], b[i]) << 1 | fp2_sgn0((a[i], b[i])) << 2, words 1..13 zero
 *   row operations (a wave with row constants and an LDS power table, as k_hash_map_rows and k_hash_one set it up):
 *     ROW_MUL a b / ROW_SQR a (four operands per wave, one per DPP row), POW_PER_ROW (k_hash_map_rows' form: four operands per wave),
 *     POW_TWO_ROWS (k_hash_one's form: the operands of lanes 0 and 1 of a wave); the two POW forms return a^((p-3)/4) as the functor does. */
enum {
    MI355_BLS_FPOP_FP_MUL = 0, MI355_BLS_FPOP_FP_SQR = 1, MI355_BLS_FPOP_FP_SQR_N1 = 2, MI355_BLS_FPOP_FP_SQR_N4 = 3, MI355_BLS_FPOP_FP_DOT2 = 4,
    MI355_BLS_FPOP_FP_REDUCE = 5, MI355_BLS_FPOP_FP_INV = 6, MI355_BLS_FPOP_FP_POW = 7, MI355_BLS_FPOP_PRED = 8,
    MI355_BLS_FPOP_ROW_MUL = 16, MI355_BLS_FPOP_ROW_SQR = 17, MI355_BLS_FPOP_POW_PER_ROW = 18, MI355_BLS_FPOP_POW_TWO_ROWS = 19
};
int mi355_bls_debug_fp_op(mi355_bls_ctx* ctx, int op, const uint32_t* a, const uint32_t* b, size_t n, uint32_t* out);

/* TEST HOOK: the SSWU map + 3-isogeny of the batch path on CHOSEN field elements: us = n pairs (u0, u1) of Fp2 elements as raw images
 * (4 x 14 words per pair), out_p2 = 2n blst_p2 images (Jacobian, 288 B): the mapped points before cofactor clearing.  The kernel is the
 * form hash_map_for names for this context and n (rows / spread / plain), with the body of k_hash_map* and the field elements loaded where
 * those hash a message. */
int mi355_bls_debug_map_to_g2(mi355_bls_ctx* ctx, const uint32_t* us, size_t n, uint8_t* out_p2);

/* TEST HOOK: mi355_bls_batch_verify_serial with blinding scalars of the CALLER'S choice: r[i] (non-zero u64) takes the place of the i-th link of the
 * SHA-256 chain, everything behind the scalars is the serial call's for this n on this context - the same plan (csrc/plan.hpp slice_for), k_pkmul or
 * k_pkmul_spread, the signature side's digit sort and buckets, the same forks, the same verdict (1 / 0) - and mi355_bls_fetch_stage 0 .. 5 work after
 * it as after any batch call.  The production scalars come from a hash no test can steer; this puts the scalar-dependent code (signed digits and
 * their carries, a not-started accumulator, zero digits, waves whose lanes all agree, empty and crowded buckets) under inputs picked for it
 * (tests/blind_scalars.py).  sets, r: host memory; one slice only, 1 <= n <= max_sets.  MI355_BLS_ERR_ARG for a null pointer, n == 0, n > max_sets,
 * a context with a batch pending, or ANY r[i] == 0 (the chain never yields zero: the hook does not take the kernels outside their contract). */
int mi355_bls_debug_batch_verify_scalars(mi355_bls_ctx* ctx, const void* sets, size_t n, const uint64_t r[]);

/* Test hooks (no reference counterpart).  debug_fail_next_enqueue: the next batch / shard enqueue on this context fails with
 * MI355_BLS_ERR_HIP before touching the device (exercises the multi-device driver's clean-up path).  debug_multi_enqueue_us:
 * host time in microseconds, counted from the start of the last mi355_bls_batch_verify_multi* call of this thread, at which each
 * device's shard was handed to its stream (the start skew between devices); returns the number of devices recorded. */
int mi355_bls_debug_fail_next_enqueue(mi355_bls_ctx* ctx);
/* mi355_bls_verify_each with the value of every set: gt_out gets n x 576 B, final_exp(f_i) as a blst_fp12 image (what
 * mi355_bls_fetch_stage(4) is to the batch paths).  debug_verify_each_passes: per-set passes this context has made so far. */
int mi355_bls_debug_verify_each_gt(mi355_bls_ctx* ctx, const void* sets, size_t n, uint8_t verdicts[], uint8_t* gt_out);
int mi355_bls_debug_verify_each_passes(mi355_bls_ctx* ctx);
/* mi355_bls_pop_verify_each with the value of every pair (n x 576 B), as mi355_bls_debug_verify_each_gt */
int mi355_bls_debug_pop_verify_each_gt(mi355_bls_ctx* ctx, const void* pks96, const void* proofs192, size_t n, uint8_t verdicts[], uint8_t* gt_out);
size_t mi355_bls_debug_multi_enqueue_us(float* out, size_t cap);
/* Batches submitted and not yet waited for, over all contexts of the process: what the library looks at when it chooses between the
 * low-latency and the least-work fold of the line products (a batch enqueued while this is zero has the chip to itself).  The tests
 * check that submit / wait / destroy keep it balanced. */
int mi355_bls_debug_batches_in_flight(void);
/* Device buffers, events, streams and pinned host buffers the library owns at this moment, over all contexts of the process (the lanes of
 * sliced calls and the lazily made workspaces included).  The tests check that destroying a context brings it back to where it was before
 * the context was created, whatever the context was used for. */
int mi355_bls_debug_live_resources(void);
/* Which fold of the per-lane line products the LAST batch / shard call on this context enqueued: 1 = the low-latency form on the Fp12 engine
 * (k_fold: latency-mode contexts, and any call enqueued while no other batch of the process was in flight), 0 = the least-work form
 * (k_lineprod2: throughput-mode contexts with other batches in flight).  Same GT bytes either way; profiles and the bench line record it so
 * that a kernel mix can be attributed.  Negative: bad argument. */
int mi355_bls_last_fold_form(mi355_bls_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
