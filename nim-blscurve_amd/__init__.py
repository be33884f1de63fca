"""Host-side mirror of nim-blscurve's batch-verifier API over the MI355X C ABI.

Python stands in for the Nim host layer (no Nim toolchain in the build image); names, argument
meaning and error behaviour follow ``blscurve/bls_batch_verifier.nim``:

  SignatureSet            (pubkey, message[32], signature) triplet, 320-byte record  (:34)
  BatchedBLSVerifierCache reusable per-caller scratch -> persistent device workspace  (:62-69,:108-119)
  batchVerifySerial       (:121-177)      batchVerifyParallel (:296-416)      batchVerify (:420-495)

The compute lives entirely in ``libblscurve_mi355x.so`` (hand-written HIP, gfx950).  There is no
CPU fallback: importing works without a GPU (so symbols can be checked), every compute call
raises ``BlsGpuError`` if the library or a GPU is missing.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MI355_BLS_LIB: another build of the same library (the A/B scripts under tools/ point it at nim-blscurve_amd/variants/<name>.so
# instead of copying a variant over the shipped file)
LIB_PATH = os.environ.get("MI355_BLS_LIB") or os.path.join(_HERE, "libblscurve_mi355x.so")
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "blscurve_mi355x.h"))

SIGSET_BYTES = 320
DEFAULT_NUM_THREADS = 4096


class BlsGpuError(RuntimeError):
    pass


_lib = None


def lib():
    """The C-ABI library; raises loudly when the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise BlsGpuError("HIP extension missing: %s (run nim-blscurve_amd/build.sh); no CPU fallback exists" % LIB_PATH)
        # torch bundles its own HIP runtime with the same soname as /opt/rocm's: whichever loads first
        # serves both, and torch must be that one or it later reports "No HIP GPUs are available".
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        vp, sz, u32, i32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
        L.mi355_bls_ctx_create.argtypes = [ctypes.POINTER(vp), i32, sz]
        L.mi355_bls_ctx_destroy.argtypes = [vp]
        L.mi355_bls_ctx_destroy.restype = None
        L.mi355_bls_last_error.restype = ctypes.c_char_p
        L.mi355_bls_build_info.restype = ctypes.c_char_p
        L.mi355_bls_ctx_set_num_threads.argtypes = [vp, u32]
        L.mi355_bls_ctx_set_cooperative.argtypes = [vp, i32]
        L.mi355_bls_batch_verify.argtypes = [vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_batch_verify_serial.argtypes = [vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_batch_verify_device.argtypes = [vp, vp, sz, ctypes.c_char_p, vp]
        L.mi355_bls_batch_submit_device.argtypes = [vp, vp, sz, ctypes.c_char_p, vp, vp]
        L.mi355_bls_batch_wait.argtypes = [vp]
        L.mi355_bls_batch_verify_many.argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.c_char_p, sz, ctypes.c_char_p]
        L.mi355_bls_batch_verify_many_device.argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.c_char_p, sz, ctypes.c_char_p, vp]
        for name in ("mi355_bls_batch_verify_many_each", "mi355_bls_batch_verify_many_locate"):
            getattr(L, name).argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.c_char_p, sz, ctypes.c_char_p]
            getattr(L, name + "_device").argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.c_char_p, sz, ctypes.c_char_p, vp]
        L.mi355_bls_debug_batch_verify_many_each_gt.argtypes = [vp, vp, ctypes.POINTER(sz), ctypes.c_char_p, sz, ctypes.c_char_p, ctypes.c_char_p]
        L.mi355_bls_debug_batch_verify_many_each_passes.argtypes = [vp]
        L.mi355_bls_verify_each.argtypes = [vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_verify_each_device.argtypes = [vp, vp, sz, ctypes.c_char_p, vp]
        L.mi355_bls_batch_verify_locate.argtypes = [vp, vp, sz, ctypes.c_char_p, ctypes.c_char_p]
        L.mi355_bls_batch_verify_locate_device.argtypes = [vp, vp, sz, ctypes.c_char_p, ctypes.c_char_p, vp]
        L.mi355_bls_debug_verify_each_gt.argtypes = [vp, vp, sz, ctypes.c_char_p, ctypes.c_char_p]
        L.mi355_bls_debug_verify_each_passes.argtypes = [vp]
        L.mi355_bls_pop_verify_each.argtypes = [vp, vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_pop_verify_each_device.argtypes = [vp, vp, vp, sz, ctypes.c_char_p, vp]
        L.mi355_bls_debug_pop_verify_each_gt.argtypes = [vp, vp, vp, sz, ctypes.c_char_p, ctypes.c_char_p]
        L.mi355_bls_batch_pop_verify.argtypes = [vp, vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_batch_pop_verify_device.argtypes = [vp, vp, vp, sz, ctypes.c_char_p, vp]
        L.mi355_bls_batch_pop_verify_locate.argtypes = [vp, vp, vp, sz, ctypes.c_char_p, ctypes.c_char_p]
        L.mi355_bls_batch_pop_verify_locate_device.argtypes = [vp, vp, vp, sz, ctypes.c_char_p, ctypes.c_char_p, vp]
        L.mi355_bls_compress_public_keys.argtypes = [vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_compress_public_keys_device.argtypes = [vp, vp, sz, vp, vp]
        L.mi355_bls_pop_prove.argtypes = [vp, ctypes.c_char_p, sz, vp, vp, vp]
        L.mi355_bls_pop_prove_device.argtypes = [vp, vp, sz, vp, vp, vp, vp]
        L.mi355_bls_batch_shard_device.argtypes = [vp, vp, sz, u32, u32, ctypes.c_char_p, vp, ctypes.c_char_p, ctypes.POINTER(i32)]
        L.mi355_bls_batch_shard_submit_device.argtypes = [vp, vp, sz, u32, u32, ctypes.c_char_p, vp, vp]
        L.mi355_bls_batch_shard_wait.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(i32)]
        L.mi355_bls_finalverify_shards.argtypes = [vp, ctypes.c_char_p, sz]
        L.mi355_bls_chunk_range.argtypes = [sz, u32, u32, u32, ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.mi355_bls_chunk_range.restype = None
        L.mi355_bls_ctx_shard_blob_device.argtypes = [vp, ctypes.POINTER(vp)]
        L.mi355_bls_ctx_set_shard_blob_device.argtypes = [vp, vp]
        L.mi355_bls_finalverify_blobs_submit_device.argtypes = [vp, vp, sz, sz, vp]
        L.mi355_bls_finalverify_wait.argtypes = [vp]
        L.mi355_bls_shard_plan.argtypes = [sz, u32, u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.mi355_bls_batch_verify_multi.argtypes = [ctypes.POINTER(vp), sz, vp, sz, ctypes.c_char_p]
        L.mi355_bls_batch_verify_multi_device.argtypes = [ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz, ctypes.c_char_p]
        L.mi355_bls_batch_verify_once.argtypes = [vp, sz, ctypes.c_char_p, u32]
        L.mi355_bls_default_ctx_release.argtypes = []
        L.mi355_bls_default_ctx_release.restype = None
        L.mi355_p1s_mult_pippenger_scratch_sizeof.argtypes = [sz]
        L.mi355_p1s_mult_pippenger_scratch_sizeof.restype = sz
        L.mi355_p1s_mult_pippenger.argtypes = [vp, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz, vp]
        L.mi355_p1s_mult_pippenger.restype = None
        L.mi355_p2s_mult_pippenger_scratch_sizeof.argtypes = [sz]
        L.mi355_p2s_mult_pippenger_scratch_sizeof.restype = sz
        L.mi355_p2s_mult_pippenger.argtypes = [vp, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz, vp]
        L.mi355_p2s_mult_pippenger.restype = None
        L.mi355_bls_p2s_mult_pippenger.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz]
        L.mi355_bls_p2s_mult_pippenger_device.argtypes = [vp, ctypes.c_char_p, vp, sz, vp, sz, vp]
        L.mi355_bls_g1_aggregate.argtypes = [vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_g1_aggregate_device.argtypes = [vp, vp, sz, vp, ctypes.c_char_p]
        L.mi355_bls_g2_aggregate.argtypes = [vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_g2_aggregate_device.argtypes = [vp, vp, sz, vp, ctypes.c_char_p]
        L.mi355_bls_recommend_hw_queues.argtypes = []
        L.mi355_bls_fast_aggregate_verify.argtypes = [vp, vp, sz, ctypes.c_char_p, sz, ctypes.c_char_p]
        L.mi355_bls_fast_aggregate_verify_device.argtypes = [vp, vp, sz, ctypes.c_char_p, sz, ctypes.c_char_p, vp]
        L.mi355_bls_fast_aggregate_verify_multi.argtypes = [ctypes.POINTER(vp), sz, vp, sz, ctypes.c_char_p, sz, ctypes.c_char_p]
        L.mi355_bls_verify_aggregate.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, sz, ctypes.c_char_p]
        pu32, psz = ctypes.POINTER(u32), ctypes.POINTER(sz)
        L.mi355_bls_aggregate_sets.argtypes = [vp, vp, sz, pu32, psz, sz, vp, vp, vp, vp]
        L.mi355_bls_aggregate_sets_device.argtypes = [vp, vp, sz, vp, psz, sz, vp, vp, vp, vp, vp]
        L.mi355_bls_fast_aggregate_verify_each.argtypes = [vp, vp, sz, pu32, psz, sz, vp, vp, vp]
        L.mi355_bls_fast_aggregate_verify_each_device.argtypes = [vp, vp, sz, vp, psz, sz, vp, vp, vp, vp]
        L.mi355_bls_batch_fast_aggregate_verify.argtypes = [vp, vp, sz, pu32, psz, sz, vp, vp, ctypes.c_char_p]
        L.mi355_bls_batch_fast_aggregate_verify_device.argtypes = [vp, vp, sz, vp, psz, sz, vp, vp, ctypes.c_char_p, vp]
        L.mi355_bls_aggregate_sets_bits.argtypes = [vp, vp, sz, pu32, psz, sz, vp, sz, pu32, vp, sz, vp, vp, vp, vp]
        L.mi355_bls_aggregate_sets_bits_device.argtypes = [vp, vp, sz, vp, psz, sz, vp, sz, pu32, vp, sz, vp, vp, vp, vp, vp]
        L.mi355_bls_fast_aggregate_verify_each_bits.argtypes = [vp, vp, sz, pu32, psz, sz, vp, sz, pu32, vp, sz, vp, vp, vp]
        L.mi355_bls_fast_aggregate_verify_each_bits_device.argtypes = [vp, vp, sz, vp, psz, sz, vp, sz, pu32, vp, sz, vp, vp, vp, vp]
        L.mi355_bls_batch_fast_aggregate_verify_bits.argtypes = [vp, vp, sz, pu32, psz, sz, vp, sz, pu32, vp, sz, vp, vp, ctypes.c_char_p]
        L.mi355_bls_batch_fast_aggregate_verify_bits_device.argtypes = [vp, vp, sz, vp, psz, sz, vp, sz, pu32, vp, sz, vp, vp, ctypes.c_char_p, vp]
        L.mi355_bls_debug_aggregate_bits_routes.argtypes = [vp, pu32]
        L.mi355_bls_aggregate_verify_each.argtypes = [vp, vp, sz, pu32, psz, sz, vp, vp, vp]
        L.mi355_bls_aggregate_verify_each_device.argtypes = [vp, vp, sz, vp, psz, sz, vp, vp, vp, vp]
        L.mi355_bls_debug_aggregate_verify_each_gt.argtypes = [vp, vp, sz, pu32, psz, sz, vp, vp, vp, vp]
        L.mi355_bls_pairing_check_each.argtypes = [vp, vp, vp, psz, sz, u32, vp, vp]
        L.mi355_bls_pairing_check_each_device.argtypes = [vp, vp, vp, psz, sz, u32, vp, vp, vp]
        L.mi355_bls_pairing_products.argtypes = [vp, vp, vp, psz, sz, u32, vp, vp, vp]
        L.mi355_bls_pairing_products_device.argtypes = [vp, vp, vp, psz, sz, u32, vp, vp, vp, vp]
        L.mi355_bls_batch_pairing_check.argtypes = [vp, vp, vp, psz, sz, u32, vp, vp]
        L.mi355_bls_batch_pairing_check_device.argtypes = [vp, vp, vp, psz, sz, u32, vp, vp, vp]
        L.mi355_bls_batch_pairing_check_locate.argtypes = [vp, vp, vp, psz, sz, u32, vp, vp, vp]
        L.mi355_bls_batch_pairing_check_locate_device.argtypes = [vp, vp, vp, psz, sz, u32, vp, vp, vp, vp]
        L.mi355_bls_debug_batch_pairing_check_scalars.argtypes = [vp, vp, vp, psz, sz, u32, ctypes.POINTER(ctypes.c_uint64), vp, vp]
        L.mi355_bls_aggregate_signature_sets.argtypes = [vp, vp, sz, pu32, psz, sz, vp, vp, vp]
        L.mi355_bls_aggregate_signature_sets_device.argtypes = [vp, vp, sz, vp, psz, sz, vp, vp, vp, vp]
        L.mi355_bls_recover_signature_sets.argtypes = [vp, vp, sz, pu32, psz, sz, vp, vp, vp, vp]
        L.mi355_bls_recover_signature_sets_device.argtypes = [vp, vp, sz, vp, psz, sz, vp, vp, vp, vp, vp]
        L.mi355_bls_compress_signatures.argtypes = [vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_compress_signatures_device.argtypes = [vp, vp, sz, vp, vp]
        L.mi355_bls_deserialize_signatures.argtypes = [vp, ctypes.c_char_p, sz, u32, vp, vp]
        L.mi355_bls_deserialize_signatures_device.argtypes = [vp, vp, sz, u32, vp, vp, vp]
        L.mi355_bls_deserialize_public_keys.argtypes = [vp, ctypes.c_char_p, sz, u32, vp, vp]
        L.mi355_bls_deserialize_public_keys_device.argtypes = [vp, vp, sz, u32, vp, vp, vp]
        L.mi355_bls_admit_keys.argtypes = [vp, ctypes.c_char_p, ctypes.c_char_p, sz, u32, ctypes.c_char_p, vp, vp]
        L.mi355_bls_admit_keys_device.argtypes = [vp, vp, vp, sz, u32, ctypes.c_char_p, vp, vp, vp]
        L.mi355_bls_combine_sets.argtypes = [vp, vp, sz, pu32, psz, sz, ctypes.c_char_p, vp, vp]
        L.mi355_bls_combine_sets_device.argtypes = [vp, vp, sz, vp, psz, sz, ctypes.c_char_p, vp, vp, vp]
        L.mi355_bls_batch_verify_combined.argtypes = [vp, vp, sz, pu32, psz, sz, ctypes.c_char_p, ctypes.c_char_p]
        L.mi355_bls_batch_verify_combined_device.argtypes = [vp, vp, sz, vp, psz, sz, ctypes.c_char_p, ctypes.c_char_p, vp]
        L.mi355_bls_group_by_message.argtypes = [vp, sz, pu32, psz, psz]
        L.mi355_bls_p1s_mult_pippenger_scratch_sizeof.argtypes = [sz]
        L.mi355_bls_p1s_mult_pippenger_scratch_sizeof.restype = sz
        L.mi355_bls_p1s_mult_pippenger.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz]
        L.mi355_bls_p1s_mult_pippenger_device.argtypes = [vp, ctypes.c_char_p, vp, sz, vp, sz, vp]
        L.mi355_bls_p1s_mult_pippenger_many.argtypes = [vp, vp, vp, sz, vp, psz, sz, sz]
        L.mi355_bls_p1s_mult_pippenger_many_device.argtypes = [vp, vp, vp, vp, sz, vp, psz, sz, sz, vp]
        L.mi355_bls_p2s_mult_pippenger_many.argtypes = [vp, vp, vp, sz, vp, psz, sz, sz]
        L.mi355_bls_p2s_mult_pippenger_many_device.argtypes = [vp, vp, vp, vp, sz, vp, psz, sz, sz, vp]
        L.mi355_bls_p1s_to_affine.argtypes = [vp, vp, sz, vp]
        L.mi355_bls_p1s_to_affine_device.argtypes = [vp, vp, sz, vp, vp]
        L.mi355_bls_p2s_to_affine.argtypes = [vp, vp, sz, vp]
        L.mi355_bls_p2s_to_affine_device.argtypes = [vp, vp, sz, vp, vp]
        L.mi355_bls_debug_to_affine_set_run.argtypes = [vp, u32]
        for name in ("mi355_bls_p1s_lincomb_many", "mi355_bls_p2s_lincomb_many"):
            getattr(L, name).argtypes = [vp, vp, sz, pu32, psz, sz, vp, sz, u32, vp, vp]
            getattr(L, name + "_device").argtypes = [vp, vp, sz, vp, psz, sz, vp, sz, u32, vp, vp, vp]
        L.mi355_bls_debug_lincomb_set_chunk.argtypes = [vp, sz]
        L.mi355_bls_fr_open_many.argtypes = [vp, vp, sz, vp, sz, u32, vp, vp, vp, vp]
        L.mi355_bls_fr_open_many_device.argtypes = [vp, vp, sz, vp, sz, u32, vp, vp, vp, vp, vp]
        L.mi355_bls_debug_fropen_set_pass.argtypes = [vp, sz]
        L.mi355_bls_fr_ntt_many.argtypes = [vp, vp, sz, sz, u32, vp, vp, vp]
        L.mi355_bls_fr_ntt_many_device.argtypes = [vp, vp, sz, sz, u32, vp, vp, vp, vp]
        L.mi355_bls_fr_domain.argtypes = [vp, sz, u32, vp]
        L.mi355_bls_fr_domain_device.argtypes = [vp, sz, u32, vp, vp]
        L.mi355_bls_debug_frntt_set_tile.argtypes = [vp, u32]
        L.mi355_bls_debug_frntt_set_pass.argtypes = [vp, sz]
        L.mi355_bls_p1s_ntt_many.argtypes = [vp, vp, sz, sz, u32, vp]
        L.mi355_bls_p1s_ntt_many_device.argtypes = [vp, vp, sz, sz, u32, vp, vp]
        L.mi355_bls_debug_p1ntt_set_pass.argtypes = [vp, sz]
        L.mi355_bls_fk20_setup_sizeof.argtypes = [sz]
        L.mi355_bls_fk20_setup_sizeof.restype = sz
        L.mi355_bls_fk20_setup_create.argtypes = [vp, vp, vp, sz]
        L.mi355_bls_fk20_setup_create_device.argtypes = [vp, vp, vp, sz, vp]
        L.mi355_bls_fk20_setup_destroy.argtypes = [vp]
        L.mi355_bls_fk20_setup_destroy.restype = None
        L.mi355_bls_fk20_open_all_many.argtypes = [vp, vp, vp, sz, u32, vp, vp]
        L.mi355_bls_fk20_open_all_many_device.argtypes = [vp, vp, vp, sz, u32, vp, vp, vp]
        L.mi355_bls_debug_fk20_set_pass.argtypes = [vp, sz]
        L.mi355_bls_fk20_setup_create_cells.argtypes = [vp, vp, vp, sz, sz]
        L.mi355_bls_fk20_setup_create_cells_device.argtypes = [vp, vp, vp, sz, sz, vp]
        L.mi355_bls_fk20_open_cells_many.argtypes = [vp, vp, vp, sz, sz, u32, vp, vp]
        L.mi355_bls_fk20_open_cells_many_device.argtypes = [vp, vp, vp, sz, sz, u32, vp, vp, vp]
        L.mi355_bls_p1s_table_sizeof.argtypes = [sz, sz, sz]
        L.mi355_bls_p1s_table_sizeof.restype = sz
        L.mi355_bls_p1s_table_create.argtypes = [vp, vp, vp, sz, sz, sz]
        L.mi355_bls_p1s_table_create_device.argtypes = [vp, vp, vp, sz, sz, sz, vp]
        L.mi355_bls_p1s_table_destroy.argtypes = [vp]
        L.mi355_bls_p1s_table_destroy.restype = None
        L.mi355_bls_p1s_mult_table.argtypes = [vp, vp, vp, vp, sz]
        L.mi355_bls_p1s_mult_table_device.argtypes = [vp, vp, vp, vp, sz, vp]
        L.mi355_bls_p1s_mult_table_many.argtypes = [vp, vp, vp, vp, sz, sz]
        L.mi355_bls_p1s_mult_table_many_device.argtypes = [vp, vp, vp, vp, vp, sz, sz, vp]
        L.mi355_bls_debug_p1s_table_rows.argtypes = [vp, sz, sz, sz, sz, vp]
        L.mi355_bls_debug_p1s_table_last_plan.argtypes = [vp, pu32]
        L.mi355_bls_debug_p1s_table_set_plan.argtypes = [vp, u32, u32]
        cp = ctypes.c_char_p
        L.mi355_bls_deserialize_sets.argtypes = [vp, cp, cp, cp, sz, vp, vp]
        L.mi355_bls_deserialize_sets_device.argtypes = [vp, vp, vp, vp, sz, vp, vp, vp]
        L.mi355_bls_deserialize_sets_ex.argtypes = [vp, cp, cp, cp, sz, u32, vp, vp]
        L.mi355_bls_deserialize_sets_ex_device.argtypes = [vp, vp, vp, vp, sz, u32, vp, vp, vp]
        L.mi355_bls_batch_verify_compressed.argtypes = [vp, cp, cp, cp, sz, cp, vp]
        L.mi355_bls_batch_verify_compressed_device.argtypes = [vp, vp, vp, vp, sz, cp, vp, vp]
        L.mi355_bls_last_deser_ms.argtypes = [vp]
        L.mi355_bls_last_deser_ms.restype = ctypes.c_float
        L.mi355_bls_combine.argtypes = [vp, cp, cp, cp, sz, cp, cp]
        L.mi355_bls_sign_sets.argtypes = [vp, cp, cp, sz, vp, vp]
        L.mi355_bls_sign_sets_device.argtypes = [vp, vp, vp, sz, vp, vp, vp]
        L.mi355_bls_aggregate_verify.argtypes = [vp, cp, cp, ctypes.POINTER(ctypes.c_uint32), sz, cp]
        L.mi355_bls_aggv_init.argtypes = [vp]
        L.mi355_bls_aggv_update.argtypes = [vp, cp, cp, sz]
        L.mi355_bls_aggv_finish.argtypes = [vp, cp]
        L.mi355_bls_aggv_finish_p2.argtypes = [vp, cp]
        L.mi355_bls_aggregate_verify_p2.argtypes = [vp, cp, cp, ctypes.POINTER(ctypes.c_uint32), sz, cp]
        L.mi355_bls_msm_shard_range.argtypes = [sz, u32, u32, ctypes.POINTER(sz), ctypes.POINTER(sz)]
        L.mi355_bls_msm_shard_range.restype = None
        L.mi355_bls_p1s_mult_pippenger_multi.argtypes = [ctypes.POINTER(vp), sz, ctypes.c_char_p, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz]
        L.mi355_bls_p2s_mult_pippenger_multi.argtypes = [ctypes.POINTER(vp), sz, ctypes.c_char_p, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz]
        L.mi355_bls_p1s_mult_pippenger_multi_device.argtypes = [ctypes.POINTER(vp), sz, ctypes.c_char_p, ctypes.POINTER(vp), sz, ctypes.POINTER(vp), sz]
        L.mi355_bls_p1s_mult_pippenger_partial_device.argtypes = [vp, vp, vp, sz, vp, sz, vp]
        L.mi355_bls_p1s_add.argtypes = [vp, ctypes.c_char_p, cp, sz]
        L.mi355_bls_p2s_add.argtypes = [vp, ctypes.c_char_p, cp, sz]
        L.mi355_bls_p1s_add_device.argtypes = [vp, ctypes.c_char_p, vp, sz, sz, vp]
        L.mi355_bls_debug_fail_next_enqueue.argtypes = [vp]
        L.mi355_bls_debug_batches_in_flight.argtypes = []
        L.mi355_bls_debug_live_resources.argtypes = []
        L.mi355_bls_debug_live_resources.restype = i32
        L.mi355_bls_last_fold_form.argtypes = [vp]
        L.mi355_bls_debug_g2_clear_cofactor.argtypes = [vp, cp, sz, cp]
        L.mi355_bls_debug_hash_to_g2.argtypes = [vp, cp, sz, cp, sz, cp]
        L.mi355_bls_debug_fp_op.argtypes = [vp, i32, cp, cp, sz, cp]
        L.mi355_bls_debug_map_to_g2.argtypes = [vp, cp, sz, cp]
        L.mi355_bls_debug_batch_verify_scalars.argtypes = [vp, vp, sz, ctypes.POINTER(ctypes.c_uint64)]
        L.mi355_bls_batch_verify_by_message.argtypes = [vp, vp, sz, ctypes.c_char_p]
        L.mi355_bls_batch_verify_by_message_device.argtypes = [vp, vp, sz, ctypes.c_char_p, vp]
        L.mi355_bls_last_message_groups.argtypes = [vp]
        L.mi355_bls_debug_batch_verify_by_message_scalars.argtypes = [vp, vp, sz, ctypes.POINTER(ctypes.c_uint64)]
        L.mi355_bls_debug_multi_enqueue_us.argtypes = [ctypes.POINTER(ctypes.c_float), sz]
        L.mi355_bls_debug_multi_enqueue_us.restype = sz
        L.mi355_bls_fetch_stage.argtypes = [vp, i32, vp, sz]
        L.mi355_bls_last_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.mi355_bls_last_kernel_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        _lib = L
    return _lib


def build_info():
    """mi355_bls_build_info() as a dict: {"aligned": bool, "dpp_combine_off": bool, "stamp": str}."""
    kv = dict(x.split("=", 1) for x in lib().mi355_bls_build_info().decode().split())
    return {"aligned": kv.get("aligned") == "1", "dpp_combine_off": kv.get("dpp_combine") == "off", "stamp": kv.get("stamp", "unknown")}


def _check(rc):
    if rc < 0:
        raise BlsGpuError("mi355_bls error %d: %s" % (rc, lib().mi355_bls_last_error().decode()))
    return rc


def _rnd32(secureRandomBytes):
    """secureRandomBytes is `array[32, byte]` in the reference (bls_batch_verifier.nim:301): exactly 32 bytes,
    bytes-like.  (bytes(int) would silently give that many ZERO bytes, a short buffer lets the C side read past it.)"""
    if not isinstance(secureRandomBytes, (bytes, bytearray, memoryview)):
        raise ValueError("secureRandomBytes must be a bytes-like object of 32 bytes")
    b = bytes(secureRandomBytes)
    if len(b) != 32:
        raise ValueError("secureRandomBytes must be exactly 32 bytes, got %d" % len(b))
    return b


def pack_signature_sets(sets):
    """[(pubkey96, message32, signature192)] -> contiguous 320-byte records (the Nim tuple layout)."""
    out = bytearray()
    for pk, msg, sig in sets:
        if len(pk) != 96 or len(msg) != 32 or len(sig) != 192:
            raise ValueError("SignatureSet = (96-byte blst_p1_affine, 32-byte message, 192-byte blst_p2_affine)")
        out += pk + msg + sig
    return bytes(out)


def _as_records(input_):
    if isinstance(input_, (bytes, bytearray, memoryview)):
        b = bytes(input_)
        if len(b) % SIGSET_BYTES:
            raise ValueError("record buffer is not a multiple of 320 bytes")
        return b
    return pack_signature_sets(input_)


def chunk_range(n_total, num_threads, chunk_lo, chunk_hi):
    """Tuple range of chunks [chunk_lo, chunk_hi) (parallel_chunks.nim:42-66)."""
    first, count = ctypes.c_size_t(), ctypes.c_size_t()
    lib().mi355_bls_chunk_range(n_total, num_threads, chunk_lo, chunk_hi, ctypes.byref(first), ctypes.byref(count))
    return first.value, count.value


class BatchedBLSVerifierCache:
    """bls_batch_verifier.nim:62-69.  ``init(numThreads=...)`` mirrors ``init(tp: Taskpool)``:
    numThreads is the number of blinding chains the parallel path uses (B = min(n, numThreads))."""

    def __init__(self, max_sets=65536, numThreads=DEFAULT_NUM_THREADS, device=0):
        self._h = ctypes.c_void_p()
        self.max_sets = max_sets
        self.numThreads = numThreads
        _check(lib().mi355_bls_ctx_create(ctypes.byref(self._h), device, max_sets))
        _check(lib().mi355_bls_ctx_set_num_threads(self._h, numThreads))

    @classmethod
    def init(cls, max_sets=65536, numThreads=DEFAULT_NUM_THREADS, device=0):
        return cls(max_sets, numThreads, device)

    def close(self):
        if self._h:
            lib().mi355_bls_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- stage outputs of the last call (parity tests) --
    def set_cooperative(self, on):
        """Small batches: 8 lanes per set (latency, default) or one lane per set (throughput with many batches in flight)."""
        _check(lib().mi355_bls_ctx_set_cooperative(self._h, 1 if on else 0))

    def fetch(self, what, nbytes):
        b = ctypes.create_string_buffer(nbytes)
        _check(lib().mi355_bls_fetch_stage(self._h, what, b, nbytes))
        return b.raw

    def timings(self):
        t = (ctypes.c_float * 8)()
        _check(lib().mi355_bls_last_timings(self._h, t))
        names = ["blinding", "hash_to_g2", "pk_mul", "sig_mul_sum", "miller_lines", "line_products", "final", "total"]
        return dict(zip(names, list(t)))

    def kernel_timings(self):
        """ms of the kernels inside the two-kernel stages of the last batch call."""
        t = (ctypes.c_float * 4)()
        _check(lib().mi355_bls_last_kernel_timings(self._h, t))
        return dict(zip(["k_hash_map", "k_hash_clear", "k_lineprod", "k_lineprod2"], list(t)))

    def fold_form(self):
        """which fold of the line products the last batch call enqueued: 1 = the Fp12 engine (k_fold), 0 = k_lineprod2"""
        return lib().mi355_bls_last_fold_form(self._h)

    # -- device-resident entry points --
    def verify_device(self, d_ptr, n, secureRandomBytes, stream=0):
        return bool(_check(lib().mi355_bls_batch_verify_device(self._h, d_ptr, n, _rnd32(secureRandomBytes), stream)))

    def submit_device(self, d_ptr, n, secureRandomBytes, stream=0, after=None):
        """Enqueue a batch verification and return at once; wait() gives its verdict.  after: a context whose
        batch was submitted before; this one then starts beside that batch's serial tail."""
        _check(lib().mi355_bls_batch_submit_device(self._h, d_ptr, n, _rnd32(secureRandomBytes), stream, after._h if after is not None else None))

    def wait(self):
        return bool(_check(lib().mi355_bls_batch_wait(self._h)))

    def shard_device(self, d_ptr, n_total, chunk_lo, chunk_hi, secureRandomBytes, stream=0):
        out = ctypes.create_string_buffer(576)
        ok = ctypes.c_int()
        _check(lib().mi355_bls_batch_shard_device(self._h, d_ptr, n_total, chunk_lo, chunk_hi, _rnd32(secureRandomBytes), stream, out, ctypes.byref(ok)))
        return out.raw, bool(ok.value)

    def shard_submit_device(self, d_ptr, n_total, chunk_lo, chunk_hi, secureRandomBytes, stream=0, after=None):
        _check(lib().mi355_bls_batch_shard_submit_device(self._h, d_ptr, n_total, chunk_lo, chunk_hi, _rnd32(secureRandomBytes), stream,
                                                         after._h if after is not None else None))

    def shard_wait(self):
        out = ctypes.create_string_buffer(576)
        ok = ctypes.c_int()
        _check(lib().mi355_bls_batch_shard_wait(self._h, out, ctypes.byref(ok)))
        return out.raw, bool(ok.value)

    BLOB_BYTES = 640

    def shard_blob_ptr(self):
        """Device address of this context's shard blob (state | ok word), written by every shard submit on its stream."""
        p = ctypes.c_void_p()
        _check(lib().mi355_bls_ctx_shard_blob_device(self._h, ctypes.byref(p)))
        return p.value

    def set_shard_blob_ptr(self, d_ptr):
        """Shard submits write their blob (640 bytes) to this device address instead (the collective's send buffer); None resets."""
        _check(lib().mi355_bls_ctx_set_shard_blob_device(self._h, d_ptr))

    def finalverify_blobs_submit(self, d_blobs, k, stride=640, stream=0):
        """merge + finalVerify on k gathered shard blobs resident in device memory; finalverify_wait() gives the verdict."""
        _check(lib().mi355_bls_finalverify_blobs_submit_device(self._h, d_blobs, k, stride, stream))

    def finalverify_wait(self):
        return bool(_check(lib().mi355_bls_finalverify_wait(self._h)))

    def finalverify_shards(self, states):
        blob = b"".join(states)
        return bool(_check(lib().mi355_bls_finalverify_shards(self._h, blob, len(states))))


def shard_plan(n_total, num_threads, world, rank):
    """(chunk_lo, chunk_hi, first_tuple, tuple_count) of device `rank` (mi355_bls_shard_plan)."""
    lo, hi, first, count = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_size_t(), ctypes.c_size_t()
    _check(lib().mi355_bls_shard_plan(n_total, num_threads, world, rank, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(first), ctypes.byref(count)))
    return lo.value, hi.value, first.value, count.value


def batchVerifyMulti(caches, input_, secureRandomBytes):
    """batchVerifyParallel over several devices from one host thread (mi355_bls_batch_verify_multi): caches[g] lives on
    device g; all must share numThreads.  Empty input -> False."""
    rec = _as_records(input_)
    n = len(rec) // SIGSET_BYTES
    if n == 0:
        return False
    arr = (ctypes.c_void_p * len(caches))(*[c._h for c in caches])
    return bool(_check(lib().mi355_bls_batch_verify_multi(arr, len(caches), rec, n, _rnd32(secureRandomBytes))))


def batchVerifyMulti_device(caches, d_ptrs, n, secureRandomBytes):
    """Same with shard g's records already resident on device g (d_ptrs[g])."""
    arr = (ctypes.c_void_p * len(caches))(*[c._h for c in caches])
    ptrs = (ctypes.c_void_p * len(caches))(*d_ptrs)
    return bool(_check(lib().mi355_bls_batch_verify_multi_device(arr, len(caches), ptrs, n, _rnd32(secureRandomBytes))))


def batchVerifyOnce(input_, secureRandomBytes, numThreads=DEFAULT_NUM_THREADS):
    """The cache-less overloads batchVerify(tp, input, rnd) (bls_batch_verifier.nim:475-495) on the process-wide default context."""
    rec = _as_records(input_)
    n = len(rec) // SIGSET_BYTES
    if n == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_verify_once(rec, n, _rnd32(secureRandomBytes), numThreads)))


def batchVerifyMany(cache, inputs, secureRandomBytes_list):
    """k independent batches in ONE device pass (mi355_bls_batch_verify_many): inputs[b] is batch b (records or SignatureSet list),
    secureRandomBytes_list[b] its random bytes.  -> [bool] * k, each what batchVerify(cache, inputs[b], rnd[b]) returns."""
    recs = [_as_records(x) for x in inputs]
    if len(recs) != len(secureRandomBytes_list):
        raise ValueError("one secureRandomBytes per batch")
    k = len(recs)
    if k == 0:
        return []
    counts = (ctypes.c_size_t * k)(*[len(r) // SIGSET_BYTES for r in recs])
    rnds = b"".join(_rnd32(r) for r in secureRandomBytes_list)
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_batch_verify_many(cache._h, b"".join(recs) or b"\0", counts, rnds, k, out))
    return [bool(v) for v in out.raw]


def batchVerifyMany_device(cache, d_ptr, counts, secureRandomBytes_list, stream=0):
    """Same with the tuples of all batches contiguous in device memory."""
    k = len(counts)
    carr = (ctypes.c_size_t * k)(*counts)
    rnds = b"".join(_rnd32(r) for r in secureRandomBytes_list)
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_batch_verify_many_device(cache._h, d_ptr, carr, rnds, k, out, stream))
    return [bool(v) for v in out.raw]


def _many_host(inputs, secureRandomBytes_list):
    """the batches of a k-batch call -> (records end to end, counts array, rnds, k)"""
    recs = [_as_records(x) for x in inputs]
    if len(recs) != len(secureRandomBytes_list):
        raise ValueError("one secureRandomBytes per batch")
    k = len(recs)
    counts = (ctypes.c_size_t * max(k, 1))(*[len(r) // SIGSET_BYTES for r in recs])
    return b"".join(recs) or b"\0", counts, b"".join(_rnd32(r) for r in secureRandomBytes_list), k


def _many_device(counts, secureRandomBytes_list):
    k = len(counts)
    if k != len(secureRandomBytes_list):
        raise ValueError("one secureRandomBytes per batch")
    return (ctypes.c_size_t * max(k, 1))(*counts), b"".join(_rnd32(r) for r in secureRandomBytes_list), k


def batchVerifyManyEach(cache, inputs, secureRandomBytes_list):
    """Per-batch verdicts for k batches in ONE device pass (mi355_bls_batch_verify_many_each): arguments as batchVerifyMany.  -> [bool] * k,
    each what batchVerify(cache, inputs[b], rnd[b]) returns, computed as batch b's own product - one bad batch costs the others nothing."""
    rec, counts, rnds, k = _many_host(inputs, secureRandomBytes_list)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_batch_verify_many_each(cache._h, rec, counts, rnds, k, out))
    return [v == 1 for v in out.raw]


def batchVerifyManyEach_device(cache, d_ptr, counts, secureRandomBytes_list, stream=0):
    """Same with the records of all batches contiguous in device memory."""
    carr, rnds, k = _many_device(counts, secureRandomBytes_list)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_batch_verify_many_each_device(cache._h, d_ptr, carr, rnds, k, out, stream))
    return [v == 1 for v in out.raw]


def batchVerifyManyLocate(cache, inputs, secureRandomBytes_list):
    """batchVerifyMany's merged pass first; only if it fails (or cannot run) one batchVerifyManyEach pass (mi355_bls_batch_verify_many_locate).
    -> [bool] * k, the verdicts of batchVerifyMany."""
    rec, counts, rnds, k = _many_host(inputs, secureRandomBytes_list)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_batch_verify_many_locate(cache._h, rec, counts, rnds, k, out))
    return [v == 1 for v in out.raw]


def batchVerifyManyLocate_device(cache, d_ptr, counts, secureRandomBytes_list, stream=0):
    """Same with the records of all batches contiguous in device memory."""
    carr, rnds, k = _many_device(counts, secureRandomBytes_list)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_batch_verify_many_locate_device(cache._h, d_ptr, carr, rnds, k, out, stream))
    return [v == 1 for v in out.raw]


def batchVerifyManyEachValues(cache, inputs, secureRandomBytes_list):
    """Test hook (mi355_bls_debug_batch_verify_many_each_gt): -> ([bool], [576-byte blst_fp12 image of batch b's value after the final
    exponentiation]); an empty batch's value is 576 zero bytes."""
    rec, counts, rnds, k = _many_host(inputs, secureRandomBytes_list)
    if k == 0:
        return [], []
    out, gt = ctypes.create_string_buffer(k), ctypes.create_string_buffer(k * 576)
    _check(lib().mi355_bls_debug_batch_verify_many_each_gt(cache._h, rec, counts, rnds, k, out, gt))
    raw = gt.raw
    return [v == 1 for v in out.raw], [raw[576 * i:576 * i + 576] for i in range(k)]


def batchVerifyManyEachPasses(cache):
    """per-batch passes the cache's context has made (test hook)"""
    return _check(lib().mi355_bls_debug_batch_verify_many_each_passes(cache._h))


def verifyEach(cache, input_):
    """verify(publicKey, message, signature) (bls_sig_min_pubkey.nim:108-125) for every set of the input in one device pass
    (mi355_bls_verify_each): -> [bool], one per set; no random bytes, set i's verdict depends on set i alone.  Empty input -> []."""
    rec = _as_records(input_)
    n = len(rec) // SIGSET_BYTES
    if n == 0:
        return []
    out = ctypes.create_string_buffer(n)
    _check(lib().mi355_bls_verify_each(cache._h, rec, n, out))
    return [v == 1 for v in out.raw]


def verifyEach_device(cache, d_ptr, n, stream=0):
    """Same with the n records in device memory."""
    if n == 0:
        return []
    out = ctypes.create_string_buffer(n)
    _check(lib().mi355_bls_verify_each_device(cache._h, d_ptr, n, out, stream))
    return [v == 1 for v in out.raw]


def verifyEachValues(cache, input_):
    """Test hook (mi355_bls_debug_verify_each_gt): -> ([bool], [576-byte blst_fp12 image of final_exp(f_i)])."""
    rec = _as_records(input_)
    n = len(rec) // SIGSET_BYTES
    if n == 0:
        return [], []
    out, gt = ctypes.create_string_buffer(n), ctypes.create_string_buffer(n * 576)
    _check(lib().mi355_bls_debug_verify_each_gt(cache._h, rec, n, out, gt))
    raw = gt.raw                      # one copy: .raw copies the whole buffer at every access
    return [v == 1 for v in out.raw], [raw[576 * i:576 * i + 576] for i in range(n)]


def verifyEachPasses(cache):
    """per-set passes the cache's context has made (test hook)"""
    return _check(lib().mi355_bls_debug_verify_each_passes(cache._h))


FPOP = {"fp_mul": 0, "fp_sqr": 1, "fp_sqr_n1": 2, "fp_sqr_n4": 3, "fp_dot2": 4, "fp_reduce": 5, "fp_inv": 6, "fp_pow": 7, "pred": 8,
        "row_mul": 16, "row_sqr": 17, "pow_per_row": 18, "pow_two_rows": 19}      # MI355_BLS_FPOP_*
FP_IMAGE_BYTES = 56                   # a raw fp image: 14 uint32 words, signed 28-bit limbs


def debugFpOp(cache, op, a, b=None):
    """Test hook (mi355_bls_debug_fp_op): the device's field arithmetic bodies on chosen raw images.  a, b: bytes of n images each (FPOP "fp_dot2":
    2n each); b defaults to a.  -> the bytes of n raw results (the predicate word of "pred" in word 0 of each)."""
    b = a if b is None else b
    per = FP_IMAGE_BYTES * (2 if op == "fp_dot2" else 1)
    if len(a) % per or len(a) != len(b):
        raise ValueError("operands must be the same number of 56-byte images")
    n = len(a) // per
    out = ctypes.create_string_buffer(max(n, 1) * FP_IMAGE_BYTES)
    _check(lib().mi355_bls_debug_fp_op(cache._h, FPOP[op], bytes(a), bytes(b), n, out))
    return out.raw


def debugMapToG2(cache, us):
    """Test hook (mi355_bls_debug_map_to_g2): us = bytes of n pairs (u0, u1) of Fp2 elements as raw images (224 bytes per pair) -> the bytes of the 2n
    mapped points (288-byte Jacobian images), by the form of the map kernel the batch path would take for this cache and n."""
    if len(us) % (4 * FP_IMAGE_BYTES):
        raise ValueError("us must be pairs of Fp2 elements: 224 bytes each")
    n = len(us) // (4 * FP_IMAGE_BYTES)
    out = ctypes.create_string_buffer(max(n, 1) * 576)
    _check(lib().mi355_bls_debug_map_to_g2(cache._h, bytes(us), n, out))
    return out.raw


def debugBatchVerifyScalars(cache, sets, scalars):
    """Test hook (mi355_bls_debug_batch_verify_scalars): batchVerifySerial of one slice with scalars[i] (a non-zero u64) as the blinding scalar of
    set i instead of the SHA-256 chain; cache.fetch(0 .. 5) show its stages.  1 <= n <= cache.max_sets; a zero scalar is refused."""
    rec = _as_records(sets)
    n = len(rec) // SIGSET_BYTES
    if len(scalars) != n:
        raise ValueError("one scalar per set: %d sets, %d scalars" % (n, len(scalars)))
    r = (ctypes.c_uint64 * max(n, 1))(*scalars)
    return bool(_check(lib().mi355_bls_debug_batch_verify_scalars(cache._h, rec, n, r)))


def batchVerifyByMessage(cache, input_, secureRandomBytes):
    """mi355_bls_batch_verify_by_message: batchVerifyParallel's verdict (same scalars, same final value) with hashing and the Miller loop run
    once per distinct message - the sets that share a message are found on the device.  Empty input -> False."""
    rec = _as_records(input_)
    n = len(rec) // SIGSET_BYTES
    if n == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_verify_by_message(cache._h, rec, n, _rnd32(secureRandomBytes))))


def batchVerifyByMessage_device(cache, d_ptr, n, secureRandomBytes, stream=0):
    """Same with the n records resident in device memory (raw pointer, 4-byte aligned)."""
    return bool(_check(lib().mi355_bls_batch_verify_by_message_device(cache._h, d_ptr, n, _rnd32(secureRandomBytes), stream)))


def lastMessageGroups(cache):
    """The number of distinct messages the last by-message call found in its (last) slice."""
    return _check(lib().mi355_bls_last_message_groups(cache._h))


def debugBatchVerifyByMessageScalars(cache, sets, scalars):
    """Test hook (mi355_bls_debug_batch_verify_by_message_scalars): debugBatchVerifyScalars' contract for the by-message pass."""
    rec = _as_records(sets)
    n = len(rec) // SIGSET_BYTES
    if len(scalars) != n:
        raise ValueError("one scalar per set: %d sets, %d scalars" % (n, len(scalars)))
    r = (ctypes.c_uint64 * max(n, 1))(*scalars)
    return bool(_check(lib().mi355_bls_debug_batch_verify_by_message_scalars(cache._h, rec, n, r)))


def batchVerifyLocate(cache, input_, secureRandomBytes):
    """batchVerify first; a failing batch gets one verifyEach pass (mi355_bls_batch_verify_locate).
    -> (ok, [bool] per set): (True, all True) for a passing batch, (False, the per-set verdicts) otherwise; empty input -> (False, [])."""
    rec = _as_records(input_)
    n = len(rec) // SIGSET_BYTES
    rnd = _rnd32(secureRandomBytes)
    if n == 0:
        return False, []
    out = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_batch_verify_locate(cache._h, rec, n, rnd, out))
    return bool(ok), [v == 1 for v in out.raw]


def batchVerifyLocate_device(cache, d_ptr, n, secureRandomBytes, stream=0):
    """Same with the n records in device memory."""
    rnd = _rnd32(secureRandomBytes)
    if n == 0:
        return False, []
    out = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_batch_verify_locate_device(cache._h, d_ptr, n, rnd, out, stream))
    return bool(ok), [v == 1 for v in out.raw]


def _keys_and_proofs(publicKeys, proofs):
    """n x 96-byte blst_p1_affine images, n x 192-byte blst_p2_affine images (lists or concatenated) -> (keys, proofs, n).  A proof of possession is a
    Signature on the wire (96 bytes): deserializeSets decodes it like any signature, with a message column that is not used."""
    pk = bytes(publicKeys) if isinstance(publicKeys, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in publicKeys)
    pr = bytes(proofs) if isinstance(proofs, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in proofs)
    if len(pk) % 96 or len(pr) % 192 or len(pk) // 96 != len(pr) // 192:
        raise ValueError("n x 96-byte public keys (blst_p1_affine), n x 192-byte proofs (blst_p2_affine)")
    return pk, pr, len(pk) // 96


def popVerifyEach(cache, publicKeys, proofs):
    """popVerify(publicKey, proof) (bls_sig_min_pubkey.nim:60-74) for every (key, proof) pair in one device pass (mi355_bls_pop_verify_each):
    -> [bool], one per pair; no random bytes, pair i's verdict depends on pair i alone.  Empty input -> []."""
    pk, pr, n = _keys_and_proofs(publicKeys, proofs)
    if n == 0:
        return []
    out = ctypes.create_string_buffer(n)
    _check(lib().mi355_bls_pop_verify_each(cache._h, pk, pr, n, out))
    return [v == 1 for v in out.raw]


def popVerifyEach_device(cache, d_pks, d_proofs, n, stream=0):
    """Same with the n keys and n proofs in device memory."""
    if n == 0:
        return []
    out = ctypes.create_string_buffer(n)
    _check(lib().mi355_bls_pop_verify_each_device(cache._h, d_pks, d_proofs, n, out, stream))
    return [v == 1 for v in out.raw]


def popVerifyEachValues(cache, publicKeys, proofs):
    """Test hook (mi355_bls_debug_pop_verify_each_gt): -> ([bool], [576-byte blst_fp12 image of final_exp(f_i)])."""
    pk, pr, n = _keys_and_proofs(publicKeys, proofs)
    if n == 0:
        return [], []
    out, gt = ctypes.create_string_buffer(n), ctypes.create_string_buffer(n * 576)
    _check(lib().mi355_bls_debug_pop_verify_each_gt(cache._h, pk, pr, n, out, gt))
    raw = gt.raw
    return [v == 1 for v in out.raw], [raw[576 * i:576 * i + 576] for i in range(n)]


def batchPopVerify(cache, publicKeys, proofs, secureRandomBytes):
    """The blinded batch check over the sets (pk_i, compress(pk_i), proof_i) under DST_POP (mi355_bls_batch_pop_verify; no reference
    counterpart): one verdict for the whole table; empty input -> False."""
    pk, pr, n = _keys_and_proofs(publicKeys, proofs)
    rnd = _rnd32(secureRandomBytes)
    if n == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_pop_verify(cache._h, pk, pr, n, rnd)))


def batchPopVerify_device(cache, d_pks, d_proofs, n, secureRandomBytes, stream=0):
    """Same with the n keys and n proofs in device memory."""
    rnd = _rnd32(secureRandomBytes)
    if n == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_pop_verify_device(cache._h, d_pks, d_proofs, n, rnd, stream)))


def batchPopVerifyLocate(cache, publicKeys, proofs, secureRandomBytes):
    """batchPopVerify first; a failing table gets one popVerifyEach pass (mi355_bls_batch_pop_verify_locate).
    -> (ok, [bool] per pair), as batchVerifyLocate; empty input -> (False, [])."""
    pk, pr, n = _keys_and_proofs(publicKeys, proofs)
    rnd = _rnd32(secureRandomBytes)
    if n == 0:
        return False, []
    out = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_batch_pop_verify_locate(cache._h, pk, pr, n, rnd, out))
    return bool(ok), [v == 1 for v in out.raw]


def batchPopVerifyLocate_device(cache, d_pks, d_proofs, n, secureRandomBytes, stream=0):
    """Same with the n keys and n proofs in device memory."""
    rnd = _rnd32(secureRandomBytes)
    if n == 0:
        return False, []
    out = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_batch_pop_verify_locate_device(cache._h, d_pks, d_proofs, n, rnd, out, stream))
    return bool(ok), [v == 1 for v in out.raw]


def compressPublicKeys(cache, publicKeys):
    """rawFromPublic / serialize (bls_sig_io.nim:203-211) for n keys (mi355_bls_compress_public_keys): n x 96-byte images -> [48-byte strings]."""
    pk = bytes(publicKeys) if isinstance(publicKeys, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in publicKeys)
    if len(pk) % 96:
        raise ValueError("n x 96-byte public keys (blst_p1_affine)")
    n = len(pk) // 96
    if n == 0:
        return []
    out = ctypes.create_string_buffer(48 * n)
    _check(lib().mi355_bls_compress_public_keys(cache._h, pk, n, out))
    raw = out.raw
    return [raw[48 * i:48 * i + 48] for i in range(n)]


def compressPublicKeys_device(cache, d_pks, n, d_out, stream=0):
    """Same with the keys and the n x 48 output bytes in device memory (raw pointers)."""
    if n:
        _check(lib().mi355_bls_compress_public_keys_device(cache._h, d_pks, n, d_out, stream))


def popProve(cache, secret_keys):
    """popProve (bls_sig_min_pubkey.nim:34-58) for n secret keys on the device, VARIABLE TIME (test and bench inputs only, like signSets).
    secret_keys: n x 32-byte little-endian scalars (list or concatenated).
    -> (all_valid, n x 96-byte keys, n x 192-byte proofs, per-key status bytes: 1 = sk == 0 or sk >= r, outputs zeroed)."""
    sk = bytes(secret_keys) if isinstance(secret_keys, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in secret_keys)
    if len(sk) % 32:
        raise ValueError("n x 32-byte secret keys")
    n = len(sk) // 32
    if n == 0:
        return True, b"", b"", b""
    pks, prs, st = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(192 * n), ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_pop_prove(cache._h, sk, n, pks, prs, st))
    return bool(ok), pks.raw, prs.raw, st.raw


def popProve_device(cache, d_sks, n, d_out_pks, d_out_proofs, stream=0):
    """Same with the scalars and both outputs resident in device memory (raw pointers)."""
    st = ctypes.create_string_buffer(max(n, 1))
    ok = _check(lib().mi355_bls_pop_prove_device(cache._h, d_sks, n, d_out_pks, d_out_proofs, stream, st))
    return bool(ok), st.raw[:n]


def batchVerifySerial(cache, input_, secureRandomBytes):
    """bls_batch_verifier.nim:121-160.  Empty input -> False."""
    rec = _as_records(input_)
    n = len(rec) // SIGSET_BYTES
    if n == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_verify_serial(cache._h, rec, n, _rnd32(secureRandomBytes))))


def batchVerifyParallel(cache, input_, secureRandomBytes):
    """bls_batch_verifier.nim:296-416."""
    rec = _as_records(input_)
    n = len(rec) // SIGSET_BYTES
    if n == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_verify(cache._h, rec, n, _rnd32(secureRandomBytes))))


def batchVerify(cache, input_, secureRandomBytes):
    """bls_batch_verifier.nim:420-495: parallel iff numThreads > 1 and n >= 3, else serial."""
    rec = _as_records(input_)
    n = len(rec) // SIGSET_BYTES
    if cache.numThreads > 1 and n >= 3:
        return batchVerifyParallel(cache, rec, secureRandomBytes)
    return batchVerifySerial(cache, rec, secureRandomBytes)


def aggregateAll(cache, publicKeys):
    """G1 aggregateAll (blst_min_pubkey_sig_core.nim:179-195): n x 96-byte affine keys -> 144-byte blst_p1.
    Empty input -> None (the reference returns false)."""
    buf = bytes(publicKeys) if isinstance(publicKeys, (bytes, bytearray, memoryview)) else b"".join(publicKeys)
    if len(buf) % 96:
        raise ValueError("public keys are 96-byte blst_p1_affine images")
    n = len(buf) // 96
    if n == 0:
        return None
    out = ctypes.create_string_buffer(144)
    _check(lib().mi355_bls_g1_aggregate(cache._h, buf, n, out))
    return out.raw


def aggregateAllSignatures(cache, signatures):
    """aggregateAll on signatures (genAggregatorProcedures(AggregateSignature, Signature, p2), blst_min_pubkey_sig_core.nim:179-195,211):
    n x 192-byte affine signatures -> 288-byte blst_p2 (an AggregateSignature).  Empty input -> None (the reference returns false)."""
    buf = bytes(signatures) if isinstance(signatures, (bytes, bytearray, memoryview)) else b"".join(signatures)
    if len(buf) % 192:
        raise ValueError("signatures are 192-byte blst_p2_affine images")
    n = len(buf) // 192
    if n == 0:
        return None
    out = ctypes.create_string_buffer(288)
    _check(lib().mi355_bls_g2_aggregate(cache._h, buf, n, out))
    return out.raw


def fastAggregateVerify(cache, publicKeys, message, signature):
    """bls_sig_min_pubkey.nim:234-258.  Empty key list -> False."""
    buf = bytes(publicKeys) if isinstance(publicKeys, (bytes, bytearray, memoryview)) else b"".join(publicKeys)
    if len(buf) % 96 or len(signature) != 192:
        raise ValueError("public keys are 96-byte, the signature a 192-byte BLST affine image")
    n = len(buf) // 96
    if n == 0:
        return False
    return bool(_check(lib().mi355_bls_fast_aggregate_verify(cache._h, buf, n, bytes(message), len(message), bytes(signature))))


def fastAggregateVerifyMulti(caches, publicKeys, message, signature):
    """fastAggregateVerify with the keys sharded over several devices (caches[g] on device g), one pairing on caches[0]."""
    buf = bytes(publicKeys) if isinstance(publicKeys, (bytes, bytearray, memoryview)) else b"".join(publicKeys)
    if len(buf) % 96 or len(signature) != 192:
        raise ValueError("public keys are 96-byte, the signature a 192-byte BLST affine image")
    n = len(buf) // 96
    if n == 0:
        return False
    arr = (ctypes.c_void_p * len(caches))(*[c._h for c in caches])
    return bool(_check(lib().mi355_bls_fast_aggregate_verify_multi(arr, len(caches), buf, n, bytes(message), len(message), bytes(signature))))


AGG_OK, AGG_EMPTY, AGG_INFINITY, AGG_BAD_INDEX = 0, 1, 2, 3      # status bytes of aggregateSets


def _join(x, unit, what):
    b = bytes(x) if isinstance(x, (bytes, bytearray, memoryview)) else b"".join(bytes(e) for e in x)
    if len(b) % unit:
        raise ValueError("%s: a multiple of %d bytes" % (what, unit))
    return b


def _key_lists(keys, messages, signatures):
    """The key lists of the aggregateSets family -> (key table bytes, n_table, idx array or None, offsets array, k, messages, signatures).
    keys: a list of key lists (each a list of 96-byte blst_p1_affine images, or their concatenation) - they are laid end to end and no index
    array is sent - or a tuple (table, idx, offsets): table = the 96-byte keys, idx = None or a sequence of table indices, offsets = k + 1
    non-decreasing positions (into idx, or into the table when idx is None)."""
    if isinstance(keys, tuple):
        table, idx, offsets = keys
        table = _join(table, 96, "key table")
        offsets = [int(x) for x in offsets]
        if idx is not None:
            idx = [int(x) for x in idx]
            if any(x < 0 or x >= 1 << 32 for x in idx):
                raise ValueError("indices are 32-bit unsigned")
            if offsets and offsets[-1] != len(idx):
                raise ValueError("offsets[k] is the length of the index array")
    else:
        lists = [_join(x, 96, "public keys") for x in keys]
        table, idx, offsets = b"".join(lists), None, [0]
        for x in lists:
            offsets.append(offsets[-1] + len(x) // 96)
    if not offsets or any(x < 0 for x in offsets):
        raise ValueError("offsets: k + 1 non-negative positions")
    k = len(offsets) - 1
    ms, sg = _join(messages, 32, "messages"), _join(signatures, 192, "signatures")
    if len(ms) != 32 * k or len(sg) != 192 * k:
        raise ValueError("one 32-byte message and one 192-byte signature per key list")
    iarr = (ctypes.c_uint32 * max(len(idx), 1))(*idx) if idx is not None else None
    return table, len(table) // 96, iarr, (ctypes.c_size_t * (k + 1))(*offsets), k, ms, sg


def aggregateSets(cache, keys, messages, signatures):
    """aggregateAll (blst_min_pubkey_sig_core.nim:179-195) for every key list in one device pass (mi355_bls_aggregate_sets); keys as
    _key_lists takes them.  -> (all_ok, k x 320-byte SignatureSet records with the aggregate keys, k status bytes: 0 ok, 1 empty list,
    2 aggregate at infinity, 3 index out of range; a record whose status is not 0 carries the infinity key)."""
    table, n_table, idx, offs, k, ms, sg = _key_lists(keys, messages, signatures)
    if k == 0:
        return False, b"", b""
    out, st = ctypes.create_string_buffer(320 * k), ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_aggregate_sets(cache._h, table or b"\0", n_table, idx, offs, k, ms, sg, out, st))
    return bool(ok), out.raw, st.raw


def aggregateSets_device(cache, d_keys, n_table, d_idx, offsets, d_msgs, d_sigs, d_out, stream=0):
    """Same with the key table, the indices (0 / None: none), messages, signatures and the output records in device memory (raw pointers);
    offsets stay on the host.  -> (all_ok, status bytes)."""
    k = len(offsets) - 1
    if k <= 0:
        return False, b""
    st = ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_aggregate_sets_device(cache._h, d_keys, n_table, d_idx or None, (ctypes.c_size_t * (k + 1))(*offsets), k, d_msgs, d_sigs,
                                                      d_out, st, stream))
    return bool(ok), st.raw


def fastAggregateVerifyEach(cache, keys, messages, signatures):
    """fastAggregateVerify (bls_sig_min_pubkey.nim:234-258) for every (key list, message, signature) in one device pass
    (mi355_bls_fast_aggregate_verify_each): -> [bool], one per list; an empty list gives False."""
    table, n_table, idx, offs, k, ms, sg = _key_lists(keys, messages, signatures)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_fast_aggregate_verify_each(cache._h, table or b"\0", n_table, idx, offs, k, ms, sg, out))
    return [v == 1 for v in out.raw]


def fastAggregateVerifyEach_device(cache, d_keys, n_table, d_idx, offsets, d_msgs, d_sigs, stream=0):
    k = len(offsets) - 1
    if k <= 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_fast_aggregate_verify_each_device(cache._h, d_keys, n_table, d_idx or None, (ctypes.c_size_t * (k + 1))(*offsets), k, d_msgs,
                                                              d_sigs, out, stream))
    return [v == 1 for v in out.raw]


def batchFastAggregateVerify(cache, keys, messages, signatures, secureRandomBytes):
    """batchVerify over the sets (aggregateAll(keys_s), message_s, signature_s) (mi355_bls_batch_fast_aggregate_verify): False when a list
    gives no key (empty, out-of-range index, aggregate at infinity) or the batch does not verify; no lists -> False."""
    rnd = _rnd32(secureRandomBytes)
    table, n_table, idx, offs, k, ms, sg = _key_lists(keys, messages, signatures)
    if k == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_fast_aggregate_verify(cache._h, table or b"\0", n_table, idx, offs, k, ms, sg, rnd)))


def batchFastAggregateVerify_device(cache, d_keys, n_table, d_idx, offsets, d_msgs, d_sigs, secureRandomBytes, stream=0):
    rnd = _rnd32(secureRandomBytes)
    k = len(offsets) - 1
    if k <= 0:
        return False
    return bool(_check(lib().mi355_bls_batch_fast_aggregate_verify_device(cache._h, d_keys, n_table, d_idx or None, (ctypes.c_size_t * (k + 1))(*offsets), k,
                                                                          d_msgs, d_sigs, rnd, stream)))


def _bit_sets(committees, which, bits, messages, signatures, committee_aggs, agg_stride):
    """The arguments of the aggregateSetsBits family -> (key table bytes, n_table, idx array or None, c_offsets array, m, aggregates or None,
    agg_stride, which array, bits, k, messages, signatures).  committees: as _key_lists takes key lists (a list of key lists laid end to
    end, or a tuple (table, idx, c_offsets)); which: k committee numbers; bits: the packed fields, or a list of one bytes object per set -
    set s owns exactly ceil(L / 8) bytes, L the length of its committee, position i at bit i % 8 of byte i // 8; committee_aggs: None, or
    m 96-byte aggregate keys agg_stride bytes apart (320: the records aggregateSets wrote for the committees)."""
    if isinstance(committees, tuple):
        m = len(committees[2]) - 1
    else:
        committees = list(committees)
        m = len(committees)
    table, n_table, idx, offs, m, _, _ = _key_lists(committees, bytes(32 * max(m, 0)), bytes(192 * max(m, 0)))
    if any(offs[c + 1] < offs[c] for c in range(m)):
        raise ValueError("committee offsets do not decrease")
    which = [int(x) for x in which]
    if any(x < 0 or x >= m for x in which):
        raise ValueError("which: committee numbers below %d" % m)
    k = len(which)
    need = [(offs[c + 1] - offs[c] + 7) // 8 for c in which]
    if isinstance(bits, (bytes, bytearray, memoryview)):
        bits = bytes(bits)
    else:
        bits = [bytes(b) for b in bits]
        if len(bits) != k or any(len(b) != n for b, n in zip(bits, need)):
            raise ValueError("bits: one field of ceil(L / 8) bytes per set")
        bits = b"".join(bits)
    if len(bits) != sum(need):
        raise ValueError("bits: %d bytes for these sets, not %d" % (sum(need), len(bits)))
    ms, sg = _join(messages, 32, "messages"), _join(signatures, 192, "signatures")
    if len(ms) != 32 * k or len(sg) != 192 * k:
        raise ValueError("one 32-byte message and one 192-byte signature per set")
    if committee_aggs is not None:
        committee_aggs, agg_stride = bytes(committee_aggs), int(agg_stride)
        if agg_stride < 96 or agg_stride % 4:
            raise ValueError("agg_stride: at least 96 and a multiple of 4")
        if m and len(committee_aggs) < (m - 1) * agg_stride + 96:
            raise ValueError("committee_aggs: one 96-byte aggregate per committee, agg_stride bytes apart")
    return table, n_table, idx, offs, m, committee_aggs, agg_stride, (ctypes.c_uint32 * max(k, 1))(*which), bits, k, ms, sg


def aggregateSetsBits(cache, committees, which, bits, messages, signatures, committee_aggs=None, agg_stride=96):
    """aggregateSets from committees and participation bits (mi355_bls_aggregate_sets_bits): the key of set s is aggregateAll over the keys
    of committee which[s] whose bit is set - computed, where committee_aggs is given and more than half of the committee signed, as
    subtractAll (blst_min_pubkey_sig_core.nim:197-209) of the absentees from the committee's aggregate.  Arguments as _bit_sets takes
    them.  -> (all_ok, k x 320-byte records, k status bytes), byte for byte aggregateSets' for the expanded index lists."""
    table, n_table, idx, offs, m, aggs, stride, wh, bits, k, ms, sg = _bit_sets(committees, which, bits, messages, signatures, committee_aggs, agg_stride)
    if k == 0:
        return False, b"", b""
    out, st = ctypes.create_string_buffer(320 * k), ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_aggregate_sets_bits(cache._h, table or b"\0", n_table, idx, offs, m, aggs, stride, wh, bits or b"\0", k, ms, sg, out, st))
    return bool(ok), out.raw, st.raw


def _bits_device_args(c_offsets, which):
    m, k = len(c_offsets) - 1, len(which)
    if m < 0 or any(int(x) < 0 or int(x) >= m for x in which):
        raise ValueError("which: committee numbers below %d" % max(m, 0))
    return (ctypes.c_size_t * (m + 1))(*c_offsets), m, (ctypes.c_uint32 * max(k, 1))(*which), k


def aggregateSetsBits_device(cache, d_keys, n_table, d_idx, c_offsets, d_committee_aggs, agg_stride, which, d_bits, d_msgs, d_sigs, d_out, stream=0):
    """Same with the key table, the indices (0 / None: none), the committee aggregates (0 / None: none), the bits, messages, signatures and
    the output records in device memory (raw pointers); c_offsets and which stay on the host.  -> (all_ok, status bytes)."""
    offs, m, wh, k = _bits_device_args(c_offsets, which)
    if k == 0:
        return False, b""
    st = ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_aggregate_sets_bits_device(cache._h, d_keys, n_table, d_idx or None, offs, m, d_committee_aggs or None, agg_stride, wh, d_bits, k,
                                                           d_msgs, d_sigs, d_out, st, stream))
    return bool(ok), st.raw


def fastAggregateVerifyEachBits(cache, committees, which, bits, messages, signatures, committee_aggs=None, agg_stride=96):
    """fastAggregateVerify (bls_sig_min_pubkey.nim:234-258) of every set's participants (mi355_bls_fast_aggregate_verify_each_bits):
    -> [bool], one per set; a set without a set bit gives False."""
    table, n_table, idx, offs, m, aggs, stride, wh, bits, k, ms, sg = _bit_sets(committees, which, bits, messages, signatures, committee_aggs, agg_stride)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_fast_aggregate_verify_each_bits(cache._h, table or b"\0", n_table, idx, offs, m, aggs, stride, wh, bits or b"\0", k, ms, sg, out))
    return [v == 1 for v in out.raw]


def fastAggregateVerifyEachBits_device(cache, d_keys, n_table, d_idx, c_offsets, d_committee_aggs, agg_stride, which, d_bits, d_msgs, d_sigs, stream=0):
    offs, m, wh, k = _bits_device_args(c_offsets, which)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_fast_aggregate_verify_each_bits_device(cache._h, d_keys, n_table, d_idx or None, offs, m, d_committee_aggs or None, agg_stride, wh,
                                                                   d_bits, k, d_msgs, d_sigs, out, stream))
    return [v == 1 for v in out.raw]


def batchFastAggregateVerifyBits(cache, committees, which, bits, messages, signatures, secureRandomBytes, committee_aggs=None, agg_stride=96):
    """batchVerify over the sets (aggregateAll(participants_s), message_s, signature_s) (mi355_bls_batch_fast_aggregate_verify_bits): False
    when a set gives no key or the batch does not verify; no sets -> False."""
    rnd = _rnd32(secureRandomBytes)
    table, n_table, idx, offs, m, aggs, stride, wh, bits, k, ms, sg = _bit_sets(committees, which, bits, messages, signatures, committee_aggs, agg_stride)
    if k == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_fast_aggregate_verify_bits(cache._h, table or b"\0", n_table, idx, offs, m, aggs, stride, wh, bits or b"\0", k, ms,
                                                                        sg, rnd)))


def batchFastAggregateVerifyBits_device(cache, d_keys, n_table, d_idx, c_offsets, d_committee_aggs, agg_stride, which, d_bits, d_msgs, d_sigs, secureRandomBytes,
                                        stream=0):
    rnd = _rnd32(secureRandomBytes)
    offs, m, wh, k = _bits_device_args(c_offsets, which)
    if k == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_fast_aggregate_verify_bits_device(cache._h, d_keys, n_table, d_idx or None, offs, m, d_committee_aggs or None,
                                                                               agg_stride, wh, d_bits, k, d_msgs, d_sigs, rnd, stream)))


def debug_aggregate_bits_routes(cache):
    """Test hook (mi355_bls_debug_aggregate_bits_routes): (sets summed directly, sets by exclusion) of the cache's last bits call."""
    out = (ctypes.c_uint32 * 2)()
    _check(lib().mi355_bls_debug_aggregate_bits_routes(cache._h, out))
    return out[0], out[1]


def _position_messages(messages, n_positions):
    """The per-position messages of aggregateVerifyEach -> n_positions x 32 bytes.  messages: their concatenation, a flat list of 32-byte
    messages, or a list of per-group lists (laid end to end, like the key lists of _key_lists)."""
    if isinstance(messages, (bytes, bytearray, memoryview)):
        ms = bytes(messages)
    else:
        ms = b"".join(bytes(e) if isinstance(e, (bytes, bytearray, memoryview)) else b"".join(bytes(x) for x in e) for e in messages)
    if len(ms) != 32 * n_positions:
        raise ValueError("one 32-byte message per position: %d x 32 bytes" % n_positions)
    return ms


def _pair_lists(keys, messages, signatures):
    """keys as _key_lists takes them, one 192-byte signature per group, one 32-byte message per position (_position_messages)."""
    k = len(keys[2]) - 1 if isinstance(keys, tuple) else len(keys)
    table, n_table, idx, offs, k, _, sg = _key_lists(keys, bytes(32 * max(k, 0)), signatures)
    return table, n_table, idx, offs, k, _position_messages(messages, offs[k]), sg


def aggregateVerifyEach(cache, keys, messages, signatures):
    """aggregateVerify (bls_sig_min_pubkey.nim:127-199) for every group of (key, message) pairs under its aggregate signature, in one device
    pass (mi355_bls_aggregate_verify_each): -> [bool], one per group.  keys as _key_lists takes them; messages: one 32-byte message per
    position (_position_messages); signatures: one 192-byte blst_p2_affine image per group.  An empty group, a group with an infinity key
    and a group with an index out of the table give False."""
    table, n_table, idx, offs, k, ms, sg = _pair_lists(keys, messages, signatures)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_aggregate_verify_each(cache._h, table or b"\0", n_table, idx, offs, k, ms or b"\0", sg, out))
    return [v == 1 for v in out.raw]


def aggregateVerifyEach_device(cache, d_keys, n_table, d_idx, offsets, d_msgs, d_sigs, stream=0):
    """Same with the key table, the indices (0 / None: none), the per-position messages and the k signatures in device memory (raw
    pointers); offsets stay on the host.  d_sigs is what aggregateSignatureSets_device writes as d_out192."""
    k = len(offsets) - 1
    if k <= 0:
        return []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_aggregate_verify_each_device(cache._h, d_keys, n_table, d_idx or None, (ctypes.c_size_t * (k + 1))(*offsets), k, d_msgs, d_sigs,
                                                         out, stream))
    return [v == 1 for v in out.raw]


def aggregateVerifyEachValues(cache, keys, messages, signatures):
    """Test hook (mi355_bls_debug_aggregate_verify_each_gt): -> ([bool], [576-byte blst_fp12 image of final_exp(f_g)]); an empty group's
    value is 576 zero bytes."""
    table, n_table, idx, offs, k, ms, sg = _pair_lists(keys, messages, signatures)
    if k == 0:
        return [], []
    out, gt = ctypes.create_string_buffer(k), ctypes.create_string_buffer(k * 576)
    _check(lib().mi355_bls_debug_aggregate_verify_each_gt(cache._h, table or b"\0", n_table, idx, offs, k, ms or b"\0", sg, out, gt))
    raw = gt.raw
    return [v == 1 for v in out.raw], [raw[576 * i:576 * i + 576] for i in range(k)]


PAIR_VALIDATE = 1
PAIR_OK, PAIR_P_OFF_CURVE, PAIR_P_NOT_IN_G1, PAIR_Q_OFF_CURVE, PAIR_Q_NOT_IN_G2 = range(5)


def _pair_groups(groups, flags):
    """groups: a list of groups, each a list of (96-byte blst_p1_affine image, 192-byte blst_p2_affine image) pairs (all zero: infinity)
    -> (p1s, q2s, offsets array, k, n, status buffer or None).  The pairs are laid end to end."""
    if flags & ~PAIR_VALIDATE:
        raise ValueError("unknown flag bits: %#x" % flags)
    offs, ps, qs = [0], [], []
    for g in groups:
        for p, q in g:
            if len(p) != 96 or len(q) != 192:
                raise ValueError("a pair is a 96-byte blst_p1_affine and a 192-byte blst_p2_affine image, got %d and %d bytes" % (len(p), len(q)))
            ps.append(bytes(p))
            qs.append(bytes(q))
        offs.append(len(ps))
    k, n = len(offs) - 1, len(ps)
    return b"".join(ps), b"".join(qs), (ctypes.c_size_t * (k + 1))(*offs), k, n, ctypes.create_string_buffer(max(n, 1))


def _pair_scalars(r, k):
    if len(r) != k:
        raise ValueError("one scalar per group: %d scalars for %d groups" % (len(r), k))
    if any(not 0 <= x < 1 << 64 for x in r):
        raise ValueError("a scalar is an unsigned 64-bit integer")
    return (ctypes.c_uint64 * max(k, 1))(*r)


def pairingCheckEach(cache, groups, flags=0, with_status=False):
    """k pairing-product checks in one device pass (mi355_bls_pairing_check_each): -> [bool], one per group: final_exp(prod miller(P, Q)) == 1.
    A pair with an operand at infinity contributes 1; an EMPTY group is the empty product, True.  flags = PAIR_VALIDATE: the device checks every
    finite operand (on the curve, in G1 / G2); a group holding a failing pair is False.  with_status: -> ([bool], [PAIR_* per pair])."""
    p1, q2, offs, k, n, st = _pair_groups(groups, flags)
    if k == 0:
        return ([], []) if with_status else []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_pairing_check_each(cache._h, p1 or None, q2 or None, offs, k, flags, out, st))
    v = [x == 1 for x in out.raw]
    return (v, list(st.raw[:n])) if with_status else v


def pairingProducts(cache, groups, flags=0, with_status=False):
    """The same pass with every group's value (mi355_bls_pairing_products): -> ([bool], [576-byte blst_fp12 image of the group's product after
    the final exponentiation]); an empty group's value is the image of one.  Two products are equal iff their images are."""
    p1, q2, offs, k, n, st = _pair_groups(groups, flags)
    if k == 0:
        return ([], [], []) if with_status else ([], [])
    out, gt = ctypes.create_string_buffer(k), ctypes.create_string_buffer(k * 576)
    _check(lib().mi355_bls_pairing_products(cache._h, p1 or None, q2 or None, offs, k, flags, out, st, gt))
    raw = gt.raw
    v, g = [x == 1 for x in out.raw], [raw[576 * i:576 * i + 576] for i in range(k)]
    return (v, g, list(st.raw[:n])) if with_status else (v, g)


def batchPairingCheck(cache, groups, secureRandomBytes, flags=0, with_status=False):
    """One verdict for all k checks (mi355_bls_batch_pairing_check): P of every pair of group g is multiplied by the g-th 64-bit scalar of the
    serial blinding chain from secureRandomBytes, and one product is formed.  Sound only for operands in G1 / G2: vouched for, or checked with
    flags = PAIR_VALIDATE.  No group: False."""
    rnd = _rnd32(secureRandomBytes)
    p1, q2, offs, k, n, st = _pair_groups(groups, flags)
    if k == 0:
        return (False, []) if with_status else False
    ok = bool(_check(lib().mi355_bls_batch_pairing_check(cache._h, p1 or None, q2 or None, offs, k, flags, rnd, st)))
    return (ok, list(st.raw[:n])) if with_status else ok


def batchPairingCheckLocate(cache, groups, secureRandomBytes, flags=0):
    """batchPairingCheck first; only behind a failure the per-group pass (mi355_bls_batch_pairing_check_locate) -> (bool, [bool] per group)."""
    rnd = _rnd32(secureRandomBytes)
    p1, q2, offs, k, n, st = _pair_groups(groups, flags)
    if k == 0:
        return False, []
    out = ctypes.create_string_buffer(k)
    ok = bool(_check(lib().mi355_bls_batch_pairing_check_locate(cache._h, p1 or None, q2 or None, offs, k, flags, rnd, st, out)))
    return ok, [x == 1 for x in out.raw]


def batchPairingCheckScalars(cache, groups, scalars, flags=0):
    """Test hook (mi355_bls_debug_batch_pairing_check_scalars): the blinded form with one scalar per group of the test's choice
    -> (bool, the 576-byte value of the one product)."""
    p1, q2, offs, k, n, st = _pair_groups(groups, flags)
    r = _pair_scalars(scalars, k)
    if k == 0:
        return False, b""
    gt = ctypes.create_string_buffer(576)
    ok = bool(_check(lib().mi355_bls_debug_batch_pairing_check_scalars(cache._h, p1 or None, q2 or None, offs, k, flags, r, st, gt)))
    return ok, gt.raw


def _pair_device_args(offsets, flags, n_status):
    if flags & ~PAIR_VALIDATE:
        raise ValueError("unknown flag bits: %#x" % flags)
    k = len(offsets) - 1
    if k >= 0 and (offsets[0] != 0 or any(b < a for a, b in zip(offsets, offsets[1:]))):
        raise ValueError("offsets start at 0 and never decrease")
    return k, ctypes.create_string_buffer(max(n_status, 1))


def pairingCheckEach_device(cache, d_p1s, d_q2s, offsets, flags=0, stream=0):
    """pairingCheckEach with the two arrays in device memory (raw pointers, 4-byte aligned); offsets stay on the host -> ([bool], [status])."""
    k, st = _pair_device_args(offsets, flags, offsets[-1] if offsets else 0)
    if k <= 0:
        return [], []
    out = ctypes.create_string_buffer(k)
    _check(lib().mi355_bls_pairing_check_each_device(cache._h, d_p1s or None, d_q2s or None, (ctypes.c_size_t * (k + 1))(*offsets), k, flags, out, st, stream))
    return [x == 1 for x in out.raw], list(st.raw[:offsets[-1]])


def pairingProducts_device(cache, d_p1s, d_q2s, offsets, flags=0, stream=0):
    k, st = _pair_device_args(offsets, flags, offsets[-1] if offsets else 0)
    if k <= 0:
        return [], []
    out, gt = ctypes.create_string_buffer(k), ctypes.create_string_buffer(k * 576)
    _check(lib().mi355_bls_pairing_products_device(cache._h, d_p1s or None, d_q2s or None, (ctypes.c_size_t * (k + 1))(*offsets), k, flags, out, st, gt, stream))
    raw = gt.raw
    return [x == 1 for x in out.raw], [raw[576 * i:576 * i + 576] for i in range(k)]


def batchPairingCheck_device(cache, d_p1s, d_q2s, offsets, secureRandomBytes, flags=0, stream=0):
    rnd = _rnd32(secureRandomBytes)
    k, st = _pair_device_args(offsets, flags, offsets[-1] if offsets else 0)
    if k <= 0:
        return False
    return bool(_check(lib().mi355_bls_batch_pairing_check_device(cache._h, d_p1s or None, d_q2s or None, (ctypes.c_size_t * (k + 1))(*offsets), k, flags, rnd, st,
                                                                   stream)))


def batchPairingCheckLocate_device(cache, d_p1s, d_q2s, offsets, secureRandomBytes, flags=0, stream=0):
    rnd = _rnd32(secureRandomBytes)
    k, st = _pair_device_args(offsets, flags, offsets[-1] if offsets else 0)
    if k <= 0:
        return False, []
    out = ctypes.create_string_buffer(k)
    ok = bool(_check(lib().mi355_bls_batch_pairing_check_locate_device(cache._h, d_p1s or None, d_q2s or None, (ctypes.c_size_t * (k + 1))(*offsets), k, flags, rnd,
                                                                        st, out, stream)))
    return ok, [x == 1 for x in out.raw]


def _signature_lists(signatures, row=192, what="signature"):
    """The signature lists of aggregateSignatureSets -> (table bytes, n_table, idx array or None, offsets array, k).  signatures: a list of
    signature lists (each a list of 192-byte blst_p2_affine images, or their concatenation) - they are laid end to end and no index array is
    sent - or a tuple (table, idx, offsets) as aggregateSets takes it for keys.  row, what: the same for other rows (the points of the
    lincomb calls)."""
    if isinstance(signatures, tuple):
        table, idx, offsets = signatures
        table = _join(table, row, what + " table")
        offsets = [int(x) for x in offsets]
        if idx is not None:
            idx = [int(x) for x in idx]
            if any(x < 0 or x >= 1 << 32 for x in idx):
                raise ValueError("indices are 32-bit unsigned")
            if offsets and offsets[-1] != len(idx):
                raise ValueError("offsets[k] is the length of the index array")
    else:
        lists = [_join(x, row, what + "s") for x in signatures]
        table, idx, offsets = b"".join(lists), None, [0]
        for x in lists:
            offsets.append(offsets[-1] + len(x) // row)
    if not offsets or any(x < 0 for x in offsets):
        raise ValueError("offsets: k + 1 non-negative positions")
    k = len(offsets) - 1
    iarr = (ctypes.c_uint32 * max(len(idx), 1))(*idx) if idx is not None else None
    return table, len(table) // row, iarr, (ctypes.c_size_t * (k + 1))(*offsets), k


def aggregateSignatureSets(cache, signatures, want192=True, want96=True):
    """aggregateAll on signatures (blst_min_pubkey_sig_core.nim:142-211) for every group in one device pass, finished and serialised
    (mi355_bls_aggregate_signature_sets); signatures as _signature_lists takes them.  -> (all_ok, k x 192-byte blst_p2_affine images or None,
    k x 96-byte wire forms or None, k status bytes: 0 ok, 1 empty group, 2 the aggregate is the point at infinity (its valid encodings are
    returned), 3 index out of range)."""
    if not (want192 or want96):
        raise ValueError("at least one of the two outputs")
    table, n_table, idx, offs, k = _signature_lists(signatures)
    if k == 0:
        return False, (b"" if want192 else None), (b"" if want96 else None), b""
    o192 = ctypes.create_string_buffer(192 * k) if want192 else None
    o96 = ctypes.create_string_buffer(96 * k) if want96 else None
    st = ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_aggregate_signature_sets(cache._h, table or b"\0", n_table, idx, offs, k, o192, o96, st))
    return bool(ok), (o192.raw if want192 else None), (o96.raw if want96 else None), st.raw


def aggregateSignatureSets_device(cache, d_sigs, n_table, d_idx, offsets, d_out192, d_out96, stream=0):
    """Same with the signature table, the indices (0 / None: none) and the outputs (0 / None: not wanted; not both) in device memory (raw
    pointers); offsets stay on the host.  d_out192 is what aggregateSets_device / batchFastAggregateVerify_device take as d_sigs.
    -> (all_ok, status bytes)."""
    k = len(offsets) - 1
    if k <= 0:
        return False, b""
    st = ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_aggregate_signature_sets_device(cache._h, d_sigs, n_table, d_idx or None, (ctypes.c_size_t * (k + 1))(*offsets), k,
                                                                d_out192 or None, d_out96 or None, st, stream))
    return bool(ok), st.raw


REC_ZERO_ID, REC_DUP_ID = 6, 7         # status bytes of recoverSignatureSets beyond 0 .. 3


def idFromUint32(words):
    """ID.fromUint32 (blst_recovery.nim): 8 uint32 words, words[0] lowest -> the 32 little-endian bytes of the id."""
    words = [int(w) for w in words]
    if len(words) != 8 or any(w < 0 or w >= 1 << 32 for w in words):
        raise ValueError("an id is 8 uint32 words")
    return b"".join(w.to_bytes(4, "little") for w in words)


def _ids_by_position(ids, n_members):
    """ids: a list of lists of 32-byte ids (one list per group), or their concatenation by position -> n_members x 32 bytes"""
    if isinstance(ids, (bytes, bytearray, memoryview)):
        b = bytes(ids)
        if len(b) % 32:
            raise ValueError("ids: 32 bytes each")
    else:
        flat = []
        for x in ids:
            flat += [bytes(x)] if isinstance(x, (bytes, bytearray, memoryview)) else [bytes(e) for e in x]
        if any(len(e) != 32 for e in flat):
            raise ValueError("ids: 32 bytes each")
        b = b"".join(flat)
    if len(b) != 32 * n_members:
        raise ValueError("one id per member: %d ids for %d members" % (len(b) // 32, n_members))
    return b


def recoverSignatureSets(cache, signatures, ids, want192=True, want96=True):
    """recover(signs, ids) (blst_recovery.nim:150-156) for every group of threshold-signature shares in one device pass
    (mi355_bls_recover_signature_sets); signatures as _signature_lists takes them, ids as a list of lists of 32-byte ids (idFromUint32) or
    their concatenation by sequence position; an id's value is its 256-bit little-endian integer mod r.  -> (all_ok, k x 192-byte
    blst_p2_affine images or None, k x 96-byte wire forms or None, k status bytes: 0 recovered, 1 empty group, 2 the recovered point is
    infinity, 3 index out of range, REC_ZERO_ID, REC_DUP_ID).  VARIABLE TIME: signature shares only, never secret keys."""
    if not (want192 or want96):
        raise ValueError("at least one of the two outputs")
    table, n_table, idx, offs, k = _signature_lists(signatures)
    idb = _ids_by_position(ids, offs[k] if k else 0)
    if k == 0:
        return False, (b"" if want192 else None), (b"" if want96 else None), b""
    o192 = ctypes.create_string_buffer(192 * k) if want192 else None
    o96 = ctypes.create_string_buffer(96 * k) if want96 else None
    st = ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_recover_signature_sets(cache._h, table or b"\0", n_table, idx, offs, k, idb or b"\0", o192, o96, st))
    return bool(ok), (o192.raw if want192 else None), (o96.raw if want96 else None), st.raw


def recoverSignatureSets_device(cache, d_sigs, n_table, d_idx, offsets, d_ids, d_out192, d_out96, stream=0):
    """Same with the share table, the indices (0 / None: none), the ids (32 bytes per sequence position) and the outputs (0 / None: not
    wanted; not both) in device memory (raw pointers); offsets stay on the host.  d_out192 is what aggregateSets_device /
    batchFastAggregateVerify_device take as d_sigs.  -> (all_ok, status bytes)."""
    k = len(offsets) - 1
    if k <= 0:
        return False, b""
    st = ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_recover_signature_sets_device(cache._h, d_sigs, n_table, d_idx or None, (ctypes.c_size_t * (k + 1))(*offsets), k, d_ids,
                                                              d_out192 or None, d_out96 or None, st, stream))
    return bool(ok), st.raw


LINCOMB_SUBGROUP = 1                   # flag of p2sLincombMany: the caller vouches that every point is in G2


def _scalars_by_position(scalars, n_terms):
    """scalars: a list of lists (one per group) of 32-byte little-endian images or of integers below 2^256, or their concatenation by
    position -> n_terms x 32 bytes"""
    if isinstance(scalars, (bytes, bytearray, memoryview)):
        b = bytes(scalars)
    else:
        flat = []
        for x in scalars:
            flat += [x] if isinstance(x, (int, bytes, bytearray, memoryview)) else list(x)
        flat = [int(e).to_bytes(32, "little") if isinstance(e, int) else bytes(e) for e in flat]      # OverflowError is a ValueError's kin: let it out
        if any(len(e) != 32 for e in flat):
            raise ValueError("scalars: 32 bytes each")
        b = b"".join(flat)
    if len(b) != 32 * n_terms:
        raise ValueError("one 32-byte scalar per term: %d bytes for %d terms" % (len(b), n_terms))
    return b


def _lincomb_args(nbits, flags, g2):
    if not 1 <= int(nbits) <= 256:
        raise ValueError("nbits is 1..256")
    if int(flags) & ~(LINCOMB_SUBGROUP if g2 else 0):
        raise ValueError("flags: LINCOMB_SUBGROUP on the G2 call, nothing else")


def _lincomb_many(cache, g2, points, scalars, nbits, flags):
    _lincomb_args(nbits, flags, g2)
    row = 192 if g2 else 96
    table, n_table, idx, offs, k = _signature_lists(points, row, "point")
    sc = _scalars_by_position(scalars, offs[k] if k else 0)
    if k == 0:
        return False, b"", b""
    out, st = ctypes.create_string_buffer(row * k), ctypes.create_string_buffer(k)
    fn = lib().mi355_bls_p2s_lincomb_many if g2 else lib().mi355_bls_p1s_lincomb_many
    ok = _check(fn(cache._h, table or b"\0", n_table, idx, offs, k, sc or b"\0", int(nbits), int(flags), out, st))
    return bool(ok), out.raw, st.raw


def _lincomb_many_device(cache, g2, d_points, n_table, d_idx, offsets, d_scalars, d_out, nbits, flags, stream):
    _lincomb_args(nbits, flags, g2)
    k = len(offsets) - 1
    if k <= 0:
        return False, b""
    st = ctypes.create_string_buffer(k)
    fn = lib().mi355_bls_p2s_lincomb_many_device if g2 else lib().mi355_bls_p1s_lincomb_many_device
    ok = _check(fn(cache._h, d_points, n_table, d_idx or None, (ctypes.c_size_t * (k + 1))(*offsets), k, d_scalars, int(nbits), int(flags), d_out or None, st, stream))
    return bool(ok), st.raw


def p1sLincombMany(cache, points, scalars, nbits=255, flags=0):
    """out[g] = sum_p [s_p mod 2^nbits] P_p for every group of (point, scalar) terms in one device pass (mi355_bls_p1s_lincomb_many): the call
    for many SHORT groups.  points: a list of point lists (96-byte blst_p1_affine images, or their concatenation), or a tuple (table, idx,
    offsets) as aggregateSets takes it; scalars: one per sequence position (_scalars_by_position), never taken through idx.
    -> (all_ok, k x 96-byte affine images, k status bytes: 0 ok, 1 empty group, 2 the sum is infinity, 3 index out of range; any status but 0
    gives the all-zero image).  VARIABLE TIME: public scalars only."""
    return _lincomb_many(cache, False, points, scalars, nbits, flags)


def p2sLincombMany(cache, points, scalars, nbits=255, flags=0):
    """The same on G2 (192-byte blst_p2_affine images; mi355_bls_p2s_lincomb_many).  flags = LINCOMB_SUBGROUP: the caller vouches that every
    point is in G2, and the multiplication walks 64 doublings through the psi endomorphism instead of nbits; with flags = 0 the scalar acts
    as an integer and nothing is assumed about the points."""
    return _lincomb_many(cache, True, points, scalars, nbits, flags)


def p1sLincombMany_device(cache, d_points, n_table, d_idx, offsets, d_scalars, d_out, nbits=255, flags=0, stream=0):
    """Same with the point table, the indices (0 / None: none), the scalars (32 bytes per sequence position) and the output (k x 96 bytes) in
    device memory (raw pointers); offsets stay on the host.  -> (all_ok, status bytes)."""
    return _lincomb_many_device(cache, False, d_points, n_table, d_idx, offsets, d_scalars, d_out, nbits, flags, stream)


def p2sLincombMany_device(cache, d_points, n_table, d_idx, offsets, d_scalars, d_out, nbits=255, flags=0, stream=0):
    """The G2 form (k x 192 bytes out): d_out is, as it stands, the d_q2s argument of pairingCheckEach_device."""
    return _lincomb_many_device(cache, True, d_points, n_table, d_idx, offsets, d_scalars, d_out, nbits, flags, stream)


def debug_lincomb_set_chunk(cache, terms=0):
    """TEST HOOK (mi355_bls_debug_lincomb_set_chunk): the terms per chunk of the following lincomb calls on this context; 0: the plan's own."""
    _check(lib().mi355_bls_debug_lincomb_set_chunk(cache._h, int(terms)))


FR_OPEN_EVAL = 1                       # flag of frOpenMany: the polynomials are given by their values over a domain of n-th roots of unity


def _fr_open_args(n, flags, have_domain):
    n, flags = int(n), int(flags)
    if n < 1:
        raise ValueError("n is at least 1")
    if flags & ~FR_OPEN_EVAL:
        raise ValueError("flags: FR_OPEN_EVAL, nothing else")
    if bool(flags & FR_OPEN_EVAL) != bool(have_domain):
        raise ValueError("the domain goes with FR_OPEN_EVAL: not one without the other")
    if flags and (n & (n - 1) or n > 1 << 32):
        raise ValueError("evaluation form: n is a power of two, at most 2^32")
    return n, flags


def frOpenMany(cache, polys, n, zs, flags=0, domain=None, want_ys=True, want_quot=True):
    """k polynomials of n scalars over Fr opened at k points in one device pass (mi355_bls_fr_open_many): y_g = p_g(z_g) and the quotient
    (p_g(X) - y_g) / (X - z_g).  polys: k x n 32-byte little-endian images, polynomial g at [g n, (g + 1) n); zs: k images; any 256-bit image
    acts as its value mod r.  flags = 0: coefficients, and quotient slot n - 1 is 0 (the padding slot: the table that committed to p serves q).
    flags = FR_OPEN_EVAL: values over `domain`, n images of the n distinct n-th roots of unity in the caller's order, n a power of two - that
    the domain is this set is NOT checked.
    -> (polynomials with status bit 2, k x 32 bytes of y or None, k x n x 32 bytes of quotients or None, k status bytes: 1 z is in the
    domain, 2 an image was >= r and was reduced; both informational).  VARIABLE TIME: public polynomials only.  One workgroup per polynomial:
    a single very long polynomial is correct but slow."""
    n, flags = _fr_open_args(n, flags, domain is not None)
    polys, zs = bytes(polys), bytes(zs)
    if len(zs) % 32:
        raise ValueError("zs: 32 bytes each")
    k = len(zs) // 32
    if len(polys) != k * n * 32:
        raise ValueError("polys: k x n x 32 bytes (%d for k = %d, n = %d)" % (len(polys), k, n))
    if domain is not None and len(domain) != n * 32:
        raise ValueError("domain: n x 32 bytes")
    if not (want_ys or want_quot):
        raise ValueError("values or quotients: ask for one at least")
    if k == 0:
        return 0, b"" if want_ys else None, b"" if want_quot else None, b""
    ys = ctypes.create_string_buffer(32 * k) if want_ys else None
    quot = ctypes.create_string_buffer(32 * k * n) if want_quot else None
    st = ctypes.create_string_buffer(k)
    rc = _check(lib().mi355_bls_fr_open_many(cache._h, polys, n, zs, k, flags, bytes(domain) if domain is not None else None, ys, quot, st))
    return rc, ys.raw if want_ys else None, quot.raw if want_quot else None, st.raw


def frOpenMany_device(cache, d_polys, n, d_zs, k, flags=0, d_domain=None, d_out_ys=None, d_out_quot=None, stream=0, want_status=True):
    """The same with polynomials, points, domain and outputs in device memory (raw pointers; an output of 0 / None is not wanted):
    d_out_quot is, as it stands, the d_scalars argument of p1s_mult_table_many_device and p1s_mult_pippenger_many_device.
    -> (polynomials with status bit 2, status bytes or None)."""
    n, flags = _fr_open_args(n, flags, bool(d_domain))
    k = int(k)
    if k < 0:
        raise ValueError("k is a count")
    if not (d_out_ys or d_out_quot or want_status):
        raise ValueError("every output is None")
    if k == 0:
        return 0, b"" if want_status else None
    if not d_polys or not d_zs:
        raise ValueError("polynomials and points: device pointers")
    st = ctypes.create_string_buffer(k) if want_status else None
    rc = _check(lib().mi355_bls_fr_open_many_device(cache._h, d_polys, n, d_zs, k, flags, d_domain or None, d_out_ys or None, d_out_quot or None, st, stream))
    return rc, st.raw if want_status else None


def debug_fropen_set_pass(cache, polys_per_pass=0):
    """TEST HOOK (mi355_bls_debug_fropen_set_pass): the polynomials per pass of the following frOpenMany calls on this context; 0: the plan's own."""
    _check(lib().mi355_bls_debug_fropen_set_pass(cache._h, int(polys_per_pass)))


FR_NTT_INVERSE = 1                     # flags of frNttMany: values in, coefficients out (the exact inverse map, 1 / n included)
FR_NTT_BITREV = 2                      # the evaluation side is in bit-reversed order: slot i holds the value at omega_n^rev(i)
_FR_R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def _fr_ntt_args(n, flags, shift, allowed=FR_NTT_INVERSE | FR_NTT_BITREV):
    n, flags = int(n), int(flags)
    if n < 1 or n & (n - 1) or n > 1 << 32:
        raise ValueError("n is a power of two, 1 .. 2^32")
    if flags & ~allowed:
        raise ValueError("flags: an unknown bit")
    if shift is not None:
        shift = bytes(shift)
        if len(shift) != 32:
            raise ValueError("shift: one 32-byte image")
        if int.from_bytes(shift, "little") % _FR_R == 0:
            raise ValueError("shift: 0 mod r")
    return n, flags, shift


def frNttMany(cache, vectors, n, flags=0, shift=None):
    """The forward or inverse number-theoretic transform of k vectors of n = 2^m scalars over Fr in one device pass (mi355_bls_fr_ntt_many).
    vectors: k x n 32-byte little-endian images, vector g at [g n, (g + 1) n); any 256-bit image acts as its value mod r.  Forward:
    out[i] = sum_j in[j] (g omega_n^i)^j with omega_n = 7^((r - 1) / n) and g = shift (host bytes; None: 1).  FR_NTT_INVERSE: the exact inverse.
    FR_NTT_BITREV: the evaluation side is bit-reversed.  -> (vectors with status bit 2, k x n x 32 bytes in [0, r), k status bytes: 2 an
    image was >= r and was reduced).  VARIABLE TIME: public vectors only."""
    n, flags, shift = _fr_ntt_args(n, flags, shift)
    vectors = bytes(vectors)
    if len(vectors) % (n * 32):
        raise ValueError("vectors: k x n x 32 bytes (%d for n = %d)" % (len(vectors), n))
    k = len(vectors) // (n * 32)
    if k == 0:
        return 0, b"", b""
    out, st = ctypes.create_string_buffer(len(vectors)), ctypes.create_string_buffer(k)
    rc = _check(lib().mi355_bls_fr_ntt_many(cache._h, vectors, n, k, flags, shift, out, st))
    return rc, out.raw, st.raw


def frNttMany_device(cache, d_in, n, k, flags=0, shift=None, d_out=None, stream=0, want_status=True):
    """The same with the vectors and the output in device memory (raw pointers; d_out None: in place, d_out == d_in); the shift stays host
    bytes.  d_out is, as it stands, the d_polys argument of frOpenMany_device.  -> (vectors with status bit 2, status bytes or None)."""
    n, flags, shift = _fr_ntt_args(n, flags, shift)
    k = int(k)
    if k < 0:
        raise ValueError("k is a count")
    if k == 0:
        return 0, b"" if want_status else None
    if not d_in:
        raise ValueError("vectors: a device pointer")
    st = ctypes.create_string_buffer(k) if want_status else None
    rc = _check(lib().mi355_bls_fr_ntt_many_device(cache._h, d_in, n, k, flags, shift, d_out or d_in, st, stream))
    return rc, st.raw if want_status else None


def frDomain(cache, n, flags=0):
    """The domain frNttMany and frOpenMany's evaluation form speak of (mi355_bls_fr_domain): omega_n^i, or omega_n^rev(i) with FR_NTT_BITREV,
    as n canonical 32-byte images."""
    n, flags, _ = _fr_ntt_args(n, flags, None, FR_NTT_BITREV)
    out = ctypes.create_string_buffer(n * 32)
    _check(lib().mi355_bls_fr_domain(cache._h, n, flags, out))
    return out.raw


def frDomain_device(cache, n, d_out, flags=0, stream=0):
    """The same into device memory (n x 32 bytes at d_out): as it stands the d_domain argument of frOpenMany_device."""
    n, flags, _ = _fr_ntt_args(n, flags, None, FR_NTT_BITREV)
    if not d_out:
        raise ValueError("the output: a device pointer")
    _check(lib().mi355_bls_fr_domain_device(cache._h, n, flags, d_out, stream))


def debug_frntt_set_tile(cache, log2_tile=0):
    """TEST HOOK (mi355_bls_debug_frntt_set_tile): log2 of the tile of the following frNttMany calls on this context; 0: the plan's own."""
    _check(lib().mi355_bls_debug_frntt_set_tile(cache._h, int(log2_tile)))


def debug_frntt_set_pass(cache, vectors_per_pass=0):
    """TEST HOOK (mi355_bls_debug_frntt_set_pass): the vectors per slice of the following frNttMany calls on this context; 0: the plan's own."""
    _check(lib().mi355_bls_debug_frntt_set_pass(cache._h, int(vectors_per_pass)))


P1S_NTT_INVERSE = 1                    # flags of p1sNttMany: the exact inverse map, [1 / n] included
P1S_NTT_BITREV = 2                     # the evaluation side (the forward output, the inverse input) is in bit-reversed order


def p1sNttMany(cache, points, n, flags=0):
    """The forward or inverse number-theoretic transform of k vectors of n = 2^m G1 points in one device pass (mi355_bls_p1s_ntt_many).
    points: k x n 96-byte blst_p1_affine images, vector g at [g n, (g + 1) n); all zero: infinity; the points must be in G1 (not checked).
    Forward: out[i] = sum_j [omega_n^(i j)] P_j with omega_n = 7^((r - 1) / n); P1S_NTT_INVERSE: the exact inverse; P1S_NTT_BITREV: the
    evaluation side is bit-reversed - frNttMany's conventions, so [a_j]G goes to [frNttMany(a)_i]G.  -> k x n canonical affine images.
    VARIABLE TIME: public points only."""
    n, flags, _ = _fr_ntt_args(n, flags, None, P1S_NTT_INVERSE | P1S_NTT_BITREV)
    points = bytes(points)
    if len(points) % (n * 96):
        raise ValueError("points: k x n x 96 bytes (%d for n = %d)" % (len(points), n))
    k = len(points) // (n * 96)
    if k == 0:
        return b""
    out = ctypes.create_string_buffer(len(points))
    _check(lib().mi355_bls_p1s_ntt_many(cache._h, points, n, k, flags, out))
    return out.raw


def p1sNttMany_device(cache, d_in, n, k, flags=0, d_out=None, stream=0):
    """The same with the points and the output in device memory (raw pointers, k x n x 96 bytes each; d_out None: in place, d_out == d_in).
    d_out is, as it stands, a points argument of the MSM and lincomb calls."""
    n, flags, _ = _fr_ntt_args(n, flags, None, P1S_NTT_INVERSE | P1S_NTT_BITREV)
    k = int(k)
    if k < 0:
        raise ValueError("k is a count")
    if k == 0:
        return
    if not d_in:
        raise ValueError("points: a device pointer")
    _check(lib().mi355_bls_p1s_ntt_many_device(cache._h, d_in, n, k, flags, d_out or d_in, stream))


def debug_p1ntt_set_pass(cache, vectors_per_pass=0):
    """TEST HOOK (mi355_bls_debug_p1ntt_set_pass): the vectors per slice of the following p1sNttMany calls on this context; 0: the plan's own."""
    _check(lib().mi355_bls_debug_p1ntt_set_pass(cache._h, int(vectors_per_pass)))


FK20_BITREV = 2                        # flags of fk20OpenAllMany: the proofs in bit-reversed order (P1S_NTT_BITREV's meaning)
FK20_H = 4                             # h_0 .. h_(n-1) instead of the proofs, stopping before the last transform


class Fk20Setup:
    """The setup of the all-openings call (mi355_bls_fk20_setup_create): the handle and its n.  It outlives the cache that made it and serves
    any cache of the same device; fk20_setup_destroy (or destroy()) releases it."""

    def __init__(self, handle, n, cell=1):
        self._h, self.n, self.cell = handle, n, cell

    def destroy(self):
        if self._h:
            lib().mi355_bls_fk20_setup_destroy(self._h)
            self._h = None


def fk20_setup_sizeof(n):
    """device bytes a setup of n points takes (2n x 96); 0 for an n that fk20_setup_create refuses"""
    return lib().mi355_bls_fk20_setup_sizeof(n)


def fk20_setup_create(cache, srs):
    """srs: n = 2^m 96-byte blst_p1_affine images S_j ([tau^j]G for a KZG setup; all zero: infinity; in G1, not checked) -> Fk20Setup"""
    srs = bytes(srs)
    if len(srs) % 96:
        raise ValueError("srs: n x 96 bytes")
    h = ctypes.c_void_p()
    _check(lib().mi355_bls_fk20_setup_create(cache._h, ctypes.byref(h), srs, len(srs) // 96))
    return Fk20Setup(h, len(srs) // 96)


def fk20_setup_create_device(cache, d_srs, n, stream=0):
    """the same with the points in device memory (a pointer as an integer)"""
    h = ctypes.c_void_p()
    _check(lib().mi355_bls_fk20_setup_create_device(cache._h, ctypes.byref(h), d_srs, n, stream))
    return Fk20Setup(h, n)


def fk20_setup_destroy(setup):
    """releases a setup; None: no-op, like mi355_bls_fk20_setup_destroy(NULL)"""
    if setup is None:
        lib().mi355_bls_fk20_setup_destroy(None)
    else:
        setup.destroy()


def _fk20_flags(flags):
    flags = int(flags)
    if flags & ~(FK20_BITREV | FK20_H):
        raise ValueError("flags: FK20_BITREV and FK20_H")
    return flags


def fk20OpenAllMany(cache, setup, polys, flags=0):
    """The KZG proofs of k polynomials at EVERY n-th root of unity in one device pass (mi355_bls_fk20_open_all_many, the Feist-Khovratovich
    route).  polys: k x n 32-byte little-endian coefficient images, n = setup.n; an image >= r acts as its value mod r.  For setup points S_j
    the call gives h_t = sum_{i <= n-2-t} [c_(i+t+1)] S_i and pi_l = sum_t [omega_n^(l t)] h_t; for S_j = [tau^j]G, pi_l is the proof at
    omega_n^l.  FK20_BITREV: slot l holds pi_rev(l); FK20_H: the h_t instead.  -> (polynomials with status bit 2, k x n canonical 96-byte
    affine images, k status bytes: 2 an image was >= r).  VARIABLE TIME: public polynomials only."""
    flags, n = _fk20_flags(flags), setup.n
    polys = bytes(polys)
    if len(polys) % (n * 32):
        raise ValueError("polys: k x n x 32 bytes (%d for n = %d)" % (len(polys), n))
    k = len(polys) // (n * 32)
    if k == 0:
        return 0, b"", b""
    out, st = ctypes.create_string_buffer(k * n * 96), ctypes.create_string_buffer(k)
    rc = _check(lib().mi355_bls_fk20_open_all_many(cache._h, setup._h, polys, k, flags, out, st))
    return rc, out.raw, st.raw


def fk20OpenAllMany_device(cache, setup, d_polys, k, d_out, flags=0, stream=0, want_status=True):
    """The same with the polynomials (k x n x 32 bytes) and the output (k x n x 96 bytes) in device memory, raw pointers.  d_out is, as it
    stands, a points argument of the pairing, MSM and lincomb calls.  -> (polynomials with status bit 2, status bytes or None)."""
    flags, k = _fk20_flags(flags), int(k)
    if k < 0:
        raise ValueError("k is a count")
    if k == 0:
        return 0, b"" if want_status else None
    if not d_polys or not d_out:
        raise ValueError("polys and the output: device pointers")
    st = ctypes.create_string_buffer(k) if want_status else None
    rc = _check(lib().mi355_bls_fk20_open_all_many_device(cache._h, setup._h, d_polys, k, flags, d_out, st, stream))
    return rc, st.raw if want_status else None


def debug_fk20_set_pass(cache, polys_per_pass=0):
    """TEST HOOK (mi355_bls_debug_fk20_set_pass): the polynomials per pass of the following fk20OpenAllMany calls on this context; 0: the plan's own."""
    _check(lib().mi355_bls_debug_fk20_set_pass(cache._h, int(polys_per_pass)))


def fk20_setup_create_cells(cache, srs, cell):
    """The setup of fk20OpenCellsMany for cells of `cell` = 2^c points (mi355_bls_fk20_setup_create_cells).  srs: n = 2^m 96-byte
    blst_p1_affine images S_i, 1 <= cell <= n; cell == 1 is fk20_setup_create.  -> Fk20Setup; with cell > 1 it serves fk20OpenCellsMany only."""
    srs = bytes(srs)
    if len(srs) % 96:
        raise ValueError("srs: n x 96 bytes")
    h = ctypes.c_void_p()
    _check(lib().mi355_bls_fk20_setup_create_cells(cache._h, ctypes.byref(h), srs, len(srs) // 96, int(cell)))
    return Fk20Setup(h, len(srs) // 96, int(cell))


def fk20_setup_create_cells_device(cache, d_srs, n, cell, stream=0):
    """the same with the points in device memory (a pointer as an integer)"""
    h = ctypes.c_void_p()
    _check(lib().mi355_bls_fk20_setup_create_cells_device(cache._h, ctypes.byref(h), d_srs, n, int(cell), stream))
    return Fk20Setup(h, n, int(cell))


def fk20_cells_rows(setup, ext_log2, flags=0):
    """the images one polynomial gives: N = (n / cell) 2^ext_log2 proofs, or n / cell with FK20_H"""
    q = setup.n // setup.cell
    return q if flags & FK20_H else q << int(ext_log2)


def fk20OpenCellsMany(cache, setup, polys, ext_log2=0, flags=0):
    """The KZG proofs of ALL cells of k polynomials in one device pass (mi355_bls_fk20_open_cells_many, the Feist-Khovratovich route over
    cosets).  setup: fk20_setup_create_cells' handle for cells of l = setup.cell points; q = n / l, N = q 2^ext_log2 cells.  polys: k x n
    32-byte little-endian coefficient images; an image >= r acts as its value mod r.  For setup points S_i the call gives
    h_s = sum_{i <= n-1-l(s+1)} [c_(i + l(s+1))] S_i and pi_j = sum_s [omega_N^(j s)] h_s; for S_i = [tau^i]G, pi_j commits to
    p(X) div (X^l - omega_N^j), the multi-proof of the coset x^l = omega_N^j.  FK20_BITREV: slot j holds pi_rev(j) (n = 4096, l = 64,
    ext_log2 = 1: PeerDAS' cell order); FK20_H: the q images h_s instead.  -> (polynomials with status bit 2, k x N (or k x q) canonical
    96-byte affine images, k status bytes: 2 an image was >= r).  VARIABLE TIME: public polynomials only."""
    flags, n, ext_log2 = _fk20_flags(flags), setup.n, int(ext_log2)
    if ext_log2 < 0:
        raise ValueError("ext_log2 is a count")
    polys = bytes(polys)
    if len(polys) % (n * 32):
        raise ValueError("polys: k x n x 32 bytes (%d for n = %d)" % (len(polys), n))
    k = len(polys) // (n * 32)
    if k == 0:
        return 0, b"", b""
    if (n << ext_log2) > 1 << 32:
        raise ValueError("ext_log2: n 2^ext_log2 <= 2^32")
    out, st = ctypes.create_string_buffer(k * fk20_cells_rows(setup, ext_log2, flags) * 96), ctypes.create_string_buffer(k)
    rc = _check(lib().mi355_bls_fk20_open_cells_many(cache._h, setup._h, polys, k, ext_log2, flags, out, st))
    return rc, out.raw, st.raw


def fk20OpenCellsMany_device(cache, setup, d_polys, k, d_out, ext_log2=0, flags=0, stream=0, want_status=True):
    """The same with the polynomials (k x n x 32 bytes) and the output (k x fk20_cells_rows x 96 bytes) in device memory, raw pointers.
    -> (polynomials with status bit 2, status bytes or None)."""
    flags, k, ext_log2 = _fk20_flags(flags), int(k), int(ext_log2)
    if k < 0 or ext_log2 < 0:
        raise ValueError("k and ext_log2 are counts")
    if k == 0:
        return 0, b"" if want_status else None
    if not d_polys or not d_out:
        raise ValueError("polys and the output: device pointers")
    st = ctypes.create_string_buffer(k) if want_status else None
    rc = _check(lib().mi355_bls_fk20_open_cells_many_device(cache._h, setup._h, d_polys, k, ext_log2, flags, d_out, st, stream))
    return rc, st.raw if want_status else None


def compressSignatures(cache, signatures):
    """serialize(Signature) (bls_sig_io.nim:225-234) for n signatures (mi355_bls_compress_signatures): n x 192-byte images -> [96-byte strings]."""
    sg = _join(signatures, 192, "signatures (blst_p2_affine)")
    n = len(sg) // 192
    if n == 0:
        return []
    out = ctypes.create_string_buffer(96 * n)
    _check(lib().mi355_bls_compress_signatures(cache._h, sg, n, out))
    raw = out.raw
    return [raw[96 * i:96 * i + 96] for i in range(n)]


def compressSignatures_device(cache, d_sigs, n, d_out, stream=0):
    """Same with the signatures and the n x 96 output bytes in device memory (raw pointers)."""
    if n:
        _check(lib().mi355_bls_compress_signatures_device(cache._h, d_sigs, n, d_out, stream))


def deserializeSignatures(cache, signatures, sig_uncompressed=False, known_on_curve=False):
    """Signature.fromBytes (bls_sig_io.nim:42-58) for n signatures without key or message (mi355_bls_deserialize_signatures): n x 96 bytes
    (n x 192 with sig_uncompressed); known_on_curve: fromBytesKnownOnCurve.  -> (all_ok, n x 192-byte images, zeroed on failure, status bytes:
    0 ok, 4 bad encoding, 5 not in G2)."""
    unit = 192 if sig_uncompressed else 96
    sg = _join(signatures, unit, "wire signatures")
    n = len(sg) // unit
    if n == 0:
        return True, b"", b""
    flags = (2 if sig_uncompressed else 0) | (4 if known_on_curve else 0)      # DESER_SIG_UNCOMPRESSED, DESER_KNOWN_ON_CURVE
    out, st = ctypes.create_string_buffer(192 * n), ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_deserialize_signatures(cache._h, sg, n, flags, out, st))
    return bool(ok), out.raw, st.raw


def deserializeSignatures_device(cache, d_sigs, n, d_out192, sig_uncompressed=False, known_on_curve=False, stream=0):
    """Same with the wire bytes and the n x 192 output bytes in device memory (raw pointers).  -> (all_ok, status bytes)."""
    if n == 0:
        return True, b""
    flags = (2 if sig_uncompressed else 0) | (4 if known_on_curve else 0)
    st = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_deserialize_signatures_device(cache._h, d_sigs, n, flags, d_out192, st, stream))
    return bool(ok), st.raw


def deserializePublicKeys(cache, publicKeys, pk_uncompressed=False, known_on_curve=False):
    """PublicKey.fromBytes (bls_sig_io.nim:81-99) for n keys without signature or message (mi355_bls_deserialize_public_keys): n x 48 bytes
    (n x 96 with pk_uncompressed); known_on_curve: fromBytesKnownOnCurve.  -> (all_ok, n x 96-byte images, zeroed on failure, status bytes:
    0 ok, 1 bad encoding, 3 infinity, 2 not in G1)."""
    unit = 96 if pk_uncompressed else 48
    pk = _join(publicKeys, unit, "wire public keys")
    n = len(pk) // unit
    if n == 0:
        return True, b"", b""
    flags = (1 if pk_uncompressed else 0) | (4 if known_on_curve else 0)       # DESER_PK_UNCOMPRESSED, DESER_KNOWN_ON_CURVE
    out, st = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_deserialize_public_keys(cache._h, pk, n, flags, out, st))
    return bool(ok), out.raw, st.raw


def deserializePublicKeys_device(cache, d_pks, n, d_out96, pk_uncompressed=False, known_on_curve=False, stream=0):
    """Same with the wire bytes and the n x 96 output bytes in device memory (raw pointers): d_out96 is then the key table the table-addressed
    calls (aggregateSets_device, popVerifyEach_device, ...) take.  -> (all_ok, status bytes)."""
    if n == 0:
        return True, b""
    flags = (1 if pk_uncompressed else 0) | (4 if known_on_curve else 0)
    st = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_deserialize_public_keys_device(cache._h, d_pks, n, flags, d_out96, st, stream))
    return bool(ok), st.raw


KEY_BAD_PROOF = 8                    # status byte of admitKeys beyond the decoders' own: both decode, popVerify is false


def _wire_keys_and_proofs(publicKeys, proofs, pk_uncompressed, sig_uncompressed):
    """n wire keys (48 bytes, 96 uncompressed), n wire proofs (96 bytes, 192 uncompressed), lists or concatenated -> (keys, proofs, n)"""
    ku, pu = (96 if pk_uncompressed else 48), (192 if sig_uncompressed else 96)
    pk, pr = _join(publicKeys, ku, "wire public keys"), _join(proofs, pu, "wire proofs of possession")
    if len(pk) // ku != len(pr) // pu:
        raise ValueError("as many proofs as public keys: got %d keys, %d proofs" % (len(pk) // ku, len(pr) // pu))
    return pk, pr, len(pk) // ku


def admitKeys(cache, publicKeys, proofs, secureRandomBytes, pk_uncompressed=False, sig_uncompressed=False):
    """PublicKey.fromBytes, Signature.fromBytes and popVerify for n (key, proof) rows on the wire (mi355_bls_admit_keys): the admission of
    deposits into the key table.  -> (all_ok, n x 96-byte key table: row i is the key where status[i] == 0 and all zero elsewhere, status bytes:
    0 admitted, 1 / 3 / 2 the key's decoding, 4 / 5 the proof's, KEY_BAD_PROOF).  Only the rows that decode reach the possession check."""
    pk, pr, n = _wire_keys_and_proofs(publicKeys, proofs, pk_uncompressed, sig_uncompressed)
    rnd = _rnd32(secureRandomBytes)
    if n == 0:
        return True, b"", b""
    flags = (1 if pk_uncompressed else 0) | (2 if sig_uncompressed else 0)
    out, st = ctypes.create_string_buffer(96 * n), ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_admit_keys(cache._h, pk, pr, n, flags, rnd, out, st))
    return bool(ok), out.raw, st.raw


def admitKeys_device(cache, d_pks, d_proofs, n, secureRandomBytes, d_out96, pk_uncompressed=False, sig_uncompressed=False, stream=0):
    """Same with both wire columns and the n x 96-byte table in device memory (raw pointers).  -> (all_ok, status bytes)."""
    rnd = _rnd32(secureRandomBytes)
    if n == 0:
        return True, b""
    flags = (1 if pk_uncompressed else 0) | (2 if sig_uncompressed else 0)
    st = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_admit_keys_device(cache._h, d_pks, d_proofs, n, flags, rnd, d_out96, st, stream))
    return bool(ok), st.raw


COMB_MIXED, COMB_INF_KEY = 4, 5      # status bytes of combineSets beyond aggregateSets' own


def _groups(sets, idx, offsets, rnds):
    """The member table, addressing and random bytes of the combineSets family -> (records, n_sets, idx array or None, offsets array, k,
    rnds).  sets: n x 320-byte SignatureSet records; idx: None or a sequence of table indices; offsets: k + 1 non-decreasing positions (into
    idx, or into the table when idx is None); rnds: k x 32 bytes (or a list of k 32-byte strings), secureRandomBytes of every group."""
    b = _as_records(sets)
    offsets = [int(x) for x in offsets]
    if not offsets or any(x < 0 for x in offsets):
        raise ValueError("offsets: k + 1 non-negative positions")
    k = len(offsets) - 1
    if idx is not None:
        idx = [int(x) for x in idx]
        if any(x < 0 or x >= 1 << 32 for x in idx):
            raise ValueError("indices are 32-bit unsigned")
        if offsets[-1] != len(idx):
            raise ValueError("offsets[k] is the length of the index array")
    r = _join(rnds, 32, "rnds")
    if len(r) != 32 * k:
        raise ValueError("32 random bytes per group")
    iarr = (ctypes.c_uint32 * max(len(idx), 1))(*idx) if idx is not None else None
    return b, len(b) // SIGSET_BYTES, iarr, (ctypes.c_size_t * (k + 1))(*offsets), k, r


def combineSets(cache, sets, idx, offsets, rnds):
    """MultiSignatureSet.combine (bls_batch_verifier.nim:47-106) for every group in one device pass (mi355_bls_combine_sets); arguments as
    _groups takes them.  -> (all_ok, k x 320-byte combined records, k status bytes: 0 ok, 1 empty group, 2 combined key at infinity, 3 index
    out of range, 4 mixed messages, 5 a member with the infinity key; a record whose status is not 0 carries the infinity key)."""
    b, n, iarr, offs, k, r = _groups(sets, idx, offsets, rnds)
    if k == 0:
        return False, b"", b""
    out, st = ctypes.create_string_buffer(320 * k), ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_combine_sets(cache._h, b or b"\0", n, iarr, offs, k, r, out, st))
    return bool(ok), out.raw, st.raw


def combineSets_device(cache, d_sets, n_sets, d_idx, offsets, rnds, d_out, stream=0):
    """Same with the member table, the indices (0 / None: none) and the output records in device memory (raw pointers); offsets and rnds
    stay on the host.  -> (all_ok, status bytes)."""
    k = len(offsets) - 1
    if k <= 0:
        return False, b""
    r = _join(rnds, 32, "rnds")
    if len(r) != 32 * k:
        raise ValueError("32 random bytes per group")
    st = ctypes.create_string_buffer(k)
    ok = _check(lib().mi355_bls_combine_sets_device(cache._h, d_sets, n_sets, d_idx or None, (ctypes.c_size_t * (k + 1))(*offsets), k, r, d_out, st, stream))
    return bool(ok), st.raw


def batchVerifyCombined(cache, sets, idx, offsets, rnds, secureRandomBytes):
    """combineSets, then batchVerify with secureRandomBytes over the k combined records (mi355_bls_batch_verify_combined): False when a
    group gives no record (any status but 0) or the batch does not verify; no groups -> False."""
    rnd = _rnd32(secureRandomBytes)
    b, n, iarr, offs, k, r = _groups(sets, idx, offsets, rnds)
    if k == 0:
        return False
    return bool(_check(lib().mi355_bls_batch_verify_combined(cache._h, b or b"\0", n, iarr, offs, k, r, rnd)))


def batchVerifyCombined_device(cache, d_sets, n_sets, d_idx, offsets, rnds, secureRandomBytes, stream=0):
    rnd = _rnd32(secureRandomBytes)
    k = len(offsets) - 1
    if k <= 0:
        return False
    r = _join(rnds, 32, "rnds")
    if len(r) != 32 * k:
        raise ValueError("32 random bytes per group")
    return bool(_check(lib().mi355_bls_batch_verify_combined_device(cache._h, d_sets, n_sets, d_idx or None, (ctypes.c_size_t * (k + 1))(*offsets), k, r, rnd,
                                                                    stream)))


def groupByMessage(sets):
    """The records of a flat batch grouped by their 32-byte message, stably (mi355_bls_group_by_message; host only, no GPU): -> (idx,
    offsets), groups in the order their message first appears, members in input order - what combineSets takes with the batch as table."""
    b = _as_records(sets)
    n = len(b) // SIGSET_BYTES
    idx, offs, k = (ctypes.c_uint32 * max(n, 1))(), (ctypes.c_size_t * (n + 1))(), ctypes.c_size_t(0)
    _check(lib().mi355_bls_group_by_message(b or b"\0", n, idx, offs, ctypes.byref(k)))
    return list(idx)[:n], list(offs)[:k.value + 1]


def verifyAggregate(cache, aggregate_p1, message, signature):
    """coreVerifyNoGroupCheck (core :269-297) on a 144-byte blst_p1 aggregate public key the caller holds."""
    if len(aggregate_p1) != 144 or len(signature) != 192:
        raise ValueError("aggregate: 144-byte blst_p1, signature: 192-byte blst_p2_affine")
    return bool(_check(lib().mi355_bls_verify_aggregate(cache._h, bytes(aggregate_p1), bytes(message), len(message), bytes(signature))))


def p1s_mult_pippenger(cache, points, scalars, nbits=255):
    """blst_p1s_mult_pippenger shape (benchmarks/bls12381_msm_g1.nim:50-59): points = n x 96-byte affine,
    scalars = n x 32-byte little-endian; returns the 144-byte blst_p1 (Jacobian) result."""
    if len(points) % 96 or len(scalars) % 32 or len(points) // 96 != len(scalars) // 32:
        raise ValueError("points: n x 96 bytes, scalars: n x 32 bytes")
    n = len(points) // 96
    pb = ctypes.create_string_buffer(bytes(points), len(points)) if n else None
    sb = ctypes.create_string_buffer(bytes(scalars), len(scalars)) if n else None
    pl = (ctypes.c_void_p * 2)(ctypes.addressof(pb) if n else None, None)       # [ptr, NULL]
    sl = (ctypes.c_void_p * 2)(ctypes.addressof(sb) if n else None, None)
    out = ctypes.create_string_buffer(144)
    _check(lib().mi355_bls_p1s_mult_pippenger(cache._h, out, pl, n, sl, nbits))
    return out.raw


def blst_p1s_mult_pippenger(points, scalars, nbits=255, per_element_pointers=False, g2=False):
    """mi355_p1s_mult_pippenger / mi355_p2s_mult_pippenger (g2=True): EXACTLY blst_pNs_mult_pippenger's argument list (no
    context, void, scalars (nbits + 7) // 8 bytes apart, NULL-terminated pointer lists).  per_element_pointers: pass one
    pointer per element instead of [ptr, NULL] (both are blst conventions).  Returns the 144-byte blst_p1 / 288-byte blst_p2."""
    sb = (nbits + 7) // 8
    ab = 192 if g2 else 96
    fn = lib().mi355_p2s_mult_pippenger if g2 else lib().mi355_p1s_mult_pippenger
    if len(points) % ab or len(scalars) % sb or len(points) // ab != len(scalars) // sb:
        raise ValueError("points: n x %d bytes, scalars: n x %d bytes" % (ab, sb))
    n = len(points) // ab
    out = ctypes.create_string_buffer(288 if g2 else 144)
    if n == 0:
        fn(out, None, 0, None, nbits, None)
        return out.raw
    pb = ctypes.create_string_buffer(bytes(points), len(points))
    scb = ctypes.create_string_buffer(bytes(scalars), len(scalars))
    pa, sa = ctypes.addressof(pb), ctypes.addressof(scb)
    if per_element_pointers:
        pl = (ctypes.c_void_p * n)(*[pa + ab * i for i in range(n)])
        sl = (ctypes.c_void_p * n)(*[sa + sb * i for i in range(n)])
    else:
        pl = (ctypes.c_void_p * 2)(pa, None)
        sl = (ctypes.c_void_p * 2)(sa, None)
    scratch = ctypes.create_string_buffer(max(8, lib().mi355_p1s_mult_pippenger_scratch_sizeof(n)))
    fn(out, pl, n, sl, nbits, scratch)
    return out.raw


def blst_p2s_mult_pippenger(points, scalars, nbits=255, per_element_pointers=False):
    return blst_p1s_mult_pippenger(points, scalars, nbits, per_element_pointers, g2=True)


def p2s_mult_pippenger_device(cache, d_points, n, d_scalars, nbits=255, stream=0):
    out = ctypes.create_string_buffer(288)
    _check(lib().mi355_bls_p2s_mult_pippenger_device(cache._h, out, d_points, n, d_scalars, nbits, stream))
    return out.raw


def p1s_mult_pippenger_device(cache, d_points, n, d_scalars, nbits=255, stream=0):
    out = ctypes.create_string_buffer(144)
    _check(lib().mi355_bls_p1s_mult_pippenger_device(cache._h, out, d_points, n, d_scalars, nbits, stream))
    return out.raw


def _many_offsets(offsets, npoints):
    offs = [int(v) for v in offsets]
    if not offs or offs[0] != 0 or offs[-1] != npoints or any(b < a for a, b in zip(offs, offs[1:])):
        raise ValueError("offsets: k + 1 non-decreasing values from 0 to the number of points")
    return offs


def p1s_mult_pippenger_many(cache, points, scalars, offsets=None, nbits=255):
    """k G1 MSMs in one device pass -> a list of k 144-byte blst_p1 (Jacobian) results.  offsets (k + 1 values): MSM j is over points and
    scalars [offsets[j], offsets[j + 1]).  offsets=None: every MSM is over all n points, scalars = k x n x 32 bytes, MSM j uses scalars
    [j n, (j + 1) n)."""
    if len(points) % 96 or len(scalars) % 32:
        raise ValueError("points: n x 96 bytes, scalars: 32 bytes each")
    n, ns = len(points) // 96, len(scalars) // 32
    if offsets is None:
        if n == 0 or ns % n:
            if ns:
                raise ValueError("shared points: scalars must be k x n x 32 bytes")
            return []
        k, arr = ns // n, None
    else:
        offs = _many_offsets(offsets, n)
        if ns != n:
            raise ValueError("ragged: one 32-byte scalar per point")
        k, arr = len(offs) - 1, (ctypes.c_size_t * len(offs))(*offs)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(144 * k)
    _check(lib().mi355_bls_p1s_mult_pippenger_many(cache._h, out, bytes(points), n, bytes(scalars), arr, k, nbits))
    return [out.raw[144 * j:144 * j + 144] for j in range(k)]


def p1s_mult_pippenger_many_device(cache, d_points, npoints, d_scalars, offsets, k, nbits=255, d_out=None, stream=0):
    """The same with both arrays in device memory (pointers as integers); offsets as above or None.  The results come back as a list and,
    when d_out (a device pointer to k x 144 bytes) is given, are left there as well."""
    if k == 0:
        return []
    arr = None
    if offsets is not None:
        offs = _many_offsets(offsets, npoints)
        if len(offs) != k + 1:
            raise ValueError("offsets: k + 1 values")
        arr = (ctypes.c_size_t * len(offs))(*offs)
    out = ctypes.create_string_buffer(144 * k)
    _check(lib().mi355_bls_p1s_mult_pippenger_many_device(cache._h, out, d_out, d_points, npoints, d_scalars, arr, k, nbits, stream))
    return [out.raw[144 * j:144 * j + 144] for j in range(k)]


def p2s_mult_pippenger_many(cache, points, scalars, offsets=None, nbits=255):
    """k G2 MSMs in one device pass -> a list of k 288-byte blst_p2 (Jacobian) results: p1s_mult_pippenger_many over 192-byte
    blst_p2_affine images, the same two addressing forms."""
    if len(points) % 192 or len(scalars) % 32:
        raise ValueError("points: n x 192 bytes, scalars: 32 bytes each")
    n, ns = len(points) // 192, len(scalars) // 32
    if offsets is None:
        if n == 0 or ns % n:
            if ns:
                raise ValueError("shared points: scalars must be k x n x 32 bytes")
            return []
        k, arr = ns // n, None
    else:
        offs = _many_offsets(offsets, n)
        if ns != n:
            raise ValueError("ragged: one 32-byte scalar per point")
        k, arr = len(offs) - 1, (ctypes.c_size_t * len(offs))(*offs)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(288 * k)
    _check(lib().mi355_bls_p2s_mult_pippenger_many(cache._h, out, bytes(points), n, bytes(scalars), arr, k, nbits))
    return [out.raw[288 * j:288 * j + 288] for j in range(k)]


def p2s_mult_pippenger_many_device(cache, d_points, npoints, d_scalars, offsets, k, nbits=255, d_out=None, stream=0, ret=True):
    """The same with both arrays in device memory (pointers as integers); offsets as above or None.  The results come back as a list
    (ret=False: nothing is copied to the host and None is returned) and, when d_out (a device pointer to k x 288 bytes) is given, are left
    there as well."""
    if k == 0:
        return []
    arr = None
    if offsets is not None:
        offs = _many_offsets(offsets, npoints)
        if len(offs) != k + 1:
            raise ValueError("offsets: k + 1 values")
        arr = (ctypes.c_size_t * len(offs))(*offs)
    out = ctypes.create_string_buffer(288 * k) if ret else None
    _check(lib().mi355_bls_p2s_mult_pippenger_many_device(cache._h, out, d_out, d_points, npoints, d_scalars, arr, k, nbits, stream))
    return [out.raw[288 * j:288 * j + 288] for j in range(k)] if ret else None


def _to_affine(cache, name, jacb, images):
    if len(images) % jacb:
        raise ValueError("Jacobian images: n x %d bytes" % jacb)
    n = len(images) // jacb
    if n == 0:
        return b""
    out = ctypes.create_string_buffer(jacb // 3 * 2 * n)
    _check(getattr(lib(), name)(cache._h, bytes(images), n, out))
    return out.raw


def p1s_to_affine(cache, images):
    """n x 144 bytes of blst_p1 (Jacobian) images -> n x 96 bytes of blst_p1_affine images; Z == 0 gives 96 zero bytes."""
    return _to_affine(cache, "mi355_bls_p1s_to_affine", 144, images)


def p2s_to_affine(cache, images):
    """n x 288 bytes of blst_p2 (Jacobian) images -> n x 192 bytes of blst_p2_affine images; Z == 0 gives 192 zero bytes."""
    return _to_affine(cache, "mi355_bls_p2s_to_affine", 288, images)


def p1s_to_affine_device(cache, d_in, n, d_out, stream=0):
    """The same between device buffers (pointers as integers, 4-byte aligned, not overlapping): d_out takes n x 96 bytes."""
    _check(lib().mi355_bls_p1s_to_affine_device(cache._h, d_in or None, n, d_out or None, stream))


def p2s_to_affine_device(cache, d_in, n, d_out, stream=0):
    """The same between device buffers: d_out takes n x 192 bytes."""
    _check(lib().mi355_bls_p2s_to_affine_device(cache._h, d_in or None, n, d_out or None, stream))


def debug_to_affine_set_run(cache, run=0):
    """TEST HOOK: the points a lane of the following to_affine calls takes (capped at 8; 0: the plan's own)."""
    _check(lib().mi355_bls_debug_to_affine_set_run(cache._h, run))


class P1sTable:
    """A fixed-base window table (mi355_bls_p1s_table_create): the handle and the parameters it was asked for.  It outlives the cache that
    made it; p1s_table_destroy (or destroy()) releases it."""

    def __init__(self, handle, npoints, wbits, nbits):
        self._h, self.npoints, self.wbits, self.nbits = handle, npoints, wbits, nbits

    def destroy(self):
        if self._h:
            lib().mi355_bls_p1s_table_destroy(self._h)
            self._h = None


def p1s_table_sizeof(npoints, wbits=0, nbits=255):
    """device bytes a table takes; 0 for arguments p1s_table_create refuses"""
    return lib().mi355_bls_p1s_table_sizeof(npoints, wbits, nbits)


def p1s_table_create(cache, points, wbits=0, nbits=255):
    """blst_p1s_mult_wbits_precompute: the rows [2^(w wbits)] P_i of n 96-byte affine points -> P1sTable.  wbits 5..16, or 0: the plan's rule."""
    if len(points) % 96:
        raise ValueError("points: n x 96 bytes")
    n = len(points) // 96
    h = ctypes.c_void_p()
    _check(lib().mi355_bls_p1s_table_create(cache._h, ctypes.byref(h), bytes(points), n, wbits, nbits))
    return P1sTable(h, n, wbits, nbits)


def p1s_table_create_device(cache, d_points, npoints, wbits=0, nbits=255, stream=0):
    """the same with the points in device memory (a pointer as an integer)"""
    h = ctypes.c_void_p()
    _check(lib().mi355_bls_p1s_table_create_device(cache._h, ctypes.byref(h), d_points, npoints, wbits, nbits, stream))
    return P1sTable(h, npoints, wbits, nbits)


def p1s_table_destroy(table):
    if table is not None:
        table.destroy()


def p1s_mult_table(cache, table, scalars, nbits=255):
    """blst_p1s_mult_wbits: sum_i [k_i mod 2^nbits] P_i over the table's points -> the 144-byte blst_p1; scalars: n x 32 bytes"""
    if len(scalars) != 32 * table.npoints:
        raise ValueError("scalars: one 32-byte scalar per point of the table")
    out = ctypes.create_string_buffer(144)
    _check(lib().mi355_bls_p1s_mult_table(cache._h, out, table._h, bytes(scalars), nbits))
    return out.raw


def p1s_mult_table_device(cache, table, d_scalars, nbits=255, stream=0):
    out = ctypes.create_string_buffer(144)
    _check(lib().mi355_bls_p1s_mult_table_device(cache._h, out, table._h, d_scalars, nbits, stream))
    return out.raw


def p1s_mult_table_many(cache, table, scalars, nbits=255):
    """k MSMs over the one table -> a list of k 144-byte blst_p1 results; scalars: k x n x 32 bytes, MSM j uses [j n, (j + 1) n)"""
    if len(scalars) % (32 * table.npoints):
        raise ValueError("scalars: k x n x 32 bytes")
    k = len(scalars) // (32 * table.npoints)
    if k == 0:
        return []
    out = ctypes.create_string_buffer(144 * k)
    _check(lib().mi355_bls_p1s_mult_table_many(cache._h, out, table._h, bytes(scalars), k, nbits))
    return [out.raw[144 * j:144 * j + 144] for j in range(k)]


def p1s_mult_table_many_device(cache, table, d_scalars, k, nbits=255, d_out=None, stream=0):
    """The same with the scalars in device memory; the results come back as a list and, when d_out (a device pointer to k x 144 bytes) is
    given, are left there as well."""
    if k == 0:
        _check(lib().mi355_bls_p1s_mult_table_many_device(cache._h, None, d_out, table._h, d_scalars, 0, nbits, stream))
        return []
    out = ctypes.create_string_buffer(144 * k)
    _check(lib().mi355_bls_p1s_mult_table_many_device(cache._h, out, d_out, table._h, d_scalars, k, nbits, stream))
    return [out.raw[144 * j:144 * j + 144] for j in range(k)]


def debug_p1s_table_rows(table, w0, nw, i0, ni):
    """TEST HOOK: rows [w0, w0 + nw) x points [i0, i0 + ni) as a list of nw lists of ni 96-byte affine images"""
    out = ctypes.create_string_buffer(max(1, 96 * nw * ni))
    _check(lib().mi355_bls_debug_p1s_table_rows(table._h, w0, nw, i0, ni, out))
    return [[out.raw[96 * (r * ni + c):96 * (r * ni + c + 1)] for c in range(ni)] for r in range(nw)]


def debug_p1s_table_last_plan(cache):
    """TEST HOOK: (W, S, buckets per set) of the last table mult call on this cache"""
    out = (ctypes.c_uint32 * 3)()
    _check(lib().mi355_bls_debug_p1s_table_last_plan(cache._h, out))
    return tuple(out)


def debug_p1s_table_set_plan(cache, force_sets=0, pairs_max=0):
    """TEST HOOK: bucket sets per MSM and pairs per pass of the following table mult calls on this cache (0: the plan's own)"""
    _check(lib().mi355_bls_debug_p1s_table_set_plan(cache._h, force_sets, pairs_max))


def _split_compressed(pubkeys, messages, signatures):
    pk = bytes(pubkeys) if isinstance(pubkeys, (bytes, bytearray, memoryview)) else b"".join(pubkeys)
    ms = bytes(messages) if isinstance(messages, (bytes, bytearray, memoryview)) else b"".join(messages)
    sg = bytes(signatures) if isinstance(signatures, (bytes, bytearray, memoryview)) else b"".join(signatures)
    if len(pk) % 48 or len(ms) % 32 or len(sg) % 96 or not (len(pk) // 48 == len(ms) // 32 == len(sg) // 96):
        raise ValueError("n x 48-byte compressed keys, n x 32-byte messages, n x 96-byte compressed signatures")
    return pk, ms, sg, len(pk) // 48


def deserializeSets(cache, pubkeys, messages, signatures):
    """Batched PublicKey.fromBytes / Signature.fromBytes (bls_sig_io.nim:42-58,81-99).
    -> (all_ok, n x 320-byte SignatureSet records, per-tuple status bytes)."""
    pk, ms, sg, n = _split_compressed(pubkeys, messages, signatures)
    if n == 0:
        return True, b"", b""
    out = ctypes.create_string_buffer(320 * n)
    st = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_deserialize_sets(cache._h, pk, ms, sg, n, out, st))
    return bool(ok), out.raw, st.raw


DESER_PK_UNCOMPRESSED, DESER_SIG_UNCOMPRESSED, DESER_KNOWN_ON_CURVE = 1, 2, 4


def deserializeSetsEx(cache, pubkeys, messages, signatures, pk_uncompressed=False, sig_uncompressed=False, known_on_curve=False):
    """The other forms of fromBytes (bls_sig_io.nim:42-121): 96-byte keys / 192-byte signatures (blst_pN_deserialize) and
    fromBytesKnownOnCurve (no subgroup checks).  -> (all_ok, records, status bytes)."""
    pk = bytes(pubkeys) if isinstance(pubkeys, (bytes, bytearray, memoryview)) else b"".join(pubkeys)
    ms = bytes(messages) if isinstance(messages, (bytes, bytearray, memoryview)) else b"".join(messages)
    sg = bytes(signatures) if isinstance(signatures, (bytes, bytearray, memoryview)) else b"".join(signatures)
    pkb, sgb = (96 if pk_uncompressed else 48), (192 if sig_uncompressed else 96)
    n = len(ms) // 32
    if len(ms) % 32 or len(pk) != pkb * n or len(sg) != sgb * n:
        raise ValueError("n x %d-byte keys, n x 32-byte messages, n x %d-byte signatures" % (pkb, sgb))
    if n == 0:
        return True, b"", b""
    flags = (DESER_PK_UNCOMPRESSED if pk_uncompressed else 0) | (DESER_SIG_UNCOMPRESSED if sig_uncompressed else 0) | (DESER_KNOWN_ON_CURVE if known_on_curve else 0)
    out = ctypes.create_string_buffer(320 * n)
    st = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_deserialize_sets_ex(cache._h, pk, ms, sg, n, flags, out, st))
    return bool(ok), out.raw, st.raw


def batchVerifyCompressed(cache, pubkeys, messages, signatures, secureRandomBytes):
    """fromBytes for every tuple, then batchVerify, on the device.  -> (verdict, per-tuple status bytes)."""
    pk, ms, sg, n = _split_compressed(pubkeys, messages, signatures)
    if n == 0:
        return False, b""
    st = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_batch_verify_compressed(cache._h, pk, ms, sg, n, _rnd32(secureRandomBytes), st))
    return bool(ok), st.raw


def signSets(cache, secret_keys, messages):
    """Batch signer / input generator: per tuple publicFromSecret + coreSign
    (blst_min_pubkey_sig_core.nim:118-133, :230-251) on the device, VARIABLE TIME (test and bench inputs only).
    secret_keys: n x 32-byte little-endian scalars, messages: n x 32 bytes (lists or concatenated).
    -> (all_valid, n x 320-byte SignatureSet records, per-tuple status bytes: 1 = sk == 0 or sk >= r)."""
    sk = secret_keys if isinstance(secret_keys, (bytes, bytearray)) else b"".join(bytes(x) for x in secret_keys)
    ms = messages if isinstance(messages, (bytes, bytearray)) else b"".join(bytes(x) for x in messages)
    assert len(sk) % 32 == 0 and len(ms) == len(sk)
    n = len(sk) // 32
    if n == 0:
        return True, b"", b""
    out = ctypes.create_string_buffer(320 * n)
    st = ctypes.create_string_buffer(n)
    ok = _check(lib().mi355_bls_sign_sets(cache._h, bytes(sk), bytes(ms), n, out, st))
    return bool(ok), out.raw, st.raw


def signSets_device(cache, d_sks, d_msgs, n, d_out, stream=0):
    """Same with the scalars, messages and the output records resident in device memory (raw pointers)."""
    st = ctypes.create_string_buffer(max(n, 1))
    ok = _check(lib().mi355_bls_sign_sets_device(cache._h, d_sks, d_msgs, n, d_out, stream, st))
    return bool(ok), st.raw[:n]


class MultiSignatureSet:
    """bls_batch_verifier.nim:47-106: signatures that all pertain to the same 32-byte message."""

    def __init__(self, pubkeys, message, signatures):
        pubkeys, signatures = list(pubkeys), list(signatures)
        assert len(pubkeys) == len(signatures) and len(pubkeys) > 0          # doAssert :80-81
        self.pubkeys, self.message, self.signatures = pubkeys, bytes(message), signatures

    @classmethod
    def init(cls, pubkeys, message=None, signatures=None):
        if message is None:                       # init(sigset: SignatureSet)  (:89-94)
            pk, msg, sig = pubkeys
            return cls([pk], msg, [sig])
        return cls(pubkeys, message, signatures)

    def add(self, sigset):
        pk, msg, sig = sigset
        assert bytes(msg) == self.message                                     # doAssert :97
        self.pubkeys.append(pk)
        self.signatures.append(sig)

    def combine(self, cache, secureRandomBytes):
        """-> SignatureSet (pubkey96, message32, signature192)."""
        n = len(self.pubkeys)
        out_pk, out_sig = ctypes.create_string_buffer(96), ctypes.create_string_buffer(192)
        _check(lib().mi355_bls_combine(cache._h, _rnd32(secureRandomBytes), b"".join(self.pubkeys), b"".join(self.signatures), n, out_pk, out_sig))
        return (out_pk.raw, self.message, out_sig.raw)


def aggregateVerify(cache, publicKeys, messages, signature):
    """bls_sig_min_pubkey.nim:153-174: one aggregate signature over distinct (public key, message) pairs.
    Length mismatch or an empty list -> False."""
    pks, msgs = list(publicKeys), [bytes(x) for x in messages]
    if len(pks) != len(msgs) or len(pks) == 0:
        return False
    if any(len(p) != 96 for p in pks) or len(signature) not in (192, 288):
        raise ValueError("public keys are 96-byte; the signature a 192-byte Signature (affine) or a 288-byte AggregateSignature (blst_p2)")
    offs = [0]
    for x in msgs:
        offs.append(offs[-1] + len(x))
    arr = (ctypes.c_uint32 * len(offs))(*offs)
    fn = lib().mi355_bls_aggregate_verify if len(signature) == 192 else lib().mi355_bls_aggregate_verify_p2
    return bool(_check(fn(cache._h, b"".join(pks), b"".join(msgs) or b"\0", arr, len(pks), bytes(signature))))


class ContextCoreAggregateVerify:
    """blst_min_pubkey_sig_core.nim:305-414, the streaming form of aggregateVerify: init() / update(publicKey, message) -> bool /
    finish(signature) -> bool, on a BatchedBLSVerifierCache's device context (mi355_bls_aggv_*)."""

    def __init__(self, cache):
        self._c = cache

    def init(self):
        _check(lib().mi355_bls_aggv_init(self._c._h))

    def update(self, publicKey, message):
        if len(publicKey) != 96:
            raise ValueError("public keys are 96-byte blst_p1_affine images")
        m = bytes(message)
        return bool(_check(lib().mi355_bls_aggv_update(self._c._h, bytes(publicKey), m or None, len(m))))

    def finish(self, signature):
        """finish(signature: Signature or AggregateSignature) (core :357): 192-byte affine or 288-byte Jacobian image"""
        if len(signature) == 288:
            return bool(_check(lib().mi355_bls_aggv_finish_p2(self._c._h, bytes(signature))))
        if len(signature) != 192:
            raise ValueError("the signature is a 192-byte blst_p2_affine or a 288-byte blst_p2 image")
        return bool(_check(lib().mi355_bls_aggv_finish(self._c._h, bytes(signature))))


def aggregateVerifyStreaming(cache, publicKeys, messages, signature):
    """aggregateVerify written as the reference writes it (bls_sig_min_pubkey.nim:153-174): ctx.init, one update per pair, finish."""
    pks, msgs = list(publicKeys), list(messages)
    if len(pks) != len(msgs) or len(pks) == 0:
        return False
    ctx = ContextCoreAggregateVerify(cache)
    ctx.init()
    for pk, m in zip(pks, msgs):
        if not ctx.update(pk, m):
            return False
    return ctx.finish(signature)


def msm_shard_range(npoints, world, rank):
    first, count = ctypes.c_size_t(), ctypes.c_size_t()
    lib().mi355_bls_msm_shard_range(npoints, world, rank, ctypes.byref(first), ctypes.byref(count))
    return first.value, count.value


def p1s_mult_pippenger_multi(caches, points, scalars, nbits=255, g2=False):
    """blst_p1s_mult_pippenger (g2: blst_p2s) point-sharded over several devices from one host thread: caches[g] lives on device g."""
    ab = 192 if g2 else 96
    if len(points) % ab or len(scalars) % 32 or len(points) // ab != len(scalars) // 32:
        raise ValueError("points: n x %d bytes, scalars: n x 32 bytes" % ab)
    n = len(points) // ab
    arr = (ctypes.c_void_p * len(caches))(*[c._h for c in caches])
    pb = ctypes.create_string_buffer(bytes(points), len(points)) if n else None
    sb = ctypes.create_string_buffer(bytes(scalars), len(scalars)) if n else None
    pl = (ctypes.c_void_p * 2)(ctypes.addressof(pb) if n else None, None)
    sl = (ctypes.c_void_p * 2)(ctypes.addressof(sb) if n else None, None)
    out = ctypes.create_string_buffer(288 if g2 else 144)
    fn = lib().mi355_bls_p2s_mult_pippenger_multi if g2 else lib().mi355_bls_p1s_mult_pippenger_multi
    _check(fn(arr, len(caches), out, pl, n, sl, nbits))
    return out.raw


def p1s_mult_pippenger_multi_device(caches, d_points, n, d_scalars, nbits=255):
    """Same with shard g's arrays (msm_shard_range(n, len(caches), g)) already resident on device g: d_points[g], d_scalars[g]."""
    arr = (ctypes.c_void_p * len(caches))(*[c._h for c in caches])
    dp = (ctypes.c_void_p * len(caches))(*d_points)
    ds = (ctypes.c_void_p * len(caches))(*d_scalars)
    out = ctypes.create_string_buffer(144)
    _check(lib().mi355_bls_p1s_mult_pippenger_multi_device(arr, len(caches), out, dp, n, ds, nbits))
    return out.raw


def p1s_mult_pippenger_partial_device(cache, d_out, d_points, n, d_scalars, nbits=255, stream=0):
    """This device's partial of a point-sharded MSM, left at d_out (144 B, device memory) behind the rest of `stream`."""
    _check(lib().mi355_bls_p1s_mult_pippenger_partial_device(cache._h, d_out, d_points, n, d_scalars, nbits, stream))


def p1s_add(cache, parts, g2=False):
    """Sum of k blst_p1 (g2: blst_p2) Jacobian images (blst_p1_add_or_double, blst_abi.nim:278): the merge of MSM partials."""
    jb = 288 if g2 else 144
    buf = bytes(parts) if isinstance(parts, (bytes, bytearray, memoryview)) else b"".join(parts)
    if len(buf) % jb or not buf:
        raise ValueError("k x %d-byte Jacobian images" % jb)
    out = ctypes.create_string_buffer(jb)
    _check((lib().mi355_bls_p2s_add if g2 else lib().mi355_bls_p1s_add)(cache._h, out, buf, len(buf) // jb))
    return out.raw


def p1s_add_device(cache, d_parts, k, stride=144, stream=0):
    out = ctypes.create_string_buffer(144)
    _check(lib().mi355_bls_p1s_add_device(cache._h, out, d_parts, k, stride, stream))
    return out.raw
