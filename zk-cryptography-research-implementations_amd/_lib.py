"""Loads libzkmle_amd.so and declares the C ABI of include/zkmle.h.  Fails loudly if it is absent."""
import ctypes as C
import os

FR381, FQ381, BN254_FQ, BN254_FR = 0, 1, 2, 3
FIELD_NAMES = {FR381: "bls12_381_fr", FQ381: "bls12_381_fq", BN254_FQ: "bn254_fq", BN254_FR: "bn254_fr"}

ZK_OK = 0
ZK_E_NOT_POW2, ZK_E_LEN_MISMATCH, ZK_E_NVARS, ZK_E_NEED_TWO, ZK_E_KZG_LEN, ZK_E_RANGE = -1, -2, -3, -4, -5, -6
ZK_E_ARG, ZK_E_NOMEM, ZK_E_NO_DEVICE, ZK_E_HIP, ZK_E_NOT_INIT, ZK_E_COMM = -7, -8, -9, -10, -11, -12
_PANIC_CODES = {ZK_E_NOT_POW2, ZK_E_LEN_MISMATCH, ZK_E_NVARS, ZK_E_NEED_TWO, ZK_E_KZG_LEN, ZK_E_RANGE, ZK_E_NOT_INIT}

_HERE = os.path.dirname(os.path.abspath(__file__))


class ZkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[zk_status {code}] {msg}")
        self.code = code


class ReferencePanic(ZkError):
    """A precondition on which the reference panics (same message text)."""


def library_path():
    return os.environ.get("ZKMLE_AMD_LIB") or os.path.join(_HERE, "libzkmle_amd.so")


_lib = None
u64p = C.POINTER(C.c_uint64)
u8p = C.POINTER(C.c_uint8)
vp = C.c_void_p
sz = C.c_size_t


def lib():
    """The loaded shared library.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ZkError(ZK_E_NO_DEVICE, f"{path} not found: build it with __graft_entry__.build() "
                                      "(zkmle_amd has no CPU fallback)")
    try:
        import torch  # noqa: F401  (loads the HIP runtime torch ships, so both share one libamdhip64)
    except Exception:
        pass
    L = C.CDLL(path)
    L.zk_status_message.restype = C.c_char_p
    L.zk_last_error.restype = C.c_char_p
    L.zk_version.restype = C.c_char_p
    L.zk_table_len.restype = sz
    L.zk_table_device_ptr.restype = vp
    L.zk_merkle_depth.restype = sz
    L.zk_fri_commitment_log_group.restype = C.c_uint32
    L.zk_fri_columns_count.restype = C.c_uint32
    # the zerocheck family (zerocheck .. plonk_lookup below): what stands behind an entry's own leading arguments
    opened = [u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p]         # ys, gamma, round polys, roots, final, challenges, indices, values, paths
    zc_prove = [vp, u64p, u64p, u64p] + opened + [u64p]                    # transcript, tau, round polys, challenges; the opening; the nonce
    zh_prove = [vp, u8p, u64p, u64p, u64p] + opened + [u64p]               # transcript, helper roots, drawn, round polys, challenges; ..
    checked = [u64p, u64p, u64p, u8p, u64p, u64p, u8p, C.c_uint32, C.c_uint64, C.POINTER(C.c_int)]   # round polys, ys, the opening; bits, nonce; ok
    zc_verify = [u64p, vp] + checked                                       # coset, transcript; ..
    zh_verify = [u64p, vp, u8p] + checked                                  # coset, transcript, helper roots; ..
    sigs = {
        "zk_device_count": [C.POINTER(C.c_int)],
        "zk_init": [C.c_int],
        "zk_field_limbs": [C.c_int],
        "zk_device_synchronize": [],
        "zk_table_alloc": [C.c_int, sz, C.POINTER(vp)],
        "zk_table_upload": [C.c_int, u64p, sz, C.POINTER(vp)],
        "zk_table_upload_raw": [C.c_int, u64p, sz, C.POINTER(vp)],
        "zk_table_download": [vp, u64p],
        "zk_table_free": [vp],
        "zk_table_len": [vp],
        "zk_table_field": [vp],
        "zk_table_device_ptr": [vp],
        "zk_table_wrap": [C.c_int, vp, sz, C.POINTER(vp)],
        "zk_table_clone": [vp, C.POINTER(vp)],
        "zk_table_fill_random": [vp, C.c_uint64],
        "zk_table_fill_random_strided": [vp, C.c_uint64, sz, sz],
        "zk_host_fill_random": [C.c_int, C.c_uint64, sz, sz, u64p],
        "zk_mle_fold": [vp, sz, u64p, vp, vp],
        "zk_mle_fold_ptr": [C.c_int, vp, sz, sz, u64p, vp, vp],
        "zk_mle_evaluate": [vp, u64p, sz, u64p],
        "zk_mle_to_bytes": [vp, u8p],
        "zk_mle_scalar_mul": [vp, u64p, vp, vp],
        "zk_mle_add": [vp, vp, vp, vp],
        "zk_mle_linear_combination": [C.POINTER(vp), sz, u64p, vp, vp],
        "zk_mle_sub_scalar": [vp, u64p, vp, vp],
        "zk_mle_tensor_add": [vp, vp, vp, vp],
        "zk_mle_tensor_mul": [vp, vp, vp, vp],
        "zk_mle_sum": [vp, u64p],
        "zk_mle_half_sums": [vp, u64p],
        "zk_mle_fold_half_sums": [vp, u64p, vp, u64p, vp],
        "zk_host_partial_evaluate": [C.c_int, u64p, sz, sz, u64p, u64p],
        "zk_host_evaluate": [C.c_int, u64p, sz, u64p, sz, u64p],
        "zk_fe_from_u64": [C.c_int, C.c_uint64, u64p],
        "zk_fe_to_bytes_be": [C.c_int, u64p, u8p],
        "zk_fe_from_le_bytes_mod_order": [C.c_int, u8p, sz, u64p],
        "zk_vec_from_canonical": [C.c_int, u64p, sz, u64p],
        "zk_vec_to_canonical": [C.c_int, u64p, sz, u64p],
        # Merkle commitment of a table (extension)
        "zk_mle_merkle_root": [vp, u8p],
        "zk_merkle_build": [vp, C.POINTER(vp)],
        "zk_merkle_free": [vp],
        "zk_merkle_depth": [vp],
        "zk_merkle_root": [vp, u8p],
        "zk_merkle_open": [vp, C.POINTER(sz), sz, u8p],
        "zk_merkle_verify": [C.c_int, u8p, sz, sz, u64p, u8p, C.POINTER(C.c_int)],
        "zk_merkle_build_grouped": [vp, C.c_uint32, C.POINTER(vp)],
        "zk_mle_merkle_root_grouped": [vp, C.c_uint32, u8p],
        "zk_merkle_verify_grouped": [C.c_int, u8p, sz, sz, C.c_uint32, u64p, u8p, C.POINTER(C.c_int)],
        # number-theoretic transform (extension)
        "zk_ntt_two_adicity": [C.c_int, C.POINTER(C.c_uint32)],
        "zk_ntt_root_of_unity": [C.c_int, C.c_uint32, u64p],
        "zk_ntt": [vp, C.c_int, u64p],
        "zk_host_ntt": [C.c_int, u64p, sz, C.c_int, u64p, u64p],
        "zk_uni_low_degree_extend": [vp, C.c_uint32, u64p, C.POINTER(vp)],
        "zk_uni_mul": [vp, vp, C.POINTER(vp)],
        # FRI low-degree proof (extension)
        "zk_fri_fold": [vp, u64p, u64p, C.POINTER(vp)],
        "zk_fri_proof_sizes": [C.c_uint32] * 4 + [C.POINTER(sz)] * 4,
        "zk_fri_prove": [vp] + [C.c_uint32] * 3 + [u64p, vp, u8p, u64p, u64p, u64p, u64p, u8p],
        "zk_fri_prove_codeword": [vp] + [C.c_uint32] * 3 + [u64p, vp, u8p, u64p, u64p, u64p, u64p, u8p],
        "zk_fri_verify": [C.c_int] + [C.c_uint32] * 4 + [u64p, vp, u8p, u64p, u64p, u8p, C.POINTER(C.c_int)],
        "zk_fri_last_stats": [vp],
        # FRI polynomial commitment: opening at a point (extension)
        "zk_fri_commit": [vp, C.c_uint32, u64p, C.POINTER(vp)],
        "zk_fri_commit_grouped": [vp, C.c_uint32, u64p, C.c_uint32, C.POINTER(vp)],
        "zk_fri_commitment_log_group": [vp],
        "zk_fri_commitment_free": [vp],
        "zk_fri_commitment_root": [vp, u8p],
        "zk_fri_commitment_codeword": [vp, C.POINTER(vp)],
        "zk_fri_pcs_sizes": [C.c_uint32] * 5 + [C.POINTER(sz)] * 6,
        "zk_uni_evaluate_device": [vp, u64p, u64p],
        "zk_fri_pcs_quotient": [C.POINTER(vp), sz, u64p, u64p, u64p, C.POINTER(vp)],
        "zk_fri_pcs_open": [C.POINTER(vp), sz, u64p, C.c_uint32, C.c_uint32, vp, u64p, u8p, u64p, u64p, u64p, u64p, u8p, u64p, u8p],
        "zk_fri_pcs_verify": [C.c_int, sz, u8p] + [C.c_uint32] * 4 + [u64p, u64p, u64p, vp, u8p, u64p, u64p, u8p, u64p, u8p, C.POINTER(C.c_int)],
        "zk_fri_pcs_last_stats": [vp],
        # FRI commitment opened as a multilinear polynomial (extension)
        "zk_fri_ml_fold": [vp, u64p, u64p, C.POINTER(vp)],
        "zk_fri_ml_sizes": [C.c_uint32] * 4 + [C.POINTER(sz)] * 5,
        "zk_fri_ml_open": [vp, u64p, C.c_uint32, C.c_uint32, vp, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p],
        "zk_fri_ml_verify": [C.c_int, u8p] + [C.c_uint32] * 4 + [u64p, u64p, u64p, vp, u64p, u8p, u64p, u64p, u8p, C.POINTER(C.c_int)],
        "zk_fri_ml_last_stats": [vp],
        "zk_fri_ml_round": [vp, vp, u64p, C.POINTER(vp), C.POINTER(vp), u64p],
        "zk_fri_ml_open_points": [vp, u64p, C.c_uint32, C.c_uint32, C.c_uint32, vp, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p],
        "zk_fri_ml_verify_points": [C.c_int, u8p] + [C.c_uint32] * 4 + [u64p, u64p, C.c_uint32, u64p, vp, u64p, u8p, u64p, u64p, u8p,
                                                                       C.POINTER(C.c_int)],
        "zk_fri_ml_fold4": [vp, u64p, u64p, u64p, C.POINTER(vp)],
        "zk_fri_ml_sizes_arity": [C.c_uint32] * 5 + [C.POINTER(sz)] * 5,
        "zk_fri_ml_open_points_arity": [vp, u64p] + [C.c_uint32] * 4 + [vp, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p],
        "zk_fri_ml_verify_points_arity": [C.c_int, u8p] + [C.c_uint32] * 5 + [u64p, u64p, C.c_uint32, u64p, vp, u64p, u8p, u64p, u64p, u8p,
                                                                             C.POINTER(C.c_int)],
        # ... with grouped leaves
        "zk_fri_ml_sizes_grouped": [C.c_uint32] * 4 + [C.POINTER(sz)] * 5,
        "zk_fri_ml_open_points_grouped": [vp, u64p] + [C.c_uint32] * 3 + [vp, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p],
        "zk_fri_ml_verify_points_grouped": [C.c_int, u8p] + [C.c_uint32] * 4 + [u64p, u64p, C.c_uint32, u64p, vp, u64p, u8p, u64p, u64p, u8p,
                                                                               C.POINTER(C.c_int)],
        # FRI commitments opened together
        "zk_fri_ml_fold_batch": [C.POINTER(vp), C.c_uint32, u64p, u64p, u64p, u64p, C.POINTER(vp)],
        "zk_fri_ml_sizes_batch": [C.c_uint32] * 7 + [C.POINTER(sz)] * 5,
        "zk_fri_ml_open_batch": [C.POINTER(vp), C.c_uint32, u64p] + [C.c_uint32] * 4 + [vp, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p],
        "zk_fri_ml_verify_batch": [C.c_int, u8p] + [C.c_uint32] * 7 + [u64p, u64p, C.c_uint32, u64p, vp, u64p, u8p, u64p, u64p, u8p, C.POINTER(C.c_int)],
        # proof-of-work grinding
        "zk_transcript_grind": [vp, C.c_uint32, C.c_uint64, C.c_uint32, u64p],
        "zk_host_transcript_grind": [vp, C.c_uint32, C.c_uint64, C.c_uint64, u64p],
        "zk_transcript_grind_check": [vp, C.c_uint32, C.c_uint64, C.POINTER(C.c_int)],
        "zk_transcript_grind_last_stats": [vp],
        "zk_fri_prove_pow": [vp] + [C.c_uint32] * 3 + [u64p, vp, u8p, u64p, u64p, u64p, u64p, u8p, C.c_uint32, u64p],
        "zk_fri_verify_pow": [C.c_int] + [C.c_uint32] * 4 + [u64p, vp, u8p, u64p, u64p, u8p, C.c_uint32, C.c_uint64, C.POINTER(C.c_int)],
        "zk_fri_ml_open_batch_pow": [C.POINTER(vp), C.c_uint32, u64p] + [C.c_uint32] * 4 + [vp, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p,
                                                                                          C.c_uint32, u64p],
        "zk_fri_ml_verify_batch_pow": [C.c_int, u8p] + [C.c_uint32] * 7 + [u64p, u64p, C.c_uint32, u64p, vp, u64p, u8p, u64p, u64p, u8p, C.c_uint32,
                                                                          C.c_uint64, C.POINTER(C.c_int)],
        # FRI commitments opened together, wide: up to 32
        "zk_fri_ml_fold_batch_wide": [C.POINTER(vp), C.c_uint32, u64p, u64p, u64p, u64p, C.POINTER(vp)],
        "zk_fri_ml_sizes_batch_wide": [C.c_uint32] * 7 + [C.POINTER(sz)] * 5,
        "zk_fri_ml_open_batch_wide_pow": [C.POINTER(vp), C.c_uint32, u64p] + [C.c_uint32] * 4 + [vp, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p,
                                                                                               C.c_uint32, u64p],
        "zk_fri_ml_verify_batch_wide_pow": [C.c_int, u8p] + [C.c_uint32] * 7 + [u64p, u64p, C.c_uint32, u64p, vp, u64p, u8p, u64p, u64p, u8p, C.c_uint32,
                                                                               C.c_uint64, C.POINTER(C.c_int)],
        # column commitments: several tables under one tree, opened together
        "zk_merkle_build_columns": [C.POINTER(vp), C.c_uint32, C.POINTER(vp)],
        "zk_mle_merkle_root_columns": [C.POINTER(vp), C.c_uint32, u8p],
        "zk_merkle_verify_columns": [C.c_int, u8p, sz, sz, C.c_uint32, u64p, u8p, C.POINTER(C.c_int)],
        "zk_fri_commit_columns": [C.POINTER(vp), C.c_uint32, C.c_uint32, u64p, C.POINTER(vp)],
        "zk_fri_columns_free": [vp],
        "zk_fri_columns_root": [vp, u8p],
        "zk_fri_columns_count": [vp],
        "zk_fri_columns_table": [vp, C.c_uint32, C.POINTER(vp)],
        "zk_fri_columns_codeword": [vp, C.c_uint32, C.POINTER(vp)],
        "zk_fri_columns_last_stats": [vp],
        "zk_fri_ml_sizes_columns": [C.POINTER(C.c_uint32)] + [C.c_uint32] * 5 + [C.POINTER(sz)] * 5,
        "zk_fri_ml_open_columns_pow": [C.POINTER(vp), C.c_uint32, u64p] + [C.c_uint32] * 4 + [vp, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p, u64p],
        "zk_fri_ml_verify_columns_pow": [C.c_int, u8p, C.POINTER(C.c_uint32)] + [C.c_uint32] * 6 + [u64p, u64p, C.c_uint32, u64p, vp, u64p, u8p, u64p, u64p, u8p,
                                                                                                   C.c_uint64, C.POINTER(C.c_int)],
        # a FRI commitment opened against a caller's weight table
        "zk_fri_ml_sizes_weighted": [C.c_uint32] * 6 + [C.POINTER(sz)] * 5,
        "zk_fri_ml_open_weighted": [vp, vp] + [C.c_uint32] * 4 + [vp, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p, u64p],
        "zk_fri_ml_verify_weighted": [C.c_int, u8p] + [C.c_uint32] * 6 + [u64p, u64p, u64p, u64p, vp, u64p, u8p, u64p, u64p, u8p, C.c_uint32, C.c_uint64,
                                                                         C.POINTER(C.c_int)],
        # zerocheck of a product of committed tables
        "zk_zerocheck_mul_round": [vp, vp, vp, vp, u64p, C.POINTER(vp), u64p],
        "zk_zerocheck_sizes": [C.c_uint32] * 6 + [C.POINTER(sz)] * 6,
        "zk_zerocheck_mul_prove": [vp, vp, vp] + [C.c_uint32] * 4 + zc_prove,
        "zk_zerocheck_mul_verify": [C.c_int, u8p] + [C.c_uint32] * 6 + zc_verify,
        "zk_zerocheck_last_stats": [vp],
        # zerocheck of a Plonk gate over committed tables
        "zk_zerocheck_gate_round": [C.POINTER(vp), u64p, C.POINTER(vp), u64p],
        "zk_zerocheck_gate_sizes": [C.c_uint32] * 6 + [C.POINTER(sz)] * 6,
        "zk_zerocheck_gate_prove": [C.POINTER(vp)] + [C.c_uint32] * 4 + zc_prove,
        "zk_zerocheck_gate_verify": [C.c_int, u8p] + [C.c_uint32] * 6 + zc_verify,
        # wiring: a permutation check over committed tables
        "zk_wiring_fractions": [vp, vp, C.c_uint64, u64p, u64p, C.POINTER(vp)],
        "zk_wiring_round": [C.POINTER(vp), u64p, u64p, u64p, u64p, u64p, C.c_uint32, u64p, C.POINTER(vp), u64p],
        "zk_wiring_sizes": [C.c_uint32] * 6 + [C.POINTER(sz)] * 7,
        "zk_wiring_prove": [C.POINTER(vp)] + [C.c_uint32] * 4 + zh_prove,
        "zk_wiring_verify": [C.c_int, u8p] + [C.c_uint32] * 6 + zh_verify,
        "zk_wiring_last_stats": [vp],
        # Plonk: gate, wiring and public inputs in one sumcheck
        "zk_plonk_round": [C.POINTER(vp), u64p, u64p, u64p, u64p, u64p, C.c_uint32, u64p, C.POINTER(vp), u64p],
        "zk_plonk_public_eval": [C.c_int, u64p, C.c_uint32, u64p, C.c_uint32, u64p],
        "zk_plonk_sizes": [C.c_uint32] * 6 + [C.POINTER(sz)] * 7,
        "zk_plonk_prove": [C.POINTER(vp), u64p] + [C.c_uint32] * 5 + zh_prove,
        "zk_plonk_verify": [C.c_int, u8p, u64p] + [C.c_uint32] * 7 + zh_verify,
        "zk_plonk_last_stats": [vp],
        # lookup: rows of a committed table
        "zk_lookup_multiplicities": [C.POINTER(vp), C.POINTER(vp), u64p],
        "zk_lookup_hash_slots": [C.POINTER(vp), C.POINTER(C.c_uint32)],
        "zk_lookup_fractions": [C.POINTER(vp), u64p, u64p, C.POINTER(vp)],
        "zk_lookup_round": [C.POINTER(vp), u64p, u64p, u64p, u64p, C.POINTER(vp), u64p],
        "zk_lookup_sizes": [C.c_uint32] * 6 + [C.POINTER(sz)] * 7,
        "zk_lookup_prove": [C.POINTER(vp)] + [C.c_uint32] * 4 + zh_prove,
        "zk_lookup_verify": [C.c_int, u8p] + [C.c_uint32] * 6 + zh_verify,
        "zk_lookup_last_stats": [vp],
        # Plonk with lookups: gate, wiring, public inputs and lookup rows in one sumcheck
        "zk_plonk_lookup_round": [C.POINTER(vp), u64p, u64p, u64p, u64p, u64p, C.c_uint32, u64p, C.POINTER(vp), u64p],
        "zk_plonk_lookup_sizes": [C.c_uint32] * 6 + [C.POINTER(sz)] * 7,
        "zk_plonk_lookup_prove": [C.POINTER(vp), u64p] + [C.c_uint32] * 5 + zh_prove,
        "zk_plonk_lookup_verify": [C.c_int, u8p, u64p] + [C.c_uint32] * 7 + zh_verify,
        "zk_plonk_lookup_last_stats": [vp],
        # Plonk with lookups on column commitments
        "zk_plonk_lookup_helpers": [C.POINTER(vp), u64p, u64p, C.POINTER(vp)],
        "zk_plonk_lookup_helpers_batch": [],
        "zk_plonk_lookup_sizes_columns": [C.c_uint32] * 4 + [C.POINTER(sz)] * 7,
        "zk_plonk_lookup_prove_columns": [vp, vp, u64p] + [C.c_uint32] * 4 + zh_prove,
        "zk_plonk_lookup_verify_columns": [C.c_int, u8p, u8p, u64p] + [C.c_uint32] * 5 + zh_verify,
        "zk_plonk_lookup_columns_last_stats": [vp],
        # R1CS instance: three sparse matrices, their products with a table and their rows bound at a point
        "zk_r1cs_create": [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(u64p),
                           C.POINTER(sz), C.POINTER(vp)],
        "zk_r1cs_free": [vp],
        "zk_r1cs_digest": [vp, u8p],
        "zk_r1cs_shape": [vp, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64p, u64p],
        "zk_r1cs_matvec": [vp, vp, C.POINTER(vp)],
        "zk_r1cs_bind_rows": [vp, u64p, u64p, C.c_int, C.POINTER(vp)],
        "zk_r1cs_last_stats": [vp],
        "zk_r1cs_sizes": [C.c_uint32] * 7 + [C.POINTER(sz)] * 6,
        "zk_r1cs_prove": [vp, vp, u64p] + [C.c_uint32] * 5 + [vp, u64p, u64p, u64p, u64p, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p, u64p],
        "zk_r1cs_verify": [vp, u8p, u64p] + [C.c_uint32] * 6 + [u64p, vp, u64p, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u8p, C.c_uint32, C.c_uint64,
                                                               C.POINTER(C.c_int)],
        "zk_r1cs_public_terms": [vp, u64p, C.c_uint32, u64p, u64p, u64p, C.c_uint32, u64p, u64p],
        # sparse GKR: one phase's table kernel on caller-chosen tables (a gate array is passed as a void pointer)
        "zk_gkr_sparse_phase_tables": [C.c_int, C.c_int, vp, sz, C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.c_uint32, vp, vp, vp, vp, C.c_uint32, u64p,
                                       C.POINTER(vp), C.POINTER(vp)],
        "zk_sumcheck_basic_prove_succinct": [vp, C.c_uint32, C.c_uint32, vp, u64p, u64p, u64p, u64p, u64p, u8p, u64p, u64p, u64p, u64p, u8p],
        "zk_sumcheck_basic_verify_succinct": [C.c_int, u8p] + [C.c_uint32] * 4 + [u64p, vp, u64p, u64p, u64p, u64p, u8p, u64p, u64p, u8p,
                                                                                 C.POINTER(C.c_int)],
    }
    for name, args in sigs.items():
        fn = getattr(L, name)       # AttributeError = missing export: loud
        fn.argtypes = args
        if name not in ("zk_table_len", "zk_table_device_ptr", "zk_merkle_depth", "zk_fri_commitment_log_group"):
            fn.restype = C.c_int
    _lib = L
    return L


def check(rc):
    if rc == ZK_OK:
        return
    L = lib()
    msg = L.zk_status_message(rc).decode()
    if rc == ZK_E_HIP or rc == ZK_E_NO_DEVICE or rc == ZK_E_COMM:
        msg += ": " + L.zk_last_error().decode()
    raise (ReferencePanic if rc in _PANIC_CODES else ZkError)(rc, msg)


def p64(arr):
    return arr.ctypes.data_as(u64p)


def p8(arr):
    return arr.ctypes.data_as(u8p)
