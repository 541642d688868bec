"""fhe_sign -- Python host binding of the MI355X-native TFHE radix engine (fhe-sign_amd).

Mirrors the reference crate's surface (coset-io/fhe-sign):
  generate_keys / set_server_key      tfhe HL API as used at src/schnorr.rs:441-443
  FheUint{8,32,64}                    tfhe FheUint ops used by src/biguint.rs and src/perf_test.rs
  BigUintFHE (+, *)                   src/biguint.rs:8-265
  CompressedFheUint / CompressedBigUintFHE   tfhe's seeded ciphertexts (try_encrypt / decompress)
  CompressedServerKey                 tfhe's seeded server key (new / decompress; Context.set_server_key
                                      installs it on the GPU from its bodies)
  CompressionKeys / CompressedCiphertextList   tfhe's compression of computed ciphertexts: x.compress() on
                                      the GPU, .serialize(), .decrypt(private) on the client, .decompress()
  CompressedCompressionKey            tfhe's seeded compression key (CompressionKeys.generate_compressed /
                                      decompress; Context.set_compression_key installs it from its bodies)
  CompactPublicKey / CompactCiphertextList   tfhe's public-key encryption: builder(pk).push(..).build_packed()
                                      without any secret, .expand() on the GPU
  Context.set_public_key / x.re_randomize(seed)   tfhe's re_randomize: a fresh public-key encryption of zero added
                                      to every block on the GPU (rerandomize_host: the host definition)
  ReRandomizationContext / re_randomize_bound / x.digest()   tfhe's ReRandomizationContext: the seed is a hash of
                                      the ciphertexts' own bytes, digested on the GPU (ct_digest_host: the host
                                      definition), plus domain separators
  Context.set_modulus_switch("centered")   tfhe's centered mean noise reduction: the public half of the modulus
                                      switch's rounding error leaves the body on the GPU before every blind
                                      rotation (ms_center_host: the host definition)
  FheUint.random(seed) / random_below(bound, seed) / BigUintFHE.random(bits, seed)   tfhe's
                                      generate_oblivious_pseudo_random[_bounded]: a seed becomes an encrypted uniformly
                                      random value on the GPU, one blind rotation per block, no keyswitch, no upload
                                      (oprf_rows_host, oprf_lut_host: the host definitions)
  x.compress_switched() / SwitchedCiphertextList   tfhe's FheUint::compress(): the keyswitched, modulus-switched rows,
                                      12 bits per value and no extra key; .decrypt(client_key) with the small key
                                      alone, .decompress() by one blind rotation per block (switched_pack_host,
                                      switched_unpack_host, SwitchedCiphertextList.compress_host: the host definitions)
  Schnorr.sign_fhe_with_k0 / sign_fhe src/schnorr.rs:154-290
  x.rem_pseudo_mersenne(k, c) / Schnorr.eval_s / sign_fhe_with_k0(reduce=True)   x mod (2^k - c) by folds (both
                                      secp256k1 moduli: SECP256K1_N_C, SECP256K1_P_C); the signer reduces s mod n
                                      under encryption, so the one decrypted value is the signature's s
All ciphertext arithmetic runs on the GPU through lib/libfhe_rocm.so; this package only marshals.
"""
from ._lib import CompressionParams, FheError, FheParams, load  # noqa: F401
from .core import (ClientKey, RekeyKey, CompactPublicKey, CompressedCompressionKey, CompressedServerKey, CompressionKey, CompressionKeys, CompressionPrivateKey, Context, ServerKey, comm_unique_id, default_params,  # noqa: F401
                   default_compression_params, generate_keys, ms_center_host, ms_stride, multi_bit_params, oprf_lut_host, oprf_rows_host, tuning, fault_arm, FAULT_LEVEL, FAULT_STAGE,
                   FAULT_WORKSPACE, FAULT_DEFERRED, FAULT_RECORD, FAULT_CLIENT, FAULT_ALL,
                   switched_pack_host, switched_row_bytes, switched_unpack_host, SimContext, SimKey, noise_audit)
from .integer import (  # noqa: F401,E402
    COMPAT, FAST, PUBLIC, BigUintFHE, FheBool, FheUint, FheUint8, FheUint32, FheUint64, FheUint128, FheUint256, set_server_key,
    LEVEL_SPLIT, level_log, rank_pbs, stats, to_u32_digits, SECP256K1_N_C, SECP256K1_P_C,
    trace_enable, trace_read, pending_info, block_addrs, lut_table, export_luts, LUT_INTEGER, LUT_HALF_STEP, LUT_OPRF,
    CompressedBigUintFHE, CompressedFheUint, CompressedFheUint8, CompressedFheUint32, CompressedFheUint64,
    CompressedFheUint128, CompressedFheUint256, CompressedCiphertextList, SwitchedCiphertextList,
    CompactCiphertextList, CompactCiphertextListBuilder,
    rerandomization_seed, rerandomize_host, rerandomize_rows, rerandomize_zero_host,
    ReRandomizationContext, ct_digest_host, ct_digest_rows, ct_value_digest_host, re_randomize_bound)
from .schnorr import Schnorr, compute_nonce, public_key_x  # noqa: F401,E402
