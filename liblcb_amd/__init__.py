"""liblcb_amd — MI355X-native batch digest engine for liblcb's crypto/hash path.

The product is the C-ABI library liblcb_hash_gpu.so (include/lcb_hash_gpu.h,
HIP kernels in csrc/).  This package is its host-side Python mirror of the
reference's one-shot API (liblcb_amd.hash), the CRC-32 family of
include/math/crc32.h (liblcb_amd.crc32), the ChaCha / XChaCha cipher of
include/crypto/cipher/chacha.h (liblcb_amd.chacha), the GOST 28147-89 block
cipher and MAC of include/crypto/cipher/gost28147.h (liblcb_amd.gost28147,
its own library liblcb_gost28147_gpu.so), the asynchronous
packet ingestion queue (liblcb_amd.queue) and batched RADIUS packet
signing / verification: per packet over the keyed batches with the packet
logic on the host (liblcb_amd.radius) and packed, wholly on the device
(liblcb_amd.radius_batch, its own library liblcb_radius_gpu.so), and batched
streaming digests, device-resident init / update / final contexts
(liblcb_amd.stream, its own library liblcb_hash_stream_gpu.so), and batched
ECDSA / GOST R 34.10 signature verification of include/crypto/dsa/ecdsa.h
(liblcb_amd.ecdsa, its own library liblcb_ecdsa_gpu.so) and its other half,
batched signing, key generation and public keys from private keys
(liblcb_amd.ecdsa_sign, its own library liblcb_ecdsa_sign_gpu.so), and
batched ECDH key agreement (liblcb_amd.ecdsa_dh, its own library
liblcb_ecdsa_dh_gpu.so), and batched public-key import and export, the
compressed and packed wire forms (liblcb_amd.ecdsa_key, its own library
liblcb_ecdsa_key_gpu.so), and the verification again on the 384- and 512-bit
curves (liblcb_amd.ecdsa_wide, its own library liblcb_ecdsa_wide_gpu.so) and
signing, key generation and public keys on them (liblcb_amd.ecdsa_wide_sign,
its own library liblcb_ecdsa_wide_sign_gpu.so).
"""
from ._lib import (ALG_IDS, ALG_NAMES, BLOCK_SIZE, DIGEST_SIZE, GOST256, GOST512, MD5, SHA1,
                   SHA224, SHA256, SHA384, SHA512, LcbHashError, ecdsa_dh_lib, ecdsa_key_lib, lib)
from .hash import *  # noqa: F401,F403
from . import chacha, crc32, ecdsa, ecdsa_dh, ecdsa_key, ecdsa_sign, ecdsa_wide, ecdsa_wide_sign, gost28147, queue, radius, radius_batch, stream  # noqa: F401,E402  (ciphers, CRC-32, ECDSA, ingestion queue, RADIUS, streaming)
from .ecdsa import ecdsa_lib  # noqa: F401,E402
from .ecdsa_sign import ecdsa_sign_lib  # noqa: F401,E402
from .ecdsa_wide import ecdsa_wide_lib  # noqa: F401,E402
from .ecdsa_wide_sign import ecdsa_wide_sign_lib  # noqa: F401,E402
from .gost28147 import gost28147_lib  # noqa: F401,E402
from .radius_batch import radius_lib  # noqa: F401,E402
from .stream import StreamSet, stream_lib  # noqa: F401,E402

__all__ = ["ALG_IDS", "ALG_NAMES", "BLOCK_SIZE", "DIGEST_SIZE", "MD5", "SHA1", "SHA224",
           "SHA256", "SHA384", "SHA512", "GOST256", "GOST512", "LcbHashError", "lib", "gost28147_lib", "radius_lib",
           "StreamSet", "stream_lib", "ecdsa_lib", "ecdsa_sign", "ecdsa_sign_lib", "ecdsa_dh",
           "ecdsa_dh_lib", "ecdsa_key", "ecdsa_key_lib", "ecdsa_wide", "ecdsa_wide_lib",
           "ecdsa_wide_sign", "ecdsa_wide_sign_lib"]
