"""The ciphertext digests and the re-randomization context (include/fhe_rocm.h "ciphertext digests, bound
seeds") restated in hashlib and numpy, nothing else: what tests/test_ct_digest.py pins fhe_ct_digest_host and the
context functions to, and tests/test_ct_digest_gpu.py the kernel.  Not collected by pytest."""
import hashlib
import struct

import numpy as np

ROW = 2049
ZERO_ROW_DIGEST = "3c4ea852595c986cd5f1502f0b051cc3e145cdc099d76615e86ddf72455bc628"
RAMP_ROW_DIGEST = "d485c2a9c9757a3cb8fdae6059fb8e4a3396c53cffd8755fa672ad695f5fb5e0"
FLIP_WORDS = (0, 31, 32, 255, 256, 2047, 2048)  # the leaf edge, the node edge, the last mask word, the body


def tagged(tag: str, msg: bytes) -> bytes:
    t = hashlib.sha256(tag.encode()).digest()
    return hashlib.sha256(t + t + msg).digest()


def row_digest(row) -> bytes:
    b = np.asarray(row, dtype="<u8").reshape(ROW).tobytes()
    leaves = [tagged("fhe-rocm/ct-leaf", b[256 * j:256 * j + 256]) for j in range(64)]
    nodes = [tagged("fhe-rocm/ct-node", b"".join(leaves[8 * g:8 * g + 8])) for g in range(8)]
    return tagged("fhe-rocm/ct-row", b"".join(nodes) + b[16384:16392])


def rows_digest(rows) -> np.ndarray:
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, ROW)
    return np.frombuffer(b"".join(row_digest(r) for r in rows), np.uint8).reshape(-1, 32)


def value_digest(kind: int, bits: int, blocks) -> bytes:
    """blocks: (tag, degree, noise, rowdigest) per block"""
    msg = struct.pack("<BII", kind, bits, len(blocks))
    for tag, degree, noise, rd in blocks:
        msg += struct.pack("<BII", tag, degree, noise) + bytes(rd)
    return tagged("fhe-rocm/ct-value", msg)


class Context:
    def __init__(self, domain: bytes):
        t = hashlib.sha256(b"fhe-rocm/rerandomize-context").digest()
        self.msg = t + t + struct.pack("<Q", len(domain)) + domain

    def add_bytes(self, b: bytes):
        self.msg += struct.pack("<BQ", 1, len(b)) + b
        return self

    def add_digest(self, d: bytes):
        assert len(d) == 32
        self.msg += struct.pack("<BQ", 2, 32) + d
        return self

    def seed(self, i: int) -> bytes:
        return tagged("fhe-rocm/rerandomize-seed", hashlib.sha256(self.msg).digest() + struct.pack("<Q", i))


def ramp_row() -> np.ndarray:
    return np.array([(i + 1) * 0x0123456789ABCDEF % 2**64 for i in range(ROW)], dtype=np.uint64)


def hand_rows() -> np.ndarray:
    """the all-zero row, the ramp, the all-ones row, then the ramp with one bit flipped at each of FLIP_WORDS"""
    rows = [np.zeros(ROW, np.uint64), ramp_row(), np.full(ROW, 2**64 - 1, np.uint64)]
    for k, w in enumerate(FLIP_WORDS):
        r = ramp_row()
        r[w] ^= np.uint64(1) << np.uint64((9 * k + 5) % 64)
        rows.append(r)
    return np.stack(rows)
