"""Recipe and ctypes wrapper of the Ed25519 oracle built from ring's C (TEST
INFRASTRUCTURE ONLY): oracle/ring_ed25519_driver.c compiled with the reference
tree's utils/ring/third_party/fiat/curve25519.c and crypto/mem.c into
oracle/_ref/libring_ed25519.so (git-ignored; nothing of the reference is
copied or committed).  Plain gcc, the reference's include/, its root and
third_party/fiat on the include path.

Covered by ring's C: the key's decoding, the digest's reduction mod L, the
double scalar multiplication and the encoding of the result.  The glue between
them (lengths, S < L, the negation of A, the byte comparison, the codes) is the
driver's restatement of ring's Rust; see the driver's header.

Called by tests/golden/gen_ring_ed25519_crafted.py and by the oracle-rebuild
test of tests/test_ed25519_crafted.py, never by build().

Usage: python -m oracle.ring_ed25519_ref [reference root]   (builds, prints the path)
"""
import ctypes
import hashlib
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "ring_ed25519_driver.c")
OUT = os.path.join(HERE, "_ref", "libring_ed25519.so")
DEFAULT_REFERENCE = os.environ.get("CESS_REFERENCE_TREE", "/root/reference")
RING_SOURCES = ("third_party/fiat/curve25519.c", "crypto/mem.c")


def ring_root(reference=None):
    return os.path.join(reference or DEFAULT_REFERENCE, "utils", "ring")


def available(reference=None):
    """the reference's sources and gcc are both here"""
    root = ring_root(reference)
    return shutil.which("gcc") is not None and all(os.path.exists(os.path.join(root, s)) for s in RING_SOURCES)


def build(reference=None, out=OUT):
    """compile the oracle; returns the library's path"""
    root = ring_root(reference)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["gcc", "-O2", "-std=c11", "-shared", "-fPIC", "-w",
           "-I" + os.path.join(root, "include"), "-I" + root, "-I" + os.path.join(root, "third_party", "fiat"),
           DRIVER] + [os.path.join(root, s) for s in RING_SOURCES] + ["-o", out]
    subprocess.check_call(cmd)
    return out


class Oracle:
    def __init__(self, path):
        lib = ctypes.CDLL(path)
        lib.ring_ed_verify.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t]
        lib.ring_ed_sc_reduce.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        lib.ring_ed_decode.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
        self.lib = lib

    def verify_code(self, key, msg, sig):
        digest = hashlib.sha512(sig[:32] + key + msg).digest()
        return self.lib.ring_ed_verify(key, len(key), digest, sig, len(sig))

    def sc_reduce(self, x64):
        assert len(x64) == 64
        out = ctypes.create_string_buffer(32)
        self.lib.ring_ed_sc_reduce(x64, out)
        return out.raw

    def decode(self, key):
        """(x, y) as integers, or None"""
        assert len(key) == 32
        x, y = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
        if not self.lib.ring_ed_decode(key, x, y):
            return None
        return int.from_bytes(x.raw, "little"), int.from_bytes(y.raw, "little")


def load(reference=None, out=OUT):
    return Oracle(build(reference, out))


if __name__ == "__main__":
    print(build(sys.argv[1] if len(sys.argv) > 1 else None))
