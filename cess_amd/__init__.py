"""cess_amd — MI355X-native batch verifier for the BLS12-381 signature path of
CESS (utils/verify-bls-signatures).  See DESIGN.md."""
from .bls import (  # noqa: F401
    CODE_NAMES, Context, DeserializeError, DeviceUnavailable, InvalidPrivateKey, InvalidPublicKey,
    InvalidSignature, PrivateKey, PublicKey, Result, Signature, Verdicts, default_context, load_library,
    verify_batch, verify_bls_signature,
    ED25519_CODE_NAMES, ED25519_KEY, ED25519_MISMATCH, ED25519_OK, ED25519_POLICY_RING, ED25519_SIG_LEN,
    ED25519_SIG_RANGE, verify_ed25519,
    ECDSA_ALG_P256_SHA256_ASN1, ECDSA_ALG_P256_SHA256_FIXED, ECDSA_ALG_P256_SHA384_ASN1, ECDSA_CODE_NAMES, ECDSA_KEY,
    ECDSA_MISMATCH, ECDSA_OK, ECDSA_SIG_FORMAT, ECDSA_SIG_RANGE, verify_ecdsa,
    ED25519_E_INCONSISTENT, ED25519_SIGN_OK, ED25519_SIGN_SIGNER, Ed25519PrivateKey, sign_ed25519,
)
