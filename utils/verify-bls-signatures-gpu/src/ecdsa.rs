//! include/cess_ecdsa.h: batch ECDSA P-256 verification on the GPU under the
//! rules of ring's `ECDSA_P256_SHA256_FIXED`, `ECDSA_P256_SHA256_ASN1` and
//! `ECDSA_P256_SHA384_ASN1`.  The declarations are in ffi.rs; the safe wrapper
//! is a set of methods on `Verifier`.  No node host function is wired to it.
//!
//! NOT COMPILED in this repository's image, like the rest of the crate; the
//! declarations are checked against the header by tests/test_ecdsa.py.

use core::ffi::c_int;

use crate::ffi::{cess_ecdsa_keys_load, cess_ecdsa_verify, cess_ecdsa_verify_batch};
use crate::{check, Error, Verifier};

/// The three algorithms (`CESS_ECDSA_ALG_*`).
#[derive(Clone, Copy, Debug, Eq, PartialEq)]
#[repr(i32)]
pub enum EcdsaAlg {
    P256Sha256Fixed = 0,
    P256Sha256Asn1 = 1,
    P256Sha384Asn1 = 2,
}

fn offsets(items: &[&[u8]]) -> (Vec<u8>, Vec<u64>) {
    let mut data = Vec::new();
    let mut offs = Vec::with_capacity(items.len() + 1);
    offs.push(0u64);
    for it in items {
        data.extend_from_slice(it);
        offs.push(data.len() as u64);
    }
    (data, offs)
}

impl Verifier {
    /// Replace the context's ECDSA key table; `true` per key that loaded.
    pub fn ecdsa_keys_load(&mut self, keys: &[&[u8]]) -> Result<Vec<bool>, Error> {
        let (data, offs) = offsets(keys);
        let mut st: Vec<c_int> = vec![0; keys.len().max(1)];
        check(unsafe { cess_ecdsa_keys_load(self.ctx, keys.len(), data.as_ptr(), offs.as_ptr(), st.as_mut_ptr()) })?;
        Ok(st[..keys.len()].iter().map(|s| *s == 0).collect())
    }

    /// The codes (`CESS_ECDSA_*`) of records (key `key_idx[i]`, message i, signature i).
    pub fn ecdsa_verify_batch(&mut self, alg: EcdsaAlg, key_idx: &[u32], msgs: &[&[u8]], sigs: &[&[u8]])
                              -> Result<Vec<u8>, Error> {
        let n = key_idx.len();
        if msgs.len() != n || sigs.len() != n {
            return Err(Error::InvalidArg);
        }
        let (s, so) = offsets(sigs);
        let (m, mo) = offsets(msgs);
        let mut codes = vec![0u8; n.max(1)];
        check(unsafe {
            cess_ecdsa_verify_batch(self.ctx, alg as c_int, n, key_idx.as_ptr(), s.as_ptr(), so.as_ptr(), m.as_ptr(),
                                    mo.as_ptr(), codes.as_mut_ptr(), core::ptr::null_mut())
        })?;
        codes.truncate(n);
        Ok(codes)
    }

    /// ring's `ECDSA_P256_*.verify(key, msg, sig)`: `Ok(false)` for every failure of the record;
    /// `Err(Error::BadKey)`-class status where the key does not load.
    pub fn ecdsa_verify(&mut self, alg: EcdsaAlg, key: &[u8], msg: &[u8], sig: &[u8]) -> Result<bool, Error> {
        let mut ok: c_int = 0;
        check(unsafe {
            cess_ecdsa_verify(self.ctx, alg as c_int, key.as_ptr(), key.len(), msg.as_ptr(), msg.len(), sig.as_ptr(),
                              sig.len(), &mut ok)
        })?;
        Ok(ok == 1)
    }
}
