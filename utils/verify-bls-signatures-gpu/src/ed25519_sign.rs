//! include/cess_ed25519_sign.h: batch Ed25519 key derivation and signing on
//! the GPU under the rules of ring's `Ed25519KeyPair` (from_seed_unchecked,
//! from_seed_and_public_key, sign).  The declarations live here, not in ffi.rs,
//! whose `cess_ed25519_*` set mirrors include/cess_ed25519.h alone; the safe
//! wrapper is a set of methods on `Verifier`.
//!
//! NOT COMPILED in this repository's image, like the rest of the crate; the
//! declarations are checked against the header by tests/test_ed25519_sign.py.
//!
//! The signer is not hardened against timing or cache observation by another
//! tenant of the device; the library zeroes the device buffers that held
//! secrets, the caller's host memory is the caller's.

use core::ffi::{c_char, c_int, c_void};

use crate::ffi::cess_bls_ctx;
use crate::{check, Error, Verifier};

pub const CESS_ED25519_E_INCONSISTENT: c_int = -12;
pub const CESS_ED25519_SIGN_OK: u8 = 0;
pub const CESS_ED25519_SIGN_SIGNER: u8 = 1;

extern "C" {
    pub fn cess_ed25519_signers_load(ctx: *mut cess_bls_ctx, k: usize, seeds: *const u8, seed_offsets: *const u64,
                                     expected_pubs: *const u8, pubs_out: *mut u8, status_out: *mut c_int) -> c_int;
    pub fn cess_ed25519_sign_batch(ctx: *mut cess_bls_ctx, n: usize, signer_idx: *const u32, msgs: *const u8,
                                   msg_offsets: *const u64, sigs_out: *mut u8, codes_out: *mut u8) -> c_int;
    pub fn cess_ed25519_sign_batch_device(ctx: *mut cess_bls_ctx, n: usize, d_signer_idx: *const u32,
                                          d_msgs: *const u8, d_msg_offsets: *const u64, d_sigs_out: *mut u8,
                                          d_codes: *mut u8, stream: *mut c_void) -> c_int;
    pub fn cess_ed25519_sign(ctx: *mut cess_bls_ctx, seed: *const u8, seed_len: usize, msg: *const u8,
                             msg_len: usize, sig_out64: *mut u8, pub_out32: *mut u8) -> c_int;
    pub fn cess_ed25519_sign_stage_stats(ctx: *mut cess_bls_ctx, names: *mut *const c_char, ms: *mut f64,
                                         launches: *mut u64, max: c_int, reset: c_int) -> c_int;
}

/// Why a signer of the table did not load.
#[derive(Clone, Copy, Debug, Eq, PartialEq)]
pub enum SignerStatus {
    Loaded,
    /// the seed is not 32 bytes (ring: invalid_encoding)
    BadSeed,
    /// the expected public key differs from the derived one (ring: inconsistent_components)
    Inconsistent,
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
    /// Replace the context's signer table; returns each signer's public key
    /// (zeros for a bad seed) and status.
    pub fn ed25519_signers_load(&mut self, seeds: &[&[u8]], expected_pubs: Option<&[[u8; 32]]>)
                                -> Result<Vec<([u8; 32], SignerStatus)>, Error> {
        let k = seeds.len();
        if let Some(e) = expected_pubs {
            if e.len() != k {
                return Err(Error::InvalidArg);
            }
        }
        let (data, offs) = offsets(seeds);
        let exp: Vec<u8> = expected_pubs.map(|e| e.iter().flatten().copied().collect()).unwrap_or_default();
        let mut pubs = vec![0u8; 32 * k.max(1)];
        let mut st = vec![0 as c_int; k.max(1)];
        check(unsafe {
            cess_ed25519_signers_load(self.ctx, k, data.as_ptr(), offs.as_ptr(),
                                      if expected_pubs.is_some() { exp.as_ptr() } else { core::ptr::null() },
                                      pubs.as_mut_ptr(), st.as_mut_ptr())
        })?;
        Ok((0..k).map(|j| {
            let mut p = [0u8; 32];
            p.copy_from_slice(&pubs[32 * j..32 * j + 32]);
            let s = match st[j] {
                0 => SignerStatus::Loaded,
                CESS_ED25519_E_INCONSISTENT => SignerStatus::Inconsistent,
                _ => SignerStatus::BadSeed,
            };
            (p, s)
        }).collect())
    }

    /// Sign message i with signer `signer_idx[i]`; `None` where the signer is
    /// missing or did not load.
    pub fn ed25519_sign_batch(&mut self, signer_idx: &[u32], msgs: &[&[u8]]) -> Result<Vec<Option<[u8; 64]>>, Error> {
        let n = signer_idx.len();
        if msgs.len() != n {
            return Err(Error::InvalidArg);
        }
        let (data, offs) = offsets(msgs);
        let mut sigs = vec![0u8; 64 * n.max(1)];
        let mut codes = vec![0u8; n.max(1)];
        check(unsafe {
            cess_ed25519_sign_batch(self.ctx, n, signer_idx.as_ptr(), data.as_ptr(), offs.as_ptr(),
                                    sigs.as_mut_ptr(), codes.as_mut_ptr())
        })?;
        Ok((0..n).map(|i| {
            if codes[i] != CESS_ED25519_SIGN_OK {
                return None;
            }
            let mut s = [0u8; 64];
            s.copy_from_slice(&sigs[64 * i..64 * i + 64]);
            Some(s)
        }).collect())
    }

    /// ring's `Ed25519KeyPair::from_seed_unchecked(seed)?.sign(msg)` and the public key.
    pub fn sign_ed25519(&mut self, seed: &[u8], msg: &[u8]) -> Result<([u8; 64], [u8; 32]), Error> {
        let mut sig = [0u8; 64];
        let mut key = [0u8; 32];
        check(unsafe {
            cess_ed25519_sign(self.ctx, seed.as_ptr(), seed.len(), msg.as_ptr(), msg.len(), sig.as_mut_ptr(),
                              key.as_mut_ptr())
        })?;
        Ok((sig, key))
    }
}
