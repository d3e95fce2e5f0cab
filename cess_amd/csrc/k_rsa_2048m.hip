// RSASSA-PSS: k_rsa_verify_2048 in store mode -- the same exponentiation,
// with m = s^e mod n written out for k_rsa_pss instead of compared (k_rsa.hpp
// STORE).  A translation unit of its own, like every expanded product scan.
#include "k_rsa.hpp"

CESS_RSA_KERNEL_M(k_rsa_verify_2048m, RSA_L2048, 2, false)
