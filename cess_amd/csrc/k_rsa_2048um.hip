// RSASSA-PSS: k_rsa_verify_2048u (key-uniform waves) in store mode -- m written
// out for k_rsa_pss instead of compared (k_rsa.hpp STORE).
#include "k_rsa.hpp"

CESS_RSA_KERNEL_M(k_rsa_verify_2048um, RSA_L2048, 2, true)
