// RSASSA-PSS: k_rsa_verify_big in store mode -- the loop-form kernel's source
// itself, with m written out for k_rsa_pss instead of compared
// (k_rsa_big.hip, CESS_RSA_BIG_STORE).
#define CESS_RSA_BIG_STORE 1
#include "k_rsa_big.hip"
